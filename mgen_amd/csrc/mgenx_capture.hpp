// mgenx_capture.hpp -- what the passes over a resident capture share (mgenx_defrag.hip,
// mgenx_pcap_tcp.hip): bytewise loads, the key hash, a packet's data by either file format, and
// the aligned load of source bytes of any alignment.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "mgenx.h"

namespace mgenx {
namespace capture {

__device__ __forceinline__ uint32_t ld8(const uint8_t* b, uint64_t i) { return b[i]; }
__device__ __forceinline__ uint32_t be16(const uint8_t* b, uint64_t i) {
  return (uint32_t)b[i] << 8 | b[i + 1];
}
__device__ __forceinline__ uint32_t ld32(const uint8_t* b, uint64_t i, bool swapped) {
  const uint32_t v = (uint32_t)b[i] | (uint32_t)b[i + 1] << 8 | (uint32_t)b[i + 2] << 16 |
                     (uint32_t)b[i + 3] << 24;
  return swapped ? __builtin_bswap32(v) : v;
}
__device__ __forceinline__ uint64_t ld_bytes64(const uint8_t* b, uint64_t i, uint32_t nb) {
  uint64_t v = 0;
  for (uint32_t k = 0; k < nb; k++) v |= (uint64_t)b[i + k] << (8 * k);
  return v;
}
__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64's finalizer
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// One packet's data: offset, captured and original length.  P has buf, limit (packets lie in
// buf[0, limit) = below the scratch window), pkt_off, data_off (pcapng: the packets' data; null
// = classic records), cap_len and flags.  Every read is bounded by p.limit first, by
// subtraction.
template <typename P>
__device__ __forceinline__ bool packet_data(const P& p, uint32_t i, uint64_t& d,
                                            uint32_t& caplen, uint32_t& wirelen) {
  const bool sw = (p.flags & MGENX_PCAP_SWAPPED) != 0;
  const uint64_t ro = p.pkt_off[i];
  if (ro > p.limit) return false;
  const uint64_t room = p.limit - ro;
  if (!p.data_off) {
    if (room < 16) return false;
    caplen = ld32(p.buf, ro + 8, sw);
    wirelen = ld32(p.buf, ro + 12, sw);
    if (room - 16 < caplen) return false;
    d = ro + 16;
    return true;
  }
  if (room < 12) return false;
  const uint32_t type = ld32(p.buf, ro, sw);
  if (type == 6u || type == 2u) {
    if (room < 28) return false;
    wirelen = ld32(p.buf, ro + 24, sw);
  } else if (type == 3u) {
    wirelen = ld32(p.buf, ro + 8, sw);
  } else {
    return false;
  }
  d = p.data_off[i];
  caplen = p.cap_len[i];
  return d <= p.limit && p.limit - d >= caplen;
}

// nb (1..8) source bytes at buf + s, little-endian in one word.  A whole word comes from the
// one or two aligned words that hold it when both lie inside the allocation; the source has
// any alignment (as pcap_snap_copy_kernel's), the loads never do.
__device__ __forceinline__ uint64_t ld_word(const uint8_t* buf, uint64_t buf_bytes, uint64_t s,
                                            uint32_t nb) {
  const uint32_t sh = (uint32_t)((uintptr_t)(buf + s) & 7u);
  if (nb == 8 && s >= sh && s - sh + 16 <= buf_bytes) {
    const uint64_t* a = (const uint64_t*)(buf + (s - sh));
    const uint64_t lo = a[0];
    if (!sh) return lo;
    return lo >> (8 * sh) | a[1] << (64 - 8 * sh);
  }
  return ld_bytes64(buf, s, nb);
}

}  // namespace capture
}  // namespace mgenx
