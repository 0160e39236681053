// mgenx_defrag.hip -- reassembly of fragmented IPv4 / IPv6 datagrams for pcap2mgen
// (mgenx_pcap_defrag / mgenx_pcapng_defrag; the contract is in include/mgenx.h, the design in
// DESIGN.md 4.10).  The reference does not reassemble: this runs only when asked for.
//
// Over the whole capture in HBM, after the parse and the snap step:
//   defrag_classify_kernel  one lane per packet: the link / IP header walk of the parse up to
//                           its protocol test, the fragment rules, the key and its 64-bit hash;
//   hipcub radix sort       (hash, packet) pairs, stable: a run of equal hash holds one key's
//                           fragments in capture order (two keys of one hash are told apart by
//                           comparing the full key, below);
//   defrag_sm_kernel        one lane per run: the per-key state machine, walked serially; marks
//                           the completing packets, their length L, UDP length and source port,
//                           and each held fragment's completing packet;
//   hipcub exclusive sum    round16(L) over completing packets, in packet order -> the slots;
//   [one read-back: the counters and the total; too small a window ends the call here]
//   defrag_gather_kernel    one wave per packet: a fragment's payload to slot + off (aligned
//                           8-byte stores, sources of any alignment), the pad zeroed, and the
//                           packet's row (status, udp_off, udp_len, src.port) rewritten.
// No kernel waits on another workgroup.  Nothing but the workspace is written before the size
// check, so a call that does not fit changes no output.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <hipcub/hipcub.hpp>

#include "mgenx_capture.hpp"
#include "mgenx_internal.hpp"

namespace mgenx {
namespace defrag {

using namespace capture;

constexpr uint64_t kNoFrag = ~0ull;        // sort key of a packet that is no valid fragment
constexpr uint32_t kNone = 0xFFFFFFFFu;    // owner: the fragment's context did not complete
constexpr uint32_t kMaxFrame = 4094;       // the parse's frame rule
// cls: what the classification found
constexpr uint8_t kNotFrag = 0, kFrag = 1, kToBadIp = 2, kToTruncated = 3;
// meta: len [0,16) | v6 bit 16 | MF bit 17 | off / 8 [18,31) | id [32,64)
constexpr uint64_t kKeyBits = 0xFFFFFFFF00010000ull;  // id and version: the key's part of meta
// counters after the scan's n + 1 sizes
constexpr int kCntFrag = 1, kCntDgram = 2, kCntNotUdp = 3, kCntIncomplete = 4, kCntN = 5;

struct Params {
  uint8_t* buf;
  uint64_t limit;      // packets lie in buf[0, limit) = below the scratch window
  uint64_t buf_bytes;  // the allocation: what an aligned 8-byte load may touch
  uint64_t scratch_off;
  const uint64_t* pkt_off;
  const uint64_t* data_off;  // pcapng: the packets' data; null = classic records
  const uint32_t* cap_len;
  uint32_t n;
  uint32_t link_type;
  uint32_t flags;
  int64_t timeout_us;
  const uint32_t* rx_sec;
  const uint32_t* rx_usec;
  uint8_t* status;
  uint64_t* udp_off;
  uint32_t* udp_len;
  mgenx_addr* src;
  // workspace
  uint64_t* hash_in;
  uint64_t* hash_out;
  uint32_t* idx_in;
  uint32_t* idx_out;
  uint64_t* kw;     // 4 words per packet: the key's addresses
  uint64_t* meta;
  uint64_t* psrc;   // the payload's offset in buf
  uint8_t* cls;
  uint8_t* done;    // per sorted position: walked (a run of two keys takes two passes)
  uint32_t* owner;  // the packet that completed this fragment's datagram
  uint32_t* vd;     // completing packet: source port << 16 | UDP length (0 = not UDP)
  uint64_t* need;   // n + 1 slot sizes -> offsets, then the kCntN - 1 counters
};

// The parse's walk (mgenx_pcap.hip frame_walk) up to its protocol test, then the fragment
// rules.  kNotFrag: the packet keeps what the parse gave it.
__device__ __forceinline__ uint8_t classify(const uint8_t* d, uint32_t caplen, uint32_t wirelen,
                                            uint32_t link_type, uint64_t& meta, uint32_t& pay,
                                            uint64_t kw[4]) {
  const uint32_t num = caplen < kMaxFrame ? caplen : kMaxFrame;
  uint32_t eth_type, ip0, ip_len;
  if (link_type == MGENX_DLT_LINUX_SLL) {
    if (num < 16) return kNotFrag;
    eth_type = be16(d, 14);
    ip0 = 16;
    ip_len = num - 16;
  } else {
    if (wirelen > kMaxFrame || wirelen < 14 || num < 14) return kNotFrag;
    eth_type = be16(d, 12);
    uint32_t hl = 14;
    if (eth_type == 0x8100u) {
      if (wirelen < 18 || num < 18) return kNotFrag;
      eth_type = be16(d, 16);
      hl = 18;
    }
    ip0 = hl;
    ip_len = wirelen - hl;
  }
  if (eth_type != 0x0800u && eth_type != 0x86DDu) return kNotFrag;
  if (ip_len < 1 || ip0 >= num) return kNotFrag;
  const uint32_t ver = ld8(d, ip0) >> 4;
  uint32_t off, len, mf, id, end;
  if (ver == 4) {
    if (ip_len < 20 || ip0 + 20 > num) return kNotFrag;
    const uint32_t ihl = (ld8(d, ip0) & 15u) * 4u;
    const uint32_t tot = be16(d, ip0 + 2);
    if (ihl < 20 || tot < ihl || tot > ip_len) return kNotFrag;
    const uint32_t f = be16(d, ip0 + 6);
    mf = (f >> 13) & 1u;
    off = (f & 0x1FFFu) * 8u;
    if (!mf && !off) return kNotFrag;
    if (ld8(d, ip0 + 9) != 17u) return kNotFrag;
    id = be16(d, ip0 + 4);
    pay = ip0 + ihl;
    len = tot - ihl;
    end = ip0 + tot;
    kw[0] = ld_bytes64(d, ip0 + 12, 8);  // source, destination
    kw[1] = kw[2] = kw[3] = 0;
  } else if (ver == 6) {
    if (ip_len < 40 || ip0 + 40 > num) return kNotFrag;
    const uint32_t pl = be16(d, ip0 + 4);
    if (40u + pl > ip_len) return kNotFrag;
    if (ld8(d, ip0 + 6) != 44u) return kNotFrag;
    if (pl < 8) return kToBadIp;
    if (ip0 + 48 > num) return kToTruncated;
    if (ld8(d, ip0 + 40) != 17u) return kNotFrag;
    const uint32_t f = be16(d, ip0 + 42);
    mf = f & 1u;
    off = f & 0xFFF8u;
    id = be16(d, ip0 + 44) << 16 | be16(d, ip0 + 46);
    pay = ip0 + 48;
    len = pl - 8;
    end = ip0 + 40 + pl;
#pragma unroll
    for (int k = 0; k < 4; k++) kw[k] = ld_bytes64(d, ip0 + 8 + 8 * k, 8);
  } else {
    return kNotFrag;
  }
  if (len == 0 || (mf && (len & 7u)) || off + len > 65535u) return kToBadIp;
  if (end > num) return kToTruncated;
  meta = (uint64_t)id << 32 | (uint64_t)(off >> 3) << 18 | (uint64_t)mf << 17 |
         (uint64_t)(ver == 6) << 16 | len;
  return kFrag;
}

__global__ void __launch_bounds__(256) defrag_classify_kernel(Params p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint8_t c = kNotFrag;
  uint64_t h = kNoFrag;
  if (i < p.n) {
    const uint8_t st = p.status[i];
    uint64_t d = 0, meta = 0, kw[4] = {0, 0, 0, 0};
    uint32_t caplen = 0, wirelen = 0, pay = 0;
    if (st != MGENX_PCAP_BAD_ETH && st != MGENX_PCAP_NOT_IP && st != MGENX_PCAP_BAD_IP &&
        st != MGENX_PCAP_OOB && packet_data(p, i, d, caplen, wirelen))
      c = classify(p.buf + d, caplen, wirelen, p.link_type, meta, pay, kw);
    if (c == kFrag) {
      // IPv4 keeps source and destination apart; the IPv6 words are folded, so the two
      // directions of one address pair share a hash (the full-key compare separates them)
      h = mix64(kw[0] ^ kw[1] ^ kw[2] ^ kw[3] ^ mix64(meta & kKeyBits));
      if (h == kNoFrag) h--;
#pragma unroll
      for (int k = 0; k < 4; k++) p.kw[(uint64_t)i * 4 + k] = kw[k];
      p.meta[i] = meta;
      p.psrc[i] = d + pay;
    }
    p.cls[i] = c;
    p.done[i] = 0;
    p.owner[i] = kNone;
    p.vd[i] = 0;
    p.need[i] = 0;
    p.hash_in[i] = h;
    p.idx_in[i] = i;
  }
  const uint64_t m = __ballot(c == kFrag);
  if ((threadIdx.x & 63u) == 0 && m)
    atomicAdd((unsigned long long*)&p.need[p.n + kCntFrag], (unsigned long long)__popcll(m));
}

__device__ __forceinline__ bool key_eq(const Params& p, uint32_t i, uint64_t kbits,
                                       const uint64_t k[4]) {
  if ((p.meta[i] & kKeyBits) != kbits) return false;
  const uint64_t* w = p.kw + (uint64_t)i * 4;
  return w[0] == k[0] && w[1] == k[1] && w[2] == k[2] && w[3] == k[3];
}

// One lane per run of equal hash.  A run is one datagram's fragments, or a few datagrams' when
// an id wraps inside the capture; a capture that is one huge run is walked by one lane
// (correct, slow).  Two keys of one hash: the run is walked once per key, `done` marks what
// an earlier pass took.
__global__ void __launch_bounds__(64) defrag_sm_kernel(Params p) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.n) return;
  const uint64_t h = p.hash_out[q];
  if (h == kNoFrag || (q && p.hash_out[q - 1] == h)) return;
  uint32_t run_end = q + 1;
  while (run_end < p.n && p.hash_out[run_end] == h) run_end++;
  uint32_t held[MGENX_DEFRAG_MAX_FRAGS];  // off | end << 16 of the open context's fragments
  uint32_t n_dgram = 0, n_not_udp = 0, n_incomplete = 0;
  for (uint32_t first = q; first < run_end;) {
    const uint32_t i0 = p.idx_out[first];
    const uint64_t kbits = p.meta[i0] & kKeyBits;
    uint64_t k[4];
#pragma unroll
    for (int w = 0; w < 4; w++) k[w] = p.kw[(uint64_t)i0 * 4 + w];
    bool open = false, has_l = false;
    int64_t t0 = 0;
    uint32_t sum = 0, L = 0, cnt = 0, max_end = 0, cstart = first, next_first = run_end;
    for (uint32_t j = first; j < run_end; j++) {
      if (p.done[j]) continue;
      const uint32_t i = p.idx_out[j];
      if (!key_eq(p, i, kbits, k)) {
        if (next_first == run_end) next_first = j;
        continue;
      }
      p.done[j] = 1;
      const uint64_t m = p.meta[i];
      const uint32_t len = (uint32_t)m & 0xFFFFu, off = ((uint32_t)(m >> 18) & 0x1FFFu) * 8u;
      const bool mf = (m >> 17) & 1u;
      const uint32_t e = off + len;
      const int64_t t = (int64_t)p.rx_sec[i] * 1000000 + (int64_t)p.rx_usec[i];
      if (open && p.timeout_us > 0 && t - t0 > p.timeout_us) {
        open = false;
        n_incomplete++;
      }
      if (open) {
        bool c = cnt >= MGENX_DEFRAG_MAX_FRAGS || (has_l && (e > L || !mf)) || (!mf && e < max_end);
        for (uint32_t x = 0; x < cnt && !c; x++)
          c = off < (held[x] >> 16) && (held[x] & 0xFFFFu) < e;
        if (c) {
          open = false;
          n_incomplete++;
        }
      }
      if (!open) {
        open = true; has_l = false;
        t0 = t; sum = 0; cnt = 0; max_end = 0; cstart = j;
      }
      held[cnt++] = off | e << 16;
      sum += len;
      if (!mf) { has_l = true; L = e; }
      if (e > max_end) max_end = e;
      if (has_l && sum == L) {
        // complete at packet i: every fragment of this key since cstart is held
        uint32_t port = 0, ul = 0;
        for (uint32_t x = cstart; x <= j; x++) {
          const uint32_t ix = p.idx_out[x];
          if (!key_eq(p, ix, kbits, k)) continue;
          p.owner[ix] = i;
          if (((p.meta[ix] >> 18) & 0x1FFFu) == 0 && L >= 8) {  // holds the UDP header
            port = be16(p.buf, p.psrc[ix]);
            ul = be16(p.buf, p.psrc[ix] + 4);
          }
        }
        if (ul < 8 || ul > L) {
          ul = 0;
          n_not_udp++;
        }
        p.vd[i] = ul ? port << 16 | ul : 0u;
        p.need[i] = ((uint64_t)L + 15) & ~15ull;
        n_dgram++;
        open = false;
      }
    }
    if (open) n_incomplete++;
    first = next_first;
  }
  unsigned long long* cn = (unsigned long long*)(p.need + p.n);
  if (n_dgram) atomicAdd(cn + kCntDgram, (unsigned long long)n_dgram);
  if (n_not_udp) atomicAdd(cn + kCntNotUdp, (unsigned long long)n_not_udp);
  if (n_incomplete) atomicAdd(cn + kCntIncomplete, (unsigned long long)n_incomplete);
}

// One wave per packet (grid-stride).  A fragment of a completed datagram copies its payload to
// slot + off: off is a multiple of 8 and the slot 16-byte aligned, so every store is an aligned
// 8-byte word; the last fragment (MF 0) also writes the zeros up to round16(L).  Fragments of
// one datagram are disjoint and all but the last a multiple of 8 long, so no word is written
// twice.  Lane 0 then rewrites the packet's row.
__global__ void __launch_bounds__(256) defrag_gather_kernel(Params p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t i = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); i < p.n; i += waves) {
    const uint8_t c = p.cls[i];
    if (c == kNotFrag) continue;
    uint32_t st = c == kToBadIp ? MGENX_PCAP_BAD_IP : MGENX_PCAP_TRUNCATED;
    uint32_t ulen = 0, port = 0;
    uint64_t uoff = 0;
    bool repoint = false;
    if (c == kFrag) {
      st = MGENX_PCAP_FRAGMENT;
      const uint32_t ow = p.owner[i];
      if (ow != kNone) {
        const uint64_t m = p.meta[i];
        const uint32_t len = (uint32_t)m & 0xFFFFu, off = ((uint32_t)(m >> 18) & 0x1FFFu) * 8u;
        const uint64_t slot = p.scratch_off + p.need[ow];
        const uint64_t s = p.psrc[i];
        // words to write: the payload, and for the last fragment the pad up to round16(L)
        const uint32_t stop = (m >> 17) & 1u ? len : ((off + len + 15u) & ~15u) - off;
        uint64_t* dst = (uint64_t*)(p.buf + slot + off);
        for (uint32_t w = lane; w * 8 < stop; w += 64) {
          const uint32_t at = w * 8;
          const uint32_t nb = at >= len ? 0u : (len - at < 8u ? len - at : 8u);
          dst[w] = nb ? ld_word(p.buf, p.buf_bytes, s + at, nb) : 0ull;
        }
        if (ow == i) {  // the completing packet
          const uint32_t v = p.vd[i];
          if (v) {
            st = MGENX_PCAP_UDP;
            ulen = (v & 0xFFFFu) - 8u;
            port = v >> 16;
            uoff = slot + 8;
            repoint = true;
          } else {
            st = MGENX_PCAP_NOT_UDP;
          }
        }
      }
    }
    if (lane == 0) {
      p.status[i] = (uint8_t)st;
      p.udp_len[i] = ulen;
      p.src[i].port = (uint16_t)port;
      if (repoint) p.udp_off[i] = uoff;
    }
  }
}

static size_t cub_bytes(uint32_t n) {
  size_t a = 0, b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const uint64_t*)nullptr,
                                           (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (int)n, 0, 64, (hipStream_t)0);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (int)n + 1, (hipStream_t)0);
  return a > b ? a : b;
}

}  // namespace defrag
}  // namespace mgenx

using namespace mgenx::defrag;
using mgenx::a256;
using mgenx::Carve;

static size_t defrag_ws(uint32_t n) {
  const size_t N = n;
  return 4 * a256(N * 8) + a256(N * 32) + 4 * a256(N * 4) + 2 * a256(N) +
         a256((N + kCntN) * 8) + a256(cub_bytes(n));
}

// dev_data_off null: classic records at dev_pkt_off; else pcapng, dev_pkt_off = the packet
// blocks and dev_data_off / dev_cap_len what mgenx_pcapng_parse wrote.  `mem` holds
// defrag_ws(n) bytes.  Synchronizes the stream once (the sizes' read-back).
static int defrag_run(void* mem, uint8_t* dev_buf, uint64_t scratch_off, uint64_t buf_bytes,
                      const uint64_t* dev_pkt_off, const uint64_t* dev_data_off,
                      const uint32_t* dev_cap_len, uint32_t n, uint32_t link_type, uint32_t flags,
                      int64_t timeout_us, const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                      uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                      mgenx_addr* dev_src, mgenx_defrag_stats* stats, hipStream_t stream, char* err,
                      size_t errn) {
  Params p;
  p.buf = dev_buf; p.limit = scratch_off; p.buf_bytes = buf_bytes; p.scratch_off = scratch_off;
  p.pkt_off = dev_pkt_off; p.data_off = dev_data_off; p.cap_len = dev_cap_len; p.n = n;
  p.link_type = link_type; p.flags = flags; p.timeout_us = timeout_us;
  p.rx_sec = dev_rx_sec; p.rx_usec = dev_rx_usec; p.status = dev_status;
  p.udp_off = dev_udp_off; p.udp_len = dev_udp_len; p.src = dev_src;
  const size_t N = n;
  Carve take(mem);
  p.hash_in = (uint64_t*)take(N * 8);
  p.hash_out = (uint64_t*)take(N * 8);
  p.meta = (uint64_t*)take(N * 8);
  p.psrc = (uint64_t*)take(N * 8);
  p.kw = (uint64_t*)take(N * 32);
  p.idx_in = (uint32_t*)take(N * 4);
  p.idx_out = (uint32_t*)take(N * 4);
  p.owner = (uint32_t*)take(N * 4);
  p.vd = (uint32_t*)take(N * 4);
  p.cls = (uint8_t*)take(N);
  p.done = (uint8_t*)take(N);
  p.need = (uint64_t*)take((N + kCntN) * 8);
  size_t tmp_bytes = cub_bytes(n);
  void* tmp = take(tmp_bytes);
  auto fail = [&](hipError_t e, const char* where) {
    snprintf(err, errn, "%s: %s", where, hipGetErrorString(e));
    return MGENX_EDEVICE;
  };
  const uint32_t blocks = (n + 255) / 256;
  // the scan's last input and the counters
  hipError_t e = hipMemsetAsync(p.need + n, 0, kCntN * 8, stream);
  if (e != hipSuccess) return fail(e, "pcap_defrag clear");
  hipLaunchKernelGGL(defrag_classify_kernel, dim3(blocks), dim3(256), 0, stream, p);
  size_t have = tmp_bytes;
  e = hipcub::DeviceRadixSort::SortPairs(tmp, have, p.hash_in, p.hash_out, p.idx_in,
                                                    p.idx_out, (int)n, 0, 64, stream);
  if (e != hipSuccess) return fail(e, "pcap_defrag sort");
  hipLaunchKernelGGL(defrag_sm_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, p);
  have = tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(tmp, have, p.need, p.need, (int)n + 1, stream);
  if (e != hipSuccess) return fail(e, "pcap_defrag scan");
  uint64_t h[kCntN];
  e = hipMemcpyAsync(h, p.need + n, sizeof(h), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(e, "pcap_defrag sizes");
  stats->scratch_bytes = h[0];
  stats->n_fragments = h[kCntFrag];
  stats->n_datagrams = h[kCntDgram];
  stats->n_not_udp = h[kCntNotUdp];
  stats->n_incomplete = h[kCntIncomplete];
  if (buf_bytes - scratch_off < h[0]) return MGENX_ENOSPC;
  if (h[0] && ((uintptr_t)(dev_buf + scratch_off) & 15u)) {
    snprintf(err, errn, "pcap_defrag: the scratch window is not 16-byte aligned");
    return MGENX_EINVAL;
  }
  const uint32_t gblocks = n < 2048u * 4u ? (n + 3) / 4 : 2048u;
  hipLaunchKernelGGL(defrag_gather_kernel, dim3(gblocks), dim3(256), 0, stream, p);
  e = hipGetLastError();
  return e == hipSuccess ? MGENX_OK : fail(e, "pcap_defrag");
}

// ---- the C ABI of the defrag step ----
using mgenx::set_err;

extern "C" {

// both defrags: dev_data_off null = classic records at dev_pkt_off, else pcapng packet blocks
static int pcap_defrag_any(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off,
                           uint64_t buf_bytes, const uint64_t* dev_pkt_off,
                           const uint64_t* dev_data_off, const uint32_t* dev_cap_len, uint32_t n,
                           uint32_t link_type, uint32_t flags, int64_t timeout_us,
                           const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                           uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                           mgenx_addr* dev_src, mgenx_defrag_stats* stats, void* stream) {
  if (!ctx || !stats || buf_bytes < scratch_off || n > 0x7FFFFFFEu) return MGENX_EINVAL;
  memset(stats, 0, sizeof(*stats));
  if (n == 0) return MGENX_OK;
  if (!dev_buf || !dev_pkt_off || !dev_rx_sec || !dev_rx_usec || !dev_status || !dev_udp_off ||
      !dev_udp_len || !dev_src)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  void* m = ctx->defrag.get(defrag_ws(n));
  if (!m) return set_err(ctx, hipErrorOutOfMemory, "pcap_defrag workspace");
  return defrag_run(m, dev_buf, scratch_off, buf_bytes, dev_pkt_off, dev_data_off,
                          dev_cap_len, n, link_type, flags, timeout_us, dev_rx_sec, dev_rx_usec,
                          dev_status, dev_udp_off, dev_udp_len, dev_src, stats,
                          (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_pcap_defrag(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off, uint64_t buf_bytes,
                      const uint64_t* dev_pkt_off, uint32_t n, uint32_t link_type, uint32_t flags,
                      int64_t timeout_us, const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                      uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                      mgenx_addr* dev_src, mgenx_defrag_stats* stats, void* stream) {
  return pcap_defrag_any(ctx, dev_buf, scratch_off, buf_bytes, dev_pkt_off, nullptr, nullptr, n,
                         link_type, flags, timeout_us, dev_rx_sec, dev_rx_usec, dev_status,
                         dev_udp_off, dev_udp_len, dev_src, stats, stream);
}

int mgenx_pcapng_defrag(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off,
                        uint64_t buf_bytes, const uint64_t* dev_pkt_off,
                        const uint64_t* dev_data_off, const uint32_t* dev_cap_len, uint32_t n,
                        uint32_t link_type, uint32_t flags, int64_t timeout_us,
                        const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                        uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                        mgenx_addr* dev_src, mgenx_defrag_stats* stats, void* stream) {
  if (n && (!dev_data_off || !dev_cap_len)) return MGENX_EINVAL;
  return pcap_defrag_any(ctx, dev_buf, scratch_off, buf_bytes, dev_pkt_off, dev_data_off,
                         dev_cap_len, n, link_type, flags, timeout_us, dev_rx_sec, dev_rx_usec,
                         dev_status, dev_udp_off, dev_udp_len, dev_src, stats, stream);
}

}  // extern "C"
