// mgenx_pcapng.hpp -- the pcapng block walk (host, plain C++: no HIP, no allocation).
//
// The reference opens its capture with pcap_fopen_offline (src/common/pcap2mgen.cpp:323) and
// libpcap reads pcapng there as it reads classic pcap.  libpcap is not part of the reference
// tree, so this walk is a restatement of its pcapng reader (parity unpinned at this layer, like
// the protolib packet classes); the rules below are the contract:
//
//   block      = u32 type, u32 total_len, body, u32 total_len   (section byte order;
//                total_len a multiple of 4, >= 12; the next block total_len bytes later)
//   options    = u16 code, u16 len, value padded to 4; code 0 ends the list
//   SHB  0x0A0D0D0A  u32 magic 0x1A2B3C4D, u16 major, u16 minor, i64 section_len     (>= 28)
//   IDB  1           u16 linktype, u16 rsv, u32 snaplen, options 9 if_tsresol,
//                    14 if_tsoffset                                                  (>= 20)
//   EPB  6           u32 iface, ts_hi, ts_lo, caplen, origlen, data                  (>= 32)
//   OPB  2           u16 iface, u16 drops, then as the EPB from ts_hi                (>= 32)
//   SPB  3           u32 origlen, data                                               (>= 16)
//   anything else is skipped.
//
// Every read is checked against nbytes before it happens; a block is looked into only once
// the whole of it is known to lie inside the buffer.  Each block is judged in this order:
// 8 head bytes present (else _TRUNCATED), total_len legal for its type (else _BLOCK), the
// whole block present (else _TRUNCATED), trailing length (else _BLOCK), then its content.
// A stop keeps the packets found so far and leaves info->consumed at the stopping block.
// Options are read where they are used, in the IDB.
#pragma once

#include <stdint.h>
#include <string.h>

#include "mgenx.h"

namespace mgenx {
namespace ng {

constexpr uint32_t kShb = 0x0A0D0D0Au, kIdb = 1, kOpb = 2, kSpb = 3, kEpb = 6;
constexpr uint32_t kMagic = 0x1A2B3C4Du, kMagicSwapped = 0x4D3C2B1Au;

inline uint16_t rd16(const uint8_t* p, bool sw) {
  uint16_t v;
  memcpy(&v, p, 2);
  return sw ? __builtin_bswap16(v) : v;
}
inline uint32_t rd32(const uint8_t* p, bool sw) {
  uint32_t v;
  memcpy(&v, p, 4);
  return sw ? __builtin_bswap32(v) : v;
}
inline uint64_t rd64(const uint8_t* p, bool sw) {
  uint64_t v;
  memcpy(&v, p, 8);
  return sw ? __builtin_bswap64(v) : v;
}

// the options of one IDB in [p, end): MGENX_PCAPNG_OK, _BLOCK (an option past the block) or
// _TSRESOL (rule 4).  Both bounds are 4-aligned within the block, so a value that fits has its
// padding inside the block too.
inline int idb_options(const uint8_t* p, const uint8_t* end, bool sw, mgenx_pcapng_if* f) {
  bool have_res = false, have_off = false;
  while (end - p >= 4) {
    const uint32_t code = rd16(p, sw), len = rd16(p + 2, sw);
    if (code == 0) break;
    p += 4;
    if ((uint64_t)(end - p) < len) return MGENX_PCAPNG_BLOCK;
    if (code == 9) {  // if_tsresol
      if (len != 1 || have_res) return MGENX_PCAPNG_TSRESOL;
      have_res = true;
      const uint32_t v = p[0] & 0x7Fu;
      if (p[0] & 0x80u) {
        if (v > 63) return MGENX_PCAPNG_TSRESOL;
        f->ts_units = 1ull << v;
        f->ts_binary = 1;
      } else {
        if (v > 19) return MGENX_PCAPNG_TSRESOL;
        uint64_t u = 1;
        for (uint32_t k = 0; k < v; k++) u *= 10u;
        f->ts_units = u;
        f->ts_binary = 0;
      }
    } else if (code == 14) {  // if_tsoffset
      if (len != 8 || have_off) return MGENX_PCAPNG_TSRESOL;
      have_off = true;
      f->ts_offset = (int64_t)rd64(p, sw);
    }
    p += (len + 3u) & ~3u;
  }
  return MGENX_PCAPNG_OK;
}

// mgenx_pcapng_index (include/mgenx.h)
inline int index(const uint8_t* buf, uint64_t nbytes, uint64_t* pkt_off, uint32_t* pkt_if,
                 uint64_t cap, mgenx_pcapng_if* ifaces, uint32_t if_cap,
                 mgenx_pcapng_info* info) {
  if (!buf || !info || (cap && (!pkt_off || !pkt_if)) || (if_cap && !ifaces))
    return MGENX_EINVAL;
  memset(info, 0, sizeof(*info));
  // rule 1: an SHB first, its magic gives the byte order
  if (nbytes < 12 || rd32(buf, false) != kShb) return MGENX_EINVAL;
  const uint32_t magic = rd32(buf + 8, false);
  if (magic != kMagic && magic != kMagicSwapped) return MGENX_EINVAL;
  const bool sw = magic == kMagicSwapped;
  info->flags = MGENX_PCAP_NG | (sw ? MGENX_PCAP_SWAPPED : 0u);

  uint64_t off = 0, n = 0;
  uint32_t n_if = 0;         // rows of the interface table (all sections)
  uint32_t sec_base = 0;     // the current section's first row
  uint32_t sec_snap0 = 0;    // the snaplen of its interface 0 (the SPB's)
  bool have_link = false;
  int status = MGENX_PCAPNG_OK;
  while (off < nbytes) {
    const uint64_t left = nbytes - off;
    const uint8_t* b = buf + off;
    if (left < 8) { status = MGENX_PCAPNG_TRUNCATED; break; }
    const uint32_t type = rd32(b, sw);  // the SHB's type reads the same in either order
    if (type == kShb) {  // rule 2: its magic first, the lengths are in the new order
      if (left < 12) { status = MGENX_PCAPNG_TRUNCATED; break; }
      if (rd32(b + 8, false) != magic) { status = MGENX_PCAPNG_SECTION; break; }
    }
    const uint32_t len = rd32(b + 4, sw);
    const uint32_t min_len = type == kShb ? 28u : type == kIdb ? 20u
                             : (type == kEpb || type == kOpb) ? 32u : type == kSpb ? 16u : 12u;
    if (len < min_len || (len & 3u)) { status = MGENX_PCAPNG_BLOCK; break; }
    if (left < len) { status = MGENX_PCAPNG_TRUNCATED; break; }
    if (rd32(b + len - 4, sw) != len) { status = MGENX_PCAPNG_BLOCK; break; }
    if (type == kShb) {
      if (rd16(b + 12, sw) != 1) {
        if (off == 0) return MGENX_EINVAL;
        status = MGENX_PCAPNG_SECTION;
        break;
      }
      info->n_sections++;
      sec_base = n_if;
      sec_snap0 = 0;
    } else if (type == kIdb) {
      mgenx_pcapng_if f;
      memset(&f, 0, sizeof(f));
      f.ts_units = 1000000u;
      f.snaplen = rd32(b + 12, sw);
      status = idb_options(b + 16, b + len - 4, sw, &f);
      if (status != MGENX_PCAPNG_OK) break;
      const uint32_t link = rd16(b + 8, sw);
      if (have_link && link != info->link_type) { status = MGENX_PCAPNG_LINKTYPE; break; }
      if (!have_link) {  // rule 3: the first IDB's link type and snaplen are the file's
        have_link = true;
        info->link_type = link;
        info->snaplen = f.snaplen;
      }
      if (n_if == sec_base) sec_snap0 = f.snaplen;
      if (n_if < if_cap) ifaces[n_if] = f;
      n_if++;
    } else if (type == kEpb || type == kOpb || type == kSpb) {
      uint32_t iface = 0, caplen, origlen;
      if (type == kSpb) {
        origlen = rd32(b + 8, sw);
      } else {
        iface = type == kEpb ? rd32(b + 8, sw) : rd16(b + 8, sw);
        origlen = rd32(b + 24, sw);
      }
      if (iface >= n_if - sec_base) { status = MGENX_PCAPNG_NO_IFACE; break; }  // rule 5
      if (type == kSpb) {  // rule 6
        caplen = origlen;
        if (sec_snap0 && caplen > sec_snap0) caplen = sec_snap0;
        if (caplen > len - 16) caplen = len - 16;
      } else {
        caplen = rd32(b + 20, sw);
        if (caplen > len - 32) { status = MGENX_PCAPNG_CAPLEN; break; }
      }
      if (caplen < origlen) info->snap_bytes += ((uint64_t)origlen + 15) & ~15ull;
      if (n < cap) {
        pkt_off[n] = off;
        pkt_if[n] = sec_base + iface;
      }
      n++;
    }
    off += len;
  }
  info->status = status;
  info->n_records = n;
  info->consumed = off;
  info->n_ifaces = n_if;
  return MGENX_OK;
}

}  // namespace ng
}  // namespace mgenx
