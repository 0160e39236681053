// mgenx_binlogparse.hpp -- the per-record decoder of MGEN binary logs: plain functions over
// (pointer, length), compiled for the device by mgenx_binlogparse.hip and for the host by
// tests/cpp/binlog_parse_host.cpp (g++ with sanitizers).  No read leaves [p, p + n): every
// offset is checked against the record before it is read, so a record the index would have
// stopped at decodes to MGENX_PARSE_MALFORMED instead of reading its neighbour.
//
// Record (mgenMsg.cpp:1521-1555): {type u8, protocol u8, recordLength BE u16} then the body.
//   RECV  (:1560-1609)  event time (sec, usec BE u32), srcPort u16, addrType u8, addrLen u8,
//                       the address, then the stored message
//   SEND  (:1610-1627)  [mgen_msg_len BE u32 when protocol is TCP] then the stored message
//   others (:1628-1891) event time, then fields the columns do not hold
// The stored message is read the way MgenMsg::Unpack reads it (mgenMsg.cpp:315-500; the device
// form is mgenx::parse_header in mgenx_parse.hpp), bounded at the record.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "mgenx.h"

#if defined(__HIPCC__)
#define MGENX_BP_HD __host__ __device__ inline
#else
#define MGENX_BP_HD inline
#endif

namespace mgenx {
namespace bp {

constexpr uint32_t kLead = 128;       // bytes of a record a kernel stages (header + prefix + message
                                      // header need 4 + 28 + 76 = 108)
constexpr uint32_t kMaxRecord = 1024; // the reference's read buffer (:1434)

// A record's bytes: the first n_lead of them at `lead` (a staged copy, or the record itself),
// all `len` of them at `rec`.  Offsets at or past len are never read.
struct View {
  const uint8_t* lead;
  const uint8_t* rec;
  uint32_t n_lead, len;
  MGENX_BP_HD uint32_t u8(uint32_t i) const { return i < n_lead ? lead[i] : rec[i]; }
  MGENX_BP_HD uint32_t be16(uint32_t i) const { return u8(i) << 8 | u8(i + 1); }
  MGENX_BP_HD uint32_t be32(uint32_t i) const {
    return u8(i) << 24 | u8(i + 1) << 16 | u8(i + 2) << 8 | u8(i + 3);
  }
};

struct Rec {
  uint8_t event, status, protocol, flags, gps_status, err, rsv[2];
  uint16_t present, rsv2;
  uint32_t rx_sec, rx_usec, tx_sec, tx_usec, flow, seq, size, lat_raw, lon_raw;
  uint32_t data_len, data_pos;  // the data> bytes: rec[data_pos, data_pos + data_len)
  int32_t ttl, alt;
  mgenx_addr src, dst, host;
};

// The stop rule of the record walk (mgenx_binlog_index): what the walk does at a record whose
// first byte is p[0] when `avail` bytes remain in the file from there.  kWalkEnd: fewer than
// 4 bytes remain (end of file, MGENX_BINLOG_OK); kWalkNext: the record is whole and the walk
// goes on at 4 + recordLength; else the MGENX_BINLOG_* status the walk stops with.  Reads only
// bytes of the record it has checked to be there.
enum : int { kWalkNext = -1, kWalkEnd = -2 };

MGENX_BP_HD int walk_step(const View& v, uint64_t avail, uint32_t* step) {
  if (avail < 4) return kWalkEnd;
  const uint32_t ev = v.u8(0), rl = v.be16(2);
  if (rl > kMaxRecord) return MGENX_BINLOG_TOO_LONG;
  if (4ull + rl > avail) return MGENX_BINLOG_SHORT;
  if (ev == 0 || ev == 2 || ev > 16) return MGENX_BINLOG_EVENT;
  const bool addr_ev = ev == 1 || ev == 6 || ev == 7 || (ev >= 10 && ev <= 16);
  bool shortrec = rl < 8;
  if (!shortrec) {  // body offsets from 4: b[k] = v.u8(4 + k)
    if (ev == 1) shortrec = rl < 12 || rl < 12u + v.u8(15);
    else if (ev == 4 || ev == 5) shortrec = rl < 12;
    else if (ev == 6 || ev == 7) {
      shortrec = rl < 13 || rl < 13u + v.u8(15);
      if (!shortrec) shortrec = rl < 13u + v.u8(15) + v.u8(16 + v.u8(15));
    } else if (ev >= 10 && ev <= 16) shortrec = rl < 12 || rl < 18u + v.u8(15);
  }
  if (shortrec) return MGENX_BINLOG_SHORT;
  if (addr_ev && v.u8(14) != 1 && v.u8(14) != 2) return MGENX_BINLOG_EVENT;
  *step = 4 + rl;
  return kWalkNext;
}

MGENX_BP_HD void addr_clear(mgenx_addr* a) {
  a->type = a->len = 0;
  a->port = 0;
  for (int k = 0; k < 16; k++) a->addr[k] = 0;
}

MGENX_BP_HD void rec_init(Rec* r) {
  r->event = MGENX_EVENT_NONE;
  r->status = MGENX_PARSE_MALFORMED;
  r->protocol = r->flags = r->gps_status = 0;
  r->err = MGENX_ERROR_NOT_RECV;
  r->rsv[0] = r->rsv[1] = 0;
  r->present = r->rsv2 = 0;
  r->rx_sec = r->rx_usec = r->tx_sec = r->tx_usec = r->flow = r->seq = r->size = 0;
  r->lat_raw = r->lon_raw = r->data_len = r->data_pos = 0;
  r->ttl = -1;
  r->alt = 0;
  addr_clear(&r->src);
  addr_clear(&r->dst);
  addr_clear(&r->host);
}

// an address the text log prints: IPv4 with 4 bytes or IPv6 with 16 (any other pair prints
// "(invalid)", which no text parser takes back)
MGENX_BP_HD bool addr_fits(uint32_t type, uint32_t len) {
  return (type == 1 && len == 4) || (type == 2 && len == 16);
}

// min(n, room) address bytes from offset `at`; the rest stay 0
MGENX_BP_HD void addr_bytes(const View& v, uint32_t at, uint32_t n, uint32_t room, mgenx_addr* a) {
  const uint32_t lim = n < room ? n : room;
  for (uint32_t k = 0; k < lim && k < 16; k++) a->addr[k] = (uint8_t)v.u8(at + k);
}

// The stored message v[mo, mo + ml) as Unpack reads it into the fields of a RECV / SEND line.
// false: Unpack rejects it (shorter than 28 bytes, version not 2, destination type unknown) or
// an address in it has a length that does not fit its type.
MGENX_BP_HD bool decode_msg(const View& v, uint32_t mo, uint32_t ml, bool recv, Rec* r) {
  if (ml < MGENX_MIN_SIZE) return false;
  if (v.u8(mo + 2) != 2) return false;
  const uint32_t t = v.u8(mo + 22), D = v.u8(mo + 23);
  if (t != 1 && t != 2) return false;
  if (!addr_fits(t, D)) return false;
  const uint32_t msg_len = v.be16(mo), flags = v.u8(mo + 3);
  r->flow = v.be32(mo + 4);
  r->seq = v.be32(mo + 8);
  const uint32_t sec = v.be32(mo + 12), usec = v.be32(mo + 16);
  r->dst.type = (uint8_t)t;
  r->dst.len = (uint8_t)D;
  r->dst.port = (uint16_t)v.be16(mo + 20);
  addr_bytes(v, mo + 24, D, ml - 24, &r->dst);
  // the members of a fresh MgenMsg that a short message leaves alone
  uint32_t lat = 10800000u, lon = 10800000u, alt = 0, gps = 0, ptype = 0, plen = 0, poff = 0;
  uint32_t len = 24 + D;
  do {
    if (len + 4 > ml) break;
    const uint32_t hport = v.be16(mo + len), ht = v.u8(mo + len + 2), H = v.u8(mo + len + 3);
    len += 4;
    if (len + H > ml) break;
    if (ht == 1 || ht == 2) {
      if (!addr_fits(ht, H)) return false;
      r->host.type = (uint8_t)ht;
      r->host.len = (uint8_t)H;
      r->host.port = (uint16_t)hport;
      addr_bytes(v, mo + len, H, H, &r->host);
      r->present |= MGENX_HAS_HOST;
    }
    len += H;
    if (len + 13 > ml) break;
    lat = v.be32(mo + len);
    lon = v.be32(mo + len + 4);
    alt = v.be32(mo + len + 8);
    gps = v.u8(mo + len + 12);
    len += 13;
    if (len + 1 > ml) break;
    ptype = v.u8(mo + len);
    len += 1;
    if (len + 2 > ml) break;
    plen = v.be16(mo + len);
    len += 2;
    if (plen != 0 && len + plen <= ml) poff = len & ~3u;  // payload_data: the word-floored end
    else plen = 0;
  } while (false);
  if (!recv) {  // SEND line: the message's tx time is the line's stamp; no sent>, gps>, data>
    r->rx_sec = sec;
    r->rx_usec = usec;
    r->size = msg_len;
    return true;
  }
  r->tx_sec = sec;
  r->tx_usec = usec;
  r->size = msg_len;
  if (gps > 2) return true;  // LogRecvEvent ends the line at an unknown GPS status (:1056-1072)
  r->present |= MGENX_HAS_GPS;
  r->gps_status = (uint8_t)gps;
  r->lat_raw = lat;
  r->lon_raw = lon;
  r->alt = (int32_t)alt;
  if (plen && ptype == 0) {
    r->present |= MGENX_HAS_DATA;
    r->data_len = plen;
    r->data_pos = mo + poff;
  }
  r->flags = (uint8_t)(flags & (MGENX_FLAG_CONTINUES | MGENX_FLAG_END_OF_MSG |
                                MGENX_FLAG_CHECKSUM_ERROR));
  if (r->flags) r->present |= MGENX_HAS_FLAGS;
  return true;
}

// One record -> the fields of its line (include/mgenx.h, mgenx_binlog_parse).
MGENX_BP_HD void decode_record(const View& v, Rec* r) {
  rec_init(r);
  if (v.len < 4) return;
  const uint32_t ev = v.u8(0), proto = v.u8(1), rl = v.be16(2);
  r->event = ev <= 16 ? (uint8_t)ev : (uint8_t)MGENX_EVENT_NONE;
  uint32_t step = 0;
  if (walk_step(v, v.len, &step) != kWalkNext) return;
  if (ev == MGENX_EVENT_RECV) {
    const uint32_t at = v.u8(14), alen = v.u8(15);
    r->rx_sec = v.be32(4);
    r->rx_usec = v.be32(8);
    r->protocol = proto >= 1 && proto <= 3 ? (uint8_t)proto : (uint8_t)0;
    if (!addr_fits(at, alen)) return;
    r->src.type = (uint8_t)at;
    r->src.len = (uint8_t)alen;
    r->src.port = (uint16_t)v.be16(12);
    addr_bytes(v, 16, alen, alen, &r->src);
    if (!decode_msg(v, 16 + alen, rl - 12 - alen, true, r)) return;
    r->status = MGENX_PARSE_OK;
    r->err = 0;
  } else if (ev == MGENX_EVENT_SEND) {
    const uint32_t idx = proto == MGENX_PROTO_TCP ? 4u : 0u;
    r->protocol = proto >= 1 && proto <= 3 ? (uint8_t)proto : (uint8_t)0;
    if (!decode_msg(v, 4 + idx, rl - idx, false, r)) return;
    if (idx) r->size = v.be32(4);
    r->status = MGENX_PARSE_OK;
  } else {
    r->rx_sec = v.be32(4);
    r->rx_usec = v.be32(8);
    r->status = MGENX_PARSE_OK;
  }
}

}  // namespace bp
}  // namespace mgenx
