// mgenx_unpack.hpp -- what the unpack kernel families share (internal): the braid CRC
// primitives and LDS table staging, the header prefix helpers, the column and row stores, and
// the launchers that launch_unpack (mgenx_unpack.hip) dispatches to:
//   mgenx_unpack.hip        the general kernel and launch_unpack; it also compiles
//   mgenx_unpack_var.hpp      per-record lengths, rows in a load ring across groups, and
//   mgenx_unpack_long.hpp     long records, one wave per record
//   mgenx_unpack_fixed.hip  fixed-length records: the pipelined and the ring kernel
#pragma once

#include <type_traits>

#include "mgenx_kernels.hpp"
#include "mgenx_parse.hpp"

namespace mgenx {

constexpr int kUnpackThreads = 1024;
constexpr int kRep = 32;                       // A_64 replicas (one per LDS bank)
constexpr int kRepDwords = 4 * 256 * kRep;     // 32768 dwords = 128 KiB
constexpr int kSmallTabDwords = 1024;          // one shift operator: 4 x 256 dwords
// fold operators A_4, A_8, A_12, A_16, A_32, A_48 (not replicated)
constexpr int kFoldTabs = 6;
constexpr size_t kUnpackLdsBytes = (size_t)(kRepDwords + kFoldTabs * kSmallTabDwords) * 4u;


// Replicated A_64 tables.  Entry (k, v, copy) -- table k (byte k of the state), byte value v,
// replica copy = lane & 31 -- sits at LDS byte address
//     (k >> 1) * 65536 + v * 256 + (k & 1) * 128 + copy * 4,
// so lane l always reads bank l (conflict-free ds_read_b32), and ONE v_perm_b32 forms each
// address from the state word: byte 1 <- byte k of the state, byte 0 <- copy * 4 and
// byte 2 <- k >> 1 (both from the lane constant s1 = copy * 4 | 1 << 16); (k & 1) * 128 is
// the ds_read immediate.  That is one VALU op per lookup, plus one v_bitop3 (XOR3) per
// three lookups to combine them.
__device__ __forceinline__ uint32_t a64_s1(uint32_t lane) { return ((lane & 31u) << 2) | (1u << 16); }

// The tables are addressed by absolute LDS address: these kernels have no static LDS, so the
// dynamic allocation starts at 0.  (Going through the extern array pointer would cost one
// v_add of its link-time base, 0, per lookup.)
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
__device__ __forceinline__ uint32_t lds_u32(const uint8_t*, uint32_t addr, uint32_t imm) {
  return *(const lds_u32_t*)(addr + imm);
}

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// A_64(c) as two partial words (A_64(c) = ha ^ hb), so the caller folds them together with
// the next row's data in one XOR3.
__device__ __forceinline__ void a64_parts(const uint8_t* ldsb, uint32_t c, uint32_t s1,
                                          uint32_t& ha, uint32_t& hb) {
  const uint32_t t0 = lds_u32(ldsb, __builtin_amdgcn_perm(c, s1, 0x0c0c0400u), 0);
  const uint32_t t1 = lds_u32(ldsb, __builtin_amdgcn_perm(c, s1, 0x0c0c0500u), 128);
  const uint32_t t2 = lds_u32(ldsb, __builtin_amdgcn_perm(c, s1, 0x0c020600u), 0);
  const uint32_t t3 = lds_u32(ldsb, __builtin_amdgcn_perm(c, s1, 0x0c020700u), 128);
  ha = xor3(t0, t1, t2);
  hb = t3;
}

// Stage the replicated A_64 tables (tabs[0..1023] = table k entry v at k * 256 + v) and the
// fold tables (tabs[1024..]) into LDS, in two halves so a caller can put other loads in
// flight between them: table_loads() reads this thread's entries (a workgroup of NT threads:
// 1024 / NT A_64 entries and six times as many fold entries, entry e = thread + i * NT),
// table_writes() stores them.  Caller synchronises.
template <int NT = 1024>
struct TableRegs {
  static_assert(1024 % NT == 0, "every thread stages the same number of entries");
  static constexpr int kPer = 1024 / NT;
  uint32_t a64[kPer], fold[kFoldTabs][kPer];
};
template <int NT = 1024>
__device__ __forceinline__ TableRegs<NT> table_loads(const uint32_t* tabs) {
  TableRegs<NT> r;
#pragma unroll
  for (int i = 0; i < r.kPer; i++) {
    const uint32_t e = threadIdx.x + (uint32_t)(i * NT);
    r.a64[i] = tabs[e];
#pragma unroll
    for (int k = 0; k < kFoldTabs; k++) r.fold[k][i] = tabs[1024 + k * 1024 + e];
  }
  return r;
}
template <int NT>
__device__ __forceinline__ void table_writes(uint32_t* lds, const TableRegs<NT>& r) {
  typedef __attribute__((address_space(3))) u32x4_t lds_u32x4_t;
  uint32_t* fold = lds + kRepDwords;
#pragma unroll
  for (int i = 0; i < r.kPer; i++) {
    const uint32_t e = threadIdx.x + (uint32_t)(i * NT);
    const uint32_t k = e >> 8, val = e & 255u;
    const u32x4_t s = {r.a64[i], r.a64[i], r.a64[i], r.a64[i]};
    lds_u32x4_t* dst = (lds_u32x4_t*)((k >> 1) * 65536u + val * 256u + (k & 1u) * 128u);
#pragma unroll
    for (int c = 0; c < kRep / 4; c++) dst[c] = s;
#pragma unroll
    for (int k2 = 0; k2 < kFoldTabs; k2++) fold[k2 * 1024 + e] = r.fold[k2][i];
  }
}
__device__ __forceinline__ void stage_tables(uint32_t* lds, const uint32_t* tabs) {
  table_writes(lds, table_loads(tabs));
}

__device__ __forceinline__ uint32_t shift_tab(const uint32_t* t, uint32_t x) {
  return t[x & 0xffu] ^ t[256 + ((x >> 8) & 0xffu)] ^ t[512 + ((x >> 16) & 0xffu)] ^
         t[768 + (x >> 24)];
}

// 128-bit little-endian left shift by s bytes (0 < s < 16), zero fill.
__device__ __forceinline__ u32x4_t shl_bytes(u32x4_t v, int s) {
  const int a = s >> 2;
  const int c = (s & 3) * 8;
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int hi_i = i - a, lo_i = i - a - 1;
    uint32_t hi = 0, lo = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      hi = (k == hi_i) ? w[k] : hi;
      lo = (k == lo_i) ? w[k] : lo;
    }
    o[i] = c ? ((hi << c) | (lo >> (32 - c))) : hi;
  }
  return u32x4_t{o[0], o[1], o[2], o[3]};
}

// load_addr16, Hdr, load_fixed, fixed_ok, parse_header: mgenx_parse.hpp (shared with the
// resident single-message worker, mgenx_worker.hip)

// Layouts the register-only parse handles (given the first 64 bytes pw[0..15] of a record
// with buf_len >= 64): version 2, dst type IPv4/IPv6, dst and host address lengths in
// {0,4,16} (every later field is then word-aligned) and header <= 64 bytes (so not IPv6
// dst + IPv6 host).  Field meaning follows mgenMsg.cpp:323-497 as in parse_header.
__device__ __forceinline__ bool fast_layout(uint32_t w0, uint32_t w5, uint32_t hw) {
  const uint32_t t = (w5 >> 16) & 0xffu;
  const uint32_t D = w5 >> 24;
  const uint32_t H = hw >> 24;
  return ((w0 >> 16) & 0xffu) == 2u && (t == 1u || t == 2u) && (D == 4u || D == 16u) &&
         (H == 0u || H == 4u || H == 16u) && D + H <= 20u;
}

// CRC-32 (init/xorout ~0) computed bit by bit: used only for records shorter than 32 B.
__device__ bool small_crc_ok(const uint8_t* r, uint32_t L) {
  if (L < 4) return false;
  uint32_t c = 0xFFFFFFFFu;
  for (uint32_t i = 0; i < L - 4; i++) {
    c ^= r[i];
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? kPoly : 0u);
  }
  c ^= 0xFFFFFFFFu;
  const uint32_t t = ((uint32_t)r[L - 4] << 24) | ((uint32_t)r[L - 3] << 16) |
                     ((uint32_t)r[L - 2] << 8) | r[L - 1];
  return c == t;
}

// Word k (0..15) of the quad's 64-byte header prefix, read from quad lane k/4's chunk by
// DPP at the point of use (k is a constant after inlining, so the switch folds away).
// All four lanes of the quad must be active.
__device__ __forceinline__ uint32_t prefix_word(const u32x4_t& pf, int k) {
#define MGENX_PW(K, C, LN) \
  case K: return (uint32_t)__builtin_amdgcn_mov_dpp((int)pf.C, LN * 0x55, 0xf, 0xf, false);
  switch (k) {
    MGENX_PW(0, x, 0) MGENX_PW(1, y, 0) MGENX_PW(2, z, 0) MGENX_PW(3, w, 0)
    MGENX_PW(4, x, 1) MGENX_PW(5, y, 1) MGENX_PW(6, z, 1) MGENX_PW(7, w, 1)
    MGENX_PW(8, x, 2) MGENX_PW(9, y, 2) MGENX_PW(10, z, 2) MGENX_PW(11, w, 2)
    MGENX_PW(12, x, 3) MGENX_PW(13, y, 3) MGENX_PW(14, z, 3) MGENX_PW(15, w, 3)
    default: return 0u;
  }
#undef MGENX_PW
}

// ---- column stores (quad lane 0 of the record) ----

// The caller's receive check: a CRC mismatch becomes ERROR_CHECKSUM, plus the
// CHECKSUM_ERROR flag on TCP (mgenTransport.cpp:971-975, 1552-1560).
__device__ __forceinline__ void crc_verdict(bool crc_ok, bool tcp, uint8_t& err,
                                            uint8_t& flags) {
  if (!crc_ok) {
    err = MGENX_ERROR_CHECKSUM;
    if (tcp) flags |= MGENX_FLAG_CHECKSUM_ERROR;
  }
}

// Extended columns of a fast-layout record: every word is read with all lanes active (the
// DPP reads cross the quad), then only `do_store` lanes (quad lane 0) store.
template <typename PW>
__device__ __forceinline__ void store_fast_ext(const mgenx_cols& c, uint64_t i, const PW& pw,
                                               uint32_t buf_len, bool do_store) {
  uint32_t wd[16];
#pragma unroll
  for (int k = 0; k < 16; k++) wd[k] = pw(k);
  const uint32_t D = wd[5] >> 24;
  const uint32_t hw = (D == 4u) ? wd[7] : wd[10];
  const uint32_t H = hw >> 24;
  const uint32_t ht = (hw >> 16) & 0xffu;
  const bool hv = ht == 1u || ht == 2u;
  const uint32_t gi = (28u + D + H) >> 2;  // GPS block word: 8, 9, 11 or 12
  // AND/OR masks, not selects: LLVM folds a select chain over an array back into a
  // dynamic index, which puts the array in scratch memory
  const uint32_t m8 = 0u - (uint32_t)(gi == 8u), m9 = 0u - (uint32_t)(gi == 9u);
  const uint32_t m11 = 0u - (uint32_t)(gi == 11u), m12 = 0u - (uint32_t)(gi == 12u);
  auto gword = [&](int k) {
    return (wd[8 + k] & m8) | (wd[9 + k] & m9) | (wd[11 + k] & m11) | (wd[12 + k] & m12);
  };
  const uint32_t g3 = gword(3);
  const uint32_t len = 44u + D + H;
  const uint16_t plen = bswap16((uint16_t)(g3 >> 16));
  const bool pl_ok = plen != 0 && len + plen <= buf_len;  // mgenMsg.cpp:488-497
  const uint32_t lat = bswap32(gword(0)), lon = bswap32(gword(1)), alt = bswap32(gword(2));
  const bool d16 = D == 16u;
  const u32x4_t dst = {wd[6], d16 ? wd[7] : 0u, d16 ? wd[8] : 0u, d16 ? wd[9] : 0u};
  // host address at word 8 (dst IPv4) or 11 (dst IPv6); zero unless a valid type
  const uint32_t a0 = (!hv || H == 0u) ? 0u : (D == 4u ? wd[8] : wd[11]);
  const bool h16 = hv && H == 16u;  // only with dst IPv4 (D + H <= 20)
  const u32x4_t host = {a0, h16 ? wd[9] : 0u, h16 ? wd[10] : 0u, h16 ? wd[11] : 0u};
  if (!do_store) return;
  if (c.decoded)  // a fast layout decodes every field (header <= 64 <= buf_len)
    c.decoded[i] = (uint8_t)(MGENX_DEC_MSGLEN | MGENX_DEC_BASE | MGENX_DEC_DST | MGENX_DEC_HDRLEN |
                             MGENX_DEC_GPS | MGENX_DEC_PTYPE | MGENX_DEC_PLEN |
                             (hv ? MGENX_DEC_HOST : 0));
  if (c.hdr_len) c.hdr_len[i] = (uint16_t)len;
  if (c.payload_off) c.payload_off[i] = pl_ok ? len : 0u;  // len % 4 == 0
  if (c.host_port) c.host_port[i] = hv ? bswap16((uint16_t)(hw & 0xffffu)) : 0;
  if (c.host_type) c.host_type[i] = hv ? (uint8_t)ht : 0;
  if (c.host_len) c.host_len[i] = hv ? (uint8_t)H : 0;
  if (c.lat_raw) c.lat_raw[i] = lat;
  if (c.lon_raw) c.lon_raw[i] = lon;
  if (c.alt) c.alt[i] = (int32_t)alt;
  if (c.dst_addr) *reinterpret_cast<u32x4_t*>(c.dst_addr + i * 16) = dst;
  if (c.host_addr) *reinterpret_cast<u32x4_t*>(c.host_addr + i * 16) = host;
}

// Extended columns of a record decoded by parse_header (quad lane 0).
__device__ __forceinline__ void store_hdr_ext(const mgenx_cols& c, uint64_t i, const Hdr& h) {
  if (c.decoded) c.decoded[i] = h.dec;
  if (c.hdr_len) c.hdr_len[i] = h.hdr_len;
  if (c.payload_off) c.payload_off[i] = h.poff;
  if (c.host_port) c.host_port[i] = h.host_port;
  if (c.host_type) c.host_type[i] = h.host_type;
  if (c.host_len) c.host_len[i] = h.host_len;
  if (c.lat_raw) c.lat_raw[i] = h.lat;
  if (c.lon_raw) c.lon_raw[i] = h.lon;
  if (c.alt) c.alt[i] = h.alt;
  if (c.host_addr) {
    u32x4_t* hp = reinterpret_cast<u32x4_t*>(c.host_addr + i * 16);
    *hp = u32x4_t{h.host_addr[0], h.host_addr[1], h.host_addr[2], h.host_addr[3]};
  }
  if (c.dst_addr) {
    u32x4_t* dp = reinterpret_cast<u32x4_t*>(c.dst_addr + i * 16);
    *dp = u32x4_t{h.dst_addr[0], h.dst_addr[1], h.dst_addr[2], h.dst_addr[3]};
  }
}

// A record decoded by parse_header, stored whole by quad lane 0 (the rare general
// layouts and short records): core fields as a row or as columns, then extended columns.
__device__ __forceinline__ void store_hdr_q0(const mgenx_cols& c, uint64_t i, const Hdr& h,
                                             bool crc_ok, bool tcp) {
  uint8_t err = h.err, flags = h.flags;
  crc_verdict(crc_ok, tcp, err, flags);
  if (c.rows) {
    u32x4_t* r = reinterpret_cast<u32x4_t*>(c.rows + i);
    r[0] = u32x4_t{h.flow, h.seq, h.sec, h.usec};
    r[1] = u32x4_t{h.dst4, (uint32_t)h.msg_len | ((uint32_t)h.dst_port << 16),
                   (uint32_t)h.plen | ((uint32_t)flags << 16) | ((uint32_t)err << 24),
                   (uint32_t)h.dst_type | ((uint32_t)h.dst_len << 8) |
                       ((uint32_t)h.ptype << 16) | ((uint32_t)h.gps << 24)};
  } else {
    c.flow_id[i] = h.flow;
    c.seq_num[i] = h.seq;
    c.tx_sec[i] = h.sec;
    c.tx_usec[i] = h.usec;
    c.msg_len[i] = h.msg_len;
    c.dst_port[i] = h.dst_port;
    c.flags[i] = flags;
    c.err[i] = err;
    c.dst_type[i] = h.dst_type;
    c.dst_len[i] = h.dst_len;
    c.dst_addr4[i] = h.dst4;
    c.payload_len[i] = h.plen;
    c.payload_type[i] = h.ptype;
    c.gps_status[i] = h.gps;
  }
  store_hdr_ext(c, i, h);
}

// Fast-layout record stored whole by quad lane 0 from the gathered prefix words pw[16]
// (general kernel): core fields as a row or as columns, then extended columns.
__device__ __forceinline__ void store_fast_q0(const mgenx_cols& c, uint64_t i,
                                              const uint32_t (&pw)[16], uint32_t buf_len,
                                              bool crc_ok, bool tcp) {
  const uint32_t D = pw[5] >> 24;
  const uint32_t hw = (D == 4u) ? pw[7] : pw[10];
  const uint32_t gi = (28u + D + (hw >> 24)) >> 2;
  const uint32_t g3 = (pw[11] & (0u - (uint32_t)(gi == 8u))) |
                      (pw[12] & (0u - (uint32_t)(gi == 9u))) |
                      (pw[14] & (0u - (uint32_t)(gi == 11u))) |
                      (pw[15] & (0u - (uint32_t)(gi == 12u)));
  const uint32_t len = 44u + D + (hw >> 24);
  uint32_t plen = bswap16((uint16_t)(g3 >> 16));
  if (!(plen != 0 && len + plen <= buf_len)) plen = 0;  // mgenMsg.cpp:488-497
  uint8_t flags = (uint8_t)(pw[0] >> 24), err = 0;
  crc_verdict(crc_ok, tcp, err, flags);
  const uint32_t msg_len = bswap16((uint16_t)(pw[0] & 0xffffu));
  const uint32_t dport = bswap16((uint16_t)(pw[5] & 0xffffu));
  const uint32_t dtype = (pw[5] >> 16) & 0xffu;
  if (c.rows) {
    u32x4_t* r = reinterpret_cast<u32x4_t*>(c.rows + i);
    r[0] = u32x4_t{bswap32(pw[1]), bswap32(pw[2]), bswap32(pw[3]), bswap32(pw[4])};
    r[1] = u32x4_t{pw[6], msg_len | (dport << 16), plen | ((uint32_t)flags << 16) |
                   ((uint32_t)err << 24),
                   dtype | (D << 8) | (((g3 >> 8) & 0xffu) << 16) | ((g3 & 0xffu) << 24)};
  } else {
    c.msg_len[i] = (uint16_t)msg_len;
    c.flags[i] = flags;
    c.err[i] = err;
    c.flow_id[i] = bswap32(pw[1]);
    c.seq_num[i] = bswap32(pw[2]);
    c.tx_sec[i] = bswap32(pw[3]);
    c.tx_usec[i] = bswap32(pw[4]);
    c.dst_port[i] = (uint16_t)dport;
    c.dst_type[i] = (uint8_t)dtype;
    c.dst_len[i] = (uint8_t)D;
    c.dst_addr4[i] = pw[6];
    c.payload_len[i] = (uint16_t)plen;
    c.payload_type[i] = (uint8_t)(g3 >> 8);
    c.gps_status[i] = (uint8_t)g3;
  }
}

// A descriptor outside the slab: ERROR_OOB and zeroed core fields (quad lane 0).
__device__ __forceinline__ void store_oob_q0(const mgenx_cols& c, uint64_t i) {
  if (c.decoded) c.decoded[i] = 0;
  if (c.rows) {
    u32x4_t* r = reinterpret_cast<u32x4_t*>(c.rows + i);
    r[0] = u32x4_t{0u, 0u, 0u, 0u};
    r[1] = u32x4_t{0u, 0u, (uint32_t)MGENX_ERROR_OOB << 24, 0u};
    return;
  }
  c.err[i] = MGENX_ERROR_OOB;
  c.flags[i] = 0;
  c.msg_len[i] = 0;
  c.flow_id[i] = 0;
  c.seq_num[i] = 0;
  c.tx_sec[i] = 0;
  c.tx_usec[i] = 0;
  c.dst_port[i] = 0;
  c.dst_type[i] = 0;
  c.dst_len[i] = 0;
  c.dst_addr4[i] = 0;
  c.payload_len[i] = 0;
  c.payload_type[i] = 0;
  c.gps_status[i] = 0;
}

// The core fields of one record, as every lane of its quad holds them.
struct Core {
  uint32_t flow, seq, sec, usec, dst4, msg_len, dport, plen, flags, err, dtype, dlen, ptype, gps;
};

// Branch-free core output of a quad: lane q stores column q (u32 / u16 / u8 groups, five
// store instructions), or bytes 8q..8q+7 of the record's mgenx_rec row.  Lanes whose
// record is past the batch end store to the sink.  Every lane must call it (no branch
// around the stores: see unpack_fixed_kernel on vmcnt and skipped stores).
template <bool kRows>
__device__ __forceinline__ void store_core_quad(const UnpackParams& p, uint64_t idx, bool in,
                                                int lane, int q, const Core& v) {
  const uint64_t sink = (uint64_t)p.sink + 8u * (uint32_t)lane;
  if (kRows) {
    const uint64_t x =
        q == 0 ? ((uint64_t)v.seq << 32 | v.flow)
      : q == 1 ? ((uint64_t)v.usec << 32 | v.sec)
      : q == 2 ? ((uint64_t)((v.msg_len & 0xffffu) | v.dport << 16) << 32 | v.dst4)
               : ((uint64_t)(v.dtype | v.dlen << 8 | v.ptype << 16 | v.gps << 24) << 32 |
                  ((v.plen & 0xffffu) | v.flags << 16 | v.err << 24));
    st_g64(in ? (uint64_t)p.cols.rows + idx * 32 + 8u * q : sink, x);
    return;
  }
  const mgenx_cols& c = p.cols;
  auto at = [&](uint64_t base, uint32_t size) { return in ? base + idx * size : sink; };
  const uint64_t u32 = pick4(q, (uint64_t)c.flow_id, (uint64_t)c.seq_num, (uint64_t)c.tx_sec,
                             (uint64_t)c.tx_usec);
  const uint64_t u16 = pick4(q, (uint64_t)c.msg_len, (uint64_t)c.dst_port,
                             (uint64_t)c.payload_len, (uint64_t)c.payload_len);
  const uint64_t u8a = pick4(q, (uint64_t)c.flags, (uint64_t)c.err, (uint64_t)c.dst_type,
                             (uint64_t)c.dst_len);
  const uint64_t u8b = pick4(q, (uint64_t)c.payload_type, (uint64_t)c.gps_status,
                             (uint64_t)c.payload_type, (uint64_t)c.gps_status);
  st_g32(at(u32, 4), q == 0 ? v.flow : q == 1 ? v.seq : q == 2 ? v.sec : v.usec);
  st_g32(at((uint64_t)c.dst_addr4, 4), v.dst4);
  st_g16(at(u16, 2), q == 0 ? v.msg_len : q == 1 ? v.dport : v.plen);
  st_g8(at(u8a, 1), q == 0 ? v.flags : q == 1 ? v.err : q == 2 ? v.dtype : v.dlen);
  st_g8(at(u8b, 1), (q & 1) == 0 ? v.ptype : v.gps);
}

// store_core_quad with the per-lane field picked by AND/OR masks over scalars (a select
// chain over a struct can be folded back into a dynamic index, which puts it in scratch)
__device__ __forceinline__ void store_core_quad_m(const UnpackParams& p, uint64_t idx, bool in,
                                                  int lane, int q, const Core& v) {
  const uint32_t m0 = 0u - (uint32_t)(q == 0), m1 = 0u - (uint32_t)(q == 1);
  const uint32_t m2 = 0u - (uint32_t)(q == 2), m3 = 0u - (uint32_t)(q == 3);
  auto pick = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return (a & m0) | (b & m1) | (c & m2) | (d & m3);
  };
  const uint64_t sink = (uint64_t)p.sink + 8u * (uint32_t)lane;
  if (p.cols.rows) {
    const uint32_t lo = pick(v.flow, v.sec, v.dst4, (v.plen & 0xffffu) | v.flags << 16 | v.err << 24);
    const uint32_t hi = pick(v.seq, v.usec, (v.msg_len & 0xffffu) | v.dport << 16,
                             v.dtype | v.dlen << 8 | v.ptype << 16 | v.gps << 24);
    st_g64(in ? (uint64_t)p.cols.rows + idx * 32 + 8u * q : sink, (uint64_t)hi << 32 | lo);
    return;
  }
  const mgenx_cols& c = p.cols;
  const uint64_t a32 = pick4(q, (uint64_t)c.flow_id, (uint64_t)c.seq_num, (uint64_t)c.tx_sec,
                             (uint64_t)c.tx_usec);
  const uint64_t a16 = pick4(q, (uint64_t)c.msg_len, (uint64_t)c.dst_port,
                             (uint64_t)c.payload_len, (uint64_t)c.payload_len);
  const uint64_t a8a = pick4(q, (uint64_t)c.flags, (uint64_t)c.err, (uint64_t)c.dst_type,
                             (uint64_t)c.dst_len);
  const uint64_t a8b = pick4(q, (uint64_t)c.payload_type, (uint64_t)c.gps_status,
                             (uint64_t)c.payload_type, (uint64_t)c.gps_status);
  st_g32(in ? a32 + idx * 4 : sink, pick(v.flow, v.seq, v.sec, v.usec));
  st_g32(in ? (uint64_t)c.dst_addr4 + idx * 4 : sink, v.dst4);
  st_g16(in ? a16 + idx * 2 : sink, pick(v.msg_len, v.dport, v.plen, v.plen));
  st_g8(in ? a8a + idx : sink, pick(v.flags, v.err, v.dtype, v.dlen));
  st_g8(in ? a8b + idx : sink, pick(v.ptype, v.gps, v.ptype, v.gps));
}

// pw[4*LN .. 4*LN+3] = quad lane LN's 16-byte prefix chunk (DPP quad_perm broadcast; all
// four lanes of the quad must be active).
template <int LN>
__device__ __forceinline__ void quad_bcast(const u32x4_t& pf, uint32_t (&pw)[16]) {
  constexpr int ctrl = LN | (LN << 2) | (LN << 4) | (LN << 6);
  pw[4 * LN + 0] = (uint32_t)__builtin_amdgcn_mov_dpp((int)pf.x, ctrl, 0xf, 0xf, false);
  pw[4 * LN + 1] = (uint32_t)__builtin_amdgcn_mov_dpp((int)pf.y, ctrl, 0xf, 0xf, false);
  pw[4 * LN + 2] = (uint32_t)__builtin_amdgcn_mov_dpp((int)pf.z, ctrl, 0xf, 0xf, false);
  pw[4 * LN + 3] = (uint32_t)__builtin_amdgcn_mov_dpp((int)pf.w, ctrl, 0xf, 0xf, false);
}

// Is any extended column requested?  (They take the batch off the fixed-length kernels, and
// the other kernels store them only then.  The var kernel writes the test out: see there.)
__host__ __device__ __forceinline__ bool any_ext_cols(const mgenx_cols& c) {
  return c.hdr_len || c.payload_off || c.host_port || c.host_type || c.host_len || c.lat_raw ||
         c.lon_raw || c.alt || c.dst_addr || c.host_addr || c.decoded;
}

// ---- launchers, as launch_unpack calls them.  grid: workgroups of kUnpackThreads threads;
//      cus: the ring kernel sizes its own grid.  The fixed-length family's are defined in
//      mgenx_unpack_fixed.hip, the others in launch_unpack's translation unit ----
typedef hipError_t (*unpack_launcher)(const UnpackParams& p, int grid, int cus, hipStream_t s);

// a batch that meets launch_unpack's `fixed` condition, by record length and output form
hipError_t launch_fixed_product(const UnpackParams& p, int grid, int cus, hipStream_t s);

#if MGENX_DIAG
// The ablation masks M of the aligned 1024-byte kernel (unpack_fixed_kernel's MODE) that the
// diagnostics build instantiates, variant 1024 + M: the one list behind both launch_unpack's
// table and the instantiations in mgenx_unpack_fixed.hip.
#define MGENX_FIXED_ABL_MODES(X) X(1) X(2) X(3) X(4) X(5) X(8) X(16) X(128)
// unpack_fixed_kernel<16, M, rows?, kAligned> on 1024-byte records (rows or columns: p.cols.rows)
template <int M, bool kAligned>
hipError_t launch_fixed_1024(const UnpackParams& p, int grid, int cus, hipStream_t s);
// unpack_fixed_ring_kernel<8 or 16 rows, BR, NB, K, NW, kNt> on 512- / 1024-byte records
template <int BR, int NB, int K, int NW, bool kNt>
hipError_t launch_ring_shape(const UnpackParams& p, int grid, int cus, hipStream_t s);
#endif

}  // namespace mgenx
