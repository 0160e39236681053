// mgenx_pcap_tcp.hip -- TCP stream reassembly for pcap2mgen (mgenx_pcap_tcp / mgenx_pcapng_tcp)
// and the framing of the rebuilt streams into records (mgenx_tcp_frame).  The contract is in
// include/mgenx.h, the design in DESIGN.md 4.10.1.  The reference drops TCP (pcap2mgen.cpp:425):
// this runs only when asked for.
//
// mgenx_pcap_tcp, over the whole capture in HBM, after the parse, the snap and the defrag step.
// No kernel walks a stream's segments in one lane: everything per key or per stream is a scan
// by key over a sorted order.
//   tcp_classify_kernel  one lane per packet: the link / IP / TCP header walk, the key, its hash
//   radix sort 1         (hash, packet), stable: a run of equal hash in capture order
//   tcp_kid_kernel       the key's id = the sorted position of the first segment with the same
//                        FULL key (the run head unless two keys share a hash)
//   radix sort 2         (key id, packet), stable: one key's segments together, capture order
//   scans by key         the latest earlier SYN -> which segments open a stream; the stream's
//                        first segment (numbering by its capture index: a flag per packet and an
//                        exclusive sum); the first payload (the base of a stream without SYN)
//   tcp_rel_kernel       rel = seq - base, stale segments, the sort key (stream, rel)
//   radix sort 3         (stream << 32 | rel, packet), stable: the contract's (rel, capture index)
//   scans by stream      E (exclusive max of rel + len), the hole (min of the positions with
//                        rel > E), the completing packet (max of the piece packets); exclusive
//                        sums give the piece numbers and the slots
//   [one read-back: the counters; too small a window or stream table ends the call here]
//   tcp_status_kernel, tcp_stream_kernel, tcp_copy_kernel (one wave per contributing segment)
// Nothing but the workspace is written before the size check.
//
// mgenx_tcp_frame: streams below long_bytes are framed one lane per stream (offset += msg_len),
// the others one at a time by the parallel scan of mgenx_scan.hip; each record's completing
// packet is a binary search in the piece table; one stable radix sort by (packet, stream) gives
// the output order.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include <vector>

#include <hipcub/hipcub.hpp>

#include "mgenx_capture.hpp"
#include "mgenx_internal.hpp"


namespace mgenx {
namespace ptcp {

using namespace capture;

constexpr uint64_t kNoSeg = ~0ull;       // sort key of a packet that takes no part
constexpr uint32_t kNoPos = 0xFFFFFFFFu;
constexpr uint8_t kNotSeg = 0, kSeg = 1, kToTruncated = 2;  // cls
constexpr uint8_t kSyn = 1;                                 // tfl
constexpr int kCntSeg = 0, kCntStale = 1, kCntGap = 2, kCntDropped = 3, kCntStreams = 4,
              kCntPieces = 5, kCntScratch = 6, kCntN = 7;
// streams from here on take the parallel scan (about 36 us a call), shorter ones a serial lane
// (0.5 to 1.8 us a record): the measurement is in DESIGN.md 4.10.1
constexpr uint64_t kDefaultLongBytes = 4ull << 20;

__device__ __forceinline__ uint32_t be32(const uint8_t* b, uint64_t i) {
  return be16(b, i) << 16 | be16(b, i + 2);
}

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
  uint8_t* status;
  mgenx_tcp_stream* streams;
  uint64_t* piece_end;
  uint32_t* piece_pkt;
  // workspace, per packet
  uint64_t* kw;    // 5 words: the addresses, then version << 32 | source port << 16 | dest port
  uint64_t* psrc;  // the payload's offset in buf
  uint32_t* seq;
  uint32_t* plen;  // payload bytes that count (0 for a SYN segment)
  uint8_t* cls;
  uint8_t* tfl;
  // sort 1 (by hash) and sort 3 (by stream and rel) share their buffers
  uint64_t* key_in;
  uint64_t* key_out;
  uint32_t* val_in;
  uint32_t* val_out;
  // in the order of sort 1
  uint32_t* headv;
  uint32_t* headpos;
  uint32_t* kid_in;
  // in the order of sort 2
  uint32_t* kid;
  uint32_t* idx2;
  uint32_t* synv;
  uint32_t* prevsyn;   // 1 + position of the key's latest earlier SYN segment, 0 = none
  uint32_t* openv;
  uint32_t* start1;    // 1 + position of the segment that opened this one's stream
  uint32_t* fpv;
  uint32_t* firstpay;  // position of the stream's first payload at or before this one
  uint32_t* isfirst;   // n + 1, per packet: the first segment of a stream
  uint32_t* srank;     // n + 1: its exclusive sum = the stream numbers
  // in the order of sort 3 (reusing the arrays of the orders before)
  uint32_t* skey;
  uint32_t* endv;
  uint32_t* E;
  uint32_t* hv;
  uint32_t* hfirst;    // position of the stream's first hole at or before this one
  uint32_t* pv;
  uint32_t* ppkt;
  uint32_t* ispiece;   // n + 1
  uint32_t* pidx;      // n + 1
  // per stream
  uint32_t* st_len;
  uint32_t* st_first;
  uint32_t* st_nseg;
  uint32_t* st_flags;
  uint64_t* st_drop;
  uint64_t* need;      // n + 1 slot sizes
  uint64_t* slot;      // n + 1 slot offsets
  uint64_t* cnt;       // kCntN counters
};

struct Seg {
  uint64_t kw[5];
  uint32_t seq, pay, plen;
  uint8_t tfl;
};

// The parse's link / IP walk without its 4094-byte frame rule, then the TCP header.
__device__ __forceinline__ uint8_t classify(const uint8_t* d, uint32_t num, uint32_t wirelen,
                                            uint32_t link_type, Seg& s) {
  uint32_t eth_type, ip0, ip_len;
  if (link_type == MGENX_DLT_LINUX_SLL) {
    if (num < 16) return kNotSeg;
    eth_type = be16(d, 14);
    ip0 = 16;
    ip_len = num - 16;
  } else {
    if (wirelen < 14 || num < 14) return kNotSeg;
    eth_type = be16(d, 12);
    uint32_t hl = 14;
    if (eth_type == 0x8100u) {
      if (wirelen < 18 || num < 18) return kNotSeg;
      eth_type = be16(d, 16);
      hl = 18;
    }
    ip0 = hl;
    ip_len = wirelen - hl;
  }
  if (eth_type != 0x0800u && eth_type != 0x86DDu) return kNotSeg;
  if (ip_len < 1 || ip0 >= num) return kNotSeg;
  const uint32_t ver = ld8(d, ip0) >> 4;
  uint32_t l4, ip_end;
  if (ver == 4) {
    if (ip_len < 20 || num - ip0 < 20) return kNotSeg;
    const uint32_t ihl = (ld8(d, ip0) & 15u) * 4u;
    const uint32_t tot = be16(d, ip0 + 2);
    if (ihl < 20 || tot < ihl || tot > ip_len) return kNotSeg;
    if (be16(d, ip0 + 6) & 0x3FFFu) return kNotSeg;  // MF or an offset: a fragment
    if (ld8(d, ip0 + 9) != 6u) return kNotSeg;
    l4 = ip0 + ihl;
    ip_end = ip0 + tot;
    s.kw[0] = ld_bytes64(d, ip0 + 12, 8);  // source, destination
    s.kw[1] = s.kw[2] = s.kw[3] = 0;
  } else if (ver == 6) {
    if (ip_len < 40 || num - ip0 < 40) return kNotSeg;
    const uint32_t pl = be16(d, ip0 + 4);
    if (40u + pl > ip_len) return kNotSeg;
    if (ld8(d, ip0 + 6) != 6u) return kNotSeg;
    l4 = ip0 + 40;
    ip_end = l4 + pl;
#pragma unroll
    for (int k = 0; k < 4; k++) s.kw[k] = ld_bytes64(d, ip0 + 8 + 8 * k, 8);
  } else {
    return kNotSeg;
  }
  if (l4 + 20 > num || l4 + 20 > ip_end) return kNotSeg;
  const uint32_t doff = (ld8(d, l4 + 12) >> 4) * 4u;
  if (doff < 20 || l4 + doff > ip_end) return kNotSeg;
  if (ip_end > num) return kToTruncated;
  s.kw[4] = (uint64_t)ver << 32 | (uint64_t)be16(d, l4) << 16 | be16(d, l4 + 2);
  s.seq = be32(d, l4 + 4);
  s.tfl = (ld8(d, l4 + 13) & 2u) ? kSyn : 0;
  s.pay = l4 + doff;
  s.plen = s.tfl ? 0u : ip_end - s.pay;  // a SYN segment's own payload is ignored
  return kSeg;
}

__global__ void __launch_bounds__(256) tcp_classify_kernel(Params p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint8_t c = kNotSeg;
  if (i < p.n) {
    uint64_t h = kNoSeg, d = 0;
    uint32_t caplen = 0, wirelen = 0;
    Seg s;
    if (p.status[i] != MGENX_PCAP_OOB && packet_data(p, i, d, caplen, wirelen))
      c = classify(p.buf + d, caplen, wirelen, p.link_type, s);
    if (c == kSeg) {
      // source and destination enter in turn: the two directions of a connection differ
      h = mix64(s.kw[4]);
#pragma unroll
      for (int k = 3; k >= 0; k--) h = mix64(h ^ s.kw[k]);
      if (h == kNoSeg) h--;
#pragma unroll
      for (int k = 0; k < 5; k++) p.kw[(uint64_t)i * 5 + k] = s.kw[k];
      p.psrc[i] = d + s.pay;
      p.seq[i] = s.seq;
      p.plen[i] = s.plen;
      p.tfl[i] = s.tfl;
    }
    p.cls[i] = c;
    p.key_in[i] = h;
    p.val_in[i] = i;
    p.isfirst[i] = 0;
    p.ispiece[i] = 0;
    p.st_len[i] = 0;
    p.st_flags[i] = 0;
    p.st_drop[i] = 0;
  }
  const uint64_t m = __ballot(c == kSeg);
  if ((threadIdx.x & 63u) == 0 && m)
    atomicAdd((unsigned long long*)&p.cnt[kCntSeg], (unsigned long long)__popcll(m));
}

__device__ __forceinline__ bool key_eq(const Params& p, uint32_t i, uint32_t j) {
  const uint64_t* a = p.kw + (uint64_t)i * 5;
  const uint64_t* b = p.kw + (uint64_t)j * 5;
  return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3] && a[4] == b[4];
}

// order of sort 1: the heads of the runs of equal hash
__global__ void __launch_bounds__(256) tcp_head_kernel(Params p) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.n) return;
  p.headv[q] = q && p.key_out[q] != p.key_out[q - 1] ? q : 0u;
}

// order of sort 1: the key's id.  A segment whose key is the run head's takes the head's
// position; only where two keys share a hash does a lane look further, for the first segment
// of the run with its own key (itself at the latest).
__global__ void __launch_bounds__(256) tcp_kid_kernel(Params p) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.n) return;
  uint32_t kid = kNoPos;
  if (p.key_out[q] != kNoSeg) {
    const uint32_t i = p.val_out[q];
    kid = p.headpos[q];
    while (kid < q && !key_eq(p, i, p.val_out[kid])) kid++;
  }
  p.kid_in[q] = kid;
}

// order of sort 2: SYN segments, for the scan that finds each segment's latest earlier SYN
__global__ void __launch_bounds__(256) tcp_syn_kernel(Params p) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.n) return;
  p.synv[q] = p.kid[q] != kNoPos && p.tfl[p.idx2[q]] ? q + 1 : 0u;
}

// order of sort 2: the segments that open a stream -- a key's first segment, and a SYN whose
// seq differs from the key's latest earlier SYN's
__global__ void __launch_bounds__(256) tcp_open_kernel(Params p) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.n) return;
  uint32_t open = 0, fp = kNoPos;
  if (p.kid[q] != kNoPos) {
    const uint32_t i = p.idx2[q];
    const uint32_t ps = p.prevsyn[q];
    if (q == 0 || p.kid[q - 1] != p.kid[q] ||
        (p.tfl[i] && (ps == 0 || p.seq[p.idx2[ps - 1]] != p.seq[i]))) {
      open = q + 1;
      p.isfirst[i] = 1;
    }
    if (p.plen[i]) fp = q;
  }
  p.openv[q] = open;
  p.fpv[q] = fp;
}

// order of sort 2: the stream number, rel, the stale test, sort 3's key; the stream's first
// segment and its last write the stream's row
__global__ void __launch_bounds__(256) tcp_rel_kernel(Params p) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  bool stale = false;
  if (q < p.n) {
    uint64_t key = kNoSeg;
    const uint32_t i = p.idx2[q];
    if (p.kid[q] != kNoPos) {
      const uint32_t sq = p.start1[q] - 1;
      const uint32_t i0 = p.idx2[sq];
      const uint32_t s = p.srank[i0];
      const bool syn = p.tfl[i0] != 0;
      if (sq == q) {
        p.st_first[s] = i;
        if (syn) p.st_flags[s] = MGENX_TCP_SYN;
      }
      if (q + 1 == p.n || p.kid[q + 1] == kNoPos || p.openv[q + 1]) p.st_nseg[s] = q + 1 - sq;
      const uint32_t len = p.plen[i];
      if (len) {
        const uint32_t base = syn ? p.seq[i0] + 1u : p.seq[p.idx2[p.firstpay[q]]];
        const uint32_t rel = p.seq[i] - base;
        stale = rel >= 0x80000000u || (uint64_t)rel + len > 0x80000000ull;
        if (!stale) key = (uint64_t)s << 32 | rel;
      }
    }
    p.key_in[q] = key;
    p.val_in[q] = i;
  }
  const uint64_t m = __ballot(stale);
  if ((threadIdx.x & 63u) == 0 && m)
    atomicAdd((unsigned long long*)&p.cnt[kCntStale], (unsigned long long)__popcll(m));
}

// order of sort 3: the stream and rel + len of each contributing segment
__global__ void __launch_bounds__(256) tcp_end_kernel(Params p) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  const uint64_t k = p.key_out[r];
  const uint32_t i = p.val_out[r];
  p.skey[r] = (uint32_t)(k >> 32);
  p.endv[r] = k == kNoSeg ? 0u : (uint32_t)k + p.plen[i];
}

// order of sort 3: a segment that starts past everything before it is a hole
__global__ void __launch_bounds__(256) tcp_hole_kernel(Params p) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  const uint64_t k = p.key_out[r];
  p.hv[r] = k != kNoSeg && (uint32_t)k > p.E[r] ? r : kNoPos;
}

// order of sort 3: the pieces; a stream's last segment writes its length
__global__ void __launch_bounds__(256) tcp_piece_kernel(Params p) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p.n) return;
  const uint64_t k = p.key_out[r];
  uint32_t pv = 0;
  if (k != kNoSeg) {
    const uint32_t s = p.skey[r], rel = (uint32_t)k, end = p.endv[r], e = p.E[r];
    const uint32_t from = rel > e ? rel : e;
    const uint32_t piece = end > from ? end - from : 0u;
    const uint32_t hole = p.hfirst[r];
    if (hole != kNoPos) {
      if (piece) {
        atomicAdd((unsigned long long*)&p.st_drop[s], (unsigned long long)piece);
        atomicAdd((unsigned long long*)&p.cnt[kCntDropped], (unsigned long long)piece);
      }
    } else if (piece) {
      p.ispiece[r] = 1;
      pv = p.val_out[r];
    }
    if (r + 1 == p.n || p.skey[r + 1] != s) {
      if (hole != kNoPos) {
        p.st_len[s] = p.E[hole];
        p.st_flags[s] |= MGENX_TCP_GAP;
        atomicAdd((unsigned long long*)&p.cnt[kCntGap], 1ull);
      } else {
        p.st_len[s] = end > e ? end : e;
      }
    }
  }
  p.pv[r] = pv;
}

// per stream: the slot sizes
__global__ void __launch_bounds__(256) tcp_need_kernel(Params p) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= p.n) return;
  p.need[s] = s < p.srank[p.n] ? ((uint64_t)p.st_len[s] + 15) & ~15ull : 0ull;
}

__global__ void tcp_totals_kernel(Params p) {
  p.cnt[kCntStreams] = p.srank[p.n];
  p.cnt[kCntPieces] = p.pidx[p.n];
  p.cnt[kCntScratch] = p.slot[p.n];
}

__global__ void __launch_bounds__(256) tcp_status_kernel(Params p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const uint8_t c = p.cls[i];
  if (c == kSeg) p.status[i] = MGENX_PCAP_TCP;
  if (c == kToTruncated) p.status[i] = MGENX_PCAP_TRUNCATED;
}

__device__ __forceinline__ void put_addr(mgenx_addr& a, const uint64_t* w, bool v6, uint32_t port) {
  a.type = v6 ? 2 : 1;
  a.len = v6 ? 16 : 4;
  a.port = (uint16_t)port;
#pragma unroll
  for (int k = 0; k < 16; k++) a.addr[k] = k < a.len ? (uint8_t)(w[k >> 3] >> (8 * (k & 7))) : 0;
}

// per stream: its row, and the zero pad of its slot
__global__ void __launch_bounds__(256) tcp_stream_kernel(Params p, uint32_t n_streams) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  const uint32_t i = p.st_first[s];
  const uint64_t* w = p.kw + (uint64_t)i * 5;
  const bool v6 = (w[4] >> 32) == 6;
  mgenx_tcp_stream t;
  if (v6) {
    put_addr(t.src, w, true, (uint32_t)(w[4] >> 16) & 0xFFFFu);
    put_addr(t.dst, w + 2, true, (uint32_t)w[4] & 0xFFFFu);
  } else {
    const uint64_t d = w[0] >> 32;
    put_addr(t.src, w, false, (uint32_t)(w[4] >> 16) & 0xFFFFu);
    put_addr(t.dst, &d, false, (uint32_t)w[4] & 0xFFFFu);
  }
  const uint32_t len = p.st_len[s];
  t.off = p.scratch_off + p.slot[s];
  t.len = len;
  t.dropped = p.st_drop[s];
  t.first_pkt = i;
  t.n_segments = p.st_nseg[s];
  t.flags = p.st_flags[s];
  t.rsv = 0;
  p.streams[s] = t;
  for (uint64_t at = t.off + len; at < t.off + p.need[s]; at++) p.buf[at] = 0;
}

// One wave per position of sort 3 (grid-stride).  A piece goes to slot + max(rel, E): source
// and destination have any alignment, and a neighbouring piece may share the destination's
// first or last 8-byte word, so the bytes before the first aligned word and after the last
// whole one are stored singly and only the words between as words.  Lane 0 writes the piece's
// row in the piece table.
__global__ void __launch_bounds__(256) tcp_copy_kernel(Params p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (blockDim.x / 64);
  for (uint32_t r = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); r < p.n; r += waves) {
    if (!p.ispiece[r]) continue;
    const uint32_t i = p.val_out[r], s = p.skey[r];
    const uint32_t rel = (uint32_t)p.key_out[r], end = p.endv[r], e = p.E[r];
    const uint32_t from = rel > e ? rel : e;
    const uint32_t len = end - from;
    const uint64_t slot = p.scratch_off + p.slot[s];
    const uint64_t dst = slot + from;
    const uint64_t src = p.psrc[i] + (from - rel);
    uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)(p.buf + dst)) & 7u;
    if (head > len) head = len;
    const uint32_t words = (len - head) / 8;
    const uint32_t tail = head + words * 8;
    if (lane < head) p.buf[dst + lane] = p.buf[src + lane];
    uint64_t* out = (uint64_t*)(p.buf + dst + head);
    for (uint32_t w = lane; w < words; w += 64)
      out[w] = ld_word(p.buf, p.buf_bytes, src + head + w * 8, 8);
    if (lane < len - tail) p.buf[dst + tail + lane] = p.buf[src + tail + lane];
    if (lane == 0) {
      const uint32_t k = p.pidx[r];
      p.piece_end[k] = slot + end;
      p.piece_pkt[k] = p.ppkt[r];
    }
  }
}

// the most temporary storage any of the library calls below asks for
static size_t cub_bytes(uint32_t n) {
  size_t best = 0, b = 0;
  const hipStream_t s = 0;
  uint64_t* k64 = nullptr;
  uint32_t* u = nullptr;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t*)k64, k64,
                                           (const uint32_t*)u, u, (int)n, 0, 64, s);
  best = b;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)u, u, (const uint32_t*)u,
                                           u, (int)n, 0, 32, s);
  best = b > best ? b : best;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, k64, k64, (int)n + 1, s);
  best = b > best ? b : best;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, u, u, (int)n + 1, s);
  best = b > best ? b : best;
  (void)hipcub::DeviceScan::InclusiveScan(nullptr, b, u, u, hipcub::Max(), (int)n, s);
  best = b > best ? b : best;
  (void)hipcub::DeviceScan::ExclusiveScanByKey(nullptr, b, u, u, u, hipcub::Max(), 0u, (int)n,
                                               hipcub::Equality(), s);
  best = b > best ? b : best;
  (void)hipcub::DeviceScan::InclusiveScanByKey(nullptr, b, u, u, u, hipcub::Min(), (int)n,
                                               hipcub::Equality(), s);
  best = b > best ? b : best;
  return best;
}

// ------------------------------------------------------------------ mgenx_tcp_frame
struct Frame {
  const uint8_t* buf;
  const mgenx_tcp_stream* streams;
  uint32_t n_streams;
  const uint64_t* piece_end;
  const uint32_t* piece_pkt;
  uint32_t n_pieces;
  uint64_t long_bytes;
  uint64_t cap;
  uint64_t* count;   // n_streams + 1 record counts of the short streams -> their bases
  uint64_t* t_off;   // cap records in stream order: the short streams', then the long ones'
  uint32_t* t_len;
  uint32_t* t_stream;
  uint8_t* stream_status;
};

// One lane per stream below long_bytes: MgenTcpTransport's framing rule (mgenx_scan.hip).
// write false: the counts and statuses; true: the records, at the stream's base.
__global__ void __launch_bounds__(64) frame_short_kernel(Frame f, bool write) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= f.n_streams) return;
  const uint64_t len = f.streams[s].len;
  uint64_t n = 0;
  if (len < f.long_bytes) {
    const uint64_t off = f.streams[s].off, end = off + len;
    uint8_t st = 0;
    uint64_t at = off;
    while (end - at >= 2) {
      const uint32_t L = be16(f.buf, at);
      if (L < 4) { st = 1; break; }
      if (end - at < L) break;
      if (write && f.count[s] + n < f.cap) {
        const uint64_t j = f.count[s] + n;
        f.t_off[j] = at;
        f.t_len[j] = L;
        f.t_stream[j] = s;
      }
      n++;
      at += L;
    }
    if (!write) f.stream_status[s] = st;
  }
  if (!write) f.count[s] = n;
}

// a long stream's records as the scan wrote them, relative to the stream: make them absolute
__global__ void __launch_bounds__(256) frame_long_fix_kernel(uint64_t* t_off, uint32_t* t_stream,
                                                             uint64_t n, uint64_t off,
                                                             uint32_t s) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  t_off[j] += off;
  t_stream[j] = s;
}

// per record: the completing packet = the packet of the first piece that ends at or after
// the record's end, and the sort key (packet, stream)
__global__ void __launch_bounds__(256) frame_key_kernel(Frame f, uint32_t n, uint64_t* key,
                                                        uint32_t* val) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t e = f.t_off[j] + f.t_len[j];
  uint32_t lo = 0, hi = f.n_pieces;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (f.piece_end[mid] < e) lo = mid + 1; else hi = mid;
  }
  // a record lies inside its stream, and the stream ends with a piece: lo < n_pieces
  const uint32_t pkt = lo < f.n_pieces ? f.piece_pkt[lo] : kNoPos;
  key[j] = (uint64_t)pkt << 32 | f.t_stream[j];
  val[j] = j;
}

__global__ void __launch_bounds__(256) frame_out_kernel(
    Frame f, uint32_t n, const uint64_t* key, const uint32_t* val, const uint32_t* pkt_rx_sec,
    const uint32_t* pkt_rx_usec, uint64_t* rec_off, uint32_t* rec_len, uint32_t* rec_stream,
    uint32_t* rec_pkt, mgenx_addr* rec_src, uint32_t* rec_rx_sec, uint32_t* rec_rx_usec) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t t = val[j], pkt = (uint32_t)(key[j] >> 32), s = (uint32_t)key[j];
  rec_off[j] = f.t_off[t];
  rec_len[j] = f.t_len[t];
  rec_stream[j] = s;
  rec_pkt[j] = pkt;
  rec_src[j] = f.streams[s].src;
  rec_rx_sec[j] = pkt == kNoPos ? 0u : pkt_rx_sec[pkt];  // kNoPos: a piece table that does not
  rec_rx_usec[j] = pkt == kNoPos ? 0u : pkt_rx_usec[pkt];  // cover the stream (frame_key_kernel)
}

static size_t frame_cub_bytes(uint64_t cap, uint32_t n_streams) {
  size_t a = 0, b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const uint64_t*)nullptr,
                                           (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (int)cap, 0, 64, (hipStream_t)0);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (int)n_streams + 1, (hipStream_t)0);
  return a > b ? a : b;
}

}  // namespace ptcp
}  // namespace mgenx

using namespace mgenx::ptcp;
using mgenx::a256;
using mgenx::Carve;

static size_t pcap_tcp_ws(uint32_t n) {
  const size_t N = n;
  return 4 * a256(N * 8) + a256(N * 40) + 4 * a256((N + 1) * 4) + 19 * a256(N * 4) +
         2 * a256(N) + 2 * a256((N + 1) * 8) + a256(kCntN * 8) + a256(cub_bytes(n));
}

// dev_data_off null: classic records at dev_pkt_off; else pcapng (as defrag_run of
// mgenx_defrag.hip).  `mem` holds pcap_tcp_ws(n) bytes.  Synchronizes the stream once (the counters' read-back).
static int pcap_tcp_run(void* mem, uint8_t* dev_buf, uint64_t scratch_off, uint64_t buf_bytes,
                        const uint64_t* dev_pkt_off, const uint64_t* dev_data_off,
                        const uint32_t* dev_cap_len, uint32_t n, uint32_t link_type, uint32_t flags,
                        uint8_t* dev_status, mgenx_tcp_stream* dev_streams, uint32_t stream_cap,
                        uint64_t* dev_piece_end, uint32_t* dev_piece_pkt, mgenx_tcp_stats* stats,
                        hipStream_t stream, char* err, size_t errn) {
  Params p;
  p.buf = dev_buf; p.limit = scratch_off; p.buf_bytes = buf_bytes; p.scratch_off = scratch_off;
  p.pkt_off = dev_pkt_off; p.data_off = dev_data_off; p.cap_len = dev_cap_len; p.n = n;
  p.link_type = link_type; p.flags = flags; p.status = dev_status; p.streams = dev_streams;
  p.piece_end = dev_piece_end; p.piece_pkt = dev_piece_pkt;
  const size_t N = n;
  Carve take(mem);
  auto u32s = [&](size_t k) { return (uint32_t*)take(k * 4); };
  p.key_in = (uint64_t*)take(N * 8);
  p.key_out = (uint64_t*)take(N * 8);
  p.psrc = (uint64_t*)take(N * 8);
  p.st_drop = (uint64_t*)take(N * 8);
  p.kw = (uint64_t*)take(N * 40);
  p.isfirst = u32s(N + 1); p.srank = u32s(N + 1); p.ispiece = u32s(N + 1); p.pidx = u32s(N + 1);
  p.val_in = u32s(N); p.val_out = u32s(N); p.seq = u32s(N); p.plen = u32s(N);
  p.headv = u32s(N); p.headpos = u32s(N);
  p.kid_in = u32s(N); p.kid = u32s(N); p.idx2 = u32s(N); p.synv = u32s(N);
  p.prevsyn = u32s(N); p.openv = u32s(N); p.start1 = u32s(N); p.fpv = u32s(N);
  p.firstpay = u32s(N);
  p.st_len = u32s(N); p.st_first = u32s(N); p.st_nseg = u32s(N); p.st_flags = u32s(N);
  p.cls = (uint8_t*)take(N);
  p.tfl = (uint8_t*)take(N);
  p.need = (uint64_t*)take((N + 1) * 8);
  p.slot = (uint64_t*)take((N + 1) * 8);
  p.cnt = (uint64_t*)take(kCntN * 8);
  // the order of sort 3 reuses arrays that are dead by then
  p.skey = p.headv; p.endv = p.headpos; p.E = p.kid_in; p.hv = p.synv; p.hfirst = p.prevsyn;
  p.pv = p.fpv; p.ppkt = p.firstpay;
  size_t tmp_bytes = cub_bytes(n);
  void* tmp = take(tmp_bytes);
  auto fail = [&](hipError_t e, const char* where) {
    snprintf(err, errn, "%s: %s", where, hipGetErrorString(e));
    return MGENX_EDEVICE;
  };
  const int ni = (int)n;
  const dim3 grid((n + 255) / 256), block(256);
  const hipcub::Equality eq;
  size_t have;
  hipError_t e = hipMemsetAsync(p.cnt, 0, kCntN * 8, stream);
  if (e == hipSuccess) e = hipMemsetAsync(p.isfirst + n, 0, 4, stream);
  if (e == hipSuccess) e = hipMemsetAsync(p.ispiece + n, 0, 4, stream);
  if (e == hipSuccess) e = hipMemsetAsync(p.need + n, 0, 8, stream);
  if (e != hipSuccess) return fail(e, "pcap_tcp clear");
#define TCP_CUB(call, where)                 \
  have = tmp_bytes;                          \
  if ((e = (call)) != hipSuccess) return fail(e, where)
  hipLaunchKernelGGL(tcp_classify_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceRadixSort::SortPairs(tmp, have, p.key_in, p.key_out, p.val_in, p.val_out,
                                             ni, 0, 64, stream), "pcap_tcp sort 1");
  hipLaunchKernelGGL(tcp_head_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceScan::InclusiveScan(tmp, have, p.headv, p.headpos, hipcub::Max(), ni,
                                            stream), "pcap_tcp heads");
  hipLaunchKernelGGL(tcp_kid_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceRadixSort::SortPairs(tmp, have, p.kid_in, p.kid, p.val_out, p.idx2, ni,
                                             0, 32, stream), "pcap_tcp sort 2");
  hipLaunchKernelGGL(tcp_syn_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceScan::ExclusiveScanByKey(tmp, have, p.kid, p.synv, p.prevsyn,
                                                 hipcub::Max(), 0u, ni, eq, stream),
          "pcap_tcp SYN scan");
  hipLaunchKernelGGL(tcp_open_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceScan::InclusiveScan(tmp, have, p.openv, p.start1, hipcub::Max(), ni,
                                            stream), "pcap_tcp stream starts");
  TCP_CUB(hipcub::DeviceScan::ExclusiveSum(tmp, have, p.isfirst, p.srank, ni + 1, stream),
          "pcap_tcp stream numbers");
  TCP_CUB(hipcub::DeviceScan::InclusiveScanByKey(tmp, have, p.start1, p.fpv, p.firstpay,
                                                 hipcub::Min(), ni, eq, stream),
          "pcap_tcp first payload");
  hipLaunchKernelGGL(tcp_rel_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceRadixSort::SortPairs(tmp, have, p.key_in, p.key_out, p.val_in, p.val_out,
                                             ni, 0, 64, stream), "pcap_tcp sort 3");
  hipLaunchKernelGGL(tcp_end_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceScan::ExclusiveScanByKey(tmp, have, p.skey, p.endv, p.E, hipcub::Max(),
                                                 0u, ni, eq, stream), "pcap_tcp E scan");
  hipLaunchKernelGGL(tcp_hole_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceScan::InclusiveScanByKey(tmp, have, p.skey, p.hv, p.hfirst,
                                                 hipcub::Min(), ni, eq, stream),
          "pcap_tcp hole scan");
  hipLaunchKernelGGL(tcp_piece_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceScan::InclusiveScanByKey(tmp, have, p.skey, p.pv, p.ppkt, hipcub::Max(),
                                                 ni, eq, stream), "pcap_tcp packet scan");
  TCP_CUB(hipcub::DeviceScan::ExclusiveSum(tmp, have, p.ispiece, p.pidx, ni + 1, stream),
          "pcap_tcp piece numbers");
  hipLaunchKernelGGL(tcp_need_kernel, grid, block, 0, stream, p);
  TCP_CUB(hipcub::DeviceScan::ExclusiveSum(tmp, have, p.need, p.slot, ni + 1, stream),
          "pcap_tcp slots");
#undef TCP_CUB
  hipLaunchKernelGGL(tcp_totals_kernel, dim3(1), dim3(1), 0, stream, p);
  uint64_t h[kCntN];
  e = hipMemcpyAsync(h, p.cnt, sizeof(h), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(e, "pcap_tcp sizes");
  stats->n_segments = h[kCntSeg];
  stats->n_streams = h[kCntStreams];
  stats->n_gap_streams = h[kCntGap];
  stats->n_stale = h[kCntStale];
  stats->dropped_bytes = h[kCntDropped];
  stats->n_pieces = h[kCntPieces];
  stats->scratch_bytes = h[kCntScratch];
  if (stream_cap < h[kCntStreams] || buf_bytes - scratch_off < h[kCntScratch])
    return MGENX_ENOSPC;
  if (h[kCntScratch] && ((uintptr_t)(dev_buf + scratch_off) & 15u)) {
    snprintf(err, errn, "pcap_tcp: the scratch window is not 16-byte aligned");
    return MGENX_EINVAL;
  }
  hipLaunchKernelGGL(tcp_status_kernel, grid, block, 0, stream, p);
  const uint32_t ns = (uint32_t)h[kCntStreams];
  if (ns)
    hipLaunchKernelGGL(tcp_stream_kernel, dim3((ns + 255) / 256), block, 0, stream, p, ns);
  if (h[kCntPieces]) {
    const uint32_t cblocks = n < 2048u * 4u ? (n + 3) / 4 : 2048u;
    hipLaunchKernelGGL(tcp_copy_kernel, dim3(cblocks), block, 0, stream, p);
  }
  e = hipGetLastError();
  return e == hipSuccess ? MGENX_OK : fail(e, "pcap_tcp");
}

static size_t tcp_frame_ws(uint32_t n_streams, uint64_t cap) {
  const size_t S = n_streams, C = cap;
  return a256((S + 1) * 8) + 3 * a256(C * 8) + 4 * a256(C * 4) +
         a256(frame_cub_bytes(cap, n_streams));
}

// `mem` holds tcp_frame_ws(n_streams, cap) bytes; scan_ws: the context's stream-scan
// workspace.  Synchronous: the stream table (checked against buf_bytes) and the short streams'
// total are read back, and each long stream's scan synchronizes.
static int tcp_frame_run(void* mem, mgenx_scan_ws* scan_ws, const uint8_t* dev_buf,
                         uint64_t buf_bytes, const mgenx_tcp_stream* dev_streams,
                         uint32_t n_streams, const uint64_t* dev_piece_end,
                         const uint32_t* dev_piece_pkt, uint32_t n_pieces,
                         const uint32_t* dev_pkt_rx_sec, const uint32_t* dev_pkt_rx_usec,
                         uint64_t long_bytes, uint64_t* dev_rec_off, uint32_t* dev_rec_len,
                         uint32_t* dev_rec_stream, uint32_t* dev_rec_pkt, mgenx_addr* dev_rec_src,
                         uint32_t* dev_rec_rx_sec, uint32_t* dev_rec_rx_usec, uint64_t cap,
                         uint8_t* dev_stream_status, uint64_t* n_records, hipStream_t stream,
                         char* err, size_t errn) {
  Frame f;
  f.buf = dev_buf; f.streams = dev_streams; f.n_streams = n_streams;
  f.piece_end = dev_piece_end; f.piece_pkt = dev_piece_pkt; f.n_pieces = n_pieces;
  f.long_bytes = long_bytes ? long_bytes : kDefaultLongBytes;
  f.cap = cap; f.stream_status = dev_stream_status;
  Carve take(mem);
  f.count = (uint64_t*)take(((size_t)n_streams + 1) * 8);
  f.t_off = (uint64_t*)take(cap * 8);
  uint64_t* key_in = (uint64_t*)take(cap * 8);
  uint64_t* key_out = (uint64_t*)take(cap * 8);
  f.t_len = (uint32_t*)take(cap * 4);
  f.t_stream = (uint32_t*)take(cap * 4);
  uint32_t* val_in = (uint32_t*)take(cap * 4);
  uint32_t* val_out = (uint32_t*)take(cap * 4);
  size_t tmp_bytes = frame_cub_bytes(cap, n_streams);
  void* tmp = take(tmp_bytes);
  auto fail = [&](hipError_t e, const char* where) {
    snprintf(err, errn, "%s: %s", where, hipGetErrorString(e));
    return MGENX_EDEVICE;
  };
  std::vector<mgenx_tcp_stream> hs(n_streams);
  hipError_t e = hipMemcpyAsync(hs.data(), dev_streams, sizeof(mgenx_tcp_stream) * n_streams,
                                hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemsetAsync(f.count + n_streams, 0, 8, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(e, "tcp_frame streams");
  for (const mgenx_tcp_stream& t : hs)
    if (t.off > buf_bytes || buf_bytes - t.off < t.len) {
      snprintf(err, errn, "tcp_frame: a stream does not lie inside the buffer");
      return MGENX_EINVAL;
    }
  const dim3 sgrid((n_streams + 63) / 64), sblock(64);
  hipLaunchKernelGGL(frame_short_kernel, sgrid, sblock, 0, stream, f, false);
  size_t have = tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(tmp, have, f.count, f.count, (int)n_streams + 1, stream);
  if (e != hipSuccess) return fail(e, "tcp_frame scan");
  uint64_t total = 0;
  e = hipMemcpyAsync(&total, f.count + n_streams, 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(e, "tcp_frame sizes");
  if (cap) hipLaunchKernelGGL(frame_short_kernel, sgrid, sblock, 0, stream, f, true);
  std::vector<uint8_t> long_status(n_streams, 0);
  for (uint32_t s = 0; s < n_streams; s++) {
    if (hs[s].len < f.long_bytes) continue;
    const uint64_t at = total < cap ? total : cap;  // where this stream's records go
    mgenx_scan_info info;
    memset(&info, 0, sizeof(info));
    const int rc = mgenx::scan_run(scan_ws, dev_buf + hs[s].off, hs[s].len, MGENX_SCAN_TCP,
                                  f.t_off + at, f.t_len + at, cap - at, &info, stream, err, errn);
    if (rc != MGENX_OK) return rc;
    const uint64_t wrote = info.n_records < cap - at ? info.n_records : cap - at;
    if (wrote)
      hipLaunchKernelGGL(frame_long_fix_kernel, dim3((uint32_t)((wrote + 255) / 256)), dim3(256),
                         0, stream, f.t_off + at, f.t_stream + at, wrote, hs[s].off, s);
    long_status[s] = (uint8_t)info.status;
    e = hipMemcpyAsync(dev_stream_status + s, &long_status[s], 1, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return fail(e, "tcp_frame status");
    total += info.n_records;
  }
  *n_records = total;
  if (total && total <= cap) {
    const uint32_t n = (uint32_t)total;
    const dim3 grid((n + 255) / 256), block(256);
    hipLaunchKernelGGL(frame_key_kernel, grid, block, 0, stream, f, n, key_in, val_in);
    have = tmp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(tmp, have, key_in, key_out, val_in, val_out, (int)n, 0,
                                           64, stream);
    if (e != hipSuccess) return fail(e, "tcp_frame sort");
    hipLaunchKernelGGL(frame_out_kernel, grid, block, 0, stream, f, n, key_out, val_out,
                       dev_pkt_rx_sec, dev_pkt_rx_usec, dev_rec_off, dev_rec_len, dev_rec_stream,
                       dev_rec_pkt, dev_rec_src, dev_rec_rx_sec, dev_rec_rx_usec);
  }
  e = hipStreamSynchronize(stream);  // long_status is read by the copies above
  if (e == hipSuccess) e = hipGetLastError();
  return e == hipSuccess ? MGENX_OK : fail(e, "tcp_frame");
}

// ---- the C ABI of the TCP reassembly and framing steps ----
using mgenx::set_err;

extern "C" {

// both TCP reassemblies: dev_data_off null = classic records, else pcapng packet blocks
static int pcap_tcp_any(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off,
                        uint64_t buf_bytes, const uint64_t* dev_pkt_off,
                        const uint64_t* dev_data_off, const uint32_t* dev_cap_len, uint32_t n,
                        uint32_t link_type, uint32_t flags, uint8_t* dev_status,
                        mgenx_tcp_stream* dev_streams, uint32_t stream_cap,
                        uint64_t* dev_piece_end, uint32_t* dev_piece_pkt, mgenx_tcp_stats* stats,
                        void* stream) {
  if (!ctx || !stats || buf_bytes < scratch_off || n > 0x7FFFFFFEu) return MGENX_EINVAL;
  memset(stats, 0, sizeof(*stats));
  if (n == 0) return MGENX_OK;
  if (!dev_buf || !dev_pkt_off || !dev_status || (stream_cap && !dev_streams) ||
      !dev_piece_end || !dev_piece_pkt)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  void* m = ctx->ptcp.get(pcap_tcp_ws(n));
  if (!m) return set_err(ctx, hipErrorOutOfMemory, "pcap_tcp workspace");
  return pcap_tcp_run(m, dev_buf, scratch_off, buf_bytes, dev_pkt_off, dev_data_off,
                            dev_cap_len, n, link_type, flags, dev_status, dev_streams,
                            stream_cap, dev_piece_end, dev_piece_pkt, stats,
                            (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_pcap_tcp(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off, uint64_t buf_bytes,
                   const uint64_t* dev_pkt_off, uint32_t n, uint32_t link_type, uint32_t flags,
                   uint8_t* dev_status, mgenx_tcp_stream* dev_streams, uint32_t stream_cap,
                   uint64_t* dev_piece_end, uint32_t* dev_piece_pkt, mgenx_tcp_stats* stats,
                   void* stream) {
  return pcap_tcp_any(ctx, dev_buf, scratch_off, buf_bytes, dev_pkt_off, nullptr, nullptr, n,
                      link_type, flags, dev_status, dev_streams, stream_cap, dev_piece_end,
                      dev_piece_pkt, stats, stream);
}

int mgenx_pcapng_tcp(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off, uint64_t buf_bytes,
                     const uint64_t* dev_pkt_off, const uint64_t* dev_data_off,
                     const uint32_t* dev_cap_len, uint32_t n, uint32_t link_type, uint32_t flags,
                     uint8_t* dev_status, mgenx_tcp_stream* dev_streams, uint32_t stream_cap,
                     uint64_t* dev_piece_end, uint32_t* dev_piece_pkt, mgenx_tcp_stats* stats,
                     void* stream) {
  if (n && (!dev_data_off || !dev_cap_len)) return MGENX_EINVAL;
  return pcap_tcp_any(ctx, dev_buf, scratch_off, buf_bytes, dev_pkt_off, dev_data_off,
                      dev_cap_len, n, link_type, flags, dev_status, dev_streams, stream_cap,
                      dev_piece_end, dev_piece_pkt, stats, stream);
}

int mgenx_tcp_frame(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                    const mgenx_tcp_stream* dev_streams, uint32_t n_streams,
                    const uint64_t* dev_piece_end, const uint32_t* dev_piece_pkt,
                    uint32_t n_pieces, const uint32_t* dev_pkt_rx_sec,
                    const uint32_t* dev_pkt_rx_usec, uint64_t long_bytes, uint64_t* dev_rec_off,
                    uint32_t* dev_rec_len, uint32_t* dev_rec_stream, uint32_t* dev_rec_pkt,
                    mgenx_addr* dev_rec_src, uint32_t* dev_rec_rx_sec, uint32_t* dev_rec_rx_usec,
                    uint64_t cap, uint8_t* dev_stream_status, uint64_t* n_records, void* stream) {
  if (!ctx || !n_records || n_streams > 0x7FFFFFFEu || cap > 0x7FFFFFFEu) return MGENX_EINVAL;
  *n_records = 0;
  if (n_streams == 0) return MGENX_OK;
  if (!dev_buf || !dev_streams || !dev_stream_status || (n_pieces && (!dev_piece_end ||
      !dev_piece_pkt)) || !dev_pkt_rx_sec || !dev_pkt_rx_usec ||
      (cap && (!dev_rec_off || !dev_rec_len || !dev_rec_stream || !dev_rec_pkt || !dev_rec_src ||
               !dev_rec_rx_sec || !dev_rec_rx_usec)))
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->scan_ws) ctx->scan_ws = mgenx::scan_ws_new();
  void* m = ctx->tcpf.get(tcp_frame_ws(n_streams, cap));
  if (!m) return set_err(ctx, hipErrorOutOfMemory, "tcp_frame workspace");
  return tcp_frame_run(m, ctx->scan_ws, dev_buf, buf_bytes, dev_streams, n_streams, dev_piece_end,
                             dev_piece_pkt, n_pieces, dev_pkt_rx_sec, dev_pkt_rx_usec, long_bytes,
                             dev_rec_off, dev_rec_len, dev_rec_stream, dev_rec_pkt, dev_rec_src,
                             dev_rec_rx_sec, dev_rec_rx_usec, cap, dev_stream_status, n_records,
                             (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

}  // extern "C"
