// mgenx_logparse.hip -- text log ingest: MGEN text log lines -> columns.
//
//   mgenx_text_index       LF positions -> line offsets (count per tile, hipcub scan, write)
//   mgenx_log_parse_text   a workgroup takes a run of consecutive lines, stages their
//                          contiguous bytes into LDS with 16-byte loads, then each lane parses
//                          one line from LDS with the scalar parser of mgenx_logparse.hpp; a
//                          run that outgrows the staging budget is split, and a line longer
//                          than the budget is parsed from global memory by its lane.  Then
//                          the day reconstruction of legacy stamps (a hipcub prefix scan of
//                          (first tod, last tod, wraps, has)) and the data> hex decode.
// No kernel here waits on another workgroup.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <stdio.h>

#include "mgenx_internal.hpp"
#include "mgenx_logparse.hpp"

namespace mgenx {

// ---------------------------------------------------------------- line index
constexpr int kIdxThreads = 256;
constexpr int kIdxChunks = 4;                                   // 16-byte chunks per thread
constexpr uint64_t kIdxTile = (uint64_t)kIdxThreads * 16 * kIdxChunks;  // bytes per workgroup

// bit 8j+7 set for every byte j of w that is '\n' (exact: no borrow between bytes)
__device__ __forceinline__ uint32_t lf_mask(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  const uint32_t y = ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x;
  return ~y & 0x80808080u;
}

// the LF bytes of text[pos, pos + 16) as a 16-bit mask (bytes past nbytes are not read)
__device__ __forceinline__ uint32_t lf_mask16(const uint8_t* text, uint64_t pos, uint64_t nbytes) {
  if (pos >= nbytes) return 0;
  uint32_t m = 0;
  if (pos + 16 <= nbytes) {
    const u32x4_t v = ldu128(text + pos);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t b = lf_mask(w[k]);
      m |= (((b >> 7) & 1u) | ((b >> 14) & 2u) | ((b >> 21) & 4u) | ((b >> 28) & 8u)) << (4 * k);
    }
  } else {
    for (uint32_t j = 0; pos + j < nbytes; j++) m |= (uint32_t)(text[pos + j] == '\n') << j;
  }
  return m;
}

__global__ void __launch_bounds__(kIdxThreads)
text_index_count_kernel(const uint8_t* __restrict__ text, uint64_t nbytes, uint64_t* counts,
                        uint32_t n_tiles) {
  typedef hipcub::BlockReduce<uint32_t, kIdxThreads> Reduce;
  __shared__ typename Reduce::TempStorage tmp;
  const uint64_t start = (uint64_t)blockIdx.x * kIdxTile;
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < kIdxChunks; k++)
    c += __popc(lf_mask16(text, start + ((uint64_t)k * kIdxThreads + threadIdx.x) * 16, nbytes));
  const uint32_t sum = Reduce(tmp).Sum(c);
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = sum;
    if (blockIdx.x == 0) counts[n_tiles] = 0;
  }
}

// counts: the exclusive scan (n_tiles + 1 entries; the last one = the number of LFs)
__global__ void __launch_bounds__(kIdxThreads)
text_index_write_kernel(const uint8_t* __restrict__ text, uint64_t nbytes,
                        const uint64_t* __restrict__ counts, uint32_t n_tiles, uint64_t* line_off,
                        uint64_t cap, uint64_t* n_lines_out) {
  typedef hipcub::BlockScan<uint32_t, kIdxThreads> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const uint64_t lfs = counts[n_tiles];
  const bool open_tail = nbytes > 0 && text[nbytes - 1] != '\n';
  const uint64_t n_lines = lfs + (open_tail ? 1u : 0u);
  if (blockIdx.x == 0 && threadIdx.x == 0) n_lines_out[0] = n_lines;
  if (n_lines > cap || !line_off) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    line_off[0] = 0;
    line_off[n_lines] = nbytes;
  }
  const uint64_t start = (uint64_t)blockIdx.x * kIdxTile;
  uint64_t at = counts[blockIdx.x] + 1;  // line_off slot of this tile's next LF
  for (int k = 0; k < kIdxChunks; k++) {
    const uint64_t pos = start + ((uint64_t)k * kIdxThreads + threadIdx.x) * 16;
    uint32_t m = lf_mask16(text, pos, nbytes);
    uint32_t before, total;
    Scan(tmp).ExclusiveSum((uint32_t)__popc(m), before, total);
    uint64_t slot = at + before;
    while (m) {
      const uint32_t j = (uint32_t)__ffs((int)m) - 1u;
      m &= m - 1u;
      if (slot <= n_lines) line_off[slot] = pos + j + 1;
      slot++;
    }
    at += total;
    __syncthreads();  // the scan's storage is reused by the next chunk
  }
}

__global__ void text_index_empty_kernel(uint64_t* line_off, uint64_t* n_lines_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    n_lines_out[0] = 0;
    if (line_off) line_off[0] = 0;
  }
}

// ---------------------------------------------------------------- per-line parse
constexpr int kParseThreads = 256;
constexpr uint32_t kStageBytes = 40960;  // LDS staging budget of one run of lines

// the day scan's element over OK lines with a legacy stamp: (first tod, last tod, wraps, has)
struct DayElem {
  uint32_t first, last, wraps, has;
};
struct DayOp {
  __host__ __device__ __forceinline__ DayElem operator()(const DayElem& a, const DayElem& b) const {
    if (!a.has) return b;
    if (!b.has) return a;
    DayElem r;
    r.first = a.first;
    r.last = b.last;
    r.wraps = a.wraps + b.wraps + ((int32_t)a.last - (int32_t)b.first > 43200 ? 1u : 0u);
    r.has = 1;
    return r;
  }
};

struct ParseParams {
  const uint8_t* text;
  uint64_t nbytes;
  const uint64_t* line_off;
  uint32_t n;
  uint32_t opts;
  uint32_t day_base;
  mgenx_logparse_out out;
  // workspace, one element per line
  DayElem* elem;
  uint32_t* rxs;
  uint32_t* rxu;
  uint8_t* kind;
  uint64_t* pay_len;  // n + 1 (NULL without payload_off)
  uint64_t* pay_pos;
};

__device__ void store_line(const ParseParams& p, uint32_t k, const lp::Line& r, uint64_t line_at) {
  const mgenx_logparse_out& o = p.out;
  const mgenx_cols& c = o.cols;
  const bool ok = r.status == MGENX_PARSE_OK;
  o.event[k] = r.event;
  o.status[k] = r.status;
  if (o.protocol) o.protocol[k] = r.protocol;
  if (o.present) o.present[k] = r.present;
  if (o.rx_sec) o.rx_sec[k] = r.rx_sec;
  if (o.rx_usec) o.rx_usec[k] = r.rx_usec;
  if (o.src) o.src[k] = r.src;
  if (o.ttl) o.ttl[k] = r.ttl;
  if (o.size) o.size[k] = r.size;
  uint8_t err = MGENX_ERROR_NOT_RECV;
  if (ok && r.event == MGENX_EVENT_RECV) err = 0;
  else if (ok && r.event == MGENX_EVENT_RERR) err = r.rerr;
  if (c.flow_id) c.flow_id[k] = r.flow;
  if (c.seq_num) c.seq_num[k] = r.seq;
  if (c.tx_sec) c.tx_sec[k] = r.tx_sec;
  if (c.tx_usec) c.tx_usec[k] = r.tx_usec;
  if (c.msg_len) c.msg_len[k] = (uint16_t)(r.size < 65535u ? r.size : 65535u);
  if (c.dst_port) c.dst_port[k] = r.dst.port;
  if (c.flags) c.flags[k] = r.flags;
  if (c.err) c.err[k] = err;
  if (c.dst_type) c.dst_type[k] = r.dst.type;
  if (c.dst_len) c.dst_len[k] = r.dst.len;
  if (c.dst_addr4)
    c.dst_addr4[k] = (uint32_t)r.dst.addr[0] | (uint32_t)r.dst.addr[1] << 8 |
                     (uint32_t)r.dst.addr[2] << 16 | (uint32_t)r.dst.addr[3] << 24;
  if (c.payload_len) c.payload_len[k] = (uint16_t)r.data_len;
  if (c.payload_type) c.payload_type[k] = 0;
  if (c.gps_status) c.gps_status[k] = r.gps_status;
  if (c.lat_raw) c.lat_raw[k] = r.lat_raw;
  if (c.lon_raw) c.lon_raw[k] = r.lon_raw;
  if (c.alt) c.alt[k] = r.alt;
  if (c.host_port) c.host_port[k] = r.host.port;
  if (c.host_type) c.host_type[k] = r.host.type;
  if (c.host_len) c.host_len[k] = r.host.len;
  if (c.host_addr) {
    for (int j = 0; j < 16; j++) c.host_addr[(size_t)k * 16 + j] = r.host.addr[j];
  }
  if (c.dst_addr) {
    for (int j = 0; j < 16; j++) c.dst_addr[(size_t)k * 16 + j] = r.dst.addr[j];
  }
  DayElem e;
  e.first = e.last = r.rx_sec;
  e.wraps = 0;
  e.has = ok && (r.ts_kind & lp::kRxLegacy) ? 1u : 0u;
  p.elem[k] = e;
  p.rxs[k] = r.rx_sec;
  p.rxu[k] = r.rx_usec;
  p.kind[k] = ok ? r.ts_kind : (uint8_t)0;
  if (p.pay_len) {
    const bool data = ok && (r.present & MGENX_HAS_DATA);
    p.pay_len[k] = data ? r.data_len : 0u;
    p.pay_pos[k] = line_at + r.data_pos;
    if (k == 0) p.pay_len[p.n] = 0;
  }
}

__global__ void __launch_bounds__(kParseThreads) log_parse_kernel(ParseParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t buf[kStageBytes];
  __shared__ uint32_t s_m, s_span;
  const uint32_t t = threadIdx.x;
  const uint32_t first = blockIdx.x * (uint32_t)kParseThreads;
  const uint32_t last = p.n - first < (uint32_t)kParseThreads ? p.n : first + kParseThreads;
  uint32_t lo = first;
  while (lo < last) {  // uniform over the workgroup
    const uint32_t cnt = last - lo;
    const uint64_t base = p.line_off[lo];
    const uint32_t k = lo + t;
    const bool mine = t < cnt;
    uint64_t b = 0, e = 0;
    if (mine) {
      b = p.line_off[k];
      e = p.line_off[k + 1];
    }
    // a line whose offsets are not a range inside the text is not read (malformed)
    const bool valid = mine && b <= e && e <= p.nbytes;
    // lanes 0 .. m-1 take part in this run: their lines lie inside the staged bytes
    const bool in_run = mine && (!valid || (b >= base && e - base <= kStageBytes));
    if (t == 0) {
      s_m = cnt;
      s_span = 0;
    }
    __syncthreads();
    if (mine && !in_run) atomicMin(&s_m, t);
    __syncthreads();
    const uint32_t m = s_m;
    if (valid && t < m) atomicMax(&s_span, (uint32_t)(e - base));
    __syncthreads();
    const uint32_t span = s_span;
    const uint8_t* ptr = nullptr;
    bool work;
    uint32_t adv;
    if (m == 0) {  // line lo alone outgrows the budget: its lane reads global memory
      work = t == 0;
      ptr = p.text + b;
      adv = 1;
    } else {
      const uint8_t* src = p.text + base;
      const uint32_t whole = span & ~15u;
      for (uint32_t o = t * 16u; o < whole; o += kParseThreads * 16u)
        *reinterpret_cast<u32x4_t*>(buf + o) = ldu128(src + o);
      if (t < span - whole) buf[whole + t] = src[whole + t];
      __syncthreads();
      work = t < m;
      ptr = buf + (valid ? (uint32_t)(b - base) : 0u);
      adv = m;
    }
    if (work) {
      lp::Line r;
      if (valid) lp::parse_line(ptr, (size_t)(e - b), &r);
      else lp::line_init(&r);
      store_line(p, k, r, b);
    }
    __syncthreads();  // the staged bytes are overwritten by the next run
    lo += adv;
  }
}

// legacy stamps -> epoch seconds (elem: the inclusive day scan)
__global__ void __launch_bounds__(256) log_days_kernel(ParseParams p) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= p.n) return;
  const uint8_t kind = p.kind[k];  // 0 for lines that are not OK
  if (!kind) return;
  int64_t rx = p.rxs[k];
  int64_t rx_tod = rx % 86400;
  if (kind & lp::kRxLegacy) {
    rx_tod = rx;
    rx = (int64_t)p.day_base + 86400ll * (int64_t)p.elem[k].wraps + rx;
    if (p.out.rx_sec) p.out.rx_sec[k] = (uint32_t)rx;
  }
  const mgenx_cols& c = p.out.cols;
  if ((kind & lp::kTxLegacy) && c.tx_sec) {
    const int64_t day0 = rx - rx_tod;
    const int64_t rx_us = rx * 1000000ll + p.rxu[k];
    const int64_t tod = c.tx_sec[k];
    const int64_t tu = c.tx_usec ? (int64_t)c.tx_usec[k] : 0;
    int64_t best = 0, best_d = -1;
    for (int d = -1; d <= 1; d++) {  // earlier day first: it wins a tie
      const int64_t tx = day0 + 86400ll * d + tod;
      int64_t diff = tx * 1000000ll + tu - rx_us;
      if (diff < 0) diff = -diff;
      if (best_d < 0 || diff < best_d) {
        best_d = diff;
        best = tx;
      }
    }
    c.tx_sec[k] = (uint32_t)best;
  }
}

// data> hex -> bytes, a wave per line
__global__ void __launch_bounds__(256) log_payload_kernel(ParseParams p) {
  const uint32_t k = blockIdx.x * 4u + threadIdx.x / 64u;
  if (k >= p.n) return;
  const uint64_t len = p.pay_len[k];
  const uint64_t* off = p.out.payload_off;
  if (!len || off[p.n] > p.out.payload_cap) return;
  const uint8_t* src = p.text + p.pay_pos[k];
  uint8_t* dst = p.out.payload + off[k];
  for (uint64_t j = threadIdx.x % 64u; j < len; j += 64)
    dst[j] = (uint8_t)(lp::hex_val(src[2 * j]) << 4 | lp::hex_val(src[2 * j + 1]));
}

}  // namespace mgenx

using namespace mgenx;

size_t mgenx::text_index_ws(uint64_t nbytes) {
  const uint64_t n_tiles = (nbytes + kIdxTile - 1) / kIdxTile;
  size_t scan_bytes = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint64_t*)nullptr,
                                         (uint64_t*)nullptr, (int)n_tiles + 1, nullptr);
  return a256((n_tiles + 1) * 8) + scan_bytes;
}

int mgenx::text_index_run(void* ws, const uint8_t* text, uint64_t nbytes, uint64_t* line_off,
                          uint64_t cap, uint64_t* n_lines, hipStream_t stream, char* err,
                          size_t errn) {
  if (nbytes == 0) {
    hipLaunchKernelGGL(text_index_empty_kernel, dim3(1), dim3(64), 0, stream, line_off, n_lines);
  } else {
    const uint32_t n_tiles = (uint32_t)((nbytes + kIdxTile - 1) / kIdxTile);
    uint64_t* counts = static_cast<uint64_t*>(ws);
    const size_t cnt_bytes = a256(((size_t)n_tiles + 1) * 8);
    size_t scan_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint64_t*)nullptr,
                                           (uint64_t*)nullptr, (int)n_tiles + 1, stream);
    hipLaunchKernelGGL(text_index_count_kernel, dim3(n_tiles), dim3(kIdxThreads), 0, stream, text,
                       nbytes, counts, n_tiles);
    if (hipcub::DeviceScan::ExclusiveSum(static_cast<uint8_t*>(ws) + cnt_bytes, scan_bytes, counts,
                                         counts, (int)n_tiles + 1, stream) != hipSuccess) {
      snprintf(err, errn, "text_index: scan failed");
      return MGENX_EDEVICE;
    }
    hipLaunchKernelGGL(text_index_write_kernel, dim3(n_tiles), dim3(kIdxThreads), 0, stream, text,
                       nbytes, counts, n_tiles, line_off, cap, n_lines);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "text_index: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  return MGENX_OK;
}

static void parse_scan_bytes(uint32_t n, size_t* day, size_t* pay) {
  *day = *pay = 0;
  (void)hipcub::DeviceScan::InclusiveScan(nullptr, *day, (DayElem*)nullptr, (DayElem*)nullptr,
                                          DayOp(), (int)n, nullptr);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, *pay, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (int)n + 1, nullptr);
}

size_t mgenx::log_parse_ws(uint32_t n) {
  size_t day, pay;
  parse_scan_bytes(n, &day, &pay);
  return a256((size_t)n * 16) + 2 * a256((size_t)n * 4) + a256(n) +
         2 * a256(((size_t)n + 1) * 8) + a256(day > pay ? day : pay);
}

int mgenx::log_parse_run(void* ws, const uint8_t* text, uint64_t nbytes, const uint64_t* line_off,
                         uint32_t n, uint32_t opts, uint32_t day_base,
                         const mgenx_logparse_out* out, hipStream_t stream, char* err,
                         size_t errn) {
  ParseParams p;
  p.text = text; p.nbytes = nbytes; p.line_off = line_off; p.n = n; p.opts = opts;
  p.day_base = day_base; p.out = *out;
  uint8_t* w = static_cast<uint8_t*>(ws);
  p.elem = reinterpret_cast<DayElem*>(w); w += a256((size_t)n * 16);
  p.rxs = reinterpret_cast<uint32_t*>(w); w += a256((size_t)n * 4);
  p.rxu = reinterpret_cast<uint32_t*>(w); w += a256((size_t)n * 4);
  p.kind = w; w += a256(n);
  uint64_t* pay_len = reinterpret_cast<uint64_t*>(w); w += a256(((size_t)n + 1) * 8);
  p.pay_pos = reinterpret_cast<uint64_t*>(w); w += a256(((size_t)n + 1) * 8);
  p.pay_len = out->payload_off ? pay_len : nullptr;
  size_t day_bytes, pay_bytes;
  parse_scan_bytes(n, &day_bytes, &pay_bytes);
  const uint32_t grid = (n + kParseThreads - 1) / kParseThreads;
  hipLaunchKernelGGL(log_parse_kernel, dim3(grid), dim3(kParseThreads), 0, stream, p);
  if (!(opts & MGENX_PARSE_NO_DAYS)) {
    if (hipcub::DeviceScan::InclusiveScan(w, day_bytes, p.elem, p.elem, DayOp(), (int)n, stream) !=
        hipSuccess) {
      snprintf(err, errn, "log_parse: day scan failed");
      return MGENX_EDEVICE;
    }
    hipLaunchKernelGGL(log_days_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p);
  }
  if (p.pay_len) {
    if (hipcub::DeviceScan::ExclusiveSum(w, pay_bytes, p.pay_len, out->payload_off, (int)n + 1,
                                         stream) != hipSuccess) {
      snprintf(err, errn, "log_parse: payload scan failed");
      return MGENX_EDEVICE;
    }
    if (out->payload)
      hipLaunchKernelGGL(log_payload_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, p);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(err, errn, "log_parse: %s", hipGetErrorString(e));
    return MGENX_EDEVICE;
  }
  return MGENX_OK;
}
