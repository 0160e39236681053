// mgenx_binlogparse.hip -- binary log ingest: MGEN binary log records -> the columns of
// mgenx_logparse_out, in one pass over each record's leading bytes.
//
//   mgenx_binlog_header   the header-line rules of mgenx_binlog_index alone (host)
//   mgenx_binlog_parse    a workgroup takes 256 consecutive records.  Eight lanes per record
//                         load its first 128 bytes (the 4-byte header, at most 28 bytes of RECV
//                         prefix, at most 76 bytes of message header) with 16-byte loads into a
//                         record slot in LDS; the slots are 33 words apart, so the 64 lanes of a
//                         wave that then decode one record each (mgenx_binlogparse.hpp) read 64
//                         different banks.  A field past the staged bytes (only a message whose
//                         unknown host type carries a length) is read from global memory.  The
//                         data> bytes are copied by a second kernel after a hipcub scan of their
//                         lengths, a wave per record.
// No read leaves a record or the buffer; no kernel here waits on another workgroup.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <stdio.h>
#include <string.h>

#include "mgenx_internal.hpp"
#include "mgenx_binlogparse.hpp"

namespace mgenx {

constexpr int kBpThreads = 256;
constexpr uint32_t kBpSlotWords = bp::kLead / 4 + 1;  // 33: odd, so slots rotate over the banks
constexpr uint32_t kBpLanesPerRec = bp::kLead / 16;   // 8
constexpr uint32_t kBpRecsPerStep = kBpThreads / kBpLanesPerRec;  // 32

struct BinParseParams {
  const uint8_t* buf;
  uint64_t nbytes;
  const uint64_t* rec_off;
  uint32_t n;
  mgenx_logparse_out out;
  uint64_t* pay_len;  // n + 1 (NULL without payload_off)
  uint64_t* pay_pos;  // n
};

__device__ void store_rec(const BinParseParams& p, uint32_t k, const bp::Rec& r, uint64_t rec_at) {
  const mgenx_logparse_out& o = p.out;
  const mgenx_cols& c = o.cols;
  o.event[k] = r.event;
  o.status[k] = r.status;
  if (o.protocol) o.protocol[k] = r.protocol;
  if (o.present) o.present[k] = r.present;
  if (o.rx_sec) o.rx_sec[k] = r.rx_sec;
  if (o.rx_usec) o.rx_usec[k] = r.rx_usec;
  if (o.src) o.src[k] = r.src;
  if (o.ttl) o.ttl[k] = r.ttl;
  if (o.size) o.size[k] = r.size;
  if (c.flow_id) c.flow_id[k] = r.flow;
  if (c.seq_num) c.seq_num[k] = r.seq;
  if (c.tx_sec) c.tx_sec[k] = r.tx_sec;
  if (c.tx_usec) c.tx_usec[k] = r.tx_usec;
  if (c.msg_len) c.msg_len[k] = (uint16_t)(r.size < 65535u ? r.size : 65535u);
  if (c.dst_port) c.dst_port[k] = r.dst.port;
  if (c.flags) c.flags[k] = r.flags;
  if (c.err) c.err[k] = r.err;
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
  if (p.pay_len) {
    p.pay_len[k] = r.data_len;
    p.pay_pos[k] = rec_at + r.data_pos;
    if (k == 0) p.pay_len[p.n] = 0;
  }
}

__global__ void __launch_bounds__(kBpThreads) binlog_ingest_kernel(BinParseParams p) {
  __shared__ uint32_t lead[kBpThreads * kBpSlotWords];
  __shared__ uint32_t s_len[kBpThreads];  // bytes of the record that lie inside the buffer
  const uint32_t t = threadIdx.x;
  const uint32_t first = blockIdx.x * (uint32_t)kBpThreads;
  // stage: lane (t % 8) of record slot (step * 32 + t / 8) loads chunk [16 c, 16 c + 16)
  const uint32_t c = t % kBpLanesPerRec;
#pragma unroll 2
  for (uint32_t step = 0; step < kBpThreads / kBpRecsPerStep; step++) {
    const uint32_t slot = step * kBpRecsPerStep + t / kBpLanesPerRec;
    const uint32_t k = first + slot;
    uint32_t len = 0;
    const uint8_t* rec = p.buf;
    if (k < p.n) {
      const uint64_t at = p.rec_off[k];
      if (at < p.nbytes && p.nbytes - at >= 4) {  // the header lies inside the buffer
        rec = p.buf + at;
        const uint64_t avail = p.nbytes - at;
        const uint32_t h = ldu32(rec);  // {type, protocol, BE recordLength}
        const uint32_t rl = (h >> 8 & 0xFF00u) | h >> 24;
        len = (uint32_t)(4ull + rl < avail ? 4ull + rl : avail);
      }
    }
    uint32_t* dst = lead + slot * kBpSlotWords + c * 4u;
    const uint32_t o = c * 16u;
    if (o + 16u <= len) {
      const u32x4_t v = ldu128(rec + o);
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    } else if (o < len) {  // the record's last, partial chunk: byte by byte
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t j = o; j < len; j++) w[(j - o) >> 2] |= (uint32_t)rec[j] << (8u * (j & 3u));
      dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2]; dst[3] = w[3];
    }
    if (c == 0) s_len[slot] = len;
  }
  __syncthreads();
  const uint32_t k = first + t;
  if (k >= p.n) return;
  const uint64_t at = p.rec_off[k];
  bp::View v;
  v.lead = reinterpret_cast<const uint8_t*>(lead + t * kBpSlotWords);
  v.len = s_len[t];
  v.n_lead = v.len < bp::kLead ? v.len : bp::kLead;
  v.rec = v.len ? p.buf + at : p.buf;
  bp::Rec r;
  bp::decode_record(v, &r);
  store_rec(p, k, r, at);
}

// the data> bytes, a wave per record
__global__ void __launch_bounds__(256) binlog_payload_kernel(BinParseParams p) {
  const uint32_t k = blockIdx.x * 4u + threadIdx.x / 64u;
  if (k >= p.n) return;
  const uint64_t len = p.pay_len[k];
  const uint64_t* off = p.out.payload_off;
  if (!len || off[p.n] > p.out.payload_cap) return;
  const uint8_t* src = p.buf + p.pay_pos[k];
  uint8_t* dst = p.out.payload + off[k];
  for (uint64_t j = threadIdx.x % 64u; j < len; j += 64) dst[j] = src[j];
}

static size_t binlog_parse_scan_bytes(uint32_t n) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                         (int)n + 1, nullptr);
  return b;
}

}  // namespace mgenx

using namespace mgenx;

extern "C" {

int mgenx_binlog_header(const uint8_t* buf, uint64_t nbytes, mgenx_binlog_info* info) {
  if (!buf || !info) return MGENX_EINVAL;
  memset(info, 0, sizeof(*info));
  info->status = MGENX_BINLOG_HEADER;
  // "mgen ... version=<4|5> ... type=binary_log\n" and its NUL (mgenMsg.cpp:1437-1518)
  if (nbytes < 4 || memcmp(buf, "mgen", 4) != 0) return MGENX_OK;
  char hdr[1024];
  uint64_t k = 3;
  memcpy(hdr, buf, 4);
  while (hdr[k] != '\0') {
    if (++k >= sizeof(hdr) || k >= nbytes) return MGENX_OK;
    hdr[k] = (char)buf[k];
  }
  const char* v = strstr(hdr, "version=");
  int version = 0;
  if (!v || 1 != sscanf(v, "version=%d", &version) || (version != 4 && version != 5))
    return MGENX_OK;
  const char* t = strstr(v, "type=");
  char ftype[128];
  if (!t || 1 != sscanf(t, "type=%127s", ftype) || strcmp(ftype, "binary_log")) return MGENX_OK;
  info->version = (uint32_t)version;
  info->status = MGENX_BINLOG_OK;
  info->consumed = k + 1;
  return MGENX_OK;
}

int mgenx_binlog_parse(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                       const uint64_t* dev_rec_off, uint32_t n, uint32_t opts,
                       const mgenx_logparse_out* out, void* stream) {
  if (!ctx || !out || !out->event || !out->status || (n && (!dev_rec_off || !dev_buf)) ||
      (out->payload_cap && !out->payload) || (out->payload && !out->payload_off) || opts ||
      n > 0x7FFFFFFEu)
    return MGENX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipSetDevice(ctx->device);
  if (n == 0) {
    if (out->payload_off && hipMemsetAsync(out->payload_off, 0, 8, s) != hipSuccess)
      return set_err(ctx, hipGetLastError(), "binlog_parse");
    return MGENX_OK;
  }
  BinParseParams p;
  p.buf = dev_buf; p.nbytes = buf_bytes; p.rec_off = dev_rec_off; p.n = n; p.out = *out;
  p.pay_len = p.pay_pos = nullptr;
  size_t scan_bytes = 0;
  uint8_t* scan_ws = nullptr;
  if (out->payload_off) {
    scan_bytes = binlog_parse_scan_bytes(n);
    const size_t a8 = a256(((size_t)n + 1) * 8);
    uint8_t* w = static_cast<uint8_t*>(ctx->lp.get(2 * a8 + a256(scan_bytes)));
    if (!w) return set_err(ctx, hipErrorOutOfMemory, "binlog_parse workspace");
    p.pay_len = reinterpret_cast<uint64_t*>(w);
    p.pay_pos = reinterpret_cast<uint64_t*>(w + a8);
    scan_ws = w + 2 * a8;
  }
  hipLaunchKernelGGL(binlog_ingest_kernel, dim3((n + kBpThreads - 1) / kBpThreads),
                     dim3(kBpThreads), 0, s, p);
  if (p.pay_len) {
    if (hipcub::DeviceScan::ExclusiveSum(scan_ws, scan_bytes, p.pay_len, out->payload_off,
                                         (int)n + 1, s) != hipSuccess) {
      snprintf(ctx->err, sizeof(ctx->err), "binlog_parse: payload scan failed");
      return MGENX_EDEVICE;
    }
    if (out->payload)
      hipLaunchKernelGGL(binlog_payload_kernel, dim3((n + 3) / 4), dim3(256), 0, s, p);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(ctx, e, "binlog_parse");
  return MGENX_OK;
}

}  // extern "C"
