// mgenx_api.hip -- C ABI (include/mgenx.h) over the gfx950 kernels: argument checks,
// hipSetDevice and one call into a module.
//
// The context (mgenx_ctx.hip) owns only constant tables; every data buffer belongs to the
// caller.  No entry point allocates, synchronises or copies from host memory except
// mgenx_ctx_create, mgenx_set_fill_time and mgenx_pack_prepare (table setup) and a call that
// outgrows its workspace (mgenx::DevBuf), so batch calls can be captured in a hipGraph.
// The other entry points sit with the code they drive: the worker in mgenx_worker_host.hip,
// mgenx_pack_tcp in mgenx_tcp.hip, the capture steps in mgenx_pcap.hip, mgenx_defrag.hip and
// mgenx_pcap_tcp.hip, ConvertBinaryLog in mgenx_binlog.hip, the flow table in mgenx_flowtab.hip,
// the collectives in mgenx_comm.hip.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "mgenx_flowdist.hpp"
#include "mgenx_internal.hpp"
#if MGENX_DIAG
#include "mgenx_diag.h"
#endif

using mgenx::set_err;

// Pack for mgenx_pack_batch, mgenx_pack_msgs and the rounds of mgenx_pack_tcp (mgenx_tcp.hip)
int mgenx::pack_common(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                       const uint32_t* dev_tmpl_crc, const mgenx_pack_desc* dev_desc, uint32_t n,
                       const uint8_t* dev_pool, uint8_t* dev_slab, uint64_t slab_bytes,
                       const uint64_t* dev_rec_off, uint64_t stride, const uint32_t* dev_buf_len,
                       const uint32_t* dev_crc_in, uint32_t* dev_out_len, uint32_t* dev_tx_crc,
                       uint32_t* dev_state, uint32_t opts, uint32_t fill_time, void* stream,
                       const uint32_t* dev_frag_len, int frag_ck, const uint32_t* dev_skip) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_tmpl || !dev_tmpl_crc || !dev_desc || !dev_slab || !dev_out_len) return MGENX_EINVAL;
  if (!dev_rec_off && stride == 0 && n > 1) return MGENX_EINVAL;
  if (opts & MGENX_PACK_RANDOM_FILL) {
    if (!ctx->rand_ready || ctx->rand_time != fill_time) return MGENX_EINVAL;
  }
  mgenx::PackParams p;
  p.tmpl = dev_tmpl;
  p.tmpl_crc = dev_tmpl_crc;
  p.desc = dev_desc;
  p.n = n;
  p.pool = dev_pool;
  p.slab = dev_slab;
  p.slab_bytes = slab_bytes;
  p.rec_off = dev_rec_off;
  p.stride = stride;
  p.out_len = dev_out_len;
  p.opts = opts;
  p.byte_tab = ctx->d_bytetab;
  p.a4_tab = ctx->d_tabs + 1024;  // [A_64 | A_4 | ...]
  p.variant = MGENX_DIAG ? ctx->pack_variant : 0;
  p.xpow = ctx->d_xpow;
  p.ia = ctx->d_ia;
  p.rtab = ctx->d_rtab;
  p.rcrc = ctx->d_rcrc;
  p.buf_len = dev_buf_len;
  p.crc_in = dev_crc_in;
  p.tx_crc = dev_tx_crc;
  p.state = dev_state;
  p.frag_len = dev_frag_len;
  p.frag_ck = frag_ck;
  p.skip = dev_skip;
  const uint64_t batches = ((uint64_t)n + 63) / 64;
  uint64_t grid = (batches + 3) / 4;                // groups of 4 batches (kProd)
  // 76 KB of LDS per workgroup: two per CU, except for the aligned-stride layout (the
  // recvmmsg slots, config 2), whose joint 4-KB-chunk store runs faster with one workgroup --
  // eight waves -- per CU (config 2: 0.199 against 0.211 ms; config 3's packed slab the other
  // way: 0.214 against 0.188 ms)
  const bool stride_layout = !dev_rec_off && !dev_frag_len && !(opts & MGENX_PACK_RANDOM_FILL) &&
                             (stride & 15u) == 0 && stride >= 32 && stride <= 65536;
  uint64_t cap = (uint64_t)ctx->cu_count * (stride_layout ? 1u : 2u);
  if (MGENX_DIAG && ctx->pack_variant >= 7 && ctx->pack_variant <= 9)
    cap *= (uint64_t)(ctx->pack_variant - 5);  // (diag)
#if MGENX_DIAG
  if (const char* v = getenv("MGENX_PACK_GRID")) cap = (uint64_t)std::max(1, atoi(v));  // (diag)
#endif
  if (grid > cap) grid = cap;
  hipError_t e = mgenx::launch_pack(p, (int)grid, (hipStream_t)stream);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "pack");
}

extern "C" {

int mgenx_abi_version(void) { return MGENX_ABI_VERSION; }

int mgenx_unpack_batch(mgenx_ctx* ctx, const uint8_t* dev_slab, uint64_t slab_bytes,
                       const uint64_t* dev_rec_off, uint64_t stride,
                       const uint32_t* dev_rec_len, uint32_t fixed_len, uint32_t n,
                       const mgenx_cols* cols, uint32_t opts, void* stream) {
  if (!ctx || !cols) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_slab) return MGENX_EINVAL;
  if (!dev_rec_off && stride == 0 && n > 1) return MGENX_EINVAL;
  const mgenx_cols& k = *cols;
  if (!k.rows && (!k.flow_id || !k.seq_num || !k.tx_sec || !k.tx_usec || !k.msg_len ||
                  !k.dst_port || !k.flags || !k.err || !k.dst_type || !k.dst_len ||
                  !k.dst_addr4 || !k.payload_len || !k.payload_type || !k.gps_status))
    return MGENX_EINVAL;
  mgenx::UnpackParams p;
  p.slab = dev_slab;
  p.slab_bytes = slab_bytes;
  p.rec_off = dev_rec_off;
  p.stride = stride;
  p.rec_len = dev_rec_len;
  p.fixed_len = fixed_len;
  p.n = n;
  p.opts = opts;
  p.tabs = ctx->d_tabs;
  p.expect = ctx->d_expect;
  p.expect_fixed = fixed_len < ctx->h_expect.size() ? ctx->h_expect[fixed_len] : 0u;
  p.sink = ctx->d_sink;
  p.variant = MGENX_DIAG ? ctx->unpack_variant : 0;
  p.cols = k;
  const uint64_t groups = ((uint64_t)n + 15) / 16;
  const uint64_t per_block = (uint64_t)mgenx::unpack_threads() / 64;  // waves per block
  uint64_t grid = (groups + per_block - 1) / per_block;
  if (grid > (uint64_t)ctx->cu_count) grid = ctx->cu_count;
  hipError_t e = mgenx::launch_unpack(p, (int)grid, ctx->cu_count, (hipStream_t)stream,
                                      &ctx->unpack_last);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "unpack");
}

int mgenx_unpack_last_kernel(const mgenx_ctx* ctx) { return ctx ? ctx->unpack_last : 0; }

int mgenx_pack_prepare(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl, uint32_t n_tmpl,
                       const uint8_t* dev_pool, uint32_t* dev_tmpl_crc, void* stream) {
  if (!ctx || (n_tmpl && (!dev_tmpl || !dev_tmpl_crc))) return MGENX_EINVAL;
  hipError_t e = mgenx::launch_pack_prepare(dev_tmpl, n_tmpl, dev_pool, ctx->d_bytetab,
                                            dev_tmpl_crc, (hipStream_t)stream);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "pack_prepare");
}

int mgenx_pack_batch(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                     const uint32_t* dev_tmpl_crc, const mgenx_pack_desc* dev_desc, uint32_t n,
                     const uint8_t* dev_pool, uint8_t* dev_slab, uint64_t slab_bytes,
                     const uint64_t* dev_rec_off, uint64_t stride, uint32_t* dev_out_len,
                     uint32_t opts, uint32_t fill_time, void* stream) {
  if (opts & MGENX_PACK_RAW) return MGENX_EINVAL;  // mgenx_pack_msgs is the raw form
  return mgenx::pack_common(ctx, dev_tmpl, dev_tmpl_crc, dev_desc, n, dev_pool, dev_slab,
                            slab_bytes, dev_rec_off, stride, nullptr, nullptr, dev_out_len, nullptr,
                            nullptr, opts, fill_time, stream);
}

int mgenx_pack_msgs(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                    const uint32_t* dev_tmpl_crc, const mgenx_pack_desc* dev_desc, uint32_t n,
                    const uint8_t* dev_pool, uint8_t* dev_slab, uint64_t slab_bytes,
                    const uint64_t* dev_rec_off, uint64_t stride, const uint32_t* dev_buf_len,
                    const uint32_t* dev_crc_in, uint32_t* dev_out_len, uint32_t* dev_tx_crc,
                    uint32_t* dev_state, uint32_t opts, uint32_t fill_time, void* stream) {
  return mgenx::pack_common(ctx, dev_tmpl, dev_tmpl_crc, dev_desc, n, dev_pool, dev_slab,
                            slab_bytes, dev_rec_off, stride, dev_buf_len, dev_crc_in, dev_out_len,
                            dev_tx_crc, dev_state, opts | MGENX_PACK_RAW, fill_time, stream);
}

int mgenx_tcp_rx_persist(mgenx_ctx* ctx, const uint8_t* dev_slab, const uint64_t* dev_rec_off,
                         const uint32_t* dev_rec_len, uint32_t n, const mgenx_cols* cols,
                         mgenx_rx_state* dev_state, uint32_t* dev_payload_rec, uint32_t opts,
                         void* stream) {
  if (!ctx || !cols || !dev_state || (opts & ~(uint32_t)(MGENX_RX_NOLOG | MGENX_RX_FORCE)))
    return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  const mgenx_cols& c = *cols;
  if (!c.flow_id || !c.seq_num || !c.tx_sec || !c.tx_usec || !c.msg_len || !c.dst_port ||
      !c.flags || !c.err || !c.dst_type || !c.dst_len || !c.dst_addr4 || !c.payload_len ||
      !c.payload_type || !c.gps_status || !c.decoded || !dev_slab || !dev_rec_off || !dev_rec_len)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  const size_t need = mgenx::rx_persist_ws_bytes(n);
  hipError_t e = ctx->rx_ws.reserve(need);  // allocates only when the batch outgrows it
  if (e != hipSuccess) return set_err(ctx, e, "rx workspace");
  e = mgenx::launch_rx_persist(c, n, opts, static_cast<int32_t*>(ctx->rx_ws.p), dev_state, dev_slab,
                               dev_rec_off, dev_rec_len, ctx->d_bytetab, dev_payload_rec,
                               (hipStream_t)stream);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "rx persist");
}

#if MGENX_DIAG
int mgenx_set_tuning(mgenx_ctx* ctx, int key, int value) {
  if (!ctx) return MGENX_EINVAL;
  if (key == MGENX_TUNE_PACK_VARIANT) {
    if (value < 0 || value > 10) return MGENX_EINVAL;
    ctx->pack_variant = value;
    return MGENX_OK;
  }
  if (key == MGENX_TUNE_UNPACK_VARIANT) {
    if (value < 0 || value > 2047) return MGENX_EINVAL;
    ctx->unpack_variant = value;
    return MGENX_OK;
  }
  return MGENX_EINVAL;
}

int mgenx_diag_stream_read(mgenx_ctx* ctx, const uint8_t* dev_data, uint64_t bytes,
                           uint32_t* dev_scratch, int grid, void* stream) {
  if (!ctx || !dev_data || !dev_scratch || grid <= 0) return MGENX_EINVAL;
  hipError_t e = mgenx::launch_stream_read(dev_data, bytes, dev_scratch, grid,
                                           (hipStream_t)stream);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "stream_read");
}

int mgenx_diag_stream_read_w(mgenx_ctx* ctx, const uint8_t* dev_data, uint64_t bytes,
                             uint32_t* dev_scratch, int grid, int width, void* stream) {
  if (!ctx || !dev_data || !dev_scratch || grid <= 0) return MGENX_EINVAL;
  hipError_t e = mgenx::launch_stream_read_w(dev_data, bytes, dev_scratch, grid, width,
                                             (hipStream_t)stream);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "stream_read_w");
}

int mgenx_diag_group_rw(mgenx_ctx* ctx, const uint8_t* dev_data, uint64_t bytes,
                        uint8_t* dev_out, int mode, void* stream) {
  if (!ctx || !dev_data || !dev_out || bytes % 16384 != 0) return MGENX_EINVAL;
  hipError_t e = mgenx::launch_group_rw(dev_data, bytes, dev_out, mode, ctx->cu_count,
                                        (hipStream_t)stream);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "group_rw");
}

#endif  // MGENX_DIAG

int mgenx_stream_scan(mgenx_ctx* ctx, const uint8_t* dev_stream, uint64_t nbytes, int mode,
                      uint64_t* dev_rec_off, uint32_t* dev_rec_len, uint64_t cap,
                      mgenx_scan_info* info, void* stream) {
  if (!ctx || (nbytes && !dev_stream) || (cap && (!dev_rec_off || !dev_rec_len)) ||
      (mode != MGENX_SCAN_TCP && mode != MGENX_SCAN_SINK))
    return MGENX_EINVAL;
  if (nbytes == 0) {
    if (info) memset(info, 0, sizeof(*info));
    return MGENX_OK;
  }
  hipSetDevice(ctx->device);
  if (!ctx->scan_ws) ctx->scan_ws = mgenx::scan_ws_new();
  return mgenx::scan_run(ctx->scan_ws, dev_stream, nbytes, mode, dev_rec_off, dev_rec_len, cap,
                        info, (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_stream_scan_exits(mgenx_ctx* ctx, const uint8_t* dev_stream, uint64_t nbytes, int mode,
                            uint64_t window, uint64_t limit, uint64_t* dev_entries,
                            uint64_t* dev_exits, uint32_t cap, uint32_t* candidates,
                            void* stream) {
  if (!ctx || !dev_stream || nbytes == 0 || limit > nbytes || (cap && (!dev_entries || !dev_exits)) ||
      (mode != MGENX_SCAN_TCP && mode != MGENX_SCAN_SINK))
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->scan_ws) ctx->scan_ws = mgenx::scan_ws_new();
  return mgenx::scan_exits_run(ctx->scan_ws, dev_stream, nbytes, mode, window, limit, dev_entries,
                              dev_exits, cap, candidates, (hipStream_t)stream, ctx->err,
                              sizeof(ctx->err));
}

int mgenx_stream_scan_range(mgenx_ctx* ctx, const uint8_t* dev_stream, uint64_t nbytes, int mode,
                            uint64_t entry, uint64_t limit, int flags, uint64_t* dev_rec_off,
                            uint32_t* dev_rec_len, uint64_t cap, mgenx_scan_info* info,
                            void* stream) {
  if (!ctx || !dev_stream || nbytes == 0 || limit > nbytes || (cap && (!dev_rec_off || !dev_rec_len)) ||
      (mode != MGENX_SCAN_TCP && mode != MGENX_SCAN_SINK) || (flags & ~MGENX_SCAN_REUSE))
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->scan_ws) ctx->scan_ws = mgenx::scan_ws_new();
  return mgenx::scan_range_run(ctx->scan_ws, dev_stream, nbytes, mode, entry, limit,
                              flags & MGENX_SCAN_REUSE, dev_rec_off, dev_rec_len, cap, info,
                              (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_flow_init(mgenx_ctx* ctx, mgenx_flow_state* dev_flows, uint32_t n_flows,
                    double window_sec, void* stream) {
  if (!ctx || (n_flows && !dev_flows) || !(window_sec >= 0.0)) return MGENX_EINVAL;
  return mgenx::flow_init_run(dev_flows, n_flows, window_sec, (hipStream_t)stream);
}

int mgenx_flow_reduce(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_seq,
                      const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                      const uint16_t* dev_msg_len, const uint32_t* dev_rx_sec,
                      const uint32_t* dev_rx_usec, uint32_t n, mgenx_flow_state* dev_flows,
                      uint32_t n_flows, mgenx_flow_report* dev_reports, uint32_t per_flow,
                      uint32_t* dev_report_count, void* stream) {
  return mgenx_flow_reduce_ex(ctx, dev_flow_idx, dev_seq, dev_tx_sec, dev_tx_usec, dev_msg_len,
                              dev_rx_sec, dev_rx_usec, n, dev_flows, n_flows, dev_reports,
                              per_flow, dev_report_count, nullptr, stream);
}

int mgenx_flow_reduce_ex(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_seq,
                         const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                         const uint16_t* dev_msg_len, const uint32_t* dev_rx_sec,
                         const uint32_t* dev_rx_usec, uint32_t n, mgenx_flow_state* dev_flows,
                         uint32_t n_flows, mgenx_flow_report* dev_reports, uint32_t per_flow,
                         uint32_t* dev_report_count, uint32_t* dev_report_rec, void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0 || n_flows == 0) return MGENX_OK;
  if (!dev_flow_idx || !dev_seq || !dev_tx_sec || !dev_tx_usec || !dev_msg_len ||
      !dev_rx_sec || !dev_rx_usec || !dev_flows ||
      (per_flow && (!dev_reports || !dev_report_count)) || n > 0x7FFFFFFFu)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->flow_ws) ctx->flow_ws = mgenx::flow_ws_new();
  return mgenx::flow_reduce_run(ctx->flow_ws, dev_flow_idx, dev_seq, dev_tx_sec, dev_tx_usec,
                               dev_msg_len, nullptr, dev_rx_sec, dev_rx_usec, n, dev_flows,
                               n_flows, dev_reports, per_flow, dev_report_count, dev_report_rec,
                               (hipStream_t)stream,
                               ctx->err, sizeof(ctx->err));
}

int mgenx_flow_reduce_rows(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const mgenx_rec* dev_rows,
                           const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec, uint32_t n,
                           mgenx_flow_state* dev_flows, uint32_t n_flows,
                           mgenx_flow_report* dev_reports, uint32_t per_flow,
                           uint32_t* dev_report_count, uint32_t* dev_report_rec, void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0 || n_flows == 0) return MGENX_OK;
  if (!dev_flow_idx || !dev_rows || !dev_rx_sec || !dev_rx_usec || !dev_flows ||
      (per_flow && (!dev_reports || !dev_report_count)) || n > 0x7FFFFFFFu)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->flow_ws) ctx->flow_ws = mgenx::flow_ws_new();
  return mgenx::flow_reduce_run(ctx->flow_ws, dev_flow_idx, nullptr, nullptr, nullptr, nullptr,
                               dev_rows, dev_rx_sec, dev_rx_usec, n, dev_flows, n_flows,
                               dev_reports, per_flow, dev_report_count, dev_report_rec,
                               (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_flow_dist_init(mgenx_ctx* ctx, struct mgenx_flow_dist* dev_dist, uint64_t* dev_hist,
                         uint32_t n_flows, void* stream) {
  if (!ctx || (n_flows && !dev_dist) || n_flows > 0x7FFFFFFFu) return MGENX_EINVAL;
  if (n_flows == 0) return MGENX_OK;
  hipSetDevice(ctx->device);
  return mgenx::flow_dist_init_run(dev_dist, dev_hist, n_flows, (hipStream_t)stream);
}

int mgenx_flow_dist(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_seq,
                    const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                    const uint16_t* dev_msg_len, const uint32_t* dev_rx_sec,
                    const uint32_t* dev_rx_usec, uint32_t n, struct mgenx_flow_dist* dev_dist,
                    uint64_t* dev_hist, uint32_t n_flows, void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0 || n_flows == 0) return MGENX_OK;
  if (!dev_flow_idx || !dev_seq || !dev_tx_sec || !dev_tx_usec || !dev_msg_len || !dev_rx_sec ||
      !dev_rx_usec || !dev_dist || n > 0x7FFFFFFFu || n_flows > 0x7FFFFFFFu)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return mgenx::flow_dist_run(ctx->flowdist_ws, dev_flow_idx, dev_seq, dev_tx_sec, dev_tx_usec,
                             dev_msg_len, dev_rx_sec, dev_rx_usec, n, dev_dist, dev_hist, n_flows,
                             (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_flow_dist_quantiles(mgenx_ctx* ctx, const struct mgenx_flow_dist* dev_dist,
                              const uint64_t* dev_hist, uint32_t n_flows,
                              const uint32_t* permille, uint32_t n_q, int64_t* dev_out,
                              void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n_flows == 0 || n_q == 0) return MGENX_OK;
  if (!dev_dist || !dev_hist || !permille || !dev_out) return MGENX_EINVAL;
  for (uint32_t j = 0; j < n_q; j++)
    if (permille[j] < 1u || permille[j] > 1000u) return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return mgenx::flow_dist_quantiles_run(dev_dist, dev_hist, n_flows, permille, n_q, dev_out,
                                       (hipStream_t)stream);
}

uint32_t mgenx_flow_dist_bin(uint64_t v) { return mgenx::flow_dist_bin(v); }
uint64_t mgenx_flow_dist_bin_lo(uint32_t bin) { return mgenx::flow_dist_bin_lo(bin); }

int mgenx_flow_series_init(mgenx_ctx* ctx, struct mgenx_flow_series_state* dev_state,
                           struct mgenx_flow_series_bin* dev_bins, uint32_t n_flows,
                           uint32_t n_bins, void* stream) {
  if (!ctx || n_bins == 0 || (uint64_t)n_flows * n_bins >= (1ull << 31)) return MGENX_EINVAL;
  if (n_flows == 0) return MGENX_OK;
  if (!dev_state || !dev_bins) return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return mgenx::flow_series_init_run(dev_state, dev_bins, n_flows, n_bins, (hipStream_t)stream);
}

int mgenx_flow_series(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_seq,
                      const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                      const uint16_t* dev_msg_len, const uint32_t* dev_rx_sec,
                      const uint32_t* dev_rx_usec, uint32_t n, int64_t t0_us, uint64_t width_us,
                      uint32_t n_bins, struct mgenx_flow_series_state* dev_state,
                      struct mgenx_flow_series_bin* dev_bins, uint32_t n_flows, void* stream) {
  if (!ctx || width_us == 0 || n_bins == 0 || (uint64_t)n_flows * n_bins >= (1ull << 31))
    return MGENX_EINVAL;
  if (n == 0 || n_flows == 0) return MGENX_OK;
  if (!dev_flow_idx || !dev_seq || !dev_tx_sec || !dev_tx_usec || !dev_msg_len || !dev_rx_sec ||
      !dev_rx_usec || !dev_state || !dev_bins || n > 0x7FFFFFFFu)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return mgenx::flow_series_run(ctx->flowseries_ws, dev_flow_idx, dev_seq, dev_tx_sec, dev_tx_usec,
                               dev_msg_len, dev_rx_sec, dev_rx_usec, n, t0_us, width_us, n_bins,
                               dev_state, dev_bins, n_flows, (hipStream_t)stream, ctx->err,
                               sizeof(ctx->err));
}

int mgenx_flow_series_quantiles(mgenx_ctx* ctx, const uint32_t* dev_flow_idx,
                                const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                                const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec, uint32_t n,
                                int64_t t0_us, uint64_t width_us, uint32_t n_bins,
                                uint32_t n_flows, const uint32_t* permille, uint32_t n_q,
                                int64_t* dev_out, void* stream) {
  if (!ctx || width_us == 0 || n_bins == 0 || n_q == 0 || n_q > MGENX_FLOW_SERIES_MAX_Q ||
      !permille || (uint64_t)n_flows * n_bins >= (1ull << 31))
    return MGENX_EINVAL;
  for (uint32_t j = 0; j < n_q; j++)
    if (permille[j] < 1u || permille[j] > 1000u) return MGENX_EINVAL;
  if (!dev_out || n > 0x7FFFFFFFu) return MGENX_EINVAL;
  if (n && (!dev_flow_idx || !dev_tx_sec || !dev_tx_usec || !dev_rx_sec || !dev_rx_usec))
    return MGENX_EINVAL;
  if (n_flows == 0) return MGENX_OK;
  hipSetDevice(ctx->device);
  return mgenx::flow_quant_run(ctx->flowquant_ws, ctx->cu_count, dev_flow_idx, dev_tx_sec,
                              dev_tx_usec, dev_rx_sec, dev_rx_usec, n, t0_us, width_us, n_bins,
                              n_flows, permille, n_q, dev_out, (hipStream_t)stream, ctx->err,
                              sizeof(ctx->err));
}

int mgenx_match_side(mgenx_ctx* ctx, const uint8_t* dev_event, const uint8_t* dev_status,
                     const mgenx_addr* dev_src, uint32_t n, uint32_t want_event,
                     mgenx_addr* dev_src_out, uint8_t* dev_err_out, void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_event || !dev_status || !dev_src || !dev_src_out || !dev_err_out) return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return mgenx::match_side_run(dev_event, dev_status, dev_src, n, want_event, dev_src_out,
                              dev_err_out, (hipStream_t)stream);
}

int mgenx_msg_match(mgenx_ctx* ctx, const uint32_t* dev_send_flow_idx,
                    const uint32_t* dev_send_seq, const uint32_t* dev_send_t_sec,
                    const uint32_t* dev_send_t_usec, const uint32_t* dev_send_len, uint32_t ns,
                    const uint32_t* dev_recv_flow_idx, const uint32_t* dev_recv_seq,
                    const uint32_t* dev_recv_tx_sec, const uint32_t* dev_recv_tx_usec,
                    const uint32_t* dev_recv_rx_sec, const uint32_t* dev_recv_rx_usec,
                    uint32_t nr, uint32_t n_flows, uint32_t opts, uint32_t* dev_send_rx_count,
                    uint32_t* dev_send_first_rx, uint32_t* dev_recv_send,
                    struct mgenx_flow_match* dev_flows, struct mgenx_match_stats* dev_stats,
                    void* stream) {
  return mgenx_msg_match_ex(ctx, dev_send_flow_idx, dev_send_seq, dev_send_t_sec, dev_send_t_usec,
                            dev_send_len, ns, dev_recv_flow_idx, dev_recv_seq, dev_recv_tx_sec,
                            dev_recv_tx_usec, dev_recv_rx_sec, dev_recv_rx_usec, nr, n_flows, opts,
                            dev_send_rx_count, dev_send_first_rx, dev_recv_send, dev_flows,
                            dev_stats, nullptr, stream);
}

int mgenx_msg_match_ex(mgenx_ctx* ctx, const uint32_t* dev_send_flow_idx,
                       const uint32_t* dev_send_seq, const uint32_t* dev_send_t_sec,
                       const uint32_t* dev_send_t_usec, const uint32_t* dev_send_len, uint32_t ns,
                       const uint32_t* dev_recv_flow_idx, const uint32_t* dev_recv_seq,
                       const uint32_t* dev_recv_tx_sec, const uint32_t* dev_recv_tx_usec,
                       const uint32_t* dev_recv_rx_sec, const uint32_t* dev_recv_rx_usec,
                       uint32_t nr, uint32_t n_flows, uint32_t opts, uint32_t* dev_send_rx_count,
                       uint32_t* dev_send_first_rx, uint32_t* dev_recv_send,
                       struct mgenx_flow_match* dev_flows, struct mgenx_match_stats* dev_stats,
                       const mgenx_match_timeline* tl, void* stream) {
  if (!ctx || !dev_stats || ns > (1u << 30) || nr > 0x7FFFFFFFu || n_flows > 0x7FFFFFFFu)
    return MGENX_EINVAL;
  if (ns && (!dev_send_flow_idx || !dev_send_seq || !dev_send_t_sec || !dev_send_t_usec ||
             !dev_send_len || !dev_send_rx_count || !dev_send_first_rx))
    return MGENX_EINVAL;
  if (nr && (!dev_recv_flow_idx || !dev_recv_seq || !dev_recv_tx_sec || !dev_recv_tx_usec ||
             !dev_recv_rx_sec || !dev_recv_rx_usec || !dev_recv_send))
    return MGENX_EINVAL;
  if (n_flows && !dev_flows) return MGENX_EINVAL;
  if (tl && tl->n_bins) {
    const int64_t lim = (int64_t)1 << 62;
    if (tl->width_us == 0 || tl->t0_us < -lim || tl->t0_us > lim ||
        (uint64_t)n_flows * tl->n_bins >= (1ull << 31) ||
        (n_flows && (!tl->dev_bins || !tl->dev_outside)))
      return MGENX_EINVAL;
  }
  if (tl && tl->dev_n_runs && tl->run_cap && !tl->dev_runs) return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return mgenx::msg_match_run(ctx->match_ws, dev_send_flow_idx, dev_send_seq, dev_send_t_sec,
                             dev_send_t_usec, dev_send_len, ns, dev_recv_flow_idx, dev_recv_seq,
                             dev_recv_tx_sec, dev_recv_tx_usec, dev_recv_rx_sec, dev_recv_rx_usec,
                             nr, n_flows, opts, dev_send_rx_count, dev_send_first_rx,
                             dev_recv_send, dev_flows, dev_stats, tl, (hipStream_t)stream,
                             ctx->err, sizeof(ctx->err));
}

int mgenx_msg_match_multi(mgenx_ctx* ctx, const uint32_t* dev_send_flow_idx,
                          const uint32_t* dev_send_seq, const uint32_t* dev_send_t_sec,
                          const uint32_t* dev_send_t_usec, const uint32_t* dev_send_len,
                          uint32_t ns, const uint32_t* dev_recv_flow_idx,
                          const uint32_t* dev_recv_seq, const uint32_t* dev_recv_tx_sec,
                          const uint32_t* dev_recv_tx_usec, const uint32_t* dev_recv_rx_sec,
                          const uint32_t* dev_recv_rx_usec, const uint32_t* dev_recv_rcv,
                          uint32_t nr, uint32_t n_rcv, uint32_t n_flows, uint32_t opts,
                          uint64_t* dev_send_mask, uint32_t* dev_recv_send,
                          uint8_t* dev_recv_first, struct mgenx_rcv_cell* dev_cells,
                          struct mgenx_flow_fanout* dev_fanout,
                          struct mgenx_match_stats* dev_stats, const mgenx_multi_timeline* tl,
                          void* stream) {
  return mgenx_msg_match_multi_ex(ctx, dev_send_flow_idx, dev_send_seq, dev_send_t_sec,
                                  dev_send_t_usec, dev_send_len, ns, dev_recv_flow_idx,
                                  dev_recv_seq, dev_recv_tx_sec, dev_recv_tx_usec, dev_recv_rx_sec,
                                  dev_recv_rx_usec, dev_recv_rcv, nr, n_rcv, n_flows, opts,
                                  dev_send_mask, dev_recv_send, dev_recv_first, dev_cells,
                                  dev_fanout, dev_stats, tl, nullptr, stream);
}

int mgenx_msg_match_multi_ex(mgenx_ctx* ctx, const uint32_t* dev_send_flow_idx,
                             const uint32_t* dev_send_seq, const uint32_t* dev_send_t_sec,
                             const uint32_t* dev_send_t_usec, const uint32_t* dev_send_len,
                             uint32_t ns, const uint32_t* dev_recv_flow_idx,
                             const uint32_t* dev_recv_seq, const uint32_t* dev_recv_tx_sec,
                             const uint32_t* dev_recv_tx_usec, const uint32_t* dev_recv_rx_sec,
                             const uint32_t* dev_recv_rx_usec, const uint32_t* dev_recv_rcv,
                             uint32_t nr, uint32_t n_rcv, uint32_t n_flows, uint32_t opts,
                             uint64_t* dev_send_mask, uint32_t* dev_recv_send,
                             uint8_t* dev_recv_first, struct mgenx_rcv_cell* dev_cells,
                             struct mgenx_flow_fanout* dev_fanout,
                             struct mgenx_match_stats* dev_stats, const mgenx_multi_timeline* tl,
                             const mgenx_multi_loss* lx, void* stream) {
  if (lx) {
    if (lx->dev_pairs && n_rcv >= 1u && n_rcv <= 64u &&
        (uint64_t)n_flows * n_rcv * n_rcv >= (1ull << 31))
      return MGENX_EINVAL;
    if (lx->dev_n_runs && !lx->dev_runs && lx->run_cap > 0) return MGENX_EINVAL;
  }
  if (!ctx || !dev_stats || n_rcv < 1u || n_rcv > 64u || ns > (1u << 30) || nr > (1u << 30) ||
      (uint64_t)n_flows * n_rcv >= (1ull << 31))
    return MGENX_EINVAL;
  if (ns && (!dev_send_flow_idx || !dev_send_seq || !dev_send_t_sec || !dev_send_t_usec ||
             !dev_send_len || !dev_send_mask))
    return MGENX_EINVAL;
  if (nr && (!dev_recv_flow_idx || !dev_recv_seq || !dev_recv_tx_sec || !dev_recv_tx_usec ||
             !dev_recv_rx_sec || !dev_recv_rx_usec || !dev_recv_rcv || !dev_recv_send ||
             !dev_recv_first))
    return MGENX_EINVAL;
  if (n_flows && (!dev_cells || !dev_fanout)) return MGENX_EINVAL;
  if (tl && tl->n_bins) {
    const int64_t lim = (int64_t)1 << 62;
    if (tl->width_us == 0 || tl->t0_us < -lim || tl->t0_us > lim ||
        (uint64_t)n_flows * tl->n_bins >= (1ull << 31) ||
        (n_flows && (!tl->dev_bins || !tl->dev_outside)))
      return MGENX_EINVAL;
  }
  hipSetDevice(ctx->device);
  return mgenx::msg_match_multi_run(ctx->match_ws, dev_send_flow_idx, dev_send_seq, dev_send_t_sec,
                                   dev_send_t_usec, dev_send_len, ns, dev_recv_flow_idx,
                                   dev_recv_seq, dev_recv_tx_sec, dev_recv_tx_usec,
                                   dev_recv_rx_sec, dev_recv_rx_usec, dev_recv_rcv, nr, n_rcv,
                                   n_flows, opts, dev_send_mask, dev_recv_send, dev_recv_first,
                                   dev_cells, dev_fanout, dev_stats, tl, lx, (hipStream_t)stream,
                                   ctx->err, sizeof(ctx->err));
}

static int log_recv(mgenx_ctx* ctx, bool binary, const uint8_t* dev_slab, uint64_t slab_bytes,
                    const uint64_t* dev_rec_off, const uint32_t* dev_rec_len, uint64_t stride,
                    const mgenx_cols* cols,
                    const mgenx_addr* dev_src, const uint32_t* dev_rx_sec,
                    const uint32_t* dev_rx_usec, const int32_t* dev_ttl, uint32_t n,
                    int protocol, uint32_t opts, char* dev_text, uint64_t text_cap,
                    uint64_t* dev_line_off, void* stream) {
  if (!ctx || !cols || !dev_line_off) return MGENX_EINVAL;
  if (n == 0) return hipMemsetAsync(dev_line_off, 0, 8, (hipStream_t)stream) == hipSuccess
                         ? MGENX_OK : MGENX_EDEVICE;
  const mgenx_cols& k = *cols;
  const bool core = k.rows || (k.flow_id && k.seq_num && k.tx_sec && k.tx_usec && k.msg_len &&
                               k.dst_port && k.flags && k.err && k.dst_type && k.dst_len &&
                               k.payload_len && k.payload_type && k.gps_status);
  const bool ext = k.dst_addr && k.host_addr && k.host_port && k.host_type && k.host_len &&
                   k.lat_raw && k.lon_raw && k.alt && k.payload_off && (!binary || k.hdr_len);
  if (!core || !ext || !dev_slab || !dev_src || !dev_rx_sec || !dev_rx_usec ||
      (!dev_rec_off && stride == 0 && n > 1) || (text_cap && !dev_text) || n > 0x7FFFFFFEu)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->log_ws) ctx->log_ws = mgenx::log_ws_new();
  return mgenx::log_recv_run(ctx->log_ws, binary, dev_slab, slab_bytes, dev_rec_off, dev_rec_len,
                            stride, cols,
                            dev_src, dev_rx_sec, dev_rx_usec, dev_ttl, n, protocol, opts,
                            dev_text, text_cap, dev_line_off, (hipStream_t)stream, ctx->err,
                            sizeof(ctx->err));
}

int mgenx_log_recv_text(mgenx_ctx* ctx, const uint8_t* dev_slab, const uint64_t* dev_rec_off,
                        uint64_t stride, const mgenx_cols* cols, const mgenx_addr* dev_src,
                        const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                        const int32_t* dev_ttl, uint32_t n, int protocol, uint32_t opts,
                        char* dev_text, uint64_t text_cap, uint64_t* dev_line_off,
                        void* stream) {
  return log_recv(ctx, false, dev_slab, ~0ull, dev_rec_off, nullptr, stride, cols, dev_src,
                  dev_rx_sec,
                  dev_rx_usec, dev_ttl, n, protocol, opts, dev_text, text_cap, dev_line_off,
                  stream);
}

int mgenx_log_recv_binary(mgenx_ctx* ctx, const uint8_t* dev_slab, uint64_t slab_bytes,
                          const uint64_t* dev_rec_off, uint64_t stride,
                          const uint32_t* dev_rec_len, const mgenx_cols* cols,
                          const mgenx_addr* dev_src, const uint32_t* dev_rx_sec,
                          const uint32_t* dev_rx_usec, uint32_t n, int protocol,
                          uint8_t* dev_out, uint64_t out_cap, uint64_t* dev_rec_pos,
                          void* stream) {
  return log_recv(ctx, true, dev_slab, slab_bytes, dev_rec_off, dev_rec_len, stride, cols, dev_src,
                  dev_rx_sec, dev_rx_usec, nullptr, n, protocol, 0, (char*)dev_out, out_cap,
                  dev_rec_pos, stream);
}

static int log_send(mgenx_ctx* ctx, bool binary, const mgenx_flow_tmpl* dev_tmpl,
                    const mgenx_pack_desc* dev_desc, const uint16_t* dev_src_port,
                    const uint32_t* dev_out_len, const uint32_t* dev_msg_total,
                    const uint8_t* dev_slab, uint64_t slab_bytes, const uint64_t* dev_rec_off,
                    uint64_t stride, uint32_t n, int protocol, uint32_t opts, uint8_t* dev_out,
                    uint64_t out_cap, uint64_t* dev_pos, void* stream) {
  if (!ctx || !dev_pos) return MGENX_EINVAL;
  if (n == 0) return hipMemsetAsync(dev_pos, 0, 8, (hipStream_t)stream) == hipSuccess
                         ? MGENX_OK : MGENX_EDEVICE;
  if (!dev_tmpl || !dev_desc || (!binary && !dev_src_port) || (out_cap && !dev_out) ||
      (binary && (!dev_slab || (!dev_rec_off && stride == 0 && n > 1))) || n > 0x7FFFFFFEu)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->log_ws) ctx->log_ws = mgenx::log_ws_new();
  return mgenx::log_send_exec(ctx->log_ws, dev_tmpl, dev_desc, dev_src_port, dev_out_len,
                             dev_msg_total, dev_slab, slab_bytes, dev_rec_off, stride, n,
                             protocol, opts, binary, dev_out, out_cap, dev_pos,
                             (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_log_send_text(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                        const mgenx_pack_desc* dev_desc, const uint16_t* dev_src_port,
                        const uint32_t* dev_out_len, const uint32_t* dev_msg_total, uint32_t n,
                        int protocol, uint32_t opts, char* dev_text, uint64_t text_cap,
                        uint64_t* dev_line_off, void* stream) {
  return log_send(ctx, false, dev_tmpl, dev_desc, dev_src_port, dev_out_len, dev_msg_total,
                  nullptr, 0, nullptr, 0, n, protocol, opts, (uint8_t*)dev_text, text_cap,
                  dev_line_off, stream);
}

int mgenx_log_send_binary(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                          const mgenx_pack_desc* dev_desc, const uint32_t* dev_out_len,
                          const uint32_t* dev_msg_total, const uint8_t* dev_slab,
                          uint64_t slab_bytes, const uint64_t* dev_rec_off, uint64_t stride,
                          uint32_t n, int protocol, uint8_t* dev_out, uint64_t out_cap,
                          uint64_t* dev_rec_pos, void* stream) {
  return log_send(ctx, true, dev_tmpl, dev_desc, nullptr, dev_out_len, dev_msg_total, dev_slab,
                  slab_bytes, dev_rec_off, stride, n, protocol, 0, dev_out, out_cap, dev_rec_pos,
                  stream);
}

int mgenx_report_build(mgenx_ctx* ctx, const mgenx_flow_report* dev_reports, uint32_t n_flows,
                       uint32_t per_flow, const uint32_t* dev_report_count,
                       const mgenx_report_key* dev_keys, uint8_t* dev_sign,
                       const double* dev_offset, uint8_t* dev_items, uint8_t* dev_item_len,
                       void* stream) {
  if (!ctx || (n_flows && per_flow && (!dev_reports || !dev_report_count || !dev_keys ||
                                       !dev_sign || !dev_items || !dev_item_len)))
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  return mgenx::report_build_run(dev_reports, n_flows, per_flow, dev_report_count, dev_keys,
                                dev_sign, dev_offset, ctx->d_rq, dev_items, dev_item_len,
                                (hipStream_t)stream);
}

int mgenx_log_report_text(mgenx_ctx* ctx, const uint8_t* dev_items,
                          const mgenx_flow_report* dev_reports, uint32_t n_flows,
                          uint32_t per_flow, const uint32_t* dev_report_count, uint32_t opts,
                          char* dev_text, uint64_t text_cap, uint64_t* dev_line_off,
                          void* stream) {
  const uint64_t n = (uint64_t)n_flows * per_flow;
  if (!ctx || n > 0xFFFFFFFFull || !dev_line_off ||
      (n && (!dev_items || !dev_reports || !dev_report_count)) || (text_cap && !dev_text))
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->log_ws) ctx->log_ws = mgenx::log_ws_new();
  return mgenx::report_lines(ctx->log_ws, dev_items, dev_reports, dev_report_count, per_flow,
                            nullptr, nullptr, nullptr, nullptr, nullptr, (uint32_t)n, opts,
                            ctx->d_rq, dev_text, text_cap, dev_line_off, (hipStream_t)stream,
                            ctx->err, sizeof(ctx->err));
}

int mgenx_data_walk(mgenx_ctx* ctx, const uint8_t* dev_slab, const uint64_t* dev_rec_off,
                    uint64_t stride, const mgenx_cols* cols, uint32_t n, uint32_t opts,
                    uint8_t* dev_status, uint8_t* dev_needs_host, uint32_t* dev_cmds,
                    uint32_t cmd_cap, uint64_t* dev_reps, uint32_t rep_cap,
                    uint32_t* dev_totals, void* stream) {
  if (!ctx || !cols || (opts & ~(uint32_t)MGENX_DATA_CONTROLLER)) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_slab || (!dev_rec_off && stride == 0 && n > 1) || !cols->err || !cols->payload_type ||
      !cols->payload_len || !cols->payload_off || !dev_status || !dev_needs_host ||
      (cmd_cap && !dev_cmds) || (rep_cap && !dev_reps))
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->log_ws) ctx->log_ws = mgenx::log_ws_new();
  return mgenx::data_walk_exec(ctx->log_ws, dev_slab, dev_rec_off, stride, cols, n, opts,
                              ctx->d_rq, dev_status, dev_needs_host, dev_cmds, cmd_cap, dev_reps,
                              rep_cap, dev_totals, (hipStream_t)stream, ctx->err,
                              sizeof(ctx->err));
}

int mgenx_log_report_recv_text(mgenx_ctx* ctx, const uint8_t* dev_slab, const uint64_t* dev_reps,
                               uint32_t n_reps, const mgenx_addr* dev_src,
                               const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                               uint32_t opts, char* dev_text, uint64_t text_cap,
                               uint64_t* dev_line_off, void* stream) {
  if (!ctx || !dev_line_off || (n_reps && (!dev_slab || !dev_reps || !dev_src || !dev_rx_sec ||
                                          !dev_rx_usec)) || (text_cap && !dev_text))
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (!ctx->log_ws) ctx->log_ws = mgenx::log_ws_new();
  return mgenx::report_lines(ctx->log_ws, nullptr, nullptr, nullptr, 1, dev_reps, dev_slab,
                            dev_src, dev_rx_sec, dev_rx_usec, n_reps, opts, ctx->d_rq, dev_text,
                            text_cap, dev_line_off, (hipStream_t)stream, ctx->err,
                            sizeof(ctx->err));
}

int mgenx_flow_export(mgenx_ctx* ctx, const mgenx_flow_state* dev_flows, uint32_t n_flows,
                      mgenx_flow_counters* dev_out, void* stream) {
  if (!ctx || (n_flows && (!dev_flows || !dev_out))) return MGENX_EINVAL;
  return mgenx::flow_export_run(dev_flows, n_flows, dev_out, (hipStream_t)stream);
}

int mgenx_crc32_batch(mgenx_ctx* ctx, const uint8_t* dev_data, const uint64_t* dev_off,
                      const uint32_t* dev_len, uint32_t n, uint32_t* dev_out, void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_data || !dev_off || !dev_len || !dev_out) return MGENX_EINVAL;
  hipError_t e = mgenx::launch_crc32(dev_data, dev_off, dev_len, n, ctx->d_bytetab,
                                     ctx->d_tabs + 1024, ctx->d_xpow, nullptr,
                                     dev_out, (hipStream_t)stream);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "crc32");
}

int mgenx_crc32_update(mgenx_ctx* ctx, const uint8_t* dev_data, const uint64_t* dev_off,
                       const uint32_t* dev_len, uint32_t n, const uint32_t* dev_state_in,
                       uint32_t* dev_state_out, void* stream) {
  if (!ctx) return MGENX_EINVAL;
  if (n == 0) return MGENX_OK;
  if (!dev_data || !dev_off || !dev_len || !dev_state_in || !dev_state_out) return MGENX_EINVAL;
  hipError_t e = mgenx::launch_crc32(dev_data, dev_off, dev_len, n, ctx->d_bytetab,
                                     ctx->d_tabs + 1024, ctx->d_xpow, dev_state_in,
                                     dev_state_out, (hipStream_t)stream);
  return e == hipSuccess ? MGENX_OK : set_err(ctx, e, "crc32_update");
}

int mgenx_text_interleave(mgenx_ctx* ctx, const mgenx_text_src* srcs, uint32_t n_src,
                          uint32_t n_rec, char* dev_out, uint64_t out_cap, uint64_t* dev_rec_off,
                          void* stream) {
  if (!ctx || !dev_rec_off || n_src > MGENX_TEXT_MAX_SRC || (n_src && !srcs) ||
      (out_cap && !dev_out) || n_rec > 0x7FFFFFFEu)
    return MGENX_EINVAL;
  for (uint32_t s = 0; s < n_src; s++) {
    const mgenx_text_src& t = srcs[s];
    if (t.kind > MGENX_TEXT_SCATTER || !t.line_off ||
        (t.kind != MGENX_TEXT_PER_RECORD && !t.index) ||
        (t.kind == MGENX_TEXT_OWNER && t.index_stride == 0))
      return MGENX_EINVAL;
  }
  hipSetDevice(ctx->device);
  if (!ctx->log_ws) ctx->log_ws = mgenx::log_ws_new();
  return mgenx::text_interleave_run(ctx->log_ws, srcs, n_src, n_rec, dev_out, out_cap,
                                   dev_rec_off, (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_text_index(mgenx_ctx* ctx, const char* dev_text, uint64_t nbytes,
                     uint64_t* dev_line_off, uint64_t cap, uint64_t* dev_n_lines, void* stream) {
  if (!ctx || !dev_n_lines || (nbytes && !dev_text) || (cap && !dev_line_off) ||
      nbytes > (1ull << 44))
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  void* ws = nullptr;
  if (nbytes) {
    ws = ctx->lp.get(mgenx::text_index_ws(nbytes));
    if (!ws) return set_err(ctx, hipErrorOutOfMemory, "text_index workspace");
  }
  return mgenx::text_index_run(ws, (const uint8_t*)dev_text, nbytes, dev_line_off, cap, dev_n_lines,
                              (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

int mgenx_log_parse_text(mgenx_ctx* ctx, const char* dev_text, uint64_t nbytes,
                         const uint64_t* dev_line_off, uint32_t n, uint32_t opts,
                         uint32_t day_base_sec, const mgenx_logparse_out* out, void* stream) {
  if (!ctx || !out || !out->event || !out->status || (n && (!dev_line_off || !dev_text)) ||
      (out->payload_cap && !out->payload) || (out->payload && !out->payload_off) ||
      (opts & ~(uint32_t)MGENX_PARSE_NO_DAYS) || n > 0x7FFFFFFEu)
    return MGENX_EINVAL;
  hipSetDevice(ctx->device);
  if (n == 0) {
    if (out->payload_off &&
        hipMemsetAsync(out->payload_off, 0, 8, (hipStream_t)stream) != hipSuccess)
      return set_err(ctx, hipGetLastError(), "log_parse_text");
    return MGENX_OK;
  }
  void* ws = ctx->lp.get(mgenx::log_parse_ws(n));
  if (!ws) return set_err(ctx, hipErrorOutOfMemory, "log_parse_text workspace");
  return mgenx::log_parse_run(ws, (const uint8_t*)dev_text, nbytes, dev_line_off, n, opts,
                             day_base_sec, out, (hipStream_t)stream, ctx->err, sizeof(ctx->err));
}

}  // extern "C"
