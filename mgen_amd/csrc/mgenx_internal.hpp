// mgenx_internal.hpp -- the host-side contract between the library's .hip files.
//
// Three headers are shared by the translation units, and each holds one kind of thing:
//   mgenx_kernels.hpp   what it takes to launch another file's kernel: the parameter blocks, the
//                       launch_* functions, and the layouts host and device agree on (the
//                       worker's mailbox, the report quantizer tables kRq*, the operator tables
//                       kTab*).
//   mgenx_blockscan.hpp device code only, for the per-flow passes (flow_dist, flow_series,
//                       flow_clock, msg_match, msg_match_multi): the chunk size kChunk, word-wise
//                       lane shuffles, the wave reduction, the segmented scan over a workgroup
//                       and its carry over the chunks.  Included by the .hip files that use it,
//                       not by this header.
//   this header         host code only: device memory that grows on demand (DevBuf, Carve), the
//                       context, and every host function that one file defines and another
//                       calls.  Each is declared here once, in namespace mgenx, and both the
//                       defining file and the calling files include this header: the compiler
//                       checks the definition against the declaration, the mangled name makes
//                       the linker check the callers, and the name stays out of the library's C
//                       namespace, which is include/mgenx.h (and mgenx_diag.h) alone.
#pragma once

#include <stdio.h>

#include <vector>

#include "mgenx_kernels.hpp"

struct mgenx_scan_ws;  // mgenx_scan.hip: tables of the last stream built, host-mapped words
struct mgenx_flow_ws;  // mgenx_analytic.hip: the workspace, the CU count, the scan's epoch words
struct mgenx_log_ws;   // mgenx_log.hip: one scratch area per stream

namespace mgenx {

struct DistRec;  // mgenx_flowdist.hpp: one packed record of the per-flow passes

// Ends the resident worker waves (mgenx_worker_*, mgenx_worker_host.hip) of `device` (every
// device when device < 0) and waits for them; the calling thread's current device is left as it
// was.  hipFree / hipHostFree synchronise the device, so with a wave still polling its mailbox
// they would wait for its idle timeout: every workspace growth frees through these.
void quiesce_workers(int device);
inline void dev_free(void* p) {
  if (!p) return;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  quiesce_workers(dev);  // hipFree synchronises the current device only
  (void)hipFree(p);
}
inline void host_free(void* p) {
  if (!p) return;
  quiesce_workers(-1);  // pinned host memory may be mapped on every device
  (void)hipHostFree(p);
}

// A device buffer that grows on demand and never shrinks.  reserve(need) allocates only when
// `need` exceeds what the buffer holds (the old block goes through dev_free first; its contents
// are not kept), so a call that fits performs no allocation, no synchronisation and no copy.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t need) {
    if (bytes >= need) return hipSuccess;
    dev_free(p);
    p = nullptr;
    bytes = 0;
    const hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) bytes = need;
    else p = nullptr;
    return e;
  }
  void* get(size_t need) { return reserve(need) == hipSuccess ? p : nullptr; }  // null: no memory
  void release() {
    dev_free(p);
    p = nullptr;
    bytes = 0;
  }
};

inline size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

// A cursor over a 256-byte-aligned base pointer that hands out 256-byte-aligned pieces in call
// order: `Carve take(buf.p); T* a = (T*)take(bytes_a); ...`.  Where a size function and a run
// function carve the same buffer (flow_sort_ws / flow_sort_run, flow_prep_ws / flow_prep_run, the
// *_ws / *_run pairs of the capture files), the size is the sum of a256() over the same pieces.
struct Carve {
  char* at;
  explicit Carve(void* base) : at(static_cast<char*>(base)) {}
  char* operator()(size_t bytes) {
    char* q = at;
    at += a256(bytes);
    return q;
  }
};

}  // namespace mgenx

// The context owns only constant tables (CRC shift operators, x^(8n) mod P, the random fill
// stream, the report quantizers) and the workspaces of the composite calls; every data buffer
// belongs to the caller.
struct mgenx_ctx {
  int device = 0;
  int cu_count = 0;
  uint32_t* d_tabs = nullptr;     // [A64 | A4 | A8 | A12 | A16 | A32 | A48 | A128 | A256 | A512 | A1024]
  uint32_t* d_expect = nullptr;   // [65536]
  std::vector<uint32_t> h_expect;  // host copy of the expect table
  uint32_t* d_xpow = nullptr;     // [65536]
  uint32_t* d_ia = nullptr;       // [65536]
  uint32_t* d_bytetab = nullptr;  // [256]
  uint8_t* d_rtab = nullptr;      // 16 + 65536 + 32 bytes
  uint32_t* d_rcrc = nullptr;     // [65536]
  uint8_t* d_sink = nullptr;      // 1 KiB: column stores of lanes past the batch end
  double* d_rq = nullptr;         // report quantizer tables (mgenx::kRq*), built with host libm
  mgenx_scan_ws* scan_ws = nullptr;  // stream-scan workspace (mgenx_scan.hip), made on first use
  mgenx_flow_ws* flow_ws = nullptr;  // flow-reduce workspace (mgenx_analytic.hip), likewise
  mgenx_log_ws* log_ws = nullptr;    // log-format workspace (mgenx_log.hip), likewise
  mgenx::DevBuf flowdist_ws;      // flow-dist workspace (mgenx_flowdist.hip)
  mgenx::DevBuf flowseries_ws;    // flow-series workspace (mgenx_flowseries.hip)
  mgenx::DevBuf flowquant_ws;     // windowed-percentile workspace (mgenx_flowquant.hip)
  mgenx::DevBuf flowclock_ws;     // clock offset / skew workspace (mgenx_flowclock.hip)
  mgenx::DevBuf match_ws;         // msg-match workspace (mgenx_match.hip, mgenx_matchmulti.hip)
  mgenx::DevBuf tcp_ws;           // TCP transmit workspace (mgenx_pack_tcp)
  uint64_t* tcp_host = nullptr;   // host-mapped words: the plan's verdict (16 bytes)
  void* tcp_plan = nullptr;       // the plan's maximum word, skip word and look-back words
  uint32_t tcp_plan_blocks = 0;   // (look-back words it holds)
  uint32_t tcp_epoch = 0;         // the plan's epoch (its words are cleared when it wraps)
  mgenx::DevBuf rx_ws;            // rx-persist workspace
  uint64_t* tcp_host_dev = nullptr;
  int unpack_variant = 0;          // diagnostic kernel ablation (mgenx_set_tuning)
  int unpack_last = 0;             // MGENX_UNPACK_K_* of the last mgenx_unpack_batch
  int pack_variant = 0;
  mgenx::DevBuf bl[5];             // mgenx_convert_binary_log: records, lines, pairs, report text
  mgenx::DevBuf snap;              // mgenx_pcap_snap: per-packet sizes + scan scratch
  mgenx::DevBuf defrag;            // mgenx_pcap_defrag: per-packet arrays + sort / scan scratch
  mgenx::DevBuf ptcp;              // mgenx_pcap_tcp: per-packet arrays + sort / scan scratch
  mgenx::DevBuf tcpf;              // mgenx_tcp_frame: per-record arrays + sort scratch
  mgenx::DevBuf lp;                // mgenx_text_index / mgenx_log_parse_text: per-line scratch
  bool rand_ready = false;
  uint32_t rand_time = 0;
  std::vector<mgenx_worker*> workers;  // live workers on this context (stopped by ctx destroy)
  char err[256] = {0};
};

namespace mgenx {

inline int set_err(mgenx_ctx* c, hipError_t e, const char* where) {
  if (c) snprintf(c->err, sizeof(c->err), "%s: %s", where, hipGetErrorString(e));
  return MGENX_EDEVICE;
}

// ---- mgenx_worker_host.hip ----
// the wave stopped and the device resources freed; the handle stays (ctx = null)
void worker_detach(mgenx_worker* w);

// ---- mgenx_api.hip ----
// Pack for mgenx_pack_batch, mgenx_pack_msgs and the rounds of mgenx_pack_tcp (mgenx_tcp.hip)
int pack_common(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl, const uint32_t* dev_tmpl_crc,
                const mgenx_pack_desc* dev_desc, uint32_t n, const uint8_t* dev_pool,
                uint8_t* dev_slab, uint64_t slab_bytes, const uint64_t* dev_rec_off,
                uint64_t stride, const uint32_t* dev_buf_len, const uint32_t* dev_crc_in,
                uint32_t* dev_out_len, uint32_t* dev_tx_crc, uint32_t* dev_state, uint32_t opts,
                uint32_t fill_time, void* stream, const uint32_t* dev_frag_len = nullptr,
                int frag_ck = 0, const uint32_t* dev_skip = nullptr);

// ---- mgenx_scan.hip ----
mgenx_scan_ws* scan_ws_new();
void scan_ws_free(mgenx_scan_ws* ws);
int scan_run(mgenx_scan_ws* ws, const uint8_t* s, uint64_t nbytes, int mode, uint64_t* rec_off,
             uint32_t* rec_len, uint64_t cap, mgenx_scan_info* info, hipStream_t stream, char* err,
             size_t errn);
int scan_exits_run(mgenx_scan_ws* ws, const uint8_t* s, uint64_t nbytes, int mode, uint64_t window,
                   uint64_t limit, uint64_t* entries, uint64_t* exits, uint32_t cap,
                   uint32_t* candidates, hipStream_t stream, char* err, size_t errn);
int scan_range_run(mgenx_scan_ws* ws, const uint8_t* s, uint64_t nbytes, int mode, uint64_t entry,
                   uint64_t limit, int reuse, uint64_t* rec_off, uint32_t* rec_len, uint64_t cap,
                   mgenx_scan_info* info, hipStream_t stream, char* err, size_t errn);

// ---- mgenx_analytic.hip ----
mgenx_flow_ws* flow_ws_new();
void flow_ws_free(mgenx_flow_ws* ws);
int flow_init_run(mgenx_flow_state* flows, uint32_t n_flows, double window, hipStream_t stream);
int flow_export_run(const mgenx_flow_state* flows, uint32_t n_flows, mgenx_flow_counters* out,
                    hipStream_t stream);
int flow_reduce_run(mgenx_flow_ws* ws, const uint32_t* flow_idx, const uint32_t* seq,
                    const uint32_t* txs, const uint32_t* txu, const uint16_t* len,
                    const mgenx_rec* rows, const uint32_t* rxs, const uint32_t* rxu, uint32_t n,
                    mgenx_flow_state* flows, uint32_t n_flows, mgenx_flow_report* reports,
                    uint32_t per_flow, uint32_t* report_count, uint32_t* report_rec,
                    hipStream_t stream, char* err, size_t errn);
size_t flow_sort_ws(uint32_t n, uint32_t n_flows);
int flow_sort_run(void* mem, const uint32_t* flow_idx, uint32_t n, uint32_t n_flows,
                  const uint32_t** keys, const uint32_t** order, const uint32_t** bnd,
                  hipStream_t stream, char* err, size_t errn);

// ---- mgenx_flowdist.hip, mgenx_flowseries.hip, mgenx_flowquant.hip, mgenx_flowclock.hip,
// ---- mgenx_match.hip, mgenx_matchmulti.hip ----
int flow_dist_init_run(struct mgenx_flow_dist* dist, uint64_t* hist, uint32_t n_flows,
                       hipStream_t stream);
// The passes mgenx_flow_dist and mgenx_flow_series share: the stable sort by flow (keys / order /
// bnd as flow_sort_run leaves them), the packed records rec[i] of the input order, and scan[c],
// the largest seq of chunk c's last flow over chunk c and the chunks before it that this flow
// fills.  mem: flow_prep_ws(n, n_flows) bytes of device memory, 256-B aligned; n, n_flows >= 1.
size_t flow_prep_ws(uint32_t n, uint32_t n_flows);
int flow_prep_run(void* mem, const uint32_t* flow_idx, const uint32_t* seq, const uint32_t* txs,
                  const uint32_t* txu, const uint16_t* len, const uint32_t* rxs,
                  const uint32_t* rxu, uint32_t n, uint32_t n_flows, const uint32_t** keys,
                  const uint32_t** order, const uint32_t** bnd, const DistRec** rec,
                  const int64_t** scan, hipStream_t stream, char* err, size_t errn);
int flow_dist_run(DevBuf& ws, const uint32_t* flow_idx, const uint32_t* seq, const uint32_t* txs,
                  const uint32_t* txu, const uint16_t* len, const uint32_t* rxs,
                  const uint32_t* rxu, uint32_t n, struct mgenx_flow_dist* dist, uint64_t* hist,
                  uint32_t n_flows, hipStream_t stream, char* err, size_t errn);
int flow_dist_quantiles_run(const struct mgenx_flow_dist* dist, const uint64_t* hist,
                            uint32_t n_flows, const uint32_t* permille, uint32_t n_q, int64_t* out,
                            hipStream_t stream);
int flow_series_init_run(struct mgenx_flow_series_state* state, struct mgenx_flow_series_bin* bins,
                         uint32_t n_flows, uint32_t n_bins, hipStream_t stream);
int flow_series_run(DevBuf& ws, const uint32_t* flow_idx, const uint32_t* seq, const uint32_t* txs,
                    const uint32_t* txu, const uint16_t* len, const uint32_t* rxs,
                    const uint32_t* rxu, uint32_t n, int64_t t0, uint64_t width, uint32_t n_bins,
                    struct mgenx_flow_series_state* state, struct mgenx_flow_series_bin* bins,
                    uint32_t n_flows, hipStream_t stream, char* err, size_t errn);
// n_flows >= 1, n_flows * n_bins < 2^31, 1 <= n_q <= MGENX_FLOW_SERIES_MAX_Q, n < 2^31; permille is
// a host array.  cu_count sizes the grids that walk the tier lists.
int flow_quant_run(DevBuf& ws, int cu_count, const uint32_t* flow_idx, const uint32_t* txs,
                   const uint32_t* txu, const uint32_t* rxs, const uint32_t* rxu, uint32_t n,
                   int64_t t0, uint64_t width, uint32_t n_bins, uint32_t n_flows,
                   const uint32_t* permille, uint32_t n_q, int64_t* out, hipStream_t stream,
                   char* err, size_t errn);
// mgenx_flowclock.hip: n_flows >= 1; n, n_flows < 2^31; resid optional, sec_out / usec_out both
// or neither.  cu_count sizes the grids that walk the flows.
int flow_clock_run(DevBuf& ws, int cu_count, const uint32_t* flow_idx, const uint32_t* txs,
                   const uint32_t* txu, const uint32_t* rxs, const uint32_t* rxu, uint32_t n,
                   uint32_t n_flows, uint32_t opts, struct mgenx_flow_clock* flows, int64_t* resid,
                   uint32_t* sec_out, uint32_t* usec_out, hipStream_t stream, char* err,
                   size_t errn);
int match_side_run(const uint8_t* event, const uint8_t* status, const mgenx_addr* src, uint32_t n,
                   uint32_t want_event, mgenx_addr* src_out, uint8_t* err_out, hipStream_t stream);
int msg_match_run(DevBuf& ws, const uint32_t* s_flow, const uint32_t* s_seq, const uint32_t* s_sec,
                  const uint32_t* s_usec, const uint32_t* s_len, uint32_t ns,
                  const uint32_t* r_flow, const uint32_t* r_seq, const uint32_t* r_txs,
                  const uint32_t* r_txu, const uint32_t* r_rxs, const uint32_t* r_rxu, uint32_t nr,
                  uint32_t n_flows, uint32_t opts, uint32_t* send_rx_count, uint32_t* send_first_rx,
                  uint32_t* recv_send, struct mgenx_flow_match* flows,
                  struct mgenx_match_stats* stats, const mgenx_match_timeline* tl,
                  hipStream_t stream, char* err, size_t errn);
// mgenx_matchmulti.hip: ns, nr <= 2^30; 1 <= n_rcv <= 64; n_flows * n_rcv, n_flows * n_bins < 2^31
int msg_match_multi_run(DevBuf& ws, const uint32_t* s_flow, const uint32_t* s_seq,
                        const uint32_t* s_sec, const uint32_t* s_usec, const uint32_t* s_len,
                        uint32_t ns, const uint32_t* r_flow, const uint32_t* r_seq,
                        const uint32_t* r_txs, const uint32_t* r_txu, const uint32_t* r_rxs,
                        const uint32_t* r_rxu, const uint32_t* r_rcv, uint32_t nr, uint32_t n_rcv,
                        uint32_t n_flows, uint32_t opts, uint64_t* send_mask, uint32_t* recv_send,
                        uint8_t* recv_first, struct mgenx_rcv_cell* cells,
                        struct mgenx_flow_fanout* fanout, struct mgenx_match_stats* stats,
                        const mgenx_multi_timeline* tl, const mgenx_multi_loss* lx,
                        hipStream_t stream, char* err, size_t errn);
// mgenx_matchloss.hip: the loss runs and the pair matrix of mgenx_msg_match_multi_ex, run by
// msg_match_multi_run after its main pass on what the join holds by then.  lx has at least one
// part on.  mem: multi_loss_ws(ns, n_flows, n_rcv) bytes of device memory, 256-B aligned; its
// first piece, multi_loss_rank(mem), takes every owner's rank per sorted position (ns words).
// account false (no send record or no flow): only the empty values are written.
struct MultiLossIn {
  const uint32_t *keys, *order, *bnd, *own;   // flow_sort_run's and match_mark_kernel's
  const uint64_t *send_mask, *minp, *maxp;    // [ns], [n_cells], [n_cells]
  const struct mgenx_flow_fanout* fanout;     // sent complete
  const uint32_t *t_sec, *t_usec;             // the send stamps
  uint32_t ns, n_flows, n_rcv;
};
size_t multi_loss_ws(uint32_t ns, uint32_t n_flows, uint32_t n_rcv);
uint32_t* multi_loss_rank(void* mem);
int multi_loss_run(void* mem, const MultiLossIn& in, const mgenx_multi_loss* lx, bool account,
                   hipStream_t stream, char* err, size_t errn);

// ---- mgenx_log.hip ----
mgenx_log_ws* log_ws_new();
void log_ws_free(mgenx_log_ws* ws);
int log_recv_run(mgenx_log_ws* ws, bool binary, const uint8_t* slab, uint64_t slab_bytes,
                 const uint64_t* rec_off, const uint32_t* rec_len, uint64_t stride,
                 const mgenx_cols* cols, const mgenx_addr* src, const uint32_t* rx_sec,
                 const uint32_t* rx_usec, const int32_t* ttl, uint32_t n, int protocol,
                 uint32_t opts, char* text, uint64_t text_cap, uint64_t* line_off,
                 hipStream_t stream, char* err, size_t errn);
int report_build_run(const mgenx_flow_report* reps, uint32_t n_flows, uint32_t per_flow,
                     const uint32_t* count, const mgenx_report_key* keys, uint8_t* sign,
                     const double* offset, const double* rq, uint8_t* items, uint8_t* item_len,
                     hipStream_t stream);
int text_interleave_run(mgenx_log_ws* ws, const mgenx_text_src* srcs, uint32_t n_src,
                        uint32_t n_rec, char* out, uint64_t cap, uint64_t* rec_off,
                        hipStream_t stream, char* err, size_t errn);
int binlog_parse_exec(const uint8_t* buf, const uint64_t* rec_off, uint32_t n, uint64_t* msg_off,
                      uint32_t* msg_len, mgenx_addr* src, uint32_t* ev_sec, uint32_t* ev_usec,
                      uint32_t* aux, uint8_t* kind, uint8_t* proto, hipStream_t stream);
int binlog_lines_exec(mgenx_log_ws* ws, const uint8_t* buf, const uint64_t* rec_off, uint32_t n,
                      uint64_t* msg_off, uint32_t* msg_len, mgenx_addr* src, uint32_t* ev_sec,
                      uint32_t* ev_usec, uint32_t* aux, uint8_t* kind, uint8_t* proto,
                      const mgenx_cols* cols, uint32_t log_rx, uint32_t flush, uint32_t opts,
                      char* text, uint64_t cap, uint64_t* line_off, hipStream_t stream, char* err,
                      size_t errn);
int report_lines(mgenx_log_ws* ws, const uint8_t* items, const mgenx_flow_report* reps,
                 const uint32_t* count, uint32_t per_flow, const uint64_t* pairs,
                 const uint8_t* slab, const mgenx_addr* reporter, const uint32_t* rx_sec,
                 const uint32_t* rx_usec, uint32_t n, uint32_t opts, const double* rq, char* text,
                 uint64_t cap, uint64_t* line_off, hipStream_t stream, char* err, size_t errn);
int data_walk_exec(mgenx_log_ws* ws, const uint8_t* slab, const uint64_t* rec_off, uint64_t stride,
                   const mgenx_cols* cols, uint32_t n, uint32_t opts, const double* rq,
                   uint8_t* status, uint8_t* needs_host, uint32_t* cmds, uint32_t cmd_cap,
                   uint64_t* reps, uint32_t rep_cap, uint32_t* totals, hipStream_t stream,
                   char* err, size_t errn);
int log_send_exec(mgenx_log_ws* ws, const mgenx_flow_tmpl* tmpl, const mgenx_pack_desc* desc,
                  const uint16_t* src_port, const uint32_t* out_len, const uint32_t* msg_total,
                  const uint8_t* slab, uint64_t slab_bytes, const uint64_t* rec_off,
                  uint64_t stride, uint32_t n, int protocol, uint32_t opts, bool binary,
                  uint8_t* out, uint64_t out_cap, uint64_t* pos, hipStream_t stream, char* err,
                  size_t errn);

// ---- mgenx_logparse.hip ----
size_t text_index_ws(uint64_t nbytes);
int text_index_run(void* ws, const uint8_t* text, uint64_t nbytes, uint64_t* line_off, uint64_t cap,
                   uint64_t* n_lines, hipStream_t stream, char* err, size_t errn);
size_t log_parse_ws(uint32_t n);
int log_parse_run(void* ws, const uint8_t* text, uint64_t nbytes, const uint64_t* line_off,
                  uint32_t n, uint32_t opts, uint32_t day_base, const mgenx_logparse_out* out,
                  hipStream_t stream, char* err, size_t errn);

}  // namespace mgenx
