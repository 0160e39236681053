/*
 * mgenx_diag.h -- diagnostics of libmgenx_diag.so (NOT part of the product ABI).
 *
 * libmgenx_diag.so is built from the same sources as libmgenx.so with the kernel ablation
 * variants and the memory-pattern probes compiled in; benchmark and tuning scripts load it
 * (mgen_amd.Engine(diag=True)).  The product library exports none of these symbols.
 */
#ifndef MGENX_DIAG_H
#define MGENX_DIAG_H

#include "mgenx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning knobs (per context; for benchmarking kernel variants).  MGENX_TUNE_UNPACK_VARIANT:
 * 0 = the product dispatch.  The other values are listed in one table, kUnpackVariants in
 * mgen_amd/csrc/mgenx_unpack.hip, each with the kind of batch it applies to and a
 * description.  They are of three kinds: ablations of a product kernel (what bounds it: loads
 * only, no tail, no stores, stores to a scratch line, the other cache policy), a product
 * kernel forced onto a batch the dispatch would route elsewhere, and the few shapes a
 * committed test or script still runs.  A variant that does not apply to the batch (or a
 * number not in the table) leaves the batch to the long / var / general kernels. */
#define MGENX_TUNE_UNPACK_VARIANT 1
/* MGENX_TUNE_PACK_VARIANT: 0 = product; ablations 1 = no unit stores, 2 = no CRC work, 3-6
 * store-scheme ablations, 7-9 = grid x2..x4, 10 = the meta waves never help the joint
 * store.  (Env MGENX_PACK_GRID: the grid, diagnostics build only.) */
#define MGENX_TUNE_PACK_VARIANT 2
int mgenx_set_tuning(mgenx_ctx* ctx, int key, int value);
/* Diagnostic: plain 16-B-per-lane streaming read of `bytes` (the achievable-HBM reference
 * next to the roofline); dev_scratch holds `grid` words. */
int mgenx_diag_stream_read(mgenx_ctx* ctx, const uint8_t* dev_data, uint64_t bytes,
                           uint32_t* dev_scratch, int grid, void* stream);
/* Diagnostic: the same read at `width` bytes per lane (4, 8 or 24), coalesced -- FETCH_SIZE
 * calibration for the config-4 kernels' access shapes. */
int mgenx_diag_stream_read_w(mgenx_ctx* ctx, const uint8_t* dev_data, uint64_t bytes,
                             uint32_t* dev_scratch, int grid, int width, void* stream);
/* Diagnostic: the fixed-length unpack's memory pattern without its compute -- waves take
 * 16-KiB groups of `data` round-robin (16 loads of 1 KiB each, consumed by XOR) and, when
 * `mode` & 1, store 512 B per group to dev_out (bytes / 32 bytes); `mode` & 2: the stores
 * are write-through (sc1). */
int mgenx_diag_group_rw(mgenx_ctx* ctx, const uint8_t* dev_data, uint64_t bytes,
                        uint8_t* dev_out, int mode, void* stream);

/* Diagnostic: s_memtime phase cycles of the analytics kernels' first wave: n == 10
 * flow_update_kernel (detect, bulk, exact, lat' stores, rounds, exact steps, bulk runs, total,
 * restart cycles, restarts); n == 16 flow_order_kernel (8 entries). */
int mgenx_diag_seg_prof(unsigned long long* out, int n);

/* The ordering in front of mgenx_flow_reduce's update, forced (environment, read per call by
 * this library only): MGENX_AN_RADIX=1 the radix sort; MGENX_AN_SCAN1=1 / 0 the counting sort's
 * single-pass scan / its three kernels (colpart, colbase, colscan); MGENX_AN_TILE=4096 / 4608
 * the tile size (4608 only where its LDS fits: n_flows <= 1222).
 * MGENX_AN_C1_GIVEUP=M (M >= 1): blocks j > 0 of the single-pass scan with j mod M == M - 1 skip
 * their look-back poll and take the give-up branch (the block sums the histogram itself); it
 * shortens a wait and never lengthens one.  MGENX_AN_C1_WRAP=1: a context's first single-pass
 * scan starts at epoch kC1Epochs - 2, so its third call restarts the epochs.
 * mgenx_diag_c1_giveups: waits for the device, then *out = the blocks that took the give-up
 * branch since the last call of this function (forced or not), and clears the count. */
int mgenx_diag_c1_giveups(unsigned long long* out);

/* Diagnostic: the resident worker's own time for its last Unpack / receive request, in 10-ns
 * ticks from the poll that saw it: header parsed, checksum done, reply stored; out[3] = the
 * request number they belong to; out[4], out[5] = shader clocks (s_memtime) to the parse and
 * to the reply (out[7] = the request number); out holds 8 words. */
int mgenx_diag_worker_stamps(const mgenx_worker* w, uint32_t* out);

/* Diagnostic: s_memtime stamps of the scan's chain kernel (scan_chain_kernel), thread 0 of
 * groups 0..63, 8 per group: start, counts prefix, marks, H list, look-back, end; out holds
 * 512 words. */
int mgenx_diag_chain_prof(unsigned long long* out);

/* Diagnostic: the segmented inclusive scan of the per-flow passes (mgen_amd/csrc/
 * mgenx_blockscan.hpp) alone: one workgroup of 1024 lanes, one scan.  dev_head: 1024 words, a
 * non-zero word starts a segment at its lane.  dev_open: null (the scan is then asked for no
 * open flags) or 1024 words that receive 1 where no segment starts at or before the lane.
 *   kind 0: dev_val and dev_out 1024 x uint32_t, the sum modulo 2^32;
 *   kind 1: dev_val and dev_out 1024 x int64_t, the maximum;
 *   kind 2: dev_val 1024 x uint64_t, dev_out 1024 x 12 x uint64_t: lane t enters the 96-B value
 *           whose field k = 0..11 is dev_val[t] * (2 k + 1) + k modulo 2^64; fields with
 *           k % 3 == 0 are summed modulo 2^64, k % 3 == 1 take the minimum and k % 3 == 2 the
 *           maximum, both as int64_t. */
int mgenx_diag_blockscan(int kind, const void* dev_val, const uint32_t* dev_head, void* dev_out,
                         uint32_t* dev_open, void* stream);
/* Diagnostic: the same scan over n entries by one workgroup, 1024 entries a round, as the
 * one-workgroup carry kernels run it.  dev_val, dev_head and dev_out hold n entries.
 *   kind 0: uint32_t, the segmented sum modulo 2^32;  kind 1: int64_t, the segmented maximum;
 *   kind 2: uint32_t, one sum over all entries (dev_head is not read and may be null). */
int mgenx_diag_chunk_carry(int kind, const void* dev_val, const uint32_t* dev_head, uint32_t n,
                           void* dev_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
