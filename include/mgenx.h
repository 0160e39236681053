/*
 * mgenx.h -- C ABI of the MI355X MgenMsg pack/parse engine (libmgenx.so).
 *
 * Plain pointers and sizes only.  Every `dev_*` pointer is device (HBM) memory; the
 * caller owns every buffer (the library never allocates or frees them, matching the
 * reference's caller-owned UINT32 buffers, mgenTransport.cpp:944,1023).  Calls are
 * asynchronous on the caller's hipStream_t (passed as void*), never synchronise and
 * never allocate, so they can be captured in a hipGraph.  One mgenx_ctx per device.
 * Exceptions, each stated at its entry point: calls whose output size decides later
 * launches (the stream scans, mgenx_pack_tcp) read small results back, and calls with
 * scratch grow it (hipMalloc) the first time a larger batch arrives -- warm them up with
 * the largest batch before capturing a graph.  The log / report / walk formatters keep
 * one workspace per stream; the stream scans, mgenx_flow_reduce, mgenx_flow_dist,
 * mgenx_flow_series, mgenx_flow_series_quantiles, mgenx_flow_clock, mgenx_pack_tcp and mgenx_tcp_rx_persist keep one per
 * context, so those run on one stream
 * at a time per context (one context per concurrent stream).
 *
 * Return value: 0 = launched, <0 = argument/launch error (MGENX_E*).  Per-record
 * outcomes go to the `err` column with MgenMsg::Error codes (include/mgenMsg.h:63-70).
 *
 * Reference interfaces replaced (USNavalResearchLaboratory/mgen):
 *   mgenx_unpack_batch  <- MgenMsg::Unpack            include/mgenMsg.h:110
 *                          + receive CRC check        src/common/mgenTransport.cpp:958-975
 *                          (SINK 2092-2112, TCP CalcRxChecksum 1516-1564)
 *   mgenx_pack_batch    <- MgenMsg::Pack              include/mgenMsg.h:108
 *                          + MgenMsg::WriteChecksum   include/mgenMsg.h:111
 *                          + UDP/SINK send sequence   src/common/mgenTransport.cpp:1011-1031
 *   mgenx_stream_scan   <- TCP/SINK record framing    src/common/mgenTransport.cpp:1683-1760,
 *                                                     mgenAppSinkTransport.cpp:369-434
 *   mgenx_flow_reduce   <- MgenAnalytic::Update       include/mgenAnalytic.h:91-94
 *                          via Mgen::UpdateRecvAnalytics src/common/mgen.cpp:1027-1070
 *   mgenx_pack_msgs     <- MgenMsg::Pack alone (TCP fragments, the MgenMsg shim)
 *   mgenx_crc32_update  <- MgenMsg::ComputeCRC32      include/mgenMsg.h:201-203
 *   mgenx_allreduce_flows  the per-flow counter merge of flow-sharded analytics (RCCL)
 *   mgenx_flow_lookup   <- MgenAnalyticTable::FindFlow  include/mgenAnalytic.h:387
 *   mgenx_flow_dist     no reference code: the latency distribution, jitter and re-ordering
 *                       the manual reads logs for (doc/mgen.xml:3399-3450)
 *   mgenx_flow_series   no reference code: rate, loss, latency and jitter per flow and window
 *                       of receive time, what the manual plots with trpr (doc/mgen.xml:3452-3457)
 *   mgenx_flow_series_quantiles   no reference code: the exact latency percentiles of those windows
 *   mgenx_flow_clock    no reference code: per-flow clock offset and skew removed from the
 *                       one-way latencies (Moon, Skelly, Towsley, INFOCOM 1999)
 */
#ifndef MGENX_H
#define MGENX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGENX_ABI_VERSION 1

/* ---- status codes ---- */
#define MGENX_OK          0
#define MGENX_EINVAL     -1   /* bad argument (null pointer, zero stride ...) */
#define MGENX_EDEVICE    -2   /* HIP error (no device, launch failure) */
#define MGENX_ENOMEM     -3   /* context workspace allocation failed (create only) */
#define MGENX_ENOSPC     -4   /* a caller-given output window is too small: nothing was
                                 written, the need is reported (mgenx_pcap_defrag) */

/* ---- wire constants (include/mgenGlobals.h:70-80, include/mgenMsg.h:60-103) ---- */
#define MGENX_MIN_SIZE        28
#define MGENX_MAX_SIZE        8192
#define MGENX_TX_BUFFER_SIZE  8192
#define MGENX_MAX_FRAG_SIZE   65535
#define MGENX_FLAG_CONTINUES      0x01
#define MGENX_FLAG_END_OF_MSG     0x02
#define MGENX_FLAG_CHECKSUM       0x04
#define MGENX_FLAG_LAST_BUFFER    0x08
#define MGENX_FLAG_CHECKSUM_ERROR 0x10
#define MGENX_ERROR_NONE      0
#define MGENX_ERROR_VERSION   1
#define MGENX_ERROR_CHECKSUM  2
#define MGENX_ERROR_LENGTH    3
#define MGENX_ERROR_DSTADDR   4
#define MGENX_ERROR_OOB       0x80  /* record lies outside the slab: not touched */
#define MGENX_ERROR_RERR_NONE 0x40  /* log formatters only: a RERR event of a message whose
                                       error is ERROR_NONE ("type>none", mgenMsg.cpp:716) */

/* ---- unpack options ---- */
#define MGENX_OPT_CHECKSUM_FORCE  0x1  /* Mgen checksum_force (mgen.cpp:2076-2087) */
#define MGENX_OPT_TCP             0x2  /* TCP receive rules: Unpack sees min(len, 8192)
                                          bytes; a CRC mismatch also sets
                                          CHECKSUM_ERROR in flags (mgenTransport.cpp:1555) */
#define MGENX_OPT_SKIP_CRC        0x4  /* header-only decode (benchmark mode; NOT the
                                          reference receive path) */

typedef struct mgenx_ctx mgenx_ctx;

int  mgenx_abi_version(void);
int  mgenx_ctx_create(int device, mgenx_ctx** out);
int  mgenx_ctx_destroy(mgenx_ctx* ctx);
/* Last HIP error string seen by this context (static storage). */
const char* mgenx_last_error(const mgenx_ctx* ctx);
/* The HIP device of a context. */
int  mgenx_ctx_device(const mgenx_ctx* ctx);

/* One decoded record's core fields, packed (32 B): the row-major alternative to the core
 * columns -- the batch analogue of one unpacked MgenMsg object.  Written whole lines at a
 * time (16 records = 512 contiguous bytes per wave store), it is the fastest output. */
typedef struct {
    uint32_t flow_id, seq_num, tx_sec, tx_usec;
    uint32_t dst_addr4;              /* first 4 address bytes, in wire order in memory */
    uint16_t msg_len, dst_port;
    uint16_t payload_len;
    uint8_t  flags, err;             /* err: MgenMsg::Error (+ MGENX_ERROR_OOB) */
    uint8_t  dst_type, dst_len, payload_type, gps_status;
} mgenx_rec;                         /* 32 bytes */

/* ------------------------------------------------------------------ */
/* Columns written by unpack: the MgenMsg state after Unpack() on a    */
/* fresh MgenMsg (mgenMsg.cpp:315-500), one element per record.        */
/* Core columns (32 bytes per record) are required; extended columns   */
/* may be NULL (not written).                                          */
/* ------------------------------------------------------------------ */
typedef struct {
    /* core */
    uint32_t* flow_id;
    uint32_t* seq_num;
    uint32_t* tx_sec;
    uint32_t* tx_usec;
    uint16_t* msg_len;
    uint16_t* dst_port;
    uint8_t*  flags;
    uint8_t*  err;          /* MgenMsg::Error (+ MGENX_ERROR_OOB) */
    uint8_t*  dst_type;     /* ProtoAddress type (0 = not decoded, 1 IPv4, 2 IPv6) */
    uint8_t*  dst_len;      /* dst address length byte from the wire */
    uint32_t* dst_addr4;    /* first 4 address bytes, in wire order in memory */
    uint16_t* payload_len;
    uint8_t*  payload_type;
    uint8_t*  gps_status;
    /* extended (optional) */
    uint16_t* hdr_len;      /* packet_header_len */
    uint32_t* payload_off;  /* payload_data - record start = (hdr_len/4)*4 */
    uint16_t* host_port;
    uint8_t*  host_type;
    uint8_t*  host_len;
    uint8_t*  host_addr;    /* 16 bytes per record */
    uint8_t*  dst_addr;     /* 16 bytes per record */
    uint32_t* lat_raw;      /* ntohl(latitude word): degrees = raw/60000 - 180 */
    uint32_t* lon_raw;
    int32_t*  alt;
    /* row-major output: when set, unpack writes these 32-B records instead of the core
     * columns (which may then be NULL); extended columns still go to their arrays */
    mgenx_rec* rows;
    /* extended (optional): MGENX_DEC_* mask of the MgenMsg members this record's Unpack
     * assigned.  Unpack leaves the other members as they were, which matters on a reused
     * MgenMsg (the TCP receiver's rx_msg, mgenTransport.cpp:1501-1513) and for the shim. */
    uint8_t*  decoded;
} mgenx_cols;

#define MGENX_DEC_MSGLEN 0x01  /* msg_len, version (bufferLen >= MIN_SIZE, mgenMsg.cpp:323-336) */
#define MGENX_DEC_BASE   0x02  /* flags, flow_id, seq_num, tx_time (version 2, :345-366) */
#define MGENX_DEC_DST    0x04  /* dst_addr and port (dst type IPv4/IPv6, :373-398) */
#define MGENX_DEC_HDRLEN 0x08  /* packet_header_len (:437-487) */
#define MGENX_DEC_HOST   0x10  /* host_addr set (valid type, fits: :425-431) */
#define MGENX_DEC_GPS    0x20  /* latitude, longitude, altitude, gps_status (:449-465) */
#define MGENX_DEC_PTYPE  0x40  /* payload_type (:472-475) */
#define MGENX_DEC_PLEN   0x80  /* payload_len, payload_data (:482-497) */

/* Decode n records.  Record i starts at dev_slab + (dev_rec_off ? dev_rec_off[i] :
 * i*stride) and is (dev_rec_len ? dev_rec_len[i] : fixed_len) bytes long (the receive
 * length: recvfrom's len for UDP, the framed msg_len for TCP/SINK).  Records extending
 * past slab_bytes are flagged MGENX_ERROR_OOB and not read. */
int mgenx_unpack_batch(mgenx_ctx* ctx, const uint8_t* dev_slab, uint64_t slab_bytes,
                       const uint64_t* dev_rec_off, uint64_t stride,
                       const uint32_t* dev_rec_len, uint32_t fixed_len, uint32_t n,
                       const mgenx_cols* cols, uint32_t opts, void* stream);

/* Which kernel the last mgenx_unpack_batch on this context launched (host-side record of
 * the dispatch; a test and profiling aid -- the choice follows the layout, the options and
 * the batch size, never the data).  0 before the first call. */
#define MGENX_UNPACK_K_HEADER     1  /* MGENX_OPT_SKIP_CRC: header-only decode */
#define MGENX_UNPACK_K_GENERAL    2  /* any layout, one group of 16 records per wave */
#define MGENX_UNPACK_K_VAR        3  /* per-record lengths, >= 2 tiles of 64 records per
                                        wave: length-ranked groups, load ring (config 3) */
#define MGENX_UNPACK_K_FIXED      4  /* fixed stride, one length in [65, 1024] */
#define MGENX_UNPACK_K_FIXED_RING 5  /* fixed 512 / 1024-B records into rows (config 2) */
#define MGENX_UNPACK_K_OTHER      6  /* a diagnostics-build ablation */
#define MGENX_UNPACK_K_LONG       7  /* mean record >= 4 KiB (TCP streams): a wave per record */
int mgenx_unpack_last_kernel(const mgenx_ctx* ctx);

/* ------------------------------------------------------------------ */
/* Pack.  A per-flow template table holds what MgenFlow::SendMessage    */
/* takes from flow state (mgenFlow.cpp:946-983, 1039-1129); a 20-byte   */
/* descriptor per record holds the per-message fields.                 */
/* ------------------------------------------------------------------ */
typedef struct {
    uint32_t flow_id;
    uint8_t  dst_type, dst_len; uint16_t dst_port;    /* dst_type: 1 IPv4, 2 IPv6 */
    uint8_t  dst_addr[16];
    uint8_t  host_type, host_len; uint16_t host_port;  /* host_type 0 = invalid (no host) */
    uint8_t  host_addr[16];
    uint32_t lat_raw, lon_raw;   /* (UINT32)((deg + 180.0) * 60000.0), mgenMsg.cpp:221,225 */
    int32_t  alt;
    uint8_t  gps_status, payload_type; uint16_t payload_len;
    uint32_t payload_off;        /* into dev_pool */
    uint8_t  has_payload, rsv0; uint16_t rsv1;
} mgenx_flow_tmpl;               /* 68 bytes */

typedef struct {
    uint32_t tmpl;               /* index into the template table */
    uint32_t seq_num, tx_sec, tx_usec;
    uint16_t msg_len;            /* MgenMsg::msg_len = the record length */
    uint8_t  flags;              /* MgenMsg flags before the transport sets LAST_BUFFER */
    uint8_t  rsv;
} mgenx_pack_desc;               /* 20 bytes */

#define MGENX_PACK_CHECKSUM    0x1   /* Mgen checksum_enable */
#define MGENX_PACK_RANDOM_FILL 0x2   /* the RANDOM_FILL build: fill = glibc rand() bytes
                                        after srand(fill_time) (mgenMsg.cpp:277-292) */
#define MGENX_PACK_RAW         0x4   /* (set by mgenx_pack_msgs) MgenMsg::Pack alone */

/* Pack n records with the UDP/SINK send sequence (LAST_BUFFER, Pack, WriteChecksum)
 * into dev_slab at dev_rec_off[i] (or i*stride).  dev_out_len[i] = Pack()'s return
 * (0 = MSG_SEND_FAILED).  Template CRCs must be prepared by mgenx_pack_prepare when
 * the template table or pool changes. */
int mgenx_pack_prepare(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl, uint32_t n_tmpl,
                       const uint8_t* dev_pool, uint32_t* dev_tmpl_crc, void* stream);
/* Select the RANDOM_FILL stream (time(NULL) value the reference would seed srand with).
 * Host-side table setup (synchronous); call when fill_time changes. */
int mgenx_set_fill_time(mgenx_ctx* ctx, uint32_t fill_time);

int mgenx_pack_batch(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                     const uint32_t* dev_tmpl_crc, const mgenx_pack_desc* dev_desc, uint32_t n,
                     const uint8_t* dev_pool, uint8_t* dev_slab, uint64_t slab_bytes,
                     const uint64_t* dev_rec_off, uint64_t stride, uint32_t* dev_out_len,
                     uint32_t opts, uint32_t fill_time, void* stream);

/* MgenMsg::Pack alone (mgenMsg.cpp:83-313), without the UDP send sequence: the
 * descriptor's flags are used as given (the caller sets LAST_BUFFER or not: with it the CRC
 * runs over bufferLen - 4 bytes, without it over bufferLen), no trailer is written
 * (MgenMsg::WriteChecksum is the caller's), and the MgenMsg state Pack leaves is returned:
 *   dev_buf_len[i]  (optional) Pack's bufferLen argument; NULL = the descriptor's msg_len
 *                   (the TCP fragment path packs msg_len 16384 into bufferLen 8192/8188,
 *                   mgenTransport.cpp:1915-1926);
 *   dev_crc_in[i]   (optional) the tx_checksum argument on entry (NULL = 0);
 *   dev_tx_crc[i]   (optional) tx_checksum after Pack (unchanged when Pack returned early);
 *   dev_state[i]    (optional) packet_header_len | flags member << 16 after Pack
 *                   (packet_header_len 0xFFFF when Pack failed: not assigned).
 * A failed Pack (return 0) writes no bytes (the reference leaves a partial header). */
int mgenx_pack_msgs(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                    const uint32_t* dev_tmpl_crc, const mgenx_pack_desc* dev_desc, uint32_t n,
                    const uint8_t* dev_pool, uint8_t* dev_slab, uint64_t slab_bytes,
                    const uint64_t* dev_rec_off, uint64_t stride, const uint32_t* dev_buf_len,
                    const uint32_t* dev_crc_in, uint32_t* dev_out_len, uint32_t* dev_tx_crc,
                    uint32_t* dev_state, uint32_t opts, uint32_t fill_time, void* stream);

/* TCP transmit: the byte stream MgenTcpTransport sends for n messages (SendMessage with
 * GetNextTxFragmentSize / GetNextTxFragment / SetupNextTxBuffer / CalcTxChecksum,
 * src/common/mgenTransport.cpp:1320-1400, 1818-1993), back to back.  dev_msg_total[i] is the
 * message's mgen_msg_len (fragments of <= 65535 bytes past that, CONTINUES / END_OF_MSG);
 * the descriptor's msg_len is ignored.  A fragment over 8192 bytes is one 8-KiB Pack whose
 * buffer is re-sent from its start, the CRC (MGENX_PACK_CHECKSUM) covering every byte
 * before the trailer.  dev_msg_off[i] = the message's offset in the stream (a message whose
 * first Pack fails, or of length 0, takes no bytes); *total_bytes = the stream length.
 * Waits for the plan only (the stream layout decides the launches): it returns once the
 * stream length is known, with the stores still running on `stream` (stream-ordered, as any
 * launch).  When the stream would exceed stream_cap nothing is written, *total_bytes is set
 * and MGENX_EINVAL returned.  A context's TCP transmit calls must all use ONE stream: the plan
 * leaves its verdict in a per-context device word that the queued Pack reads, so a call on
 * another stream could overwrite it before the first call's Pack has read it. */
int mgenx_pack_tcp(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl, const uint32_t* dev_tmpl_crc,
                   const mgenx_pack_desc* dev_desc, const uint32_t* dev_msg_total, uint32_t n,
                   const uint8_t* dev_pool, uint8_t* dev_stream, uint64_t stream_cap,
                   uint64_t* dev_msg_off, uint64_t* total_bytes, uint32_t opts,
                   uint32_t fill_time, void* stream);

/* MgenMsg::ComputeCRC32(checksum, buffer, len) (mgenMsg.cpp:524-541) over n byte ranges:
 * dev_state_out[i] = the running CRC after feeding dev_data[off[i] .. off[i]+len[i]) to
 * dev_state_in[i] (0 restarts from CRC32_XINIT; no final xor). */
int mgenx_crc32_update(mgenx_ctx* ctx, const uint8_t* dev_data, const uint64_t* dev_off,
                       const uint32_t* dev_len, uint32_t n, const uint32_t* dev_state_in,
                       uint32_t* dev_state_out, void* stream);

/* Standard CRC-32 (MgenMsg::ComputeCRC32 from a zero state + CRC32_XOROT) of n
 * byte ranges: out[i] = crc(dev_data[off[i] .. off[i]+len[i])). */
int mgenx_crc32_batch(mgenx_ctx* ctx, const uint8_t* dev_data, const uint64_t* dev_off,
                      const uint32_t* dev_len, uint32_t n, uint32_t* dev_out, void* stream);

/* ---- the resident single-message worker ----
 * For callers that stay one message at a time (an unchanged MgenUdpTransport calls
 * MgenMsg::Unpack once per datagram, mgenTransport.cpp:948-997, and ComputeCRC32 once per
 * message): a batch entry point per message costs a launch, copies and a synchronisation.
 * A worker keeps ONE wave resident on the context's device, polling a mailbox in pinned host
 * memory: a call copies the message into the mailbox, the wave decodes or checksums it and
 * writes the reply back; the call spins until it arrives.  Host buffers in, results out --
 * no device pointers.  The wave exits after idle_ms without a request (the next call
 * relaunches it), on mgenx_worker_stop / mgenx_worker_destroy, and when its context is
 * destroyed (mgenx_ctx_destroy stops and frees every worker created on it; the handle then
 * only accepts mgenx_worker_destroy, other calls return MGENX_EINVAL).  While its wave runs
 * it holds up device-wide synchronisations (hipFree, hipHostFree, hipDeviceSynchronize) until
 * it idles out: the library's own workspace growth ends every worker's wave first (the next
 * call relaunches it); a caller about to synchronise the device calls mgenx_worker_stop.
 * Calls on one worker are serialised by the worker; results equal the batch entry points' on
 * the same bytes.
 *   mgenx_worker_unpack  <- MgenMsg::Unpack (include/mgenMsg.h:110, mgenMsg.cpp:315-500) on a
 *                           fresh MgenMsg: the members it assigned (`decoded`, MGENX_DEC_*) and
 *                           err (MgenMsg::Error; 0 = Unpack returned true); no CRC check
 *   mgenx_worker_crc32   <- MgenMsg::ComputeCRC32 (include/mgenMsg.h:201-203, mgenMsg.cpp:
 *                           524-541): the running checksum in and out
 *   mgenx_worker_recv    <- Unpack + the receive path's ComputeCRC32 in one reply (below)
 *   mgenx_worker_pack    <- MgenMsg::Pack alone (below)
 *   mgenx_worker_flow_update <- MgenAnalytic::Update of one record (below) */
#define MGENX_WORKER_MAX_BYTES 65536u
#define MGENX_WORKER_PACK_MAX  16384u   /* mgenx_worker_pack's largest bufferLen */
typedef struct {
    uint32_t flow_id, seq_num, tx_sec, tx_usec, payload_off;
    uint32_t lat_raw, lon_raw;
    int32_t  alt;
    uint16_t msg_len, dst_port, payload_len, hdr_len, host_port;
    uint8_t  flags, err, dst_type, dst_len, payload_type, gps_status, host_type, host_len;
    uint8_t  decoded, version, rsv[2];
    uint8_t  dst_addr[16], host_addr[16];
} mgenx_unpacked;                    /* 88 bytes */
typedef struct mgenx_worker mgenx_worker;
int mgenx_worker_create(mgenx_ctx* ctx, uint32_t idle_ms, mgenx_worker** out);
int mgenx_worker_destroy(mgenx_worker* w);
int mgenx_worker_stop(mgenx_worker* w);  /* end the wave now (the next call relaunches it) */
/* *flags: MGENX_WORKER_DEVICE_MAILBOX when requests go to fine-grained device memory the host
 * stores into through the BAR (the runtime granted the CPU access), else pinned host memory
 * (environment MGENX_WORKER_HOST_MAILBOX=1 forces the latter). */
#define MGENX_WORKER_DEVICE_MAILBOX 0x1u
int mgenx_worker_info(const mgenx_worker* w, uint32_t* flags);
int mgenx_worker_unpack(mgenx_worker* w, const uint8_t* msg, uint32_t len, mgenx_unpacked* out);
int mgenx_worker_crc32(mgenx_worker* w, const uint8_t* data, uint32_t len, uint32_t state_in,
                       uint32_t* state_out);
/* The UDP / SINK receive path's two calls in one reply (mgenTransport.cpp:958-965,
 * 2092-2100): MgenMsg::Unpack as mgenx_worker_unpack, then -- when Unpack succeeded and `force`
 * (checksum_force) is set or the decoded flags carry CHECKSUM -- ComputeCRC32(0, msg, len - 4):
 * *crc_done = 1 and *crc_state the running CRC the caller then XORs with CRC32_XOROT and
 * compares with the trailer (no final xor here, as ComputeCRC32); else *crc_done = 0. */
int mgenx_worker_recv(mgenx_worker* w, const uint8_t* msg, uint32_t len, uint32_t force,
                      mgenx_unpacked* out, uint32_t* crc_state, uint32_t* crc_done);
/* MgenAnalytic::Update (include/mgenAnalytic.h:91-94, mgenAnalytic.cpp:74-258) of ONE record
 * on the device flow state dev_flows[slot] (mgenx_flow_init / mgenx_flow_reduce's array; the
 * worker's wave reads and writes it in place).  The wave is NOT on the caller's stream: the
 * stream that last wrote dev_flows (a queued mgenx_flow_reduce or mgenx_flow_init) must be
 * synchronised before this call, and later batch work on dev_flows enqueued only after it
 * returns.  *updated = 1 when the record closed a window, with the report in *report (index =
 * the flow's report number; latency_ave from the window's in-order latency sum).  Equal to
 * mgenx_flow_reduce of the same records one call at a time. */
struct mgenx_flow_state;
struct mgenx_flow_report;
int mgenx_worker_flow_update(mgenx_worker* w, struct mgenx_flow_state* dev_flows, uint32_t slot,
                             uint32_t seq, uint32_t rx_sec, uint32_t rx_usec, uint32_t msg_size,
                             uint32_t tx_sec, uint32_t tx_usec, uint32_t* updated,
                             struct mgenx_flow_report* report);
/* MgenMsg::Pack (include/mgenMsg.h:108, mgenMsg.cpp:83-313) of one message, as mgenx_pack_msgs
 * with n = 1: the message as a template (its payload bytes at `payload`, payload_off ignored)
 * and a descriptor; bufferLen, the tx_checksum argument, MGENX_PACK_CHECKSUM /
 * MGENX_PACK_RANDOM_FILL and the fill time.  out (bufferLen bytes) receives *ret bytes
 * (Pack's return; 0: failed, nothing written); *tx_crc the tx_checksum after; *state
 * packet_header_len | flags << 16.  bufferLen <= MGENX_WORKER_PACK_MAX. */
int mgenx_worker_pack(mgenx_worker* w, const mgenx_flow_tmpl* tmpl, const uint8_t* payload,
                      const mgenx_pack_desc* desc, uint32_t buf_len, uint32_t crc_in,
                      uint32_t opts, uint32_t fill_time, uint8_t* out, uint32_t* ret,
                      uint32_t* tx_crc, uint32_t* state);

/* ---- the TCP receiver's persistent rx_msg ----
 * MgenTcpTransport decodes every message of a connection into ONE MgenMsg (rx_msg,
 * src/common/mgenTransport.cpp:1082): ResetRxMsgState (:1501-1513) zeroes only
 * mgen_msg_len / msg_len / flow_id / seq_num / the error between messages, Unpack runs only
 * while a log file is open (:2016-2028) and assigns members stage by stage (mgenMsg.cpp:
 * 315-500), and the CRC check reads the flags rx_msg holds (:1516-1564).  So a record that
 * stops early keeps the previous record's flags, tx time, destination, header length, GPS
 * position and payload; with no log file nothing is decoded at all (flow id and sequence
 * number stay 0) and the CRC is checked only under checksum_force.
 * mgenx_tcp_rx_persist rewrites n consecutive records of one connection, decoded by
 * mgenx_unpack_batch(MGENX_OPT_TCP) into core + extended columns with `decoded`, into that
 * rx_msg view, in place: every member group a record did not assign comes from the latest
 * earlier record that did, or from *dev_state (rx_msg before the batch; updated to rx_msg
 * after it).  dev_payload_rec[i] (optional) = the record whose bytes the payload member
 * points into (MGENX_RX_PREV: before this batch).  Options:
 *   MGENX_RX_NOLOG  no log file on this connection: no record is decoded (host address
 *                   and gps_status read invalid; the caller unpacks with
 *                   MGENX_OPT_CHECKSUM_FORCE to have the CRC verdicts when it needs them);
 *   MGENX_RX_FORCE  checksum_force (the receiver's setting, for records without flags).
 * Core columns are required (not the row layout). */
#define MGENX_RX_NOLOG 0x1
#define MGENX_RX_FORCE 0x2
#define MGENX_RX_PREV  0xFFFFFFFFu
typedef struct {
    uint32_t tx_sec, tx_usec, lat_raw, lon_raw;
    int32_t  alt;
    uint32_t payload_off;
    uint16_t dst_port, hdr_len, payload_len;
    uint8_t  flags, dst_type, dst_len, payload_type, rsv[2];
    uint8_t  dst_addr[16];
} mgenx_rx_state;                /* 48 bytes; zero = a fresh MgenMsg's members */
int mgenx_tcp_rx_persist(mgenx_ctx* ctx, const uint8_t* dev_slab, const uint64_t* dev_rec_off,
                         const uint32_t* dev_rec_len, uint32_t n, const mgenx_cols* cols,
                         mgenx_rx_state* dev_state, uint32_t* dev_payload_rec, uint32_t opts,
                         void* stream);

/* ---- stream framing (TCP / SINK record boundaries) ----
 * mgenx_stream_scan finds the record chain of a byte stream from offset 0 exactly as the
 * reference receivers frame it -- TCP: MgenTcpTransport::GetRxNumBytes / OnRecvMsg
 * (src/common/mgenTransport.cpp:1683-1760; msg_len < 4 is a stream error that stops the
 * scan); SINK: MgenAppSinkTransport::OnInputReady (src/common/mgenAppSinkTransport.cpp:
 * 369-434; msg_len outside [28, 8192] skips the 2 length bytes) -- and writes the records'
 * offsets and lengths in stream order (the first `cap` of them).  The output feeds
 * mgenx_unpack_batch directly (rec_off / rec_len; MGENX_OPT_TCP for TCP streams).
 * Synchronous on `stream` (the record count decides the launches); the context keeps a
 * workspace that grows with the stream (about 1/32 of its size). */
#define MGENX_SCAN_TCP  0
#define MGENX_SCAN_SINK 1
typedef struct mgenx_scan_info {
  uint64_t n_records;   /* records found (only the first `cap` are written) */
  uint64_t consumed;    /* bytes consumed: offset just past the last whole record/skip */
  int32_t  status;      /* 0 = ok, 1 = TCP record with msg_len < 4 (scan stopped there) */
  uint32_t candidates;  /* diagnostic: plausible starts found by the parallel pass */
  uint64_t resolved;    /* diagnostic: records framed by the sequential resolver */
  uint32_t path;        /* diagnostic: how the chain was found -- 0 lifting (and resolver),
                           1 every candidate a record, 2 the successor-marked hypothesis */
  uint32_t reserved;
} mgenx_scan_info;
int mgenx_stream_scan(mgenx_ctx* ctx, const uint8_t* dev_stream, uint64_t nbytes, int mode,
                      uint64_t* dev_rec_off, uint32_t* dev_rec_len, uint64_t cap,
                      mgenx_scan_info* info, void* stream);

/* ---- sharded framing (one stream split over ranks; no reference counterpart: the
 * reference frames one socket sequentially) ----
 * Rank r owns the records that START in [a_r, b_r) of the global stream and holds the
 * bytes [a_r, min(b_r + MGENX_SCAN_HALO, N)) (a record starting before b_r ends within the
 * halo).  Its chain entry e_r (the first chain position >= a_r) lies below
 * a_r + MGENX_SCAN_HALO.  Protocol (mgen_amd/shard.py):
 *   1. mgenx_stream_scan_exits on the local bytes with window = MGENX_SCAN_HALO and
 *      limit = b_r - a_r: for each candidate entry below the window, where its chain first
 *      reaches >= limit (dev_exits; bit 63 set = the chain leaves the candidate set first,
 *      exit unknown).  Unused rows are ~0.
 *   2. all-gather the (entry, exit) tables; every rank stitches e_0 = 0, e_{r+1} = exit_r(e_r)
 *      identically; a missing or unknown exit is settled by that rank's
 *      mgenx_stream_scan_range (its info.consumed is the exit) and one more all-gather.
 *   3. mgenx_stream_scan_range(entry = e_r - a_r, limit, MGENX_SCAN_REUSE): the rank's
 *      records (local offsets; add a_r for global ones), on the tables of step 1.
 * The union over ranks equals mgenx_stream_scan of the whole stream. */
#define MGENX_SCAN_HALO  65536ull
#define MGENX_SCAN_REUSE 1   /* flags: reuse the tables of the last build on this context */
int mgenx_stream_scan_exits(mgenx_ctx* ctx, const uint8_t* dev_stream, uint64_t nbytes, int mode,
                            uint64_t window, uint64_t limit, uint64_t* dev_entries,
                            uint64_t* dev_exits, uint32_t cap, uint32_t* candidates,
                            void* stream);
/* Records of the chain from `entry` over positions < limit (limit <= nbytes): the scan
 * rule of mgenx_stream_scan started at `entry`.  info->consumed is where it stopped: the
 * first chain position >= limit, or the end / error position as for the whole stream. */
int mgenx_stream_scan_range(mgenx_ctx* ctx, const uint8_t* dev_stream, uint64_t nbytes, int mode,
                            uint64_t entry, uint64_t limit, int flags, uint64_t* dev_rec_off,
                            uint32_t* dev_rec_len, uint64_t cap, mgenx_scan_info* info,
                            void* stream);

/* A socket address as recvfrom reports it (ProtoAddress type / length / port / bytes). */
typedef struct {
    uint8_t  type;      /* MgenMsg::AddressType: 1 IPv4, 2 IPv6 */
    uint8_t  len;       /* address length (4 / 16) */
    uint16_t port;
    uint8_t  addr[16];  /* network byte order */
} mgenx_addr;           /* 20 bytes */

/* ---- per-flow receive analytics (MgenAnalytic::Update) ----
 * Restates MgenAnalytic::Init/Update (src/common/mgenAnalytic.cpp:28-258) as called by
 * Mgen::UpdateRecvAnalytics (src/common/mgen.cpp:1027-1070): per flow, an order-dependent
 * window state machine with a 1024-bit ProtoSlidingMask of received sequence numbers
 * (duplicate detection), FP64 latency sum/min/max and a report when rx >= window end.
 * The caller maps its flow key (src addr, dst addr, flow id: FindFlow, mgenAnalytic.cpp:
 * 312-328) to a dense flow index; records are passed in receive order.  State persists in
 * the caller's mgenx_flow_state array across calls (streaming batches).
 * Parity: bit-exact (FP64 included, no contraction) with the oracle restatement; the
 * protolib primitives themselves are unpinned (ProtoSlidingMask, ProtoTime::Delta). */
typedef struct mgenx_flow_state {   /* 256 B; set up by mgenx_flow_init */
  uint32_t mask[32];                /* bit i <-> sequence number mask_first + i */
  uint32_t mask_first, mask_n;      /* lowest set sequence number, number of set bits */
  uint32_t seq_start, window_valid;
  int64_t  win_start_sec, win_start_usec, win_end_sec, win_end_usec;
  double   window_size;             /* quantized as Report::Quantize/UnquantizeTimeValue */
  uint64_t msg_count, byte_count, dup_count;
  double   latency_sum, latency_min, latency_max;
  uint64_t n_reports;
  uint64_t rsv[2];
} mgenx_flow_state;

typedef struct mgenx_flow_report {  /* one closed window (MgenAnalytic::Report) */
  uint32_t flow, index;             /* flow index, report number within the flow */
  int64_t  start_sec, start_usec;   /* window start */
  double   duration;
  uint64_t msg_count;
  double   rate, loss, latency_ave, latency_min, latency_max;
  int64_t  rx_sec, rx_usec;         /* receive time of the message that closed it */
} mgenx_flow_report;

/* ---- MGEN_DATA items: MgenAnalytic::Report and MgenFlowCommand ----
 * Wire format include/mgenAnalytic.h:14-57 (ProtoPkt fields network order); quantizers
 * mgenAnalytic.cpp:568-642 -- the device quantizes through tables the context builds with
 * the host's libm (log, log10, pow), so results equal the reference's host arithmetic.
 *
 * mgenx_report_build: the report_msg bytes MgenAnalytic keeps (Init :28-71, the window
 * close :245-253, GetReport :296-310) for every kept report of mgenx_flow_reduce:
 * slot f * per_flow + j (j < min(report_count[f], per_flow)) gets 52 bytes (dev_items) and
 * its length (dev_item_len: 24 / 28 IPv4, 48 / 52 IPv6, per the flow-id flag).  Keys: the
 * analytic's src / dst / flow id / protocol.  dev_sign[f] carries FLAG_LATENCY_SIGN, which
 * SetLatencyAve sets and nothing clears (in/out).  dev_offset (optional, per slot): the
 * seconds GetReport's window offset measures (the send time minus the window end; the
 * analytics caller itself reports 0). */
#define MGENX_REPORT_MAX        52
#define MGENX_PAYLOAD_MGEN_DATA 1    /* MgenMsg::MGEN_DATA payload type (mgenMsg.h:102) */
#define MGENX_MAX_FLOW          40   /* MgenEvent::FlowStatus::MAX_FLOW (mgenEvent.h:194) */
typedef struct {
    mgenx_addr src, dst;
    uint32_t flow_id;
    uint8_t  protocol;           /* Protocol: 1 UDP, 2 TCP, 3 SINK */
    uint8_t  rsv[3];
} mgenx_report_key;              /* 48 bytes */
int mgenx_report_build(mgenx_ctx* ctx, const mgenx_flow_report* dev_reports, uint32_t n_flows,
                       uint32_t per_flow, const uint32_t* dev_report_count,
                       const mgenx_report_key* dev_keys, uint8_t* dev_sign,
                       const double* dev_offset, uint8_t* dev_items, uint8_t* dev_item_len,
                       void* stream);
/* REPORT log lines of the kept reports, as Mgen::UpdateRecvAnalytics logs them at each
 * window close (MgenAnalytic::Log, mgenAnalytic.cpp:260-295: the report_msg's key fields,
 * the analytic's unquantized values, timestamp = the closing message's rx time), in slot
 * order (flow-major; each flow's lines in time order; empty slots give no line).
 * Two passes like mgenx_log_recv_text: dev_line_off[n_flows * per_flow + 1]. */
int mgenx_log_report_text(mgenx_ctx* ctx, const uint8_t* dev_items,
                          const mgenx_flow_report* dev_reports, uint32_t n_flows,
                          uint32_t per_flow, const uint32_t* dev_report_count, uint32_t opts,
                          char* dev_text, uint64_t text_cap, uint64_t* dev_line_off,
                          void* stream);
/* MgenTransport::ProcessRecvMessage (mgenTransport.cpp:2132-2191) over the MGEN_DATA
 * payloads of n decoded records (err == 0, payload_type == MGEN_DATA; columns err,
 * payload_type, payload_len, payload_off required):
 *   dev_status[i]   0 walked to the end, 1 invalid MGEN_DATA payload (a flow command
 *                   longer than the rest), 2 invalid REPORT, 3 an item of length 0 (the
 *                   reference loops forever on it; the walk stops), 0xFF not MGEN_DATA;
 *   dev_needs_host[i]  1 when the payload carries flow commands or (with a controller)
 *                   reports: the host's control plane acts on them (Mgen::ProcessFlowCommand,
 *                   MgenController::OnRecvReport);
 *   dev_cmds        pairs (record, flow_id << 2 | status) for every flow whose status is
 *                   not FLOW_UNCHANGED (MgenFlowCommand::GetStatus, flows 1..MAX_FLOW);
 *   dev_reps        pairs (record, slab offset of the report item) (MGENX_DATA_CONTROLLER:
 *                   type bytes > 0x0f are reports, else skipped as generic items);
 *   dev_totals[2]   the number of commands and reports (only the first cap are written).
 * Bytes past a payload read as 0. */
#define MGENX_DATA_CONTROLLER 0x1
int mgenx_data_walk(mgenx_ctx* ctx, const uint8_t* dev_slab, const uint64_t* dev_rec_off,
                    uint64_t stride, const mgenx_cols* cols, uint32_t n, uint32_t opts,
                    uint8_t* dev_status, uint8_t* dev_needs_host, uint32_t* dev_cmds,
                    uint32_t cmd_cap, uint64_t* dev_reps, uint32_t rep_cap,
                    uint32_t* dev_totals, void* stream);
/* REPORT lines of received reports (MgenAnalytic::Report::Log, mgenAnalytic.cpp:747-786):
 * dev_reps = mgenx_data_walk's pairs; per record the source (the reporter) and rx time.
 * "sent>" prints the rx time again, as the reference does. */
int mgenx_log_report_recv_text(mgenx_ctx* ctx, const uint8_t* dev_slab, const uint64_t* dev_reps,
                               uint32_t n_reps, const mgenx_addr* dev_src,
                               const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                               uint32_t opts, char* dev_text, uint64_t text_cap,
                               uint64_t* dev_line_off, void* stream);

/* Packed per-flow counters for the multi-GPU merge (one RCCL all-reduce(sum) of
 * n_flows x 64 B: flows are owned by one rank, the others contribute zeros). */
typedef struct mgenx_flow_counters {
  uint64_t msg_count, byte_count, dup_count, n_reports;
  double   latency_sum, latency_min, latency_max;
  uint64_t seq_start;
} mgenx_flow_counters;

int mgenx_flow_init(mgenx_ctx* ctx, mgenx_flow_state* dev_flows, uint32_t n_flows,
                    double window_sec, void* stream);
/* Records i < n with dev_flow_idx[i] < n_flows update flow dev_flow_idx[i], in order.
 * Columns: seq_num, tx_sec, tx_usec, msg_len (from mgenx_unpack_batch); rx time per
 * record in dev_rx_sec/dev_rx_usec.  Reports go to dev_reports[f * per_flow + k] for
 * k < per_flow; dev_report_count[f] (zeroed by the caller) counts all of them.  With
 * per_flow == 0, dev_reports and dev_report_count may be NULL (the states' n_reports still
 * count every report).  Synchronous on `stream` only when its workspace must grow.
 * Values: the four times are any uint32_t.  tx_usec and rx_usec are taken as they are, 10^6
 * and more included: ProtoTime::Delta subtracts the fields widened to int64 (latencies of any
 * sign and size), receive times compare by seconds, then microseconds, and only a window end
 * is normalised (its seconds may pass 2^32: no record closes that window).  Receive times
 * need not increase.  A window that quantizes to 0 (window_sec < 0.5 us) closes on every
 * record after a flow's first, nothing is written past slot per_flow - 1 of a flow, and a
 * duration of 0 gives the reference's inf and 0 / 0.  Where the oracle's double is NaN, the
 * GPU's must be NaN of any sign or payload.  Everything else is byte-equal. */
int mgenx_flow_reduce(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_seq,
                      const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                      const uint16_t* dev_msg_len, const uint32_t* dev_rx_sec,
                      const uint32_t* dev_rx_usec, uint32_t n, mgenx_flow_state* dev_flows,
                      uint32_t n_flows, mgenx_flow_report* dev_reports, uint32_t per_flow,
                      uint32_t* dev_report_count, void* stream);
/* mgenx_flow_reduce plus, per kept report slot f * per_flow + k, the input record whose
 * Update closed the window (dev_report_rec, optional): the record after which the reference
 * logs the REPORT line (pcap2mgen.cpp:468-470, mgen.cpp:1055-1060). */
int mgenx_flow_reduce_ex(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_seq,
                         const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                         const uint16_t* dev_msg_len, const uint32_t* dev_rx_sec,
                         const uint32_t* dev_rx_usec, uint32_t n, mgenx_flow_state* dev_flows,
                         uint32_t n_flows, mgenx_flow_report* dev_reports, uint32_t per_flow,
                         uint32_t* dev_report_count, uint32_t* dev_report_rec, void* stream);
/* The same reduction reading seq_num, tx_sec, tx_usec and msg_len from the 32-B rows
 * mgenx_unpack_batch writes (cols.rows): the unpack -> FindFlow -> Update pipeline without
 * the column layout.  dev_report_rec as mgenx_flow_reduce_ex (optional). */
int mgenx_flow_reduce_rows(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const mgenx_rec* dev_rows,
                           const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec, uint32_t n,
                           mgenx_flow_state* dev_flows, uint32_t n_flows,
                           mgenx_flow_report* dev_reports, uint32_t per_flow,
                           uint32_t* dev_report_count, uint32_t* dev_report_rec, void* stream);
int mgenx_flow_export(mgenx_ctx* ctx, const mgenx_flow_state* dev_flows, uint32_t n_flows,
                      mgenx_flow_counters* dev_out, void* stream);

/* ---- per-flow delivery statistics: latency histogram, jitter, reordering ----
 * What the MGEN manual names as the uses of a log beside rate and loss (doc/mgen.xml, the
 * table at 3399-3450): the distribution of the delivery latency, how far it moves from one
 * message to the next, and how many messages arrive out of order.  Integer arithmetic on
 * microseconds over the columns mgenx_flow_reduce takes; the result does not depend on the
 * order in which workgroups finish and equals a serial walk of the records exactly.
 *
 * Records i < n with dev_flow_idx[i] < n_flows count, in receive order (others are skipped,
 * MGENX_FLOW_NONE included).  For record k of a flow, in signed 64-bit (the u32 columns
 * widened first; a tx_usec >= 10^6 is taken as it is):
 *   rx  = rx_sec * 10^6 + rx_usec
 *   lat = (rx_sec - tx_sec) * 10^6 + rx_usec - tx_usec
 * Per flow (struct mgenx_flow_dist, 160 B; the name is also the function's, so C code writes
 * the struct keyword):
 *   n, bytes             records; sum of msg_len
 *   lat_sum/min/max      over all records (INT64_MAX / INT64_MIN while n == 0; the sum wraps)
 *   lat_neg, lat_over    records with lat < 0, with lat >= 2^32
 *   jitter_sum/max       abs(lat_k - lat_{k-1}) over consecutive records of the flow (n - 1
 *                        terms; jitter_sum / (n - 1) is the mean jitter, not RFC 3550's filter)
 *   gap_min/max          rx_k - rx_{k-1}, signed (INT64_MAX / INT64_MIN below two records)
 *   reordered, reorder_sum, reorder_max
 *                        record k is reordered iff seq_k < M, M the largest seq among the
 *                        flow's earlier records (plain unsigned compare: a sequence wrap is not
 *                        followed; a record equal to M is not reordered; duplicates are not
 *                        removed); its distance is M - seq_k
 *   seq_min, seq_max     over all records (UINT32_MAX / 0 while n == 0)
 *   first_rx, last_rx, last_lat   carried between calls (0 while n == 0)
 * Histogram (optional): dev_hist[f * MGENX_FLOW_DIST_BINS + b] counts the records of flow f
 * with 0 <= lat < 2^32 in bin b = mgenx_flow_dist_bin(lat): one bin per value below 64 us,
 * then 32 bins per octave (bin b >= 64 starts at mgenx_flow_dist_bin_lo(b); bin_lo(896) =
 * 2^32; mgenx_flow_dist_bin of a value >= 2^32 gives 896, no bin).
 * Streaming: state and histogram persist in the caller's arrays; calls over consecutive
 * batches leave the bytes one call over the concatenation leaves.
 * mgenx_flow_dist_quantiles: dev_out[f * n_q + j] for permille[j] in 1..1000 (host array;
 * anything else is MGENX_EINVAL): with rank r = max(1, (q * n + 999) / 1000) over the order
 * lat_neg records < bins 0..895 < lat_over records, -1 when the rank falls among the negative
 * latencies, the inclusive upper edge of its bin, 2^32 among the overflows, INT64_MIN for a
 * flow without records.  The r-th smallest latency x has bin_lo <= x <= value.
 * Synchronous on `stream` only when the workspace must grow. */
#define MGENX_FLOW_DIST_BINS 896
struct mgenx_flow_dist {            /* 160 B; set up by mgenx_flow_dist_init */
  uint64_t n, bytes;
  int64_t  lat_sum, lat_min, lat_max;
  uint64_t lat_neg, lat_over;
  uint64_t jitter_sum, jitter_max;
  int64_t  gap_min, gap_max;
  uint64_t reordered, reorder_sum;
  uint32_t reorder_max, seq_min, seq_max, rsv32;
  int64_t  first_rx, last_rx, last_lat;
  uint64_t rsv[2];
};
int mgenx_flow_dist_init(mgenx_ctx* ctx, struct mgenx_flow_dist* dev_dist, uint64_t* dev_hist,
                         uint32_t n_flows, void* stream);
int mgenx_flow_dist(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_seq,
                    const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                    const uint16_t* dev_msg_len, const uint32_t* dev_rx_sec,
                    const uint32_t* dev_rx_usec, uint32_t n, struct mgenx_flow_dist* dev_dist,
                    uint64_t* dev_hist, uint32_t n_flows, void* stream);
int mgenx_flow_dist_quantiles(mgenx_ctx* ctx, const struct mgenx_flow_dist* dev_dist,
                              const uint64_t* dev_hist, uint32_t n_flows,
                              const uint32_t* permille, uint32_t n_q, int64_t* dev_out,
                              void* stream);
uint32_t mgenx_flow_dist_bin(uint64_t v);
uint64_t mgenx_flow_dist_bin_lo(uint32_t bin);

/* ---- per-flow time series: windowed rate, loss, latency and jitter ----
 * What a receiver log is plotted as (doc/mgen.xml:3452-3457 sends the user to trpr for it):
 * per flow and per window of receive time, on one time axis for all flows, how much arrived,
 * how the sequence numbers moved and what the latency did.  No reference code: the definition
 * below is the contract.  Integer arithmetic; the result is the bytes a serial walk of the
 * records leaves, whatever order the workgroups finish in.
 *
 * Records i < n with dev_flow_idx[i] < n_flows count, in receive order (others are skipped,
 * MGENX_FLOW_NONE included); rx and lat are mgenx_flow_dist's, signed 64-bit microseconds.
 * Sequence numbers compare as plain unsigned 32-bit values (a wrap is not followed).
 * For record k of a flow:
 *   M   the largest seq among the flow's earlier records, earlier calls included (the flow's
 *       first record has none)
 *   b   floor((rx - t0_us) / width_us), a signed floor: rx < t0_us gives b < 0
 * A record whose b lies outside [0, n_bins) adds 1 to state.outside and to no bin; it still
 * counts in state.n, still moves M, and is still the predecessor of the next record's jitter.
 * Otherwise dev_bins[f * n_bins + b] takes
 *   n += 1, bytes += msg_len, lat_sum / lat_min / lat_max from lat
 *   jitter_sum += abs(lat - lat_prev)   when the flow has an earlier record (any bin, any call)
 *   the flow's first record:  fresh += 1, advance += 1
 *   seq > M:                  fresh += 1, advance += seq - M
 *   seq < M:                  late += 1
 *   seq == M:                 neither
 * Reading the sequence terms: advance is how many sequence numbers the window moved past,
 * advance - fresh the number skipped in that window (the loss as seen then), late the number
 * of records that arrived after being skipped (loss taken back).  Over a flow whose records
 * all fall inside bins, the sum of advance is seq_max - (the first record's seq) + 1.
 * Streaming: calls over consecutive batches with the same t0_us, width_us and n_bins leave
 * the bytes one call over the concatenation leaves.  n == 0 or n_flows == 0 touches nothing.
 * MGENX_EINVAL: width_us == 0, n_bins == 0, a null required pointer, n_flows * n_bins >= 2^31.
 * Synchronous on `stream` only when the workspace must grow. */
struct mgenx_flow_series_bin {       /* 64 B; one per (flow, time bin) */
  uint64_t n, bytes;                 /* records; sum of msg_len */
  int64_t  lat_sum, lat_min, lat_max;/* INT64_MAX / INT64_MIN while n == 0; the sum wraps */
  uint64_t jitter_sum;               /* sum of |lat_k - lat_{k-1}| credited to record k's bin */
  uint64_t advance;
  uint32_t fresh, late;              /* counts, modulo 2^32 */
};
struct mgenx_flow_series_state {     /* 32 B; per flow, carried between calls */
  uint64_t n;                        /* records counted so far, inside a bin or not */
  int64_t  last_lat;
  uint64_t outside;                  /* records whose bin index fell outside [0, n_bins) */
  uint32_t seq_max, rsv;
};
int mgenx_flow_series_init(mgenx_ctx* ctx, struct mgenx_flow_series_state* dev_state,
                           struct mgenx_flow_series_bin* dev_bins, uint32_t n_flows,
                           uint32_t n_bins, void* stream);
/* dev_bins: [n_flows * n_bins], row f = flow f */
int mgenx_flow_series(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_seq,
                      const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                      const uint16_t* dev_msg_len, const uint32_t* dev_rx_sec,
                      const uint32_t* dev_rx_usec, uint32_t n, int64_t t0_us, uint64_t width_us,
                      uint32_t n_bins, struct mgenx_flow_series_state* dev_state,
                      struct mgenx_flow_series_bin* dev_bins, uint32_t n_flows, void* stream);

/* ---- per-flow time series: exact latency percentiles per window ----
 * p50 / p95 / p99 over time: per flow and window of receive time, the exact order statistics of
 * the latency.  No reference code: the definition below is the contract.  Integer arithmetic;
 * the result is a pure function of the inputs, whatever order the workgroups finish in.
 *
 * Records i < n with dev_flow_idx[i] < n_flows count (others are skipped, MGENX_FLOW_NONE
 * included).  rx and lat are mgenx_flow_dist's (signed 64-bit, the u32 columns widened first, a
 * tx_usec >= 10^6 taken as it is) and the bin is mgenx_flow_series's:
 *   b = floor((rx - t0_us) / width_us), a signed floor
 * A record whose b lies outside [0, n_bins) belongs to no cell and is ignored; there is no
 * per-flow state.  Cell (f, b) holds the multiset of lat of its records: duplicates count
 * separately and the receive order plays no part.  With c the cell's size and permille[j] = q in
 * 1..1000 (host array), r = max(1, (q * c + 999) / 1000) in unsigned 64-bit division -- the rank
 * rule of mgenx_flow_dist_quantiles -- and
 *   dev_out[(f * n_bins + b) * n_q + j] = the r-th smallest lat of the cell,
 * exact: negative latencies in their signed order, no clamping at 2^32.  INT64_MIN for an empty
 * cell.  Every element of dev_out [n_flows * n_bins * n_q] is written on every call and nothing
 * beyond it; n == 0 fills it with INT64_MIN; n_flows == 0 touches nothing and returns MGENX_OK.
 * Not streaming, by design: an exact order statistic needs every value of its cell, so one call
 * takes the whole log, as mgenx_msg_match does.
 * MGENX_EINVAL (found before any HIP call): a null ctx; width_us == 0; n_bins == 0; n_q == 0 or
 * n_q > MGENX_FLOW_SERIES_MAX_Q; a permille outside 1..1000; a null permille or dev_out; a null
 * column with n > 0; n >= 2^31; n_flows * n_bins >= 2^31.
 * Workspace: owned by the context and grown when needed; the call is synchronous on `stream`
 * only when it grows.  With C = n_flows * n_bins its size is, each piece rounded up to 256 B,
 *   36 n + 4 (C + 1) + the radix sort's temporary storage for n pairs           (grouping)
 *   + 4 (min(C, n/9) + min(C, n/257) + min(C, n/2049) + min(C, n/16385)) + 16   (tier lists)
 *   + min(C, n/16385) * 32 * (8 + 4 + 1024)            (radix select over cells above 16384)
 * bytes.  Asynchronous otherwise; one such call per context at a time. */
#define MGENX_FLOW_SERIES_MAX_Q 32
int mgenx_flow_series_quantiles(mgenx_ctx* ctx, const uint32_t* dev_flow_idx,
                                const uint32_t* dev_tx_sec, const uint32_t* dev_tx_usec,
                                const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec, uint32_t n,
                                int64_t t0_us, uint64_t width_us, uint32_t n_bins,
                                uint32_t n_flows, const uint32_t* permille, uint32_t n_q,
                                int64_t* dev_out, void* stream);

/* ---- per-flow clock offset and skew removal for one-way latencies ----
 * Every latency above is rx - tx, two stamps from two hosts' clocks: a receiver clock that is
 * off by milliseconds or drifts by tens of ppm shows up in every histogram and percentile.
 * The remedy is Moon, Skelly and Towsley, "Estimation and removal of clock skew from network
 * delay measurements" (INFOCOM 1999): per flow, the straight line that lies under every
 * (send time, latency) point and is closest to the points is the clock offset plus skew plus
 * the minimum path delay; what remains above it is queueing and jitter.  No reference code: the
 * definition below is the contract.  Integer arithmetic, exact for every input; the result is a
 * pure function of the inputs, whatever order the workgroups finish in.
 *
 * Records i < n with dev_flow_idx[i] < n_flows count (others are skipped, MGENX_FLOW_NONE
 * included).  In 64-bit, the u32 columns widened first and a tx_usec >= 10^6 taken as it is:
 *   x_i = tx_sec * 10^6 + tx_usec                              (unsigned, below 2^52)
 *   d_i = (rx_sec - tx_sec) * 10^6 + rx_usec - tx_usec         (signed: mgenx_flow_dist's lat)
 * The fit, per flow, over the set of its points (x_i, d_i).  H is the lower convex hull of the
 * set: vertices in increasing x; among equal x only the lowest d can be a vertex; a point
 * collinear with its hull neighbours is not a vertex.  S is the sum of x_i over the flow's n
 * counted records as an exact integer.  With at least two distinct x, A and B are the
 * consecutive vertices of H with n * x_A <= S < n * x_B: the hull edge over the mean send time
 * (the edge that starts at the mean when the mean falls on a vertex).  Among all lines that
 * pass under every point it minimises the sum of d_i - line(x_i).  With all x equal (n = 1
 * included) A = B = (x, the lowest d).  With MGENX_CLOCK_OFFSET_ONLY the slope is forced to 0:
 * A = B = the point of lowest d, of lowest x among those.  ia / ib: the lowest record index i
 * whose point equals A / B.
 *   line(x) = d_A + floor((d_B - d_A) * (x - x_A) / (x_B - x_A))     (d_A when x_A = x_B)
 * with the mathematical floor (toward -inf) and x - x_A signed, and
 *   c_i = d_i - line(x_i)
 * c_i >= 0, and 0 at A and B.  Products reach 2^106: the arithmetic is 128-bit.  c_i is kept
 * modulo 2^64 as a signed value; it leaves 63 bits only where the chosen edge is steeper than
 * 2^11 us per us and the flow's send times reach further than 2^63 / that slope from it.
 * Outputs; every element of every array given is written on every call and nothing beyond it:
 *   dev_flows [n_flows]   struct mgenx_flow_clock (64 B): n; A = (xa, da), B = (xb, db); ia, ib;
 *                         resid_sum = sum of c_i (wraps), resid_max = max c_i.  An empty flow:
 *                         n = 0, xa = xb = 0, da = db = 0, resid_sum = 0, resid_max =
 *                         INT64_MIN, ia = ib = MGENX_CLOCK_NONE.  No skew figure: floor(10^9 *
 *                         (db - da) / (xb - xa)) does not fit 64 bits for every input; callers
 *                         derive it from A and B.
 *   dev_resid [n]         optional: c_i; INT64_MIN for a skipped record.
 *   dev_rx_sec_out, dev_rx_usec_out [n]   optional, both or neither: the receive stamp on the
 *                         sender's clock with the floor removed: with r = x_i + c_i, sec =
 *                         (r / 10^6) mod 2^32 and usec = r mod 10^6; a skipped record gets its
 *                         input stamp.  mgenx_flow_dist, mgenx_flow_series and
 *                         mgenx_flow_series_quantiles fed these two columns in place of rx_*
 *                         compute their statistics of c_i with no change of their own.  They
 *                         must not overlap the input columns.
 * dev_flow_idx may be any dense grouping: one index per sender host fits one clock per host.
 * One call takes the whole log; it does not stream (a later record can lower the hull
 * anywhere), as mgenx_msg_match does not.  n == 0 writes the empty structs; n_flows == 0
 * touches nothing and returns MGENX_OK.
 * MGENX_EINVAL (found before any HIP call): a null ctx or dev_flows; a null column with n > 0;
 * only one of the two stamp outputs; unknown opts bits; n >= 2^31 or n_flows >= 2^31.
 * Workspace: owned by the context and grown when needed; the call is synchronous on `stream`
 * only when it grows.  Its size is, each piece rounded up to 256 B,
 *   16 n + 4 (n_flows + 1) + the radix sort's temporary storage for n pairs     (grouping)
 *   + 32 n                                      (the points, in input order and by flow)
 *   + 4 + 4 min(n_flows, n / 2049)                     (the flows served by a workgroup)
 * bytes.  Asynchronous otherwise; one such call per context at a time.
 * Cost: a flow's fit reads its points once per round of the hull search (4-7 rounds on drift
 * plus delay noise, more when every point is a hull vertex), a flow of more than 2048 points on
 * one workgroup: a single flow of millions of records is the slow case. */
#define MGENX_CLOCK_NONE        0xFFFFFFFFu
#define MGENX_CLOCK_OFFSET_ONLY 0x1u
struct mgenx_flow_clock {           /* 64 B; one per flow */
  uint64_t n;
  uint64_t xa;
  int64_t  da;
  uint64_t xb;
  int64_t  db;
  int64_t  resid_sum, resid_max;
  uint32_t ia, ib;
};
int mgenx_flow_clock(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_tx_sec,
                     const uint32_t* dev_tx_usec, const uint32_t* dev_rx_sec,
                     const uint32_t* dev_rx_usec, uint32_t n, uint32_t n_flows, uint32_t opts,
                     struct mgenx_flow_clock* dev_flows, int64_t* dev_resid,
                     uint32_t* dev_rx_sec_out, uint32_t* dev_rx_usec_out, void* stream);


/* ---- MgenAnalyticTable::FindFlow for batches (mgenAnalytic.cpp:312-328) ----
 * A device hash table from the reference's flow key -- dst addr | dst port | src addr |
 * src port | flowId -- to dense flow indices 0, 1, ... (new keys are numbered in the order
 * of their first record, so the mapping is deterministic).  mgenx_flow_lookup maps n decoded
 * records (columns dst_addr, dst_len, dst_port, flow_id, and err when given: err != 0 maps
 * to MGENX_FLOW_NONE) with their recvfrom source addresses to dev_flow_idx[i] -- the input
 * mgenx_flow_reduce takes -- and copies the table's flow count to dev_n_flows[0] (optional,
 * device memory).  Keys persist across calls (streaming batches).  An empty batch (n == 0)
 * changes nothing and still reports the table's count to dev_n_flows, in stream order.
 * With cols->rows (the 32-B mgenx_rec output) the key fields and err come from the rows;
 * the destination address from the dst_addr column when given, else from the rows'
 * dst_addr4 -- exact for IPv4 destinations; a record whose dst_len exceeds 4 then maps to
 * MGENX_FLOW_NONE (pass dst_addr when IPv6 destinations can occur).
 * A table takes new keys while it holds fewer than its max_flows (rounded up to half its
 * power-of-two slot count; keys created concurrently may pass that bound together) and probes
 * at most 1024 slots per lookup: a record whose key finds no room maps to MGENX_FLOW_NONE (an
 * undersized table; the caller redoes the batch on a larger one).  Near the bound that
 * refusal can be spurious (a record racing the creation of its own key, or a key past the
 * probe limit): MGENX_FLOW_NONE means "redo on a larger table", never "no such flow".
 * Performance: a table of at most 2048 flows (4096 slots) is probed from a copy of its keys
 * staged in LDS (up to 1536 keys; keys past that, and keys new in the call, take the atomic
 * path); larger tables probe HBM.  Steady state, config 4: 8.4M lookups in ~0.10 ms. */
#define MGENX_FLOW_NONE 0xFFFFFFFFu
typedef struct mgenx_flow_table mgenx_flow_table;
int mgenx_flow_table_create(mgenx_ctx* ctx, uint32_t max_flows, mgenx_flow_table** out);
int mgenx_flow_table_destroy(mgenx_flow_table* table);
int mgenx_flow_lookup(mgenx_ctx* ctx, mgenx_flow_table* table, const mgenx_cols* cols,
                      const mgenx_addr* dev_src, uint32_t n, uint32_t* dev_flow_idx,
                      uint32_t* dev_n_flows, void* stream);
/* The key of every flow index < cap (MgenAnalytic::Init's src / dst / flow id, with
 * `protocol`): the report_msg keys mgenx_report_build takes (mgenAnalytic.cpp:28-71). */
int mgenx_flow_keys(mgenx_ctx* ctx, const mgenx_flow_table* table, int protocol,
                    mgenx_report_key* dev_keys, uint32_t cap, void* stream);
/* The sizes a batch's report slots need, on the device: dev_out[0] = the most records any flow
 * index < n_flows holds, dev_out[1] / dev_out[2] = the lowest / highest receive time (sec *
 * 1e6 + usec) over those records (UINT64_MAX / 0 when there are none).  dev_counts: n_flows
 * words of scratch (cleared here).  pcap2mgen sizes its per-flow report slots from these
 * (a window closes at most once per record and once per window of capture time). */
int mgenx_flow_span(mgenx_ctx* ctx, const uint32_t* dev_flow_idx, const uint32_t* dev_rx_sec,
                    const uint32_t* dev_rx_usec, uint32_t n, uint32_t n_flows,
                    uint32_t* dev_counts, uint64_t* dev_out, void* stream);

/* ---- event log (MgenMsg::LogRecvEvent / LogRecvError, text form) ----
 * One line per record, as the UDP receive path logs it (src/common/mgenTransport.cpp:
 * 976-994): "RECV proto>... flow>... seq>... src>... dst>... sent>... size>... [host>...]
 * [ttl>...] [gps>...] [data>...] [flags>...]" for a good record
 * (src/common/mgenMsg.cpp:1034-1102), "RERR type>... src>..." for a record with an error
 * (:711-735); timestamps GMT "HH:MM:SS.usec" or epoch "sec.usec" (src/common/mgen.cpp:55-83).
 * Byte-exact with the reference's fprintf output on x86-64 Linux.
 * Inputs: the unpack outputs for the same records -- core fields (rows or columns) plus the
 * extended columns dst_addr, host_addr, host_port, host_type, host_len, lat_raw, lon_raw,
 * alt, payload_off (all required) --, the slab and record placement (for the data> hex),
 * the recvfrom source address, the receive time and (optional, NULL = unknown) TTL.
 * Output: dev_line_off[i] = byte offset of record i's line, dev_line_off[n] = total bytes;
 * the lines are written to dev_text only when the total fits text_cap (read
 * dev_line_off[n] and call again with a larger buffer otherwise).  No NUL terminator. */

#define MGENX_PROTO_UDP  1   /* Protocol (include/mgenGlobals.h:61-68) */
#define MGENX_PROTO_TCP  2
#define MGENX_PROTO_SINK 3
#define MGENX_LOG_EPOCH   0x1  /* Mgen::SetEpochTimestamp(true) */
#define MGENX_LOG_NO_DATA 0x2  /* log_data off */
#define MGENX_LOG_NO_GPS  0x4  /* log_gps_data off */
#define MGENX_LOG_SKIP_ERR 0x8 /* records with err != 0 get no line (pcap2mgen.cpp:428-432
                                  skips a packet Unpack rejects instead of logging RERR) */

int mgenx_log_recv_text(mgenx_ctx* ctx, const uint8_t* dev_slab, const uint64_t* dev_rec_off,
                        uint64_t stride, const mgenx_cols* cols, const mgenx_addr* dev_src,
                        const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                        const int32_t* dev_ttl, uint32_t n, int protocol, uint32_t opts,
                        char* dev_text, uint64_t text_cap, uint64_t* dev_line_off, void* stream);
/* The binary log form of the same events (MgenMsg::LogRecvEvent / LogRecvError binary
 * branches, src/common/mgenMsg.cpp:652-710, 958-1033): per record an event header (type,
 * protocol, BE length, BE rx time, BE source port, source type/length/address) followed, for
 * RECV, by hdr_len + payload_len message bytes with CHECKSUM cleared in the flags byte
 * (the hdr_len extended column is also required); RERR ends with the BE error code.
 * The message bytes are the receive buffer's: the record's dev_rec_len[i] bytes (the
 * recvfrom length; when dev_rec_len is NULL, its msg_len field), then zeros where the
 * reference's buffer holds stale bytes; bytes past slab_bytes are zero too.
 * dev_rec_pos has the same meaning as dev_line_off.  The file header line the reference
 * writes once per log file is the caller's. */
int mgenx_log_recv_binary(mgenx_ctx* ctx, const uint8_t* dev_slab, uint64_t slab_bytes,
                          const uint64_t* dev_rec_off, uint64_t stride,
                          const uint32_t* dev_rec_len, const mgenx_cols* cols,
                          const mgenx_addr* dev_src, const uint32_t* dev_rx_sec,
                          const uint32_t* dev_rx_usec, uint32_t n, int protocol,
                          uint8_t* dev_out, uint64_t out_cap, uint64_t* dev_rec_pos,
                          void* stream);

/* SEND events (MgenMsg::LogSendEvent, src/common/mgenMsg.cpp:1145-1241) of records packed
 * by a send path, as the transport logs them after each successful send
 * (mgenTransport.cpp:1060, 1392, 1805: theTime = the message's tx time):
 *   text:   "<tx time> SEND proto>P flow>F seq>S srcPort>SP dst>A/port size>N [host>H/port]\n"
 *           (size = msg_len; TCP: mgen_msg_len from dev_msg_total);
 *   binary: {SEND_EVENT 3, protocol, BE recordLength [, TCP: BE mgen_msg_len]} and then
 *           recordLength bytes of the packed message (UDP / SINK) with CHECKSUM cleared,
 *           recordLength = 12 + dst length + packet_header_len (+ host length + 4 with a
 *           host); bytes past the packed message read as 0.
 * dev_src_port[t]: template t's source port (the flow transport's socket port,
 * mgenFlow.cpp:975-977).  dev_out_len (optional): Pack's return per record -- 0 means the
 * message was not sent and gets no event.  Two passes as mgenx_log_recv_text:
 * dev_pos[n + 1] = byte offsets; written only when the total fits out_cap. */
int mgenx_log_send_text(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                        const mgenx_pack_desc* dev_desc, const uint16_t* dev_src_port,
                        const uint32_t* dev_out_len, const uint32_t* dev_msg_total, uint32_t n,
                        int protocol, uint32_t opts, char* dev_text, uint64_t text_cap,
                        uint64_t* dev_line_off, void* stream);
int mgenx_log_send_binary(mgenx_ctx* ctx, const mgenx_flow_tmpl* dev_tmpl,
                          const mgenx_pack_desc* dev_desc, const uint32_t* dev_out_len,
                          const uint32_t* dev_msg_total, const uint8_t* dev_slab,
                          uint64_t slab_bytes, const uint64_t* dev_rec_off, uint64_t stride,
                          uint32_t n, int protocol, uint8_t* dev_out, uint64_t out_cap,
                          uint64_t* dev_rec_pos, void* stream);

/* ---- one log file from several line sources, in record order ----
 * The reference writes, per received message, the lines of several loggers in turn: e.g.
 * pcap2mgen (pcap2mgen.cpp:445-476) logs the analytic's REPORT line when Update closed a
 * window, then the RECV line, then the REPORT lines of the reports the payload carries.
 * mgenx_text_interleave concatenates, for record 0, 1, ..., n_rec - 1, each source's lines
 * of that record in source order.  A source is a text with line offsets (line k =
 * text[line_off[k], line_off[k+1])) and the record each line belongs to:
 *   MGENX_TEXT_PER_RECORD  line i is record i's (n_lines = n_rec; empty lines allowed);
 *   MGENX_TEXT_OWNER       owner[k * index_stride] = line k's record, non-decreasing in k;
 *   MGENX_TEXT_MAP         index[i] = record i's line (at most one), or MGENX_FLOW_NONE;
 *   MGENX_TEXT_SCATTER     index[k] = line k's record (at most one line per record, any
 *                          order; MGENX_FLOW_NONE = no record): e.g. the slots of
 *                          mgenx_log_report_text with mgenx_flow_reduce_ex's dev_report_rec.
 * Two passes like mgenx_log_recv_text: dev_rec_off[n_rec + 1] = byte offsets of each record's
 * output; dev_out is written only when the total fits out_cap.  srcs is a HOST array. */
#define MGENX_TEXT_PER_RECORD 0
#define MGENX_TEXT_OWNER      1
#define MGENX_TEXT_MAP        2
#define MGENX_TEXT_SCATTER    3
#define MGENX_TEXT_MAX_SRC    4
typedef struct {
    const char*     text;         /* may be NULL only when every line is empty */
    const uint64_t* line_off;     /* n_lines + 1 entries */
    uint32_t        n_lines;
    uint32_t        kind;         /* MGENX_TEXT_* */
    const uint32_t* index;        /* owner (OWNER), record -> line (MAP), line -> record
                                     (SCATTER) */
    uint32_t        index_stride; /* OWNER: u32 elements between owners (1, or 4 for the
                                     (record, offset) u64 pairs of mgenx_data_walk) */
    uint32_t        rsv;
} mgenx_text_src;
int mgenx_text_interleave(mgenx_ctx* ctx, const mgenx_text_src* srcs, uint32_t n_src,
                          uint32_t n_rec, char* dev_out, uint64_t out_cap, uint64_t* dev_rec_off,
                          void* stream);

/* ---- pcap2mgen: captured packets -> MgenMsg records (src/common/pcap2mgen.cpp:252-482) ----
 * mgenx_pcap_index (HOST memory, no device work: the pcap_next loop, :344) reads the pcap
 * file header and walks the record headers: the offsets of the first `cap` records' 16-byte
 * headers go to pkt_off (host memory).  info: link type, flags, records found, bytes consumed
 * (a record cut short by the end of the buffer ends the walk, as pcap_next returns NULL).
 * Returns MGENX_EINVAL for a buffer that is not a pcap file.
 * mgenx_pcap_parse (device) restates, per record, pcap2mgen's frame walk (:346-436) over
 * protolib's ProtoPktETH / ProtoPktIP / ProtoPktUDP (restated: protolib is not vendored,
 * so this layer is parity unpinned): DLT_LINUX_SLL (16-byte header) or, for every
 * other link type as in the reference, Ethernet frames (hdr.len <= 4094 bytes, optional
 * 802.1Q tag), IPv4 / IPv6, UDP.  Per record:
 * udp_off / udp_len = the UDP payload (the Unpack buffer; udp_len 0 when status != 0, so
 * Unpack rejects it), src = IP source + UDP source port (msg.SetSrcAddr, :434-435),
 * ttl = IPv4 TTL / IPv6 hop limit, rx time = the pcap timestamp (ProtoTime(hdr.ts); a
 * nanosecond file is read at microsecond precision, as pcap_fopen_offline does). */
#define MGENX_DLT_EN10MB    1
#define MGENX_DLT_LINUX_SLL 113
#define MGENX_PCAP_NSEC    0x1  /* nanosecond timestamps (magic 0xa1b23c4d) */
#define MGENX_PCAP_SWAPPED 0x2  /* the file's byte order is not the host's */
#define MGENX_PCAP_UDP       0  /* status: a UDP datagram */
#define MGENX_PCAP_BAD_ETH   1  /* "invalid Ether frame" (:370-373) */
#define MGENX_PCAP_NOT_IP    2  /* not IPv4 / IPv6 (:422) */
#define MGENX_PCAP_BAD_IP    3  /* "bad IP packet" (:388-391) */
#define MGENX_PCAP_NOT_UDP   4  /* (:425) */
#define MGENX_PCAP_TRUNCATED 5  /* UDP payload past the captured bytes: skipped (the
                                   reference reads stale buffer bytes there) */
#define MGENX_PCAP_OOB       6  /* record past the buffer */
#define MGENX_PCAP_SNAPPED   7  /* a UDP datagram cut by the capture's snapshot length whose
                                   UDP header and >= MIN_SIZE payload bytes were captured:
                                   mgenx_pcap_snap moves it into scratch, zero-extended to the
                                   UDP length (then MGENX_PCAP_UDP); left alone it is skipped */
typedef struct {
    uint32_t link_type;   /* DLT_* */
    uint32_t flags;       /* MGENX_PCAP_NSEC | MGENX_PCAP_SWAPPED */
    uint32_t snaplen;
    uint32_t rsv;
    uint64_t n_records;   /* records found (only the first cap offsets are written) */
    uint64_t consumed;    /* bytes of whole records, file header included */
    uint64_t snap_bytes;  /* scratch mgenx_pcap_snap may need: sum over records captured
                             short of their wire length of that length, 16-byte rounded */
} mgenx_pcap_info;
int mgenx_pcap_index(const uint8_t* buf, uint64_t nbytes, uint64_t* pkt_off, uint64_t cap,
                     mgenx_pcap_info* info);
int mgenx_pcap_parse(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                     const uint64_t* dev_pkt_off, uint32_t n, uint32_t link_type,
                     uint32_t flags, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                     mgenx_addr* dev_src, int32_t* dev_ttl, uint32_t* dev_rx_sec,
                     uint32_t* dev_rx_usec, uint8_t* dev_status, void* stream);
/* A capture taken with a snapshot length (tcpdump -s N) cuts datagrams short; the reference
 * parses such a frame by its wire length and Unpacks the UDP payload from its parse buffer,
 * so the MGEN header comes from the captured bytes and the rest of the buffer is stale.
 * mgenx_pcap_snap copies every MGENX_PCAP_SNAPPED packet's captured UDP payload into
 * dev_buf[file_bytes, buf_bytes) (scratch after the file image; info.snap_bytes is enough)
 * zero-extended to its UDP length, points dev_udp_off / dev_udp_len there and sets its
 * status to MGENX_PCAP_UDP; a packet that does not fit stays SNAPPED.  Asynchronous. */
int mgenx_pcap_snap(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t file_bytes, uint64_t buf_bytes,
                    const uint64_t* dev_pkt_off, uint32_t n, uint32_t flags, uint8_t* dev_status,
                    uint64_t* dev_udp_off, uint32_t* dev_udp_len, void* stream);

/* ---- pcap2mgen: pcapng captures (what Wireshark, dumpcap and tshark write) ----
 * The reference opens its input with pcap_fopen_offline (pcap2mgen.cpp:323) and libpcap reads
 * pcapng there as it reads pcap.  libpcap is not part of the reference tree, so this layer
 * restates its pcapng reader (parity unpinned, like the protolib packet classes); the walk
 * rules are the contract and are listed in DESIGN.md 4.10 and mgen_amd/csrc/mgenx_pcapng.hpp.
 * mgenx_pcapng_index (HOST memory, no device work) walks the blocks of a file image: Section
 * Header (the section's byte order), Interface Description (link type, snaplen, if_tsresol,
 * if_tsoffset), Enhanced / obsolete / Simple Packet blocks; every other block is skipped.
 * The offsets of the first `cap` packet blocks go to pkt_off and each packet's row in the
 * interface table to pkt_if; the first `if_cap` interfaces go to ifaces (rows are appended
 * across sections).  The counts in info are always complete, so a first call with cap =
 * if_cap = 0 sizes the arrays.  Returns MGENX_EINVAL for a buffer that does not start with a
 * version-1 Section Header Block.  Otherwise info->status says how the walk ended; a stop
 * keeps every packet before it (the reference loop ends when pcap_next returns NULL) and
 * info->consumed is the offset of the block that stopped it:
 *   _TRUNCATED the file ends inside a block
 *   _BLOCK     a malformed block: a length below the type's minimum or not a multiple of 4,
 *              a trailing length that differs from the leading one, an IDB option past its block
 *   _SECTION   a later section of another byte order, a bad magic or a major version != 1
 *   _LINKTYPE  an IDB of another link type than the file's first (pcap_datalink is one value)
 *   _NO_IFACE  a packet on an interface its section has not described (an SPB: interface 0)
 *   _TSRESOL   if_tsresol beyond 10^-19 / 2^-63, a wrong length of if_tsresol (1) or
 *              if_tsoffset (8), or either option given twice
 *   _CAPLEN    a captured length larger than the block's room for data
 * mgenx_pcapng_parse (device, one lane per packet) reads each packet block (EPB / OPB / SPB),
 * converts its 64-bit time stamp with its interface's resolution and offset -- uint64
 * arithmetic that wraps, as libpcap's: sec = t / R + if_tsoffset, usec from t % R scaled to
 * microseconds -- and runs the frame walk of mgenx_pcap_parse over the packet data.  Outputs
 * as mgenx_pcap_parse, plus each packet's data offset and captured length (for the snap
 * step).  A packet whose block head or data does not lie inside buf_bytes, whose pkt_if is not
 * below n_ifaces or whose block is not a packet block gets MGENX_PCAP_OOB.
 * mgenx_pcapng_snap is mgenx_pcap_snap for these packets. */
#define MGENX_PCAP_NG 0x4            /* info.flags: offsets are pcapng packet blocks */
#define MGENX_PCAPNG_OK        0
#define MGENX_PCAPNG_TRUNCATED 1
#define MGENX_PCAPNG_BLOCK     2
#define MGENX_PCAPNG_SECTION   3
#define MGENX_PCAPNG_LINKTYPE  4
#define MGENX_PCAPNG_NO_IFACE  5
#define MGENX_PCAPNG_TSRESOL   6
#define MGENX_PCAPNG_CAPLEN    7
typedef struct {
    uint64_t ts_units;    /* time stamp units per second: 10^k or 2^k */
    int64_t  ts_offset;   /* if_tsoffset (seconds) */
    uint32_t snaplen;     /* 0 = no limit */
    uint8_t  ts_binary;   /* ts_units is a power of two */
    uint8_t  rsv[3];
} mgenx_pcapng_if;        /* 24 bytes */
typedef struct {
    uint32_t link_type;   /* the first IDB's */
    uint32_t flags;       /* MGENX_PCAP_NG | MGENX_PCAP_SWAPPED */
    uint32_t snaplen;     /* the first IDB's */
    int32_t  status;      /* MGENX_PCAPNG_* */
    uint64_t n_records;   /* packet blocks found (only the first cap are written) */
    uint64_t consumed;    /* bytes of whole blocks walked */
    uint64_t snap_bytes;  /* as mgenx_pcap_info */
    uint32_t n_ifaces;    /* interface rows (only the first if_cap are written) */
    uint32_t n_sections;
} mgenx_pcapng_info;
int mgenx_pcapng_index(const uint8_t* buf, uint64_t nbytes, uint64_t* pkt_off, uint32_t* pkt_if,
                       uint64_t cap, mgenx_pcapng_if* ifaces, uint32_t if_cap,
                       mgenx_pcapng_info* info);
int mgenx_pcapng_parse(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                       const uint64_t* dev_pkt_off, const uint32_t* dev_pkt_if, uint32_t n,
                       const mgenx_pcapng_if* dev_ifaces, uint32_t n_ifaces, uint32_t link_type,
                       uint32_t flags, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                       mgenx_addr* dev_src, int32_t* dev_ttl, uint32_t* dev_rx_sec,
                       uint32_t* dev_rx_usec, uint8_t* dev_status, uint64_t* dev_data_off,
                       uint32_t* dev_cap_len, void* stream);
int mgenx_pcapng_snap(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t file_bytes, uint64_t buf_bytes,
                      const uint64_t* dev_data_off, const uint32_t* dev_cap_len, uint32_t n,
                      uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                      void* stream);

/* ---- pcap2mgen: reassembly of fragmented IPv4 / IPv6 datagrams (an option; the reference
 * does not reassemble, and without this call nothing below happens) ----
 * mgenx_pcap_defrag / mgenx_pcapng_defrag run after the parse (and after the snap step) over
 * the same packets, in place.  A packet that is not a fragment is not touched.
 *
 * Which packets are fragments.  Only a packet whose status is not BAD_ETH / NOT_IP / BAD_IP /
 * OOB is examined, by the link-layer and IP-header walk of the parse up to its protocol test
 * (ip0 = the IP header's offset, num = min(caplen, 4094)):
 *   IPv4: F = be16(ip0+6), MF = F & 0x2000, off = (F & 0x1FFF) * 8; a fragment iff MF || off;
 *         protocol 17 only (another protocol stays NOT_UDP); id = be16(ip0+4); payload
 *         [ip0+ihl, ip0+tot); key (4, src, dst, id).
 *   IPv6: the fixed header's next header is 44 (only this position is opened); pl < 8 is
 *         BAD_IP; the 8-byte fragment header at ip0+40 must lie inside num (else TRUNCATED):
 *         byte 0 = the inner next header, 17 only (else NOT_UDP stays); off = be16(+2) &
 *         0xFFF8, MF = be16(+2) & 1, id = be32(+4); payload [ip0+48, ip0+40+pl); an atomic
 *         fragment (off 0, MF 0) is a fragment and completes on its own; key (6, src, dst, id).
 *   Payload of len bytes, tested in this order: len == 0 -> BAD_IP; MF && len % 8 -> BAD_IP;
 *         off + len > 65535 -> BAD_IP; not wholly inside num -> TRUNCATED.  Such a packet gets
 *         that status, udp_len 0 and src.port 0 and takes no part in reassembly.
 *
 * The state machine, per key, over its valid fragments in capture order; t = the packet's
 * receive time rx_sec * 10^6 + rx_usec as int64; at most one context is open per key.  On
 * fragment p:
 *   1. an open context with timeout_us > 0 and t - ctx.t0 > timeout_us is dropped (a negative
 *      difference does not expire it);
 *   2. an open context that p conflicts with is dropped: [off, off+len) intersects a held
 *      fragment (an exact duplicate too); the total L is known and off+len > L; MF == 0 and L
 *      is known; MF == 0 and off+len is below a held fragment's end; it holds 64 fragments;
 *   3. with no context open, one opens with t0 = t;
 *   4. p is added: sum += len; L = off+len when MF == 0; status[p] = MGENX_PCAP_FRAGMENT,
 *      udp_len[p] = 0, src[p].port = 0;
 *   5. with L known and sum == L the datagram is complete at p and the context closes.
 * A dropped context, and one open at the end of the capture, is incomplete; its packets stay
 * FRAGMENT.  (Dropping on overlap rather than ignoring the newcomer keeps a datagram that lost
 * a fragment from splicing into the next one that reuses its id: DESIGN.md 4.10.)
 *
 * Completion at packet p over the L assembled bytes D: L < 8, or ul = be16(D+4) below 8 or
 * above L: status[p] = NOT_UDP, udp_len[p] = 0.  Otherwise status[p] = MGENX_PCAP_UDP,
 * udp_off[p] = the scratch position of D + 8, udp_len[p] = ul - 8, src[p].port = be16(D).
 * Source address, ttl and receive time stay the completing packet's own.  The 4094-byte frame
 * rule applies to each fragment's frame, not to the datagram.
 *
 * Scratch: dev_buf[scratch_off, buf_bytes), at or after the file image and any snap scratch;
 * every packet must lie below scratch_off (one reaching past it is not examined).  Datagrams
 * are laid out in order of their completing packet's index, each in a slot of round16(L)
 * bytes whose pad bytes are zero (rejected datagrams too); dev_buf + scratch_off must be
 * 16-byte aligned when anything is written.  stats (host memory) is always filled; the call is
 * synchronous (one read-back of the sizes).  With a window smaller than stats->scratch_bytes no
 * output array and no scratch byte is changed and MGENX_ENOSPC comes back: a call with an empty
 * window sizes the scratch.  mgenx_pcap_defrag takes the records as mgenx_pcap_snap does;
 * mgenx_pcapng_defrag takes the packet blocks (for each packet's original length) and the
 * data_off / cap_len mgenx_pcapng_parse wrote (flags: MGENX_PCAP_SWAPPED as there). */
#define MGENX_PCAP_FRAGMENT  8  /* status: a fragment of a datagram that did not complete here */
#define MGENX_DEFRAG_MAX_FRAGS 64
typedef struct {
    uint64_t n_fragments;    /* valid fragments that entered the state machine */
    uint64_t n_datagrams;    /* datagrams completed */
    uint64_t n_not_udp;      /* completed datagrams rejected as UDP */
    uint64_t n_incomplete;   /* contexts dropped, expired or open at the end */
    uint64_t scratch_bytes;  /* the exact need: sum of round16(L) over completed datagrams */
} mgenx_defrag_stats;
int mgenx_pcap_defrag(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off, uint64_t buf_bytes,
                      const uint64_t* dev_pkt_off, uint32_t n, uint32_t link_type, uint32_t flags,
                      int64_t timeout_us, const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                      uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                      mgenx_addr* dev_src, mgenx_defrag_stats* stats, void* stream);
int mgenx_pcapng_defrag(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off,
                        uint64_t buf_bytes, const uint64_t* dev_pkt_off,
                        const uint64_t* dev_data_off, const uint32_t* dev_cap_len, uint32_t n,
                        uint32_t link_type, uint32_t flags, int64_t timeout_us,
                        const uint32_t* dev_rx_sec, const uint32_t* dev_rx_usec,
                        uint8_t* dev_status, uint64_t* dev_udp_off, uint32_t* dev_udp_len,
                        mgenx_addr* dev_src, mgenx_defrag_stats* stats, void* stream);

/* ---- pcap2mgen: MGEN messages sent over TCP (an option; the reference drops every packet that
 * is not UDP, pcap2mgen.cpp:425, and without these calls nothing below happens) ----
 * mgenx_pcap_tcp / mgenx_pcapng_tcp run after the parse, the snap step and the defrag step,
 * over the same packets: captured segments -> each connection's byte stream, in scratch.
 *
 * Which packets are segments.
 *   Every packet whose status is not OOB is examined.  The walk is the parse's link / IP walk,
 *   but without the 4094-byte frame rule (num = caplen): a capture taken on the sending host
 *   holds segments of up to 64 KiB before segmentation offload.
 *   - IPv4: ihl >= 20, tot >= ihl, ip0 + tot <= wire length (SLL: the captured length, as the
 *     parse), not a fragment (MF == 0 and off == 0), protocol 6.
 *   - IPv6: the fixed header's next header is 6.  No extension headers are opened.
 *   - l4 is the IP payload start and ip_end = ip0 + tot (v6: ip0 + 40 + pl).  Ethernet padding
 *     past ip_end is not payload.
 *   - The 20 TCP header bytes must lie inside num and inside ip_end.
 *     doff = (b[l4+12] >> 4) * 4 must be >= 20, and l4 + doff <= ip_end.
 *   - Anything else is not a segment and stays untouched.
 *   - A segment whose payload [l4+doff, ip_end) is not wholly inside num (ip_end > num) gets
 *     MGENX_PCAP_TRUNCATED and takes no part.
 *   - Every other segment gets MGENX_PCAP_TCP.  udp_len, udp_off and src keep what the parse
 *     wrote.
 *   - Key: (version, src addr, dst addr, src port, dst port).  One direction is one key.
 *
 * Streams, per key, over its segments in capture order.
 *   - A segment with SYN set whose seq differs from that of the key's latest earlier SYN
 *     segment opens a new stream with base = seq + 1.  A SYN segment's own payload is ignored.
 *     A SYN repeated with the same seq changes nothing.
 *   - Segments before the key's first SYN belong to a stream without MGENX_TCP_SYN.  Its base
 *     is the seq of the first of them that carries payload.
 *   - A segment belongs to the stream open at its position.
 *   - rel = (uint32)(seq - base).  A payload-carrying segment with rel >= 2^31 or
 *     rel + len > 2^31 is stale.  It is counted in n_stale and contributes nothing.  A stream
 *     holds at most 2 GiB.
 *   - FIN and RST delimit nothing.
 *   - A stream with no payload-carrying segment that is not stale still counts in n_streams,
 *     with len 0.
 *
 * Content of a stream.
 *   - Order its non-stale payload segments by (rel, capture index).
 *   - Let E be the largest rel + len over the segments before a segment in that order (0 for
 *     the first).  The segment contributes the piece [max(rel, E), rel + len) when that is not
 *     empty.  Left-most start wins; a retransmission contributes nothing.
 *   - The first segment in that order with rel > E is a hole.  The stream's len is E there, and
 *     the flag MGENX_TCP_GAP is set.
 *   - dropped is the sum of the piece lengths from that segment on.
 *   - Without a hole, len is the final E.
 *   - Resynchronising behind a hole is out of scope.  The framing of what follows is unknown.
 *
 * Layout.
 *   - Streams are numbered by first_pkt, the capture index of their first segment of any kind.
 *     n_segments counts a stream's segments of any kind.
 *   - Each stream with len > 0 takes a slot of round16(len) bytes at
 *     dev_buf + scratch_off + (sum of earlier slots).  The pad is zeroed.  off is absolute in
 *     dev_buf (a stream of len 0: where its empty slot would start).
 *   - scratch_bytes is the exact sum.
 *   - dev_buf + scratch_off must be 16-byte aligned.  Every packet lies below scratch_off (one
 *     reaching past it is not examined).
 *
 * Pieces.
 *   - For every piece that ends at or below its stream's len, in stream order and then offset
 *     order: dev_piece_end[k] is the absolute offset in dev_buf of the piece's end.
 *   - These are strictly increasing over all k, because slots ascend.
 *   - dev_piece_pkt[k] is the largest capture index among its stream's pieces 0..k.  This is
 *     the packet at which every byte up to there had arrived.
 *   - n_pieces <= n.  The caller gives arrays of n.
 *
 * Sizing, as mgenx_pcap_defrag.
 *   - stats (host memory) is always filled.  The call is synchronous: one read-back.
 *   - With stream_cap < n_streams, or a window below scratch_bytes, no output array, status or
 *     scratch byte changes and MGENX_ENOSPC comes back.
 * mgenx_pcapng_tcp takes the packet blocks and the data_off / cap_len of mgenx_pcapng_parse, as
 * mgenx_pcapng_defrag does. */
#define MGENX_PCAP_TCP 9          /* status: a TCP segment taken by mgenx_pcap_tcp */
#define MGENX_TCP_SYN 0x1         /* stream flags: opened by a SYN */
#define MGENX_TCP_GAP 0x2         /* cut at a hole: bytes past `len` were dropped */
typedef struct {
    mgenx_addr src, dst;
    uint64_t off, len, dropped;
    uint32_t first_pkt, n_segments, flags, rsv;
} mgenx_tcp_stream;               /* 80 bytes */
typedef struct {
    uint64_t n_segments;     /* packets given MGENX_PCAP_TCP */
    uint64_t n_streams;
    uint64_t n_gap_streams;  /* streams with MGENX_TCP_GAP */
    uint64_t n_stale;
    uint64_t dropped_bytes;  /* sum of the streams' dropped */
    uint64_t n_pieces;
    uint64_t scratch_bytes;  /* the exact need: sum of round16(len) over the streams */
} mgenx_tcp_stats;
int mgenx_pcap_tcp(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off, uint64_t buf_bytes,
                   const uint64_t* dev_pkt_off, uint32_t n, uint32_t link_type, uint32_t flags,
                   uint8_t* dev_status, mgenx_tcp_stream* dev_streams, uint32_t stream_cap,
                   uint64_t* dev_piece_end, uint32_t* dev_piece_pkt, mgenx_tcp_stats* stats,
                   void* stream);
int mgenx_pcapng_tcp(mgenx_ctx* ctx, uint8_t* dev_buf, uint64_t scratch_off, uint64_t buf_bytes,
                     const uint64_t* dev_pkt_off, const uint64_t* dev_data_off,
                     const uint32_t* dev_cap_len, uint32_t n, uint32_t link_type, uint32_t flags,
                     uint8_t* dev_status, mgenx_tcp_stream* dev_streams, uint32_t stream_cap,
                     uint64_t* dev_piece_end, uint32_t* dev_piece_pkt, mgenx_tcp_stats* stats,
                     void* stream);
/* mgenx_tcp_frame: the rebuilt streams -> records, in completion order.
 *   - Per stream, the records are those mgenx_stream_scan(MGENX_SCAN_TCP) finds in
 *     [off, off + len) alone.  dev_stream_status[s] is that scan's status.  A record cut by the
 *     stream's end is not a record.
 *   - Per record, rec_pkt = dev_piece_pkt[k], where k is the first piece with
 *     piece_end >= rec_off + rec_len.  rx_sec / rx_usec are that packet's (dev_pkt_rx_*: the
 *     parse's per-packet times).  src is the stream's src.
 *   - Output order is by (rec_pkt, stream number, offset).  Within a stream this is chain
 *     order, because piece_pkt never decreases.  So dev_rec_pkt is non-decreasing and can be
 *     mgenx_text_interleave's MGENX_TEXT_OWNER index as it is.
 *   - Two passes.  *n_records (host memory) is always set.  The record arrays are written only
 *     when it fits cap; dev_stream_status (n_streams bytes) always.  Synchronous.
 *   - Streams of at least long_bytes go through the parallel scan of mgenx_stream_scan, one
 *     stream at a time.  The others take one lane per stream, following offset += msg_len.
 *     long_bytes 0 selects the default, 4 MiB. */
int mgenx_tcp_frame(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                    const mgenx_tcp_stream* dev_streams, uint32_t n_streams,
                    const uint64_t* dev_piece_end, const uint32_t* dev_piece_pkt,
                    uint32_t n_pieces, const uint32_t* dev_pkt_rx_sec,
                    const uint32_t* dev_pkt_rx_usec, uint64_t long_bytes, uint64_t* dev_rec_off,
                    uint32_t* dev_rec_len, uint32_t* dev_rec_stream, uint32_t* dev_rec_pkt,
                    mgenx_addr* dev_rec_src, uint32_t* dev_rec_rx_sec, uint32_t* dev_rec_rx_usec,
                    uint64_t cap, uint8_t* dev_stream_status, uint64_t* n_records, void* stream);

/* ---- MgenMsg::ConvertBinaryLog: binary log -> text log (src/common/mgenMsg.cpp:1417-1900) --
 * mgenx_binlog_index (HOST memory, no device work) checks the header line ("mgen
 * version=<4|5> ... type=binary_log\n" and its NUL, :1437-1518) and walks the records
 * {type, protocol, BE recordLength <= 1024, body}: the offsets of the records the reference
 * converts go to rec_off (host memory), up to the first one it stops at -- info->status:
 * MGENX_BINLOG_OK (end of file), _HEADER (not a binary log), _TOO_LONG (recordLength > 1024),
 * _EVENT (RERR or an unknown event type, or an unknown address type: the reference returns
 * false there, :1586-1590, 1892-1895), _SHORT (the file ends inside a record, or a record is
 * too short for the fields its type reads -- the event time; RECV 12 + source length; LISTEN
 * / IGNORE 12; JOIN / LEAVE 13 + group length + name length; ON ... RECONNECT 18 + address
 * length -- which mgen never writes and the reference would parse from stale buffer bytes).
 * mgenx_convert_binary_log (device) writes the text the reference writes for those records,
 * in order: RECV (Unpack of the stored message + LogRecvEvent text with the source and event
 * time, the converter's argument order at :1607 putting log_flush in the ttl slot, then the
 * REPORT lines of MGEN_DATA items), SEND (Unpack + LogSendEvent text: tx time, srcPort 0),
 * LISTEN / IGNORE / JOIN / LEAVE / START / STOP / ON / ACCEPT / CONNECT / DISCONNECT / OFF /
 * SHUTDOWN / RECONNECT lines (:1628-1891).  A RECV / SEND record whose stored message Unpack
 * rejects (mgen never writes one) is logged all the same, as the reference ignores Unpack's
 * result: the fields a fresh MgenMsg keeps, RECV's tx time = the event time.  flags: MGENX_BINLOG_NO_RX (log_rx off),
 * MGENX_BINLOG_FLUSH (log_flush on); opts: MGENX_LOG_EPOCH / _NO_DATA / _NO_GPS.
 * dev_rec_pos[n + 1] = byte offsets of each record's text; dev_text is written only when the
 * total fits text_cap.  Synchronous (intermediate sizes are read back); the context keeps a
 * workspace that grows with the log. */
#define MGENX_BINLOG_OK       0
#define MGENX_BINLOG_HEADER   1
#define MGENX_BINLOG_TOO_LONG 2
#define MGENX_BINLOG_EVENT    3
#define MGENX_BINLOG_SHORT    4
#define MGENX_BINLOG_NO_RX  0x1
#define MGENX_BINLOG_FLUSH  0x2
typedef struct {
    uint64_t n_records;   /* records to convert (only the first cap offsets are written) */
    uint64_t consumed;    /* bytes up to the end of the last of them */
    int32_t  status;      /* MGENX_BINLOG_* */
    uint32_t version;     /* the header line's major version */
} mgenx_binlog_info;
int mgenx_binlog_index(const uint8_t* buf, uint64_t nbytes, uint64_t* rec_off, uint64_t cap,
                       mgenx_binlog_info* info);
int mgenx_convert_binary_log(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                             const uint64_t* dev_rec_off, uint32_t n, uint32_t flags,
                             uint32_t opts, char* dev_text, uint64_t text_cap,
                             uint64_t* dev_rec_pos, void* stream);

/* ---- text log ingest: MGEN text log -> columns (the inverse of the text formatters) ----
 * The lines `mgen output <file>`, pcap2mgen and ConvertBinaryLog write (doc/mgen.xml, "MGEN Log
 * File Format"), read back into the columns mgenx_flow_lookup / mgenx_flow_reduce take.
 * Line grammar ("text log ingest"):
 *   <ts> SP+ <EVENT> (SP+ <key>'>'<value>)* SP* [CR] LF
 * <ts> is "HH:MM:SS.uuuuuu" or "<sec>.uuuuuu", told apart per token.  RECV, RERR and SEND
 * lines have their keys parsed (unknown keys are skipped); every other event gives its code
 * and timestamp only.  An empty line is MGENX_EVENT_NONE with status OK.
 *
 * mgenx_text_index: line k = dev_text[dev_line_off[k], dev_line_off[k + 1]) including its
 * LF; dev_n_lines[0] = the line count (a final non-empty piece without LF counts).
 * dev_line_off holds cap + 1 entries and is written only when the count fits cap (the
 * two-pass convention of mgenx_log_recv_text: read dev_n_lines[0] and call again).
 * Asynchronous; the context keeps a workspace (about nbytes / 2048 bytes), so these calls run on
 * one stream at a time per context. */
#define MGENX_EVENT_NONE        0   /* LogEventType (include/mgenGlobals.h:36-56) */
#define MGENX_EVENT_RECV        1
#define MGENX_EVENT_RERR        2
#define MGENX_EVENT_SEND        3
#define MGENX_EVENT_LISTEN      4
#define MGENX_EVENT_IGNORE      5
#define MGENX_EVENT_JOIN        6
#define MGENX_EVENT_LEAVE       7
#define MGENX_EVENT_START       8
#define MGENX_EVENT_STOP        9
#define MGENX_EVENT_ON         10
#define MGENX_EVENT_ACCEPT     11
#define MGENX_EVENT_DISCONNECT 12
#define MGENX_EVENT_CONNECT    13
#define MGENX_EVENT_OFF        14
#define MGENX_EVENT_SHUTDOWN   15
#define MGENX_EVENT_RECONNECT  16
#define MGENX_EVENT_REPORT     17   /* not a LogEventType: REPORT lines, classified only */
#define MGENX_PARSE_OK         0
#define MGENX_PARSE_MALFORMED  1
#define MGENX_HAS_HOST   0x01       /* mgenx_logparse_out.present: optional keys on the line */
#define MGENX_HAS_TTL    0x02
#define MGENX_HAS_GPS    0x04
#define MGENX_HAS_DATA   0x08
#define MGENX_HAS_FLAGS  0x10
#define MGENX_ERROR_NOT_RECV 0x20   /* cols.err of every line that is not an OK RECV / RERR */
#define MGENX_PARSE_NO_DAYS  0x1    /* opts: legacy stamps stay times of day */

int mgenx_text_index(mgenx_ctx* ctx, const char* dev_text, uint64_t nbytes,
                     uint64_t* dev_line_off, uint64_t cap, uint64_t* dev_n_lines, void* stream);

/* mgenx_log_parse_text: n lines -> one element per line in every array given.  A line is
 * MGENX_PARSE_OK iff its timestamp parses, its event is known, every required key is there
 * (RECV: proto flow seq src dst sent size; RERR: type src; SEND: proto flow seq srcPort dst
 * size) and every known key's value is valid and fits its field; else MGENX_PARSE_MALFORMED,
 * its other outputs unspecified.  Absent optional fields read 0 (ttl -1).
 * cols.err: 0 for an OK RECV line, the RERR code (MGENX_ERROR_RERR_NONE for "none") for an OK
 * RERR line, MGENX_ERROR_NOT_RECV for every other line -- so the columns go to
 * mgenx_flow_lookup as they are (those lines map to MGENX_FLOW_NONE and mgenx_flow_reduce skips
 * them).
 * Legacy stamps hold the time of day only: rx_sec = day_base_sec + 86400 * wraps + tod, where
 * wraps counts the OK legacy lines up to this one whose time of day lies more than 43200 s
 * below that of the nearest earlier OK legacy line; a legacy sent> time is put on the day among
 * {rx day - 1, rx day, rx day + 1} closest to the rx time (the earlier one on a tie).
 * MGENX_PARSE_NO_DAYS leaves both as times of day.  Epoch stamps are taken as they are.
 * The decoded data> bytes go to payload at payload_off[k] (n + 1 offsets), written only when
 * the total fits payload_cap (two passes).  Asynchronous; per-context workspace (about 48
 * bytes per line), shared with mgenx_text_index. */
typedef struct {            /* every pointer optional unless noted; n elements each */
    uint8_t*  event;        /* required: MGENX_EVENT_* */
    uint8_t*  status;       /* required: MGENX_PARSE_OK / _MALFORMED */
    uint8_t*  protocol;     /* MGENX_PROTO_*, 0 for any other proto> word */
    uint16_t* present;      /* MGENX_HAS_HOST | _TTL | _GPS | _DATA | _FLAGS */
    uint32_t* rx_sec; uint32_t* rx_usec;   /* the line's own timestamp */
    mgenx_addr* src;        /* RECV / RERR src; SEND: type 0, port = srcPort */
    int32_t*  ttl;          /* -1 when absent */
    uint32_t* size;         /* the full size> value */
    mgenx_cols cols;        /* flow_id seq_num tx_sec tx_usec msg_len (= min(size, 65535))
                               dst_port flags err dst_type dst_len dst_addr4 dst_addr payload_len
                               payload_type (0) gps_status lat_raw lon_raw alt host_*; the other
                               members and rows are ignored */
    uint8_t*  payload; uint64_t payload_cap; uint64_t* payload_off;
} mgenx_logparse_out;

int mgenx_log_parse_text(mgenx_ctx* ctx, const char* dev_text, uint64_t nbytes,
                         const uint64_t* dev_line_off, uint32_t n, uint32_t opts,
                         uint32_t day_base_sec, const mgenx_logparse_out* out, void* stream);

/* ---- binary log ingest: MGEN binary log records -> the same columns ----
 * mgenx_binlog_header (HOST memory, no device work) applies the header-line rules of
 * mgenx_binlog_index and nothing else: status MGENX_BINLOG_OK or _HEADER, version, and
 * consumed = the offset of the first record (n_records stays 0).
 *
 * mgenx_binlog_parse: n records at dev_rec_off (what mgenx_binlog_index found) -> one element
 * per record in every array of `out` that is given, with the optional-pointer rules and the
 * two-pass payload / payload_cap / payload_off convention of mgenx_log_parse_text.  opts must be
 * 0.  For record i the outputs are what mgenx_log_parse_text gives for that record's own line
 * in mgenx_convert_binary_log(flags 0, opts MGENX_LOG_EPOCH) -- the REPORT lines that MGEN_DATA
 * items add are not records and have no element -- except, decided from the record's bytes:
 *   ttl        -1 and MGENX_HAS_TTL clear, always: the record holds no TTL (the converter's
 *              ttl> value is its log_flush flag, mgenMsg.cpp:1607).
 *   rejected   a RECV / SEND record whose stored message Unpack rejects (shorter than 28 bytes,
 *              version not 2, unknown destination type) has event set, status
 *              MGENX_PARSE_MALFORMED and its other outputs unspecified (the converter logs a
 *              fresh MgenMsg's members there).
 *   values the text grammar refuses (tx_usec or an event's usec >= 10^6 ...) are kept as they
 *              are, status OK.
 *   SEND       rx_sec / rx_usec = the stored message's tx time (the record has no event time,
 *              mgenMsg.cpp:1152-1209; it is the converted line's stamp too); src all zero (type
 *              0, port 0: the record has no source port); size = the stored mgen_msg_len word
 *              for a TCP SEND, the header's msg_len otherwise; cols.tx_sec / tx_usec 0.
 *   others     LISTEN ... RECONNECT and START / STOP: event, the stamp, status OK, cols.err
 *              MGENX_ERROR_NOT_RECV, protocol 0, the rest 0 (ttl -1).
 *   cols.err   0 for an OK RECV record only (a binary log never holds RERR).
 * Where the text route agrees, so does this one: a source, destination or host address whose
 * length does not fit its type (the converter prints "(invalid)") is MGENX_PARSE_MALFORMED; a
 * RECV whose GPS status is unknown has no GPS, data or flags (LogRecvEvent ends the line
 * there); cols.flags holds the CONTINUES / END_OF_MSG / CHECKSUM_ERROR bits only; the data>
 * bytes start at the word-floored end of the message header (payload_data) and are there for
 * payload type 0 only; a message too short for its GPS fields reads INVALID,0,0,0.
 * A record the index would have stopped at (short for its type, RERR, unknown event, cut by
 * buf_bytes) is MGENX_PARSE_MALFORMED: no read leaves [rec_off[i], rec_off[i] + 4 +
 * recordLength) nor buf_bytes.  Asynchronous; n == 0 is legal; with payload_off the context
 * keeps a workspace (16 bytes per record), shared with mgenx_log_parse_text. */
int mgenx_binlog_header(const uint8_t* buf, uint64_t nbytes, mgenx_binlog_info* info);
int mgenx_binlog_parse(mgenx_ctx* ctx, const uint8_t* dev_buf, uint64_t buf_bytes,
                       const uint64_t* dev_rec_off, uint32_t n, uint32_t opts,
                       const mgenx_logparse_out* out, void* stream);

/* ---- a sender's log joined with a receiver's log: per-message loss ----
 * A sender logging SEND lines (TXLOG) and a receiver logging RECV lines is the manual's basic
 * workflow.  On the UDP and TCP paths the SEND line carries the message's own tx_time
 * (mgenTransport.cpp:1060,1392,1805 -> mgenMsg.cpp:1213), which is the RECV line's sent> field,
 * and flow id, sequence number and destination are on both lines: the join is exact.  No
 * reference code: the definition below is the contract.  Integer arithmetic only; every output
 * byte is a function of the inputs alone, whatever the launch geometry and whichever workgroup
 * finishes first.
 *
 * Inputs: two record sets as device columns, with flow indices from one shared numbering:
 *   send  (ns records, sender-log order):   flow_idx seq t_sec t_usec (the SEND line's stamp)
 *                                           len (the u32 size)
 *   recv  (nr records, receiver-log order): flow_idx seq tx_sec tx_usec (sent>) rx_sec rx_usec
 * A record whose flow_idx >= n_flows (MGENX_FLOW_NONE included) is skipped and counted in
 * stats.send_skipped / stats.recv_skipped.
 * Identity of a message: (flow_idx, seq, sec, usec) compared as plain u32 values, from t_* on the
 * send side and tx_* on the recv side; with MGENX_MATCH_NO_TIME, (flow_idx, seq) only (SINK-sent
 * logs, whose SEND stamp is the wall clock, mgenAppSinkTransport.cpp:191, and logs whose two
 * time-stamp styles cannot be reconciled).
 * Owner: among the counted send records of equal identity the one with the lowest index; the
 * others are send duplicates.
 * Per send record i (always written):
 *   send_rx_count[i]  for an owner the number of counted recv records with its identity; 0 for a
 *                     send duplicate or a skipped record
 *   send_first_rx[i]  for an owner the lowest such recv index, else MGENX_MATCH_NONE
 * Per recv record j: recv_send[j] = its owner's index, or MGENX_MATCH_NONE (skipped or no owner).
 * Per flow, over the flow's owners in send-log order (an owner is delivered iff its
 * send_rx_count > 0):
 *   sent, sent_bytes            owners; sum of their len
 *   send_dup                    send duplicates
 *   delivered, delivered_bytes  delivered owners; sum of their len
 *   rx_dup                      sum of send_rx_count - 1 over delivered owners
 *   rx_orphan                   counted recv records of this flow with no owner
 *   lost_head                   undelivered owners before the first delivered one (sent if none
 *                               was delivered)
 *   lost_tail                   undelivered owners after the last delivered one (0 if none was)
 *   loss_runs, loss_run_max     maximal runs of consecutive undelivered owners (send duplicates
 *                               do not break a run; head and tail runs count); the longest
 *   loss_run_hist[k]            runs with min(floor(log2(length)), 17) == k
 *   lat_sum, lat_min, lat_max   over delivered owners, signed 64-bit microseconds
 *                               (rx_sec - t_sec) * 10^6 + rx_usec - t_usec with the u32 values
 *                               widened first and rx_* of recv record send_first_rx;
 *                               INT64_MAX / INT64_MIN while delivered == 0; the sum wraps
 * sent - delivered is the exact loss; lost_head + lost_tail the part no receiver-only analysis
 * sees.  Global: send_skipped, recv_skipped, recv_unmatched (counted recv records with no owner:
 * the sum of rx_orphan) and send_dup (the sum over the flows).
 *
 * mgenx_msg_match: asynchronous; every output is fully written (no init call; a flow without
 * records gets the empty values); ns == 0 and nr == 0 are legal.  One call per pair of logs: it
 * does not stream across calls.  The context keeps the workspace (at most about 64 bytes per send
 * record, the stable sort's share included, plus 4 (n_flows + 1)), so the call runs on one
 * stream at a time per context and synchronises only when the workspace must grow.
 * MGENX_EINVAL: a null required pointer (the columns of an empty side and, with n_flows == 0,
 * dev_flows may be null), ns above 2^30, nr or n_flows above 2^31 - 1.
 *
 * mgenx_match_side prepares a parsed log (mgenx_log_parse_text) for mgenx_flow_lookup:
 * dev_err_out[k] = 0 exactly for an MGENX_PARSE_OK line of `want_event` (MGENX_EVENT_SEND or
 * MGENX_EVENT_RECV), else MGENX_ERROR_NOT_RECV; dev_src_out[k] = the line's src with the address
 * cleared (type 0, length 0, address bytes 0) and the port kept.  Given as cols.err and dev_src,
 * a SEND line (which has srcPort only) and the RECV line of the same flow then give
 * mgenx_flow_lookup the same key: dst addr, dst port, src port, flow id.  Call the lookup once
 * for the sender log and once for the receiver log on one table, sender first: flows are numbered
 * by first SEND line, receiver-only flows after them. */
#define MGENX_MATCH_NONE    0xFFFFFFFFu
#define MGENX_MATCH_NO_TIME 0x1
struct mgenx_flow_match {            /* 256 B */
  uint64_t sent, sent_bytes, send_dup;
  uint64_t delivered, delivered_bytes, rx_dup, rx_orphan;
  uint64_t lost_head, lost_tail, loss_runs, loss_run_max;
  uint64_t loss_run_hist[18];
  int64_t  lat_sum, lat_min, lat_max;
};
struct mgenx_match_stats {           /* 32 B */
  uint64_t send_skipped, recv_skipped, recv_unmatched, send_dup;
};
int mgenx_match_side(mgenx_ctx* ctx, const uint8_t* dev_event, const uint8_t* dev_status,
                     const mgenx_addr* dev_src, uint32_t n, uint32_t want_event,
                     mgenx_addr* dev_src_out, uint8_t* dev_err_out, void* stream);
int mgenx_msg_match(mgenx_ctx* ctx, const uint32_t* dev_send_flow_idx,
                    const uint32_t* dev_send_seq, const uint32_t* dev_send_t_sec,
                    const uint32_t* dev_send_t_usec, const uint32_t* dev_send_len, uint32_t ns,
                    const uint32_t* dev_recv_flow_idx, const uint32_t* dev_recv_seq,
                    const uint32_t* dev_recv_tx_sec, const uint32_t* dev_recv_tx_usec,
                    const uint32_t* dev_recv_rx_sec, const uint32_t* dev_recv_rx_usec,
                    uint32_t nr, uint32_t n_flows, uint32_t opts, uint32_t* dev_send_rx_count,
                    uint32_t* dev_send_first_rx, uint32_t* dev_recv_send,
                    struct mgenx_flow_match* dev_flows, struct mgenx_match_stats* dev_stats,
                    void* stream);

/* ---- the same join on the sender's time axis: loss per send-time window, and the loss runs ----
 * mgenx_msg_match_ex is mgenx_msg_match (the same arguments, the same outputs, the same bytes)
 * plus a timeline of up to three optional parts, all in mgenx_msg_match's terms: counted record,
 * identity, owner, send duplicate, delivered.  With tl == NULL, or a timeline with all three
 * parts off, the call is mgenx_msg_match: the same launches and the same bytes.
 *
 * Owner column (dev_send_owner, ns elements; null: not wanted): dev_send_owner[i] = the lowest
 * index among the counted send records with record i's identity (i itself for an owner), or
 * MGENX_MATCH_NONE for a skipped record.
 *
 * Send stamp of record i: t = t_sec[i] * 10^6 + t_usec[i], the u32 values widened to signed 64
 * bit first; a t_usec >= 10^6 is taken as it is.  The latency of a delivered owner is
 * mgenx_msg_match's: the rx stamp of recv record send_first_rx minus t.
 *
 * Series (n_bins > 0): dev_bins[f * n_bins + b] is the window [t0_us + b width_us,
 * t0_us + (b + 1) width_us) of send time of flow f.  For every owner i of flow f,
 * b = floor((t - t0_us) / width_us), a signed floor; outside [0, n_bins) the owner adds 1 to
 * dev_outside[f] and touches no bin; else the cell takes sent += 1 and sent_bytes += len, and
 * when the owner is delivered also delivered += 1, delivered_bytes += len,
 * rx_dup += send_rx_count - 1, and lat_sum / lat_min / lat_max from the latency.  Send duplicates
 * and skipped records count nowhere: under MGENX_MATCH_NO_TIME a duplicate may carry another
 * stamp, and only the owner's stamp places the message.  Every cell and every dev_outside
 * element is written on every call (no init call); an empty cell holds zeros, INT64_MAX and
 * INT64_MIN.  Over a flow with outside == 0 the bins sum to mgenx_flow_match's sent, sent_bytes,
 * delivered, delivered_bytes, rx_dup and (wrapping) lat_sum, and the extreme of the bins' minima
 * and maxima is the flow's lat_min / lat_max.
 *
 * Run list (dev_n_runs non-null): the runs are mgenx_msg_match's, maximal runs of consecutive
 * undelivered owners of a flow in send-log order; send duplicates are transparent, head and tail
 * runs count.  One mgenx_loss_run per run with length >= max(min_run, 1), ordered by flow_idx,
 * then by first_send.  first_send and last_send are the run's first and last undelivered owner
 * (never a send duplicate next to it), t_first_us / t_last_us their send stamps.
 * MGENX_RUN_HEAD: no delivered owner of the flow before the run; MGENX_RUN_TAIL: none after it (a
 * flow never delivered has one run with both).  dev_n_runs[0] = the number of such runs, always
 * written; dev_runs[0 .. count) is written only when count <= run_cap, else not one byte of
 * dev_runs changes: call once with run_cap 0, size the list, call again (the two-pass convention
 * of mgenx_log_recv_text).  With min_run <= 1 the count is the sum of loss_runs over the flows.
 *
 * ns == 0, nr == 0 and n_flows == 0 are legal: empty cells, zero counts.  The timeline adds 8
 * bytes per send record and 20 per 1024 of them to the workspace.  MGENX_EINVAL, before any HIP
 * call, beside mgenx_msg_match's: with n_bins > 0 a width_us of 0, a t0_us outside
 * [-2^62, 2^62], n_flows * n_bins >= 2^31, or a null dev_bins or dev_outside while n_flows > 0;
 * dev_n_runs given with a null dev_runs while run_cap > 0.  Integer arithmetic only; every
 * output byte is a function of the inputs alone. */
#define MGENX_RUN_HEAD 0x1   /* no delivered owner of the flow before the run */
#define MGENX_RUN_TAIL 0x2   /* none after it (a flow never delivered: both) */
struct mgenx_match_bin {     /* 64 B; one per (flow, window of send time) */
  uint64_t sent, sent_bytes, delivered, delivered_bytes, rx_dup;
  int64_t  lat_sum, lat_min, lat_max;   /* INT64_MAX / INT64_MIN while delivered == 0; the sum wraps */
};
struct mgenx_loss_run {      /* 40 B */
  uint32_t flow_idx, length;            /* undelivered owners in the run */
  uint32_t first_send, last_send;       /* send-record indices of its first and last undelivered owner */
  uint32_t flags, rsv;                  /* MGENX_RUN_*; 0 */
  int64_t  t_first_us, t_last_us;       /* the send stamps of first_send / last_send */
};
typedef struct {             /* HOST struct; each of the three parts is optional */
  int64_t  t0_us; uint64_t width_us; uint32_t n_bins;   /* n_bins == 0: no series */
  uint32_t min_run;                                      /* 0 is taken as 1 */
  struct mgenx_match_bin* dev_bins;    /* [n_flows * n_bins], row f = flow f */
  uint64_t* dev_outside;               /* [n_flows] */
  struct mgenx_loss_run* dev_runs; uint64_t run_cap;
  uint64_t* dev_n_runs;                /* null: no run list */
  uint32_t* dev_send_owner;            /* [ns], null: not wanted */
} mgenx_match_timeline;
int mgenx_msg_match_ex(mgenx_ctx* ctx, const uint32_t* dev_send_flow_idx,
                       const uint32_t* dev_send_seq, const uint32_t* dev_send_t_sec,
                       const uint32_t* dev_send_t_usec, const uint32_t* dev_send_len, uint32_t ns,
                       const uint32_t* dev_recv_flow_idx, const uint32_t* dev_recv_seq,
                       const uint32_t* dev_recv_tx_sec, const uint32_t* dev_recv_tx_usec,
                       const uint32_t* dev_recv_rx_sec, const uint32_t* dev_recv_rx_usec,
                       uint32_t nr, uint32_t n_flows, uint32_t opts, uint32_t* dev_send_rx_count,
                       uint32_t* dev_send_first_rx, uint32_t* dev_recv_send,
                       struct mgenx_flow_match* dev_flows, struct mgenx_match_stats* dev_stats,
                       const mgenx_match_timeline* tl, void* stream);

/* ---- one sender's log joined with many receivers' logs: the delivery matrix ----
 * A multicast run (doc/example.mgn: the flows go to 224.225.1.2 and every listener JOINs it) has
 * one sender log and a log per receiver.  mgenx_msg_match_multi joins them in one call: which
 * receivers got each message, the exact loss per (flow, receiver) with what a late joiner
 * missed at the head, and how many messages reached all, some or none of the group over send
 * time.  No reference code: this block is the contract.  Integer arithmetic only; every output
 * byte is written on every call (no init call) and is a function of the inputs alone.
 *
 * Inputs: the send columns of mgenx_msg_match (flow_idx seq t_sec t_usec len, ns records) and
 * its recv columns plus dev_recv_rcv (u32, the receiver's index): nr records, the receivers'
 * logs one after the other, or in any other order.  n_rcv is 1..64; opts 0 or
 * MGENX_MATCH_NO_TIME.  Identity, owner, send duplicate and counted / skipped send record are
 * mgenx_msg_match's.  A recv record is counted iff flow_idx < n_flows and rcv < n_rcv; else it
 * is skipped and adds to stats.recv_skipped.  An owner is delivered to r iff at least one
 * counted recv record has its identity and rcv == r; its first arrival at r is the lowest-index
 * such record.
 *
 * Per send record i: dev_send_mask[i] (u64) has bit r set iff i is an owner delivered to r; 0 for
 * a send duplicate or a skipped record.
 * Per recv record j: dev_recv_send[j] = the owner's index or MGENX_MATCH_NONE (skipped or no
 * owner); dev_recv_first[j] (u8) = 1 iff the record is counted, has an owner and is that owner's
 * first arrival at its receiver, else 0.
 * dev_cells[f * n_rcv + r], struct mgenx_rcv_cell:
 *   delivered, delivered_bytes  owners of f delivered to r; the sum of their len
 *   rx_dup                      counted recv records of (f, r) that have an owner, minus delivered
 *   rx_orphan                   counted recv records of (f, r) with no owner
 *   lost_head                   owners of f before, in send-log order, the first owner delivered
 *                               to r; the flow's sent when none was
 *   lost_tail                   owners after the last owner delivered to r; 0 when none was
 *   first_send, last_send       the send-record indices of those two owners, or MGENX_MATCH_NONE
 *   lat_sum, lat_min, lat_max   signed 64-bit microseconds over the owners delivered to r: the rx
 *                               stamp of the first arrival at r minus the owner's send stamp,
 *                               widened as mgenx_msg_match_ex states; INT64_MAX / INT64_MIN in
 *                               an empty cell; the sum wraps
 * The loss at r is sent - delivered; its middle part sent - delivered - lost_head - lost_tail.
 * dev_fanout[f], struct mgenx_flow_fanout: sent, sent_bytes, send_dup as in mgenx_flow_match;
 * deliveries = the sum over the owners of popcount(mask); reached_all = owners whose mask has
 * all n_rcv bits; reach_hist[k] = owners with popcount(mask) == k (0 above n_rcv).
 * dev_stats: send_skipped, recv_skipped, recv_unmatched (counted recv records with no owner),
 * send_dup.
 *
 * Series (tl non-null and n_bins > 0): the windows of send time are mgenx_msg_match_ex's (signed
 * floor; dev_outside[f] counts the owners outside them).  dev_bins[f * n_bins + b], struct
 * mgenx_multi_bin, over the owners in the window: sent, sent_bytes; deliveries (the sum of
 * popcount) and delivered_bytes (len x popcount); reached_any (popcount > 0), reached_all;
 * reach_min / reach_max, the least and greatest popcount (UINT64_MAX and 0 in an empty cell).
 *
 * The loss runs per receiver, their list, and the loss that receivers share:
 * mgenx_msg_match_multi_ex below.
 *
 * Asynchronous; ns == 0, nr == 0 and n_flows == 0 are legal.  The workspace is the context's,
 * shared with mgenx_msg_match (one stream at a time per context; it synchronises only to grow):
 * 12 to 20 bytes per send record plus the stable sort's share (about 64 in all), 8 to 16 bytes
 * per recv record (the (owner, receiver) table: a power of two >= 2 nr slots of 4 B), 16 bytes
 * per cell and 12 per 1024 send records.  MGENX_EINVAL, before any HIP call: n_rcv outside
 * 1..64; ns or nr above 2^30; n_flows * n_rcv or n_flows * n_bins >= 2^31; with n_bins > 0 a
 * width_us of 0 or a t0_us outside [-2^62, 2^62]; a null required pointer (the columns and
 * per-record outputs of an empty side and, with n_flows == 0, dev_cells, dev_fanout, dev_bins
 * and dev_outside may be null). */
struct mgenx_rcv_cell {      /* 80 B; one per (flow, receiver) */
  uint64_t delivered, delivered_bytes, rx_dup, rx_orphan, lost_head, lost_tail;
  uint32_t first_send, last_send;
  int64_t  lat_sum, lat_min, lat_max;
};
struct mgenx_flow_fanout {   /* 560 B */
  uint64_t sent, sent_bytes, send_dup, deliveries, reached_all;
  uint64_t reach_hist[65];
};
struct mgenx_multi_bin {     /* 64 B; one per (flow, window of send time) */
  uint64_t sent, sent_bytes, deliveries, delivered_bytes, reached_any, reached_all;
  uint64_t reach_min, reach_max;        /* UINT64_MAX / 0 while sent == 0 */
};
typedef struct {             /* HOST struct */
  int64_t  t0_us; uint64_t width_us; uint32_t n_bins;   /* n_bins == 0: no series */
  struct mgenx_multi_bin* dev_bins;    /* [n_flows * n_bins], row f = flow f */
  uint64_t* dev_outside;               /* [n_flows] */
} mgenx_multi_timeline;
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
                          void* stream);

/* ---- the same join, plus when each receiver was cut off and which receivers lose together ----
 * mgenx_msg_match_multi_ex is mgenx_msg_match_multi (the same arguments, the same outputs, the
 * same bytes) plus up to three optional parts, all in the terms above: counted record, identity,
 * owner, send duplicate, delivered to r, send stamp, send-log order.  With lx == NULL, or with all
 * three parts off, the call is mgenx_msg_match_multi: the same launches and the same bytes.  No
 * reference code: this block is the contract.  Integer arithmetic only; every output byte is a
 * function of the inputs alone; every output asked for is written on every call (no init call).
 *
 * For flow f let O_f[0 .. sent) be its owners in send-log order, the rank of an owner its
 * position in that list, and D(k, r) = the owner of rank k was delivered to receiver r (bit r of
 * its dev_send_mask).
 *
 * Run statistics (dev_rcv_runs non-null), dev_rcv_runs[f * n_rcv + r]: the runs of (f, r) are
 * the maximal runs of consecutive ranks k with !D(k, r).  Send duplicates and skipped records are
 * transparent, head and tail runs count, and a flow with sent > 0 that never reached r has one
 * run of length sent.  loss_runs = their number, loss_run_max = the longest (0 when there is
 * none), loss_run_hist[k] = the runs with min(floor(log2(length)), 17) == k.  The run lengths of a
 * cell sum to sent - delivered, and the cell equals the loss_runs / loss_run_max / loss_run_hist
 * that mgenx_msg_match leaves for flow f on the same send records and r's recv records alone.
 *
 * Run list (dev_n_runs non-null): one mgenx_rcv_loss_run per run of any (f, r) with
 * length >= max(min_run, 1).  first_send / last_send are the send-record indices of the run's
 * first and last undelivered owner (never a send duplicate next to it), t_first_us / t_last_us
 * their send stamps, widened as mgenx_msg_match_ex states.  MGENX_RUN_HEAD: no owner of f before
 * the run was delivered to r; MGENX_RUN_TAIL: none after it was (a cell never delivered has one
 * run with both).  The order is by flow_idx, then last_send, then rcv; filtered to one receiver
 * the list is mgenx_msg_match_ex's for that receiver's records, entry for entry, with rcv where
 * that one has rsv.  dev_n_runs[0] = the number of such runs, always written;
 * dev_runs[0 .. count) is written only when count <= run_cap, else not one byte of dev_runs
 * changes (the two-pass convention of mgenx_msg_match_ex).
 *
 * Pair matrix (dev_pairs non-null), dev_pairs[(f * n_rcv + a) * n_rcv + b]: the span of (f, r)
 * is the ranks from the owner dev_cells names first_send to the one it names last_send, ends
 * included; empty when nothing was delivered to r.  The common span of (a, b) is the
 * intersection of the two spans (empty when either is, or when they do not overlap), so that a
 * late joiner's head loss and an early leaver's tail loss do not read as shared loss.  Over the
 * owners k of the common span: span = their number, lost_a = those with !D(k, a), lost_b = those
 * with !D(k, b), lost_both = those with neither.  An empty common span gives four zeros.  Entry
 * (a, b)'s lost_a is entry (b, a)'s lost_b; on the diagonal span is the receiver's own span and
 * the three loss fields equal the cell's sent - delivered - lost_head - lost_tail.
 *
 * Asynchronous; ns == 0, nr == 0 and n_flows == 0 are legal (with n_flows == 0 the three arrays
 * may be null).  Beside mgenx_msg_match_multi's workspace the parts add, whichever of them are
 * on, 20 bytes per send record, 4 (n_flows + 1), and 12 + 8 n_rcv bytes per 1024 send records
 * (nothing per cell); the call synchronises only to grow the workspace.  MGENX_EINVAL, before
 * any HIP call and with nothing written: whatever mgenx_msg_match_multi refuses; dev_pairs given
 * with n_flows * n_rcv^2 >= 2^31; dev_n_runs given with a null dev_runs while run_cap > 0. */
struct mgenx_rcv_runs {      /* 160 B; one per (flow, receiver) */
  uint64_t loss_runs, loss_run_max, loss_run_hist[18];
};
struct mgenx_rcv_loss_run {  /* 40 B; mgenx_loss_run's layout with rcv where it has rsv */
  uint32_t flow_idx, length;            /* undelivered owners in the run */
  uint32_t first_send, last_send;       /* send-record indices of its first and last undelivered owner */
  uint32_t flags, rcv;                  /* MGENX_RUN_*; the receiver */
  int64_t  t_first_us, t_last_us;       /* the send stamps of first_send / last_send */
};
struct mgenx_rcv_pair {      /* 32 B; one per (flow, receiver a, receiver b) */
  uint64_t span, lost_a, lost_b, lost_both;
};
typedef struct {             /* HOST struct; each of the three parts is optional */
  struct mgenx_rcv_runs* dev_rcv_runs;        /* [n_flows * n_rcv]; null: not wanted */
  uint32_t min_run, rsv;                      /* 0 is taken as 1 */
  struct mgenx_rcv_loss_run* dev_runs; uint64_t run_cap;
  uint64_t* dev_n_runs;                       /* null: no run list */
  struct mgenx_rcv_pair* dev_pairs;           /* [n_flows * n_rcv * n_rcv]; null: not wanted */
} mgenx_multi_loss;
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
                             const mgenx_multi_loss* lx, void* stream);

/* ---- multi-GPU exchange (RCCL over xGMI) ----
 * One communicator per rank (one process per GPU): rank 0 calls mgenx_comm_unique_id and
 * hands the MGENX_COMM_ID_BYTES bytes to every rank (any out-of-band channel), then every
 * rank calls mgenx_comm_init.  Collectives are asynchronous on `stream`. */
typedef struct mgenx_comm mgenx_comm;
#define MGENX_COMM_ID_BYTES 128
int mgenx_comm_unique_id(void* id_out);
int mgenx_comm_init(mgenx_ctx* ctx, int nranks, int rank, const void* id, mgenx_comm** out);
int mgenx_comm_destroy(mgenx_comm* comm);
/* The per-flow counter merge after flow-sharded mgenx_flow_reduce: in-place SUM of
 * n_flows x 64 B over the ranks (one ncclAllReduce).  Exact when every flow has one owner and
 * the other ranks export zeros for it (mgenx_flow_export of a flow never updated there):
 * integer sums of the 64-bit words leave the owner's counters, FP64 fields included, bit for
 * bit. */
int mgenx_allreduce_flows(mgenx_ctx* ctx, mgenx_comm* comm, mgenx_flow_counters* dev_counters,
                          uint32_t n_flows, void* stream);
/* dev_out[r * count + k] = rank r's dev_in[k] (the stream-shard stitch). */
int mgenx_allgather_u64(mgenx_ctx* ctx, mgenx_comm* comm, const uint64_t* dev_in,
                        uint64_t* dev_out, uint32_t count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
