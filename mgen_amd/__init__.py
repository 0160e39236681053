"""mgen_amd -- MI355X-native MgenMsg pack/parse engine (host binding).

Thin ctypes binding of the C ABI in ``include/mgenx.h`` (libmgenx.so, built from
``mgen_amd/csrc`` for gfx950).  PyTorch is used only for device memory and streams.
There is no CPU fallback: if the HIP library is missing, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._abi import (  # noqa: F401
    COLS_CORE, COLS_DEC, COLS_EXT, DESC_DTYPE, TMPL_DTYPE, MgenxCols, ERROR_CHECKSUM, ERROR_DSTADDR,
    ERROR_LENGTH, ERROR_NONE, ERROR_OOB, ERROR_VERSION, FLAG_CHECKSUM, FLAG_CHECKSUM_ERROR,
    FLAG_LAST_BUFFER, OPT_CHECKSUM_FORCE, OPT_SKIP_CRC, OPT_TCP, PACK_CHECKSUM,
    PACK_RANDOM_FILL, SCAN_SINK, SCAN_TCP, ScanInfo, FLOW_COUNTERS_DTYPE, FLOW_REPORT_DTYPE,
    FLOW_STATE_BYTES, FLOW_STATE_DTYPE, REC_DTYPE, PACK_RAW, DEC_MSGLEN, DEC_BASE, DEC_DST,
    DEC_HDRLEN, DEC_HOST, DEC_GPS, DEC_PTYPE, DEC_PLEN, RX_NOLOG, RX_FORCE, RX_PREV,
    RX_STATE_DTYPE, SCAN_HALO, SCAN_REUSE, ADDR_DTYPE, REPORT_KEY_DTYPE, DATA_CONTROLLER,
    PcapInfo, TextSrc, TEXT_PER_RECORD, TEXT_OWNER, TEXT_MAP, TEXT_SCATTER, PCAP_NSEC, PCAP_SWAPPED, LOG_EPOCH, LOG_NO_DATA, LOG_NO_GPS,
    LOG_SKIP_ERR, FLOW_NONE, DLT_EN10MB, DLT_LINUX_SLL, BinlogInfo, BINLOG_NO_RX, BINLOG_FLUSH,
    UNPACK_K_HEADER, UNPACK_K_GENERAL, UNPACK_K_VAR, UNPACK_K_FIXED, UNPACK_K_FIXED_RING,
    UNPACK_K_OTHER, UNPACK_K_LONG, UNPACKED_DTYPE,
    EVENT_NONE, EVENT_RECV, EVENT_RERR, EVENT_SEND, EVENT_REPORT, PARSE_OK, PARSE_MALFORMED,
    HAS_HOST, HAS_TTL, HAS_GPS, HAS_DATA, HAS_FLAGS, ERROR_RERR_NONE, ERROR_NOT_RECV,
    PARSE_NO_DAYS, LOGPARSE_COLS, LogparseOut,
    PCAP_NG, PcapngInfo, PCAPNG_IF_DTYPE, PCAPNG_OK, PCAPNG_TRUNCATED, PCAPNG_BLOCK,
    PCAPNG_SECTION, PCAPNG_LINKTYPE, PCAPNG_NO_IFACE, PCAPNG_TSRESOL, PCAPNG_CAPLEN,
    FLOW_DIST_BINS, FLOW_DIST_DTYPE, FLOW_SERIES_BIN_DTYPE, FLOW_SERIES_STATE_DTYPE,
    ENOSPC, PCAP_FRAGMENT, DEFRAG_MAX_FRAGS, DefragStats,
    PCAP_TCP, TCP_SYN, TCP_GAP, TCP_STREAM_DTYPE, TcpStats,
    MATCH_NONE, MATCH_NO_TIME, MATCH_RUN_BINS, FLOW_MATCH_DTYPE, MATCH_STATS_DTYPE,
    RUN_HEAD, RUN_TAIL, MATCH_BIN_DTYPE, LOSS_RUN_DTYPE, MatchTimeline,
    BINLOG_OK, BINLOG_HEADER, BINLOG_TOO_LONG, BINLOG_EVENT, BINLOG_SHORT,
    CLOCK_NONE, CLOCK_OFFSET_ONLY, FLOW_CLOCK_DTYPE,
    MATCH_MAX_RCV, RCV_CELL_DTYPE, FLOW_FANOUT_DTYPE, MULTI_BIN_DTYPE, MultiTimeline,
    RCV_RUNS_DTYPE, RCV_LOSS_RUN_DTYPE, RCV_PAIR_DTYPE, MultiLoss,
)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmgenx.so")
DIAG_LIB_PATH = os.path.join(HERE, "libmgenx_diag.so")   # + include/mgenx_diag.h

# every function include/mgenx.h declares (tests/test_abi_cpu.py checks the header agrees)
EXPORTED_SYMBOLS = (
    "mgenx_abi_version", "mgenx_ctx_create", "mgenx_ctx_destroy", "mgenx_last_error",
    "mgenx_ctx_device", "mgenx_unpack_batch", "mgenx_pack_prepare", "mgenx_set_fill_time",
    "mgenx_pack_batch", "mgenx_pack_msgs", "mgenx_pack_tcp", "mgenx_crc32_update", "mgenx_crc32_batch",
    "mgenx_tcp_rx_persist", "mgenx_report_build", "mgenx_log_report_text", "mgenx_data_walk",
    "mgenx_log_report_recv_text", "mgenx_log_send_text", "mgenx_log_send_binary",
    "mgenx_stream_scan", "mgenx_stream_scan_exits", "mgenx_stream_scan_range", "mgenx_flow_init", "mgenx_flow_reduce", "mgenx_flow_export",
    "mgenx_log_recv_text", "mgenx_log_recv_binary", "mgenx_comm_unique_id", "mgenx_comm_init",
    "mgenx_comm_destroy", "mgenx_allreduce_flows", "mgenx_allgather_u64",
    "mgenx_flow_table_create", "mgenx_flow_table_destroy", "mgenx_flow_lookup",
    "mgenx_flow_reduce_ex", "mgenx_flow_keys", "mgenx_flow_span", "mgenx_text_interleave",
    "mgenx_pcap_index",
    "mgenx_pcap_parse", "mgenx_binlog_index", "mgenx_convert_binary_log",
    "mgenx_unpack_last_kernel", "mgenx_pcap_snap", "mgenx_flow_reduce_rows",
    "mgenx_worker_create", "mgenx_worker_destroy", "mgenx_worker_unpack", "mgenx_worker_crc32",
    "mgenx_worker_pack", "mgenx_worker_stop", "mgenx_worker_info", "mgenx_worker_recv",
    "mgenx_worker_flow_update", "mgenx_text_index", "mgenx_log_parse_text",
    "mgenx_pcapng_index", "mgenx_pcapng_parse", "mgenx_pcapng_snap",
    "mgenx_flow_dist_init", "mgenx_flow_dist", "mgenx_flow_dist_quantiles",
    "mgenx_flow_dist_bin", "mgenx_flow_dist_bin_lo",
    "mgenx_flow_series_init", "mgenx_flow_series", "mgenx_flow_series_quantiles",
    "mgenx_pcap_defrag", "mgenx_pcapng_defrag",
    "mgenx_pcap_tcp", "mgenx_pcapng_tcp", "mgenx_tcp_frame",
    "mgenx_match_side", "mgenx_msg_match", "mgenx_flow_clock", "mgenx_msg_match_ex",
    "mgenx_msg_match_multi", "mgenx_binlog_header", "mgenx_binlog_parse",
    "mgenx_msg_match_multi_ex",
)
DIAG_SYMBOLS = ("mgenx_set_tuning", "mgenx_diag_stream_read", "mgenx_diag_group_rw",
                "mgenx_diag_seg_prof", "mgenx_diag_stream_read_w", "mgenx_diag_worker_stamps",
                "mgenx_diag_chain_prof", "mgenx_diag_c1_giveups", "mgenx_diag_blockscan",
                "mgenx_diag_chunk_carry")


class MgenxError(RuntimeError):
    pass


_libs = {}


def load(diag: bool = False):
    """Load libmgenx.so (or the diagnostics build libmgenx_diag.so); fails loudly when the
    HIP build is missing."""
    path = DIAG_LIB_PATH if diag else LIB_PATH
    # geometry experiments (scripts/*_exp.sh): another build of the same sources
    path = os.environ.get("MGENX_LIB_OVERRIDE", path)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise MgenxError(f"{path} not built: run __graft_entry__.build() "
                         "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(path)
    P, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.mgenx_abi_version.restype = i32
    L.mgenx_ctx_create.argtypes = [i32, ctypes.POINTER(P)]
    L.mgenx_ctx_destroy.argtypes = [P]
    L.mgenx_last_error.argtypes = [P]
    L.mgenx_last_error.restype = ctypes.c_char_p
    L.mgenx_unpack_batch.argtypes = [P, P, u64, P, u64, P, u32, u32,
                                     ctypes.POINTER(MgenxCols), u32, P]
    L.mgenx_unpack_last_kernel.argtypes = [P]
    L.mgenx_unpack_last_kernel.restype = i32
    L.mgenx_pack_prepare.argtypes = [P, P, u32, P, P, P]
    L.mgenx_set_fill_time.argtypes = [P, u32]
    L.mgenx_pack_batch.argtypes = [P, P, P, P, u32, P, P, u64, P, u64, P, u32, u32, P]
    L.mgenx_pack_msgs.argtypes = [P, P, P, P, u32, P, P, u64, P, u64, P, P, P, P, P, u32, u32,
                                  P]
    L.mgenx_pack_tcp.argtypes = [P, P, P, P, P, u32, P, P, u64, P, ctypes.POINTER(u64), u32,
                                 u32, P]
    L.mgenx_crc32_batch.argtypes = [P, P, P, P, u32, P, P]
    L.mgenx_crc32_update.argtypes = [P, P, P, P, u32, P, P, P]
    L.mgenx_ctx_device.argtypes = [P]
    L.mgenx_comm_unique_id.argtypes = [P]
    L.mgenx_comm_init.argtypes = [P, i32, i32, P, ctypes.POINTER(P)]
    L.mgenx_comm_destroy.argtypes = [P]
    L.mgenx_allreduce_flows.argtypes = [P, P, P, u32, P]
    L.mgenx_allgather_u64.argtypes = [P, P, P, P, u32, P]
    L.mgenx_flow_table_create.argtypes = [P, u32, ctypes.POINTER(P)]
    L.mgenx_flow_table_destroy.argtypes = [P]
    L.mgenx_flow_lookup.argtypes = [P, P, ctypes.POINTER(MgenxCols), P, u32, P, P, P]
    L.mgenx_flow_reduce_ex.argtypes = [P, P, P, P, P, P, P, P, u32, P, u32, P, u32, P, P, P]
    L.mgenx_flow_keys.argtypes = [P, P, i32, P, u32, P]
    L.mgenx_flow_span.argtypes = [P, P, P, P, u32, u32, P, P, P]
    L.mgenx_text_interleave.argtypes = [P, P, u32, u32, P, u64, P, P]
    L.mgenx_pcap_index.argtypes = [P, u64, P, u64, ctypes.POINTER(PcapInfo)]
    L.mgenx_pcap_parse.argtypes = [P, P, u64, P, u32, u32, u32, P, P, P, P, P, P, P, P]
    L.mgenx_pcap_snap.argtypes = [P, P, u64, u64, P, u32, u32, P, P, P, P]
    L.mgenx_pcapng_index.argtypes = [P, u64, P, P, u64, P, u32, ctypes.POINTER(PcapngInfo)]
    L.mgenx_pcapng_parse.argtypes = [P, P, u64, P, P, u32, P, u32, u32, u32, P, P, P, P, P, P, P,
                                     P, P, P]
    L.mgenx_pcapng_snap.argtypes = [P, P, u64, u64, P, P, u32, P, P, P, P]
    L.mgenx_pcap_defrag.argtypes = [P, P, u64, u64, P, u32, u32, u32, ctypes.c_int64, P, P, P, P,
                                    P, P, ctypes.POINTER(DefragStats), P]
    L.mgenx_pcapng_defrag.argtypes = [P, P, u64, u64, P, P, P, u32, u32, u32, ctypes.c_int64, P,
                                      P, P, P, P, P, ctypes.POINTER(DefragStats), P]
    L.mgenx_pcap_tcp.argtypes = [P, P, u64, u64, P, u32, u32, u32, P, P, u32, P, P,
                                 ctypes.POINTER(TcpStats), P]
    L.mgenx_pcapng_tcp.argtypes = [P, P, u64, u64, P, P, P, u32, u32, u32, P, P, u32, P, P,
                                   ctypes.POINTER(TcpStats), P]
    L.mgenx_tcp_frame.argtypes = [P, P, u64, P, u32, P, P, u32, P, P, u64, P, P, P, P, P, P, P,
                                  u64, P, ctypes.POINTER(u64), P]
    L.mgenx_binlog_index.argtypes = [P, u64, P, u64, ctypes.POINTER(BinlogInfo)]
    L.mgenx_convert_binary_log.argtypes = [P, P, u64, P, u32, u32, u32, P, u64, P, P]
    L.mgenx_binlog_header.argtypes = [P, u64, ctypes.POINTER(BinlogInfo)]
    L.mgenx_binlog_parse.argtypes = [P, P, u64, P, u32, u32, ctypes.POINTER(LogparseOut), P]
    L.mgenx_text_index.argtypes = [P, P, u64, P, u64, P, P]
    L.mgenx_log_parse_text.argtypes = [P, P, u64, P, u32, u32, u32, ctypes.POINTER(LogparseOut),
                                       P]
    if diag:
        L.mgenx_set_tuning.argtypes = [P, i32, i32]
        L.mgenx_diag_stream_read.argtypes = [P, P, u64, P, i32, P]
        L.mgenx_diag_group_rw.argtypes = [P, P, u64, P, i32, P]
        L.mgenx_diag_seg_prof.argtypes = [P, i32]
        L.mgenx_diag_stream_read_w.argtypes = [P, P, u64, P, i32, i32, P]
        L.mgenx_diag_worker_stamps.argtypes = [P, P]
        L.mgenx_diag_chain_prof.argtypes = [P]
        L.mgenx_diag_c1_giveups.argtypes = [ctypes.POINTER(u64)]
        L.mgenx_diag_blockscan.argtypes = [i32, P, P, P, P, P]
        L.mgenx_diag_chunk_carry.argtypes = [i32, P, P, u32, P, P]
    L.mgenx_stream_scan.argtypes = [P, P, u64, i32, P, P, u64, ctypes.POINTER(ScanInfo), P]
    L.mgenx_tcp_rx_persist.argtypes = [P, P, P, P, u32, P, P, P, u32, P]
    L.mgenx_report_build.argtypes = [P, P, u32, u32, P, P, P, P, P, P, P]
    L.mgenx_log_report_text.argtypes = [P, P, P, u32, u32, P, u32, P, u64, P, P]
    L.mgenx_data_walk.argtypes = [P, P, P, u64, P, u32, u32, P, P, P, u32, P, u32, P, P]
    L.mgenx_log_report_recv_text.argtypes = [P, P, P, u32, P, P, P, u32, P, u64, P, P]
    L.mgenx_log_send_text.argtypes = [P, P, P, P, P, P, u32, i32, u32, P, u64, P, P]
    L.mgenx_log_send_binary.argtypes = [P, P, P, P, P, P, u64, P, u64, u32, i32, P, u64, P, P]
    L.mgenx_stream_scan_exits.argtypes = [P, P, u64, i32, u64, u64, P, P, u32,
                                          ctypes.POINTER(u32), P]
    L.mgenx_stream_scan_range.argtypes = [P, P, u64, i32, u64, u64, i32, P, P, u64,
                                          ctypes.POINTER(ScanInfo), P]
    L.mgenx_flow_init.argtypes = [P, P, u32, ctypes.c_double, P]
    L.mgenx_flow_reduce.argtypes = [P, P, P, P, P, P, P, P, u32, P, u32, P, u32, P, P]
    L.mgenx_flow_reduce_rows.argtypes = [P, P, P, P, P, u32, P, u32, P, u32, P, P, P]
    L.mgenx_flow_export.argtypes = [P, P, u32, P, P]
    L.mgenx_flow_dist_init.argtypes = [P, P, P, u32, P]
    L.mgenx_flow_dist.argtypes = [P, P, P, P, P, P, P, P, u32, P, P, u32, P]
    L.mgenx_flow_dist_quantiles.argtypes = [P, P, P, u32, ctypes.POINTER(u32), u32, P, P]
    L.mgenx_flow_series_init.argtypes = [P, P, P, u32, u32, P]
    L.mgenx_flow_series.argtypes = [P, P, P, P, P, P, P, P, u32, ctypes.c_int64, u64, u32, P, P,
                                    u32, P]
    L.mgenx_flow_series_quantiles.argtypes = [P, P, P, P, P, P, u32, ctypes.c_int64, u64, u32, u32,
                                              ctypes.POINTER(u32), u32, P, P]
    L.mgenx_flow_clock.argtypes = [P, P, P, P, P, P, u32, u32, u32, P, P, P, P, P]
    L.mgenx_match_side.argtypes = [P, P, P, P, u32, u32, P, P, P]
    L.mgenx_msg_match.argtypes = [P, P, P, P, P, P, u32, P, P, P, P, P, P, u32, u32, u32, P, P, P,
                                  P, P, P]
    L.mgenx_msg_match_ex.argtypes = [P, P, P, P, P, P, u32, P, P, P, P, P, P, u32, u32, u32, P, P,
                                     P, P, P, ctypes.POINTER(MatchTimeline), P]
    L.mgenx_msg_match_multi.argtypes = [P, P, P, P, P, P, u32, P, P, P, P, P, P, P, u32, u32, u32,
                                        u32, P, P, P, P, P, P, ctypes.POINTER(MultiTimeline), P]
    L.mgenx_msg_match_multi_ex.argtypes = [P, P, P, P, P, P, u32, P, P, P, P, P, P, P, u32, u32,
                                           u32, u32, P, P, P, P, P, P,
                                           ctypes.POINTER(MultiTimeline),
                                           ctypes.POINTER(MultiLoss), P]
    L.mgenx_flow_dist_bin.argtypes = [u64]
    L.mgenx_flow_dist_bin.restype = u32
    L.mgenx_flow_dist_bin_lo.argtypes = [u32]
    L.mgenx_flow_dist_bin_lo.restype = u64
    L.mgenx_log_recv_text.argtypes = [P, P, P, u64, ctypes.POINTER(MgenxCols), P, P, P, P, u32,
                                      i32, u32, P, u64, P, P]
    L.mgenx_log_recv_binary.argtypes = [P, P, u64, P, u64, P, ctypes.POINTER(MgenxCols), P, P,
                                        P, u32, i32, P, u64, P, P]
    L.mgenx_worker_create.argtypes = [P, u32, ctypes.POINTER(P)]
    L.mgenx_worker_destroy.argtypes = [P]
    L.mgenx_worker_stop.argtypes = [P]
    L.mgenx_worker_info.argtypes = [P, ctypes.POINTER(u32)]
    L.mgenx_worker_recv.argtypes = [P, ctypes.c_char_p, u32, u32, P, ctypes.POINTER(u32),
                                    ctypes.POINTER(u32)]
    L.mgenx_worker_flow_update.argtypes = [P, P, u32, u32, u32, u32, u32, u32, u32,
                                           ctypes.POINTER(u32), P]
    L.mgenx_worker_unpack.argtypes = [P, ctypes.c_char_p, u32, P]
    L.mgenx_worker_crc32.argtypes = [P, ctypes.c_char_p, u32, u32, ctypes.POINTER(u32)]
    L.mgenx_worker_pack.argtypes = [P, P, ctypes.c_char_p, P, u32, u32, u32, u32, P,
                                    ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    _libs[path] = L
    return L


def _ptr(t):
    """Raw device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    import torch
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(device))


class Engine:
    """One mgenx context on one GPU (``mgenx_ctx``)."""

    def __init__(self, device: int = 0, diag: bool = False):
        import torch
        self.torch = torch
        self.device = device
        self.lib = load(diag)
        self.ctx = ctypes.c_void_p()
        rc = self.lib.mgenx_ctx_create(device, ctypes.byref(self.ctx))
        if rc != 0:
            raise MgenxError(f"mgenx_ctx_create({device}) failed: {rc}")

    def close(self):
        if self.ctx:
            self.lib.mgenx_ctx_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.mgenx_last_error(self.ctx)
            raise MgenxError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    # ------------------------------------------------------------ single messages
    def worker(self, idle_ms: int = 200):
        """A resident single-message worker on this engine's device (mgenx_worker_*)."""
        return Worker(self, idle_ms)

    # ------------------------------------------------------------ columns
    def alloc_cols(self, n: int, ext: bool = False):
        torch = self.torch
        dev = f"cuda:{self.device}"
        cols = {name: torch.empty(n * w if w > 1 else n, dtype=getattr(torch, dt), device=dev)
                for name, dt, w in COLS_CORE}
        if ext:
            for name, dt, w in COLS_EXT + COLS_DEC:
                cols[name] = torch.empty(n * w if w > 1 else n, dtype=getattr(torch, dt),
                                         device=dev)
        return cols

    def alloc_rows(self, n: int):
        """mgenx_rec rows (32 B per record) as a uint8 tensor; pass as cols={"rows": t}."""
        return self.torch.empty(n * 32, dtype=self.torch.uint8, device=f"cuda:{self.device}")

    @staticmethod
    def _cols_struct(cols):
        s = MgenxCols()
        for name, _ in MgenxCols._fields_:
            t = cols.get(name)
            setattr(s, name, t.data_ptr() if t is not None else None)
        return s

    # ------------------------------------------------------------ unpack
    def unpack(self, slab, n, *, rec_off=None, stride=0, rec_len=None, fixed_len=0, opts=0,
               cols=None, ext=False, slab_bytes=None):
        """MgenMsg::Unpack + receive CRC check over n records (async on the current stream)."""
        if cols is None:
            cols = self.alloc_cols(n, ext)
        cs = self._cols_struct(cols)
        nbytes = slab.numel() if slab_bytes is None else slab_bytes
        rc = self.lib.mgenx_unpack_batch(self.ctx, _ptr(slab), nbytes, _ptr(rec_off), stride,
                                         _ptr(rec_len), fixed_len, n, ctypes.byref(cs), opts,
                                         _stream(self.device))
        self._check(rc, "mgenx_unpack_batch")
        return cols

    def last_unpack_kernel(self):
        """UNPACK_K_* of the kernel the last unpack() launched (mgenx_unpack_last_kernel)."""
        return int(self.lib.mgenx_unpack_last_kernel(self.ctx))

    def rx_state_init(self):
        """mgenx_rx_state of a fresh MgenMsg (GPS words 10800000 = 0 degrees), on the device."""
        from ._abi import RX_STATE_DTYPE
        st = np.zeros(1, RX_STATE_DTYPE)
        st["lat_raw"] = st["lon_raw"] = 10800000
        return self.torch.from_numpy(st.view(np.uint8).copy()).to(f"cuda:{self.device}")

    def tcp_rx_persist(self, slab, rec_off, rec_len, n, cols, state, *, payload_rec=None,
                       opts=0):
        """The TCP receiver's persistent rx_msg view of n decoded records, in place
        (mgenx_tcp_rx_persist); state: the 48-B mgenx_rx_state tensor (updated)."""
        cs = self._cols_struct(cols)
        rc = self.lib.mgenx_tcp_rx_persist(self.ctx, _ptr(slab), _ptr(rec_off), _ptr(rec_len), n,
                                           ctypes.byref(cs), _ptr(state), _ptr(payload_rec), opts,
                                           _stream(self.device))
        self._check(rc, "mgenx_tcp_rx_persist")
        return cols

    # ------------------------------------------------------------ event log
    def log_recv_text(self, slab, n, cols, src, rx_sec, rx_usec, *, rec_off=None, stride=0,
                      ttl=None, protocol=1, opts=0, text_cap=None):
        """RECV / RERR text log lines of n decoded records (mgenx_log_recv_text).  cols: the
        unpack outputs with the extended columns; src: uint8 tensor of n x 20 (mgenx_addr).
        Returns (text tensor, line offsets tensor of n + 1)."""
        torch = self.torch
        dev = slab.device
        line_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        cap = text_cap if text_cap is not None else max(1, n) * 160
        for _ in range(2):
            text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            cs = self._cols_struct(cols)
            rc = self.lib.mgenx_log_recv_text(self.ctx, _ptr(slab), _ptr(rec_off), stride,
                                              ctypes.byref(cs), _ptr(src), _ptr(rx_sec),
                                              _ptr(rx_usec), _ptr(ttl), n, protocol, opts,
                                              _ptr(text), cap, _ptr(line_off),
                                              _stream(self.device))
            self._check(rc, "mgenx_log_recv_text")
            total = int(line_off[n].item())
            if total <= cap:
                return text[:total], line_off
            cap = total
        raise MgenxError("mgenx_log_recv_text: text did not fit")

    def log_recv_binary(self, slab, n, cols, src, rx_sec, rx_usec, *, rec_off=None, stride=0,
                        rec_len=None, protocol=1, slab_bytes=None, cap=None):
        """Binary RECV / RERR log records (mgenx_log_recv_binary; rec_len: the received
        lengths, else each record's msg_len bounds its bytes).  Returns (bytes tensor,
        record positions tensor of n + 1)."""
        torch = self.torch
        dev = slab.device
        pos = torch.empty(n + 1, dtype=torch.int64, device=dev)
        cap = cap if cap is not None else max(1, n) * 128
        sb = slab.numel() if slab_bytes is None else slab_bytes
        for _ in range(2):
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            cs = self._cols_struct(cols)
            rc = self.lib.mgenx_log_recv_binary(self.ctx, _ptr(slab), sb, _ptr(rec_off), stride,
                                                _ptr(rec_len), ctypes.byref(cs), _ptr(src),
                                                _ptr(rx_sec),
                                                _ptr(rx_usec), n, protocol, _ptr(out), cap,
                                                _ptr(pos), _stream(self.device))
            self._check(rc, "mgenx_log_recv_binary")
            total = int(pos[n].item())
            if total <= cap:
                return out[:total], pos
            cap = total
        raise MgenxError("mgenx_log_recv_binary: output did not fit")

    # ------------------------------------------------------------ text log ingest
    def text_index(self, text, nbytes=None):
        """Line offsets of a text log on the device (mgenx_text_index): text is a uint8 tensor;
        returns (line_off int64 tensor of n_lines + 1, n_lines).  Line k is
        text[line_off[k]:line_off[k + 1]], its LF included."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        nbytes = text.numel() if nbytes is None else nbytes
        n_lines = torch.zeros(1, dtype=torch.int64, device=dev)
        cap = max(1, nbytes // 64)
        for _ in range(2):
            line_off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
            rc = self.lib.mgenx_text_index(self.ctx, _ptr(text), nbytes, _ptr(line_off), cap,
                                           _ptr(n_lines), _stream(self.device))
            self._check(rc, "mgenx_text_index")
            n = int(n_lines.item())
            if n <= cap:
                return line_off[:n + 1], n
            cap = n
        raise MgenxError("mgenx_text_index: line offsets did not fit")

    def log_parse_text(self, text, line_off, n, *, opts=0, day_base=0, payload=False,
                       nbytes=None):
        """Parse n text log lines into columns (mgenx_log_parse_text).  Returns a dict of
        tensors: event, status, protocol, present, rx_sec, rx_usec, src (n x 20), ttl, size,
        the mgenx_cols columns (core + extended, ready for flow_lookup / flow_reduce) and, with
        payload=True, payload (the decoded data> bytes) and payload_off (n + 1)."""
        nbytes = text.numel() if nbytes is None else nbytes

        def call(s):
            rc = self.lib.mgenx_log_parse_text(self.ctx, _ptr(text), nbytes, _ptr(line_off), n,
                                               opts, day_base, ctypes.byref(s),
                                               _stream(self.device))
            self._check(rc, "mgenx_log_parse_text")
        return self._logparse_out(n, payload, call)

    def binlog_parse(self, buf, rec_off, n, *, payload=False, nbytes=None):
        """Parse n binary log records into columns (mgenx_binlog_parse): buf is the log image
        (uint8 tensor), rec_off the record offsets (int64 tensor, from binlog_index).  Returns
        the same dict of tensors as log_parse_text, one element per record."""
        nbytes = buf.numel() if nbytes is None else nbytes

        def call(s):
            rc = self.lib.mgenx_binlog_parse(self.ctx, _ptr(buf), nbytes, _ptr(rec_off), n, 0,
                                             ctypes.byref(s), _stream(self.device))
            self._check(rc, "mgenx_binlog_parse")
        return self._logparse_out(n, payload, call)

    def _logparse_out(self, n, payload, call):
        """The output tensors of a mgenx_logparse_out, filled by call(struct) (twice when the
        payload bytes did not fit the first time)."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        m = max(n, 1)
        out = {name: torch.zeros(m * w, dtype=getattr(torch, dt), device=dev)
               for name, dt, w in LOGPARSE_COLS}
        cols = {name: torch.zeros(m * w, dtype=getattr(torch, dt), device=dev)
                for name, dt, w in COLS_CORE + COLS_EXT}
        s = LogparseOut()
        for name, _, _ in LOGPARSE_COLS:
            setattr(s, name, out[name].data_ptr())
        s.cols = self._cols_struct(cols)
        if payload:
            out["payload_off"] = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            s.payload_off = out["payload_off"].data_ptr()
        cap = 0
        for _ in range(2):
            if payload:
                out["payload"] = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
                s.payload, s.payload_cap = out["payload"].data_ptr(), cap
            call(s)
            if not payload:
                break
            total = int(out["payload_off"][n].item())
            if total <= cap:
                out["payload"] = out["payload"][:total]
                break
            cap = total
        for name, _, w in LOGPARSE_COLS:
            out[name] = out[name][:n * w]
        # mgenx_cols members the parser does not write (hdr_len, the u32 payload_off) stay out
        out.update({k: v[:n * (16 if k in ("dst_addr", "host_addr") else 1)]
                    for k, v in cols.items() if k not in ("hdr_len", "payload_off")})
        return out

    # ------------------------------------------------------------ pack
    def pack_prepare(self, tmpl, n_tmpl, pool, tmpl_crc):
        rc = self.lib.mgenx_pack_prepare(self.ctx, _ptr(tmpl), n_tmpl, _ptr(pool),
                                         _ptr(tmpl_crc), _stream(self.device))
        self._check(rc, "mgenx_pack_prepare")

    def set_fill_time(self, fill_time: int):
        self._check(self.lib.mgenx_set_fill_time(self.ctx, fill_time), "mgenx_set_fill_time")

    def pack(self, tmpl, tmpl_crc, desc, n, pool, slab, *, rec_off=None, stride=0, opts=0,
             fill_time=0, out_len=None):
        if out_len is None:
            out_len = self.torch.empty(n, dtype=self.torch.int32, device=slab.device)
        rc = self.lib.mgenx_pack_batch(self.ctx, _ptr(tmpl), _ptr(tmpl_crc), _ptr(desc), n,
                                       _ptr(pool), _ptr(slab), slab.numel(), _ptr(rec_off),
                                       stride, _ptr(out_len), opts, fill_time,
                                       _stream(self.device))
        self._check(rc, "mgenx_pack_batch")
        return out_len

    def pack_msgs(self, tmpl, tmpl_crc, desc, n, pool, slab, *, rec_off=None, stride=0,
                  buf_len=None, crc_in=None, opts=0, fill_time=0):
        """MgenMsg::Pack alone (mgenx_pack_msgs): returns (out_len, tx_crc, state) tensors."""
        torch = self.torch
        out_len = torch.empty(n, dtype=torch.int32, device=slab.device)
        tx_crc = torch.empty(n, dtype=torch.int32, device=slab.device)
        state = torch.empty(n, dtype=torch.int32, device=slab.device)
        rc = self.lib.mgenx_pack_msgs(self.ctx, _ptr(tmpl), _ptr(tmpl_crc), _ptr(desc), n,
                                      _ptr(pool), _ptr(slab), slab.numel(), _ptr(rec_off), stride,
                                      _ptr(buf_len), _ptr(crc_in), _ptr(out_len), _ptr(tx_crc),
                                      _ptr(state), opts, fill_time, _stream(self.device))
        self._check(rc, "mgenx_pack_msgs")
        return out_len, tx_crc, state

    def pack_tcp(self, tmpl, tmpl_crc, desc, msg_total, n, pool, *, opts=0, fill_time=0,
                 out=None, offs=None):
        """The MgenTcpTransport transmit stream of n messages (mgenx_pack_tcp): returns
        (stream uint8 tensor, message offsets int64 tensor).  out: a stream buffer to fill
        (else one is sized by a first call)."""
        torch = self.torch
        dev = msg_total.device
        if offs is None:
            offs = torch.empty(n, dtype=torch.int64, device=dev)
        total = ctypes.c_uint64(0)
        cap = None if out is None else out.numel()
        if cap is None:  # size query: a first call with no room reports the length
            rc = self.lib.mgenx_pack_tcp(self.ctx, _ptr(tmpl), _ptr(tmpl_crc), _ptr(desc),
                                         _ptr(msg_total), n, _ptr(pool), None, 0, _ptr(offs),
                                         ctypes.byref(total), opts, fill_time,
                                         _stream(self.device))
            if rc not in (0, -1):
                self._check(rc, "mgenx_pack_tcp")
            cap = int(total.value)
            out = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
        rc = self.lib.mgenx_pack_tcp(self.ctx, _ptr(tmpl), _ptr(tmpl_crc), _ptr(desc),
                                     _ptr(msg_total), n, _ptr(pool), _ptr(out), cap, _ptr(offs),
                                     ctypes.byref(total), opts, fill_time, _stream(self.device))
        self._check(rc, "mgenx_pack_tcp")
        return out[:int(total.value)], offs

    def crc32_update(self, data, off, length, n, state_in, out=None):
        """MgenMsg::ComputeCRC32 running states (mgenx_crc32_update)."""
        if out is None:
            out = self.torch.empty(n, dtype=self.torch.int32, device=data.device)
        rc = self.lib.mgenx_crc32_update(self.ctx, _ptr(data), _ptr(off), _ptr(length), n,
                                         _ptr(state_in), _ptr(out), _stream(self.device))
        self._check(rc, "mgenx_crc32_update")
        return out

    def set_pack_variant(self, v: int):
        self._check(self.lib.mgenx_set_tuning(self.ctx, 2, v), "mgenx_set_tuning")

    def set_unpack_variant(self, v: int):
        self._check(self.lib.mgenx_set_tuning(self.ctx, 1, v), "mgenx_set_tuning")

    def stream_read(self, data, grid=2048, scratch=None):
        if scratch is None:
            scratch = self.torch.empty(grid, dtype=self.torch.int32, device=data.device)
        rc = self.lib.mgenx_diag_stream_read(self.ctx, _ptr(data), data.numel(), _ptr(scratch),
                                             grid, _stream(self.device))
        self._check(rc, "mgenx_diag_stream_read")

    def stream_read_w(self, data, width, grid=2048, scratch=None):
        """Diagnostic: coalesced read at `width` (4, 8, 24) bytes per lane."""
        if scratch is None:
            scratch = self.torch.empty(grid, dtype=self.torch.int32, device=data.device)
        rc = self.lib.mgenx_diag_stream_read_w(self.ctx, _ptr(data), data.numel(), _ptr(scratch),
                                               grid, width, _stream(self.device))
        self._check(rc, "mgenx_diag_stream_read_w")

    def group_rw(self, data, out, mode=1):
        """Diagnostic: the fixed unpack's read pattern (+ 512-B stores per 16-KiB group)."""
        rc = self.lib.mgenx_diag_group_rw(self.ctx, _ptr(data), data.numel(), _ptr(out), mode,
                                          _stream(self.device))
        self._check(rc, "mgenx_diag_group_rw")

    def stream_scan(self, data, mode=SCAN_TCP, cap=None, nbytes=None, out=None):
        """TCP / SINK record framing of a device byte stream (mgenx_stream_scan).  Returns
        (rec_off int64 tensor, rec_len int32 tensor, ScanInfo); synchronous.  out: optional
        preallocated (rec_off int64, rec_len int32) tensors of equal length (the capacity)."""
        torch = self.torch
        nbytes = data.numel() if nbytes is None else nbytes
        if out is not None:
            offs, lens = out
            if offs.dtype != torch.int64 or lens.dtype != torch.int32 or \
                    offs.numel() != lens.numel():
                raise ValueError("stream_scan out: (int64, int32) tensors of one length")
            cap = offs.numel()
        else:
            if cap is None:
                cap = nbytes // 4 + 1
            offs = torch.empty(cap, dtype=torch.int64, device=data.device)
            lens = torch.empty(cap, dtype=torch.int32, device=data.device)
        info = ScanInfo()
        rc = self.lib.mgenx_stream_scan(self.ctx, _ptr(data), nbytes, mode, _ptr(offs),
                                        _ptr(lens), cap, ctypes.byref(info),
                                        _stream(self.device))
        self._check(rc, "mgenx_stream_scan")
        n = min(int(info.n_records), cap)
        return offs[:n], lens[:n], info

    def stream_scan_exits(self, data, mode, window, limit, cap=4096, nbytes=None):
        """Step 1 of the sharded framing (mgenx_stream_scan_exits): builds the candidate
        tables of `data` and returns (entries, exits) uint64 device tensors of `cap` rows
        (as int64) plus the candidate count."""
        torch = self.torch
        nbytes = data.numel() if nbytes is None else nbytes
        ent = torch.empty(cap, dtype=torch.int64, device=data.device)
        ext = torch.empty(cap, dtype=torch.int64, device=data.device)
        cands = ctypes.c_uint32(0)
        rc = self.lib.mgenx_stream_scan_exits(self.ctx, _ptr(data), nbytes, mode, window, limit,
                                              _ptr(ent), _ptr(ext), cap, ctypes.byref(cands),
                                              _stream(self.device))
        self._check(rc, "mgenx_stream_scan_exits")
        return ent, ext, int(cands.value)

    def stream_scan_range(self, data, mode, entry, limit, reuse=False, cap=None, nbytes=None):
        """Records of the chain from `entry` below `limit` (mgenx_stream_scan_range); reuse:
        the tables of the last build on this engine (same tensor, unchanged)."""
        torch = self.torch
        nbytes = data.numel() if nbytes is None else nbytes
        if cap is None:
            cap = max(limit - entry, 0) // 4 + 1
        offs = torch.empty(max(cap, 1), dtype=torch.int64, device=data.device)
        lens = torch.empty(max(cap, 1), dtype=torch.int32, device=data.device)
        info = ScanInfo()
        rc = self.lib.mgenx_stream_scan_range(self.ctx, _ptr(data), nbytes, mode, entry, limit,
                                              1 if reuse else 0, _ptr(offs), _ptr(lens), cap,
                                              ctypes.byref(info), _stream(self.device))
        self._check(rc, "mgenx_stream_scan_range")
        n = min(int(info.n_records), cap)
        return offs[:n], lens[:n], info

    # ------------------------------------------------------------ analytics
    def flow_init(self, n_flows, window=1.0):
        """Fresh MgenAnalytic state for n_flows flows (mgenx_flow_init); a uint8 tensor of
        n_flows x 256 B."""
        flows = self.torch.empty(n_flows * FLOW_STATE_BYTES, dtype=self.torch.uint8,
                                 device=f"cuda:{self.device}")
        self._check(self.lib.mgenx_flow_init(self.ctx, _ptr(flows), n_flows, window,
                                             _stream(self.device)), "mgenx_flow_init")
        return flows

    def flow_reduce(self, flows, n_flows, flow_idx, seq, tx_sec, tx_usec, msg_len, rx_sec,
                    rx_usec, n=None, reports=None, per_flow=0, report_count=None,
                    report_rec=None):
        """MgenAnalytic::Update over records in receive order (mgenx_flow_reduce; with
        report_rec, mgenx_flow_reduce_ex: the record that closed each kept report).  Returns
        report_count (None when per_flow is 0 and none was passed: nothing to count into)."""
        torch = self.torch
        n = flow_idx.numel() if n is None else n
        if report_count is None and per_flow:
            report_count = torch.zeros(n_flows, dtype=torch.int32, device=flows.device)
        if report_rec is None:
            rc = self.lib.mgenx_flow_reduce(self.ctx, _ptr(flow_idx), _ptr(seq), _ptr(tx_sec),
                                            _ptr(tx_usec), _ptr(msg_len), _ptr(rx_sec),
                                            _ptr(rx_usec), n, _ptr(flows), n_flows, _ptr(reports),
                                            per_flow, _ptr(report_count), _stream(self.device))
        else:
            rc = self.lib.mgenx_flow_reduce_ex(self.ctx, _ptr(flow_idx), _ptr(seq), _ptr(tx_sec),
                                               _ptr(tx_usec), _ptr(msg_len), _ptr(rx_sec),
                                               _ptr(rx_usec), n, _ptr(flows), n_flows,
                                               _ptr(reports), per_flow, _ptr(report_count),
                                               _ptr(report_rec), _stream(self.device))
        self._check(rc, "mgenx_flow_reduce")
        return report_count

    def flow_reduce_rows(self, flows, n_flows, flow_idx, rows, rx_sec, rx_usec, n=None,
                         reports=None, per_flow=0, report_count=None, report_rec=None):
        """flow_reduce with seq / tx time / msg_len read from the unpack's 32-B rows
        (mgenx_flow_reduce_rows): the same result as the column form."""
        torch = self.torch
        n = flow_idx.numel() if n is None else n
        if report_count is None and per_flow:
            report_count = torch.zeros(n_flows, dtype=torch.int32, device=flows.device)
        rc = self.lib.mgenx_flow_reduce_rows(self.ctx, _ptr(flow_idx), _ptr(rows), _ptr(rx_sec),
                                             _ptr(rx_usec), n, _ptr(flows), n_flows,
                                             _ptr(reports), per_flow, _ptr(report_count),
                                             _ptr(report_rec), _stream(self.device))
        self._check(rc, "mgenx_flow_reduce_rows")
        return report_count

    def flow_dist_init(self, n_flows, hist=True):
        """Fresh per-flow delivery statistics (mgenx_flow_dist_init): (dist, hist), a uint8
        tensor of n_flows x 160 B (FLOW_DIST_DTYPE) and an int64 tensor of n_flows x
        FLOW_DIST_BINS counts (None with hist=False)."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        dist = torch.empty(n_flows * FLOW_DIST_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        h = torch.empty((n_flows, FLOW_DIST_BINS), dtype=torch.int64, device=dev) if hist else None
        self._check(self.lib.mgenx_flow_dist_init(self.ctx, _ptr(dist), _ptr(h), n_flows,
                                                  _stream(self.device)), "mgenx_flow_dist_init")
        return dist, h

    def flow_dist(self, dist, hist, n_flows, flow_idx, seq, tx_sec, tx_usec, msg_len, rx_sec,
                  rx_usec, n=None):
        """Latency / jitter / gap / reordering statistics over records in receive order
        (mgenx_flow_dist), added to dist and (unless None) hist; batches may follow each
        other."""
        n = flow_idx.numel() if n is None else n
        self._check(self.lib.mgenx_flow_dist(self.ctx, _ptr(flow_idx), _ptr(seq), _ptr(tx_sec),
                                             _ptr(tx_usec), _ptr(msg_len), _ptr(rx_sec),
                                             _ptr(rx_usec), n, _ptr(dist), _ptr(hist), n_flows,
                                             _stream(self.device)), "mgenx_flow_dist")

    def flow_dist_quantiles(self, dist, hist, n_flows, permille, out=None):
        """Latency quantiles from the histogram (mgenx_flow_dist_quantiles): an int64 tensor
        [n_flows, len(permille)] of bin upper edges in microseconds (-1 among the negative
        latencies, 2**32 among those past the histogram, INT64_MIN for an empty flow)."""
        torch = self.torch
        q = (ctypes.c_uint32 * len(permille))(*[int(v) for v in permille])
        if out is None:
            out = torch.empty((n_flows, len(permille)), dtype=torch.int64,
                              device=f"cuda:{self.device}")
        self._check(self.lib.mgenx_flow_dist_quantiles(self.ctx, _ptr(dist), _ptr(hist), n_flows,
                                                       q, len(permille), _ptr(out),
                                                       _stream(self.device)),
                    "mgenx_flow_dist_quantiles")
        return out

    def flow_series_init(self, n_flows, n_bins):
        """Fresh per-flow time series (mgenx_flow_series_init): (state, bins), uint8 tensors of
        n_flows x 32 B (FLOW_SERIES_STATE_DTYPE) and n_flows x n_bins x 64 B
        (FLOW_SERIES_BIN_DTYPE, row f = flow f)."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        state = torch.empty(n_flows * FLOW_SERIES_STATE_DTYPE.itemsize, dtype=torch.uint8,
                            device=dev)
        bins = torch.empty(n_flows * n_bins * FLOW_SERIES_BIN_DTYPE.itemsize, dtype=torch.uint8,
                           device=dev)
        self._check(self.lib.mgenx_flow_series_init(self.ctx, _ptr(state), _ptr(bins), n_flows,
                                                    n_bins, _stream(self.device)),
                    "mgenx_flow_series_init")
        return state, bins

    def flow_series(self, state, bins, n_flows, n_bins, t0_us, width_us, flow_idx, seq, tx_sec,
                    tx_usec, msg_len, rx_sec, rx_usec, n=None):
        """Records in receive order added to the bins floor((rx - t0_us) / width_us) of their
        flows (mgenx_flow_series); batches may follow each other with the same t0_us, width_us
        and n_bins."""
        n = flow_idx.numel() if n is None else n
        self._check(self.lib.mgenx_flow_series(self.ctx, _ptr(flow_idx), _ptr(seq), _ptr(tx_sec),
                                               _ptr(tx_usec), _ptr(msg_len), _ptr(rx_sec),
                                               _ptr(rx_usec), n, int(t0_us), int(width_us),
                                               int(n_bins), _ptr(state), _ptr(bins), n_flows,
                                               _stream(self.device)), "mgenx_flow_series")

    def flow_series_quantiles(self, n_flows, n_bins, t0_us, width_us, permille, flow_idx, tx_sec,
                              tx_usec, rx_sec, rx_usec, n=None, out=None):
        """Exact latency percentiles per flow and window (mgenx_flow_series_quantiles): an int64
        tensor [n_flows, n_bins, len(permille)], the r-th smallest latency of each cell with
        mgenx_flow_dist_quantiles' rank rule, INT64_MIN for an empty cell.  One call takes the
        whole log; `out` may pass a tensor of that many elements to write into."""
        torch = self.torch
        n = flow_idx.numel() if n is None else n
        q = (ctypes.c_uint32 * len(permille))(*[int(v) for v in permille])
        if out is None:
            out = torch.empty((n_flows, n_bins, len(permille)), dtype=torch.int64,
                              device=f"cuda:{self.device}")
        self._check(self.lib.mgenx_flow_series_quantiles(
            self.ctx, _ptr(flow_idx), _ptr(tx_sec), _ptr(tx_usec), _ptr(rx_sec), _ptr(rx_usec),
            n, int(t0_us), int(width_us), int(n_bins), n_flows, q, len(permille), _ptr(out),
            _stream(self.device)), "mgenx_flow_series_quantiles")
        return out

    def flow_clock(self, n_flows, flow_idx, tx_sec, tx_usec, rx_sec, rx_usec, n=None, *,
                   offset_only=False, resid=False, stamps=False, opts=None):
        """Per-flow clock offset and skew (mgenx_flow_clock): the hull edge over the mean send
        time of every flow and the latencies above it.  Returns (clock, resid, rx_sec_out,
        rx_usec_out): a uint8 tensor of n_flows x 64 B (FLOW_CLOCK_DTYPE), an int64 tensor of n
        residuals (None unless resid=True) and two int32 tensors of n corrected receive stamps
        (None unless stamps=True), which mgenx_flow_dist / flow_series / flow_series_quantiles take
        in place of rx_sec / rx_usec.  resid and stamps may also pass tensors to write into
        (stamps: a pair).  One call takes the whole log."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        n = flow_idx.numel() if n is None else n
        if opts is None:
            opts = CLOCK_OFFSET_ONLY if offset_only else 0
        clock = torch.empty(max(n_flows, 1) * FLOW_CLOCK_DTYPE.itemsize, dtype=torch.uint8,
                            device=dev)
        if resid is True:
            resid = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        elif resid is False:
            resid = None
        if stamps is True:
            stamps = (torch.empty(max(n, 1), dtype=torch.int32, device=dev),
                      torch.empty(max(n, 1), dtype=torch.int32, device=dev))
        elif stamps is False or stamps is None:
            stamps = (None, None)
        self._check(self.lib.mgenx_flow_clock(
            self.ctx, _ptr(flow_idx), _ptr(tx_sec), _ptr(tx_usec), _ptr(rx_sec), _ptr(rx_usec), n,
            n_flows, opts, _ptr(clock), _ptr(resid), _ptr(stamps[0]), _ptr(stamps[1]),
            _stream(self.device)), "mgenx_flow_clock")
        return clock[:n_flows * FLOW_CLOCK_DTYPE.itemsize], resid, stamps[0], stamps[1]

    def match_side(self, parsed, n, want_event):
        """A parsed log (log_parse_text) made ready for flow_lookup as one side of msg_match
        (mgenx_match_side): returns (cols, src) where cols is `parsed` with err = 0 exactly for
        the OK lines of want_event (EVENT_SEND / EVENT_RECV) and src holds the lines' source
        ports with the addresses cleared, so a SEND line and the RECV line of its flow share
        one key."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        err = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        src = torch.empty(max(n, 1) * ADDR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._check(self.lib.mgenx_match_side(self.ctx, _ptr(parsed["event"]),
                                              _ptr(parsed["status"]), _ptr(parsed["src"]), n,
                                              want_event, _ptr(src), _ptr(err),
                                              _stream(self.device)), "mgenx_match_side")
        cols = dict(parsed)
        cols["err"] = err
        return cols, src

    def msg_match(self, n_flows, send, recv, *, opts=0, ns=None, nr=None):
        """Join a sender's records with a receiver's (mgenx_msg_match).  send: dict of int32
        tensors flow_idx, seq, t_sec, t_usec, len; recv: flow_idx, seq, tx_sec, tx_usec, rx_sec,
        rx_usec (flow indices from one numbering).  Returns (send_rx_count, send_first_rx,
        recv_send, flows, stats): int32 tensors of ns, ns and nr elements and uint8 tensors of
        n_flows x 256 B (FLOW_MATCH_DTYPE) and 32 B (MATCH_STATS_DTYPE)."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        ns = send["flow_idx"].numel() if ns is None else ns
        nr = recv["flow_idx"].numel() if nr is None else nr
        cnt = torch.empty(max(ns, 1), dtype=torch.int32, device=dev)
        first = torch.empty(max(ns, 1), dtype=torch.int32, device=dev)
        rs = torch.empty(max(nr, 1), dtype=torch.int32, device=dev)
        flows = torch.empty(max(n_flows, 1) * FLOW_MATCH_DTYPE.itemsize, dtype=torch.uint8,
                            device=dev)
        stats = torch.empty(MATCH_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._check(self.lib.mgenx_msg_match(
            self.ctx, _ptr(send["flow_idx"]), _ptr(send["seq"]), _ptr(send["t_sec"]),
            _ptr(send["t_usec"]), _ptr(send["len"]), ns, _ptr(recv["flow_idx"]),
            _ptr(recv["seq"]), _ptr(recv["tx_sec"]), _ptr(recv["tx_usec"]), _ptr(recv["rx_sec"]),
            _ptr(recv["rx_usec"]), nr, n_flows, opts, _ptr(cnt), _ptr(first), _ptr(rs),
            _ptr(flows), _ptr(stats), _stream(self.device)), "mgenx_msg_match")
        return (cnt[:ns], first[:ns], rs[:nr], flows[:n_flows * FLOW_MATCH_DTYPE.itemsize],
                stats)

    def msg_match_multi(self, n_flows, n_rcv, send, recv, *, opts=0, timeline=None, ns=None,
                        nr=None):
        """Join a sender's records with the records of n_rcv receivers (mgenx_msg_match_multi).
        send: msg_match's dict; recv: msg_match's dict plus rcv (int32, the receiver's index of
        every record), the receivers' records one after the other.  timeline: None or
        (t0_us, width_us, n_bins), the windows of send time.  Returns (send_mask, recv_send,
        recv_first, cells, fanout, stats): int64 [ns], int32 [nr], uint8 [nr], and uint8 tensors
        of n_flows x n_rcv x 80 B (RCV_CELL_DTYPE), n_flows x 560 B (FLOW_FANOUT_DTYPE) and 32 B
        (MATCH_STATS_DTYPE); with a timeline also bins (uint8, n_flows x n_bins x 64 B:
        MULTI_BIN_DTYPE) and outside (int64, n_flows)."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        ns = send["flow_idx"].numel() if ns is None else ns
        nr = recv["flow_idx"].numel() if nr is None else nr
        mask = torch.empty(max(ns, 1), dtype=torch.int64, device=dev)
        rs = torch.empty(max(nr, 1), dtype=torch.int32, device=dev)
        first = torch.empty(max(nr, 1), dtype=torch.uint8, device=dev)
        n_cells = n_flows * n_rcv
        cells = torch.empty(max(n_cells, 1) * RCV_CELL_DTYPE.itemsize, dtype=torch.uint8,
                            device=dev)
        fanout = torch.empty(max(n_flows, 1) * FLOW_FANOUT_DTYPE.itemsize, dtype=torch.uint8,
                             device=dev)
        stats = torch.empty(MATCH_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        tl, n_bins = None, 0
        if timeline is not None:
            t0_us, width_us, n_bins = (int(v) for v in timeline)
            bins = torch.empty(max(n_flows * n_bins, 1) * MULTI_BIN_DTYPE.itemsize,
                               dtype=torch.uint8, device=dev)
            outside = torch.zeros(max(n_flows, 1), dtype=torch.int64, device=dev)
            tl = ctypes.byref(MultiTimeline(t0_us=t0_us, width_us=width_us, n_bins=n_bins,
                                            dev_bins=bins.data_ptr(),
                                            dev_outside=outside.data_ptr()))
        self._check(self.lib.mgenx_msg_match_multi(
            self.ctx, _ptr(send["flow_idx"]), _ptr(send["seq"]), _ptr(send["t_sec"]),
            _ptr(send["t_usec"]), _ptr(send["len"]), ns, _ptr(recv["flow_idx"]),
            _ptr(recv["seq"]), _ptr(recv["tx_sec"]), _ptr(recv["tx_usec"]), _ptr(recv["rx_sec"]),
            _ptr(recv["rx_usec"]), _ptr(recv["rcv"]), nr, n_rcv, n_flows, opts, _ptr(mask),
            _ptr(rs), _ptr(first), _ptr(cells), _ptr(fanout), _ptr(stats), tl,
            _stream(self.device)), "mgenx_msg_match_multi")
        res = (mask[:ns], rs[:nr], first[:nr], cells[:n_cells * RCV_CELL_DTYPE.itemsize],
               fanout[:n_flows * FLOW_FANOUT_DTYPE.itemsize], stats)
        if timeline is not None:
            res += (bins[:n_flows * n_bins * MULTI_BIN_DTYPE.itemsize], outside[:n_flows])
        return res

    def msg_match_multi_loss(self, n_flows, n_rcv, send, recv, *, run_stats=True, min_run=1,
                             pairs=True, opts=0, timeline=None, ns=None, nr=None):
        """msg_match_multi plus the parts of mgenx_msg_match_multi_ex.  Returns msg_match_multi's
        tuple (six tensors, eight with a timeline) followed by (rcv_runs, runs, pairs): uint8 tensors of n_flows x n_rcv x 160 B
        (RCV_RUNS_DTYPE; None unless run_stats), n_runs x 40 B (RCV_LOSS_RUN_DTYPE: the runs of
        at least min_run lost messages by flow, last send index and receiver; None when min_run
        is None) and n_flows x n_rcv x n_rcv x 32 B (RCV_PAIR_DTYPE; None unless pairs).  The run
        list is sized by a first call and the call is repeated once (one read-back)."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        ns = send["flow_idx"].numel() if ns is None else ns
        nr = recv["flow_idx"].numel() if nr is None else nr
        mask = torch.empty(max(ns, 1), dtype=torch.int64, device=dev)
        rs = torch.empty(max(nr, 1), dtype=torch.int32, device=dev)
        first = torch.empty(max(nr, 1), dtype=torch.uint8, device=dev)
        n_cells = n_flows * n_rcv
        cells = torch.empty(max(n_cells, 1) * RCV_CELL_DTYPE.itemsize, dtype=torch.uint8,
                            device=dev)
        fanout = torch.empty(max(n_flows, 1) * FLOW_FANOUT_DTYPE.itemsize, dtype=torch.uint8,
                             device=dev)
        stats = torch.empty(MATCH_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        tl, n_bins = None, 0
        if timeline is not None:
            t0_us, width_us, n_bins = (int(v) for v in timeline)
            bins = torch.empty(max(n_flows * n_bins, 1) * MULTI_BIN_DTYPE.itemsize,
                               dtype=torch.uint8, device=dev)
            outside = torch.zeros(max(n_flows, 1), dtype=torch.int64, device=dev)
            tl = ctypes.byref(MultiTimeline(t0_us=t0_us, width_us=width_us, n_bins=n_bins,
                                            dev_bins=bins.data_ptr(),
                                            dev_outside=outside.data_ptr()))
        lx = MultiLoss(min_run=0 if min_run is None else int(min_run), run_cap=0)
        rcv_runs = runs = pair = n_runs = None
        if run_stats:
            rcv_runs = torch.empty(max(n_cells, 1) * RCV_RUNS_DTYPE.itemsize, dtype=torch.uint8,
                                   device=dev)
            lx.dev_rcv_runs = rcv_runs.data_ptr()
        if pairs:
            pair = torch.empty(max(n_cells * n_rcv, 1) * RCV_PAIR_DTYPE.itemsize,
                               dtype=torch.uint8, device=dev)
            lx.dev_pairs = pair.data_ptr()
        if min_run is not None:
            n_runs = torch.zeros(1, dtype=torch.int64, device=dev)
            runs = torch.empty(0, dtype=torch.uint8, device=dev)
            lx.dev_n_runs = n_runs.data_ptr()
        for again in (False, True):
            self._check(self.lib.mgenx_msg_match_multi_ex(
                self.ctx, _ptr(send["flow_idx"]), _ptr(send["seq"]), _ptr(send["t_sec"]),
                _ptr(send["t_usec"]), _ptr(send["len"]), ns, _ptr(recv["flow_idx"]),
                _ptr(recv["seq"]), _ptr(recv["tx_sec"]), _ptr(recv["tx_usec"]),
                _ptr(recv["rx_sec"]), _ptr(recv["rx_usec"]), _ptr(recv["rcv"]), nr, n_rcv,
                n_flows, opts, _ptr(mask), _ptr(rs), _ptr(first), _ptr(cells), _ptr(fanout),
                _ptr(stats), tl, ctypes.byref(lx), _stream(self.device)),
                "mgenx_msg_match_multi_ex")
            if again or n_runs is None:
                break
            count = int(n_runs.item())
            if count == 0:
                break
            runs = torch.empty(count * RCV_LOSS_RUN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            lx.dev_runs, lx.run_cap = runs.data_ptr(), count
        res = (mask[:ns], rs[:nr], first[:nr], cells[:n_cells * RCV_CELL_DTYPE.itemsize],
               fanout[:n_flows * FLOW_FANOUT_DTYPE.itemsize], stats)
        if timeline is not None:
            res += (bins[:n_flows * n_bins * MULTI_BIN_DTYPE.itemsize], outside[:n_flows])
        return res + (
                None if rcv_runs is None else rcv_runs[:n_cells * RCV_RUNS_DTYPE.itemsize],
                runs,
                None if pair is None else pair[:n_cells * n_rcv * RCV_PAIR_DTYPE.itemsize])

    def msg_match_timeline(self, n_flows, send, recv, t0_us, width_us, n_bins, *, min_run=1,
                           opts=0, ns=None, nr=None):
        """msg_match plus the timeline of mgenx_msg_match_ex on the sender's time axis.  Returns
        msg_match's tuple followed by bins (uint8, n_flows x n_bins x 64 B: MATCH_BIN_DTYPE),
        outside (int64, n_flows), runs (uint8, n_runs x 40 B: LOSS_RUN_DTYPE, the runs of at
        least min_run lost messages by flow and first send index) and owner (int32, ns).  The
        run list is sized by a first call and the call is repeated once (one read-back)."""
        torch = self.torch
        dev = f"cuda:{self.device}"
        ns = send["flow_idx"].numel() if ns is None else ns
        nr = recv["flow_idx"].numel() if nr is None else nr
        cnt = torch.empty(max(ns, 1), dtype=torch.int32, device=dev)
        first = torch.empty(max(ns, 1), dtype=torch.int32, device=dev)
        owner = torch.empty(max(ns, 1), dtype=torch.int32, device=dev)
        rs = torch.empty(max(nr, 1), dtype=torch.int32, device=dev)
        flows = torch.empty(max(n_flows, 1) * FLOW_MATCH_DTYPE.itemsize, dtype=torch.uint8,
                            device=dev)
        stats = torch.empty(MATCH_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        cells = n_flows * n_bins
        bins = torch.empty(max(cells, 1) * MATCH_BIN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        outside = torch.zeros(max(n_flows, 1), dtype=torch.int64, device=dev)
        n_runs = torch.zeros(1, dtype=torch.int64, device=dev)
        runs = torch.empty(0, dtype=torch.uint8, device=dev)
        tl = MatchTimeline(t0_us=t0_us, width_us=width_us, n_bins=n_bins, min_run=min_run,
                           dev_bins=bins.data_ptr(), dev_outside=outside.data_ptr(),
                           dev_runs=None, run_cap=0, dev_n_runs=n_runs.data_ptr(),
                           dev_send_owner=owner.data_ptr())
        count = 0
        for again in (False, True):
            self._check(self.lib.mgenx_msg_match_ex(
                self.ctx, _ptr(send["flow_idx"]), _ptr(send["seq"]), _ptr(send["t_sec"]),
                _ptr(send["t_usec"]), _ptr(send["len"]), ns, _ptr(recv["flow_idx"]),
                _ptr(recv["seq"]), _ptr(recv["tx_sec"]), _ptr(recv["tx_usec"]),
                _ptr(recv["rx_sec"]), _ptr(recv["rx_usec"]), nr, n_flows, opts, _ptr(cnt),
                _ptr(first), _ptr(rs), _ptr(flows), _ptr(stats), ctypes.byref(tl),
                _stream(self.device)), "mgenx_msg_match_ex")
            if again:
                break
            count = int(n_runs.item())
            if count == 0:
                break
            runs = torch.empty(count * LOSS_RUN_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            tl.dev_runs, tl.run_cap = runs.data_ptr(), count
        return (cnt[:ns], first[:ns], rs[:nr], flows[:n_flows * FLOW_MATCH_DTYPE.itemsize],
                stats, bins[:cells * MATCH_BIN_DTYPE.itemsize], outside[:n_flows], runs,
                owner[:ns])

    def flow_keys(self, table, n_flows, protocol=1, keys=None):
        """The report_msg key of every flow index < n_flows (mgenx_flow_keys): a uint8
        tensor of n_flows x 48 (mgenx_report_key)."""
        if keys is None:
            keys = self.torch.zeros(max(n_flows, 1) * REPORT_KEY_DTYPE.itemsize,
                                    dtype=self.torch.uint8, device=f"cuda:{self.device}")
        self._check(self.lib.mgenx_flow_keys(self.ctx, table, protocol, _ptr(keys), n_flows,
                                             _stream(self.device)), "mgenx_flow_keys")
        return keys

    def flow_span(self, flow_idx, rx_sec, rx_usec, n, n_flows):
        """(most records of any flow index < n_flows, lowest, highest receive time in us) over
        those records (mgenx_flow_span; (0, 2**64 - 1, 0) when there are none): one read-back."""
        torch = self.torch
        dev = flow_idx.device
        counts = torch.empty(max(n_flows, 1), dtype=torch.int32, device=dev)
        out = torch.empty(3, dtype=torch.int64, device=dev)
        self._check(self.lib.mgenx_flow_span(self.ctx, _ptr(flow_idx), _ptr(rx_sec), _ptr(rx_usec),
                                             n, n_flows, _ptr(counts), _ptr(out),
                                             _stream(self.device)), "mgenx_flow_span")
        most, lo, hi = (int(v) & 0xFFFFFFFFFFFFFFFF for v in out.cpu().tolist())
        return most, lo, hi

    def text_interleave(self, sources, n_rec, cap=None):
        """mgenx_text_interleave: sources = [(kind, text, line_off, n_lines, index,
        index_stride)] (device tensors); returns (text, record offsets of n_rec + 1)."""
        torch = self.torch
        arr = (TextSrc * max(1, len(sources)))()
        keep = []
        for k, (kind, text, line_off, n_lines, index, stride) in enumerate(sources):
            arr[k].text = text.data_ptr() if text is not None and text.numel() else None
            arr[k].line_off = line_off.data_ptr()
            arr[k].n_lines = n_lines
            arr[k].kind = kind
            arr[k].index = index.data_ptr() if index is not None else None
            arr[k].index_stride = stride
            keep.append((text, line_off, index))
        dev = f"cuda:{self.device}"
        if cap is None:
            cap = sum(int(t.numel()) for _, t, *_ in sources if t is not None)
        rec_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
        for _ in range(2):
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            self._check(self.lib.mgenx_text_interleave(self.ctx, arr, len(sources), n_rec,
                                                       _ptr(out), cap, _ptr(rec_off),
                                                       _stream(self.device)),
                        "mgenx_text_interleave")
            total = int(rec_off[n_rec].item())
            if total <= cap:
                return out[:total], rec_off
            cap = total
        raise MgenxError("mgenx_text_interleave: output did not fit")

    # ------------------------------------------------------------ ConvertBinaryLog
    def convert_binary_log(self, buf, rec_off, n, flags=0, opts=0, cap=None):
        """MgenMsg::ConvertBinaryLog over records indexed by binlog_index (device tensors):
        returns (text uint8 tensor, per-record offsets of n + 1).  Synchronous."""
        torch = self.torch
        dev = buf.device
        pos = torch.empty(n + 1, dtype=torch.int64, device=dev)
        cap = cap if cap is not None else max(1, n) * 200
        for _ in range(2):
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            self._check(self.lib.mgenx_convert_binary_log(self.ctx, _ptr(buf), buf.numel(),
                                                          _ptr(rec_off), n, flags, opts,
                                                          _ptr(out), cap, _ptr(pos),
                                                          _stream(self.device)),
                        "mgenx_convert_binary_log")
            total = int(pos[n].item())
            if total <= cap:
                return out[:total], pos
            cap = total
        raise MgenxError("mgenx_convert_binary_log: text did not fit")

    # ------------------------------------------------------------ pcap2mgen
    def pcap_parse(self, buf, pkt_off, n, link_type, flags=0):
        """pcap2mgen's frame walk per record (mgenx_pcap_parse): returns a dict of device
        tensors udp_off, udp_len, src (n x 20), ttl, rx_sec, rx_usec, status."""
        torch = self.torch
        dev = buf.device
        o = {"udp_off": torch.empty(max(n, 1), dtype=torch.int64, device=dev),
             "udp_len": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
             "src": torch.empty(max(n, 1) * 20, dtype=torch.uint8, device=dev),
             "ttl": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
             "rx_sec": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
             "rx_usec": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
             "status": torch.empty(max(n, 1), dtype=torch.uint8, device=dev)}
        self._check(self.lib.mgenx_pcap_parse(self.ctx, _ptr(buf), buf.numel(), _ptr(pkt_off), n,
                                              link_type, flags, _ptr(o["udp_off"]),
                                              _ptr(o["udp_len"]), _ptr(o["src"]), _ptr(o["ttl"]),
                                              _ptr(o["rx_sec"]), _ptr(o["rx_usec"]),
                                              _ptr(o["status"]), _stream(self.device)),
                    "mgenx_pcap_parse")
        return o

    def pcap_snap(self, buf, file_bytes, pkt_off, n, flags, parsed, buf_bytes=None):
        """mgenx_pcap_snap: move the SNAPPED packets of `parsed` (pcap_parse's dict) into
        buf[file_bytes:buf_bytes] (default: to the end of buf), zero-extended, in place."""
        self._check(self.lib.mgenx_pcap_snap(self.ctx, _ptr(buf), file_bytes,
                                             buf.numel() if buf_bytes is None else buf_bytes,
                                             _ptr(pkt_off), n, flags, _ptr(parsed["status"]),
                                             _ptr(parsed["udp_off"]), _ptr(parsed["udp_len"]),
                                             _stream(self.device)), "mgenx_pcap_snap")
        return parsed

    def pcapng_parse(self, buf, pkt_off, pkt_if, n, ifaces, n_ifaces, link_type, flags=0):
        """mgenx_pcapng_parse over pcapng packet blocks (pkt_off, pkt_if and the interface
        table as mgenx_pcapng_index gives them, on the device): pcap_parse's dict plus
        data_off and cap_len (each packet's data, for pcapng_snap)."""
        torch = self.torch
        dev = buf.device
        m = max(n, 1)
        o = {"udp_off": torch.empty(m, dtype=torch.int64, device=dev),
             "udp_len": torch.empty(m, dtype=torch.int32, device=dev),
             "src": torch.empty(m * 20, dtype=torch.uint8, device=dev),
             "ttl": torch.empty(m, dtype=torch.int32, device=dev),
             "rx_sec": torch.empty(m, dtype=torch.int32, device=dev),
             "rx_usec": torch.empty(m, dtype=torch.int32, device=dev),
             "status": torch.empty(m, dtype=torch.uint8, device=dev),
             "data_off": torch.empty(m, dtype=torch.int64, device=dev),
             "cap_len": torch.empty(m, dtype=torch.int32, device=dev)}
        self._check(self.lib.mgenx_pcapng_parse(
            self.ctx, _ptr(buf), buf.numel(), _ptr(pkt_off), _ptr(pkt_if), n, _ptr(ifaces),
            n_ifaces, link_type, flags, _ptr(o["udp_off"]), _ptr(o["udp_len"]), _ptr(o["src"]),
            _ptr(o["ttl"]), _ptr(o["rx_sec"]), _ptr(o["rx_usec"]), _ptr(o["status"]),
            _ptr(o["data_off"]), _ptr(o["cap_len"]), _stream(self.device)), "mgenx_pcapng_parse")
        return o

    def pcapng_snap(self, buf, file_bytes, n, parsed, buf_bytes=None):
        """mgenx_pcapng_snap: move the SNAPPED packets of `parsed` (pcapng_parse's dict) into
        buf[file_bytes:buf_bytes] (default: to the end of buf), zero-extended, in place."""
        self._check(self.lib.mgenx_pcapng_snap(self.ctx, _ptr(buf), file_bytes,
                                               buf.numel() if buf_bytes is None else buf_bytes,
                                               _ptr(parsed["data_off"]), _ptr(parsed["cap_len"]),
                                               n, _ptr(parsed["status"]), _ptr(parsed["udp_off"]),
                                               _ptr(parsed["udp_len"]), _stream(self.device)),
                    "mgenx_pcapng_snap")
        return parsed

    def pcap_defrag(self, buf, scratch_off, pkt_off, n, link_type, flags, parsed,
                    timeout_us=30_000_000):
        """mgenx_pcap_defrag: reassemble the fragmented datagrams of `parsed` (pcap_parse's
        dict, after pcap_snap) into buf[scratch_off:], in place.  Returns (fits, DefragStats):
        fits False = the window is smaller than stats.scratch_bytes and nothing was changed
        (an empty window sizes the scratch).  Synchronous."""
        st = DefragStats()
        rc = self.lib.mgenx_pcap_defrag(
            self.ctx, _ptr(buf), scratch_off, buf.numel(), _ptr(pkt_off), n, link_type, flags,
            int(timeout_us), _ptr(parsed["rx_sec"]), _ptr(parsed["rx_usec"]),
            _ptr(parsed["status"]), _ptr(parsed["udp_off"]), _ptr(parsed["udp_len"]),
            _ptr(parsed["src"]), ctypes.byref(st), _stream(self.device))
        if rc != ENOSPC:
            self._check(rc, "mgenx_pcap_defrag")
        return rc == 0, st

    def pcapng_defrag(self, buf, scratch_off, pkt_off, n, link_type, flags, parsed,
                      timeout_us=30_000_000):
        """mgenx_pcapng_defrag: pcap_defrag for pcapng packets (pkt_off: the packet blocks,
        `parsed`: pcapng_parse's dict with data_off and cap_len)."""
        st = DefragStats()
        rc = self.lib.mgenx_pcapng_defrag(
            self.ctx, _ptr(buf), scratch_off, buf.numel(), _ptr(pkt_off),
            _ptr(parsed["data_off"]), _ptr(parsed["cap_len"]), n, link_type, flags,
            int(timeout_us), _ptr(parsed["rx_sec"]), _ptr(parsed["rx_usec"]),
            _ptr(parsed["status"]), _ptr(parsed["udp_off"]), _ptr(parsed["udp_len"]),
            _ptr(parsed["src"]), ctypes.byref(st), _stream(self.device))
        if rc != ENOSPC:
            self._check(rc, "mgenx_pcapng_defrag")
        return rc == 0, st

    def pcap_tcp(self, buf, scratch_off, pkt_off, n, link_type, flags, parsed, stream_cap=None,
                 out=None):
        """mgenx_pcap_tcp (mgenx_pcapng_tcp when `parsed` is pcapng_parse's dict): rebuild the
        TCP streams among the packets of `parsed` into buf[scratch_off:], in place.  Returns
        (fits, TcpStats, streams, piece_end, piece_pkt): the stream table as a uint8 tensor of
        stream_cap x 80 (TCP_STREAM_DTYPE), the piece table as int64 / int32 tensors of n.
        fits False = the window or the stream table is too small and nothing was changed (an
        empty window with stream_cap 0 sizes both).  out: (streams, piece_end, piece_pkt)
        tensors to fill.  Synchronous."""
        torch = self.torch
        dev = buf.device
        if out is not None:
            streams, piece_end, piece_pkt = out
            stream_cap = streams.numel() // 80
        else:
            stream_cap = n if stream_cap is None else stream_cap
            streams = torch.zeros(max(stream_cap, 1) * 80, dtype=torch.uint8, device=dev)
            piece_end = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
            piece_pkt = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        st = TcpStats()
        tail = (_ptr(parsed["status"]), _ptr(streams), stream_cap, _ptr(piece_end),
                _ptr(piece_pkt), ctypes.byref(st), _stream(self.device))
        if "data_off" in parsed:
            what = "mgenx_pcapng_tcp"
            rc = self.lib.mgenx_pcapng_tcp(
                self.ctx, _ptr(buf), scratch_off, buf.numel(), _ptr(pkt_off),
                _ptr(parsed["data_off"]), _ptr(parsed["cap_len"]), n, link_type, flags, *tail)
        else:
            what = "mgenx_pcap_tcp"
            rc = self.lib.mgenx_pcap_tcp(self.ctx, _ptr(buf), scratch_off, buf.numel(),
                                         _ptr(pkt_off), n, link_type, flags, *tail)
        if rc != ENOSPC:
            self._check(rc, what)
        return rc == 0, st, streams, piece_end, piece_pkt

    def tcp_frame(self, buf, streams, n_streams, piece_end, piece_pkt, n_pieces, rx_sec, rx_usec,
                  long_bytes=0, cap=None):
        """mgenx_tcp_frame: the records of the streams pcap_tcp rebuilt, in completion order.
        Returns (dict of device tensors rec_off, rec_len, rec_stream, rec_pkt, rec_src
        (n x 20), rx_sec, rx_usec, each cut to the record count; stream_status; n_records).
        cap: the capacity tried first (None: two records per piece; a second call follows
        when the records do not fit); with a cap given, a result that does not fit
        comes back as (None, stream_status, n_records)."""
        torch = self.torch
        dev = buf.device
        status = torch.zeros(max(n_streams, 1), dtype=torch.uint8, device=dev)
        total = ctypes.c_uint64(0)
        retry = cap is None
        if cap is None:
            cap = max(1024, 2 * n_pieces)
        for _ in range(2):
            m = max(cap, 1)
            o = {"rec_off": torch.empty(m, dtype=torch.int64, device=dev),
                 "rec_len": torch.empty(m, dtype=torch.int32, device=dev),
                 "rec_stream": torch.empty(m, dtype=torch.int32, device=dev),
                 "rec_pkt": torch.empty(m, dtype=torch.int32, device=dev),
                 "rec_src": torch.empty(m * 20, dtype=torch.uint8, device=dev),
                 "rx_sec": torch.empty(m, dtype=torch.int32, device=dev),
                 "rx_usec": torch.empty(m, dtype=torch.int32, device=dev)}
            rc = self.lib.mgenx_tcp_frame(
                self.ctx, _ptr(buf), buf.numel(), _ptr(streams), n_streams, _ptr(piece_end),
                _ptr(piece_pkt), n_pieces, _ptr(rx_sec), _ptr(rx_usec), long_bytes,
                _ptr(o["rec_off"]), _ptr(o["rec_len"]), _ptr(o["rec_stream"]), _ptr(o["rec_pkt"]),
                _ptr(o["rec_src"]), _ptr(o["rx_sec"]), _ptr(o["rx_usec"]), cap, _ptr(status),
                ctypes.byref(total), _stream(self.device))
            self._check(rc, "mgenx_tcp_frame")
            k = int(total.value)
            if k <= cap:
                return ({name: t[:k * 20] if name == "rec_src" else t[:k]
                         for name, t in o.items()}, status[:n_streams], k)
            if not retry:
                break
            cap = k
        return None, status[:n_streams], int(total.value)

    def flow_export(self, flows, n_flows, out=None):
        if out is None:
            out = self.torch.empty(n_flows * 64, dtype=self.torch.uint8, device=flows.device)
        self._check(self.lib.mgenx_flow_export(self.ctx, _ptr(flows), n_flows, _ptr(out),
                                               _stream(self.device)), "mgenx_flow_export")
        return out

    # ------------------------------------------------------------ MGEN_DATA items
    def report_build(self, reports, n_flows, per_flow, report_count, keys, sign, offset=None):
        """MgenAnalytic report_msg bytes for the kept reports (mgenx_report_build): returns
        (items uint8 [slots*52], lengths uint8 [slots]); sign (uint8 [n_flows]) updated."""
        torch = self.torch
        slots = n_flows * per_flow
        dev = report_count.device
        items = torch.zeros(max(slots, 1) * 52, dtype=torch.uint8, device=dev)
        ilen = torch.zeros(max(slots, 1), dtype=torch.uint8, device=dev)
        self._check(self.lib.mgenx_report_build(self.ctx, _ptr(reports), n_flows, per_flow,
                                                _ptr(report_count), _ptr(keys), _ptr(sign),
                                                _ptr(offset), _ptr(items), _ptr(ilen),
                                                _stream(self.device)), "mgenx_report_build")
        return items, ilen

    def _two_pass_text(self, call, n, dev, cap):
        torch = self.torch
        line_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        for _ in range(2):
            text = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
            self._check(call(text, cap, line_off), "report text")
            total = int(line_off[-1].cpu())
            if total <= cap:
                return text[:total], line_off
            cap = total
        raise MgenxError("report text did not fit")

    def log_send(self, tmpl, desc, n, *, src_port=None, out_len=None, msg_total=None,
                 slab=None, rec_off=None, stride=0, protocol=1, opts=0, binary=False,
                 cap=None):
        """SEND events of n packed records (mgenx_log_send_text / _binary): returns (bytes
        tensor, offsets tensor of n + 1)."""
        dev = desc.device
        cap = cap if cap is not None else max(1, n) * (200 if not binary else 160)
        if binary:
            call = lambda t, c, lo: self.lib.mgenx_log_send_binary(  # noqa: E731
                self.ctx, _ptr(tmpl), _ptr(desc), _ptr(out_len), _ptr(msg_total), _ptr(slab),
                slab.numel(), _ptr(rec_off), stride, n, protocol, _ptr(t), c, _ptr(lo),
                _stream(self.device))
        else:
            call = lambda t, c, lo: self.lib.mgenx_log_send_text(  # noqa: E731
                self.ctx, _ptr(tmpl), _ptr(desc), _ptr(src_port), _ptr(out_len),
                _ptr(msg_total), n, protocol, opts, _ptr(t), c, _ptr(lo), _stream(self.device))
        return self._two_pass_text(call, n, dev, cap)

    def log_report_text(self, items, reports, n_flows, per_flow, report_count, opts=0,
                        text_cap=None):
        n = n_flows * per_flow
        cap = text_cap if text_cap is not None else max(1, n) * 220
        return self._two_pass_text(
            lambda t, c, lo: self.lib.mgenx_log_report_text(
                self.ctx, _ptr(items), _ptr(reports), n_flows, per_flow, _ptr(report_count),
                opts, _ptr(t), c, _ptr(lo), _stream(self.device)), n, items.device, cap)

    def data_walk(self, slab, n, cols, *, rec_off=None, stride=0, opts=0, cmd_cap=4096,
                  rep_cap=4096):
        """ProcessRecvMessage over MGEN_DATA payloads (mgenx_data_walk): returns (status,
        needs_host, cmds [cap x 2 u32], reps [cap x 2 u64], totals [2])."""
        torch = self.torch
        dev = slab.device
        status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        nh = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        cmds = torch.zeros(max(cmd_cap, 1) * 2, dtype=torch.int32, device=dev)
        reps = torch.zeros(max(rep_cap, 1) * 2, dtype=torch.int64, device=dev)
        totals = torch.zeros(2, dtype=torch.int32, device=dev)
        cs = self._cols_struct(cols)
        self._check(self.lib.mgenx_data_walk(self.ctx, _ptr(slab), _ptr(rec_off), stride,
                                             ctypes.byref(cs), n, opts, _ptr(status), _ptr(nh),
                                             _ptr(cmds), cmd_cap, _ptr(reps), rep_cap,
                                             _ptr(totals), _stream(self.device)),
                    "mgenx_data_walk")
        return status[:n], nh[:n], cmds, reps, totals

    def log_report_recv_text(self, slab, reps, n_reps, src, rx_sec, rx_usec, opts=0,
                             text_cap=None):
        cap = text_cap if text_cap is not None else max(1, n_reps) * 300
        return self._two_pass_text(
            lambda t, c, lo: self.lib.mgenx_log_report_recv_text(
                self.ctx, _ptr(slab), _ptr(reps), n_reps, _ptr(src), _ptr(rx_sec),
                _ptr(rx_usec), opts, _ptr(t), c, _ptr(lo), _stream(self.device)),
            n_reps, slab.device, cap)

    # ------------------------------------------------------------ multi-GPU (RCCL)
    def comm_unique_id(self) -> bytes:
        """mgenx_comm_unique_id: the 128-byte id rank 0 hands to every rank."""
        buf = ctypes.create_string_buffer(128)
        self._check(self.lib.mgenx_comm_unique_id(buf), "mgenx_comm_unique_id")
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes):
        comm = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        self._check(self.lib.mgenx_comm_init(self.ctx, nranks, rank, buf, ctypes.byref(comm)),
                    "mgenx_comm_init")
        return comm

    def comm_destroy(self, comm):
        self.lib.mgenx_comm_destroy(comm)

    def allreduce_flows(self, comm, counters, n_flows):
        """In-place SUM of n_flows x 64-B mgenx_flow_counters over the ranks (RCCL)."""
        self._check(self.lib.mgenx_allreduce_flows(self.ctx, comm, _ptr(counters), n_flows,
                                                   _stream(self.device)), "mgenx_allreduce_flows")

    def allgather_u64(self, comm, src, dst, count):
        self._check(self.lib.mgenx_allgather_u64(self.ctx, comm, _ptr(src), _ptr(dst), count,
                                                 _stream(self.device)), "mgenx_allgather_u64")

    # ------------------------------------------------------------ FindFlow
    def flow_table(self, max_flows: int):
        t = ctypes.c_void_p()
        self._check(self.lib.mgenx_flow_table_create(self.ctx, max_flows, ctypes.byref(t)),
                    "mgenx_flow_table_create")
        return t

    def flow_table_destroy(self, t):
        self.lib.mgenx_flow_table_destroy(t)

    def flow_lookup(self, table, cols, src, n, flow_idx=None, n_flows=None):
        """Dense flow index per record (mgenx_flow_lookup); returns (flow_idx, n_flows).
        n_flows[0] is the table's flow count after the call, for an empty batch (n == 0) too."""
        torch = self.torch
        dev = src.device
        if flow_idx is None:
            flow_idx = torch.empty(n, dtype=torch.int32, device=dev)
        if n_flows is None:
            n_flows = torch.zeros(1, dtype=torch.int32, device=dev)
        cs = self._cols_struct(cols)
        self._check(self.lib.mgenx_flow_lookup(self.ctx, table, ctypes.byref(cs), _ptr(src), n,
                                               _ptr(flow_idx), _ptr(n_flows),
                                               _stream(self.device)), "mgenx_flow_lookup")
        return flow_idx, n_flows

    def crc32(self, data, off, length, n, out=None):
        if out is None:
            out = self.torch.empty(n, dtype=self.torch.int32, device=data.device)
        rc = self.lib.mgenx_crc32_batch(self.ctx, _ptr(data), _ptr(off), _ptr(length), n,
                                        _ptr(out), _stream(self.device))
        self._check(rc, "mgenx_crc32_batch")
        return out


def pcap_index(buf) -> tuple:
    """mgenx_pcap_index over a host pcap image (bytes / numpy uint8): (record header offsets
    as uint64 numpy array, PcapInfo).  Host work only (the pcap_next loop)."""
    L = load()
    b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    info = PcapInfo()
    rc = L.mgenx_pcap_index(b.ctypes.data_as(ctypes.c_void_p), b.size, None, 0,
                            ctypes.byref(info))
    if rc != 0:
        raise MgenxError("mgenx_pcap_index: not a pcap file")
    offs = np.zeros(max(1, int(info.n_records)), np.uint64)
    rc = L.mgenx_pcap_index(b.ctypes.data_as(ctypes.c_void_p), b.size,
                            offs.ctypes.data_as(ctypes.c_void_p), offs.size, ctypes.byref(info))
    if rc != 0:
        raise MgenxError("mgenx_pcap_index failed")
    return offs[:int(info.n_records)], info


def pcapng_index(buf) -> tuple:
    """mgenx_pcapng_index over a host pcapng image (bytes / numpy uint8): (packet block offsets
    as uint64 numpy array, each packet's interface row as uint32 array, the interface table as
    a PCAPNG_IF_DTYPE array, PcapngInfo).  Host work only (the block walk); info.status says
    how the walk ended."""
    L = load()
    b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    info = PcapngInfo()
    p = b.ctypes.data_as(ctypes.c_void_p)
    if L.mgenx_pcapng_index(p, b.size, None, None, 0, None, 0, ctypes.byref(info)) != 0:
        raise MgenxError("mgenx_pcapng_index: not a pcapng file")
    offs = np.zeros(max(1, int(info.n_records)), np.uint64)
    pkt_if = np.zeros(offs.size, np.uint32)
    ifaces = np.zeros(max(1, int(info.n_ifaces)), PCAPNG_IF_DTYPE)
    if L.mgenx_pcapng_index(p, b.size, offs.ctypes.data_as(ctypes.c_void_p),
                            pkt_if.ctypes.data_as(ctypes.c_void_p), offs.size,
                            ifaces.ctypes.data_as(ctypes.c_void_p), ifaces.size,
                            ctypes.byref(info)) != 0:
        raise MgenxError("mgenx_pcapng_index failed")
    n = int(info.n_records)
    return offs[:n], pkt_if[:n], ifaces[:int(info.n_ifaces)], info


def is_pcapng(buf) -> bool:
    """The first four bytes are a Section Header Block's type (it reads the same in either
    byte order); a classic pcap file starts with one of its four magics instead."""
    return bytes(memoryview(buf)[:4]) == b"\x0a\x0d\x0d\x0a"


def binlog_index(buf) -> tuple:
    """mgenx_binlog_index over a host binary log image: (record offsets as uint64 numpy
    array, BinlogInfo).  Host work only."""
    L = load()
    b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    info = BinlogInfo()
    p = b.ctypes.data_as(ctypes.c_void_p)
    if L.mgenx_binlog_index(p, b.size, None, 0, ctypes.byref(info)) != 0:
        raise MgenxError("mgenx_binlog_index failed")
    offs = np.zeros(max(1, int(info.n_records)), np.uint64)
    if L.mgenx_binlog_index(p, b.size, offs.ctypes.data_as(ctypes.c_void_p), offs.size,
                            ctypes.byref(info)) != 0:
        raise MgenxError("mgenx_binlog_index failed")
    return offs[:int(info.n_records)], info


def binlog_header(buf) -> BinlogInfo:
    """mgenx_binlog_header over a host log image: the header-line rules of binlog_index alone.
    status is BINLOG_OK for a binary log (consumed = the offset of its first record), else
    BINLOG_HEADER."""
    L = load()
    b = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    info = BinlogInfo()
    if b.size == 0:
        info.status = BINLOG_HEADER
        return info
    if L.mgenx_binlog_header(b.ctypes.data_as(ctypes.c_void_p), b.size, ctypes.byref(info)) != 0:
        raise MgenxError("mgenx_binlog_header failed")
    return info


def is_binary_log(buf) -> bool:
    """True when buf starts with the header line of an MGEN binary log."""
    return binlog_header(buf).status == BINLOG_OK


_BINLOG_STATUS = {BINLOG_HEADER: "HEADER", BINLOG_TOO_LONG: "TOO_LONG", BINLOG_EVENT: "EVENT",
                  BINLOG_SHORT: "SHORT"}


def _ingest_log(eng, log_bytes, day_base):
    """A log image -> (parsed columns, n, binary): a text log through text_index and
    log_parse_text (n lines), a binary log (binlog_header says so) through binlog_index and
    binlog_parse (n records).  The columns are None when n is 0.  A binary log whose record
    walk stops before the end of the file raises MgenxError: a prefix is not analysed."""
    import torch
    dev = f"cuda:{eng.device}"
    raw = np.frombuffer(bytes(log_bytes), np.uint8)
    if is_binary_log(raw):
        offs, info = binlog_index(raw)
        if info.status != BINLOG_OK:
            raise MgenxError(f"binary log: the record walk stopped with status "
                             f"{_BINLOG_STATUS.get(info.status, info.status)} at offset "
                             f"{int(info.consumed)} after {int(info.n_records)} records")
        n = int(info.n_records)
        if n == 0:
            return None, 0, True
        buf = torch.from_numpy(raw.copy()).to(dev)
        rec_off = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
        return eng.binlog_parse(buf, rec_off, n), n, True
    n = 0
    if raw.size:
        text = torch.from_numpy(raw.copy()).to(dev)
        line_off, n = eng.text_index(text)
    if n == 0:
        return None, 0, False
    return eng.log_parse_text(text, line_off, n, day_base=day_base), n, False


def convert_binary_log(log, log_rx=True, flush=False, opts=0, device=0) -> tuple:
    """ConvertBinaryLog of a host binary log image on the GPU: (text bytes, BinlogInfo)."""
    import torch
    offs, info = binlog_index(log)
    n = int(info.n_records)
    if n == 0:
        return b"", info
    eng = Engine(device)
    try:
        dev = f"cuda:{device}"
        buf = torch.from_numpy(np.frombuffer(bytes(log), np.uint8).copy()).to(dev)
        ro = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
        flags = (0 if log_rx else BINLOG_NO_RX) | (BINLOG_FLUSH if flush else 0)
        text, _ = eng.convert_binary_log(buf, ro, n, flags, opts)
        return text.cpu().numpy().tobytes(), info
    finally:
        eng.close()


def analyze_text_log(log_bytes, window=1.0, day_base=0, device=0) -> tuple:
    """Per-flow receive analytics of an MGEN text log, on the GPU: line index -> parse ->
    FindFlow -> MgenAnalytic::Update -> counters.  Returns (keys, counters, n_lines,
    n_malformed): numpy arrays of REPORT_KEY_DTYPE and FLOW_COUNTERS_DTYPE, one element per
    flow in the order of each flow's first RECV line.  The keys' protocol is that of the
    first OK RECV line.  log_bytes may be a binary log (binlog_header says so): it is ingested by
    binlog_index and binlog_parse instead, n_lines is then the record count and n_malformed the
    MALFORMED records, and a log whose record walk stops early raises MgenxError.  The same holds
    for every analyze_text_log_* and match_text_logs* helper."""
    import torch
    eng = Engine(device)
    table = None
    try:
        p, n, _ = _ingest_log(eng, log_bytes, day_base)
        empty = (np.zeros(0, REPORT_KEY_DTYPE), np.zeros(0, FLOW_COUNTERS_DTYPE))
        if n == 0:
            return empty + (0, 0)
        n_bad = int((p["status"] != PARSE_OK).sum().item())
        table = eng.flow_table(max(n, 16))
        flow_idx, n_flows = eng.flow_lookup(table, p, p["src"], n)
        nf = int(n_flows.item())
        if nf == 0:
            return empty + (n, n_bad)
        flows = eng.flow_init(nf, window)
        eng.flow_reduce(flows, nf, flow_idx, p["seq_num"], p["tx_sec"], p["tx_usec"],
                        p["msg_len"], p["rx_sec"], p["rx_usec"], n=n)
        recv = (p["event"] == EVENT_RECV) & (p["status"] == PARSE_OK)
        proto = int(p["protocol"][recv][0].item())
        keys = eng.flow_keys(table, nf, protocol=proto)
        counters = eng.flow_export(flows, nf)
        torch.cuda.synchronize(device)
        return (keys.cpu().numpy().view(REPORT_KEY_DTYPE)[:nf].copy(),
                counters.cpu().numpy().view(FLOW_COUNTERS_DTYPE)[:nf].copy(), n, n_bad)
    finally:
        if table is not None:
            eng.flow_table_destroy(table)
        eng.close()


def flow_dist_bin(v: int) -> int:
    """The histogram bin of a latency 0 <= v < 2**32 us (mgenx_flow_dist_bin; 896 past that)."""
    return int(load().mgenx_flow_dist_bin(int(v)))


def flow_dist_bin_lo(b: int) -> int:
    """The lowest latency of bin b (mgenx_flow_dist_bin_lo; bin_lo(896) = 2**32)."""
    return int(load().mgenx_flow_dist_bin_lo(int(b)))


def _clock_opts(clock):
    """The `clock` keyword of the analysis helpers: None (raw latencies), "fit" (offset and skew
    removed per flow, mgenx_flow_clock) or "offset" (MGENX_CLOCK_OFFSET_ONLY) -> None or opts."""
    if clock is None:
        return None
    if clock == "fit":
        return 0
    if clock == "offset":
        return CLOCK_OFFSET_ONLY
    raise ValueError('clock must be None, "fit" or "offset"')


def _clock_rx(eng, clock_opts, nf, flow_idx, p, n):
    """The receive stamps an analysis reads: the parsed ones, or with a clock option the stamps
    mgenx_flow_clock corrects (the latency above each flow's fitted line, on the sender's clock)."""
    if clock_opts is None:
        return p["rx_sec"], p["rx_usec"]
    _, _, rs, ru = eng.flow_clock(nf, flow_idx, p["tx_sec"], p["tx_usec"], p["rx_sec"],
                                  p["rx_usec"], n=n, opts=clock_opts, stamps=True)
    return rs, ru


def analyze_text_log_clock(log_bytes, offset_only=False, day_base=0, device=0) -> tuple:
    """Per-flow clock offset and skew of an MGEN text log, on the GPU: line index -> parse ->
    FindFlow -> mgenx_flow_clock.  Returns (keys, clock, n_lines, n_malformed): numpy arrays of
    REPORT_KEY_DTYPE and FLOW_CLOCK_DTYPE, flows in analyze_text_log's order."""
    import torch
    eng = Engine(device)
    table = None
    try:
        p, n, _ = _ingest_log(eng, log_bytes, day_base)
        empty = (np.zeros(0, REPORT_KEY_DTYPE), np.zeros(0, FLOW_CLOCK_DTYPE))
        if n == 0:
            return empty + (0, 0)
        n_bad = int((p["status"] != PARSE_OK).sum().item())
        table = eng.flow_table(max(n, 16))
        flow_idx, n_flows = eng.flow_lookup(table, p, p["src"], n)
        nf = int(n_flows.item())
        if nf == 0:
            return empty + (n, n_bad)
        clock, _, _, _ = eng.flow_clock(nf, flow_idx, p["tx_sec"], p["tx_usec"], p["rx_sec"],
                                        p["rx_usec"], n=n, offset_only=offset_only)
        recv = (p["event"] == EVENT_RECV) & (p["status"] == PARSE_OK)
        proto = int(p["protocol"][recv][0].item())
        keys = eng.flow_keys(table, nf, protocol=proto)
        torch.cuda.synchronize(device)
        return (keys.cpu().numpy().view(REPORT_KEY_DTYPE)[:nf].copy(),
                clock.cpu().numpy().view(FLOW_CLOCK_DTYPE)[:nf].copy(), n, n_bad)
    finally:
        if table is not None:
            eng.flow_table_destroy(table)
        eng.close()


def analyze_text_log_dist(log_bytes, permille=(500, 900, 990, 999), day_base=0,
                          device=0, clock=None) -> tuple:
    """Per-flow delivery statistics of an MGEN text log, on the GPU: line index -> parse ->
    FindFlow -> mgenx_flow_dist -> quantiles.  Returns (keys, dist, quantiles, hist, n_lines,
    n_malformed): numpy arrays of REPORT_KEY_DTYPE and FLOW_DIST_DTYPE, int64 [n_flows,
    len(permille)] and uint64 [n_flows, FLOW_DIST_BINS], flows in analyze_text_log's order.
    clock="fit" or "offset" runs mgenx_flow_clock first and feeds the corrected receive stamps
    onward: every latency is then the delay above the flow's fitted line."""
    import torch
    clock_opts = _clock_opts(clock)
    eng = Engine(device)
    table = None
    try:
        p, n, _ = _ingest_log(eng, log_bytes, day_base)
        empty = (np.zeros(0, REPORT_KEY_DTYPE), np.zeros(0, FLOW_DIST_DTYPE),
                 np.zeros((0, len(permille)), np.int64), np.zeros((0, FLOW_DIST_BINS), np.uint64))
        if n == 0:
            return empty + (0, 0)
        n_bad = int((p["status"] != PARSE_OK).sum().item())
        table = eng.flow_table(max(n, 16))
        flow_idx, n_flows = eng.flow_lookup(table, p, p["src"], n)
        nf = int(n_flows.item())
        if nf == 0:
            return empty + (n, n_bad)
        rx_sec, rx_usec = _clock_rx(eng, clock_opts, nf, flow_idx, p, n)
        dist, hist = eng.flow_dist_init(nf)
        eng.flow_dist(dist, hist, nf, flow_idx, p["seq_num"], p["tx_sec"], p["tx_usec"],
                      p["msg_len"], rx_sec, rx_usec, n=n)
        quant = eng.flow_dist_quantiles(dist, hist, nf, permille)
        recv = (p["event"] == EVENT_RECV) & (p["status"] == PARSE_OK)
        proto = int(p["protocol"][recv][0].item())
        keys = eng.flow_keys(table, nf, protocol=proto)
        torch.cuda.synchronize(device)
        return (keys.cpu().numpy().view(REPORT_KEY_DTYPE)[:nf].copy(),
                dist.cpu().numpy().view(FLOW_DIST_DTYPE)[:nf].copy(), quant.cpu().numpy(),
                hist.cpu().numpy().view(np.uint64), n, n_bad)
    finally:
        if table is not None:
            eng.flow_table_destroy(table)
        eng.close()


def analyze_text_log_series(log_bytes, width_us, t0_us=None, n_bins=None, day_base=0,
                            device=0, permille=None, clock=None) -> tuple:
    """Per-flow time series of an MGEN text log, on the GPU: line index -> parse -> FindFlow ->
    mgenx_flow_series.  Returns (keys, state, bins, t0_us, n_lines, n_malformed): numpy arrays
    of REPORT_KEY_DTYPE, FLOW_SERIES_STATE_DTYPE and FLOW_SERIES_BIN_DTYPE [n_flows, n_bins],
    flows in analyze_text_log's order.  By default t0_us is the lowest receive time among the
    counted records and n_bins just enough to hold the highest (mgenx_flow_span).  With
    `permille` (values in 1..1000) the same parse also feeds mgenx_flow_series_quantiles and the
    tuple gains a seventh element: the exact latency percentiles, int64 [n_flows, n_bins,
    len(permille)].  clock="fit" or "offset" runs mgenx_flow_clock first and feeds the corrected
    receive stamps onward (the time axis is then the sender's clock, every latency the delay above
    the flow's fitted line)."""
    import torch
    clock_opts = _clock_opts(clock)
    width_us = int(width_us)
    if permille is not None:
        permille = tuple(int(q) for q in permille)
    if width_us < 1:
        raise ValueError("width_us must be at least 1")
    eng = Engine(device)
    table = None
    try:
        p, n, _ = _ingest_log(eng, log_bytes, day_base)

        def empty(n_lines, n_bad):
            r = (np.zeros(0, REPORT_KEY_DTYPE), np.zeros(0, FLOW_SERIES_STATE_DTYPE),
                 np.zeros((0, n_bins or 1), FLOW_SERIES_BIN_DTYPE),
                 0 if t0_us is None else int(t0_us), n_lines, n_bad)
            if permille is not None:
                r += (np.zeros((0, n_bins or 1, len(permille)), np.int64),)
            return r
        if n == 0:
            return empty(0, 0)
        n_bad = int((p["status"] != PARSE_OK).sum().item())
        table = eng.flow_table(max(n, 16))
        flow_idx, n_flows = eng.flow_lookup(table, p, p["src"], n)
        nf = int(n_flows.item())
        if nf == 0:
            return empty(n, n_bad)
        rx_sec, rx_usec = _clock_rx(eng, clock_opts, nf, flow_idx, p, n)
        if t0_us is None or n_bins is None:
            _, lo, hi = eng.flow_span(flow_idx, rx_sec, rx_usec, n, nf)
            if t0_us is None:
                t0_us = lo
            if n_bins is None:
                n_bins = max((hi - int(t0_us)) // width_us + 1, 1)
        t0_us, n_bins = int(t0_us), int(n_bins)
        state, bins = eng.flow_series_init(nf, n_bins)
        eng.flow_series(state, bins, nf, n_bins, t0_us, width_us, flow_idx, p["seq_num"],
                        p["tx_sec"], p["tx_usec"], p["msg_len"], rx_sec, rx_usec, n=n)
        quant = None
        if permille is not None:
            quant = eng.flow_series_quantiles(nf, n_bins, t0_us, width_us, permille, flow_idx,
                                              p["tx_sec"], p["tx_usec"], rx_sec, rx_usec, n=n)
        recv = (p["event"] == EVENT_RECV) & (p["status"] == PARSE_OK)
        proto = int(p["protocol"][recv][0].item())
        keys = eng.flow_keys(table, nf, protocol=proto)
        torch.cuda.synchronize(device)
        res = (keys.cpu().numpy().view(REPORT_KEY_DTYPE)[:nf].copy(),
               state.cpu().numpy().view(FLOW_SERIES_STATE_DTYPE).copy(),
               bins.cpu().numpy().view(FLOW_SERIES_BIN_DTYPE).reshape(nf, n_bins).copy(),
               t0_us, n, n_bad)
        if quant is not None:
            res += (quant.cpu().numpy(),)
        return res
    finally:
        if table is not None:
            eng.flow_table_destroy(table)
        eng.close()


def match_text_logs(send_log_bytes, recv_log_bytes, no_time=False, day_base=0, device=0) -> tuple:
    """A sender's text log (SEND lines) joined with a receiver's (RECV lines) on the GPU: line
    index -> parse -> match_side -> FindFlow on one table, sender first -> mgenx_msg_match.
    Returns (keys, flows, stats, send_rx_count, send_first_rx, recv_send, n_send_flows): numpy
    arrays of REPORT_KEY_DTYPE and FLOW_MATCH_DTYPE [n_flows], one MATCH_STATS_DTYPE element,
    and uint32 arrays with one element per line of the sender's log (the first two) and of the
    receiver's.  Flows are numbered by their first SEND line; the receiver-only flows follow
    from index n_send_flows.  The keys' source addresses are cleared (a SEND line has the port
    only) and their protocol is that of the first OK SEND line.  Either log may be a binary log.
    A binary SEND record has no source port, so when the sender's log is binary the port is
    cleared on both sides before the flows are looked up: flows that differ only in source port
    merge.  match_text_logs_timeline and match_text_logs_multi do the same."""
    return _match_text_logs(send_log_bytes, recv_log_bytes, no_time, day_base, device, None)


def match_text_logs_timeline(send_log, recv_log, width_us, t0_us=None, n_bins=None, min_run=1,
                             no_time=False, day_base=0, device=0) -> tuple:
    """match_text_logs on the sender's time axis (mgenx_msg_match_ex): the exact loss per window
    of send time and the loss runs.  Returns (keys, flows, stats, bins, outside, runs, t0_us,
    n_send_flows): keys, flows and stats as match_text_logs gives them, bins MATCH_BIN_DTYPE
    [n_flows, n_bins] (window b starts at t0_us + b * width_us), outside uint64 [n_flows] (the
    messages sent outside the windows), runs LOSS_RUN_DTYPE (the runs of at least min_run lost
    messages, by flow and first send index; first_send / last_send are 0-based lines of the
    sender's log).  By default t0_us is the lowest SEND stamp of the sender's log and n_bins just
    enough for the highest (mgenx_flow_span over the sender's columns)."""
    tl = dict(width_us=int(width_us), t0_us=t0_us, n_bins=n_bins, min_run=int(min_run))
    return _match_text_logs(send_log, recv_log, no_time, day_base, device, tl)


def match_text_logs_multi(send_log, recv_logs, width_us=None, t0_us=None, n_bins=None,
                          no_time=False, day_base=0, device=0, min_run=None,
                          pairs=False) -> tuple:
    """A sender's text log (SEND lines) joined with the text logs of several receivers (RECV
    lines) on the GPU: every log goes through line index -> parse -> match_side, FindFlow runs
    on one table (sender first, then the receivers in the order given), the receivers' columns
    are concatenated with the receiver's index as a column, and mgenx_msg_match_multi joins
    them.  Returns (keys, cells, fanout, stats, send_mask, n_send_flows): REPORT_KEY_DTYPE
    [n_flows], RCV_CELL_DTYPE [n_flows, n_rcv], FLOW_FANOUT_DTYPE [n_flows], one
    MATCH_STATS_DTYPE element, uint64 with one element per line of the sender's log (bit r: the
    message reached receiver r), and the number of flows the sender's log has (receiver-only
    flows follow).  With width_us also (bins, outside, t0_us): MULTI_BIN_DTYPE [n_flows, n_bins]
    over windows of send time, uint64 [n_flows], and the first window's start; by default t0_us
    is the lowest SEND stamp and n_bins just enough for the highest.
    With min_run (an int; 0 is taken as 1) or pairs=True the join is mgenx_msg_match_multi_ex and
    the tuple goes on, after whatever stands above, with: for min_run (rcv_runs, runs),
    RCV_RUNS_DTYPE [n_flows, n_rcv] and RCV_LOSS_RUN_DTYPE (the runs of at least min_run lost
    messages by flow, last send index and receiver; first_send / last_send are 0-based lines of
    the sender's log); then for pairs RCV_PAIR_DTYPE [n_flows, n_rcv, n_rcv].  Without them the
    call returns exactly what it returned before they existed."""
    import torch
    recv_logs = list(recv_logs)
    n_rcv = len(recv_logs)
    if not 1 <= n_rcv <= MATCH_MAX_RCV:
        raise ValueError(f"match_text_logs_multi: 1 to {MATCH_MAX_RCV} receiver logs")
    eng = Engine(device)
    table = None
    try:
        dev = f"cuda:{device}"

        def side(log, want, no_port=False):
            return _match_side_of(eng, log, want, day_base, no_port)

        s, s_src, ns, s_bin = side(send_log, EVENT_SEND)
        rsides = [side(log, EVENT_RECV, s_bin)[:3] for log in recv_logs]
        nr = sum(n for _, _, n in rsides)
        none = torch.zeros(0, dtype=torch.int32, device=dev)
        s_idx = none
        r_idx = [none] * n_rcv
        nf = n_send = 0
        cap = max(ns + nr, 16)
        while ns + nr:
            # FLOW_NONE on an OK line means "redo on a larger table", never "no such flow"
            table = eng.flow_table(cap)
            refused = False
            if ns:
                s_idx, n_flows = eng.flow_lookup(table, s, s_src, ns)
                n_send = int(n_flows.item())
                refused = bool(((s["err"][:ns] == 0) & (s_idx == -1)).any().item())
            nf = n_send
            for k, (r, r_src, n) in enumerate(rsides):
                if n and not refused:
                    r_idx[k], n_flows = eng.flow_lookup(table, r, r_src, n)
                    nf = int(n_flows.item())
                    refused = bool(((r["err"][:n] == 0) & (r_idx[k] == -1)).any().item())
            if not refused:
                break
            eng.flow_table_destroy(table)
            table = None
            cap *= 4
        send = dict(flow_idx=s_idx, seq=none, t_sec=none, t_usec=none, len=none)
        if ns:
            send.update(seq=s["seq_num"], t_sec=s["rx_sec"], t_usec=s["rx_usec"], len=s["size"])
        recv = dict(flow_idx=none, seq=none, tx_sec=none, tx_usec=none, rx_sec=none, rx_usec=none,
                    rcv=none)
        if nr:
            live = [(k, r, n) for k, (r, _, n) in enumerate(rsides) if n]
            cat = lambda name: torch.cat([r[name][:n].view(torch.int32)  # noqa: E731
                                          for _, r, n in live])
            recv.update(flow_idx=torch.cat([r_idx[k][:n] for k, _, n in live]),
                        seq=cat("seq_num"), tx_sec=cat("tx_sec"), tx_usec=cat("tx_usec"),
                        rx_sec=cat("rx_sec"), rx_usec=cat("rx_usec"),
                        rcv=torch.repeat_interleave(
                            torch.tensor([k for k, _, _ in live], dtype=torch.int32, device=dev),
                            torch.tensor([n for _, _, n in live], device=dev)))
        opts = MATCH_NO_TIME if no_time else 0
        timeline = None
        if width_us is not None:
            width_us = int(width_us)
            if t0_us is None or n_bins is None:
                lo, hi = 2**64 - 1, 0
                if ns and nf:
                    _, lo, hi = eng.flow_span(s_idx, s["rx_sec"], s["rx_usec"], ns, nf)
                if lo > hi:                  # no SEND line counts
                    lo = hi = 0
                if t0_us is None:
                    t0_us = lo
                if n_bins is None:
                    n_bins = max((hi - int(t0_us)) // width_us + 1, 1)
            t0_us, n_bins = int(t0_us), int(n_bins)
            timeline = (t0_us, width_us, n_bins)
        loss = min_run is not None or pairs
        if loss:
            out = eng.msg_match_multi_loss(nf, n_rcv, send, recv, run_stats=min_run is not None,
                                           min_run=min_run, pairs=pairs, opts=opts,
                                           timeline=timeline, ns=ns, nr=nr)
        else:
            out = eng.msg_match_multi(nf, n_rcv, send, recv, opts=opts, timeline=timeline, ns=ns,
                                      nr=nr)
        mask, _rs, _first, cells, fanout, stats = out[:6]
        keys = np.zeros(0, REPORT_KEY_DTYPE)
        if nf:
            proto = 1
            for p in [s] + [r for r, _, _ in rsides]:
                if p is not None:
                    ok = p["protocol"][p["err"] == 0]
                    if ok.numel():
                        proto = int(ok[0].item())
                        break
            keys = eng.flow_keys(table, nf, protocol=proto).cpu().numpy().view(
                REPORT_KEY_DTYPE)[:nf].copy()
        torch.cuda.synchronize(device)
        res = (keys, cells.cpu().numpy().view(RCV_CELL_DTYPE).reshape(nf, n_rcv).copy(),
               fanout.cpu().numpy().view(FLOW_FANOUT_DTYPE).copy(),
               stats.cpu().numpy().view(MATCH_STATS_DTYPE)[0].copy(),
               mask.cpu().numpy().view(np.uint64).copy(), n_send)
        if timeline is not None:
            res += (out[6].cpu().numpy().view(MULTI_BIN_DTYPE).reshape(nf, n_bins).copy(),
                    out[7].cpu().numpy().view(np.uint64).copy(), t0_us)
        if min_run is not None:
            res += (out[-3].cpu().numpy().view(RCV_RUNS_DTYPE).reshape(nf, n_rcv).copy(),
                    out[-2].cpu().numpy().view(RCV_LOSS_RUN_DTYPE).copy())
        if pairs:
            res += (out[-1].cpu().numpy().view(RCV_PAIR_DTYPE).reshape(nf, n_rcv, n_rcv).copy(),)
        return res
    finally:
        if table is not None:
            eng.flow_table_destroy(table)
        eng.close()


def _match_side_of(eng, log, want, day_base, no_port):
    """One log as a side of msg_match: (cols, src, n, binary) through _ingest_log and
    match_side.  A binary log's SEND records have no source port (src reads port 0), so when
    the sender's log is binary the port is cleared on both sides' src (no_port for the
    receivers' logs): the flows then differ by flow id and destination only."""
    p, n, binary = _ingest_log(eng, log, day_base)
    if n == 0:
        return None, None, 0, binary
    cols, src = eng.match_side(p, n, want)
    if no_port or (binary and want == EVENT_SEND):
        src.view(-1, ADDR_DTYPE.itemsize)[:, 2:4] = 0
    return cols, src, n, binary


def _match_text_logs(send_log_bytes, recv_log_bytes, no_time, day_base, device, tl) -> tuple:
    import torch
    eng = Engine(device)
    table = None
    try:
        dev = f"cuda:{device}"

        def side(log, want, no_port=False):
            return _match_side_of(eng, log, want, day_base, no_port)

        s, s_src, ns, s_bin = side(send_log_bytes, EVENT_SEND)
        r, r_src, nr, _ = side(recv_log_bytes, EVENT_RECV, s_bin)
        none = torch.zeros(0, dtype=torch.int32, device=dev)
        s_idx = r_idx = none
        nf = n_send = 0
        cap = max(ns + nr, 16)
        while ns + nr:
            # FLOW_NONE on an OK line means "redo on a larger table", never "no such flow"
            table = eng.flow_table(cap)
            refused = False
            if ns:
                s_idx, n_flows = eng.flow_lookup(table, s, s_src, ns)
                n_send = int(n_flows.item())
                refused = bool(((s["err"][:ns] == 0) & (s_idx == -1)).any().item())
            nf = n_send
            if nr and not refused:
                r_idx, n_flows = eng.flow_lookup(table, r, r_src, nr)
                nf = int(n_flows.item())
                refused = bool(((r["err"][:nr] == 0) & (r_idx == -1)).any().item())
            if not refused:
                break
            eng.flow_table_destroy(table)
            table = None
            cap *= 4
        send = dict(flow_idx=s_idx, seq=none, t_sec=none, t_usec=none, len=none)
        if ns:
            send.update(seq=s["seq_num"], t_sec=s["rx_sec"], t_usec=s["rx_usec"], len=s["size"])
        recv = dict(flow_idx=r_idx, seq=none, tx_sec=none, tx_usec=none, rx_sec=none, rx_usec=none)
        if nr:
            recv.update(seq=r["seq_num"], tx_sec=r["tx_sec"], tx_usec=r["tx_usec"],
                        rx_sec=r["rx_sec"], rx_usec=r["rx_usec"])
        opts = MATCH_NO_TIME if no_time else 0
        if tl is None:
            cnt, first, rs, flows, stats = eng.msg_match(nf, send, recv, opts=opts, ns=ns, nr=nr)
        else:
            t0_us, n_bins = tl["t0_us"], tl["n_bins"]
            if t0_us is None or n_bins is None:
                lo, hi = 2**64 - 1, 0
                if ns and nf:
                    _, lo, hi = eng.flow_span(s_idx, s["rx_sec"], s["rx_usec"], ns, nf)
                if lo > hi:                  # no SEND line counts
                    lo = hi = 0
                if t0_us is None:
                    t0_us = lo
                if n_bins is None:
                    n_bins = max((hi - int(t0_us)) // tl["width_us"] + 1, 1)
            t0_us, n_bins = int(t0_us), int(n_bins)
            cnt, first, rs, flows, stats, bins, outside, runs, _owner = eng.msg_match_timeline(
                nf, send, recv, t0_us, tl["width_us"], n_bins, min_run=tl["min_run"], opts=opts,
                ns=ns, nr=nr)
        keys = np.zeros(0, REPORT_KEY_DTYPE)
        if nf:
            proto = 1
            for p in (s, r):
                if p is not None:
                    ok = p["protocol"][p["err"] == 0]
                    if ok.numel():
                        proto = int(ok[0].item())
                        break
            keys = eng.flow_keys(table, nf, protocol=proto).cpu().numpy().view(
                REPORT_KEY_DTYPE)[:nf].copy()
        torch.cuda.synchronize(device)
        u32 = lambda t: t.cpu().numpy().view(np.uint32).copy()  # noqa: E731
        if tl is not None:
            return (keys, flows.cpu().numpy().view(FLOW_MATCH_DTYPE).copy(),
                    stats.cpu().numpy().view(MATCH_STATS_DTYPE)[0].copy(),
                    bins.cpu().numpy().view(MATCH_BIN_DTYPE).reshape(nf, n_bins).copy(),
                    outside.cpu().numpy().view(np.uint64).copy(),
                    runs.cpu().numpy().view(LOSS_RUN_DTYPE).copy(), t0_us, n_send)
        return (keys, flows.cpu().numpy().view(FLOW_MATCH_DTYPE).copy(),
                stats.cpu().numpy().view(MATCH_STATS_DTYPE)[0].copy(), u32(cnt), u32(first),
                u32(rs), n_send)
    finally:
        if table is not None:
            eng.flow_table_destroy(table)
        eng.close()


def to_device(arr: np.ndarray, device=0):
    """Copy a numpy (structured) array to the GPU as raw bytes (uint8 tensor)."""
    import torch
    b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    return torch.from_numpy(b.copy()).to(f"cuda:{device}")


class Worker:
    """mgenx_worker: MgenMsg::Unpack / ComputeCRC32 of one host message per call, served by a
    wave resident on the device (no launch or copy per call)."""

    def __init__(self, eng: Engine, idle_ms: int = 200):
        self.eng = eng
        self.w = ctypes.c_void_p()
        eng._check(eng.lib.mgenx_worker_create(eng.ctx, idle_ms, ctypes.byref(self.w)),
                   "mgenx_worker_create")

    def unpack(self, msg: bytes):
        """One record's mgenx_unpacked (numpy structured scalar, UNPACKED_DTYPE)."""
        out = np.zeros(1, UNPACKED_DTYPE)
        self.eng._check(self.eng.lib.mgenx_worker_unpack(self.w, bytes(msg), len(msg),
                                                         ctypes.c_void_p(out.ctypes.data)),
                        "mgenx_worker_unpack")
        return out[0]

    def recv(self, msg: bytes, force: bool = False):
        """The receive path's Unpack + ComputeCRC32(0, msg, len - 4) in one call
        (mgenx_worker_recv): (mgenx_unpacked, crc state or None when no checksum was due)."""
        out = np.zeros(1, UNPACKED_DTYPE)
        crc, done = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self.eng._check(self.eng.lib.mgenx_worker_recv(self.w, bytes(msg), len(msg), int(force),
                                                       ctypes.c_void_p(out.ctypes.data),
                                                       ctypes.byref(crc), ctypes.byref(done)),
                        "mgenx_worker_recv")
        return out[0], (crc.value if done.value else None)

    def flow_update(self, flows, slot, seq, rx_sec, rx_usec, msg_size, tx_sec, tx_usec):
        """MgenAnalytic::Update of one record on device flow state flows[slot]
        (mgenx_worker_flow_update): the closed window's report (FLOW_REPORT_DTYPE) or None."""
        rep = np.zeros(1, FLOW_REPORT_DTYPE)
        up = ctypes.c_uint32(0)
        self.eng._check(self.eng.lib.mgenx_worker_flow_update(
            self.w, _ptr(flows), slot, seq & 0xFFFFFFFF, rx_sec, rx_usec, msg_size, tx_sec,
            tx_usec, ctypes.byref(up), ctypes.c_void_p(rep.ctypes.data)), "mgenx_worker_flow_update")
        return rep[0] if up.value else None

    def device_mailbox(self) -> bool:
        """Whether requests go to device memory written through the BAR (mgenx_worker_info)."""
        f = ctypes.c_uint32(0)
        self.eng._check(self.eng.lib.mgenx_worker_info(self.w, ctypes.byref(f)), "mgenx_worker_info")
        return bool(f.value & 1)

    def crc32(self, data: bytes, state: int = 0) -> int:
        out = ctypes.c_uint32(0)
        self.eng._check(self.eng.lib.mgenx_worker_crc32(self.w, bytes(data), len(data), state,
                                                        ctypes.byref(out)),
                        "mgenx_worker_crc32")
        return out.value

    def pack(self, tmpl, payload: bytes, desc, buf_len: int, crc_in: int = 0, opts: int = 0,
             fill_time: int = 0):
        """MgenMsg::Pack of one message (mgenx_worker_pack): (bytes, tx_crc, state).  tmpl /
        desc: one-element TMPL_DTYPE / DESC_DTYPE arrays."""
        t = np.ascontiguousarray(tmpl)
        d = np.ascontiguousarray(desc)
        out = np.zeros(max(buf_len, 1), np.uint8)
        ret, tx, st = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self.eng._check(self.eng.lib.mgenx_worker_pack(
            self.w, ctypes.c_void_p(t.ctypes.data), bytes(payload), ctypes.c_void_p(d.ctypes.data),
            buf_len, crc_in, opts, fill_time, ctypes.c_void_p(out.ctypes.data), ctypes.byref(ret),
            ctypes.byref(tx), ctypes.byref(st)), "mgenx_worker_pack")
        return out[:ret.value].tobytes(), tx.value, st.value

    def stop(self):
        """End the resident wave now (the next call relaunches it)."""
        if self.w:
            self.eng._check(self.eng.lib.mgenx_worker_stop(self.w), "mgenx_worker_stop")

    def close(self):
        # (after Engine.close the handle only frees itself: mgenx_ctx_destroy stopped the wave)
        if self.w:
            self.eng.lib.mgenx_worker_destroy(self.w)
            self.w = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
