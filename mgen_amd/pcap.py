"""pcap2mgen on the GPU: a capture file -> the MGEN text log (src/common/pcap2mgen.cpp:252-482).

The reference walks the capture one packet at a time: pcap_next, an Ethernet / IP / UDP parse,
``MgenMsg::Unpack`` (no CRC check), then with ``analytic`` ``FindFlow`` + ``Update`` (logging
the analytic's REPORT line when a window closes), ``LogRecvEvent`` (the RECV line, GMT
timestamps, GPS, TTL, no data), and the REPORT lines of any reports the payload carries.
Here the whole file goes to HBM once and every stage is one batch call of the C ABI:

  mgenx_pcap_index (host: the record-header chain) -> mgenx_pcap_parse [a pcapng capture:
  mgenx_pcapng_index (host: the block walk) -> mgenx_pcapng_parse] -> mgenx_unpack_batch
  (MGENX_OPT_SKIP_CRC: Unpack alone) -> [mgenx_flow_lookup -> mgenx_flow_reduce_ex ->
  mgenx_flow_keys -> mgenx_report_build -> mgenx_log_report_text] -> mgenx_log_recv_text
  (MGENX_LOG_SKIP_ERR) -> mgenx_data_walk + mgenx_log_report_recv_text ->
  mgenx_text_interleave (per packet: analytic REPORT, RECV, received REPORTs).

``reassemble`` (not in the reference, off by default) adds mgenx_pcap_defrag /
mgenx_pcapng_defrag after the snap step: fragmented IPv4 / IPv6 datagrams are rebuilt in
scratch after the file image and logged at their completing fragment's position.

``tcp`` (not in the reference, which drops every packet that is not UDP; off by default) adds
mgenx_pcap_tcp / mgenx_pcapng_tcp -> mgenx_tcp_frame -> mgenx_unpack_batch (MGENX_OPT_TCP) ->
mgenx_log_recv_text (protocol 2, RERR lines kept): the byte stream of every TCP connection is
rebuilt in a further scratch window, framed into MGEN records, and each record is logged at the
position of the packet that completed it, after that packet's own lines.  Every record is
unpacked into a fresh message (the receiver's persistent rx_msg, mgenx_tcp_rx_persist, is not
emulated offline); ``analytic`` stays UDP-only, REPORT items inside TCP payloads are not
logged, and IP-fragmented TCP and IPv6 extension headers are not followed.

Options mirror the reference's command line (``-analytic``/``-report``, ``+rxlog on|off``,
``+window``); ``trace`` (MAC addresses in front of each line) is not supported.
"""
from __future__ import annotations

import numpy as np

from . import (DATA_CONTROLLER, FLOW_REPORT_DTYPE, LOG_EPOCH, LOG_NO_DATA, LOG_SKIP_ERR,
               OPT_SKIP_CRC, OPT_TCP, PCAP_NG, TEXT_OWNER, TEXT_PER_RECORD, TEXT_SCATTER, Engine,
               MgenxError, is_pcapng, pcap_index, pcapng_index)


def _quantized_window(window: float) -> float:
    """Report::QuantizeTimeValue / UnquantizeTimeValue (mgenAnalytic.cpp:621-642)."""
    import math
    stretch, tmin, tmax = 1.1, 1.0e-06, 600.0
    scale = 1.0 / (math.pow(stretch, 254) - stretch)
    if window > stretch * tmax:
        q = 0xFF
    elif window < tmin / 2.0:
        q = 0
    elif window < tmin:
        q = 1
    else:
        q = int((math.log(stretch + (window - tmin) / (scale * (tmax - tmin))) / math.log(stretch))
                + 0.5) & 0xFF
    return 0.0 if q == 0 else (tmax - tmin) * (math.pow(stretch, q) - stretch) * scale + tmin


class Pcap2Mgen:
    """pcap2mgen with its options; ``run(file)`` returns the log bytes.  Everything after the
    host index walk runs on the engine's GPU."""

    FIRST_FLOWS = 65536  # flow-table capacity tried first (see run_device)

    def __init__(self, engine: Engine, analytics: bool = False, log_rx: bool = True,
                 window: float = 1.0, epoch: bool = False, reassemble: bool = False,
                 frag_timeout: float = 30.0, tcp: bool = False):
        self.eng = engine
        self.tcp = tcp
        self.last_tcp_stats = None            # TcpStats of the last run with tcp
        self.last_tcp_records = 0             # records framed by the last run with tcp
        self.reassemble = reassemble
        self.frag_timeout = frag_timeout      # seconds; 0 = fragments never expire
        self.last_defrag_stats = None         # DefragStats of the last reassembling run
        self.analytics = analytics
        self.log_rx = log_rx
        self.window = window
        self.opts = LOG_EPOCH if epoch else 0

    def upload(self, file):
        """Host index walk + one H2D copy: (device file, device record offsets, PcapInfo).
        A pcapng capture (told by its first four bytes): the offsets are its packet blocks,
        the info is a PcapngInfo with two more attributes for run_device's `ng`, pkt_if and
        ifaces (device tensors: each packet's interface row, the interface table).
        With reassemble the buffer also holds the defrag scratch, from info.defrag_off on:
        as many bytes as the file (each fragment's payload is shorter than its record).
        With tcp a further window of as many bytes follows, from info.tcp_off on (each
        segment's payload is shorter than its record by more than 16 bytes)."""
        torch = self.eng.torch
        b = np.frombuffer(bytes(file), np.uint8) if not isinstance(file, np.ndarray) else file
        dev = f"cuda:{self.eng.device}"
        if is_pcapng(b):
            offs, pkt_if, ifaces, info = pcapng_index(b)
            info.pkt_if = torch.from_numpy(pkt_if.view(np.int32).copy()).to(dev)
            info.ifaces = torch.from_numpy(ifaces.view(np.uint8).copy()).to(dev)
        else:
            offs, info = pcap_index(b)
        # the file image, then scratch for packets cut by the snapshot length (mgenx_pcap_snap)
        size = b.size + int(info.snap_bytes)
        info.file_bytes = b.size
        info.defrag_off = None
        if self.reassemble:
            info.defrag_off = (size + 15) & ~15
            size = info.defrag_off + b.size
        info.tcp_off = None
        if self.tcp:
            info.tcp_off = (size + 15) & ~15
            size = info.tcp_off + b.size
        buf = torch.zeros(size, dtype=torch.uint8, device=dev)
        buf[:b.size] = torch.from_numpy(b.copy()).to(dev)
        pkt_off = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
        return buf, pkt_off, info

    def run(self, file) -> bytes:
        buf, pkt_off, info = self.upload(file)
        file_bytes = info.file_bytes
        ng = (info.pkt_if, info.ifaces) if info.flags & PCAP_NG else None
        text, _ = self.run_device(buf, pkt_off, int(info.n_records), info.link_type, info.flags,
                                  file_bytes=file_bytes, ng=ng, defrag_off=info.defrag_off,
                                  tcp_off=info.tcp_off)
        return text.cpu().numpy().tobytes()

    def run_device(self, buf, pkt_off, n, link_type, flags, file_bytes=None, ng=None,
                   defrag_off=None, tcp_off=None):
        """The device pipeline over a resident file: (text tensor, per-packet offsets).
        file_bytes: the file image's size when buf has scratch after it for snapped packets
        (None: no scratch; packets cut by the snapshot length are skipped).
        ng: for a pcapng capture, (pkt_if, ifaces) on the device -- pkt_off then holds the
        packet blocks' offsets (mgenx_pcapng_index).
        defrag_off: with reassemble, where the defrag scratch starts in buf (the snap scratch
        then ends there); None: no scratch, and a capture with fragments to rebuild raises.
        tcp_off: with tcp, where the stream scratch starts in buf (the scratch before it ends
        there); None: no scratch, and a capture with TCP payload raises."""
        eng, torch = self.eng, self.eng.torch
        dev = buf.device
        if n == 0:
            return torch.empty(0, dtype=torch.uint8, device=dev), torch.zeros(
                1, dtype=torch.int64, device=dev)
        tcp_at = buf.numel() if tcp_off is None else tcp_off
        snap_end = tcp_at if defrag_off is None else defrag_off
        snap = file_bytes is not None and file_bytes < snap_end
        if ng is not None:
            pkt_if, ifaces = ng
            p = eng.pcapng_parse(buf, pkt_off, pkt_if, n, ifaces, ifaces.numel() // 24,
                                 link_type, flags)
            if snap:
                eng.pcapng_snap(buf, file_bytes, n, p, buf_bytes=snap_end)
        else:
            p = eng.pcap_parse(buf, pkt_off, n, link_type, flags)
            if snap:
                eng.pcap_snap(buf, file_bytes, pkt_off, n, flags, p, buf_bytes=snap_end)
        if self.reassemble:
            defrag = eng.pcap_defrag if ng is None else eng.pcapng_defrag
            fits, st = defrag(buf[:tcp_at], snap_end, pkt_off, n, link_type, flags, p,
                              timeout_us=round(self.frag_timeout * 1e6))
            self.last_defrag_stats = st
            if not fits:
                raise MgenxError(f"pcap2mgen: reassembly needs {st.scratch_bytes} bytes of "
                                 f"scratch, the buffer has {tcp_at - snap_end}")
        tcp_recs = self._tcp_records(buf, tcp_at, pkt_off, n, link_type, flags, p) if self.tcp \
            else None
        cols = eng.unpack(buf, n, rec_off=p["udp_off"], rec_len=p["udp_len"], opts=OPT_SKIP_CRC,
                          ext=True)
        sources = []
        keep = []
        if self.analytics:
            # a table for up to FIRST_FLOWS flows first (a table for n flows is 64 x 2n bytes to
            # allocate, clear and free on every run); if it overflowed -- a record of a good
            # message left without a flow -- the lookup is redone on a table for n flows
            cap_flows = min(max(n, 1), self.FIRST_FLOWS)
            table = eng.flow_table(cap_flows)
            try:
                flow_idx, nfl = eng.flow_lookup(table, cols, p["src"], n)
                if cap_flows < n:
                    lost = ((flow_idx[:n] < 0) & (cols["err"][:n] == 0)).any()
                    st = torch.stack([nfl[0].to(torch.int64), lost.to(torch.int64)]).cpu()
                    n_flows, overflow = int(st[0]), bool(st[1])
                else:
                    n_flows, overflow = int(nfl.item()), False
                if overflow:
                    eng.flow_table_destroy(table)
                    table = None    # a failing create below must not free it again
                    table = eng.flow_table(max(n, 1))
                    flow_idx, nfl = eng.flow_lookup(table, cols, p["src"], n)
                    n_flows = int(nfl.item())
                if n_flows:
                    per_flow = self._per_flow(p, flow_idx, n, n_flows)
                    flows = eng.flow_init(n_flows, self.window)
                    reports = torch.zeros(n_flows * per_flow * FLOW_REPORT_DTYPE.itemsize,
                                          dtype=torch.uint8, device=dev)
                    count = torch.zeros(n_flows, dtype=torch.int32, device=dev)
                    rep_rec = torch.full((n_flows * per_flow,), -1, dtype=torch.int32,
                                         device=dev)
                    eng.flow_reduce(flows, n_flows, flow_idx, cols["seq_num"], cols["tx_sec"],
                                    cols["tx_usec"], cols["msg_len"], p["rx_sec"], p["rx_usec"],
                                    n=n, reports=reports, per_flow=per_flow, report_count=count,
                                    report_rec=rep_rec)
                    keys = eng.flow_keys(table, n_flows, protocol=1)
                    sign = torch.zeros(n_flows, dtype=torch.uint8, device=dev)
                    items, _ = eng.report_build(reports, n_flows, per_flow, count, keys, sign)
                    rtext, rline = eng.log_report_text(items, reports, n_flows, per_flow, count,
                                                       opts=self.opts)
                    sources.append((TEXT_SCATTER, rtext, rline, n_flows * per_flow, rep_rec, 1))
                    keep += [reports, count, rep_rec, items]
            finally:
                if table is not None:
                    eng.flow_table_destroy(table)
        if self.log_rx:  # LogRecvEvent(..., logData false, logGpsData true, ttl, hdr.ts)
            text, line_off = eng.log_recv_text(buf, n, cols, p["src"], p["rx_sec"],
                                               p["rx_usec"], rec_off=p["udp_off"], ttl=p["ttl"],
                                               protocol=1,
                                               opts=self.opts | LOG_NO_DATA | LOG_SKIP_ERR)
            sources.append((TEXT_PER_RECORD, text, line_off, n, None, 1))
        # the REPORT items of MGEN_DATA payloads (LogRecvEvent, mgenMsg.cpp:1104-1137)
        cap = 1024
        for _ in range(2):
            _, _, _, reps, totals = eng.data_walk(buf, n, cols, rec_off=p["udp_off"],
                                                  opts=DATA_CONTROLLER, cmd_cap=1, rep_cap=cap)
            n_reps = int(totals[1].item())
            if n_reps <= cap:
                break
            cap = n_reps
        if n_reps:
            rr_text, rr_line = eng.log_report_recv_text(buf, reps, n_reps, p["src"], p["rx_sec"],
                                                        p["rx_usec"], opts=self.opts)
            sources.append((TEXT_OWNER, rr_text, rr_line, n_reps, reps.view(torch.int32), 4))
        if tcp_recs is not None and self.log_rx:
            # each record a fresh MgenMsg, TCP receive rules and CRC check; an error logs RERR
            # (MgenTcpTransport::OnRecvMsg, mgenTransport.cpp:1736-1750)
            r, k = tcp_recs
            tcols = eng.unpack(buf, k, rec_off=r["rec_off"], rec_len=r["rec_len"], opts=OPT_TCP,
                               ext=True)
            ttext, tline = eng.log_recv_text(buf, k, tcols, r["rec_src"], r["rx_sec"],
                                             r["rx_usec"], rec_off=r["rec_off"], ttl=None,
                                             protocol=2, opts=self.opts | LOG_NO_DATA)
            sources.append((TEXT_OWNER, ttext, tline, k, r["rec_pkt"], 1))
        if not sources:
            return torch.empty(0, dtype=torch.uint8, device=dev), torch.zeros(
                n + 1, dtype=torch.int64, device=dev)
        return eng.text_interleave(sources, n)

    def _tcp_records(self, buf, tcp_at, pkt_off, n, link_type, flags, p):
        """pcap_tcp + tcp_frame over the parsed packets: (record arrays, count), or None when
        the capture holds no TCP record."""
        eng = self.eng
        cap = min(n, 4096)
        for _ in range(2):
            fits, st, streams, piece_end, piece_pkt = eng.pcap_tcp(
                buf, tcp_at, pkt_off, n, link_type, flags, p, stream_cap=cap)
            if fits or st.n_streams <= cap:
                break
            cap = int(st.n_streams)
        self.last_tcp_stats = st
        self.last_tcp_records = 0
        if not fits:
            raise MgenxError(f"pcap2mgen: the TCP streams need {st.scratch_bytes} bytes of "
                             f"scratch, the buffer has {buf.numel() - tcp_at}")
        recs, _, k = eng.tcp_frame(buf, streams, int(st.n_streams), piece_end, piece_pkt,
                                   int(st.n_pieces), p["rx_sec"], p["rx_usec"])
        self.last_tcp_records = k
        return (recs, k) if k else None

    def _per_flow(self, p, flow_idx, n, n_flows) -> int:
        """Report slots per flow: a window closes at most once per record and at most once
        per window length of capture time (the window restarts at the closing record).  The
        counts and the time range are reduced on the device (mgenx_flow_span, one read-back)."""
        most, lo, hi = self.eng.flow_span(flow_idx, p["rx_sec"], p["rx_usec"], n, n_flows)
        if most == 0:
            return 1
        span = float(hi - lo) * 1e-6
        w = _quantized_window(self.window)
        by_time = most if w <= 0.0 else int(span / w) + 2
        return max(1, min(most, by_time))


def pcap2mgen(file, analytics=False, log_rx=True, window=1.0, epoch=False, device=0,
              reassemble=False, frag_timeout=30.0, tcp=False) -> bytes:
    """One-shot helper: the log text of a pcap or pcapng file image."""
    eng = Engine(device)
    try:
        return Pcap2Mgen(eng, analytics, log_rx, window, epoch, reassemble, frag_timeout,
                         tcp).run(file)
    finally:
        eng.close()


__all__ = ["Pcap2Mgen", "pcap2mgen", "MgenxError"]
