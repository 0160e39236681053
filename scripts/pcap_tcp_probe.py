"""TCP path timing: two synthetic captures of 1 Mi TCP segments of 1448 payload
bytes each (1024-byte MGEN messages from the GPU TCP transmit path, about 1.5 GB of stream),
device-resident -- one connection, and 1024 connections interleaved packet by packet.

  python scripts/pcap_tcp_probe.py              per-stage times and the whole `tcp` pipeline of
                                                both captures, mgenx_tcp_frame under both routes
                                                (long_bytes 1 / 2^64-1) where that is sane, then
                                                the UDP pipeline over workloads.pcap_capture with
                                                the same packet count
  python scripts/pcap_tcp_probe.py --udp-only   that UDP run alone (uses nothing this feature
                                                added: run it in a checkout of the parent commit
                                                for the before / after pair)
  python scripts/pcap_tcp_probe.py --small      2^14 segments: a rehearsal of every code path

Device events (torch.cuda.Event), median of 20 after 3 warm-ups.  GB/s is over algorithmic
bytes: the file read once, the stream bytes written once and read twice (frame, unpack)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd import PACK_CHECKSUM, Engine, to_device  # noqa: E402
from mgen_amd._abi import DESC_DTYPE  # noqa: E402
from mgen_amd.pcap import Pcap2Mgen  # noqa: E402
from mgen_amd.workloads import T0, make_templates, pcap_capture  # noqa: E402

MSS, MSG = 1448, 1024
U64_MAX = 2**64 - 1


def timed(fn, reps=20, warm=3):
    ms = []
    for r in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def tcp_stream(eng, n_bytes):
    """n_bytes (a multiple of MSG) of MgenTcpTransport transmit stream, on the device."""
    n = n_bytes // MSG
    tmpl, pool = make_templates(64)
    desc = np.zeros(n, DESC_DTYPE)
    seq = np.arange(n)
    desc["tmpl"], desc["seq_num"], desc["msg_len"] = seq % 64, seq, MSG
    desc["tx_sec"], desc["tx_usec"], desc["flags"] = T0, seq % 1_000_000, 4
    tm, pl = to_device(tmpl), to_device(pool)
    crc = torch.empty(64, dtype=torch.int32, device="cuda")
    eng.pack_prepare(tm, 64, pl, crc)
    total = torch.full((n,), MSG, dtype=torch.int32, device="cuda")
    stream, _ = eng.pack_tcp(tm, crc, to_device(desc), total, n, pl, opts=PACK_CHECKSUM)
    assert stream.numel() == n_bytes, (stream.numel(), n_bytes)
    return stream


def tcp_capture(stream, n, conns, gap_us=1):
    """Ethernet / IPv4 / TCP records around MSS-sized pieces of `stream`: packet i belongs to
    connection i % conns (source 10.1.c>>8.c&255 port 40000, no SYN), which carries the
    conns-th part of the stream.  Returns (file uint8 tensor, record offsets int64 tensor)."""
    dev = stream.device
    row = 16 + 14 + 20 + 20 + MSS
    rows = torch.zeros(n, row, dtype=torch.uint8, device=dev)
    h = bytearray(70)
    h[8:12] = (row - 16).to_bytes(4, "little")
    h[12:16] = (row - 16).to_bytes(4, "little")
    h[16:22], h[22:28], h[28:30] = bytes([2, 0, 0, 0, 0, 2]), bytes([2, 0, 0, 0, 0, 1]), b"\x08\0"
    h[30:42] = bytes([0x45, 0, (40 + MSS) >> 8, (40 + MSS) & 255, 0, 0, 0x40, 0, 64, 6, 0, 0])
    h[42:46], h[46:50] = bytes([10, 1, 0, 0]), bytes([127, 0, 0, 1])
    h[50:54] = (40000).to_bytes(2, "big") + (5000).to_bytes(2, "big")
    h[62], h[63] = 0x50, 0x18
    rows[:, :70] = torch.tensor(list(h), dtype=torch.uint8, device=dev)
    i = torch.arange(n, dtype=torch.int64, device=dev)
    c, k = i % conns, i // conns
    t = T0 * 10**6 + i * gap_us
    seq = (0xFFF00000 + k * MSS) & 0xFFFFFFFF
    for b in range(4):
        rows[:, b] = (((t // 10**6) >> (8 * b)) & 255).to(torch.uint8)
        rows[:, 4 + b] = (((t % 10**6) >> (8 * b)) & 255).to(torch.uint8)
        rows[:, 54 + b] = ((seq >> (8 * (3 - b))) & 255).to(torch.uint8)
    rows[:, 44], rows[:, 45] = (c >> 8).to(torch.uint8), (c & 255).to(torch.uint8)
    rows[:, 70:] = stream.view(conns, n // conns, MSS).transpose(0, 1).reshape(n, MSS)
    gh = torch.tensor(list((0xA1B2C3D4).to_bytes(4, "little") + (2).to_bytes(2, "little") +
                           (4).to_bytes(2, "little") + bytes(8) + (65535).to_bytes(4, "little") +
                           (1).to_bytes(4, "little")), dtype=torch.uint8, device=dev)
    return torch.cat([gh, rows.view(-1)]), (24 + i * row).contiguous()


def tcp_run(eng, stream, n, conns, serial_route):
    from mgen_amd import LOG_NO_DATA, OPT_TCP, TEXT_OWNER
    file, pkt_off = tcp_capture(stream, n, conns)
    fb = file.numel()
    toff = (fb + 15) & ~15
    buf = torch.zeros(toff + fb, dtype=torch.uint8, device=file.device)
    buf[:fb] = file
    del file
    s = {}

    def parse():
        s["p"] = eng.pcap_parse(buf, pkt_off, n, 1, 0)

    def tcp():
        fits, s["st"], s["streams"], s["pe"], s["pp"] = eng.pcap_tcp(
            buf, toff, pkt_off, n, 1, 0, s["p"], stream_cap=conns, out=s.get("out"))
        assert fits
        s["out"] = (s["streams"], s["pe"], s["pp"])

    def frame(long_bytes=0):
        st = s["st"]
        s["r"], _, s["k"] = eng.tcp_frame(buf, s["streams"], int(st.n_streams), s["pe"], s["pp"],
                                          int(st.n_pieces), s["p"]["rx_sec"], s["p"]["rx_usec"],
                                          long_bytes=long_bytes, cap=stream.numel() // MSG)

    def unpack():
        r = s["r"]
        s["cols"] = eng.unpack(buf, s["k"], rec_off=r["rec_off"], rec_len=r["rec_len"],
                               opts=OPT_TCP, ext=True)

    def log():
        r = s["r"]
        s["text"], s["line"] = eng.log_recv_text(buf, s["k"], s["cols"], r["rec_src"],
                                                 r["rx_sec"], r["rx_usec"], rec_off=r["rec_off"],
                                                 protocol=2, opts=LOG_NO_DATA,
                                                 text_cap=s["k"] * 200)

    def interleave():
        eng.text_interleave([(TEXT_OWNER, s["text"], s["line"], s["k"], s["r"]["rec_pkt"], 1)], n,
                            cap=s["text"].numel())

    print(f"--- {conns} connection(s): {n} segments, file {fb / 1e6:.0f} MB, stream "
          f"{stream.numel() / 1e6:.0f} MB", flush=True)
    parse()
    stages = {}
    for name, fn in (("parse", parse), ("pcap_tcp", tcp), ("tcp_frame", frame),
                     ("unpack", unpack), ("log_recv_text", log), ("interleave", interleave)):
        stages[name] = timed(fn)
        print(f"{name:14s} {stages[name]:9.3f} ms", flush=True)
    st = s["st"].as_dict()
    assert st["n_streams"] == conns and st["n_gap_streams"] == 0 and st["n_stale"] == 0, st
    assert st["scratch_bytes"] == stream.numel() and s["k"] == stream.numel() // MSG, (st, s["k"])
    print(f"frame, parallel scan per stream (long_bytes 1): {timed(lambda: frame(1), 5, 1):.3f} "
          "ms", flush=True)
    if serial_route:
        print(f"frame, one lane per stream (long_bytes 2^64-1): "
              f"{timed(lambda: frame(U64_MAX), 5, 1):.3f} ms", flush=True)
    p = Pcap2Mgen(eng, tcp=True)
    ms = timed(lambda: p.run_device(buf, pkt_off, n, 1, 0, tcp_off=toff), reps=10)
    algo = fb + 3 * stream.numel()
    print(f"whole pipeline with tcp: {ms:.3f} ms, {algo / ms / 1e6:.1f} GB/s over {algo / 1e6:.0f} "
          f"MB of algorithmic bytes ({p.last_tcp_records} records)", flush=True)
    return ms


def udp_run(eng, n):
    buf, pkt_off, _ = pcap_capture(eng, n)
    p = Pcap2Mgen(eng)
    ms = timed(lambda: p.run_device(buf, pkt_off, n, 1, 0), reps=20)
    print(f"UDP pipeline, {n} packets of 262-B messages, analytics off: {ms:.3f} ms", flush=True)
    return ms


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    n = 1 << 14 if mode == "--small" else 1 << 20
    eng = Engine(0)
    if mode == "--udp-only":
        udp_run(eng, n)
        return
    stream = tcp_stream(eng, n * MSS)
    one = tcp_run(eng, stream, n, 1, serial_route=mode == "--small")
    conns = 64 if mode == "--small" else 1024   # each share a whole number of messages
    many = tcp_run(eng, stream, n, conns, serial_route=True)
    print(f"one connection / {conns} connections: {one / many:.2f}", flush=True)
    udp = udp_run(eng, n)
    print(f"tcp ({conns} connections) / udp, per packet: {many / udp:.2f}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
