"""Reassembly timing: about 1M packets that are the IPv4 fragments of
8192-byte MGEN messages in 1024 flows at MTU 1500 (6 fragments per message), device-resident.

  python scripts/pcap_defrag_time.py            the defrag stage and the whole pipeline with
                                                 `reassemble`, beside the unfragmented 1M-packet
                                                 capture of scripts/pcap_time.py
  python scripts/pcap_defrag_time.py --profile   a few defrag calls only, for one
      `rocprofv3 --kernel-trace --stats -- python scripts/pcap_defrag_time.py --profile`
  python scripts/pcap_defrag_time.py --default   the default pipeline (no reassembly) once over
      the fragmented capture, for a kernel trace that shows no defrag kernel in it

Device events (torch.cuda.Event), median of 20 after 3 warm-ups; every output is allocated
before the timed region except what run_device allocates itself."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mgen_amd import PACK_CHECKSUM, Engine, to_device  # noqa: E402
from mgen_amd.pcap import Pcap2Mgen  # noqa: E402
from mgen_amd.workloads import T0, pcap_capture, udp_fixed  # noqa: E402


def frag_capture(eng, n_msgs, msg_len=8192, n_flows=1024, mtu=1500, gap_us=1):
    """The capture of workloads.pcap_capture for large messages, every datagram cut at the MTU:
    (file uint8 tensor, record offsets int64 tensor, fragments per message, payload bytes)."""
    dev = f"cuda:{eng.device}"
    tmpl, pool, d = udp_fixed(n_msgs, msg_len, n_flows)
    d["flags"] = 0
    dt, dp = to_device(tmpl, eng.device), to_device(pool, eng.device)
    crc = torch.empty(n_flows, dtype=torch.int32, device=dev)
    eng.pack_prepare(dt, n_flows, dp, crc)
    L = 8 + msg_len
    slab = torch.empty(n_msgs * msg_len, dtype=torch.uint8, device=dev)
    eng.pack(dt, crc, to_device(d, eng.device), n_msgs, dp, slab, stride=msg_len,
             opts=PACK_CHECKSUM)
    dg = torch.zeros(n_msgs, L, dtype=torch.uint8, device=dev)
    dg[:, 8:] = slab.view(n_msgs, msg_len)
    del slab
    i = torch.arange(n_msgs, dtype=torch.int64, device=dev)
    f = i % n_flows
    ident = (i // n_flows) & 0xFFFF
    sp = 30000 + f
    for at, v in ((0, sp >> 8), (1, sp & 255), (2, 5000 >> 8), (3, 5000 & 255), (4, L >> 8),
                  (5, L & 255)):
        dg[:, at] = v if isinstance(v, int) else v.to(torch.uint8)
    step = (mtu - 20) & ~7
    cuts = list(range(0, L, step))
    sizes = [min(step, L - o) for o in cuts]
    row = sum(50 + s for s in sizes)
    rows = torch.zeros(n_msgs, row, dtype=torch.uint8, device=dev)
    base, rec_off = 0, []
    for k, (o, s) in enumerate(zip(cuts, sizes)):
        h = bytearray(50)
        h[8:12] = (34 + s).to_bytes(4, "little")
        h[12:16] = (34 + s).to_bytes(4, "little")
        h[16:22] = bytes([2, 0, 0, 0, 0, 2])
        h[22:28] = bytes([2, 0, 0, 0, 0, 1])
        h[28:30] = b"\x08\x00"
        frag = (0x2000 if k < len(cuts) - 1 else 0) | o >> 3
        h[30:42] = bytes([0x45, 0, (20 + s) >> 8, (20 + s) & 255, 0, 0, frag >> 8, frag & 255,
                          64, 17, 0, 0])
        h[42:46] = bytes([10, 0, 0, 0])
        h[46:50] = bytes([127, 0, 0, 1])
        rows[:, base:base + 50] = torch.tensor(list(h), dtype=torch.uint8, device=dev)
        t = T0 * 10**6 + (i * len(cuts) + k) * gap_us
        sec, usec = t // 10**6, t % 10**6
        for b in range(4):
            rows[:, base + b] = ((sec >> (8 * b)) & 255).to(torch.uint8)
            rows[:, base + 4 + b] = ((usec >> (8 * b)) & 255).to(torch.uint8)
        rows[:, base + 34] = (ident >> 8).to(torch.uint8)
        rows[:, base + 35] = (ident & 255).to(torch.uint8)
        rows[:, base + 44] = (f >> 8).to(torch.uint8)
        rows[:, base + 45] = (f & 255).to(torch.uint8)
        rows[:, base + 50:base + 50 + s] = dg[:, o:o + s]
        rec_off.append(24 + i * row + base)
        base += 50 + s
    gh = torch.tensor(list((0xA1B2C3D4).to_bytes(4, "little") + (2).to_bytes(2, "little") +
                           (4).to_bytes(2, "little") + bytes(8) + (65535).to_bytes(4, "little") +
                           (1).to_bytes(4, "little")), dtype=torch.uint8, device=dev)
    file = torch.cat([gh, rows.view(-1)])
    return file, torch.stack(rec_off, 1).reshape(-1).contiguous(), len(cuts), n_msgs * L


def timed(fn, before=None, reps=20, warm=3):
    ms = []
    for r in range(warm + reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    eng = Engine(0)
    n_msgs = (1 << 20) // 6
    file, pkt_off, per, payload = frag_capture(eng, n_msgs)
    n, fb = n_msgs * per, file.numel()
    doff = (fb + 15) & ~15
    buf = torch.zeros(doff + fb, dtype=torch.uint8, device=file.device)
    buf[:fb] = file
    del file
    if mode == "--default":
        text, _ = Pcap2Mgen(eng).run_device(buf, pkt_off, n, 1, 0)
        torch.cuda.synchronize()
        print("default pipeline over the fragmented capture:", text.numel(), "log bytes")
        return
    state = {}

    def parse():
        state["p"] = eng.pcap_parse(buf, pkt_off, n, 1, 0)

    def defrag():
        fits, st = eng.pcap_defrag(buf, doff, pkt_off, n, 1, 0, state["p"])
        assert fits
        state["st"] = st

    if mode == "--profile":
        for _ in range(5):
            parse()
            defrag()
        torch.cuda.synchronize()
        print(state["st"].as_dict())
        return
    ms = timed(defrag, before=parse)
    st = state["st"].as_dict()
    print(f"capture: {n} packets, {fb / 1e6:.0f} MB, {st}", flush=True)
    print(f"defrag stage {ms:.3f} ms ({payload / ms / 1e6:.1f} GB/s of fragment payload over "
          "the whole stage)", flush=True)
    print(f"parse {timed(parse):.3f} ms", flush=True)
    for an in (False, True):
        p = Pcap2Mgen(eng, analytics=an, window=0.25, reassemble=True)
        ms = timed(lambda: p.run_device(buf, pkt_off, n, 1, 0, file_bytes=fb, defrag_off=doff),
                   reps=10)
        print(f"whole pipeline, reassemble, analytics {'on' if an else 'off'}: {ms:.3f} ms "
              f"({n_msgs} messages)", flush=True)
    del buf
    n1 = 1 << 20
    b1, o1, _ = pcap_capture(eng, n1)
    p = Pcap2Mgen(eng, analytics=True, window=0.25)
    print(f"unfragmented 1M packets of 262-B messages, analytics on: "
          f"{timed(lambda: p.run_device(b1, o1, n1, 1, 0), reps=10):.3f} ms", flush=True)


if __name__ == "__main__":
    main()
