"""Text log corpora shared by the CPU and GPU text log ingest tests: the reference manual's own
lines (tests/golden/doc_log_lines.txt) with their hand-written expected values, and a corpus
of malformed and hostile lines for a bounded parser (bad data, not an attempt to break
anything: every line is parsed inside its own bytes)."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL = (b"1700000000.123456 RECV proto>UDP flow>7 seq>42 src>fe80::1:2/4000 dst>10.1.2.3/5000 "
        b"sent>1700000000.100000 size>1024 host>::ffff:1.2.3.4/6000 ttl>64 "
        b"gps>CURRENT,-0.000017,35.500000,-999 data>4:FFFEFFFF flags>0x01 flags>0x02 ")
HEAD = b"1700000000.000001 RECV proto>UDP flow>1 seq>2 src>1.2.3.4/5 dst>6.7.8.9/10 "
TAIL = b"sent>1700000000.000000 size>64 "


def doc_lines() -> bytes:
    with open(os.path.join(ROOT, "tests", "golden", "doc_log_lines.txt"), "rb") as f:
        return f.read()


def v4(a, port):
    return (1, 4, port, bytes(a) + bytes(12))


# hand-written from doc/mgen.xml:2948-2949, 3647-3655, 3661-3662 (fields checked per line)
DOC_EXPECT = [
    dict(event=1, protocol=1, flow=1, seq=0, src=v4([127, 0, 0, 1], 59275),
         dst=v4([127, 0, 0, 1], 5000), size=1024, gps=0, lat_raw=70740000, lon_raw=70740000,
         alt=-999, data=b"\xff\xfe\xff\xff", flags=0, rx_sec=19 * 3600 + 39 * 60 + 6,
         rx_usec=618340, tx_sec=19 * 3600 + 39 * 60 + 6, tx_usec=618199, present=4 | 8),
    dict(event=1, protocol=1, flow=1, seq=1, src=v4([127, 0, 0, 1], 59275), size=1024, gps=0,
         lat_raw=70740000, alt=-999, data=b"\xff\xfe\xff\xff", rx_usec=620218, present=4 | 8),
    dict(event=1, protocol=2, flow=1, seq=1, src=v4([10, 0, 0, 1], 35056),
         dst=v4([10, 0, 0, 2], 5000), size=65535, alt=-999, lat_raw=70740000, flags=0x01,
         present=4 | 16, rx_sec=33 * 60 + 36, tx_sec=36 * 60 + 11),
    dict(event=1, protocol=2, seq=1, size=1024, alt=-999, flags=0x02, present=4 | 16,
         dst=v4([10, 0, 0, 1], 5000)),
    dict(event=3, protocol=2, flow=1, seq=1, size=66559, src=(0, 0, 0, bytes(16)),
         dst=v4([10, 0, 0, 2], 5000), rx_sec=29 * 60 + 51, rx_usec=396962, present=0),
]


def hostile_corpus() -> bytes:
    out = [FULL + b"\n"]
    out += [FULL[:k] + b"\n" for k in range(len(FULL))]             # every truncation
    for c in (b"\0", b">", b" ", b"9"):                              # every byte replaced
        out += [FULL[:k] + c + FULL[k + 1:] + b"\n" for k in range(len(FULL))]
    wide = [b"flow>4294967296", b"flow>00000000001", b"seq>99999999999", b"size>4294967296",
            b"size>4294967295", b"ttl>256", b"ttl>255", b"src>1.2.3.4/65536", b"dst>256.1.1.1/1",
            b"dst>1.2.3/1", b"dst>1.2.3.4.5/1", b"dst>(invalid)/5", b"host>1:2:3:4:5:6:7:8:9/1",
            b"host>1:2:3:4:5:6:7:8/1", b"host>::/0", b"host>1::2::3/1", b"host>12345::1/1",
            b"host>::1.2.3.256/1", b"host>1:2:3:4:5:6:7::/1", b"host>:1:2:3:4:5:6:7/1",
            b"data>65536:00", b"data>2:FFF", b"data>2:FFFFF", b"data>1:GG", b"data>0:",
            b"data>1:ab", b"data>:", b"data>1", b"flags>0x1", b"flags>0x123", b"flags>0X01",
            b"flags>0xfF", b"gps>CURRENT,1.000000,2.000000", b"gps>BAD,1.000000,2.000000,3",
            b"gps>STALE,1.00000,2.000000,3", b"gps>STALE,-180.000001,2.000000,3",
            b"gps>STALE,-180.000000,71402.711250,4294967295", b"gps>STALE,71402.711259,0.000000,0",
            b"gps>STALE,1.000000,2.000000,-99999999999", b"proto>ICMP", b"bogus>1", b"nokey",
            b">", b"flow>", b"seq>-1", b"sent>24:00:00.000000", b"sent>23:59:59.999999",
            b"sent>12:60:00.000000", b"sent>1.0000000", b"sent>4294967296.000000"]
    out += [HEAD + w + b" " + TAIL + b"\n" for w in wide]
    out += [b"4294967296.000000 RECV " + HEAD[23:] + TAIL + b"\n",
            b"24:00:00.000000 LISTEN proto>UDP port>5000\n",
            b"23:59:59.999999 LISTEN proto>UDP port>5000\n",
            b"19:39:06.617625 START Mgen Version 5.1.1\n",
            b"19:39:06.617625 STARTED\n", b"19:39:06.617625\n", b"19:39:06.617625  \n",
            b" 19:39:06.617625 STOP\n", b"\n", b"\r\n", b"   \n", b"\r\r\n",
            b"1.000000 REPORT proto>UDP flow>1 src>1.2.3.4/5 dst>6.7.8.9/10 window>1.000000\n",
            b"1.000000 RERR type>checksum src>::1/9\n", b"1.000000 RERR type>bogus src>::1/9\n",
            b"1.000000 RERR src>::1/9\n", b"1.000000 RERR type>none src>1.2.3.4/9\r\n",
            b"1.000000 SEND proto>SINK flow>1 seq>2 srcPort>65535 dst>::1/5000 size>9 host>1.2.3.4/1\r\n",
            b"1.000000 SEND proto>TCP flow>1 seq>2 dst>::1/5000 size>9\n",
            HEAD + TAIL + b"\r\n", HEAD + TAIL + b"flow>9 \n", HEAD[:-1] + b"\n"]
    out.append(b"1.000000 RECV " + b"x" * 65536 + b"\n")             # 64 KiB, no key
    out.append(b"y" * 65536 + b"\n")                                 # 64 KiB, no space
    pay = bytes((7 * i + 3) & 0xFF for i in range(8192))
    out.append(HEAD + TAIL + b"data>8192:" + pay.hex().upper().encode() + b" flags>0x10 \n")
    out.append(HEAD + TAIL + b"data>8192:" + pay.hex().encode()[:-1] + b" \n")
    out.append(HEAD + TAIL)                                          # the last line has no LF
    return b"".join(out)


def _addr_ok(t, n):
    return (t == 1 and n == 4) or (t == 2 and n == 16)


def expect_from_fields(fields, slab, offs, src, rx_sec, rx_usec, ttl, proto, opts):
    """What parsing the RECV / RERR lines of these decoded records (the formatter inputs of
    tests/test_gpu_log.py) must give, per record, in logparse_ref.parse_line's terms: only the
    fields the line carries under `opts` (LOG_EPOCH 1, LOG_NO_DATA 2, LOG_NO_GPS 4); the others
    stay at their absent values.  Legacy stamps are times of day."""
    from logparse_ref import blank
    epoch = bool(opts & 1)
    out = []
    for i, f in enumerate(fields):
        r = blank()
        s = src[i]
        r["src"] = (int(s["type"]), int(s["len"]), int(s["port"]),
                    bytes(s["addr"][:s["len"]]) + bytes(16 - int(s["len"])))
        r["rx_sec"] = int(rx_sec[i]) if epoch else int(rx_sec[i]) % 86400
        r["rx_usec"] = int(rx_usec[i])
        r["kind"] = 0 if epoch else 1
        bad = False
        if f["err"]:
            r["event"], r["err"] = 2, int(f["err"])
        else:
            r["event"], r["err"], r["protocol"] = 1, 0, proto
            r["kind"] = 0 if epoch else 3
            r["flow"], r["seq"], r["size"] = int(f["flow_id"]), int(f["seq_num"]), int(f["msg_len"])
            r["tx_sec"] = int(f["tx_sec"]) if epoch else int(f["tx_sec"]) % 86400
            r["tx_usec"] = int(f["tx_usec"])
            bad |= r["tx_usec"] > 999999    # "%06lu" prints 7+ digits: not the grammar's stamp
            dl = int(f["dst_len"])
            bad |= not _addr_ok(int(f["dst_type"]), dl)
            r["dst"] = (int(f["dst_type"]), dl, int(f["dst_port"]),
                        bytes(f["dst_addr"][:dl]) + bytes(16 - min(dl, 16)))
            if f["host_type"] in (1, 2):
                hl = int(f["host_len"])
                bad |= not _addr_ok(int(f["host_type"]), hl)
                r["host"] = (int(f["host_type"]), hl, int(f["host_port"]),
                             bytes(f["host_addr"][:hl]) + bytes(16 - min(hl, 16)))
                r["present"] |= 1
            if ttl[i] >= 0:
                r["ttl"] = int(ttl[i])
                r["present"] |= 2
            if f["gps_status"] <= 2:   # else the reference ends the line after ttl>
                if not opts & 4:
                    r["gps"], r["alt"] = int(f["gps_status"]), int(f["alt"])
                    r["lat_raw"], r["lon_raw"] = int(f["lat_raw"]), int(f["lon_raw"])
                    r["present"] |= 4
                if f["payload_len"] and not opts & 2 and f["payload_type"] == 0:
                    at = int(offs[i]) + int(f["payload_off"])
                    r["data"] = bytes(slab[at:at + int(f["payload_len"])])
                    r["present"] |= 8
                r["flags"] = int(f["flags"]) & 0x13
                r["present"] |= 16 if r["flags"] else 0
        r["status"] = 1 if bad else 0
        out.append(r)
    return out


MATRIX_ROWS = (("udp", 0, 1), ("udp_force", 0x1, 1), ("tcp_force", 0x6, 2), ("udp", 0x7, 3))


def matrix_inputs(oracle, gold, opts):
    """Source addresses, receive times and TTLs as tests/test_gpu_log.py draws them."""
    import numpy as np
    from test_gpu_log import _sources
    n = len(gold["unpack_lens"])
    rng = np.random.default_rng(17 + opts)
    src = _sources(oracle, n, rng)
    rx_sec = rng.integers(1_600_000_000, 1_800_000_000, n, dtype=np.int64).astype(np.uint32)
    rx_usec = rng.integers(0, 1_000_000, n).astype(np.uint32)
    ttl = rng.integers(-1, 256, n).astype(np.int32)
    return src, rx_sec, rx_usec, ttl
