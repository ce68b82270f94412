"""The decoded parse (TCBEE_F_DECODE) against a byte-by-byte restatement of its rules
(include/tcbee_amd.h, tcbee_cfg) on `bytes`: records, hashes, first-seen ids, the
flow table and the counters, bit-exact. One frame builder (F), one reference
(ref_frame / ref_parse)."""
from __future__ import annotations

import sqlite3
import struct

import numpy as np
import pytest

import tcbee_amd
from tcbee_amd import _lib, host
from tcbee_amd.parser import FLOW_DTYPE
from tcbee_amd.pipeline import Pipeline
from tcbee_amd.trace import Trace

VLAN, QINQ = 0x8100, 0x88A8


def F(tags=(), v6=False, ihl=5, ver=4, proto=6, frag=0, ext=(), doff=5, fl=0x10, sp=1000,
      dp=2000, et=None, flow=1, pad=0) -> bytes:
    """One Ethernet frame. ext: IPv6 extension headers as (type, 8-B units, bytes 2..3)."""
    b = bytearray(b"\x02" * 12)
    for t in tags:
        b += struct.pack(">HH", t, 100)
    b += struct.pack(">H", et if et is not None else (0x86DD if v6 else 0x0800))
    if v6:
        chain = [e[0] for e in ext] + [proto]
        b += struct.pack(">IHBB", 0x60000000, 0, chain[0], 64)
        b += bytes([0x20, 1] + [flow] * 14) + bytes([0x20, 2] + [flow] * 14)
        for k, (_, units, w23) in enumerate(ext):
            b += bytes([chain[k + 1], units - 1]) + struct.pack(">H", w23) + bytes(8 * units - 4)
    else:
        b += bytes([ver << 4 | ihl, 0, 0, 0, 0, 0]) + struct.pack(">H", frag)
        b += bytes([64, proto, 0, 0, 10, 0, 0, flow, 10, 0, 1, flow]) + b"\x01" * (4 * max(ihl, 5) - 20)
    b += struct.pack(">HHIIBBHH", sp, dp, 0x01020300 + flow, 0x0A0B0C0D, doff << 4, fl, 0x7210,
                     0xBEEF) + bytes(2) + b"\xA5" * pad
    return bytes(b)


def ref_frame(b: bytes, ts: int, fport: int):
    """(record 74 B, key 40 B, l4) of an accepted frame, else None: rules 1-7."""
    be = lambda o, k=2: int.from_bytes(b[o:o + k], "big")
    n = len(b)
    if n < 14:
        return None
    et, l3 = be(12), 14
    for _ in range(2):
        if et not in (VLAN, QINQ):
            break
        if n < l3 + 4:
            return None
        et, l3 = be(l3 + 2), l3 + 4
    if et == 0x0800:
        if n < l3 + 20 or b[l3] >> 4 != 4 or (b[l3] & 15) < 5 or b[l3 + 9] != 6 or be(l3 + 6) & 0x1FFF:
            return None
        l4, sa, da = l3 + 4 * (b[l3] & 15), bytes(12) + b[l3 + 12:l3 + 16], bytes(12) + b[l3 + 16:l3 + 20]
        addr = sa[:11:-1] + da[:11:-1] + bytes(32)       # saddr.to_be() / daddr.to_be()
    elif et == 0x86DD:
        if n < l3 + 40:
            return None
        nh, l4, sa, da = b[l3 + 6], l3 + 40, b[l3 + 8:l3 + 24], b[l3 + 24:l3 + 40]
        addr = bytes(8) + sa + da
        for _ in range(4):
            if nh in (0, 43, 60):
                if n < l4 + 8:
                    return None
                nh, l4 = b[l4], l4 + 8 * (b[l4 + 1] + 1)
            elif nh == 44:
                if n < l4 + 8 or be(l4 + 2) & 0xFFF8:
                    return None
                nh, l4 = b[l4], l4 + 8
            else:
                break
        if nh != 6:
            return None
    else:
        return None
    if l4 + 20 > n or l4 + 20 > 128 or b[l4 + 12] >> 4 < 5:
        return None
    sp, dp = be(l4), be(l4 + 2)
    if fport and fport not in (sp, dp):
        return None
    bits = [(b[l4 + 13] >> k) & 1 for k in (5, 4, 3, 2, 1, 0)]
    rec = struct.pack("<Q", ts) + addr + struct.pack("<HHIIH6BH", sp, dp, be(l4 + 4, 4), be(l4 + 8, 4),
                                                     be(l4 + 14), *bits, be(l4 + 16)) + b"\xff" * 4
    return rec, sa + da + struct.pack("<HHB3x", sp, dp, 6), l4


def ref_parse(tr: Trace, fport=0, direction=0):
    """records [k,74], hashes, first-seen ids, flow table, counters of a batch."""
    recs, ids, hashes, flows = [], [], [], {}
    for i in range(tr.n):
        o, c = int(tr.offset[i]), int(tr.caplen[i])
        r = ref_frame(tr.arena[o:o + c].tobytes(), int(tr.ts_ns[i]), fport)
        if r is None:
            continue
        f = flows.setdefault(r[1], [len(flows), 0, 0, len(recs)])
        f[1] += 1
        f[2] += c
        h = tcbee_amd.flow_hash64(r[1])
        hashes.append((h ^ (h >> 32)) & 0xFFFFFFFF)
        ids.append(f[0])
        recs.append(r[0])
    tab = np.zeros(len(flows), FLOW_DTYPE)
    for key, (j, pk, by, fs) in flows.items():
        tab[j] = (np.frombuffer(key, np.uint8), pk, by, fs)
    k = len(recs)
    ctr = dict(ingress=k * (direction == 0), egress=k * (direction == 1), handled=k, dropped=0)
    return (np.frombuffer(b"".join(recs), np.uint8).reshape(k, 74), np.array(hashes, np.uint32),
            np.array(ids, np.uint32), tab, ctr)


def trace(frames, pad=0) -> Trace:
    """Frames back to back after `pad` bytes: the last frame ends at arena_len."""
    t = Trace.from_frames([bytes(pad)] + list(frames))
    return Trace(t.arena, t.offset[1:], t.caplen[1:], t.ts_ns[1:])


def check(res, table, exp, flows=True):
    rec, fh, fi, tab, ctr = exp
    assert res.n == len(rec) and res.counters == ctr, (res.n, len(rec), res.counters, ctr)
    bad = np.flatnonzero((res.records != rec).any(axis=1))
    assert len(bad) == 0, (bad[:5], res.records[bad[0]].tobytes().hex(), rec[bad[0]].tobytes().hex())
    if flows:
        assert np.array_equal(res.flow_hash, fh) and np.array_equal(res.flow_id, fi)
        assert np.array_equal(table, tab)


def kat_frames():
    """Every case of the rules; each accepted case (no payload: caplen = l4 + 20) is
    followed by its one-byte-short twin. l4 + 20 = 128 / 132 exactly cannot occur
    (l4 = 14 + 4 tags + 40 + 8 k is 2 mod 4 for IPv6, and IPv4 ends at 22 + 60 + 20):
    the nearest frames on either side of the limit stand in, 126 (accepted) and 130."""
    hop, rt, dst, frg = (0, 1, 0), (43, 1, 0), (60, 2, 0), (44, 1, 1)
    cases = [F(), F(tags=(VLAN,)), F(tags=(VLAN, VLAN)), F(v6=True), F(v6=True, tags=(VLAN,)),
             F(v6=True, tags=(QINQ, VLAN)), F(tags=(VLAN,) * 3), F(tags=(QINQ, VLAN), flow=2),
             F(ihl=6), F(ihl=15), F(ihl=15, tags=(VLAN, VLAN)), F(ihl=4), F(ver=6),
             F(frag=0x2000), F(frag=0x2001), F(frag=0x00B9),
             F(v6=True, ext=(hop,)), F(v6=True, ext=(rt,)), F(v6=True, ext=(dst,)),
             F(v6=True, ext=(frg,)), F(v6=True, ext=(hop, rt, dst, frg)),
             F(v6=True, ext=(hop, rt, dst, frg, hop)), F(v6=True, ext=((44, 1, 8),)),
             F(v6=True, proto=50), F(v6=True, ext=(hop,), proto=50), F(doff=4), F(doff=15),
             F(v6=True, tags=(VLAN,), ext=((0, 6, 0),)), F(v6=True, ext=((0, 7, 0),)),
             F(v6=True, ext=((60, 32, 0),), pad=300),
             *[F(fl=1 << k, flow=3) for k in range(6)], F(fl=0x3F, flow=3), F(fl=0xC0, flow=3),
             F(sp=4242), F(dp=4242, v6=True), F(sp=4243, dp=4241),
             F(proto=17), F(et=0x0806), F(tags=(VLAN,), et=0x0806), F(v6=True, proto=17)]
    out = []
    for c in cases:
        out.append(c)
        if ref_frame(c, 0, 0):
            out.append(c[:-1])
    return out + [F(tags=(VLAN,), ihl=7, flow=9)]  # stage-2 bytes end exactly at arena_len


@pytest.mark.gpu
@pytest.mark.parametrize("pad", range(16))
def test_known_answers_at_every_alignment(parser, pad):
    tr = trace(kat_frames(), pad)
    assert int(tr.offset[-1]) + int(tr.caplen[-1]) == len(tr.arena) and int(tr.offset[0]) == pad
    for fport in (0, 4242):
        parser.reset_flows()
        exp = ref_parse(tr, fport)
        assert len(exp[0]) == (30 if fport == 0 else 2)
        check(parser.parse(tr, decode=True, filter_port=fport), parser.flows(), exp)


def mixed(n, seed=7, nflows=300) -> Trace:
    """A third standard, a third VLAN-shifted IHL 5, a third general or rejected."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(n):
        fl = int(rng.integers(nflows))
        kw = dict(flow=fl % 250, sp=1000 + fl, fl=int(rng.integers(64)), pad=int(rng.integers(40)))
        kw.update([{}, {}, {}, dict(tags=(VLAN,)), dict(tags=(QINQ, VLAN)), dict(tags=(VLAN,)),
                   dict(ihl=int(rng.integers(5, 16)), tags=(VLAN,) * int(rng.integers(3))),
                   dict(v6=True, ext=((0, int(rng.integers(1, 4)), 0),) * int(rng.integers(3))),
                   dict(proto=17, v6=bool(rng.integers(2)))][int(rng.integers(9))])
        f = F(**kw)
        frames.append(f[:int(rng.integers(len(f)))] if rng.random() < 0.05 else f)
    return trace(frames, seed % 16)


@pytest.mark.gpu
@pytest.mark.parametrize("n,direction,flows,fpl,withhold", [
    (1, 0, True, None, "0"), (63, 1, True, None, "0"), (64, 0, True, None, "0"),
    (65, 0, False, None, "0"), (513, 1, True, None, "0"), (1025, 0, True, "1", "0"),
    (4099, 0, True, None, "0"), (4099, 0, True, "4", "0"), (4099, 0, True, "2", "3")])
def test_mixed_traces(parser, n, direction, flows, fpl, withhold, monkeypatch):
    """fpl: another tiling (variants build); withhold 3: every third tile never
    publishes, so its successors recount it — by the decoded accept predicate."""
    tr = mixed(n, seed=n)
    exp = ref_parse(tr, 0, direction)
    if fpl is None:
        parser.reset_flows()
        res = parser.parse(tr, decode=True, direction=direction, flows=flows)
        check(res, parser.flows() if flows else None, exp, flows)
        assert parser.status() == 0
        return
    monkeypatch.setenv("TCBEE_FPL", fpl)
    monkeypatch.setenv("TCBEE_TEST_WITHHOLD", withhold)
    with tcbee_amd.PacketParser(max_frames=1 << 13, max_arena=1 << 21, max_flows=1 << 10,
                                variants=True) as p:
        check(p.parse(tr, decode=True), p.flows(), exp)
        assert p.status() == 0


@pytest.mark.gpu
def test_standard_frames_equal_oracle_with_flag_bits(parser, oracle):
    """On frames both modes place alike (untagged, IHL 5, unfragmented, data offset
    >= 5, no extension header) the decoded output is the oracle's with the six flag
    bytes set from frame byte 47 / 67; the same context then parses the trace in the
    default mode. (mixed_trace leaves the IPv4 fragment field random: it is set to DF
    here, or no IPv4 frame would qualify.)"""
    from tracegen import mixed_trace
    tr = mixed_trace(20_000)
    v4 = np.flatnonzero((tr.caplen >= 22) & (tr.arena[tr.offset.astype(np.int64) + 12] == 8))
    tr.arena[tr.offset[v4].astype(np.int64) + 20] = 0x40
    tr.arena[tr.offset[v4].astype(np.int64) + 21] = 0
    keep, fbyte = [], []
    for i in range(tr.n):
        o = int(tr.offset[i])
        r = ref_frame(tr.arena[o:o + int(tr.caplen[i])].tobytes(), 0, 0)
        if r and (int(tr.arena[o + 12]), r[2]) in ((0x08, 34), (0x86, 54)):
            keep.append(i)
            fbyte.append(int(tr.arena[o + r[2] + 13]))
    sub = tr.select(np.array(keep))
    rec, fh, fi, ctr, table = oracle.parse(sub)
    assert len(rec) == len(keep) > 2000 and len(set(fbyte)) > 100
    want = rec.copy()
    want[:, 62:68] = (np.array(fbyte)[:, None] >> np.array([5, 4, 3, 2, 1, 0])) & 1
    parser.reset_flows()
    check(parser.parse(sub, decode=True), parser.flows(), (want, fh, fi, table, ctr))
    parser.reset_flows()
    check(parser.parse(sub), parser.flows(), (rec, fh, fi, table, ctr))


@pytest.mark.gpu
def test_pipe_windows_and_flag_bits(parser):
    tr = mixed(5000, seed=5)
    parser.reset_flows()
    want = parser.parse(tr, decode=True)
    for window in (128, 0):
        with Pipeline(chunk_frames=2048, window=window, max_flows=1 << 10, decode=True) as pipe:
            got = pipe.run(tr)
            assert got.n == want.n and np.array_equal(got.records, want.records)
            assert np.array_equal(got.flow_id, want.flow_id)
    for window in (64, 80):
        with Pipeline(chunk_frames=2048, window=window, max_flows=1 << 10) as pipe:
            with pytest.raises(tcbee_amd.TcbeeError) as e:
                pipe.run(tr, decode=True)
            assert e.value.code == _lib.EINVAL
    fr = _lib.Frames(0, 0, 0, 0, 0, 0)
    cfg = _lib.Cfg(0, 0, 0, 0x4)
    n, ctr = _lib.C.c_uint64(0), _lib.Counters()
    assert parser._L.tcbee_parse_batch(parser._h, _lib.C.byref(fr), _lib.C.byref(cfg), 0,
                                       _lib.C.c_uint64(0), 0, 0, _lib.C.byref(n),
                                       _lib.C.byref(ctr)) == _lib.EINVAL


def test_sink_keeps_the_flag_series_of_decoded_records(tmp_path):
    """SYN, three PSH|ACK data segments and FIN|ACK of one flow, as decoded records:
    the database keeps the series of the flags that occurred and deletes the others."""
    fls = [0x02, 0x18, 0x18, 0x18, 0x11]
    recs = b"".join(ref_frame(F(fl=f), 1000 + i, 0)[0] for i, f in enumerate(fls))
    path = str(tmp_path / "d.sqlite")
    s = host.Sink(path)
    s.packets(recs)
    s.close()
    c = sqlite3.connect(path)
    pts = dict(c.execute("SELECT s.name, COUNT(d.timestamp) FROM time_series s LEFT JOIN "
                         "time_series_data d ON d.time_series_id = s.time_series_id AND "
                         "d.value_boolean = 1 WHERE s.name LIKE 'FLAG_%' GROUP BY s.name"))
    c.close()
    assert pts == {"FLAG_SYN": 1, "FLAG_ACK": 4, "FLAG_PSH": 3, "FLAG_FIN": 1}
