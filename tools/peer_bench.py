#!/usr/bin/env python3
"""Time tcbee_flow_peers_device and tcbee_flow_peer_series_device (DESIGN.md "Peer join")
with HIP events.

Shapes: those of tools/group_bench.py made bidirectional — half the flows are the mirrors
of the other half, data one way and an ack after every second segment the other, now
and then a retransmission. The columns are what group_by_flow and flow_series leave (the
series call is the real one, and is timed as a yardstick on the same columns). Per shape:
the pairing; the join with every output, with `una` only and with rtt_ns + stats, each
warmed up and then timed call by call; the same with the LDS staging switched off (the
variants build's TCBEE_PEER_NOLDS); and the result at the timed size compared with numpy,
segment by segment from the definitions of include/tcbee_amd.h (every segment, or
--check-segments of them drawn at random when there are more). Writes one JSON file
(default profiles/flow_peer.json). Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tcbee_amd  # noqa: E402
from tcbee_amd.peer import NO_PEER, PEER_NONE, PEER_STATS_DTYPE, RTT_NONE  # noqa: E402
from tcbee_amd.series import STATS_DTYPE  # noqa: E402
from tools.group_bench import SHAPES, make_ids, time_calls  # noqa: E402

CALLS = {"all_outputs": ("una", "wnd_edge", "rtt_ns", "stats"), "una_only": ("una",),
         "rtt_and_stats": ("rtt_ns", "stats")}
KINDS = {"flow_start": np.uint32, "peer": np.uint32, "perm": np.uint32, "ts_ns": np.uint64,
         "seq": np.uint32, "ack": np.uint32, "window": np.uint16, "seq_rel": np.int64,
         "mark": np.uint8, "una": np.int64, "wnd_edge": np.int64, "rtt_ns": np.uint64,
         "stats": PEER_STATS_DTYPE}


def make_columns(torch, n, conns, mix, dev):
    """A capture of `conns` connections: record t belongs to connection cid[t]; inside a
    connection every third record is the reverse direction's ack of all data so far.
    Flow ids: connection c's data direction is c, its reverse c + conns."""
    g = torch.Generator(device=dev).manual_seed(4321)
    cid = make_ids(torch, n, conns, mix, dev).to(torch.int64)
    order = torch.sort(cid, stable=True).indices
    start = torch.zeros(conns + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.cumsum(torch.bincount(cid, minlength=conns), 0)
    rank = torch.empty(n, dtype=torch.int64, device=dev)
    rank[order] = torch.arange(n, device=dev) - start[cid[order]]
    del order
    rev = rank % 3 == 2
    sent = 1000 + 1448 * (rank - rank // 3)            # the data direction's next seq
    u = torch.randint(0, 64, (n,), generator=g, device=dev)
    seq = torch.where(rev, 5000, sent - torch.where(u == 0, 14480, 0)).to(torch.int32)
    ack = torch.where(rev, sent, 5000).to(torch.int32)
    ts = torch.cumsum(torch.randint(1, 2000, (n,), generator=g, device=dev), 0) + 10**18
    window = torch.randint(0, 1 << 16, (n,), generator=g, device=dev).to(torch.int16)
    fid = cid + rev * conns
    del cid, rank, sent, u
    perm = torch.sort(fid, stable=True).indices
    fs = torch.zeros(2 * conns + 2, dtype=torch.int64, device=dev)
    fs[1:2 * conns + 1] = torch.cumsum(torch.bincount(fid, minlength=2 * conns), 0)
    fs[2 * conns + 1] = n
    col = {"perm": perm.to(torch.int32), "ts_ns": ts[perm], "seq": seq[perm], "ack": ack[perm],
           "window": window[perm]}
    return fs.to(torch.int32), col


def make_entries(conns):
    """The flow table of those ids: v4-form tuples, the reverse direction's mirrored."""
    ent = np.zeros(2 * conns, tcbee_amd.FLOW_DTYPE)
    t = ent["tuple"]
    c = np.arange(conns, dtype=np.uint32)
    t[:conns, 12:16] = c.view(np.uint8).reshape(-1, 4)
    t[:conns, 28:32] = [10, 0, 0, 1]
    t[:conns, 32:36] = np.array([40000, 5201], "<u2").view(np.uint8)
    t[conns:, 0:16], t[conns:, 16:32] = t[:conns, 16:32], t[:conns, 0:16]
    t[conns:, 32:34], t[conns:, 34:36] = t[:conns, 34:36], t[:conns, 32:34]
    t[:, 36] = 6
    return ent


def check(h, n_ids, segments):
    """The outputs of these segments against the definitions; h: every array on the host."""
    fs, peer, st = h["flow_start"].astype(np.int64), h["peer"], h["stats"]
    H = {}

    def running(k):  # H of segment k
        if k not in H:
            a, b, c, d = fs[k], fs[k + 1], fs[peer[k]], fs[peer[k] + 1]
            q = np.searchsorted(h["perm"][c:d], h["perm"][a:b])
            m = c + np.maximum(q, 1) - 1
            A = h["seq_rel"][m] + (h["ack"][a:b] - h["seq"][m]).astype(np.int32)
            H[k] = (q, np.maximum.accumulate(np.where(q > 0, A, PEER_NONE)))
        return H[k]

    for k in segments:
        a, b, p = fs[k], fs[k + 1], peer[k]
        row = np.zeros((), PEER_STATS_DTYPE)
        row["peer"], row["rtt_min_ns"], row["max_outstanding"] = p, RTT_NONE, PEER_NONE
        una = np.full(b - a, PEER_NONE, np.int64)
        wnd, rtt = una.copy(), np.full(b - a, RTT_NONE, np.uint64)
        if p != NO_PEER and b > a and fs[p + 1] > fs[p]:
            c, d = fs[p], fs[p + 1]
            (q, _), (_, Hp) = running(k), running(p)
            m = c + np.maximum(q, 1) - 1
            una = np.where(q > 0, Hp[m - c], PEER_NONE)
            has, s = una != PEER_NONE, h["seq_rel"][a:b]
            wnd = np.where(has, una + h["window"][m], PEER_NONE)
            grows = np.append(np.diff(h["seq"][a:b]).astype(np.int32) > 0, False)
            f = np.maximum(np.searchsorted(Hp, s, "right"), q)
            ok = grows & ((h["mark"][a:b] & 1) == 0) & (f < d - c) & (~has | (una <= s))
            tf = h["ts_ns"][c + np.minimum(f, d - c - 1)]
            r = np.where(tf >= h["ts_ns"][a:b], tf - h["ts_ns"][a:b], 0)
            rtt = np.where(ok, r, RTT_NONE)
            if ok.any():
                row["rtt_samples"], row["rtt_min_ns"], row["rtt_max_ns"] = ok.sum(), r[ok].min(), r[ok].max()
                row["rtt_sum_ns"] = r[ok].sum(dtype=np.uint64)
            if has.any():
                row["max_outstanding"] = (s - una)[has].max()
        if not (np.array_equal(h["una"][a:b], una) and np.array_equal(h["wnd_edge"][a:b], wnd) and
                np.array_equal(h["rtt_ns"][a:b], rtt) and st[k] == row):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_peer.json"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every record count")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--check-segments", type=int, default=40000)
    a = ap.parse_args()
    import torch
    if tcbee_amd.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("peer_bench: no HIP device")
    dev = torch.device("cuda:0")

    def room(nbytes):
        return torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)

    def timed(call):
        ms = time_calls(torch, call, a.warmup, a.repeats)
        return {"ms_per_call": [round(x, 4) for x in ms], "ms_median": round(statistics.median(ms), 4),
                "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}

    rows = []
    for name, n, flows, mix in SHAPES:
        n, conns = max(int(n * a.scale), 1), max(flows // 2, 1)
        n_ids = 2 * conns
        fs, col = make_columns(torch, n, conns, mix, dev)
        ent = torch.from_numpy(make_entries(conns).view(np.uint8)).to(dev)
        peer, pscratch = room(4 * (n_ids + 1)), room(tcbee_amd.peers_scratch_bytes(n_ids))
        row = {"shape": name + ", bidirectional", "records": n, "flows": n_ids, "mix": mix}
        row["pairing"] = timed(lambda: tcbee_amd.flow_peers_device(ent, n_ids, peer=peer, scratch=pscratch))
        # the series call on the same columns: the join's inputs, and a yardstick
        flags, ack_rel = room(n), room(8 * n)
        col["seq_rel"], col["mark"] = room(8 * n), room(n)
        sstats, sscratch = room((n_ids + 1) * STATS_DTYPE.itemsize), room(tcbee_amd.series_scratch_bytes(n, n_ids))
        row["series_all_outputs"] = timed(lambda: tcbee_amd.flow_series_device(
            flow_start=fs, seq=col["seq"], ack=col["ack"], ts_ns=col["ts_ns"], window=col["window"],
            flags=flags, n_max=n, n_ids=n_ids, seq_rel=col["seq_rel"], ack_rel=ack_rel,
            mark=col["mark"], stats=sstats, scratch=sscratch))
        del flags, ack_rel, sstats, sscratch
        torch.cuda.empty_cache()
        out = {"una": room(8 * n), "wnd_edge": room(8 * n), "rtt_ns": room(8 * n),
               "stats": room((n_ids + 1) * PEER_STATS_DTYPE.itemsize)}
        scratch = room(tcbee_amd.peer_scratch_bytes(n, n_ids))

        def call(want, variants=False):
            tcbee_amd.flow_peer_series_device(flow_start=fs, peer=peer, n_max=n, n_ids=n_ids,
                                              scratch=scratch, variants=variants, **col,
                                              **{k: out[k] for k in want})

        for label, want in CALLS.items():
            row[label] = timed(lambda: call(want))
        os.environ["TCBEE_PEER_NOLDS"] = "1"
        for label, want in CALLS.items():
            row[label + "_no_lds"] = timed(lambda: call(want, variants=True))
        del os.environ["TCBEE_PEER_NOLDS"]
        for v in out.values():
            v.fill_(0x5A)
        call(CALLS["all_outputs"])
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in dict(col, flow_start=fs, peer=peer, **out).items()}
        h = {k: v.view(np.uint8)[:v.nbytes // np.dtype(KINDS[k]).itemsize * np.dtype(KINDS[k]).itemsize]
             .view(KINDS[k]) for k, v in h.items()}
        h["peer"], h["stats"] = h["peer"][:n_ids + 1], h["stats"][:n_ids + 1]
        segs = np.arange(n_ids + 1)
        if len(segs) > a.check_segments:
            segs = np.random.default_rng(1).choice(segs, a.check_segments, replace=False)
        row["peers_checked"] = bool(np.array_equal(
            h["peer"], np.concatenate([np.arange(conns, n_ids), np.arange(conns), [NO_PEER]])))
        row["checked"] = row["peers_checked"] and check(h, n_ids, segs)
        row["segments_checked"] = len(segs)
        row["rtt_samples"] = int(h["stats"]["rtt_samples"].astype(np.int64).sum())
        rows.append(row)
        print(json.dumps({k: (v["ms_median"] if isinstance(v, dict) else v) for k, v in row.items()}),
              flush=True)
        del fs, col, out, scratch, h, peer, pscratch, ent
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "tile": tcbee_amd.SERIES_TILE,
           "lds_slots": tcbee_amd.PEER_LDS_SLOTS,
           "timing": "HIP events around each call", "warmup": a.warmup, "repeats": a.repeats,
           "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not all(r["checked"] for r in rows):
        raise SystemExit("peer_bench: a result failed its check")


if __name__ == "__main__":
    main()
