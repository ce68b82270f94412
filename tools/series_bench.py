#!/usr/bin/env python3
"""Time tcbee_flow_series_device (DESIGN.md "Per-flow series") with HIP events.

Per shape (those of tools/group_bench.py; a flow's seq rises with occasional steps back):
the call with every output, with `mark` only and with `stats` only, each warmed up and
then timed call by call; the bytes-per-record model of the design (reduce 8 B, apply
19 B in and 17 B out with all outputs) as a fraction of 8 TB/s; and the result at the
timed size compared in full with numpy (the definitions of include/tcbee_amd.h, all
segments at once). Writes one JSON file (default profiles/flow_series.json). Needs a
GPU: no fallback.
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
from tcbee_amd.series import STATS_DTYPE  # noqa: E402
from tools.group_bench import SHAPES, make_ids, time_calls  # noqa: E402

PEAK_BPS = 8e12
# bytes per record: seq + ack in the reduce; seq + ack (+ ts 8, window 2, flags 1 for
# stats) into the apply; seq_rel 8 + ack_rel 8 + mark 1 out of it
CALLS = {"all_outputs": (("seq_rel", "ack_rel", "mark", "stats"), 8 + 19 + 17),
         "mark_only": (("mark",), 8 + 8 + 1),
         "stats_only": (("stats",), 8 + 19)}


def reference(fs, col):
    """Every segment at once. rel: the running sum of the differences minus its value at
    the segment's head. hwm: a running maximum cannot be restarted per segment, so each
    segment is lifted just above the one before it (by offsets from the segments' own
    minima and maxima), one maximum.accumulate runs over everything, and the lift is
    taken off again; all of it exact in int64."""
    n, n_ids = int(fs[-1]), len(fs) - 2
    some = np.flatnonzero(fs[1:] > fs[:-1])
    start = fs[:-1][some].astype(np.int64)
    lens = (fs[1:][some] - fs[:-1][some]).astype(np.int64)
    head = np.zeros(n, bool)
    head[start] = True
    stats = np.zeros(n_ids + 1, STATS_DTYPE)
    stats["win_min"] = 0xFFFF
    out = {"mark": (head * 8).astype(np.uint8), "stats": stats}
    if n == 0:
        return dict(out, seq_rel=np.zeros(0, np.int64), ack_rel=np.zeros(0, np.int64))
    for x, bit in (("seq", 1), ("ack", 2)):
        d = np.diff(col[x], prepend=col[x][:1]).astype(np.int32).astype(np.int64)
        d[head] = 0
        c = np.cumsum(d)
        rel = c - np.repeat(c[start], lens)
        lo, hi = np.minimum.reduceat(rel, start), np.maximum.reduceat(rel, start)
        lift = np.repeat(np.concatenate([[0], np.cumsum(hi[:-1] - lo[1:])]), lens)
        hwm = np.maximum.accumulate(rel + lift) - lift
        below = np.concatenate([[False], rel[1:] < hwm[:-1]]) & ~head
        out["mark"] |= (below * bit).astype(np.uint8)
        out[x + "_rel"] = rel
        stats[x + "_span"][some] = hwm[start + lens - 1]
        stats[f"n_{x}_below"][some] = np.add.reduceat(below.astype(np.int64), start)
    rep = np.concatenate([[False], (col["seq"][1:] == col["seq"][:-1]) &
                          (col["ack"][1:] == col["ack"][:-1])]) & ~head
    out["mark"] |= (rep * 4).astype(np.uint8)
    ts, win = col["ts_ns"], col["window"]
    gap = np.concatenate([[0], np.where(ts[1:] >= ts[:-1], ts[1:] - ts[:-1], 0)]).astype(np.uint64)
    gap[head] = 0
    stats["first_ts_ns"][some], stats["last_ts_ns"][some] = ts[start], ts[start + lens - 1]
    stats["records"][some] = lens
    stats["max_gap_ns"][some] = np.maximum.reduceat(gap, start)
    stats["n_repeat"][some] = np.add.reduceat(rep.astype(np.int64), start)
    stats["n_zero_window"][some] = np.add.reduceat((win == 0).astype(np.int64), start)
    stats["win_min"][some] = np.minimum.reduceat(win, start)
    stats["win_max"][some] = np.maximum.reduceat(win, start)
    stats["flags_or"][some] = np.bitwise_or.reduceat(col["flags"], start)
    return out


def make_columns(torch, n, ids, n_ids, dev):
    """flow_start from the ids' counts (the grouped order itself is not needed), and
    columns as a grouping would leave them: per record a seq step of one segment, now
    and then a step back or none at all; ack rising slowly; time rising; any window."""
    g = torch.Generator(device=dev).manual_seed(4321)
    fs = torch.zeros(n_ids + 2, dtype=torch.int64, device=dev)
    fs[1:n_ids + 1] = torch.cumsum(torch.bincount(ids.to(torch.int64), minlength=n_ids), 0)
    fs[n_ids + 1] = n
    u = torch.randint(0, 64, (n,), generator=g, device=dev)
    seq = torch.cumsum(torch.where(u == 0, -14480, torch.where(u < 3, 0, 1448)), 0).to(torch.int32)
    ack = torch.cumsum((u >= 3) * (u & 1) * 512, 0).to(torch.int32)
    ts = torch.cumsum(torch.randint(1, 2000, (n,), generator=g, device=dev), 0) + 10**18
    window = torch.randint(0, 1 << 16, (n,), generator=g, device=dev)
    window = torch.where(u == 5, 0, window).to(torch.int16)
    flags = torch.randint(0, 64, (n,), generator=g, device=dev, dtype=torch.uint8)
    return fs.to(torch.int32), {"ts_ns": ts, "seq": seq, "ack": ack, "window": window, "flags": flags}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_series.json"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every record count")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch
    if tcbee_amd.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("series_bench: no HIP device")
    dev = torch.device("cuda:0")
    rows = []
    for name, n, n_ids, mix in SHAPES:
        n = max(int(n * a.scale), 1)
        fs, col = make_columns(torch, n, make_ids(torch, n, n_ids, mix, dev), n_ids, dev)
        scratch = torch.empty(tcbee_amd.series_scratch_bytes(n, n_ids), dtype=torch.uint8, device=dev)
        out = {"seq_rel": torch.zeros(n, dtype=torch.int64, device=dev),
               "ack_rel": torch.zeros(n, dtype=torch.int64, device=dev),
               "mark": torch.zeros(n, dtype=torch.uint8, device=dev),
               "stats": torch.zeros((n_ids + 1) * STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)}

        def call(want):
            tcbee_amd.flow_series_device(flow_start=fs, n_max=n, n_ids=n_ids, scratch=scratch,
                                         **col, **{k: out[k] for k in want})

        row = {"shape": name, "records": n, "flows": n_ids, "mix": mix}
        for label, (want, model) in CALLS.items():
            ms = time_calls(torch, lambda: call(want), a.warmup, a.repeats)
            med = statistics.median(ms)
            row[label] = {"ms_per_call": [round(x, 4) for x in ms], "ms_median": round(med, 4),
                          "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                          "model_bytes_per_record": model,
                          "model_fraction_of_8TBps": round(model * n / (med * 1e-3) / PEAK_BPS, 4)}
        # the result at the size that was timed, every output, against numpy
        for v in out.values():
            v.fill_(0x5A)
        call(CALLS["all_outputs"][0])
        torch.cuda.synchronize()
        kinds = {"ts_ns": np.uint64, "seq": np.uint32, "ack": np.uint32, "window": np.uint16,
                 "flags": np.uint8}
        ref = reference(fs.cpu().numpy().view(np.uint32),
                        {k: v.cpu().numpy().view(kinds[k]) for k, v in col.items()})
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["stats"] = got["stats"].view(STATS_DTYPE)
        row["checked"] = all(np.array_equal(got[k], ref[k]) for k in out)
        row["marks"] = {k: int(ref["stats"][k].sum()) for k in ("n_seq_below", "n_ack_below", "n_repeat")}
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k not in CALLS}
                         | {k + "_ms": row[k]["ms_median"] for k in CALLS}), flush=True)
        del fs, col, scratch, out, ref, got
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "tile": tcbee_amd.SERIES_TILE,
           "timing": "HIP events around each tcbee_flow_series_device call",
           "warmup": a.warmup, "repeats": a.repeats, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not all(r["checked"] for r in rows):
        raise SystemExit("series_bench: a result failed its check")


if __name__ == "__main__":
    main()
