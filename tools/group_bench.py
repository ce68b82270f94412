#!/usr/bin/env python3
"""Time tcbee_group_by_flow_device (DESIGN.md "Grouping by flow") with HIP events.

Per shape: the call with flow_start + perm only (the sort passes and the bounds) and
with every column (plus the gather), each warmed up and then timed call by call; the
bytes-per-record model of the design (20 B per sort pass, 225 B for the gather) as a
fraction of 8 TB/s; and, for scale, numpy's stable argsort of the same ids on the host.
Writes one JSON file (default profiles/group_by_flow.json). Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tcbee_amd  # noqa: E402
from tcbee_amd.group import COLUMNS  # noqa: E402

PEAK_BPS = 8e12
PASS_BYTES, GATHER_BYTES = 20, 225
SHAPES = [("100M x 10k uniform", 100_000_000, 10_000, "uniform"),
          ("100M x 10k zipf(1.1)", 100_000_000, 10_000, "zipf"),
          ("1M x 1 flow", 1_000_000, 1, "uniform"),
          ("100M x 1M uniform", 100_000_000, 1_000_000, "uniform")]


def make_ids(torch, n, n_ids, mix, dev):
    g = torch.Generator(device=dev).manual_seed(1234)
    if mix == "uniform":
        return torch.randint(0, n_ids, (n,), generator=g, device=dev, dtype=torch.int32)
    p = 1.0 / torch.arange(1, n_ids + 1, device=dev, dtype=torch.float64) ** 1.1
    cdf = torch.cumsum(p / p.sum(), 0)
    u = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    return torch.searchsorted(cdf, u).clamp_(max=n_ids - 1).to(torch.int32)


def time_calls(torch, call, warmup, repeats):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_by_flow.json"))
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every record count")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host argsort")
    a = ap.parse_args()
    import torch
    if tcbee_amd.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("group_bench: no HIP device")
    dev = torch.device("cuda:0")
    rows = []
    for name, n, n_ids, mix in SHAPES:
        n = max(int(n * a.scale), 1)
        ids = make_ids(torch, n, n_ids, mix, dev)
        rec = torch.randint(0, 256, (n * 74,), device=dev, dtype=torch.uint8)
        scratch = torch.empty(tcbee_amd.group_scratch_bytes(n, n_ids), dtype=torch.uint8, device=dev)
        fs = torch.zeros(n_ids + 2, dtype=torch.int32, device=dev)
        perm = torch.zeros(n, dtype=torch.int32, device=dev)
        cols = {k: torch.zeros(n * np.dtype(dt).itemsize, dtype=torch.uint8, device=dev)
                for k, dt in COLUMNS.items()}

        def call(c):
            tcbee_amd.group_by_flow_device(rec, ids, None, n, n_ids, flow_start=fs, perm=perm,
                                           scratch=scratch, **c)

        passes = (n_ids.bit_length() + 7) // 8
        row = {"shape": name, "records": n, "flows": n_ids, "mix": mix, "passes": passes}
        for label, c, model in (("sort", {}, passes * PASS_BYTES),
                                ("sort_and_columns", cols, passes * PASS_BYTES + GATHER_BYTES)):
            ms = time_calls(torch, lambda: call(c), a.warmup, a.repeats)
            med = statistics.median(ms)
            row[label] = {"ms_per_call": [round(x, 4) for x in ms], "ms_median": round(med, 4),
                          "ms_min": round(min(ms), 4), "model_bytes_per_record": model,
                          "model_fraction_of_8TBps": round(model * n / (med * 1e-3) / PEAK_BPS, 4)}
        # the result at the size that was timed: bounds end at n, keys ascend, and equal
        # keys keep their input order
        key = ids.to(torch.int64)[perm.to(torch.int64)]
        step_ok = bool(((key[1:] > key[:-1]) | ((key[1:] == key[:-1]) & (perm[1:] > perm[:-1]))).all())
        row["checked"] = step_ok and int(fs[-1]) == n and int(fs[0]) == 0
        del key
        if not a.no_host:
            h = ids.cpu().numpy().view(np.uint32)
            t0 = time.perf_counter()
            hp = np.argsort(h, kind="stable")
            row["host_argsort_stable_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["checked"] = row["checked"] and bool(
                (torch.from_numpy(hp.astype(np.int32)).to(dev) == perm).all())
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if k not in ("sort", "sort_and_columns")}
                         | {"sort_ms": row["sort"]["ms_median"],
                            "all_ms": row["sort_and_columns"]["ms_median"]}), flush=True)
        del ids, rec, scratch, perm, cols
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "tile": tcbee_amd.GROUP_TILE,
           "timing": "HIP events around each tcbee_group_by_flow_device call",
           "warmup": a.warmup, "repeats": a.repeats, "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    if not all(r["checked"] for r in rows):
        raise SystemExit("group_bench: a result failed its check")


if __name__ == "__main__":
    main()
