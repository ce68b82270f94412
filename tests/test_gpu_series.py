"""Per-flow series analysis on the device against numpy, written straight from the
definitions in include/tcbee_amd.h: per segment, np.diff as int32 -> cumsum in int64 ->
maximum.accumulate; the stats follow from those. Every comparison is exact."""
import numpy as np
import pytest

import tcbee_amd
from tcbee_amd.series import STATS_DTYPE

pytestmark = pytest.mark.gpu
T = tcbee_amd.SERIES_TILE
BIG = 3 * T + 17
SENTINEL = 0x5A
INPUTS = {"ts_ns": np.uint64, "seq": np.uint32, "ack": np.uint32, "window": np.uint16,
          "flags": np.uint8}
DTYPES = {"seq_rel": np.int64, "ack_rel": np.int64, "mark": np.uint8, "stats": STATS_DTYPE}


def reference(fs, col, n_ids, n_max):
    n = min(int(fs[n_ids + 1]), n_max)
    out = {"seq_rel": np.zeros(n, np.int64), "ack_rel": np.zeros(n, np.int64),
           "mark": np.zeros(n, np.uint8), "stats": np.zeros(n_ids + 1, STATS_DTYPE)}
    out["stats"]["win_min"] = 0xFFFF
    for k in range(n_ids + 1):
        a, b = int(fs[k]), int(fs[k + 1])
        if b <= a:
            continue
        s = out["stats"][k]
        mark = np.zeros(b - a, np.uint8)
        mark[0] = 8
        for x, bit in (("seq", 1), ("ack", 2)):
            d = np.diff(col[x][a:b]).astype(np.int32)          # uint32 wraps, then signed
            rel = np.concatenate([[0], np.cumsum(d, dtype=np.int64)])
            hwm = np.maximum.accumulate(rel)
            mark[1:] |= np.where(rel[1:] < hwm[:-1], bit, 0).astype(np.uint8)
            out[x + "_rel"][a:b] = rel
            s[x + "_span"] = hwm[-1]
            s[f"n_{x}_below"] = int((mark & bit).astype(bool).sum())
        rep = (col["seq"][a + 1:b] == col["seq"][a:b - 1]) & (col["ack"][a + 1:b] == col["ack"][a:b - 1])
        mark[1:] |= np.where(rep, 4, 0).astype(np.uint8)
        out["mark"][a:b] = mark
        ts, win = col["ts_ns"][a:b], col["window"][a:b]
        gap = np.where(ts[1:] >= ts[:-1], ts[1:] - ts[:-1], 0)
        s["first_ts_ns"], s["last_ts_ns"], s["records"] = ts[0], ts[-1], b - a
        s["max_gap_ns"] = gap.max() if len(gap) else 0
        s["n_repeat"], s["n_zero_window"] = int(rep.sum()), int((win == 0).sum())
        s["win_min"], s["win_max"] = win.min(), win.max()
        s["flags_or"] = np.bitwise_or.reduce(col["flags"][a:b])
    return out


def run_device(fs, col, n_ids, n_max, want):
    """The device call into sentinel-filled buffers; returns them whole, as numpy."""
    import torch
    dev = torch.device("cuda:0")

    def up(a):  # exactly the input's bytes (an empty one still gets an address)
        return torch.from_numpy((a if a.size else np.zeros(16, a.dtype)).view(np.uint8).copy()).to(dev)

    need_in = INPUTS if "stats" in want else ("seq", "ack")
    d_in = {k: up(col[k]) for k in need_in}
    length = {k: n_ids + 1 if k == "stats" else n_max for k in want}
    out = {k: torch.full((length[k] * np.dtype(DTYPES[k]).itemsize + 16,), SENTINEL,
                         dtype=torch.uint8, device=dev) for k in want}
    scratch = torch.full((tcbee_amd.series_scratch_bytes(n_max, n_ids),), SENTINEL,
                         dtype=torch.uint8, device=dev)
    tcbee_amd.flow_series_device(flow_start=up(fs), n_max=n_max, n_ids=n_ids, scratch=scratch,
                                 **d_in, **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(fs, col, n_ids, want=tuple(DTYPES)):
    n_max = len(col["seq"])
    ref = reference(fs, col, n_ids, n_max)
    got, again = (run_device(fs, col, n_ids, n_max, want) for _ in range(2))
    for k in want:
        assert got[k].tobytes() == again[k].tobytes(), f"{k}: two runs differ"
        m = ref[k].nbytes
        typed = got[k][:m].view(DTYPES[k])
        if k == "stats":
            for f in STATS_DTYPE.names:
                assert np.array_equal(typed[f], ref[k][f]), f
        assert np.array_equal(typed, ref[k]), k
        assert (got[k][m:] == SENTINEL).all(), f"{k}: written past n"


def bounds(lengths, n_ids, trailing=0):
    """flow_start of segments with these lengths, in order, spread over n_ids flows with
    empty ones between them; `trailing` more records in the group without an id."""
    assert len(lengths) <= n_ids
    at = np.sort(np.random.default_rng(len(lengths)).choice(n_ids, len(lengths), replace=False))
    size = np.zeros(n_ids + 1, np.int64)
    size[at] = lengths
    size[n_ids] = trailing
    return np.concatenate([[0], np.cumsum(size)]).astype(np.uint32)


def columns(n, seed):
    """Hostile values: seq starts at 0xFFFFFF00 and wraps, with steps back, steps of
    exactly 0x80000000 and runs of equal seq / ack pairs; ts not monotonic; windows with
    0 and 0xFFFF among them."""
    rng = np.random.default_rng(seed)
    step = rng.choice(np.array([0, 0, 1448, 1448, 1448, -1448 * 5, 0x80000000, 70000], np.int64), (2, n))
    seq = (0xFFFFFF00 + np.cumsum(step[0])).astype(np.uint32)
    ack = (1000 + np.cumsum(step[1] // 2)).astype(np.uint32)
    ts = (10**18 + np.cumsum(rng.integers(-50, 1000, n))).astype(np.uint64)
    window = rng.choice(np.array([0, 1, 502, 0xFFFF], np.uint16), n)
    flags = rng.integers(0, 64, n).astype(np.uint8)
    return {"ts_ns": ts, "seq": seq, "ack": ack, "window": window, "flags": flags}


def random_lengths(n, seed):
    cut = np.unique(np.random.default_rng(seed).integers(0, max(n, 1), max(n // 40, 1)))
    return np.diff(np.concatenate([[0], cut[cut > 0], [n]])) if n else np.array([], np.int64)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, BIG])
def test_sizes(gpu, n):
    lengths = random_lengths(n, n)
    check(bounds(lengths, 2 * len(lengths) + 1), columns(n, n), 2 * len(lengths) + 1)


SHAPES = {
    "one_segment": ([BIG], 1, 0),                      # the carry crosses tiles without a head
    "every_record_alone": ([1] * BIG, 65537, 0),
    "heads_at_tile_edges": ([T - 1, 1, 1, T - 1, BIG - 2 * T - 1, 1], 12, 0),  # T-1, T, T+1, 2T, n-1
    "trailing_group": ([T + 3, 5], 7, BIG - T - 8),
    "count_below_n_max": ([T + 3, 5, 700], 7, 0),
}


@pytest.mark.parametrize("shape", SHAPES)
def test_segment_shapes(gpu, shape):
    lengths, n_ids, trailing = SHAPES[shape]
    check(bounds(lengths, n_ids, trailing), columns(BIG, 5), n_ids)


def test_high_water_mark_survives_whole_tiles(gpu):
    """The maximum lies in the first tile, then seq falls for more than T records: the
    carry-in has hwm > rel across whole tiles, and every later record is below it."""
    col = columns(BIG, 9)
    col["seq"] = np.concatenate([np.arange(100) * 1000, 99000 - np.arange(1, BIG - 99) * 7]).astype(np.uint32)
    check(bounds([BIG], 3), col, 3)


@pytest.mark.parametrize("want", [("mark",), ("stats",), ("seq_rel", "ack_rel")], ids="+".join)
def test_optional_outputs(gpu, want):
    lengths = random_lengths(BIG, 13)
    check(bounds(lengths, 300), columns(BIG, 13), 300, want=want)


def test_parse_group_series_end_to_end(gpu):
    from tracegen import mixed_trace
    tr = mixed_trace(4000, seed=31, n_flows=50)
    with tcbee_amd.PacketParser(device=0, max_frames=1 << 13, max_arena=1 << 24,
                                max_flows=1 << 10) as p:
        res = p.parse(tr, decode=True)
        flows = p.flows()
    g = res.group_by_flow()
    s = g.series()
    assert np.array_equal(s.stats["records"][:len(flows)], flows["pkts"])
    assert s.stats["flags_or"].any() and len(s.flow(1)["mark"]) == int(flows["pkts"][1])
    ref = reference(g.flow_start, {k: getattr(g, k) for k in INPUTS}, g.n_ids, res.n)
    for k in DTYPES:
        assert np.array_equal(getattr(s, k), ref[k]), k
