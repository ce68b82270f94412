"""Group-by-flow on the device against numpy: a stable argsort of the clamped ids,
searchsorted bounds, and the record fields at the tcbee_layout.h offsets. Every
comparison is exact."""
import numpy as np
import pytest

import tcbee_amd
from tcbee_amd.group import COLUMNS

pytestmark = pytest.mark.gpu
T = tcbee_amd.GROUP_TILE
BIG = 3 * T + 17
NOID = 0xFFFFFFFF
SENTINEL = 0x5A
OUTPUTS = ("flow_start", "perm", *COLUMNS)
DTYPES = dict(COLUMNS, flow_start=np.uint32, perm=np.uint32)


def reference(rec, ids, n, n_ids):
    key = np.where(ids[:n] < n_ids, ids[:n], n_ids)
    perm = np.argsort(key, kind="stable")
    r = rec[:n][perm]

    def field(lo, hi, dt):
        return np.ascontiguousarray(r[:, lo:hi]).view(dt).ravel()

    return {"flow_start": np.searchsorted(key[perm], np.arange(n_ids + 2)).astype(np.uint32),
            "perm": perm.astype(np.uint32), "ts_ns": field(0, 8, "<u8"),
            "seq": field(52, 56, "<u4"), "ack": field(56, 60, "<u4"),
            "window": field(60, 62, "<u2"), "checksum": field(68, 70, "<u2"),
            "flags": ((r[:, 62:68] != 0) @ np.array([32, 16, 8, 4, 2, 1])).astype(np.uint8)}


def run_device(rec, ids, n_ids, n=None, want=OUTPUTS):
    """The device call on n_max = len(ids) records (n: the device-side count, None = no
    n_dev), into sentinel-filled buffers; returns them whole, as numpy."""
    import torch
    dev = torch.device("cuda:0")
    n_max = len(ids)
    length = {k: n_ids + 2 if k == "flow_start" else n_max for k in want}

    def up(a):  # exactly the input's bytes (an empty one still gets an address)
        return torch.from_numpy(a.ravel().copy() if a.size else np.zeros(16, a.dtype)).to(dev)

    d_rec, d_ids = up(rec[:n_max]), up(ids.view(np.int32))
    d_n = None if n is None else torch.tensor([n], dtype=torch.int64, device=dev)
    out = {k: torch.full((length[k] * np.dtype(DTYPES[k]).itemsize + 16,), SENTINEL,
                         dtype=torch.uint8, device=dev) for k in want}
    scratch = torch.empty(tcbee_amd.group_scratch_bytes(n_max, n_ids), dtype=torch.uint8,
                          device=dev)
    tcbee_amd.group_by_flow_device(d_rec, d_ids, d_n, n_max, n_ids, scratch=scratch, **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(DTYPES[k]) for k, v in out.items()}


def check(rec, ids, n_ids, n=None, want=OUTPUTS):
    n_eff = len(ids) if n is None else min(n, len(ids))
    ref = reference(rec, ids, n_eff, n_ids)
    got, again = (run_device(rec, ids, n_ids, n, want) for _ in range(2))
    for k in want:
        assert got[k].tobytes() == again[k].tobytes(), f"{k}: two runs differ"
        m = len(ref[k])
        assert np.array_equal(got[k][:m], ref[k]), k
        assert (got[k][m:].view(np.uint8) == SENTINEL).all(), f"{k}: written past n"


def random_case(n, n_ids, seed):
    """Random record bytes; ids over about half of the flows (the rest stay empty) with
    0, n_ids - 1, n_ids itself and 0xFFFFFFFF among them when n allows."""
    rng = np.random.default_rng(seed)
    rec = rng.integers(0, 256, (max(n, 1), 74), dtype=np.uint8)
    rec[:, 62:68] *= rng.integers(0, 2, (max(n, 1), 6), dtype=np.uint8)  # some flag bytes 0
    pool = np.unique(np.concatenate([rng.integers(0, n_ids, max(n_ids // 2, 1)),
                                     [0, n_ids - 1, n_ids, NOID]]))
    ids = rng.choice(pool, n).astype(np.uint32)
    ids[:4] = np.array([0, n_ids - 1, n_ids, NOID], dtype=np.uint32)[:n]
    return rec, ids


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, BIG])
def test_sizes(gpu, n):
    check(*random_case(n, 300, seed=n), 300)


@pytest.mark.parametrize("n_ids", [1, 255, 256, 257, 65535, 65537])
def test_pass_counts_and_digit_edges(gpu, n_ids):
    check(*random_case(BIG, n_ids, seed=n_ids), n_ids)


@pytest.mark.parametrize("shape", ["one_flow", "runs_of_64"])
def test_wave_uniform_path(gpu, shape):
    rec, ids = random_case(BIG, 300, seed=7)
    if shape == "one_flow":
        ids[:] = 3
    else:  # 64 equal ids from a wave boundary, and 64 from one record past another
        ids[5 * 64:6 * 64] = 7
        ids[T + 9 * 64 + 1:T + 10 * 64 + 1] = 9
    check(rec, ids, 300)


def test_device_count_below_n_max(gpu):
    check(*random_case(BIG, 300, seed=11), 300, n=BIG // 3)


@pytest.mark.parametrize("want", [("flow_start", *COLUMNS), ("flow_start", "perm"),
                                  ("flow_start",), ("flow_start", "ts_ns"),
                                  ("flow_start", "flags")], ids=lambda w: "+".join(w))
def test_optional_outputs(gpu, want):
    check(*random_case(BIG, 300, seed=13), 300, want=want)


def test_parse_then_group_end_to_end(gpu):
    from tracegen import mixed_trace
    tr = mixed_trace(4000, seed=31, n_flows=50)
    with tcbee_amd.PacketParser(device=0, max_frames=1 << 13, max_arena=1 << 24,
                                max_flows=1 << 10) as p:
        res = p.parse(tr, decode=True)
        flows = p.flows()
    g = res.group_by_flow()
    assert g.n_ids == len(flows) and res.n > 100  # (the decoded parse rejects most frames)
    ref = reference(res.records, res.flow_id, res.n, g.n_ids)
    for k in OUTPUTS:
        assert np.array_equal(getattr(g, k), ref[k]), k
    assert g.flags.any()  # decoded mode: real TCP flag bits reach the column
    for k in (0, 1, len(flows) // 2, len(flows) - 1):
        rows = g.flow(k)
        assert all(len(v) == int(flows["pkts"][k]) for v in rows.values())
        assert (res.flow_id[rows["perm"]] == k).all()
