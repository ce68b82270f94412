"""Per-flow series entry points, the part that needs no GPU: the scratch formula and the
argument checks, which come before any device work."""
import ctypes as C

import pytest

import tcbee_amd
from tcbee_amd import _lib


def test_scratch_bytes_nonzero_and_monotonic():
    sb = tcbee_amd.series_scratch_bytes
    T = tcbee_amd.SERIES_TILE
    sizes = [0, 1, 63, T - 1, T, T + 1, 3 * T + 17, 1 << 20, (1 << 31) - 1]
    ids = [1, 255, 65537, 1 << 24]
    for n_ids in ids:
        row = [sb(n, n_ids) for n in sizes]
        assert all(b > 0 for b in row) and row == sorted(row)
        assert row[-2] >= (1 << 20) // 8  # one head bit per position at least
    for n in sizes:
        col = [sb(n, n_ids) for n_ids in ids]
        assert col == sorted(col)
    assert sb(1 << 31, 10) == 0 and sb(100, 0) == 0 and sb(100, (1 << 24) + 1) == 0
    assert tcbee_amd.STATS_DTYPE.itemsize == 72


BUF = (C.c_uint64 * 64)()                      # never touched: every call is refused
P = C.addressof(BUF) + 15 & ~15                # a 16-byte aligned address inside it
N, IDS = 100, 10
INPUTS = ("flow_start", "ts_ns", "seq", "ack", "window", "flags")
OUTPUTS = ("seq_rel", "ack_rel", "mark", "stats")
GOOD = dict({k: P for k in INPUTS + OUTPUTS}, cin=True, out=True, scratch=P, n_max=N, n_ids=IDS,
            short=0)


@pytest.mark.parametrize("bad", [
    dict(cin=False), dict(out=False), dict(flow_start=None), dict(seq=None), dict(ack=None),
    dict(scratch=None), dict(ts_ns=None), dict(window=None), dict(flags=None),
    dict(seq_rel=None, ack_rel=None, mark=None, stats=None),
    dict(n_ids=0), dict(n_ids=(1 << 24) + 1), dict(n_max=1 << 31), dict(short=1),
    *(dict({k: P + 8}) for k in INPUTS[1:] + OUTPUTS[:3] + ("scratch",)),
], ids=lambda d: "-".join(f"{k}{'' if v is None or v in (0, 1, False) else '!'}"
                          for k, v in d.items()))
def test_device_call_validates_before_device_work(bad):
    a = dict(GOOD, **bad)
    cin = _lib.SeriesIn(*(a[k] for k in INPUTS))
    out = _lib.SeriesOut(*(a[k] for k in OUTPUTS))
    # (a limit on n_max / n_ids is the only thing wrong in its case: ample scratch)
    scratch = 1 << 62 if {"n_max", "n_ids"} & set(bad) else \
        tcbee_amd.series_scratch_bytes(N, IDS) - a["short"]
    rc = tcbee_amd.lib().tcbee_flow_series_device(
        C.byref(cin) if a["cin"] else None, a["n_max"], a["n_ids"],
        C.byref(out) if a["out"] else None, a["scratch"], scratch, None)
    assert rc == _lib.EINVAL

