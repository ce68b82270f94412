"""Group-by-flow entry points, the part that needs no GPU: the scratch formula and the
argument checks, which come before any device work."""
import ctypes as C

import pytest

import tcbee_amd
from tcbee_amd import _lib


def test_scratch_bytes_nonzero_and_monotonic():
    sb = tcbee_amd.group_scratch_bytes
    T = tcbee_amd.GROUP_TILE
    sizes = [0, 1, 63, T - 1, T, T + 1, 3 * T + 17, 1 << 20, (1 << 31) - 1]
    ids = [1, 255, 256, 257, 65535, 65537, 1 << 24]
    for n_ids in ids:
        row = [sb(n, n_ids) for n in sizes]
        assert all(b > 0 for b in row) and row == sorted(row)
        assert row[-2] >= 4 * 4 * (1 << 20)  # two (key, index) pairs of u32
    for n in sizes:
        col = [sb(n, n_ids) for n_ids in ids]
        assert col == sorted(col)


BUF = (C.c_uint64 * 64)()                      # never touched: every call is refused
P = C.addressof(BUF) + 15 & ~15                # a 16-byte aligned address inside it
N, IDS = 100, 10
GOOD = dict(rec=P, ids=P, n_max=N, n_ids=IDS, out=True, flow_start=P, short=0)


@pytest.mark.parametrize("bad", [
    dict(rec=None), dict(ids=None), dict(out=False), dict(flow_start=None),
    dict(n_ids=0), dict(n_ids=(1 << 24) + 1), dict(n_max=1 << 31), dict(short=1),
], ids=lambda d: "-".join(d))
def test_device_call_validates_before_device_work(bad):
    a = dict(GOOD, **bad)
    L = tcbee_amd.lib()
    out = _lib.GroupOut(a["flow_start"], P, P, P, P, P, P, P)
    # (a limit on n_max / n_ids is the only thing wrong in its case: ample scratch)
    scratch = 1 << 62 if {"n_max", "n_ids"} & set(bad) else \
        tcbee_amd.group_scratch_bytes(N, IDS) - a["short"]
    rc = L.tcbee_group_by_flow_device(a["rec"], a["ids"], None, a["n_max"], a["n_ids"],
                                      C.byref(out) if a["out"] else None, P, scratch, None)
    assert rc == _lib.EINVAL
