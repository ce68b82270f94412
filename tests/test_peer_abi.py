"""Peer pairing and join entry points, the part that needs no GPU: the scratch formulas
and the argument checks, which come before any device work."""
import ctypes as C

import pytest

import tcbee_amd
from tcbee_amd import _lib


def test_scratch_bytes_nonzero_and_monotonic():
    sb, T = tcbee_amd.peer_scratch_bytes, tcbee_amd.SERIES_TILE
    sizes = [0, 1, 63, T - 1, T, T + 1, 3 * T + 17, 1 << 20, (1 << 31) - 1]
    ids = [1, 2, 3, 255, 65537, 1 << 24]
    for n_ids in ids:
        row = [sb(n, n_ids) for n in sizes]
        assert all(b > 0 for b in row) and row == sorted(row)
        assert row[-2] >= 12 << 20  # q and H of every position at least
    for n in sizes:
        col = [sb(n, n_ids) for n_ids in ids]
        assert col == sorted(col)
    assert sb(1 << 31, 10) == 0 and sb(100, 0) == 0 and sb(100, (1 << 24) + 1) == 0
    pairs = [tcbee_amd.peers_scratch_bytes(n_ids) for n_ids in ids]
    assert pairs == sorted(pairs) and all(b >= 8 * n_ids for b, n_ids in zip(pairs, ids))
    assert tcbee_amd.peers_scratch_bytes(0) == 0 and tcbee_amd.peers_scratch_bytes((1 << 24) + 1) == 0
    assert tcbee_amd.PEER_STATS_DTYPE.itemsize == 40


BUF = (C.c_uint64 * 64)()                      # never touched: every call is refused
P = C.addressof(BUF) + 15 & ~15                # a 16-byte aligned address inside it
N, IDS = 100, 10
INPUTS = ("flow_start", "peer", "perm", "ts_ns", "seq", "ack", "window", "seq_rel", "mark")
OUTPUTS = ("una", "wnd_edge", "rtt_ns", "stats")
GOOD = dict({k: P for k in INPUTS + OUTPUTS}, cin=True, out=True, scratch=P, n_max=N, n_ids=IDS,
            short=0)


@pytest.mark.parametrize("bad", [
    dict(cin=False), dict(out=False), dict(scratch=None),
    *(dict({k: None}) for k in INPUTS),     # (each optional input is wanted by an output here)
    dict(una=None, wnd_edge=None, rtt_ns=None, stats=None),
    dict(n_ids=0), dict(n_ids=(1 << 24) + 1), dict(n_max=1 << 31), dict(short=1),
    *(dict({k: P + 8}) for k in INPUTS[2:] + OUTPUTS[:3] + ("scratch",)),
    dict(flow_start=P + 2), dict(peer=P + 2), dict(stats=P + 4),
], ids=lambda d: "-".join(f"{k}{'' if v is None or v in (0, 1, False) else '!'}"
                          for k, v in d.items()))
def test_join_validates_before_device_work(bad):
    a = dict(GOOD, **bad)
    cin = _lib.PeerIn(*(a[k] for k in INPUTS))
    out = _lib.PeerOut(*(a[k] for k in OUTPUTS))
    # (a limit on n_max / n_ids is the only thing wrong in its case: ample scratch)
    scratch = 1 << 62 if {"n_max", "n_ids"} & set(bad) else \
        tcbee_amd.peer_scratch_bytes(N, IDS) - a["short"]
    rc = tcbee_amd.lib().tcbee_flow_peer_series_device(
        C.byref(cin) if a["cin"] else None, a["n_max"], a["n_ids"],
        C.byref(out) if a["out"] else None, a["scratch"], scratch, None)
    assert rc == _lib.EINVAL


@pytest.mark.parametrize("bad", [dict(ent=None), dict(peer=None), dict(scratch=None), dict(n_ids=0),
                                 dict(n_ids=(1 << 24) + 1), dict(short=1), dict(ent=P + 4),
                                 dict(peer=P + 2), dict(scratch=P + 2)], ids=str)
def test_pairing_validates_before_device_work(bad):
    a = dict(dict(ent=P, peer=P, scratch=P, n_ids=IDS, short=0), **bad)
    scratch = 1 << 62 if "n_ids" in bad else tcbee_amd.peers_scratch_bytes(IDS) - a["short"]
    rc = tcbee_amd.lib().tcbee_flow_peers_device(a["ent"], a["n_ids"], a["peer"], a["scratch"],
                                                 scratch, None)
    assert rc == _lib.EINVAL
