"""Peer pairing and join on the device against numpy, written straight from the
definitions in include/tcbee_amd.h: per segment np.searchsorted on perm,
np.maximum.accumulate, then searchsorted(H, s, "right"). Every comparison is exact."""
import numpy as np
import pytest

import tcbee_amd
from tcbee_amd.peer import NO_PEER, PEER_NONE, PEER_STATS_DTYPE, RTT_NONE
from test_gpu_series import reference as series_reference

pytestmark = pytest.mark.gpu
T, S = tcbee_amd.SERIES_TILE, tcbee_amd.PEER_LDS_SLOTS
BIG = 3 * T + 17
SENTINEL = 0x5A
INPUTS = {"perm": np.uint32, "ts_ns": np.uint64, "seq": np.uint32, "ack": np.uint32,
          "window": np.uint16, "seq_rel": np.int64, "mark": np.uint8}
DTYPES = {"una": np.int64, "wnd_edge": np.int64, "rtt_ns": np.uint64, "stats": PEER_STATS_DTYPE}
NEEDS = {"una": (), "wnd_edge": ("window",), "rtt_ns": ("ts_ns", "mark"), "stats": ("ts_ns", "mark")}


def reference(fs, peer, col, n_ids, n):
    """The outputs, and `why`: how many positions each rule of rtt_ns decided."""
    fs = np.minimum(fs.astype(np.int64), n)
    segs = [(k, fs[k], fs[k + 1], fs[peer[k]], fs[peer[k] + 1]) for k in range(n_ids)
            if peer[k] != NO_PEER and fs[k + 1] > fs[k] and fs[peer[k] + 1] > fs[peer[k]]]
    q, H = np.zeros(n, np.int64), np.full(n, PEER_NONE, np.int64)
    for k, a, b, c, d in segs:
        q[a:b] = np.searchsorted(col["perm"][c:d], col["perm"][a:b])
        m = c + np.maximum(q[a:b], 1) - 1
        A = col["seq_rel"][m] + (col["ack"][a:b] - col["seq"][m]).astype(np.int32)
        H[a:b] = np.maximum.accumulate(np.where(q[a:b] > 0, A, PEER_NONE))
    out = {"una": np.full(n, PEER_NONE, np.int64), "wnd_edge": np.full(n, PEER_NONE, np.int64),
           "rtt_ns": np.full(n, RTT_NONE, np.uint64), "stats": np.zeros(n_ids + 1, PEER_STATS_DTYPE)}
    st = out["stats"]
    st["peer"], st["rtt_min_ns"], st["max_outstanding"] = peer, RTT_NONE, PEER_NONE
    why = dict.fromkeys(("sample", "not_eligible", "below_mark", "acked", "no_later_ack"), 0)
    for k, a, b, c, d in segs:
        qq, s, ts = q[a:b], col["seq_rel"][a:b], col["ts_ns"]
        m = c + np.maximum(qq, 1) - 1
        una = np.where(qq > 0, H[m], PEER_NONE)
        has = una != PEER_NONE
        out["una"][a:b] = una
        out["wnd_edge"][a:b] = np.where(has, una + col["window"][m], PEER_NONE)
        grows = np.append(np.diff(col["seq"][a:b]).astype(np.int32) > 0, False)
        below = (col["mark"][a:b] & 1).astype(bool)
        f = np.maximum(np.searchsorted(H[c:d], s, "right"), qq)
        late, fresh = f < d - c, ~has | (una <= s)
        ok = grows & ~below & late & fresh
        tf = ts[c + np.minimum(f, d - c - 1)]
        rtt = np.where(tf >= ts[a:b], tf - ts[a:b], 0)
        out["rtt_ns"][a:b] = np.where(ok, rtt, RTT_NONE)
        for name, hit in (("sample", ok), ("not_eligible", ~grows), ("below_mark", grows & below),
                          ("acked", grows & ~below & late & ~fresh), ("no_later_ack", grows & ~below & ~late)):
            why[name] += int(hit.sum())
        if ok.any():
            st[k]["rtt_samples"], st[k]["rtt_min_ns"] = ok.sum(), rtt[ok].min()
            st[k]["rtt_max_ns"], st[k]["rtt_sum_ns"] = rtt[ok].max(), rtt[ok].sum(dtype=np.uint64)
        if has.any():
            st[k]["max_outstanding"] = (s - una)[has].max()
    return out, why


def talk(fid, peer, n_ids, seed):
    """Columns of a capture whose t-th record belongs to flow fid[t] (n_ids: no id), grouped
    as group_by_flow and series leave them. Hostile on purpose: seq starts at 0xFFFFFF00
    (even flows) or 0x90000000 (odd) and wraps, an opening record's ack is 0, steps back
    (retransmissions), acks that go backwards, ts not monotonic, windows 0 and 0xFFFF."""
    rng = np.random.default_rng(seed)
    n = len(fid)
    nxt = [0xFFFFFF00 if f % 2 == 0 else 0x90000000 for f in range(n_ids + 1)]
    seen = [False] * (n_ids + 1)
    raw = {"seq": np.zeros(n, np.uint32), "ack": np.zeros(n, np.uint32)}
    for t, f in enumerate(fid):
        p, r = (peer[f] if f < n_ids else NO_PEER), rng.random()
        back = 1448 * int(rng.integers(1, 4)) if r < 0.1 and seen[f] else 0
        raw["seq"][t] = (nxt[f] - back) & 0xFFFFFFFF
        if p != NO_PEER and seen[p]:
            raw["ack"][t] = (nxt[p] - (1448 * int(rng.integers(1, 3)) if rng.random() < 0.1 else 0)) & 0xFFFFFFFF
        if not back and r < 0.8:
            nxt[f] += 1448
        seen[f] = True
    raw["ts_ns"] = (10**18 + 1000 * np.arange(n) + rng.integers(-3000, 1000, n)).astype(np.uint64)
    raw["window"] = rng.choice(np.array([0, 1, 502, 0xFFFF], np.uint16), n)
    perm = np.argsort(fid, kind="stable").astype(np.uint32)
    fs = np.concatenate([[0], np.cumsum(np.bincount(fid, minlength=n_ids + 1))]).astype(np.uint32)
    col = {k: v[perm] for k, v in raw.items()}
    ser = series_reference(fs, dict(col, flags=np.zeros(n, np.uint8)), n_ids, n)
    return fs, dict(col, perm=perm, seq_rel=ser["seq_rel"], mark=ser["mark"])


def run_device(fs, peer, col, n_ids, n_max, want):
    """The device call into sentinel-filled buffers; returns them whole, as numpy."""
    import torch
    dev = torch.device("cuda:0")

    def up(a, pad=0):  # the input's bytes, then `pad` elements that must not matter
        a = np.concatenate([a, np.full(pad + 4, 0x77, a.dtype)])
        return torch.from_numpy(a.view(np.uint8).copy()).to(dev)

    need = {"perm", "seq", "ack", "seq_rel"}.union(*(NEEDS[k] for k in want))
    d_in = {k: up(col[k], n_max - len(col[k])) for k in need}
    length = {k: n_ids + 1 if k == "stats" else n_max for k in want}
    out = {k: torch.full((length[k] * np.dtype(DTYPES[k]).itemsize + 16,), SENTINEL,
                         dtype=torch.uint8, device=dev) for k in want}
    scratch = torch.full((tcbee_amd.peer_scratch_bytes(n_max, n_ids),), SENTINEL,
                         dtype=torch.uint8, device=dev)
    tcbee_amd.flow_peer_series_device(flow_start=up(fs), peer=up(peer), n_max=n_max, n_ids=n_ids,
                                      scratch=scratch, **d_in, **out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(fs, peer, col, n_ids, want=tuple(DTYPES)):
    n = len(col["seq"])
    n_max = n + 5                                  # the count comes from flow_start, not n_max
    ref, why = reference(fs, peer, col, n_ids, n)
    got, again = (run_device(fs, peer, col, n_ids, n_max, want) for _ in range(2))
    for k in want:
        assert got[k].tobytes() == again[k].tobytes(), f"{k}: two runs differ"
        m = ref[k].nbytes
        typed = got[k][:m].view(DTYPES[k])
        for f in PEER_STATS_DTYPE.names if k == "stats" else ():
            assert np.array_equal(typed[f], ref[k][f]), f
        assert np.array_equal(typed, ref[k]), k
        assert (got[k][m:] == SENTINEL).all(), f"{k}: written past n"
    return ref, why


def two_flows(la, lb, order, seed):
    """Flow 0 with la records and its mirror flow 1 with lb, in this capture order."""
    fid = np.concatenate([np.zeros(la, np.int64), np.ones(lb, np.int64)])
    if order == "mixed":
        np.random.default_rng(seed).shuffle(fid)
    return fid[::-1].copy() if order == "a_last" else fid


PEER2 = np.array([1, 0, NO_PEER], np.uint32)


@pytest.mark.parametrize("la,lb,order", [
    (1, 1, "mixed"), (1, 0, "mixed"), (63, 65, "mixed"), (T - 1, T + 1, "mixed"), (BIG, 5, "mixed"),
    (5, BIG, "mixed"), (63, 65, "a_first"), (T - 1, T + 1, "a_last")])
def test_join_sizes(gpu, la, lb, order):
    fs, col = talk(two_flows(la, lb, order, la + lb), PEER2, 2, seed=la)
    check(fs, PEER2, col, 2)


@pytest.mark.parametrize("slice_len", [S - 1, S, S + 1, 2 * S + 3])
def test_lds_boundary(gpu, slice_len):
    """Flow 0's first tile: exactly slice_len of the peer's records lie between the
    captures of its first and its last position."""
    inner = np.concatenate([np.zeros(T - 2, np.int64), np.ones(slice_len, np.int64)])
    np.random.default_rng(slice_len).shuffle(inner)
    tail = np.random.default_rng(1).integers(0, 2, 300)
    fs, col = talk(np.concatenate([[1, 1, 1, 0], inner, [0], tail]), PEER2, 2, seed=slice_len)
    check(fs, PEER2, col, 2)


def test_many_tiny_connections(gpu):
    """Segments of 1-3 records, n = T + 1: dozens of segments and peers meet in one tile;
    pairs in both id orders, flows without a peer, empty flows and the trailing group."""
    rng = np.random.default_rng(77)
    n_ids = 1100
    peer = np.full(n_ids + 1, NO_PEER, np.uint32)
    ids = rng.permutation(n_ids)[:1000]
    peer[ids[:450]], peer[ids[450:900]] = ids[450:900], ids[:450]   # ids[900:]: no mirror
    fid = np.repeat(ids, rng.integers(1, 4, len(ids)))[:T - 6]
    fid = rng.permutation(np.concatenate([fid, np.full(T + 1 - len(fid), n_ids)]))
    fs, col = talk(fid, peer, n_ids, seed=78)
    ref, _ = check(fs, peer, col, n_ids)
    assert (ref["una"] != PEER_NONE).sum() > 100


def test_hostile_values_and_every_rule(gpu):
    fid = np.concatenate([[0], two_flows(BIG - 21, 2000, "mixed", 3), np.zeros(20, np.int64)])
    fs, col = talk(fid, PEER2, 2, seed=4)   # (its last records: flow 0's, never acknowledged)
    assert col["seq"][0] == 0xFFFFFF00 and col["ack"][0] == 0 and col["seq"][fs[1]] >= 1 << 31
    assert (np.diff(col["ts_ns"][:fs[1]].astype(np.int64)) < 0).any()
    ref, why = check(fs, PEER2, col, 2)
    assert all(why.values()), why      # a sample, and a position excluded by each rule
    assert (ref["rtt_ns"] == 0).any()  # the clamp of a negative time difference


@pytest.mark.parametrize("want", list(DTYPES))
def test_optional_outputs(gpu, want):
    fs, col = talk(two_flows(BIG, T + 9, "mixed", 5), PEER2, 2, seed=6)
    check(fs, PEER2, col, 2, want=(want,))


def mirror(key):
    m = key.copy()
    m[..., 0:16], m[..., 16:32] = key[..., 16:32], key[..., 0:16]
    m[..., 32:34], m[..., 34:36] = key[..., 34:36], key[..., 32:34]
    return m


@pytest.mark.parametrize("n_ids", [1, 2, 3, 257, 65537])
def test_pairing(gpu, n_ids):
    """v4-form and v6 keys; mirrors, a self-mirrored key, keys that differ from a mirror in
    one port or in the protocol byte only, and keys without a mirror; shuffled ids."""
    import torch
    rng = np.random.default_rng(n_ids)
    base = rng.integers(0, 256, ((n_ids + 1) // 2, 40)).astype(np.uint8)
    base[:, 36:] = [6, 0, 0, 0]
    base[::2, 0:12], base[::2, 16:28] = 0, 0              # every other one in v4 form
    other = mirror(base)
    if n_ids > 2:
        base[1, 16:32], base[1, 34:36] = base[1, 0:16], base[1, 32:34]   # its own mirror
        other[1] = rng.integers(0, 256, 40)
    if n_ids > 100:
        other[2, 32] ^= 1                                 # one port differs
        other[3, 36] = 17                                 # the protocol differs
        other[10:40] = rng.integers(0, 256, (30, 40))     # no mirror
    keys = rng.permutation(np.concatenate([base, other])[:n_ids])
    ent = np.zeros(n_ids, tcbee_amd.FLOW_DTYPE)
    ent["tuple"], ent["pkts"] = keys, rng.integers(1, 99, n_ids)
    ident = {k.tobytes(): i for i, k in enumerate(keys)}
    assert len(ident) == n_ids
    ref = np.array([ident.get(m.tobytes(), NO_PEER) for m in mirror(keys)] + [NO_PEER], np.uint32)
    ref[:n_ids][ref[:n_ids] == np.arange(n_ids)] = NO_PEER
    assert n_ids < 3 or ((ref != NO_PEER).any() and (ref[:n_ids] == NO_PEER).any())
    dev = torch.device("cuda:0")
    got = []
    for _ in range(2):
        peer = torch.full((4 * (n_ids + 1) + 16,), SENTINEL, dtype=torch.uint8, device=dev)
        scratch = torch.full((tcbee_amd.peers_scratch_bytes(n_ids),), SENTINEL, dtype=torch.uint8, device=dev)
        tcbee_amd.flow_peers_device(torch.from_numpy(ent.view(np.uint8).copy()).to(dev), n_ids,
                                    peer=peer, scratch=scratch)
        torch.cuda.synchronize()
        got.append(peer.cpu().numpy())
    assert got[0].tobytes() == got[1].tobytes()
    assert np.array_equal(got[0][:4 * (n_ids + 1)].view(np.uint32), ref)
    assert (got[0][4 * (n_ids + 1):] == SENTINEL).all()


def test_parse_group_series_peers_end_to_end(gpu):
    from tracegen import iperf3_loopback_trace
    with tcbee_amd.PacketParser(device=0, max_frames=1 << 12, max_arena=1 << 22,
                                max_flows=1 << 8) as p:
        res = p.parse(iperf3_loopback_trace(2000), decode=True)
        flows = p.flows()
    g = res.group_by_flow()
    s = g.series()
    pr = s.peers(g, flows)
    assert pr.peer[0] == 1 and pr.peer[1] == 0 and pr.peer[g.n_ids] == NO_PEER
    assert pr.stats["rtt_samples"][0] > 0 and len(pr.flow(0)["una"]) == int(flows["pkts"][0])
    col = dict({k: getattr(g, k) for k in ("perm", "ts_ns", "seq", "ack", "window")},
               seq_rel=s.seq_rel, mark=s.mark)
    ref, why = reference(g.flow_start, pr.peer, col, g.n_ids, res.n)
    assert why["sample"] > 0
    for k in DTYPES:
        assert np.array_equal(getattr(pr, k), ref[k]), k
