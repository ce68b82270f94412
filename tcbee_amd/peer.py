"""A flow joined with its reverse direction on the device (DESIGN.md "Peer join").

``flow_peers_device`` pairs every flow of a flow table with the flow whose tuple is its
mirror. ``flow_peer_series_device`` then gives, per record of a flow-major batch, the
peer's cumulative acknowledgement in the flow's own ``seq_rel`` frame (``una``), the
upper edge of the peer's advertised window and a round-trip sample, and per flow a row
of RTT statistics and the most bytes outstanding: the series the reference draws from
kernel socket state, rebuilt from the packets. Both run asynchronously on a stream over
buffers the caller owns; ``flow_peer_series`` does the chain from host arrays. The
definitions are in include/tcbee_amd.h.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .parser import FLOW_DTYPE, _ptr

PEER_LDS_SLOTS = 4096          # entries of the peer's slice a tile stages in LDS (kPeerLdsSlots)
NO_PEER = 0xFFFFFFFF           # TCBEE_NO_PEER
PEER_NONE = -(1 << 63)         # TCBEE_PEER_NONE: una / wnd_edge / max_outstanding without a value
RTT_NONE = (1 << 64) - 1       # rtt_ns without a sample

# tcbee_peer_stats, 40 bytes
PEER_STATS_DTYPE = np.dtype([("peer", "<u4"), ("rtt_samples", "<u4"), ("rtt_min_ns", "<u8"),
                             ("rtt_max_ns", "<u8"), ("rtt_sum_ns", "<u8"),
                             ("max_outstanding", "<i8")])
assert PEER_STATS_DTYPE.itemsize == 40


def peers_scratch_bytes(n_ids: int) -> int:
    """Device scratch the pairing of n_ids flows needs."""
    return int(_lib.lib().tcbee_peers_scratch_bytes(C.c_uint64(n_ids)))


def peer_scratch_bytes(n_max: int, n_ids: int) -> int:
    """Device scratch the join of up to n_max records of n_ids flows needs."""
    return int(_lib.lib().tcbee_peer_scratch_bytes(C.c_uint64(n_max), C.c_uint64(n_ids)))


def _nbytes(scratch, default: int) -> int:
    return scratch.numel() * scratch.element_size() if hasattr(scratch, "numel") else default


def flow_peers_device(entries, n_ids: int, *, peer, scratch, stream: int = 0) -> None:
    """Asynchronous pairing of a flow table in HBM (FLOW_DTYPE entries as
    PacketParser.export_device leaves them): peer u32 [n_ids + 1], scratch at least
    peers_scratch_bytes(n_ids) bytes."""
    _lib.check(_lib.lib().tcbee_flow_peers_device(
        _ptr(entries) or None, C.c_uint64(n_ids), _ptr(peer) or None, _ptr(scratch) or None,
        C.c_uint64(_nbytes(scratch, peers_scratch_bytes(n_ids))), C.c_void_p(stream or 0)),
        "tcbee_flow_peers_device")


def flow_peer_series_device(*, flow_start, peer, perm, seq, ack, seq_rel, ts_ns=None, window=None,
                            mark=None, n_max: int, n_ids: int, una=None, wnd_edge=None,
                            rtt_ns=None, stats=None, scratch, stream: int = 0,
                            variants: bool = False) -> None:
    """Asynchronous join over grouped columns already in HBM (tensors, arrays or raw
    addresses): flow_start u32 [n_ids + 2], peer u32 [n_ids + 1], the columns [n_max] and
    16-byte aligned as group_by_flow_device and flow_series_device wrote them (window
    only for wnd_edge; ts_ns and mark only for rtt_ns and stats). Outputs, each optional:
    una / wnd_edge i64 [n_max], rtt_ns u64 [n_max], stats [n_ids + 1] rows of
    PEER_STATS_DTYPE. scratch: at least peer_scratch_bytes(n_max, n_ids) bytes.
    variants=True calls the variants build (A/B of the LDS staging, tools/peer_bench.py)."""
    cin = _lib.PeerIn(_ptr(flow_start) or None, _ptr(peer) or None, _ptr(perm) or None,
                      _ptr(ts_ns) or None, _ptr(seq) or None, _ptr(ack) or None,
                      _ptr(window) or None, _ptr(seq_rel) or None, _ptr(mark) or None)
    out = _lib.PeerOut(_ptr(una) or None, _ptr(wnd_edge) or None, _ptr(rtt_ns) or None,
                       _ptr(stats) or None)
    _lib.check(_lib.lib(variants).tcbee_flow_peer_series_device(
        C.byref(cin), C.c_uint64(n_max), C.c_uint64(n_ids), C.byref(out), _ptr(scratch) or None,
        C.c_uint64(_nbytes(scratch, peer_scratch_bytes(n_max, n_ids))), C.c_void_p(stream or 0)),
        "tcbee_flow_peer_series_device")


@dataclass
class FlowPeers:
    n_ids: int
    flow_start: np.ndarray   # uint32 [n_ids + 2], the grouping's
    peer: np.ndarray         # uint32 [n_ids + 1]: the reverse direction's id or NO_PEER
    una: np.ndarray          # int64 [n]: the peer's cumulative ack in this flow's seq_rel frame
    wnd_edge: np.ndarray     # int64 [n]: una + the peer's advertised window (unscaled)
    rtt_ns: np.ndarray       # uint64 [n]: RTT_NONE without a sample
    stats: np.ndarray        # PEER_STATS_DTYPE [n_ids + 1]

    def flow(self, k: int) -> dict:
        """Flow k's slice of the per-record outputs, its peer and its stats row."""
        lo, hi = int(self.flow_start[k]), int(self.flow_start[k + 1])
        return {"peer": int(self.peer[k]), "una": self.una[lo:hi], "wnd_edge": self.wnd_edge[lo:hi],
                "rtt_ns": self.rtt_ns[lo:hi], "stats": self.stats[k]}


def flow_peer_series(groups, series, flows, device: int = 0) -> FlowPeers:
    """Synchronous pairing and join of a FlowGroups, its FlowSeries and the parser's flow
    table (PacketParser.flows(), at least groups.n_ids entries) on the device."""
    import torch
    n, n_ids = len(groups.seq), groups.n_ids
    ent = np.ascontiguousarray(flows, dtype=FLOW_DTYPE)
    if len(ent) < n_ids:
        raise ValueError(f"{n_ids} flow ids but {len(ent)} flow table entries")
    dev = torch.device("cuda", device)

    def up(a, dt):  # the array's bytes on the device (an empty one still gets an address)
        a = np.ascontiguousarray(a, dtype=dt)
        return torch.from_numpy((a if a.size else np.zeros(16, dt)).view(np.uint8).copy()).to(dev)

    def room(count, itemsize):
        return torch.empty(max(count * itemsize, 16), dtype=torch.uint8, device=dev)

    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        d_peer = room(n_ids + 1, 4)
        flow_peers_device(up(ent[:n_ids].view(np.uint8), np.uint8), n_ids, peer=d_peer,
                          scratch=room(peers_scratch_bytes(n_ids), 1), stream=stream)
        cols = {k: up(getattr(groups, k), dt) for k, dt in
                (("flow_start", np.uint32), ("perm", np.uint32), ("ts_ns", np.uint64),
                 ("seq", np.uint32), ("ack", np.uint32), ("window", np.uint16))}
        cols["seq_rel"], cols["mark"] = up(series.seq_rel, np.int64), up(series.mark, np.uint8)
        out = {"una": room(n, 8), "wnd_edge": room(n, 8), "rtt_ns": room(n, 8),
               "stats": room(n_ids + 1, PEER_STATS_DTYPE.itemsize)}
        flow_peer_series_device(peer=d_peer, n_max=n, n_ids=n_ids, stream=stream,
                                scratch=room(peer_scratch_bytes(n, n_ids), 1), **cols, **out)
        torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    return FlowPeers(n_ids, np.ascontiguousarray(groups.flow_start, dtype=np.uint32),
                     d_peer.cpu().numpy()[:4 * (n_ids + 1)].view(np.uint32),
                     host["una"][:8 * n].view(np.int64), host["wnd_edge"][:8 * n].view(np.int64),
                     host["rtt_ns"][:8 * n].view(np.uint64),
                     host["stats"][:PEER_STATS_DTYPE.itemsize * (n_ids + 1)].view(PEER_STATS_DTYPE))
