"""Per-flow TCP series analysis on the device (DESIGN.md "Per-flow series").

Over the flow-major columns ``group_by_flow_device`` leaves in HBM: seq / ack unwrapped
relative to each flow's first record of the batch, the marks (below the high-water
mark, repeated seq/ack pair, first of its flow) and one summary row per flow — the
seq/ack plot, retransmission and window analysis the reference's visualiser computes
point by point on one host core. ``flow_series_device`` runs asynchronously on a stream;
``flow_series`` does the same from host arrays. One batch at a time: a flow's state is
not carried from one batch to the next.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .parser import _ptr

SERIES_TILE = 2048   # positions per workgroup (kSerTile, tcbee_series.hip)

MARK_SEQ_BELOW, MARK_ACK_BELOW, MARK_REPEAT, MARK_FIRST = 1, 2, 4, 8

# tcbee_flow_stats, 72 bytes
STATS_DTYPE = np.dtype([("first_ts_ns", "<u8"), ("last_ts_ns", "<u8"), ("seq_span", "<i8"),
                        ("ack_span", "<i8"), ("max_gap_ns", "<u8"), ("records", "<u4"),
                        ("n_seq_below", "<u4"), ("n_ack_below", "<u4"), ("n_repeat", "<u4"),
                        ("n_zero_window", "<u4"), ("win_min", "<u4"), ("win_max", "<u4"),
                        ("flags_or", "<u4")])
assert STATS_DTYPE.itemsize == 72


def series_scratch_bytes(n_max: int, n_ids: int) -> int:
    """Device scratch the analysis of up to n_max records of n_ids flows needs."""
    return int(_lib.lib().tcbee_series_scratch_bytes(C.c_uint64(n_max), C.c_uint64(n_ids)))


def flow_series_device(*, flow_start, seq, ack, ts_ns=None, window=None, flags=None, n_max: int,
                       n_ids: int, seq_rel=None, ack_rel=None, mark=None, stats=None, scratch,
                       stream: int = 0) -> None:
    """Asynchronous analysis of grouped columns already in HBM (tensors, arrays or raw
    addresses). flow_start: u32 [n_ids + 2]; the columns: [n_max], 16-byte aligned, as
    group_by_flow_device wrote them (ts_ns, window and flags only for stats). Outputs,
    each optional: seq_rel / ack_rel i64 [n_max], mark u8 [n_max], stats
    [n_ids + 1] rows of STATS_DTYPE. scratch: at least series_scratch_bytes(n_max,
    n_ids) bytes."""
    sb = scratch.numel() * scratch.element_size() if hasattr(scratch, "numel") else \
        series_scratch_bytes(n_max, n_ids)
    cin = _lib.SeriesIn(_ptr(flow_start) or None, _ptr(ts_ns) or None, _ptr(seq) or None,
                        _ptr(ack) or None, _ptr(window) or None, _ptr(flags) or None)
    out = _lib.SeriesOut(_ptr(seq_rel) or None, _ptr(ack_rel) or None, _ptr(mark) or None,
                         _ptr(stats) or None)
    _lib.check(_lib.lib().tcbee_flow_series_device(
        C.byref(cin), C.c_uint64(n_max), C.c_uint64(n_ids), C.byref(out), _ptr(scratch),
        C.c_uint64(sb), C.c_void_p(stream or 0)), "tcbee_flow_series_device")


@dataclass
class FlowSeries:
    n_ids: int
    flow_start: np.ndarray   # uint32 [n_ids + 2], the grouping's
    seq_rel: np.ndarray      # int64 [n]: seq unwrapped, relative to the flow's first record
    ack_rel: np.ndarray      # int64 [n]
    mark: np.ndarray         # uint8 [n]: MARK_* bits
    stats: np.ndarray        # STATS_DTYPE [n_ids + 1]

    def flow(self, k: int) -> dict:
        """Flow k's slice of the per-record outputs and its stats row (k == n_ids: the
        records without an id below n_ids)."""
        lo, hi = int(self.flow_start[k]), int(self.flow_start[k + 1])
        return {"seq_rel": self.seq_rel[lo:hi], "ack_rel": self.ack_rel[lo:hi],
                "mark": self.mark[lo:hi], "stats": self.stats[k]}

    def peers(self, groups, flows, device: int = 0):
        """Each flow joined with its reverse direction (peer.flow_peer_series): groups is
        the FlowGroups this analysis was made from, flows the parser's flow table."""
        from .peer import flow_peer_series
        return flow_peer_series(groups, self, flows, device)


def flow_series(groups, device: int = 0) -> FlowSeries:
    """Synchronous analysis of a FlowGroups (host arrays) on the device."""
    n, n_ids = len(groups.seq), groups.n_ids
    col = {k: np.ascontiguousarray(getattr(groups, k), dtype=dt) for k, dt in
           (("flow_start", np.uint32), ("ts_ns", np.uint64), ("seq", np.uint32),
            ("ack", np.uint32), ("window", np.uint16), ("flags", np.uint8))}
    seq_rel, ack_rel = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    mark = np.empty(n, dtype=np.uint8)
    stats = np.zeros(n_ids + 1, dtype=STATS_DTYPE)
    cin = _lib.SeriesIn(*(col[k].ctypes.data for k, _ in _lib.SeriesIn._fields_))
    out = _lib.SeriesOut(seq_rel.ctypes.data, ack_rel.ctypes.data, mark.ctypes.data,
                         stats.ctypes.data)
    _lib.check(_lib.lib().tcbee_flow_series(device, C.byref(cin), C.c_uint64(n),
                                            C.c_uint64(n_ids), C.byref(out)),
               "tcbee_flow_series")
    return FlowSeries(n_ids, col["flow_start"], seq_rel, ack_rel, mark, stats)
