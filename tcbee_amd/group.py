"""Records grouped by flow on the device (DESIGN.md "Grouping by flow").

The parse hands over a packet-major stream: 74-byte records in input order with a
dense flow id beside each. Every per-flow consumer (tcbee-process's time series,
db_writer.rs:51-169, flow_tracker.rs:146-221; a seq/ack plot of one connection)
wants it flow-major. ``group_by_flow_device`` regroups a batch that lives in HBM,
asynchronously on a stream; ``group_by_flow`` does the same from host arrays.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .parser import _ptr

GROUP_TILE = 4096   # records per workgroup of the sort passes (kGroupTile, tcbee_group.hip)

# column name -> dtype, in tcbee_group_out's order after flow_start and perm
COLUMNS = {"ts_ns": np.uint64, "seq": np.uint32, "ack": np.uint32, "window": np.uint16,
           "checksum": np.uint16, "flags": np.uint8}


def group_scratch_bytes(n_max: int, n_ids: int) -> int:
    """Device scratch the grouping of up to n_max records of n_ids flows needs."""
    return int(_lib.lib().tcbee_group_scratch_bytes(C.c_uint64(n_max), C.c_uint64(n_ids)))


def group_by_flow_device(rec, flow_id, n_dev, n_max: int, n_ids: int, *, flow_start, perm=None,
                         ts_ns=None, seq=None, ack=None, window=None, checksum=None, flags=None,
                         scratch, stream: int = 0) -> None:
    """Asynchronous grouping of records already in HBM (tensors, arrays or raw
    addresses). rec: [n_max, 74] bytes, 16-byte aligned; flow_id: u32 [n_max];
    n_dev: device u64 (the parse's out_n) or None for n_max; flow_start: u32
    [n_ids + 2]; perm and the columns: [n_max] or None; scratch: at least
    group_scratch_bytes(n_max, n_ids) bytes. Ids at or past n_ids form the trailing
    group [flow_start[n_ids], flow_start[n_ids + 1])."""
    sb = scratch.numel() * scratch.element_size() if hasattr(scratch, "numel") else \
        group_scratch_bytes(n_max, n_ids)
    out = _lib.GroupOut(_ptr(flow_start) or None, _ptr(perm) or None, _ptr(ts_ns) or None,
                        _ptr(seq) or None, _ptr(ack) or None, _ptr(window) or None,
                        _ptr(checksum) or None, _ptr(flags) or None)
    _lib.check(_lib.lib().tcbee_group_by_flow_device(
        _ptr(rec), _ptr(flow_id), _ptr(n_dev), C.c_uint64(n_max), C.c_uint64(n_ids),
        C.byref(out), _ptr(scratch), C.c_uint64(sb), C.c_void_p(stream or 0)),
        "tcbee_group_by_flow_device")


@dataclass
class FlowGroups:
    n_ids: int
    flow_start: np.ndarray   # uint32 [n_ids + 2]
    perm: np.ndarray         # uint32 [n]: input index of the j-th grouped record
    ts_ns: np.ndarray        # the columns, [n] each, in grouped order
    seq: np.ndarray
    ack: np.ndarray
    window: np.ndarray
    checksum: np.ndarray
    flags: np.ndarray        # bits 5..0 = urg, ack, psh, rst, syn, fin

    def flow(self, k: int) -> dict:
        """Flow k's slice of perm and of every column (k == n_ids: the records
        without an id below n_ids)."""
        lo, hi = int(self.flow_start[k]), int(self.flow_start[k + 1])
        return {name: getattr(self, name)[lo:hi] for name in ("perm", *COLUMNS)}

    def series(self, device: int = 0):
        """The per-flow series analysis of these groups (series.flow_series)."""
        from .series import flow_series
        return flow_series(self, device)


def group_by_flow(records, flow_id, n_ids: int | None = None, device: int = 0) -> FlowGroups:
    """Synchronous grouping of host arrays: records uint8 [n, 74], flow_id uint32 [n].
    n_ids defaults to one past the largest id that can be a flow (below 2^24)."""
    rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, _lib.RECORD_BYTES)
    ids = np.ascontiguousarray(flow_id, dtype=np.uint32)
    n = len(rec)
    if len(ids) != n:
        raise ValueError(f"{n} records but {len(ids)} flow ids")
    if n_ids is None:
        ok = ids[ids < (1 << 24)]
        n_ids = int(ok.max()) + 1 if len(ok) else 1
    fs = np.zeros(n_ids + 2, dtype=np.uint32)
    perm = np.empty(n, dtype=np.uint32)
    cols = {name: np.empty(n, dtype=dt) for name, dt in COLUMNS.items()}
    out = _lib.GroupOut(fs.ctypes.data, perm.ctypes.data,
                        *(cols[name].ctypes.data for name in COLUMNS))
    _lib.check(_lib.lib().tcbee_group_by_flow(
        device, rec.ctypes.data, ids.ctypes.data, C.c_uint64(n), C.c_uint64(n_ids),
        C.byref(out)), "tcbee_group_by_flow")
    return FlowGroups(n_ids, fs, perm, **cols)
