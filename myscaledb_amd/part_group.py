"""Part groups: many small resident parts searched in one fused call
(mqvs_part_group_*, include/mqvs.h).

``PartGroup(segments).search(queries, k)`` returns what a
``VectorScanSegment.search`` per part followed by
``merge_shards(..., part_merge=True)`` returns, bit for bit, plus the part
each result came from -- the labelled rows the reference's
getTotalTopSearchResultImpl hands on (MergeTreeBaseSearchManager.cpp:207-297).
``BinaryPartGroup`` is the same over ``BinaryVectorScanSegment`` parts
(FixedString codes, Hamming / Jaccard; mqvs_part_group_search_binary).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import F_DEVICE_PTRS, F_TIMING, check, lib
from .vector_scan import _host_f32, _host_u8, _is_torch, _ptr, metric_id


def set_part_group_rows(rows: int) -> int:
    """Row limit of the fused route (mqvs_set_part_group_rows): parts of more
    rows take the per-part route.  Returns the previous value; 0 only reads it."""
    return int(lib.mqvs_set_part_group_rows(int(rows)))


def set_part_group_binary_rows(rows: int) -> int:
    """Row limit of a binary group's fused route
    (mqvs_set_part_group_binary_rows).  Returns the previous value; 0 only
    reads it."""
    return int(lib.mqvs_set_part_group_binary_rows(int(rows)))


def set_part_group_batch(rows: int, max_nq: int = 0) -> None:
    """The fused batch route (mqvs_set_part_group_batch): calls of nq >= 20
    fuse the parts of at most ``rows`` rows on the fp32 MFMA scan; ``rows`` 0
    turns it off (the default).  ``max_nq`` 0: no cap, else calls of more
    queries take the per-part route."""
    check(lib.mqvs_set_part_group_batch(int(rows), int(max_nq)))


def part_group_batch():
    """(rows, max_nq) of the fused batch route; rows 0 = off."""
    rows, max_nq = ctypes.c_int64(), ctypes.c_int32()
    check(lib.mqvs_part_group_batch(ctypes.byref(rows), ctypes.byref(max_nq)))
    return rows.value, max_nq.value


def last_stats():
    """mqvs_part_group_last_stats of the calling thread as a dict."""
    st = _lib.PartGroupStats()
    check(lib.mqvs_part_group_last_stats(ctypes.byref(st)))
    return {f: getattr(st, f) for f, _ in _lib.PartGroupStats._fields_}


class PartGroup:
    """An ordered list of VectorScanSegments (the part order of the merge).
    The group borrows the segments: keep them alive while it is used."""

    _search_fn = "mqvs_part_group_search"
    _torch_dtype = "float32"
    _host = staticmethod(_host_f32)

    def _width(self):
        return self.d

    def _width_error(self, got):
        return f"query dimension {got} != column dimension {self.d}"

    def __init__(self, segments):
        self.segments = list(segments)
        arr = (ctypes.c_void_p * max(len(self.segments), 1))(*[s._h for s in self.segments])
        h = ctypes.c_void_p()
        check(lib.mqvs_part_group_create(arr, len(self.segments), ctypes.byref(h)))
        self._h = h
        self.metric = self.segments[0].metric
        self.d = self.segments[0].d

    def info(self):
        nparts, rows, d, fus, hbm = (ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32(),
                                     ctypes.c_size_t())
        check(lib.mqvs_part_group_info(self._h, ctypes.byref(nparts), ctypes.byref(rows), ctypes.byref(d),
                                       ctypes.byref(fus), ctypes.byref(hbm)))
        return dict(nparts=nparts.value, rows=rows.value, d=d.value, fusable_parts=fus.value,
                    hbm_bytes=hbm.value)

    def _bitmaps(self, maps, torch_side):
        """per-part packed bitmaps (None entries allowed) -> (host pointer array or None, keep-alive)"""
        if maps is None:
            return None, None
        maps = list(maps)
        if len(maps) != len(self.segments):
            raise _lib.MqvsError(_lib.ERR_BAD_ARGUMENTS, "one bitmap (or None) per part")
        keep = [m if (m is None or torch_side) else _host_u8(m) for m in maps]
        arr = (ctypes.c_void_p * len(keep))(*[None if m is None else _ptr(m).value for m in keep])
        return arr, keep

    def search(self, queries, k, metric=None, filters=None, row_exists=None, timing=False):
        """(part[nq,k] int32, ids[nq,k] int64, dist[nq,k] float32); padding
        slots hold part -1, id -1.  filters / row_exists: one packed LSB-first
        bitmap per part, or None.  Torch CUDA queries: the bitmaps are torch
        CUDA uint8 tensors and the results come back as tensors."""
        m = self.metric if metric is None else metric_id(metric)
        return self._search(queries, k, m, filters, row_exists, timing)

    def _search(self, queries, k, m, filters, row_exists, timing):
        """search() with the C call's fifth argument resolved (the metric id;
        an index group's parameter string)."""
        extra = F_TIMING if timing else 0
        fn = getattr(lib, self._search_fn)
        if _is_torch(queries):
            import torch
            assert queries.is_cuda and queries.is_contiguous() and queries.dtype == getattr(torch, self._torch_dtype)
            if queries.shape[1] != self._width():
                raise _lib.MqvsError(_lib.ERR_LOGICAL, self._width_error(queries.shape[1]))
            nq = queries.shape[0]
            part = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
            ids = torch.empty((nq, k), dtype=torch.int64, device=queries.device)
            dist = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
            fa, keep_f = self._bitmaps(filters, True)
            ea, keep_e = self._bitmaps(row_exists, True)
            check(fn(self._h, _ptr(queries), nq, k, m, fa, ea, _ptr(part), _ptr(ids), _ptr(dist),
                     F_DEVICE_PTRS | extra, None))
            del keep_f, keep_e
            return part, ids, dist
        q = self._host(queries)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        if q.shape[1] != self._width():
            raise _lib.MqvsError(_lib.ERR_LOGICAL, self._width_error(q.shape[1]))
        part = np.empty((nq, k), np.int32)
        ids = np.empty((nq, k), np.int64)
        dist = np.empty((nq, k), np.float32)
        fa, keep_f = self._bitmaps(filters, False)
        ea, keep_e = self._bitmaps(row_exists, False)
        check(fn(self._h, _ptr(q), nq, k, m, fa, ea, _ptr(part), _ptr(ids), _ptr(dist), extra, None))
        del keep_f, keep_e
        return part, ids, dist

    last_stats = staticmethod(last_stats)

    def free(self):
        if self._h:
            check(lib.mqvs_part_group_free(self._h))
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BinaryPartGroup(PartGroup):
    """An ordered list of BinaryVectorScanSegments of one FixedString(N) width
    (mqvs_part_group_search_binary).  ``search`` takes uint8 codes [nq, N]
    (numpy, or a torch CUDA uint8 tensor) and Hamming or Jaccard (default: the
    first segment's metric)."""

    _search_fn = "mqvs_part_group_search_binary"
    _torch_dtype = "uint8"
    _host = staticmethod(_host_u8)

    def __init__(self, segments):
        super().__init__(segments)
        self.nbytes = self.segments[0].nbytes

    def _width(self):
        return self.nbytes

    def _width_error(self, got):
        return f"query length {got} bytes != column FixedString({self.nbytes})"
