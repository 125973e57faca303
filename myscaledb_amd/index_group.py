"""Index groups: many binary indexed parts searched in one fused call
(mqvs_index_group_*, include/mqvs.h).

``BinaryIndexGroup(indexes).search(queries, k, params)`` returns what a
``BinaryVectorIndex.search`` per part (an explicit ``nprobe`` cut to the part's
list count) followed by ``merge_shards(..., part_merge=True)`` returns, bit for
bit, plus the part each result came from.
"""
from __future__ import annotations

import ctypes

from . import _lib
from ._lib import check, lib
from .part_group import BinaryPartGroup
from .vector_index import _params


def last_stats():
    """mqvs_index_group_last_stats of the calling thread as a dict."""
    st = _lib.IndexGroupStats()
    check(lib.mqvs_index_group_last_stats(ctypes.byref(st)))
    return {f: getattr(st, f) for f, _ in _lib.IndexGroupStats._fields_}


class BinaryIndexGroup(BinaryPartGroup):
    """An ordered list of BinaryVectorIndex objects of one FixedString(N) width
    (the part order of the merge).  The group borrows the indexes and their
    segments: keep them alive while it is used.  It reads them at every search,
    so a row-ids map set on an index later is honoured."""

    _search_fn = "mqvs_index_group_search_binary"

    def __init__(self, indexes):
        self.indexes = list(indexes)
        self.segments = [ix.segment for ix in self.indexes]
        arr = (ctypes.c_void_p * max(len(self.indexes), 1))(*[ix._h for ix in self.indexes])
        h = ctypes.c_void_p()
        check(lib.mqvs_index_group_create(arr, len(self.indexes), ctypes.byref(h)))
        self._h = h
        self.nbytes = self.segments[0].nbytes

    def info(self):
        nparts, rows, bits, lists, hbm = (ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64(),
                                          ctypes.c_size_t())
        check(lib.mqvs_index_group_info(self._h, ctypes.byref(nparts), ctypes.byref(rows), ctypes.byref(bits),
                                        ctypes.byref(lists), ctypes.byref(hbm)))
        return dict(nparts=nparts.value, rows=rows.value, dim_bits=bits.value, lists=lists.value,
                    hbm_bytes=hbm.value)

    def search(self, queries, k, params=None, filters=None, row_exists=None, timing=False):
        """(part[nq,k] int32, ids[nq,k] int64, dist[nq,k] float32); padding
        slots hold part -1, id -1, FLT_MAX.  params: the search parameters of
        BinaryVectorIndex.search (a dict or "k=v,k=v"); an explicit nprobe is
        cut to each part's list count.  filters / row_exists: one packed
        LSB-first bitmap per part, or None.  Torch CUDA queries: the bitmaps
        are torch CUDA uint8 tensors and the results come back as tensors."""
        return self._search(queries, k, _params(params), filters, row_exists, timing)

    last_stats = staticmethod(last_stats)

    def free(self):
        if self._h:
            check(lib.mqvs_index_group_free(self._h))
            self._h = None
