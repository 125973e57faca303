"""Host-side mirror of MyScaleDB's vector-index seam over libmqvs (index path).

* ``VectorIndex.build``   -- Search::createVectorIndex<..., FloatVector>(name,
  IndexType::MSTG, metric, dim, total_vec, params, ...) + VectorIndex::build
  (src/VectorIndex/Common/VIWithDataPart.cpp:416-447, VIWithDataPart.h:295-339).
* ``VectorIndex.search``  -- VectorIndex::search(queries, k, params,
  first_stage_only, filter) as VIWithColumnInPart::search calls it
  (VIWithDataPart.cpp:858-957; the filter is PREWHERE ∩ the delete bitmap,
  :903-908).
* ``VectorIndex.compute_top_distance_subset`` -- stage 2 of a two-stage
  search, VIWithColumnInPart::computeTopDistanceSubset (VIWithDataPart.cpp:838-856):
  mqvs_rerank on the index's segment.

The MSTG library is absent from the reference snapshot; the index here is the
library's own GPU design with MSTG's parameter surface (``alpha``,
``metric_type``), see include/mqvs.h.  Every call runs HIP kernels; there is
no CPU path.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import F_DEVICE_PTRS, F_FIRST_STAGE, F_RERANK_ALL, check, lib
from .vector_scan import (BinaryVectorScanSegment, VectorScanSegment, _host_f32, _host_u8, _is_torch, _ptr,
                          _staged_search)


def _params(p) -> bytes:
    if p is None:
        return b""
    if isinstance(p, dict):
        p = ",".join(f"{k}={v}" for k, v in p.items())
    return p.encode()


class VectorIndex:
    """An MSTG-type index over a resident segment (the segment must outlive it)."""

    def __init__(self, handle, segment: VectorScanSegment):
        self._h = handle
        self.segment = segment

    @classmethod
    def build(cls, segment: VectorScanSegment, index_type="MSTG", params=None):
        h = ctypes.c_void_p()
        check(lib.mqvs_index_build(segment._h, index_type.encode(), _params(params), ctypes.byref(h)))
        return cls(h, segment)

    def set_row_ids_map(self, row_ids_map):
        """Decoupled part (VIWithMeta::row_ids_map): source-part row -> row of
        the decoupled part; later searches return decoupled-part row ids
        (transferToNewRowIds, VIWithDataPart.cpp:56-67).  None clears it."""
        if row_ids_map is None:
            check(lib.mqvs_index_set_row_ids_map(self._h, None, 0, 0))
            return
        if _is_torch(row_ids_map):
            check(lib.mqvs_index_set_row_ids_map(self._h, _ptr(row_ids_map), row_ids_map.numel(), F_DEVICE_PTRS))
            return
        m = np.ascontiguousarray(row_ids_map, np.uint64)
        check(lib.mqvs_index_set_row_ids_map(self._h, _ptr(m), m.size, 0))

    def info(self):
        st = _lib.IndexInfo()
        check(lib.mqvs_index_info(self._h, ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in _lib.IndexInfo._fields_}

    def plane(self):
        """The list plane (mqvs_index_plane): {"format": 0 bf16 | 1 fp8 (build
        parameter ``plane``), "plane_bytes": its HBM bytes, scale array included}."""
        fmt = ctypes.c_int32()
        nbytes = ctypes.c_size_t()
        check(lib.mqvs_index_plane(self._h, ctypes.byref(fmt), ctypes.byref(nbytes)))
        return {"format": fmt.value, "plane_bytes": nbytes.value}

    def centroids(self):
        """The coarse step's centroid table, float32[nlist, dim]."""
        info = self.info()
        c = np.empty((info["nlist"], info["dim"]), np.float32)
        check(lib.mqvs_index_centroids(self._h, _ptr(c), c.size))
        return c

    def probes(self, queries, params=None):
        """The lists a search with `params` probes, int64[nq, nprobe] (no order)."""
        q = _host_f32(queries)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        pr = _params(params)
        info = self.info()
        # nprobe as the search resolves it: run the coarse step into a buffer
        # of every list, then trim to the count the stats report
        buf = np.full((nq, info["nlist"]), -1, np.int64)
        check(lib.mqvs_index_probes(self._h, _ptr(q), nq, pr, _ptr(buf)))
        npb = _lib.last_index_stats()["nprobe"]
        return buf.reshape(-1)[: nq * npb].reshape(nq, npb).copy()

    def search(self, queries, k, params=None, filter_bitmap=None, row_exists=None, first_stage_only=False,
               out=None, async_=False, stream=None, rerank_all=False, chunk_ord_base=None):
        """(ids[nq,k] int64, dist[nq,k] float32), reference order, -1 padded.
        first_stage_only: the k best rows by the approximate distance (stage 1
        of a two-stage search; re-rank with compute_top_distance_subset).
        rerank_all: re-rank every num_reorder candidate (MQVS_F_RERANK_ALL; the
        default bound pruning gives the same results).
        chunk_ord_base: the index of a row-range shard: how many granule chunks
        before its first row the reference searches (mqvs_index_search_ex;
        sharded.chunk_ordinal_base).  None: row_offset / granule.  Only cosine
        results depend on it."""
        fs = (F_FIRST_STAGE if first_stage_only else 0) | (F_RERANK_ALL if rerank_all else 0)
        pr = _params(params)
        base = -1 if chunk_ord_base is None else int(chunk_ord_base)

        def call(qp, nq, fp, ep, ip, dp, flags, st):
            check(lib.mqvs_index_search_ex(self._h, qp, nq, k, pr, fp, ep, base, ip, dp, flags | fs, st))

        return _staged_search(queries, k, np.float32, self.segment.d,
                              lambda got: "The dimension of searched index and input doesn't match.", filter_bitmap,
                              row_exists, out, async_, stream, call)

    def save(self) -> bytes:
        """The index as one byte string (mqvs_index_save; VIWithColumnInPart::
        serialize): centroids, each row's list, nlist, alpha, np95.  A row-ids
        map is not part of it."""
        size = ctypes.c_size_t()
        check(lib.mqvs_index_save_size(self._h, ctypes.byref(size)))
        buf = np.empty(size.value, np.uint8)
        written = ctypes.c_size_t()
        check(lib.mqvs_index_save(self._h, _ptr(buf), buf.size, ctypes.byref(written)))
        return buf[: written.value].tobytes()

    @classmethod
    def load(cls, segment, blob):
        """The index of a save()d byte string over the resident segment it was
        built on, without a build (mqvs_index_load; VIWithColumnInPart::load)."""
        b = np.frombuffer(bytes(blob), np.uint8)
        h = ctypes.c_void_p()
        check(lib.mqvs_index_load(segment._h, _ptr(b), b.size, ctypes.byref(h)))
        return cls(h, segment)

    def lists(self):
        """(list_off int64[nlist + 1], rows int32[npos]): the part row of every
        list position in position order, -1 = padding (mqvs_index_lists)."""
        info = self.info()
        off = np.empty(info["nlist"] + 1, np.int64)
        rows = np.empty(info["npos"], np.int32)
        check(lib.mqvs_index_lists(self._h, _ptr(off), off.size, _ptr(rows), rows.size))
        return off, rows

    def compute_top_distance_subset(self, queries, first_stage_ids, top_k, row_exists=None):
        """Exact re-rank of stage-1 ids (segment-local rows, -1 = none)."""
        ids = np.asarray(first_stage_ids, np.int64)
        local = np.where(ids >= 0, ids - self.segment.row_offset, -1)
        return self.segment.rerank(queries, local, top_k, row_exists=row_exists)

    def free(self):
        if self._h:
            check(lib.mqvs_index_free(self._h))
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BinaryVectorIndex:
    """A BINARYMSTG-type index over a resident BinaryVectorScanSegment (the
    segment must outlive it): an inverted file over k-majority lists, exact
    Hamming / Jaccard distances (mqvs_index_search_binary, include/mqvs.h)."""

    def __init__(self, handle, segment: BinaryVectorScanSegment):
        self._h = handle
        self.segment = segment

    @classmethod
    def build(cls, segment: BinaryVectorScanSegment, index_type="BINARYMSTG", params=None):
        h = ctypes.c_void_p()
        check(lib.mqvs_index_build(segment._h, index_type.encode(), _params(params), ctypes.byref(h)))
        return cls(h, segment)

    set_row_ids_map = VectorIndex.set_row_ids_map
    info = VectorIndex.info
    save = VectorIndex.save
    load = classmethod(VectorIndex.load.__func__)
    lists = VectorIndex.lists

    def _host_queries(self, queries):
        q = _host_u8(queries)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.segment.nbytes:
            raise _lib.MqvsError(_lib.ERR_LOGICAL,
                                 f"query length {q.shape[1]} bytes != column FixedString({self.segment.nbytes})")
        return q

    def centroids(self):
        """The coarse step's centroid table, uint8[nlist, N]."""
        c = np.empty((self.info()["nlist"], self.segment.nbytes), np.uint8)
        check(lib.mqvs_index_centroids_binary(self._h, _ptr(c), c.size))
        return c

    def probes(self, queries, params=None):
        """The lists a search with `params` probes, int64[nq, nprobe] (no order)."""
        q = self._host_queries(queries)
        nq = q.shape[0]
        buf = np.full((nq, self.info()["nlist"]), -1, np.int64)
        check(lib.mqvs_index_probes_binary(self._h, _ptr(q), nq, _params(params), _ptr(buf)))
        npb = _lib.last_index_stats()["nprobe"]
        return buf.reshape(-1)[: nq * npb].reshape(nq, npb).copy()

    def search(self, queries, k, params=None, filter_bitmap=None, row_exists=None, first_stage_only=False,
               out=None, async_=False, stream=None):
        """(ids[nq,k] int64, dist[nq,k] float32) as BinaryVectorScanSegment.search:
        ascending by (distance, row), -1 / FLT_MAX padded.  The distances are
        exact, so first_stage_only returns the same result."""
        fs = F_FIRST_STAGE if first_stage_only else 0
        pr = _params(params)

        def call(qp, nq, fp, ep, ip, dp, flags, st):
            check(lib.mqvs_index_search_binary(self._h, qp, nq, k, pr, fp, ep, ip, dp, flags | fs, st))

        nb = self.segment.nbytes
        return _staged_search(queries, k, np.uint8, nb,
                              lambda got: f"query length {got} bytes != column FixedString({nb})", filter_bitmap,
                              row_exists, out, async_, stream, call, torch_width_check=True)

    free = VectorIndex.free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def last_index_stats():
    return _lib.last_index_stats()


def index_blob_info(blob):
    """The header fields of a saved index (mqvs_index_blob_info: host only; the
    first block must be stored uncompressed, as save() writes it)."""
    b = np.frombuffer(bytes(blob), np.uint8)
    st = _lib.IndexBlobInfo()
    check(lib.mqvs_index_blob_info(_ptr(b), b.size, ctypes.byref(st)))
    return {f: getattr(st, f) for f, _ in _lib.IndexBlobInfo._fields_}


def decoupled_filter(new_filter, new_rows, inverted_row_ids_map, inverted_row_sources_map, own_id, old_rows):
    """getRealBitmap (VIUtils.cpp:479-497) on the GPU: a PREWHERE bitmap over
    the decoupled part's rows -> the bitmap over one source part's rows."""
    nf = _host_u8(new_filter)
    inv = None if inverted_row_ids_map is None else np.ascontiguousarray(inverted_row_ids_map, np.uint64)
    src = None if inverted_row_sources_map is None else np.ascontiguousarray(inverted_row_sources_map, np.uint8)
    out = np.zeros((old_rows + 7) // 8, np.uint8)
    check(lib.mqvs_decoupled_filter(_ptr(nf), new_rows, _ptr(inv), _ptr(src), 0 if inv is None else inv.size,
                                    own_id, _ptr(out), old_rows, 0, None))
    return out
