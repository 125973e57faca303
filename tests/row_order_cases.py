"""Parts whose rows are ordered by distance to the queries, shared by
test_row_order_cases.py (CPU) and test_gpu_row_order.py (GPU).

Every FLAT search takes its first threshold from the first P rows of the part
(the probe) and appends every later row that passes it.  On rows in random
order the probe is a fair sample; on a part whose rows drift towards the
queries (time-ordered inserts queried about recent items, an ORDER BY key that
correlates with the embedding) almost every later row passes, and a main-scan
segment longer than the candidate capacity overflows its lists with no tie
anywhere.  The recipes below build such parts from fixed seeds
(zlib.crc32 of a case name):

  trend(metric, n, d, order)    -> Trend(rows[n, d] float32, queries[32, d])
  trend_codes(n, nbits, order)  -> Trend(codes[n, nbits / 8] uint8, queries[32, nbits / 8])

order: "worst_first" (every row nearer than the ones before), "best_first"
(the reverse: the probe holds the best rows), "sawtooth" (worst to best every
8192 rows).

A part has NQ_DISTINCT = 32 distinct queries, all near its centre; tile()
repeats them (query j = distinct query j mod 32) up to the batch size a route
needs.  A query's result depends on the other queries of its call only through
the batch size that selects the distance formula (nq >= 20: the BLAS branch),
and 32 is on the same side of that switch as every tiled batch, so the
oracle's result for the 32 distinct queries, tiled the same way, is the
oracle's result for the batch.  Batches of fewer than 32 queries take
queries[:nq] and their own oracle run.
"""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

NQ_DISTINCT = 32
ORDERS = ("worst_first", "best_first", "sawtooth")
SAW = 8192

Trend = namedtuple("Trend", "rows queries")


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _t(n, order):
    i = np.arange(n, dtype=np.float64)
    if order == "worst_first":
        return i / n
    if order == "best_first":
        return 1.0 - i / n
    if order == "sawtooth":
        return (i % SAW) / SAW
    raise KeyError(order)


@lru_cache(maxsize=4)
def _geometry(n, d):
    """Centre c, unit offsets u_i perpendicular to c, 32 queries near c (fp64)."""
    rng = _rng(f"trend_{n}_{d}")
    c = rng.standard_normal(d)
    u = rng.standard_normal((n, d))
    # Without the component along c: a free u_i gives the cosine distance a
    # heavy lower tail, and the first 256 rows then hold outliers that beat the
    # trend (tens to thousands of passing rows per window instead of > 50000)
    u -= np.outer(u @ c / (c @ c), c)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = c[None, :] + 0.02 * rng.standard_normal((NQ_DISTINCT, d))
    return c, u, q


@lru_cache(maxsize=6)
def trend(metric, n, d, order):
    c, u, q = _geometry(n, d)
    t = _t(n, order)
    r = 3.0 - 2.5 * t
    if metric == "L2":
        rows = c[None, :] + r[:, None] * u
    elif metric == "Cosine":
        # (the scale of a row must not matter)
        rows = (1.0 + np.arange(n) % 7)[:, None] * (c[None, :] + r[:, None] * u)
    elif metric == "IP":
        rows = (1.0 + 2.0 * t)[:, None] * c[None, :] + 0.5 * u
    else:
        raise KeyError(metric)
    rows = np.ascontiguousarray(rows, np.float32)
    queries = np.ascontiguousarray(q, np.float32)
    rows.setflags(write=False)
    queries.setflags(write=False)
    return Trend(rows, queries)


@lru_cache(maxsize=4)
def trend_codes(n, nbits, order):
    """Centre bits Bernoulli(0.5); row i = the centre with each bit flipped
    with probability 0.45 - 0.40 t_i; queries = the centre with 2 % flipped."""
    rng = _rng(f"trend_codes_{n}_{nbits}")
    centre = rng.random(nbits) < 0.5
    p = 0.45 - 0.40 * _t(n, order)
    codes = np.empty((n, nbits // 8), np.uint8)
    for b in range(0, n, 16384):  # (bounds the fp32 uniforms held at once)
        e = min(n, b + 16384)
        flip = rng.random((e - b, nbits), dtype=np.float32) < p[b:e, None]
        codes[b:e] = np.packbits(centre[None, :] ^ flip, axis=1)
    queries = np.packbits(centre[None, :] ^ (rng.random((NQ_DISTINCT, nbits)) < 0.02), axis=1)
    codes.setflags(write=False)
    queries.setflags(write=False)
    return Trend(codes, queries)


def tile(a, nq):
    """Query j of the batch = distinct query j mod 32 (also tiles a result)."""
    return np.ascontiguousarray(a[np.arange(nq) % NQ_DISTINCT])


def distances(metric, rows, queries):
    """fp64 [nq, n], smaller = better (IP negated): what orders the rows."""
    x, q = np.asarray(rows, np.float64), np.asarray(queries, np.float64)
    ip = q @ x.T
    if metric == "IP":
        return -ip
    xn = (x * x).sum(axis=1)
    qn = (q * q).sum(axis=1)
    if metric == "L2":
        return qn[:, None] - 2.0 * ip + xn[None, :]
    if metric == "Cosine":
        return 1.0 - ip / np.sqrt(qn[:, None] * xn[None, :])
    raise KeyError(metric)


_POP = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def _bits(a):
    """Set bits per row of a [n, words] array."""
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(a).sum(axis=1, dtype=np.int64)
    return _POP[a.view(np.uint8)].sum(axis=1, dtype=np.int64)


def distances_binary(metric, codes, queries):
    """[nq, n] Hamming counts (int64) or Jaccard distances (fp64)."""
    c = np.ascontiguousarray(codes).view(np.uint64)  # (code widths are multiples of 64 bits)
    qs = np.ascontiguousarray(queries).view(np.uint64)
    out = np.empty((qs.shape[0], c.shape[0]), np.int64 if metric == "Hamming" else np.float64)
    for j, q in enumerate(qs):
        if metric == "Hamming":
            out[j] = _bits(c ^ q[None, :])
        elif metric == "Jaccard":
            out[j] = 1.0 - _bits(c & q[None, :]) / np.maximum(_bits(c | q[None, :]), 1)
        else:
            raise KeyError(metric)
    return out


def window_starts(n, window):
    """The window starts the overflow conditions are stated for."""
    return [256] + list(range(SAW, n - window + 1, SAW))


def passing(dist, b, window, k, strict=False):
    """Per query: the rows of [b, b + window) whose distance is <= (strict: <)
    the k-th best of rows [0, b)."""
    kth = np.partition(dist[:, :b], k - 1, axis=1)[:, k - 1]
    w = dist[:, b:b + window]
    return ((w < kth[:, None]) if strict else (w <= kth[:, None])).sum(axis=1)
