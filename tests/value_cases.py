"""Value classes outside the ordinary range, shared by test_oracle_values.py
(CPU) and test_gpu_values.py (GPU): non-finite, overflowing, denormal and
threshold-straddling parts and query sets, each built once from a fixed seed.

Every part is small (n 1500 .. 6000, d 24 / 40 / 96, granule 256 / 512): a
few 256-row tiles, several cosine chunks with a partial last one, and -- where
a class needs them -- more tied rows than the 4096-record LDS sort holds.

case(name) -> Case(name, rows, queries, k, granule, metrics); queries holds NQ_MAX
rows, the tests slice queries[:nq].
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

FLT_MAX = np.float32(3.4028235e38)
FLT_MIN = np.float32(1.1754944e-38)
FLT_EPSILON = np.float32(1.1920929e-07)
NQ_MAX = 200
ALL = ("L2", "IP", "Cosine")

Case = namedtuple("Case", "name rows queries k granule metrics")

# name -> (n, d, granule, k, metrics)
SHAPES = {
    "specials": (3000, 40, 512, 50, ALL),
    "big17": (1500, 40, 256, 50, ALL),
    "tiny20": (5000, 24, 512, 50, ALL),
    "cut": (2000, 40, 256, 1000, ALL),
    "negip": (1500, 40, 256, 1200, ALL),
    "eps": (1600, 96, 256, 1500, ("Cosine",)),
    "eps_plus": (1602, 96, 256, 1500, ("Cosine",)),
    "tie_inf": (6000, 24, 512, 50, ALL),
    "qspecial_base": (1500, 40, 256, 50, ALL),
    "qspecial_big17": (1500, 40, 256, 50, ALL),
    # the same parts and tie_inf's without the queries the pre-filter refuses
    "qfinite_base": (1500, 40, 256, 50, ALL),
    "qfinite_big17": (1500, 40, 256, 50, ALL),
    "tie_fin": (6000, 24, 512, 50, ALL),
}
NAMES = tuple(SHAPES)

# specials: kinds of special rows, ten rows of each
SPECIAL_KINDS = ("one_nan", "one_pinf", "one_ninf", "one_3e38", "all_3e38", "all_1e19", "all_m1e19", "all_1e-42",
                 "all_pzero", "all_nzero")


def _gauss(tag, n, d):
    return np.random.RandomState(0x56A1 + tag).standard_normal((n, d)).astype(np.float32)


@lru_cache(maxsize=None)
def base(n, d):
    """The standard-normal part of n rows (one per (n, d); read-only)."""
    a = _gauss(d, n, d)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def base_queries(d):
    a = _gauss(1000 + d, NQ_MAX, d)
    a.setflags(write=False)
    return a


@lru_cache(maxsize=None)
def special_rows():
    """{kind: sorted row numbers} of the specials part: ten rows per kind at
    seeded places, so every 512-row chunk holds some."""
    n = SHAPES["specials"][0]
    pick = np.random.RandomState(0x5BEC).permutation(n)[:10 * len(SPECIAL_KINDS)]
    return {kind: np.sort(pick[10 * i:10 * i + 10]) for i, kind in enumerate(SPECIAL_KINDS)}


def _specials():
    n, d = SHAPES["specials"][:2]
    rows = base(n, d).copy()
    rs = np.random.RandomState(0x5BED)
    for kind, where in special_rows().items():
        for r in where:
            c = rs.randint(d)
            if kind == "one_nan":
                rows[r, c] = np.nan
            elif kind == "one_pinf":
                rows[r, c] = np.inf
            elif kind == "one_ninf":
                rows[r, c] = -np.inf
            elif kind == "one_3e38":
                rows[r, c] = 3e38
            else:
                rows[r, :] = {"all_3e38": 3e38, "all_1e19": 1e19, "all_m1e19": -1e19, "all_1e-42": 1e-42,
                              "all_pzero": 0.0, "all_nzero": -0.0}[kind]
    return rows, base_queries(d)


def _eps_scaled(a, tag):
    """Each row of a scaled to norm sqrt(FLT_EPSILON) * (1 +- 0.2 %): the fp32
    squared norm falls on either side of VectorDataset::normalize's
    `sum < FLT_EPSILON` skip."""
    a64 = a.astype(np.float64)
    norm = np.sqrt((a64 * a64).sum(axis=1))
    u = np.random.RandomState(0xE95 + tag).uniform(-0.002, 0.002, a.shape[0])
    target = np.sqrt(float(FLT_EPSILON)) * (1.0 + u)
    return (a64 * (target / norm)[:, None]).astype(np.float32)


def _eps(n):
    d = SHAPES["eps"][1]
    rows = _eps_scaled(base(n, d), 0)
    q = base_queries(d).copy()
    q[1::2] = _eps_scaled(q[1::2], 1)  # every other query straddles the skip too
    return rows, q


def _eps_plus():
    rows, q = _eps(SHAPES["eps"][0])
    d = rows.shape[1]
    extra = np.zeros((2, d), np.float32)
    extra[1, :] = 1e20  # the squared norm overflows: the row normalises to zeros
    # one in the first chunk, one in the last
    return np.concatenate([rows[:100], extra[:1], rows[100:], extra[1:]]), q


def _tie_inf():
    """Finite rows, three in four with a positive first component; query 0 has
    a +inf first component, so its IP against those rows is +inf (the others
    -inf, or NaN where the component is 0)."""
    n, d = SHAPES["tie_inf"][:2]
    rows = base(n, d).copy()
    keep = np.arange(n) % 4 == 3
    rows[~keep, 0] = np.abs(rows[~keep, 0])
    q = base_queries(d).copy()
    q[0, 0] = np.inf
    return rows, q


def qspecial(d):
    """base queries with q0 = one NaN, q1 = one +inf, q2 = zeros, q3 = all
    1e30, q4 = all -0.0, q5 = all 1e-30, q6 = five +inf components.  q0, q1,
    q3 and q6 have a norm that is NaN, infinite or >= 1e18: a search that
    holds one cannot be served by the bf16 pre-filter (an infinite component
    splits into hi = inf, lo = NaN; 1e30 products overflow the MFMA sum) and
    goes to the exact kernels (k_query_bound); qfinite() is the rest.

    q6: a row's IP is +inf when its five components are all positive (1 row
    in 32), -inf when all are negative, NaN otherwise -- fewer than k = 50
    rows at +inf, more than k that are not NaN, so the k-th best value of a
    selection without a validity cut is -inf, the worst infinity."""
    q = base_queries(d).copy()
    q[0, 3] = np.nan
    q[1, 5] = np.inf
    q[2, :] = 0.0
    q[3, :] = 1e30
    q[4, :] = -0.0
    q[5, :] = 1e-30
    q[6, 26:35:2] = np.inf  # 33 rows at +inf, 44 at -inf (test_oracle_values pins both sides of k)
    return q


def _drop(q, which):
    """q without the rows `which`, topped up to NQ_MAX with negated queries."""
    keep = np.delete(np.arange(q.shape[0]), which)
    return np.concatenate([q[keep], -q[keep[-len(which):]]])


def qfinite(d):
    """qspecial without the queries a pre-filtered search is not trusted with
    (norm NaN, infinite or >= 1e18: q0, q1, q3, q6; a batch that holds one is
    served by the exact kernels).  What is left of the special queries leads
    the set -- q2 zeros, q4 -0.0, q5 all 1e-30 (values of the size of the
    bound's absolute slack) -- so every batch size runs them through the
    pre-filter."""
    return _drop(qspecial(d), [0, 1, 3, 6])


@lru_cache(maxsize=None)
def case(name):
    n, d, granule, k, metrics = SHAPES[name]
    if name == "specials":
        rows, q = _specials()
    elif name == "big17":
        rows, q = base(n, d) * np.float32(1e17), base_queries(d) * np.float32(1e17)
    elif name == "tiny20":
        rows, q = base(n, d) * np.float32(1e-20), base_queries(d) * np.float32(1e-20)
    elif name == "cut":
        rows, q = base(n, d) * np.float32(3e-20), base_queries(d) * np.float32(1e-19)
    elif name == "negip":
        rows = base(n, d)
        q = -rows[:NQ_MAX]
    elif name == "eps":
        rows, q = _eps(n)
    elif name == "eps_plus":
        rows, q = _eps_plus()
    elif name == "tie_inf":
        rows, q = _tie_inf()
    elif name == "qspecial_base":
        rows, q = base(n, d), qspecial(d)
    elif name == "qspecial_big17":
        rows, q = base(n, d) * np.float32(1e17), qspecial(d)
    elif name == "qfinite_base":
        rows, q = base(n, d), qfinite(d)
    elif name == "qfinite_big17":
        rows, q = base(n, d) * np.float32(1e17), qfinite(d)
    elif name == "tie_fin":
        rows, q = _tie_inf()
        q = _drop(q, [0])  # (without the +inf query)
    else:
        raise KeyError(name)
    rows = np.ascontiguousarray(rows, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    assert rows.shape == (n, d) and q.shape == (NQ_MAX, d)
    rows.setflags(write=False)
    q.setflags(write=False)
    return Case(name, rows, q, k, granule, metrics)


CASE_METRICS = [(name, m) for name in NAMES for m in SHAPES[name][4]]


@lru_cache(maxsize=None)
def reference(name, metric, nq, fast=True):
    """O.vector_scan of the case (no filter), computed once and shared."""
    from oracle import oracle as O
    c = case(name)
    ids, dist = O.vector_scan(c.rows, c.queries[:nq], c.k, O.METRICS[metric], c.granule, fast=fast)
    ids.setflags(write=False)
    dist.setflags(write=False)
    return ids, dist
