"""The value classes of value_cases.py on the CPU oracle alone: the two scan
loops agree, the operator's validity cuts and padding hold independently of
the scan loop (checked through O.l2sqr / O.inner_product per pair), and every
class still is what its name says (so the GPU tests of test_gpu_values.py do
not go hollow when a generator or a size changes).
"""
import numpy as np
import pytest

import value_cases as V
from oracle import oracle as O

FLT_MAX, FLT_MIN = V.FLT_MAX, V.FLT_MIN


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _count(ids):
    return (ids >= 0).sum(axis=1)


@pytest.mark.parametrize("nq", [4, 24])
@pytest.mark.parametrize("name,metric", V.CASE_METRICS, ids=[f"{n}-{m}" for n, m in V.CASE_METRICS])
def test_scan_loops_agree(name, metric, nq):
    """orc_vector_scan == orc_vector_scan_fast, ids and distance bits."""
    ids_s, dist_s = V.reference(name, metric, nq, fast=False)
    ids_f, dist_f = V.reference(name, metric, nq, fast=True)
    assert np.array_equal(ids_s, ids_f)
    assert np.array_equal(_bits(dist_s), _bits(dist_f))
    assert not np.isnan(dist_f).any()


L2_IP = [(n, m) for n, m in V.CASE_METRICS if m != "Cosine"]


@pytest.mark.parametrize("name,metric", L2_IP, ids=[f"{n}-{m}" for n, m in L2_IP])
def test_direct_formula_cut_and_padding(name, metric):
    """nq 4 (direct formula): each returned pair's distance is the helper's
    value of that pair; the count is min(k, rows passing the cut) -- L2
    d < FLT_MAX, IP ip > FLT_MIN, NaN never -- and the rest is padding."""
    c = V.case(name)
    ids, dist = V.reference(name, metric, 4)
    fn = O.l2sqr if metric == "L2" else O.inner_product
    pad = FLT_MIN if metric == "IP" else FLT_MAX
    for q in range(4):
        with np.errstate(all="ignore"):
            helper = np.array([fn(c.queries[q], c.rows[r]) for r in range(c.rows.shape[0])], np.float32)
            ok = helper < FLT_MAX if metric == "L2" else helper > FLT_MIN
        want = min(c.k, int(ok.sum()))
        got = int((ids[q] >= 0).sum())
        assert got == want, (name, metric, q, got, want)
        assert (ids[q, :got] >= 0).all() and (ids[q, got:] == -1).all()
        assert np.array_equal(_bits(dist[q, got:]), _bits(np.full(c.k - got, pad, np.float32)))
        assert np.array_equal(_bits(dist[q, :got]), _bits(helper[ids[q, :got]])), (name, metric, q)
        assert ok[ids[q, :got]].all()
        assert len(set(ids[q, :got].tolist())) == got
        # best first; equal values by ascending row
        d = dist[q, :got].astype(np.float64)
        with np.errstate(invalid="ignore"):
            step = np.diff(d) if metric == "L2" else -np.diff(d)
        same = d[1:] == d[:-1]  # (inf - inf is NaN: compare, not subtract)
        assert (same | (step > 0)).all(), (name, metric, q)
        if got < c.k:  # the whole valid set came back: its order is a total sort
            order = np.lexsort((np.arange(len(helper)), helper if metric == "L2" else -helper.astype(np.float64)))
            order = order[ok[order]]
            assert np.array_equal(ids[q, :got], order[:got]), (name, metric, q)


def test_specials_rows_returned():
    """NaN, inf, 3e38 and all-1e19 rows never come back under L2 (at d 40 the
    squared distance to a 1e19 row overflows under both formulas: 40 * 1e38);
    every other row does.  IP returns +inf distances; cosine returns the
    finite huge and tiny rows."""
    where = V.special_rows()
    c = V.case("specials")
    never = np.concatenate([where[k] for k in ("one_nan", "one_pinf", "one_ninf", "one_3e38", "all_3e38",
                                                   "all_1e19", "all_m1e19")])
    n = c.rows.shape[0]
    for nq in (3, 24):
        ids, dist = O.vector_scan(c.rows, c.queries[:nq], n, O.L2, c.granule, fast=True)
        for q in range(nq):
            got = set(ids[q][ids[q] >= 0].tolist())
            assert got == set(range(n)) - set(never.tolist()), (nq, q)
    ids, dist = V.reference("specials", "L2", 4)
    assert (_count(ids) == c.k).all()
    ids, dist = V.reference("specials", "IP", 4)
    assert np.isposinf(dist).any()
    ids, dist = O.vector_scan(c.rows, c.queries[:4], n, O.COSINE, c.granule, fast=True)
    for q in range(4):
        got = set(ids[q][ids[q] >= 0].tolist())
        for kind in ("one_3e38", "all_3e38", "all_1e19", "all_m1e19", "all_1e-42"):
            assert set(where[kind].tolist()) <= got, kind
        assert not got & set(where["one_nan"].tolist())


def test_big17_keeps_its_prefilter_and_returns_k():
    """The largest row norm stays under the 1e18 limit of the pre-filter, and
    every metric returns k finite results."""
    c = V.case("big17")
    norms = np.sqrt((c.rows.astype(np.float64) ** 2).sum(axis=1))
    assert 5e17 < norms.max() < 0.97e18
    qnorms = np.sqrt((c.queries.astype(np.float64) ** 2).sum(axis=1))
    assert qnorms.max() < 0.97e18  # (queries have the same limit, k_query_bound)
    for metric in V.ALL:
        for nq in (4, 24):
            ids, dist = V.reference("big17", metric, nq)
            assert (ids >= 0).all() and np.isfinite(dist).all()


def test_tiny20_denormal_distances():
    for nq in (4, 24):
        ids, dist = V.reference("tiny20", "L2", nq)
        assert (ids >= 0).all()
        if nq == 4:  # (the BLAS formula clamps at 0 and cancels)
            assert (dist > 0).all()
        assert (dist < FLT_MIN).all()
        ids, dist = V.reference("tiny20", "IP", nq)
        assert (ids == -1).all() and (dist == FLT_MIN).all()
        ids, dist = V.reference("tiny20", "Cosine", nq)
        assert (ids >= 0).all()


def test_cut_and_negip_lists_end_inside_k():
    for name, lo, hi in (("cut", 0.2, 0.8), ("negip", 0.4, 0.8)):
        k = V.case(name).k
        for nq in (4, 24, V.NQ_MAX):
            ids, dist = V.reference(name, "IP", nq)
            cnt = _count(ids)
            assert (cnt > lo * k).all() and (cnt < hi * k).all(), (name, nq, cnt.min(), cnt.max())
            assert (dist[ids < 0] == FLT_MIN).all() and (dist[ids >= 0] > FLT_MIN).all()


@pytest.mark.parametrize("name", ["eps", "eps_plus"])
def test_eps_rows_straddle_the_normalize_skip(name):
    c = V.case(name)
    normed = O.normalize(c.rows)
    skipped = (_bits(normed) == _bits(c.rows)).all(axis=1)
    frac = skipped.mean()
    assert 0.3 < frac < 0.7, frac
    qn = O.normalize(c.queries)
    qskip = (_bits(qn) == _bits(c.queries)).all(axis=1)
    assert 10 < qskip.sum() < V.NQ_MAX - 10
    for nq in (4, 24):
        ids, _ = V.reference(name, "Cosine", nq)
        for q in range(nq):
            got = ids[q][ids[q] >= 0]
            assert skipped[got].any() and (~skipped[got]).any(), (nq, q)
    if name == "eps_plus":
        zero, huge = 100, c.rows.shape[0] - 1
        assert not c.rows[zero].any() and (c.rows[huge] == np.float32(1e20)).all()
        assert skipped[zero] and not normed[huge].any()


def test_tie_inf_has_more_ties_than_the_lds_sort():
    c = V.case("tie_inf")
    assert np.isfinite(c.rows).all()
    with np.errstate(all="ignore"):
        ip = np.array([O.inner_product(c.queries[0], r) for r in c.rows], np.float32)
    assert np.isposinf(ip).sum() > 4200
    ids, dist = V.reference("tie_inf", "IP", 4)
    assert np.isposinf(dist[0]).all()
    assert np.array_equal(ids[0], np.flatnonzero(np.isposinf(ip))[:c.k])  # ties: ascending row


def test_qspecial_rules():
    k = V.case("qspecial_base").k
    for nq in (7, 24):
        cnt = {m: _count(V.reference("qspecial_base", m, nq)[0]) for m in V.ALL}
        assert cnt["L2"][[0, 1, 3]].tolist() == [0, 0, 0] and cnt["L2"][2] == k
        assert cnt["IP"][[0, 2]].tolist() == [0, 0] and cnt["IP"][1] == k and cnt["IP"][3] == k
        assert cnt["Cosine"][[0, 1]].tolist() == [0, 0] and cnt["Cosine"][[2, 3]].tolist() == [k, k]
        ids, dist = V.reference("qspecial_base", "IP", nq)
        assert np.isposinf(dist[1]).all()
        # q6: fewer than k rows at +inf, the rest -inf or NaN (never returned)
        assert 20 < cnt["IP"][6] < k and np.isposinf(dist[6, :cnt["IP"][6]]).all()
        assert cnt["L2"][6] == 0 and cnt["Cosine"][6] == 0
        c = V.case("qspecial_base")
        with np.errstate(all="ignore"):
            ip6 = c.rows[:, 26:35:2].astype(np.float64) @ np.full(5, np.inf)
        assert np.isneginf(ip6).sum() + cnt["IP"][6] > k
    # over big17 the summation order decides: in the direct formula the
    # rounded products are +inf and -inf, which meet (NaN: no row); the fma
    # chain adds the unrounded products, so once the sum is +inf it stays
    ids4, dist4 = V.reference("qspecial_big17", "IP", 4)
    ids24, dist24 = V.reference("qspecial_big17", "IP", 24)
    assert _count(ids4)[3] == 0
    assert _count(ids24)[3] == k and np.isposinf(dist24[3]).all()


def test_raw_ip_cut_differs_from_the_operators():
    """tryBruteForceSearch (faiss knn_inner_product) keeps every
    ip > -FLT_MAX; the operator (searchWrapper's FLT_MIN init) only
    ip > FLT_MIN."""
    c = V.case("negip")
    ids, dist = O.knn(c.queries[:4], c.rows, c.k, O.IP)
    assert (ids >= 0).all() and (dist < 0).any()
    ids, dist = V.reference("negip", "IP", 4)
    assert (dist > 0).all() and (ids < 0).any()
