"""The ordered-row recipes (row_order_cases.py) do what test_gpu_row_order.py
relies on, checked in fp64 numpy / integer arithmetic on any machine:

* worst_first overflows: every window of the length of a main-scan segment
  holds far more rows at or under the k-th best of the rows before it than a
  candidate list holds (float: 65536-row windows, capacity 32768 at nq 1024;
  binary: 131072-row windows, capacity 52224 at nq 640).  The margins (1.5x,
  1.25x) cover the search's real thresholds, which are bounds on that k-th
  value (3 radix passes; widened by 2B on the bf16 route) and so only pass
  more rows;
* no mass tie: fewer than 4096 rows tie with the k-th best of the whole part,
  so a candidate-overflow error on these parts would be a bug, not the
  documented limit;
* best_first keeps the best rows early.
"""
import numpy as np
import pytest

import row_order_cases as R

N, D, K = 262144, 16, 10
NB = 200000
FLOAT_WINDOW, FLOAT_CAP = 65536, 32768    # kMinSegRows; cand_capacity(1024, 10)
BINARY_WINDOW, BINARY_CAP = 131072, 52224  # the plan's fifth segment; cand_capacity(640, 10)


def ties_at_kth(dist, k):
    kth = np.partition(dist, k - 1, axis=1)[:, k - 1]
    return (dist == kth[:, None]).sum(axis=1)


@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
def test_float_worst_first_overflows_every_window(metric):
    tr = R.trend(metric, N, D, "worst_first")
    assert tr.rows.shape == (N, D) and tr.queries.shape == (R.NQ_DISTINCT, D)
    assert len({q.tobytes() for q in tr.queries}) == R.NQ_DISTINCT
    dist = R.distances(metric, tr.rows, tr.queries)
    starts = R.window_starts(N, FLOAT_WINDOW)
    assert starts[0] == 256 and starts[1] == 8192 and starts[-1] == N - FLOAT_WINDOW
    worst = min(int(R.passing(dist, b, FLOAT_WINDOW, K).min()) for b in starts)
    print(metric, "fewest passing rows of a window:", worst)
    assert worst >= 1.5 * FLOAT_CAP
    assert ties_at_kth(dist, K).max() < 4096


@pytest.mark.parametrize("nbits", [256, 1024])
@pytest.mark.parametrize("metric", ["Hamming", "Jaccard"])
def test_binary_worst_first_overflows_every_window(metric, nbits):
    tr = R.trend_codes(NB, nbits, "worst_first")
    assert tr.rows.shape == (NB, nbits // 8) and tr.queries.shape == (R.NQ_DISTINCT, nbits // 8)
    assert len({q.tobytes() for q in tr.queries}) == R.NQ_DISTINCT
    dist = R.distances_binary(metric, tr.rows, tr.queries)
    starts = R.window_starts(NB, BINARY_WINDOW)
    assert starts[0] == 256 and starts[-1] + BINARY_WINDOW <= NB
    worst = min(int(R.passing(dist, b, BINARY_WINDOW, K, strict=True).min()) for b in starts)
    print(metric, nbits, "fewest passing rows of a window:", worst)
    assert worst >= 1.25 * BINARY_CAP
    assert ties_at_kth(dist, K).max() < 4096


@pytest.mark.parametrize("order", ["best_first", "sawtooth"])
@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
def test_float_other_orders_have_no_mass_tie(metric, order):
    tr = R.trend(metric, N, D, order)
    assert ties_at_kth(R.distances(metric, tr.rows, tr.queries), K).max() < 4096


def k_best_rows(dist, k):
    return np.argsort(dist, axis=1, kind="stable")[:, :k]


@pytest.mark.parametrize("metric", ["L2", "IP", "Cosine"])
def test_float_best_first_keeps_the_best_early(metric):
    """The k best rows of a best_first part lie at its start.  Under IP they
    are all among the first 256 rows (the probe).  Under L2 and cosine the
    trend falls by 1e-5 of a squared radius per row while the queries' offset
    from the centre (0.02 N(0, I)) moves a row's distance by ~0.02, so the
    best rows spread over the first few thousand (the last of them at row
    2668): within the first granule of 8192 rows, which is the aligned
    cosine probe, and the probe's k-th best leaves the main scan few rows."""
    tr = R.trend(metric, N, D, "best_first")
    dist = R.distances(metric, tr.rows, tr.queries)
    last = int(k_best_rows(dist, K).max())
    print(metric, "last of the k best rows:", last)
    assert last < (256 if metric == "IP" else 8192)
    # the 65536 rows after the probe hold few rows under the probe's k-th best
    assert R.passing(dist, 256, FLOAT_WINDOW, K).max() < 4096


def test_binary_best_first_keeps_the_best_early():
    """The flip probability rises by 2e-6 per row from 0.05: the k best rows
    (13 +- 4 bits of 256 away) spread over the first eighth of the part, and
    the probe's k-th best (256 rows) leaves the main scan few rows."""
    tr = R.trend_codes(NB, 256, "best_first")
    dist = R.distances_binary("Hamming", tr.rows, tr.queries)
    last = int(k_best_rows(dist, K).max())
    print("last of the k best rows:", last)
    assert last < NB // 8
    assert R.passing(dist, 256, BINARY_WINDOW, K, strict=True).max() < 4096
