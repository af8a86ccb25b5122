"""The LKNN / SNN restatement (tests/local_neighbors_restatement.py) on the CPU: its two LKNN forms agree, and it matches
cases worked by hand.  It is the independent pin of the GPU graphs: the reference needs Rcpp and Eigen to build."""
import math

import numpy as np
import pytest

import local_neighbors_restatement as lr

F = np.float32


def _same(a, b):
    pa, ia, xa = a
    pb, ib, xb = b
    assert np.array_equal(pa, pb) and np.array_equal(ia, ib)
    assert np.array_equal(np.asarray(xa, np.float64).view(np.uint64), np.asarray(xb, np.float64).view(np.uint64))


@pytest.mark.parametrize("metric", lr.METRICS)
@pytest.mark.parametrize("radius,k,max_dist", [(1.0, 5, 0.0), (float(np.sqrt(F(2))), 3, 0.5), (2.5, 4, 0.0), (0.0, 2, 0.0)])
def test_brute_and_grid_forms_agree(metric, radius, k, max_dist):
    rng = np.random.default_rng(7)
    n = 120
    x = rng.integers(0, 9, n).astype(np.float64)
    y = rng.integers(0, 9, n).astype(np.float64) + rng.random(n) * (radius == 2.5)
    m = rng.random((4, n)) * (rng.random((4, n)) < 0.7)
    try:
        b = lr.lknn_brute(m, x, y, k, radius, metric, True, max_dist)
    except lr.SlotOverflow:
        with pytest.raises(lr.SlotOverflow):
            lr.lknn_grid(m, x, y, k, radius, metric, True, max_dist)
        return
    _same(b, lr.lknn_grid(m, x, y, k, radius, metric, True, max_dist))
    sub = lr.lknn_grid(m, x, y, k, radius, metric, True, max_dist, points=[0, 17, 119])
    for pt, (i, xv) in sub.items():
        assert np.array_equal(i, b[1][b[0][pt]:b[0][pt + 1]]) and np.array_equal(xv, b[2][b[0][pt]:b[0][pt + 1]])


def test_three_by_three_lattice():
    x, y = lr.lattice(3)
    m = np.arange(9, dtype=np.float64).reshape(1, 9)   # point j's embedding is j: euclidean distance |i - j|
    p, i, xv = lr.lknn_brute(m, x, y, 20, 1.0, "euclidean", True, 0.0)
    assert list(p) == [0, 2, 5, 7, 10, 14, 17, 19, 22, 24]
    assert list(i[p[4]:p[5]]) == [1, 3, 5, 7] and list(xv[p[4]:p[5]]) == [3, 1, 1, 3]
    assert list(i[p[0]:p[1]]) == [1, 3] and list(xv[p[0]:p[1]]) == [1, 3]
    # the diagonal neighbours join at sqrt(2), not below
    p2, _, _ = lr.lknn_brute(m, x, y, 20, float(np.nextafter(F(np.sqrt(2)), F(0))), "euclidean", True, 0.0)
    assert np.array_equal(p2, p)
    p3, i3, _ = lr.lknn_brute(m, x, y, 20, float(np.sqrt(F(2))), "euclidean", True, 0.0)
    assert list(i3[p3[4]:p3[5]]) == [0, 1, 2, 3, 5, 6, 7, 8]


@pytest.mark.parametrize("metric,similarity,want", [
    ("jaccard", True, 1 - 3 / 11), ("jaccard", False, 3 / 11),
    ("cosine", True, 1 - 1 / math.sqrt(5)), ("cosine", False, 1 / math.sqrt(5)),
    ("euclidean", True, math.sqrt(8)),
    ("manhattan", True, 2.0),            # sqrt(|1-3| + |2-0|): the reference's root of the L1 sum
    ("hamming", True, 2.0),
    ("kl", True, 3 * math.log(1 / 3)),   # q = 0 skipped in the quotient sum, counted in psum
    ("no-such-metric", True, math.sqrt(8)),
])
def test_every_metric_on_two_vectors(metric, similarity, want):
    P = np.array([[1], [2]], dtype=F)
    Q = np.array([[3], [0]], dtype=F)
    got = lr.distances(P, Q, metric if metric in lr.METRICS else "euclidean", similarity)
    assert got.dtype == F and got.shape == (1,)
    assert abs(float(got[0]) - want) <= 4 * np.spacing(F(abs(want)))


def test_zero_distance_eats_a_slot():
    x, y = np.array([0.0, 1.0, 2.0]), np.zeros(3)
    m = np.array([[1.0, 1.0, 5.0]])
    p, i, xv = lr.lknn_brute(m, x, y, 1, 2.0, "euclidean", True, 0.0)
    assert p[1] - p[0] == 0          # point 1 (distance 0) took point 0's one slot, then was dropped
    p, i, xv = lr.lknn_brute(m, x, y, 2, 2.0, "euclidean", True, 0.0)
    assert list(i[p[0]:p[1]]) == [2] and list(xv[p[0]:p[1]]) == [4.0]


def test_ties_go_to_the_lower_index_and_nan_ranks_last():
    x, y = np.arange(5.0), np.zeros(5)
    m = np.array([[0.0, 1, 1, 0, 1], [0.0, 0, 0, 0, 0]])   # points 0 and 3 all-zero: 0/0 under jaccard
    mf, cx, cy = lr.as_float_inputs(m, x, y)
    # point 1 = (1, 0): candidates 0 (1), 2 (0), 3 (1), 4 (0); the tie at 1 goes to the lower index
    j, d = lr._point(1, np.arange(5), mf, cx, cy, 2, F(5), "jaccard", True, F(0))
    assert list(j) == [2, 4] and list(d) == [0, 0]
    j, d = lr._point(1, np.arange(5), mf, cx, cy, 3, F(5), "jaccard", True, F(0))
    assert list(j) == [0, 2, 4] and list(d) == [1, 0, 0]
    # point 0 (all zero): candidate 3 (all zero) is 0/0 = NaN and ranks after every number
    j, d = lr._point(0, np.arange(5), mf, cx, cy, 3, F(5), "jaccard", True, F(0))
    assert list(j) == [1, 2, 4] and list(d) == [1, 1, 1]
    j, d = lr._point(0, np.arange(5), mf, cx, cy, 4, F(5), "jaccard", True, F(0))
    assert list(j) == [1, 2, 3, 4] and np.isnan(d[2])


def test_slot_overflow_is_detected():
    x, y = np.zeros(3), np.zeros(3)   # three points at one place, radius 0: zero slots per point
    m = np.array([[1.0, 2.0, 3.0]])
    with pytest.raises(lr.SlotOverflow):
        lr.lknn_brute(m, x, y, 5, 0.0, "euclidean", True, 0.0)
    assert lr.n_max_edges(4.0) == 80 and lr.n_max_edges(float(np.sqrt(F(2)))) == 14 and lr.n_max_edges(0.0) == 0


def test_snn_hand_case_and_diagonal_only():
    # columns: 0 = {0, 1}, 1 = {1, 2}, 2 = {}, 3 = {0, 1, 2}
    Gi = np.array([0, 1, 1, 2, 0, 1, 2])
    Gp = np.array([0, 2, 4, 4, 7])
    p, i, x = lr.snn(Gi, Gp, 3, 4, 0.0)
    assert list(p) == [0, 3, 6, 6, 9]
    assert list(i[:3]) == [0, 1, 3] and np.allclose(x[:3], [1, 1 / 3, 2 / 3])
    assert list(i[6:]) == [0, 1, 3] and np.allclose(x[6:], [2 / 3, 2 / 3, 1])
    p, i, x = lr.snn(Gi, Gp, 3, 4, 1 / 3)   # strict >: 1/3 goes
    assert list(i[p[0]:p[1]]) == [0, 3]
    for ms in (1.0, 2.0):
        p, i, x = lr.snn(Gi, Gp, 3, 4, ms)
        assert list(p) == [0, 1, 2, 2, 3] and list(i) == [0, 1, 3] and list(x) == [1.0, 1.0, 1.0]
