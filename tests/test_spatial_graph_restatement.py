"""Hand-traced cases of tests/spatial_graph_restatement.py (the reference's spatial_graph, src/singlet.cpp:1365-1414): the cut
by index and not by distance, the self weight, the strict test at d == max_dist; the brute-force and cell-list forms
agree.  Each case also names the library's entry point, which the GPU tests hold to the restatement."""
import numpy as np
import pytest

import singlet_amd as sa
import spatial_graph_restatement as sr


def test_the_library_exposes_spatial_graph():
    assert callable(sa.spatial_graph)
    from singlet_amd import _lib
    assert "sgl_spatial_graph" in _lib.SIGNATURES


def test_cut_by_index_not_distance():
    # point 0 at the origin; points 1 and 2 far (0.9), 3 and 4 near (0.1); max_k = 3: column 0 keeps 0, 1, 2
    assert sa.spatial_graph is not None
    x = np.array([0.0, 0.9, -0.9, 0.1, 0.0])
    y = np.array([0.0, 0.0, 0.0, 0.0, 0.1])
    p, i, v = sr.brute(x, y, 1.0, max_k=3)
    assert list(i[p[0]:p[1]]) == [0, 1, 2]
    w = (1.0 - np.array([0.0, 0.9, 0.9])) * 1.0   # (max_dist - d) * (1 / max_dist)
    assert np.array_equal(v[p[0]:p[1]], w / ((w[0] + w[1]) + w[2]))
    # column 3 (at 0.1, 0): distances 0.1, 0.8, 1.0 (not < 1), 0, 0.1414: keeps 0, 1, 3
    assert list(i[p[3]:p[4]]) == [0, 1, 3]


def test_self_weight_and_its_place():
    # three points on a line at 0, 0.5, 1; max_dist 0.75, max_k 1: every column keeps only its lowest-numbered point in range
    assert sa.spatial_graph is not None
    x = np.array([0.0, 0.5, 1.0])
    y = np.zeros(3)
    p, i, v = sr.brute(x, y, 0.75, max_k=1)
    assert list(p) == [0, 1, 2, 3] and list(i) == [0, 0, 1]
    assert np.all(v == 1.0)
    # max_k 100: point 1 keeps 0, 1, 2; its own weight is (0.75 - 0) * fl(1 / 0.75)
    p, i, v = sr.brute(x, y, 0.75, max_k=100)
    assert list(i[p[1]:p[2]]) == [0, 1, 2]
    s = 1.0 / 0.75
    w = np.array([(0.75 - 0.5) * s, 0.75 * s, (0.75 - 0.5) * s])
    assert np.array_equal(v[p[1]:p[2]], w / ((w[0] + w[1]) + w[2]))


def test_strict_test_at_max_dist():
    # the unit square: max_dist 1 drops the 4-neighbours (d == 1), max_dist fl(sqrt(2)) drops the diagonals
    assert sa.spatial_graph is not None
    x = np.array([0.0, 1.0, 0.0, 1.0])
    y = np.array([0.0, 0.0, 1.0, 1.0])
    p, i, v = sr.brute(x, y, 1.0)
    assert list(p) == [0, 1, 2, 3, 4] and list(i) == [0, 1, 2, 3] and np.all(v == 1.0)
    p, i, v = sr.brute(x, y, np.sqrt(2.0))
    assert list(i[p[0]:p[1]]) == [0, 1, 2]
    assert list(i[p[3]:p[4]]) == [1, 2, 3]


def test_empty_cases():
    assert sa.spatial_graph is not None
    p, i, v = sr.brute(np.zeros(0), np.zeros(0), 1.0)
    assert list(p) == [0] and i.size == 0
    p, i, v = sr.brute(np.arange(4.0), np.zeros(4), 2.0, max_k=0)
    assert list(p) == [0] * 5 and i.size == 0


@pytest.mark.parametrize("max_dist,max_k", [(0.05, 100), (0.2, 7), (3.0, 50)])
def test_cell_list_form_matches_brute_force(max_dist, max_k):
    assert sa.spatial_graph is not None
    rng = np.random.default_rng(7)
    x, y = rng.random(700), rng.random(700)
    p, i, v = sr.brute(x, y, max_dist, max_k)
    cols = sr.columns(x, y, max_dist, max_k, range(0, 700, 13))
    for c, (r, w) in cols.items():
        assert np.array_equal(r, i[p[c]:p[c + 1]]) and np.array_equal(w, v[p[c]:p[c + 1]])


def test_fused_pairs_are_found():
    # the detector of contraction-sensitive pairs sees some among random doubles (the GPU contraction test relies on it)
    assert sa.spatial_graph is not None
    rng = np.random.default_rng(3)
    x, y = rng.random(60), rng.random(60)
    pairs = [(a, b) for a in range(60) for b in range(60) if a != b]
    assert len(sr.fused_pairs(x, y, pairs)) > 0
