"""Clustering on the GPU (sgl_c_louvain, sgl_op_louvain_sweep, sgl_louvain_info, find_clusters) against the numpy
restatement of its rules (tests/louvain_restatement.py).  Everything is equality of bits: labels, Q of every level and the
sweep counts of the full runs; labels, both Q and the move count of single sweeps where the loops turn.  The rule is exact,
there is no tolerance and no share of cases left out."""
import os

import numpy as np
import pytest

import louvain_restatement as lr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -1


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def dgc(sa, p, i, x):
    n = len(p) - 1
    return sa.dgCMatrix(x, i, p, (n, n))


def from_dense(A):
    A = np.asarray(A, dtype=np.float64)
    p, i, x = [0], [], []
    for c in range(A.shape[1]):
        r = np.flatnonzero(A[:, c])
        i += r.tolist()
        x += A[r, c].tolist()
        p.append(len(i))
    return np.array(p, dtype=np.int32), np.array(i, dtype=np.int32), np.array(x, dtype=np.float64)


def from_pairs(n, pairs, weights, diagonal=None):
    """Symmetric graph from (a, b) pairs (a != b, each pair once) with one weight per pair -> (p, i, x), rows ascending."""
    a = np.array([q[0] for q in pairs] + [q[1] for q in pairs], dtype=np.int64)
    b = np.array([q[1] for q in pairs] + [q[0] for q in pairs], dtype=np.int64)
    w = np.concatenate((weights, weights)).astype(np.float64)
    if diagonal is not None:
        d = np.flatnonzero(diagonal)
        a, b, w = np.concatenate((a, d)), np.concatenate((b, d)), np.concatenate((w, np.asarray(diagonal, dtype=np.float64)[d]))
    order = np.lexsort((a, b))                                # by column b, then row a
    p = np.concatenate(([0], np.cumsum(np.bincount(b, minlength=n)))).astype(np.int32)
    return p, a[order].astype(np.int32), w[order]


def star(rng, leaves, hub=0):
    """A star with `leaves` leaves around vertex `hub`, random weights in (0.5, 1.5)."""
    n = leaves + 1
    others = [v for v in range(n) if v != hub]
    return from_pairs(n, [(hub, v) for v in others], 0.5 + rng.random(leaves))


def check_sweep(sa, p, i, x, labels, gamma, what):
    want = lr.op_sweep(p, i, x, labels, gamma)
    got = sa.op_louvain_sweep(dgc(sa, p, i, x), labels, gamma)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), (what, "labels")
    assert bits(got[1]) == bits(want[1]), (what, "Q of labels-in", got[1], want[1])
    assert bits(got[2]) == bits(want[2]), (what, "Q of labels-out", got[2], want[2])
    assert got[3] == want[3], (what, "moved")
    return want


@pytest.fixture(scope="module")
def fixtures():
    z = np.load(os.path.join(GOLD, "louvain_graphs.npz"))
    return {str(name): {k: z["%s_%s" % (name, k)] for k in ("p", "i", "x", "planted", "gammas", "nx_q")} for name in z["names"]}


@pytest.fixture(scope="module")
def want_full(fixtures):
    """The restatement on every fixture and gamma, computed once."""
    return {(name, a): lr.louvain(f["p"], f["i"], f["x"], float(g))
            for name, f in fixtures.items() for a, g in enumerate(f["gammas"])}


def same_run(got, r, want, what):
    assert np.array_equal(got["labels"][r], want["labels"]), (what, "labels")
    assert got["n_clusters"][r] == want["n_clusters"] and got["n_levels"][r] == want["n_levels"], what
    assert np.array_equal(bits(got["q_levels"][r]), bits(want["q_levels"])), (what, got["q_levels"][r][:6], want["q_levels"][:6])
    assert np.array_equal(got["sweeps_levels"][r], want["sweeps_levels"]), what


# -------------------------------------------------------------------------------------------------------------- full runs
@pytest.mark.parametrize("name", ["cliques", "sbm", "snn_noisy", "snn_weak20", "snn_diag"])
def test_full_run_equals_the_restatement_bit_for_bit(sa, fixtures, want_full, name):
    f = fixtures[name]
    G = dgc(sa, f["p"], f["i"], f["x"])
    for a, gamma in enumerate(f["gammas"]):
        got = sa.c_louvain(G, [float(gamma)])
        assert got["labels"].shape == (1, G.ncol) and got["labels"].dtype == np.int32
        same_run(got, 0, want_full[name, a], (name, gamma))
        assert got["n_levels"][0] >= 2 and got["sweeps_levels"][0][0] >= 1
    info = sa.louvain_info()
    assert info["coarse_build"] == 1 and info["slow_level0"] == 0      # no SNN column is wider than the fast path


def test_two_calls_give_the_same_bits(sa, fixtures):
    f = fixtures["snn_weak20"]
    G = dgc(sa, f["p"], f["i"], f["x"])
    a, b = sa.c_louvain(G, [1.0]), sa.c_louvain(G, [1.0])
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_several_resolutions_in_one_call_give_what_single_calls_give(sa, fixtures, want_full):
    f = fixtures["snn_noisy"]
    G = dgc(sa, f["p"], f["i"], f["x"])
    gammas = [float(g) for g in f["gammas"]]
    both = sa.c_louvain(G, gammas)
    assert both["labels"].shape == (3, G.ncol) and both["q_levels"].shape == (3, 32)
    for r, gamma in enumerate(gammas):
        same_run(both, r, want_full["snn_noisy", r], ("multi", gamma))
    f = fixtures["sbm"]
    G = dgc(sa, f["p"], f["i"], f["x"])
    both = sa.c_louvain(G, [2.0, 0.5, 1.0], tol=0.0, max_sweeps=5, max_levels=2)
    for r, gamma in enumerate([2.0, 0.5, 1.0]):
        one = sa.c_louvain(G, [gamma], tol=0.0, max_sweeps=5, max_levels=2)
        for key in one:
            assert one[key][0].tobytes() == both[key][r].tobytes(), (key, gamma)
        same_run(one, 0, lr.louvain(f["p"], f["i"], f["x"], gamma, 0.0, 5, 2), ("limits", gamma))
        assert one["n_levels"][0] <= 2 and np.all(one["sweeps_levels"][0] <= 5)


# ---------------------------------------------------------------------------------------------------------- single sweeps
def test_sweep_of_one_vertex_and_of_two(sa):
    p, i, x = from_dense([[2.5]])
    check_sweep(sa, p, i, x, [0], 1.0, "n = 1")
    p, i, x = from_dense([[0.0, 1.0], [1.0, 0.0]])
    want = check_sweep(sa, p, i, x, [0, 1], 1.0, "n = 2")
    assert want[0].tolist() == [0, 0] and want[3] == 1          # the swap rule: only the higher-numbered singleton moves
    check_sweep(sa, p, i, x, [1, 0], 1.0, "n = 2, labels swapped")
    check_sweep(sa, p, i, x, [1, 1], 0.5, "n = 2, together")
    # self-loops: column 0 holds its diagonal BEFORE its only neighbour, column 1 after it (coarse levels look like this)
    p, i, x = from_dense([[0.5, 1.0, 0.0], [1.0, 0.25, 2.0], [0.0, 2.0, 0.0]])
    for labels in ([0, 1, 2], [2, 1, 0], [1, 1, 0]):
        check_sweep(sa, p, i, x, labels, 1.0, ("two entries, diagonal first", labels))


def test_sweep_with_a_vertex_of_degree_zero_and_a_self_loop_only(sa):
    A = np.zeros((6, 6))
    for a, b, w in ((0, 1, 1.0), (1, 2, 0.75), (0, 2, 0.5), (2, 5, 0.25)):
        A[a, b] = A[b, a] = w
    A[4, 4] = 3.0                                               # vertex 3 has no entry, vertex 4 only its diagonal
    p, i, x = from_dense(A)
    for labels in (np.arange(6), [0, 0, 0, 0, 0, 0], [5, 4, 3, 2, 1, 0], [3, 3, 4, 4, 3, 3]):
        want = check_sweep(sa, p, i, x, labels, 1.0, ("degree 0", list(labels)))
        assert want[0][3] == labels[3] and want[0][4] == labels[4]


@pytest.mark.parametrize("degree", [1, 2, 63, 64, 65, 127, 128, 129])
def test_sweep_at_the_wave_edges(sa, degree):
    """A hub of the given degree (the 64-lane loops and the power-of-two sort sizes turn at 63 / 64 / 65 and 127 / 128 / 129),
    its leaves joined in a ring so that every vertex has candidates; hub first, in the middle and last."""
    rng = np.random.default_rng(degree)
    for hub in sorted({0, degree // 2, degree}):
        n = degree + 1
        others = [v for v in range(n) if v != hub]
        pairs = [(hub, v) for v in others]
        if degree > 2:
            pairs += [(others[q], others[(q + 1) % degree]) for q in range(degree)]
        w = 0.5 + rng.random(len(pairs))
        w[rng.random(len(pairs)) < 0.3] = 1.0                   # ties among the weights too
        diag = np.where(rng.random(n) < 0.3, rng.random(n), 0.0)
        p, i, x = from_pairs(n, pairs, w, diag)
        labelings = {
            "singletons": np.arange(n),
            "one community": np.full(n, n - 1),
            "hub alone": np.where(np.arange(n) == hub, hub, others[0]),
            "few": rng.integers(0, min(4, n), n),
            "many": rng.integers(0, n, n),
        }
        for name, labels in labelings.items():
            for gamma in (1.0, 0.3):
                check_sweep(sa, p, i, x, labels, gamma, (degree, hub, name, gamma))


def test_sweep_at_the_fast_path_limit_and_one_above(sa):
    """A star whose hub has exactly as many stored entries as the fast path sorts in LDS, and one more: then the hub takes
    the slow path while its leaves take the fast one.  The limit is the build's own (sgl_louvain_info)."""
    cap = sa.louvain_info()["fast_degree"]
    assert cap >= 64
    rng = np.random.default_rng(7)
    seen = set()
    for leaves, diagonal, slow in ((cap, False, 0), (cap - 1, True, 0), (cap + 1, False, 1), (cap, True, 1), (2 * cap + 3, True, 1)):
        n = leaves + 1
        hub = n // 3
        p, i, x = star(rng, leaves, hub)
        if diagonal:                                            # the diagonal is a stored entry of the column, and no candidate
            d = np.zeros(n)
            d[hub] = 0.75
            p, i, x = from_pairs(n, [(hub, v) for v in range(n) if v != hub], 0.5 + rng.random(leaves), d)
        assert p[hub + 1] - p[hub] == leaves + int(diagonal)
        labelings = {
            "singletons": np.arange(n),                         # every neighbour in a different community
            "one community": np.where(np.arange(n) == hub, hub, (hub + 1) % n),   # all neighbours in one
            "few": rng.integers(0, 5, n),
            "many": rng.integers(0, n, n),
        }
        for name, labels in labelings.items():
            check_sweep(sa, p, i, x, labels, 1.0, (leaves, diagonal, name))
            info = sa.louvain_info()
            assert info["fast_degree"] == cap and info["slow_level0"] == slow and info["slow_coarse"] == 0, (leaves, diagonal, info)
            seen.add(slow)
    assert seen == {0, 1}                                       # both paths were run


def test_sweep_with_a_hub_on_a_coarse_level(sa):
    """Labels that make a hub: a pair of vertices tied to each of cap + 20 other pairs.  Aggregated by pair (the
    restatement's aggregation), the coarse graph has self-loops on every vertex and one column wider than the fast path;
    the sweep runs on it as the optimiser's next level would, and on the fine graph from the same labels."""
    cap = sa.louvain_info()["fast_degree"]
    m = cap + 20
    rng = np.random.default_rng(11)
    pairs, labels = [(0, 1)], [0, 0]
    for q in range(m):
        a, b = 2 + 2 * q, 3 + 2 * q
        pairs += [(a, b), (0, a), (1, b)]
        labels += [a, a]
        if q % 3 == 0 and q > 0:
            pairs.append((a, a - 2))                            # some pairs know each other
    w = 0.25 + rng.random(len(pairs))
    n = 2 + 2 * m
    p, i, x = from_pairs(n, pairs, w)
    check_sweep(sa, p, i, x, labels, 1.0, "fine graph, labels by pair")
    assert sa.louvain_info()["slow_level0"] == 2                # vertices 0 and 1 have m + 1 entries each
    cmap, (cp, ci, cx) = lr.aggregate(*lr.as_graph(p, i, x), labels)
    nc = len(cp) - 1
    assert nc == m + 1 and cp[1] - cp[0] == m + 1 and np.all(np.diff(cp)[1:] <= cap)
    for name, lab in (("singletons", np.arange(nc)), ("few", rng.integers(0, 6, nc)), ("many", rng.integers(0, nc, nc))):
        check_sweep(sa, cp, ci, cx, lab, 1.0, ("coarse", name))
        assert sa.louvain_info()["slow_level0"] == 1
    # the optimiser itself meets that hub at its second level when the first level pairs the vertices up
    got = sa.c_louvain(dgc(sa, p, i, x), [1.0])
    same_run(got, 0, lr.louvain(p, i, x, 1.0), "hub graph")


def test_a_level_wider_than_one_block_of_the_sums(sa):
    """More than 1024 vertices in one community and more than 1024 communities: the blocked sums over members and over ids
    take their second block."""
    rng = np.random.default_rng(13)
    n = 2500
    pairs = [(v, v + 1) for v in range(n - 1)] + [(v, v + 7) for v in range(0, n - 7, 3)]
    p, i, x = from_pairs(n, pairs, 0.1 + rng.random(len(pairs)))
    labels = np.where(np.arange(n) < 1300, 5, np.arange(n))     # one community of 1300, 1200 singletons
    check_sweep(sa, p, i, x, labels, 1.0, "1300 members")
    check_sweep(sa, p, i, x, np.arange(n), 1.0, "2500 ids")


# -------------------------------------------------------------------------------------------------------------- refusals
TRIANGLES = [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3)]


def refused(sa, p, i, x, column, row, text, call=None):
    with pytest.raises(sa.SingletHipError) as e:
        (call or (lambda G: sa.c_louvain(G, [1.0])))(dgc(sa, p, i, x))
    assert e.value.code == EINVAL
    if column is not None:
        assert "column %d, row %d:" % (column, row) in str(e.value), str(e.value)
    assert text in str(e.value), str(e.value)
    # the library stays usable
    gp, gi, gx = from_pairs(6, TRIANGLES, np.ones(7))
    check_sweep(sa, gp, gi, gx, np.arange(6), 1.0, "after a refusal")


def test_every_defect_is_refused_by_name_and_place(sa):
    p, i, x = from_pairs(6, TRIANGLES, np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]))
    assert p.tolist() == [0, 2, 4, 7, 10, 12, 14]
    sweep = lambda G: sa.op_louvain_sweep(G, np.arange(6), 1.0)   # noqa: E731
    # column 2 holds rows 0, 1, 3 at entries 4, 5, 6
    bad = i.copy(); bad[5], bad[6] = 3, 1                        # noqa: E702
    refused(sa, p, bad, x, 2, 1, "not strictly ascending")
    refused(sa, p, bad, x, 2, 1, "not strictly ascending", sweep)
    bad = i.copy(); bad[5] = 0                                   # noqa: E702   (a repeated row)
    refused(sa, p, bad, x, 2, 0, "not strictly ascending")
    bad = i.copy(); bad[6] = 6                                   # noqa: E702
    refused(sa, p, bad, x, 2, 6, "outside [0, n)")
    refused(sa, p, bad, x, 2, 6, "outside [0, n)", sweep)
    bad = i.copy(); bad[0] = -1                                  # noqa: E702
    refused(sa, p, bad, x, 0, -1, "outside [0, n)")
    for v in (np.nan, np.inf, -np.inf):
        bx = x.copy(); bx[9] = v                                 # noqa: E702   (column 3, its last entry: row 5)
        refused(sa, p, i, bx, 3, 5, "not finite")
        refused(sa, p, i, bx, 3, 5, "not finite", sweep)
    bx = x.copy(); bx[12] = -1e-300                              # noqa: E702   (column 5, row 3)
    refused(sa, p, i, bx, 5, 3, "negative")
    refused(sa, p, i, bx, 5, 3, "negative", sweep)
    # two defects: the first in column-major order is named
    bx = x.copy(); bx[12], bx[3] = -1.0, np.nan                  # noqa: E702   (column 1, row 2 comes first)
    refused(sa, p, i, bx, 1, 2, "not finite")
    # asymmetry: entry 6 is (3, 2), its mirror (2, 3) is entry 7
    bx = x.copy(); bx[7] = np.nextafter(x[7], 8.0)               # noqa: E702
    refused(sa, p, i, bx, 2, 3, "not symmetric")
    sa.op_louvain_sweep(dgc(sa, p, i, bx), np.arange(6), 1.0)   # the stage operator takes graphs that are not symmetric
    keep = np.arange(14) != 7                                   # the mirror missing altogether
    p2 = p.copy(); p2[4:] -= 1                                   # noqa: E702
    refused(sa, p2, i[keep], x[keep], 2, 3, "not symmetric")
    # an all-zero graph: no entries, or entries that are all zero
    refused(sa, np.zeros(7, dtype=np.int32), i[:0], x[:0], None, None, "S = 0")
    refused(sa, p, i, np.zeros(14), None, None, "S = 0")
    refused(sa, p, i, np.zeros(14), None, None, "S = 0", sweep)
    # the column pointers and the parameters, before anything is uploaded
    p3 = p.copy(); p3[2] = 1                                     # noqa: E702
    refused(sa, p3, i, x, None, None, "p decreases at column 1")
    for kw, text in ((dict(tol=-1.0), "tol"), (dict(max_sweeps=0), "max_sweeps"), (dict(max_sweeps=1025), "max_sweeps"),
                     (dict(max_levels=0), "max_levels"), (dict(max_levels=33), "max_levels")):
        refused(sa, p, i, x, None, None, text, lambda G: sa.c_louvain(G, [1.0], **kw))
    for res, text in (([], "at least one resolution"), ([1.0, 0.0], "resolution 1"), ([np.inf], "resolution 0"), ([np.nan], "resolution 0")):
        refused(sa, p, i, x, None, None, text, lambda G: sa.c_louvain(G, res))
    refused(sa, p, i, x, None, None, "label 6 of vertex 2", lambda G: sa.op_louvain_sweep(G, [0, 1, 6, 3, 4, 5], 1.0))


def test_an_empty_graph_and_an_all_isolated_graph_return_singletons(sa):
    got = sa.c_louvain(sa.dgCMatrix([], [], [0], (0, 0)), [1.0, 2.0])
    assert got["labels"].shape == (2, 0) and got["n_clusters"].tolist() == [0, 0] and got["n_levels"].tolist() == [0, 0]
    assert not got["q_levels"].any() and not got["sweeps_levels"].any()
    n = 70                                                      # every vertex only its self-loop: nobody has a neighbour
    x = 0.5 + np.random.default_rng(2).random(n)
    got = sa.c_louvain(sa.dgCMatrix(x, np.arange(n), np.arange(n + 1), (n, n)), [1.0])
    want = lr.louvain(np.arange(n + 1), np.arange(n), x, 1.0)
    same_run(got, 0, want, "self-loops only")
    assert got["labels"][0].tolist() == list(range(n)) and got["n_clusters"][0] == n and got["n_levels"][0] == 1


# -------------------------------------------------------------------------------------------------------------- workflow
def test_find_neighbors_then_find_clusters_recovers_planted_blobs(sa):
    rng = np.random.default_rng(2026)
    sizes = [520, 430, 370, 310, 230, 140]                       # n = 2000, all sizes different
    centres = 12.0 * np.eye(6)
    planted = np.repeat(np.arange(6), sizes)
    order = rng.permutation(planted.size)
    planted = planted[order]
    E = centres[planted] + 0.5 * rng.standard_normal((planted.size, 6))
    graph = sa.find_neighbors(E, k_param=20)
    out = sa.find_clusters(graph, resolution=[0.8, 0.1])
    assert out["clusters"].shape == (2000, 2) and out["clusters"].dtype == np.int32
    assert out["n_clusters"][0] == 6 and np.array_equal(out["clusters"][:, 0], planted)   # planted ids are by descending size
    for r in range(2):
        count = np.bincount(out["clusters"][:, r])
        assert count.size == out["n_clusters"][r] and np.all(np.diff(count) <= 0)
    assert 0.0 < out["modularity"][0] < 1.0 and np.all(out["levels"] >= 2)
    # the same through the raw call on the same graph, bit for bit the restatement
    G = sa.api._without_diagonal(graph["snn"])
    want = lr.louvain(G.p, G.i, G.x, 0.8)
    assert np.array_equal(out["clusters"][:, 0], want["labels"])
    assert bits(out["modularity"][0]) == bits(want["q_levels"][want["n_levels"] - 1])
