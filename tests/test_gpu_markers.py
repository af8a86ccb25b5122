"""Marker genes on the device (sgl_markers, its two stage operators and the Python layer above them; kernels_markers.hip)
against the numpy restatement (markers_restatement.py) and scipy.stats.mannwhitneyu.

  integers   pos, nz, rank2, tie and group_n equal the restatement exactly, on both rank paths and whatever the batching.
  sum        transform = 0: bit for bit in the stated order.  transform = 1 (expm1 on the device), per element against a
             long-double reference r of len summed entries: |got - r| <= (len + 1 + L) * 2^-53 * |r|: len - 1 for a sum of
             positive terms in any order, 2 of slack, L the share of the device's expm1.  L is MEASURED as L_LOG1P of
             tests/test_gpu_ingest.py was: the largest excess of err / (2^-53 |r|) over len + 1 across the cases of
             test_expm1_sums_per_element was -1.104 on an MI355X -- negative: the device's expm1 and the additions together
             stayed inside the len + 1 the sum alone is given (one-entry sums among the cases) -- so, rounded up
             and plus one, the assertion runs with L_EXPM1 = ceil(-1.104) + 1 = 0, i.e. against (len + 1) * 2^-53 |r|.
  z, p       z bit for bit against the restatement's formula on the device's integers, p within 4 spacings of math.erfc.
"""
import math

import numpy as np
import pytest
import scipy.sparse as sp
from scipy import stats

import markers_restatement as mr

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
U = 2.0 ** -53
L_EXPM1 = 0          # ceil(measured L) + 1, see the module docstring
WALK = 1024          # positions per chunk of the long path's walks (include/singlet_hip.h)
_CACHE = {}


# ------------------------------------------------------------------------------------------------------------ matrices --
class Genes:
    """A matrix given gene by gene: (values, cells) in stored order.  t(A) in CSC is then at hand for the restatement."""

    def __init__(self, n):
        self.n, self.x, self.i = n, [], []

    def add(self, x, cells):
        cells = np.asarray(cells, dtype=np.int64)
        assert cells.shape == np.shape(x) and (np.diff(cells) > 0).all() and (cells.size == 0 or cells[-1] < self.n)
        self.x.append(np.asarray(x, dtype=np.float64))
        self.i.append(cells)
        return len(self.x) - 1

    def add_random(self, rng, length, values):
        cells = np.sort(rng.choice(self.n, size=length, replace=False))
        return self.add(values(rng, length), cells)

    def csc_t(self):
        p = np.concatenate([[0], np.cumsum([len(a) for a in self.x])]).astype(np.int64)
        return np.concatenate(self.x + [np.zeros(0)]), np.concatenate(self.i + [np.zeros(0, dtype=np.int64)]).astype(np.int32), p

    def dgc(self, sa):
        x, i, p = self.csc_t()
        m = len(self.x)
        A = sp.csc_matrix((x, i, p), shape=(self.n, m)).T.tocsc()   # explicit zeros and their signs are kept
        A.sort_indices()
        assert A.nnz == x.shape[0]
        return sa.dgCMatrix(A.data.astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32), (m, self.n))


def counts(r, k):
    return r.integers(1, 5, size=k).astype(np.float64)


def positive(r, k):
    return r.random(k) * 4 + 0.01


def signed(r, k):
    return np.round(r.normal(size=k), 2) + 0.0        # negatives, ties and a few explicit zeros


def with_zeros(r, k):
    v = r.integers(1, 4, size=k).astype(np.float64)
    v[r.random(k) < 0.2] = 0.0
    v[r.random(k) < 0.05] = -0.0
    return v


def edge_matrix(cap):
    """Every loop edge of the three passes as a gene's length, and the tie runs of the long path's walk."""
    n = 8200
    rng = np.random.default_rng(20)
    g = Genes(n)
    names = {}
    for length in (0, 1, 63, 64, 65, cap - 1, cap, cap + 1, 2 * cap + 3, 8191, 8192, 8193, n):
        names["len=%d" % length] = g.add_random(rng, length, (counts, positive, signed)[len(names) % 3])
    L = 3000
    base = np.sort(rng.random(L)) + 1.0
    assert np.unique(base).size == L
    runs = base.copy()
    runs[WALK - 24:WALK] = runs[WALK - 24]            # a run that ends exactly at a chunk edge
    runs[WALK:WALK + 26] = runs[WALK]                 # one that starts exactly at it
    runs[2 * WALK - 8:2 * WALK + 12] = runs[2 * WALK - 8]   # one that straddles the next
    for key, vals in (("runs at chunk edges", runs), ("one run", np.full(L, 2.5)), ("all distinct", base)):
        cells = np.sort(rng.choice(n, size=L, replace=False))
        names[key] = g.add(vals[rng.permutation(L)], cells)
    names["negative run over an edge"] = g.add(-runs[rng.permutation(L)], np.sort(rng.choice(n, size=L, replace=False)))
    names["zeros stored"] = g.add_random(rng, 2500, with_zeros)
    return g, names


def mixed_matrix():
    """A few dozen genes of every kind on 3000 cells, two of them long."""
    n = 3000
    rng = np.random.default_rng(21)
    g = Genes(n)
    for q in range(36):
        length = int(rng.integers(0, 900)) if q < 32 else (2100, 3000, 2049, 2500)[q - 32]
        g.add_random(rng, length, (counts, positive, signed, with_zeros)[q % 4])
    return g


def labels_for(n, G, kind="random"):
    rng = np.random.default_rng(100 + G)
    if kind == "two cells":
        l = np.full(n, -1, dtype=np.int32)
        l[[5, n - 3]] = [0, 1]
        return l
    l = rng.integers(0, G, size=n).astype(np.int32)
    l[rng.random(n) < 0.05] = -1                        # cells left out
    if G >= 3:
        l[l == 1] = 2                                   # a cluster with no cell
    return l


def reference(key, g, labels, G, transform):
    k = (key, G, transform, labels.tobytes())
    if k not in _CACHE:
        _CACHE[k] = mr.markers(*g.csc_t(), labels, G, transform, 1.0)
    return _CACHE[k]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def check_derived(out, G):
    """z bit for bit and p within 4 spacings of the restatement's formulas on the DEVICE's integers and sums."""
    m = out["p"].shape[0]
    for gi in range(m):
        d = mr.derive(out["group_n"], out["pos"][gi], out["sum"][gi], out["rank2"][gi], int(out["tie"][gi]), 1.0)
        assert same_bits(np.ascontiguousarray(out["z"][gi]), d["z"]), gi
        assert same_bits(np.ascontiguousarray(out["pct_in"][gi]), d["pct_in"]) and same_bits(np.ascontiguousarray(out["pct_out"][gi]), d["pct_out"]), gi
        nan = np.isnan(d["p"])
        assert np.array_equal(np.isnan(out["p"][gi]), nan), gi
        assert np.all(np.abs(out["p"][gi][~nan] - d["p"][~nan]) <= 4 * np.spacing(d["p"][~nan])), gi
        fnan = ~np.isfinite(d["log2fc"])          # a mean of -pseudocount or below (negative values): -inf or NaN on both sides
        assert np.array_equal(out["log2fc"][gi][fnan], d["log2fc"][fnan], equal_nan=True) and np.isfinite(out["log2fc"][gi][~fnan]).all(), gi
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_in = out["sum"][gi] / out["group_n"]
            bound = 4 * U * (np.abs(np.log2(mean_in + 1.0)) + np.abs(d["log2fc"]) + 1.0)
        assert np.all(np.abs(out["log2fc"][gi][~fnan] - d["log2fc"][~fnan]) <= bound[~fnan]), gi


def check_all(ctx, ref, labels, G, transform_name="identity"):
    pos, nz, s = ctx.op_marker_sums(labels, G, transform_name)
    rank2, tie = ctx.op_marker_ranks(labels, G)
    assert np.array_equal(pos, ref["pos"]) and np.array_equal(nz, ref["nz"])
    assert np.array_equal(rank2, ref["rank2"]), np.argwhere(rank2 != ref["rank2"])[:5]
    assert tie.dtype == np.uint64 and np.array_equal(tie, ref["tie"])
    N = int(ref["group_n"].sum())
    assert np.all(rank2.sum(axis=1) == N * (N + 1))
    if transform_name == "identity":
        assert same_bits(np.ascontiguousarray(s), ref["sum"])
    out = ctx.markers(labels, G, transform_name, 1.0)
    assert np.array_equal(out["group_n"], ref["group_n"])
    for k, v in (("pos", pos), ("sum", s), ("rank2", rank2), ("tie", tie)):
        assert same_bits(np.ascontiguousarray(out[k]), np.ascontiguousarray(v)), k
    check_derived(out, G)
    return out


# --------------------------------------------------------------------------------------------------------- loop edges --
def test_every_loop_edge_and_tie_run_equals_the_restatement(sa, ctx):
    ctx.upload(sa.dgCMatrix.from_dense(np.eye(3)))
    ctx.op_marker_ranks(np.zeros(3, dtype=np.int32), 1)
    cap = ctx.markers_info()["lds_cap"]
    assert cap >= 256 and cap & (cap - 1) == 0
    g, names = edge_matrix(cap)
    ctx.upload(g.dgc(sa))
    labels = (np.arange(g.n) % 3).astype(np.int32)     # every cell included: a gene's length is its sort length
    ref = reference("edges", g, labels, 3, 0)
    check_all(ctx, ref, labels, 3)
    info = ctx.markers_info()
    lens = np.array([len(a) for a in g.x])
    nzlen = ref["nz"].sum(axis=1)
    assert info["lds_genes"] == int(np.sum(nzlen <= cap)) and info["long_genes"] == int(np.sum(nzlen > cap)) >= 8
    assert info["lds_genes"] >= 8 and info["batches"] == 1
    assert nzlen[names["len=%d" % cap]] == cap and nzlen[names["len=%d" % (cap + 1)]] == cap + 1
    assert lens[names["len=8193"]] == mr.SEG + 1
    # the all-tied long gene: one run over the whole gene
    one = names["one run"]
    assert int(ref["tie"][one]) == 3000**3 - 3000 + (g.n - 3000)**3 - (g.n - 3000)
    # forcing batches: >= 3 of them, one gene above the cap alone, and not a bit changes
    rank2, tie = ctx.op_marker_ranks(labels, 3)
    r2b, tb = ctx.op_marker_ranks(labels, 3, max_batch_entries=5000)
    info = ctx.markers_info()
    assert info["batches"] >= 3 and int(nzlen.max()) > 5000 and info["long_genes"] >= 8
    assert same_bits(r2b, rank2) and same_bits(tb, tie)
    # excluded cells shorten the sort length: the same matrix, other paths
    labels2 = labels.copy()
    labels2[np.random.default_rng(3).random(g.n) < 0.6] = -1
    ref2 = reference("edges", g, labels2, 3, 0)
    check_all(ctx, ref2, labels2, 3)
    assert ctx.markers_info()["lds_genes"] > int(np.sum(nzlen <= cap))


@pytest.mark.parametrize("G", [1, 2, 3, 64, 65, 1024])
def test_cluster_counts(sa, ctx, G):
    g = mixed_matrix()
    ctx.upload(g.dgc(sa))
    labels = labels_for(g.n, G)
    ref = reference("mixed", g, labels, G, 0)
    if G >= 3:
        assert ref["group_n"][1] == 0
    out = check_all(ctx, ref, labels, G)
    if G >= 3:
        assert np.isnan(out["p"][:, 1]).all() and np.isnan(out["pct_in"][:, 1]).all()
    if G == 1:
        assert np.isnan(out["p"]).all()                # no rest to test against
    info = ctx.markers_info()
    assert info["lds_genes"] > 0 and info["long_genes"] > 0


def test_all_cells_left_out_but_two(sa, ctx):
    g = mixed_matrix()
    ctx.upload(g.dgc(sa))
    labels = labels_for(g.n, 2, "two cells")
    ref = reference("mixed", g, labels, 2, 0)
    assert ref["group_n"].tolist() == [1, 1]
    check_all(ctx, ref, labels, 2)
    assert ctx.markers_info()["long_genes"] == 0


# ------------------------------------------------------------------------------------------------------- expm1 sums --
def test_expm1_sums_per_element(sa, ctx):
    """See the module docstring for the bound.  On an MI355X the largest excess of err / (2^-53 |r|) over len + 1 was -1.104
    and the largest fraction of the bound (len + 1 + L_EXPM1) * 2^-53 |r| 0.4482."""
    n = 9000
    rng = np.random.default_rng(30)
    g = Genes(n)
    for length in (1, 1, 1, 2, 3, 63, 64, 65, 700, 2049, 8191, 8192, 8193, n) + (1,) * 20:
        g.add_random(rng, length, lambda r, k: r.random(k) * 6 + 1e-3)   # log-normalised values: positive
    ctx.upload(g.dgc(sa))
    G = 4
    labels = rng.integers(-1, G, size=n).astype(np.int32)
    pos, nz, s = ctx.op_marker_sums(labels, G, "expm1")
    ref = reference("expm1", g, labels, G, 1)
    assert np.array_equal(pos, ref["pos"]) and np.array_equal(nz, ref["nz"])
    worst_excess, worst_frac = -np.inf, 0.0
    for gi in range(len(g.x)):
        r, ln = mr.group_sums_reference(g.x[gi], g.i[gi], labels, G, 1)
        live = ln > 0
        assert np.all(s[gi][~live] == 0.0) and not np.signbit(s[gi][~live]).any()
        q = (np.abs(s[gi][live].astype(np.longdouble) - r[live]) / (np.longdouble(U) * np.abs(r[live]))).astype(np.float64)
        if q.size:
            worst_excess = max(worst_excess, float((q - (ln[live] + 1)).max()))
            worst_frac = max(worst_frac, float((q / (ln[live] + 1 + L_EXPM1)).max()))
        assert np.all(q <= ln[live] + 1 + L_EXPM1), (gi, q, ln[live])
    print("markers-figure expm1 sums: excess over len + 1 = %.3f, largest fraction of the bound = %.4f" % (worst_excess, worst_frac))


# -------------------------------------------------------------------------------------------- forms, fits, dense upload --
def test_the_forms_give_identical_bits(sa, ctx):
    g = mixed_matrix()
    A = g.dgc(sa)
    labels = labels_for(g.n, 5)
    ctx.upload(A)
    a = ctx.markers(labels, 5)
    b = ctx.markers(labels, 5)
    c = sa.c_markers(A, labels, 5)
    with sa.Context(0) as other:
        other.upload(A)
        d = other.markers(labels)             # n_groups from the labels
    pos, nz, s = ctx.op_marker_sums(labels, 5, "expm1")
    rank2, tie = ctx.op_marker_ranks(labels, 5)
    for k in a:
        for o in (b, c, d):
            assert same_bits(np.ascontiguousarray(a[k]), np.ascontiguousarray(o[k])), k
    assert same_bits(np.ascontiguousarray(a["sum"]), np.ascontiguousarray(s)) and same_bits(np.ascontiguousarray(a["rank2"]), np.ascontiguousarray(rank2))
    assert same_bits(a["tie"], tie) and same_bits(np.ascontiguousarray(a["pos"]), np.ascontiguousarray(pos))
    # any output pointer may be NULL
    import ctypes as C
    L = sa._lib.load()
    p = np.empty((5, A.nrow))
    lab = np.ascontiguousarray(labels)
    rc = L.sgl_markers(ctx._h, lab.ctypes.data_as(C.POINTER(C.c_int32)), 5, 1, 1.0, None, None, None, None, None, None, None, None, None,
                       p.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0 and same_bits(np.ascontiguousarray(p.T), np.ascontiguousarray(a["p"]))


def test_a_call_after_upload_dense_works(sa, ctx):
    rng = np.random.default_rng(8)
    D = np.where(rng.random((30, 500)) < 0.3, np.round(rng.random((30, 500)) * 3, 2), 0.0)
    labels = rng.integers(-1, 3, size=500).astype(np.int32)
    with sa.Context(0) as c:
        c.upload_dense(D)
        a = c.markers(labels, 3)
    b = sa.c_markers(sa.dgCMatrix.from_dense(D), labels, 3)
    for k in a:
        assert same_bits(np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])), k
    T = sp.csc_matrix(D.T)
    ref = mr.markers(T.data, T.indices, T.indptr, labels, 3, 1, 1.0)
    assert np.array_equal(a["rank2"], ref["rank2"]) and np.array_equal(a["tie"], ref["tie"]) and np.array_equal(a["pos"], ref["pos"])


def _same(fa, fb, what):
    for x, y in zip(fa, fb):
        assert same_bits(np.ascontiguousarray(x), np.ascontiguousarray(y)), what


def test_a_fit_continued_after_a_call_gives_the_same_bits(sa):
    m, n, k = 120, 12000, 12     # genes of about 3000 entries: the long path
    labels = (np.arange(n) % 7 - 1).astype(np.int32)
    runs = {}
    for with_call in (False, True):
        with sa.Context(0) as c:
            c.synth(m, n, 4)
            c.fit_init(k)
            c.sweeps_get(reset=True)
            tols = [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            if with_call:
                before = c.get_factors()
                x0 = c.download(1)
                out = c.markers(labels, 6)
                c.op_marker_ranks(labels, 6, max_batch_entries=1)
                _same(c.get_factors(), before, "factors")
                _same(c.download(1), x0, "matrix")
                assert out["p"].shape == (m, 6) and c.markers_info()["long_genes"] > 0
            tols += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            runs[with_call] = (c.get_factors(), tols, c.sweeps_get(reset=True))
    _same(runs[True][0], runs[False][0], "fit")
    assert runs[True][1] == runs[False][1]
    for key in ("h_sweeps", "w_sweeps"):
        assert runs[True][2][key] == runs[False][2][key], key


# ----------------------------------------------------------------------------------------------------------- refusals --
def test_refusals_return_their_code_and_leave_the_context_usable(sa):
    g = mixed_matrix()
    A = g.dgc(sa)
    n = g.n
    labels = labels_for(n, 4)
    ref = reference("mixed", g, labels, 4, 0)

    def refused(c, code, match, fn):
        dims = c.dims()
        with pytest.raises(sa.SingletHipError, match=match) as e:
            fn()
        assert e.value.code == code and c.dims() == dims

    with sa.Context(0) as c:
        refused(c, ESTATE, "no matrix resident", lambda: c.markers(labels, 4))
        refused(c, ESTATE, "no matrix resident", lambda: c.op_marker_sums(labels[:0], 4))
        refused(c, ESTATE, "no matrix resident", lambda: c.op_marker_ranks(labels[:0], 4))
        c.upload(A)
        bad = labels.copy()
        bad[77], bad[900] = 4, -2
        refused(c, EINVAL, r"labels\[77\] = 4", lambda: c.markers(bad, 4))
        bad[77] = 0
        refused(c, EINVAL, r"labels\[900\] = -2", lambda: c.op_marker_ranks(bad, 4))
        refused(c, EINVAL, r"labels\[900\] = -2", lambda: c.op_marker_sums(bad, 4))
        refused(c, EINVAL, "n_groups", lambda: c.markers(np.zeros(n, dtype=np.int32), 0))
        refused(c, EINVAL, "n_groups", lambda: c.markers(np.zeros(n, dtype=np.int32), 1025))
        for pc in (-1.0, float("nan"), float("inf")):
            refused(c, EINVAL, "pseudocount", lambda: c.markers(labels, 4, pseudocount=pc))
        refused(c, EINVAL, "max_batch_entries", lambda: c.op_marker_ranks(labels, 4, max_batch_entries=-1))
        import ctypes as C
        L = sa._lib.load()
        lp = labels.ctypes.data_as(C.POINTER(C.c_int32))
        none = (None,) * 10
        assert L.sgl_markers(c._h, lp, 4, 2, 1.0, *none) == EINVAL and b"transform" in L.sgl_last_error()
        assert L.sgl_markers(c._h, None, 4, 1, 1.0, *none) == EINVAL
        assert L.sgl_markers_info(c._h, None) == EINVAL
        c.set_allreduce(lambda dev_ptr, count: None)
        refused(c, ESTATE, "all-reduce hook", lambda: c.markers(labels, 4))
        c.set_allreduce(None)
        c.upload(A, None, cell_offset=n, ncells_total=3 * n)
        refused(c, ESTATE, "shard", lambda: c.markers(labels, 4))
        c.upload(A)
        out = c.markers(labels, 4, "identity")
        assert np.array_equal(out["rank2"], ref["rank2"]) and same_bits(np.ascontiguousarray(out["sum"]), ref["sum"])
        # more than 2^21 cells: the tie term would not fit
        wide = sa.dgCMatrix(np.ones(1), np.zeros(1, dtype=np.int32), np.concatenate([[0], np.ones((1 << 21) + 1)]).astype(np.int32),
                            (2, (1 << 21) + 1))
        c.upload(wide)
        refused(c, EINVAL, "2\\^21", lambda: c.markers(np.zeros((1 << 21) + 1, dtype=np.int32), 1))
        c.upload(A)
        assert np.array_equal(c.markers(labels, 4)["tie"], ref["tie"])
    with sa.Multi([0, 0]) as M:
        M.upload(A)
        with pytest.raises(sa.SingletHipError, match="team") as e:
            M.rank_ctx(0).markers(labels[:M.rank_ctx(0).dims()[1]], 4)
        assert e.value.code == ESTATE
    # the one-shot form refuses its arguments before anything is uploaded
    with pytest.raises(sa.SingletHipError, match=r"labels\[900\] = -2") as e:
        sa.c_markers(A, bad, 4)
    assert e.value.code == EINVAL


# -------------------------------------------------------------------------------------------------------------- pbmc3k --
def _pbmc3k(sa):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = np.load(os.path.join(root, "tests", "golden", "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)          # row indices are stored as within-column deltas
    for c in range(dim[1]):
        i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
    return sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])))


def test_pbmc3k_end_to_end(sa):
    counts_m = _pbmc3k(sa)
    A = sa.PreprocessData(counts_m)
    fit = sa.run_nmf(A, rank=10, tol=1e-4, maxit=100, verbose=False, L1=0.01, seed=123)
    graph = sa.find_neighbors(fit["h"].T, k_param=20)
    clusters = sa.find_clusters(graph, resolution=0.8)["clusters"][:, 0]
    G = int(clusters.max()) + 1
    assert G >= 3
    st = sa.c_markers(A, clusters)
    m, n = A.nrow, A.ncol
    S = sp.csc_matrix((A.x, A.i, A.p), shape=(m, n)).tocsr()
    detected = np.diff(S.indptr)
    order = np.argsort(detected, kind="stable")
    order = order[detected[order] > 0]
    genes = order[np.linspace(0, order.size - 1, 40).astype(np.int64)]   # spread over the detection range
    compared = 0
    for gi in genes:
        row = np.asarray(S[gi].todense()).ravel()
        for c in range(G):
            a, b = row[clusters == c], row[clusters != c]
            assert st["pct_in"][gi, c] == np.sum(a > 0) / a.size and st["pct_out"][gi, c] == np.sum(b > 0) / b.size
            ref = stats.mannwhitneyu(a, b, use_continuity=True, alternative="two-sided", method="asymptotic").pvalue
            got = st["p"][gi, c]
            if ref >= 1e-300:
                assert abs(got - ref) <= 1e-12 * ref, (gi, c, got, ref)
                compared += 1
    assert compared >= 40 * G - 5
    tables = sa.find_all_markers(A, clusters)
    assert len(tables) == G
    some = 0
    for c, t in enumerate(tables):
        p, fc, p1, p2 = st["p"][:, c], st["log2fc"][:, c], st["pct_in"][:, c], st["pct_out"][:, c]
        keep = (np.maximum(p1, p2) >= 0.1) & (np.abs(fc) >= 0.25) & (p < 0.01)
        assert t["cluster"] == c and np.array_equal(np.sort(t["gene"]), np.nonzero(keep)[0])
        gsel = t["gene"]
        assert np.array_equal(t["p_val"], p[gsel]) and np.array_equal(t["avg_log2FC"], fc[gsel])
        assert np.array_equal(t["pct_1"], p1[gsel]) and np.array_equal(t["pct_2"], p2[gsel])
        assert np.array_equal(t["p_val_adj"], np.minimum(1.0, p[gsel] * m))
        keys = list(zip(t["p_val"].tolist(), (-t["avg_log2FC"]).tolist(), gsel.tolist()))
        assert keys == sorted(keys)
        some += gsel.size
        pos_only = sa.find_all_markers(A, clusters, only_pos=True)[c] if c == 0 else None
        if pos_only is not None:
            assert np.array_equal(np.sort(pos_only["gene"]), np.nonzero(keep & (fc >= 0.25))[0])
    assert some > 100
    with sa.Context(0) as c:               # a Context that holds the matrix is taken as it is, and stays as it was
        c.upload(A)
        again = sa.find_all_markers(c, clusters)
        assert c.dims() == (m, n, A.nnz)
    for t, u in zip(tables, again):
        assert np.array_equal(t["gene"], u["gene"]) and np.array_equal(t["p_val"], u["p_val"]) and np.array_equal(t["avg_log2FC"], u["avg_log2FC"])
    # FindMarkers(ident.1 = 0, ident.2 = 1) is the labels {0, 1, -1}
    lab = np.where(clusters == 0, 0, np.where(clusters == 1, 1, -1)).astype(np.int32)
    pair = sa.c_markers(A, lab, 2)
    t = sa.find_markers(A, np.nonzero(clusters == 0)[0], np.nonzero(clusters == 1)[0])
    keep = (np.maximum(pair["pct_in"][:, 0], pair["pct_out"][:, 0]) >= 0.1) & (np.abs(pair["log2fc"][:, 0]) >= 0.25) & (pair["p"][:, 0] < 0.01)
    assert np.array_equal(np.sort(t["gene"]), np.nonzero(keep)[0]) and np.array_equal(t["p_val"], pair["p"][t["gene"], 0])
