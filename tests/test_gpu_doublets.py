"""Simulated doublets and doublet scores on the device (sgl_simulate_doublets, sgl_op_pair_columns, sgl_doublets_info and the
Python layer above them; kernels_doublet.hip) against the numpy restatement (doublet_restatement.py).  The merge moves bits and
makes one IEEE addition per shared row: every comparison of S is on bytes, on both paths.  The edge matrix is the smallest at
which each loop can turn wrong; the restatement of a case is computed once and shared."""
import os

import numpy as np
import pytest

import doublet_restatement as rs
from planted_doublets import planted
from test_gpu_caller_stream import bits_differ, caller_stream, contexts, the_stall

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROW, CAP, DEFAULT_CAP = 2100, 128, 4096
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_csc_bits(got, want, what):
    for name, g, w in zip("xip", got, want[:3]):
        assert same_bits(g, w), "%s: %s differs" % (what, name)


# ------------------------------------------------------------------------------------------------------- the edge matrix
def edge():
    """(x, i, p, names): 64 columns of 2100 rows, built by length and by how their rows meet."""
    def make():
        rng = np.random.default_rng(42)
        cols, names = [], {}

        def add(name, rows, x=None):
            rows = np.asarray(rows, dtype=np.int64)
            assert rows.size == 0 or (np.all(np.diff(rows) > 0) and rows[-1] < NROW)
            x = rng.integers(1, 50, size=rows.size).astype(np.float64) if x is None else np.asarray(x, dtype=np.float64)
            names[name] = len(cols)
            cols.append((rows, x))

        def rand(n):
            return np.sort(rng.choice(NROW, size=n, replace=False))
        for n in (0, 1, 63, 64, 65, CAP - 1, CAP, CAP + 1, 1996, 1997):       # 1996 / 1997 + the full column: 4096 / 4097
            add("len%d" % n, rand(n))
        add("full", np.arange(NROW))
        add("evens", np.arange(0, 128, 2))
        add("odds", np.arange(1, 128, 2))                                      # interleaved with evens, disjoint: union 128
        add("evens2", np.arange(0, 128, 2))                                    # the identical row set
        add("evens_neg", np.arange(0, 128, 2), -cols[names["evens"]][1])       # x and -x: every sum a stored zero
        add("evens_half", np.arange(0, 128, 4))                                # a subset of evens
        add("low", np.arange(0, 50))
        add("high", np.arange(1000, 1063))                                     # all rows of low below all rows of high
        add("last_a", [3, 700, NROW - 1])
        add("last_b", [4, NROW - 1])                                           # row nrow - 1 shared
        add("zeros", [10, 20, 30, 40], [0.0, -0.0, 7.0, 0.0])                  # explicit stored zeros of either sign
        add("zeros_mate", [10, 21, 40], [0.0, 2.0, -0.0])
        add("a32", np.arange(0, 32))
        add("b32", np.arange(32, 64))                                          # union with a32: 64
        add("b32_1", np.arange(31, 63))                                        # union with a32: 63 (one shared)
        add("b33", np.arange(32, 65))                                          # union with a32: 65
        while len(cols) < 64:
            add("r%d" % len(cols), rand(int(rng.integers(0, 300))))
        x = np.concatenate([c[1] for c in cols])
        i = np.concatenate([c[0] for c in cols]).astype(np.int32)
        p = np.concatenate([[0], np.cumsum([c[0].size for c in cols])]).astype(np.int32)
        return x, i, p, names
    return cached("edge", make)


def edge_pairs():
    """The named pairs, then random ones with repeats up to 5 000: more columns than one launch has workgroups."""
    def make():
        _, _, _, n = edge()
        named = [("len0", "len0"), ("len0", "len65"), ("len1", "len0"), ("len64", "len64"), ("full", "full"), ("evens", "odds"),
                 ("evens", "evens2"), ("evens", "evens_half"), ("evens_half", "evens"), ("low", "high"), ("high", "low"),
                 ("last_a", "last_b"), ("evens", "evens_neg"), ("zeros", "zeros_mate"), ("zeros", "len0"), ("a32", "b32"),
                 ("a32", "b32_1"), ("a32", "b33"), ("len63", "len64"), ("len64", "len65"), ("len63", "len65"),
                 ("len%d" % (CAP - 1), "len0"), ("len%d" % CAP, "len0"), ("len%d" % (CAP + 1), "len0"), ("len%d" % (CAP - 1), "len1"),
                 ("full", "len1996"), ("full", "len1997"), ("len1997", "full"), ("full", "len0"), ("full", "evens"), ("len1", "len1")]
        rng = np.random.default_rng(43)
        pa = np.concatenate([[n[a] for a, _ in named], rng.integers(0, 64, size=5000 - len(named))]).astype(np.int32)
        pb = np.concatenate([[n[b] for _, b in named], rng.integers(0, 64, size=5000 - len(named))]).astype(np.int32)
        return pa, pb
    return cached("pairs", make)


def edge_want():
    def make():
        x, i, p, _ = edge()
        return rs.pair_columns(x, i, p, *edge_pairs())
    return cached("want", make)


def upload_edge(sa, c):
    x, i, p, _ = edge()
    c.upload(sa.dgCMatrix(x, i, p, (NROW, 64)), None)


def transpose_slots(x, i, p, nrow):
    """(x, i, p) of t(S) as the device transpose leaves it: the entries of a row in ascending column order."""
    cols = np.repeat(np.arange(p.shape[0] - 1, dtype=np.int32), np.diff(p))
    order = np.argsort(i, kind="stable")
    tp = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=nrow))]).astype(np.int64)
    return x[order], cols[order], tp


# -------------------------------------------------------------------------------------------------------- the merge
@pytest.mark.parametrize("lds_cap", [0, CAP, 1])
def test_merge_bit_for_bit_on_both_paths(sa, lds_cap):
    """op_pair_columns at the default cap, at a cap of 128 that splits the edge matrix between the paths, and at 1, which sends
    everything but a pair of at most one entry down the long path: S bit for bit, and the info call shows what ran."""
    x, i, p, _ = edge()
    pa, pb = edge_pairs()
    want = edge_want()
    with sa.Context(0) as c:
        upload_edge(sa, c)
        got = c.op_pair_columns(pa, pb, lds_cap)
        info = c.doublets_info()
        assert c.dims() == (NROW, 64, int(p[-1])) and same_bits(c.download(0)[0], x)      # the context is only read
    assert got[2].dtype == np.int64 and got[1].dtype == np.int32
    assert_csc_bits(got, want, "lds_cap %d" % lds_cap)
    n_lds, n_long = rs.path_counts(p, pa, pb, lds_cap or DEFAULT_CAP)
    assert n_lds > 0 and n_long > 0
    assert info == {"lds_pairs": n_lds, "long_pairs": n_long, "entries": int(want[2][-1]), "shared_rows": want[3]}
    if lds_cap == 1:
        assert n_long >= 4990


def test_merge_of_a_single_pair_and_of_prefixes(sa):
    x, i, p, n = edge()
    pa, pb = edge_pairs()
    with sa.Context(0) as c:
        upload_edge(sa, c)
        for a, b in ((n["evens"], n["odds"]), (n["len0"], n["len0"]), (n["full"], n["full"])):
            assert_csc_bits(c.op_pair_columns([a], [b], CAP), rs.pair_columns(x, i, p, [a], [b]), "n_sim = 1")
        for cut in (2, 31, 65):
            assert_csc_bits(c.op_pair_columns(pa[:cut], pb[:cut]), rs.pair_columns(x, i, p, pa[:cut], pb[:cut]), "n_sim = %d" % cut)
        big = c.op_pair_columns(pa, pb, 4097)                        # a cap above the default is the default
        assert c.doublets_info()["lds_pairs"] == rs.path_counts(p, pa, pb, DEFAULT_CAP)[0]
    assert_csc_bits(big, edge_want(), "cap above the default")


def test_simulate_leaves_dst_as_an_upload_of_s_would(sa):
    x, i, p, _ = edge()
    pa, pb = edge_pairs()
    sx, si, sp, shared = edge_want()
    with sa.Context(0) as src, sa.Context(0) as dst:
        upload_edge(sa, src)
        src.simulate_doublets(dst, pa, pb)
        assert dst.dims() == (NROW, 5000, int(sp[-1])) and dst.k == 0
        assert_csc_bits(dst.download(0), (sx, si, sp), "A of dst")
        assert_csc_bits(dst.download(1), transpose_slots(sx, si, sp, NROW), "t(A) of dst")
        n_lds, n_long = rs.path_counts(p, pa, pb, DEFAULT_CAP)
        assert dst.doublets_info() == {"lds_pairs": n_lds, "long_pairs": n_long, "entries": int(sp[-1]), "shared_rows": shared}
        assert np.array_equal(dst.col_counts(0), np.diff(sp)) and np.array_equal(dst.col_counts(1), np.bincount(si, minlength=NROW))
        assert src.dims() == (NROW, 64, int(p[-1]))
        assert_csc_bits(src.download(0), (x, i, p.astype(np.int64)), "src afterwards")
        # a second call replaces S; one pair is a matrix too
        src.simulate_doublets(dst, pa[:1], pb[:1])
        assert dst.dims()[:2] == (NROW, 1)


# ------------------------------------------------------------------------------------------------------------ state
def small_problem(sa, ora):
    def make():
        A = ora.synth_csc(300, 500, 10)
        return A, sa.dgCMatrix(A.x, A.i, A.p, (A.nrow, A.ncol)), np.ascontiguousarray(ora.synth_winit(6, A.nrow))
    return cached("small", make)


def iterate(c, n):
    for _ in range(n):
        c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
    return c.get_factors()


def test_src_continues_its_fit_and_dst_fits_like_an_upload(sa, ora):
    A, dA, w0 = small_problem(sa, ora)
    pa, pb = rs.parents(500, 700, 5)
    sx, si, sp, _ = rs.pair_columns(A.x, A.i, A.p, pa, pb)
    with sa.Context(0) as ref:
        ref.upload(dA, None)
        ref.fit_init(6, w0)
        want_src = iterate(ref, 4)
        ref.upload(sa.dgCMatrix(sx, si, sp.astype(np.int32), (300, 700)), None)
        ref.fit_init(6, w0)
        want_dst = iterate(ref, 3)
    with sa.Context(0) as src, sa.Context(0) as dst:
        src.upload(dA, None)
        src.fit_init(6, w0)
        iterate(src, 2)
        dst.upload(dA, None)                                        # dst holds a matrix and a fit of its own: both are dropped
        dst.fit_init(4, None)
        iterate(dst, 1)
        src.simulate_doublets(dst, pa, pb)
        assert dst.k == 0 and dst.dims() == (300, 700, int(sp[-1]))
        with pytest.raises(sa.SingletHipError) as e:
            dst.get_factors()
        assert e.value.code == ESTATE                               # the previous fit of dst is gone
        assert not bits_differ(iterate(src, 2), want_src), "src did not continue its fit to the bits"
        assert_csc_bits(src.download(0), (A.x, A.i, A.p.astype(np.int64)), "src")
        dst.fit_init(6, w0)
        assert not bits_differ(iterate(dst, 3), want_dst), "the fit on dst is not the fit on an upload of S"


# --------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_leaves_both_contexts_as_they_were(sa, ora):
    A, dA, w0 = small_problem(sa, ora)
    ok = np.array([0, 1, 2], dtype=np.int32)
    with sa.Context(0) as src, sa.Context(0) as dst, sa.Context(0) as empty:
        src.upload(dA, None)
        dst.upload(dA, None)
        dst.fit_init(6, w0)
        before = (src.download(0), dst.download(0), dst.get_factors())

        def refused(code, fragment, call):
            with pytest.raises(sa.SingletHipError) as e:
                call()
            assert e.value.code == code and fragment in str(e.value), str(e.value)
            assert not bits_differ((src.download(0), dst.download(0), dst.get_factors()), before), fragment
        refused(ESTATE, "one context", lambda: src.simulate_doublets(src, ok, ok))
        refused(ESTATE, "no matrix resident in src", lambda: empty.simulate_doublets(dst, ok, ok))
        refused(EINVAL, "n_sim = 0", lambda: src.simulate_doublets(dst, [], []))
        refused(EINVAL, "parent_a is NULL", lambda: src.simulate_doublets(dst, None, ok))
        refused(EINVAL, "parent_b is NULL", lambda: src.simulate_doublets(dst, ok, None))
        refused(EINVAL, "parent_b[1] = 500 is outside [0, ncol = 500)", lambda: src.simulate_doublets(dst, ok, [0, 500, -1]))
        refused(EINVAL, "parent_a[2] = -1", lambda: src.simulate_doublets(dst, [0, 499, -1], [0, 499, 500]))
        refused(EINVAL, "lds_cap = -1", lambda: src.op_pair_columns(ok, ok, -1))
        refused(EINVAL, "parent_a[0] = 500", lambda: src.op_pair_columns([500], [0]))
        refused(ESTATE, "no matrix resident", lambda: empty.op_pair_columns(ok, ok))
        hook = lambda ptr, count: 0
        src.set_allreduce(hook)
        refused(ESTATE, "src is a member of a team or has an all-reduce hook", lambda: src.simulate_doublets(dst, ok, ok))
        refused(ESTATE, "all-reduce hook", lambda: src.op_pair_columns(ok, ok))
        src.set_allreduce(None)
        dst.set_allreduce(hook)
        refused(ESTATE, "dst is a member of a team or has an all-reduce hook", lambda: src.simulate_doublets(dst, ok, ok))
        dst.set_allreduce(None)
        with pytest.raises(ValueError):
            src.simulate_doublets(dst, ok, ok[:2])
        with pytest.raises(TypeError):
            src.simulate_doublets(None, ok, ok)
    with sa.Context(0) as shard, sa.Context(0) as dst:
        shard.upload(dA, None, cell_offset=100, ncells_total=1000)
        dst.upload(dA, None)
        for call, role in ((lambda: shard.simulate_doublets(dst, ok, ok), "src holds a shard"),
                           (lambda: dst.simulate_doublets(shard, ok, ok), "dst holds a shard"),
                           (lambda: shard.op_pair_columns(ok, ok), "the context holds a shard")):
            with pytest.raises(sa.SingletHipError) as e:
                call()
            assert e.value.code == ESTATE and role in str(e.value)
        assert shard.dims()[:2] == (300, 500) and dst.dims()[:2] == (300, 500)


def test_an_overflowing_sum_leaves_dst_empty_and_src_intact(sa):
    x = np.array([1.0, 1e308, 2.0, 1e308, 3.0])
    i = np.array([0, 2, 1, 2, 2], dtype=np.int32)
    p = np.array([0, 2, 4, 5], dtype=np.int32)
    with sa.Context(0) as src, sa.Context(0) as dst:
        src.upload(sa.dgCMatrix(x, i, p, (3, 3)), None)
        dst.upload(sa.dgCMatrix(x, i, p, (3, 3)), None)
        with pytest.raises(sa.SingletHipError) as e:
            src.simulate_doublets(dst, [0, 2, 0, 1], [2, 2, 1, 0])
        assert e.value.code == EINVAL and "simulated column 2" in str(e.value) and "non-finite" in str(e.value)
        assert dst.dims() == (0, 0, 0)
        assert_csc_bits(src.download(0), (x, i, p.astype(np.int64)), "src")
        sx, si, sp = src.op_pair_columns([0, 2, 0], [2, 2, 1])      # the operator returns the sum as it is
        assert np.isinf(sx[-1]) and sp.tolist() == [0, 2, 3, 6]
        src.simulate_doublets(dst, [0, 2], [2, 2])                  # and dst takes the next call
        assert dst.dims() == (3, 2, 3)


# ---------------------------------------------------------------------------------------------------------- streams
def test_stalled_streams_on_either_side_give_the_private_stream_bits(sa, ora):
    """The call between two rewrites of src (a log_normalize before it, one right after it), with a spin pending at the tail
    of the caller's stream of dst, of src, or of both (two different streams) when the call is made and again when the second
    rewrite is: dst is S of the matrix normalised ONCE, src ends up normalised twice, to the bits of the private-stream run."""
    A, dA, _ = small_problem(sa, ora)
    pa, pb = rs.parents(500, 900, 9)

    def run(src, dst, stall=lambda: None):
        src.upload(dA, None)
        src.log_normalize(10000.0)
        stall()
        src.simulate_doublets(dst, pa, pb)
        stall()
        src.log_normalize(50.0)
        return {"dst": (dst.dims(), dst.download(0), dst.download(1)), "src": src.download(0)}
    with contexts(sa, 2) as (src, dst):
        want = run(src, dst)
    assert want["dst"][0][:2] == (300, 900)
    spin = the_stall()
    with contexts(sa, 2) as (src, dst), caller_stream(dst) as S:
        got = run(src, dst, lambda: spin(S))
    assert not bits_differ(got, want), "dst on a stalled caller's stream: not the bits of the private-stream run"
    with contexts(sa, 2) as (src, dst), caller_stream(src) as S:
        got = run(src, dst, lambda: spin(S))
    assert not bits_differ(got, want), "src on a stalled caller's stream: not the bits of the private-stream run"
    with contexts(sa, 2) as (src, dst), caller_stream(src) as S1, caller_stream(dst) as S2:
        got = run(src, dst, lambda: (spin(S1), spin(S2)))
    assert not bits_differ(got, want), "both on stalled caller's streams: not the bits of the private-stream run"


# ----------------------------------------------------------------------------------------------------------- the pipe
def planted_dgc(sa):
    fx = planted()
    return sa.dgCMatrix(fx["x"], fx["i"], fx["p"], fx["dense"].shape)


def planted_device(sa, ora, sim_ratio=2.0, **kw):
    return sa.score_doublets(planted_dgc(sa), w=rs.planted_model(ora), sim_ratio=sim_ratio, **kw)


def test_batches_that_cut_the_simulated_cells_unevenly_give_the_same_bits(sa, ora):
    whole = cached("planted2", lambda: planted_device(sa, ora))
    for b in (1000, 2399, 701):
        got = planted_device(sa, ora, sim_batch=b)
        assert not bits_differ({k: got[k] for k in ("scores", "se", "sim_scores", "nd", "sim_nd", "h_sim", "h_obs", "threshold")},
                               {k: whole[k] for k in ("scores", "se", "sim_scores", "nd", "sim_nd", "h_sim", "h_obs", "threshold")}), b


def test_the_pipe_on_the_planted_fixture(sa, ora):
    """S bit for bit; H within 1e-9 relative Frobenius; a cell whose nd differs from the restatement's must sit, in the
    restatement, on a cut of its neighbour list with a relative gap of squared distances below 1e-9, and such cells are at
    most 1 % (what the CPU test established for the fixture); the AUC within 0.01 of the restatement's, the share of true
    doublets found at the automatic threshold within the same 1 %."""
    fx = planted()
    want = rs.planted_pipe(ora, 2.0)
    got = cached("planted2", lambda: planted_device(sa, ora))
    n_obs, n_sim, k_adj = want["n_obs"], want["n_sim"], want["k_adj"]
    assert got["k_adj"] == k_adj and np.array_equal(got["parent_a"], want["parent_a"]) and np.array_equal(got["parent_b"], want["parent_b"])
    with sa.Context(0) as src, sa.Context(0) as dst:
        src.upload(planted_dgc(sa), None)
        src.simulate_doublets(dst, got["parent_a"], got["parent_b"])
        assert_csc_bits(dst.download(0), want["S"], "S of the fixture")
        assert dst.doublets_info()["shared_rows"] == want["shared"]
    for name in ("h_obs", "h_sim"):
        err = np.linalg.norm(got[name] - want[name]) / np.linalg.norm(want[name])
        print("%s: relative Frobenius error %.3g" % (name, err))
        assert err < 1e-9
    nd_got, nd_want = np.concatenate([got["nd"], got["sim_nd"]]), want["nd"]
    differ = np.flatnonzero(nd_got != nd_want)
    d2 = want["dist"] ** 2
    gap = (d2[:, k_adj + 1] - d2[:, k_adj]) / np.maximum(d2[:, k_adj + 1], 1e-300)
    print("cells whose nd differs: %d of %d; their largest gap at the cut %.3g" % (differ.size, nd_want.size, gap[differ].max() if differ.size else 0.0))
    assert np.all(gap[differ] < 1e-9) and differ.size <= 0.01 * nd_want.size
    auc_got, auc_want = rs.auc(got["scores"], fx["is_doublet"]), rs.auc(want["score"][:n_obs], fx["is_doublet"])
    print("AUC: device %.4f, restatement %.4f" % (auc_got, auc_want))
    assert auc_got >= auc_want - 0.01
    thr = rs.threshold(want["score"][n_obs:])
    found_want = float((want["score"][:n_obs] > thr)[fx["is_doublet"]].mean())
    found_got = float(got["predicted"][fx["is_doublet"]].mean())
    print("threshold: device %.4f, restatement %.4f; true doublets found %.3f / %.3f" % (got["threshold"], thr, found_got, found_want))
    assert found_got >= found_want - 0.01
    assert same_bits(got["predicted"], got["scores"] > got["threshold"])


# -------------------------------------------------------------------------------------------------------------- pbmc3k
def _pbmc3k(sa):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)          # row indices are stored as within-column deltas
    for c in range(dim[1]):
        i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
    return sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])))


def test_pbmc3k_runs_twice_to_the_same_bits(sa):
    """The whole call on the counts with the variable features selected on the device and the model fitted at rank 10:
    deterministic across two runs, and the simulated cells score higher on average than the observed ones.  No biological
    claim is tested."""
    A = _pbmc3k(sa)
    kw = dict(rank=10, nfeatures=2000, seed=1, maxit=30, threshold=0.25)
    one, two = sa.score_doublets(A, **kw), sa.score_doublets(A, **kw)
    assert not bits_differ({k: one[k] for k in sorted(one)}, {k: two[k] for k in sorted(two)})
    assert one["scores"].shape == (A.ncol,) and one["sim_scores"].shape == (2 * A.ncol,) and one["w"].shape == (2000, 10)
    assert np.all(np.isfinite(one["scores"])) and one["sim_scores"].mean() > one["scores"].mean()
