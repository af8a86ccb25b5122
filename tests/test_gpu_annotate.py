"""Factor annotation on the device (sgl_group_moments, sgl_gene_group_moments, sgl_annotate and their forms;
kernels_annotate.hip) against the numpy / scipy restatement (annotate_restatement.py).

  moments    group_n, sum and rss equal the restatement bit for bit, on the embedding side (host F, held embedding, resident
             H and one-shot forms alike) and on the gene side (resident and upload_dense image alike); nz and sum of the gene
             side equal op_marker_sums.
  statistics the whole call against the restatement's statistics of the same moments, at the tolerances measured on the
             CPU (tests/test_annotate_restatement.py, STATS_TOL).
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import annotate_restatement as ar
import planted_annotation as pa
from test_annotate_restatement import STATS_OUTPUTS, STATS_TOL, worst_differences
from test_gpu_markers import Genes, same_bits, signed, with_zeros

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6
NS = (1, 255, 256, 257, 1000, 5000)
GS = (1, 2, 5, 200)


# -------------------------------------------------------------------------------------------------------------- inputs --
def labels_for(n, G, seed=0):
    """Labels with the sizes at which the loops turn, as far as n and G leave room: group 0 of exactly 256 cells, group 1 of
    257, group 2 a single cell, group 3 empty; the rest at random, about one cell in ten left out."""
    rng = np.random.default_rng(1000 * G + n + seed)
    l = rng.integers(0, G, size=n).astype(np.int32)
    l[rng.random(n) < 0.1] = -1
    if n == 1:
        l[0] = G - 1
        return l
    order = rng.permutation(n)
    want = [256, 257, 1, 0][:G]
    if sum(want) > n:
        want = [w for w in (n // 2, 1, 0) if w <= n][:G]
    for g in range(len(want)):
        l[l == g] = -1 if G <= len(want) else G - 1
    at = 0
    for g, w in enumerate(want):
        l[order[at:at + w]] = g
        at += w
    return l


def embedding(k, n, seed=0):
    rng = np.random.default_rng(7 * k + n + seed)
    return rng.gamma(2.0, 1.5, size=(k, n)) * (rng.random((k, n)) < 0.8)


def check_moments(got, want):
    group_n, s, rss = got
    assert np.array_equal(group_n, want[0])
    assert same_bits(np.ascontiguousarray(s), np.ascontiguousarray(want[1])), np.abs(s - want[1]).max()
    assert same_bits(np.ascontiguousarray(rss), np.ascontiguousarray(want[2])), np.abs(rss - want[2]).max()


def stats_vectors(out):
    v = dict(out)
    v["scalars"] = [out["df_residual"], out["s2_prior"], out["df_prior"], out["df_total"]]
    return {k: (np.asarray(v[k]).T.reshape(-1) if np.asarray(v[k]).ndim == 2 else np.asarray(v[k])) for k in STATS_OUTPUTS}


def check_stats(out, st):
    for name, d in worst_differences(stats_vectors(out), st).items():
        assert d <= STATS_TOL[name], (name, d)


# --------------------------------------------------------------------------------------------------- embedding moments --
@pytest.mark.parametrize("k", [1, 7, 64, 65, 130])
def test_embedding_moments_equal_the_restatement(sa, ctx, k):
    seen = set()
    for n in NS:
        F = embedding(k, n)
        for G in GS:
            labels = labels_for(n, G)
            want = ar.group_moments(F, labels, G)
            seen.update(want[0].tolist())
            check_moments(ctx.group_moments(labels, G, F), want)
    assert {0, 1, 256, 257} <= seen
    # the one-shot forms (sgl_c_group_moments, and the moments sgl_c_annotate returns) and a second call give the same bits
    for n, G in ((1, 1), (257, 2), (1000, 5), (5000, 200)):
        F, labels = embedding(k, n), labels_for(n, G)
        a = ctx.group_moments(labels, G, F)
        check_moments(sa.c_group_moments(F, labels, G), a)
        check_moments(ctx.group_moments(labels, G, F), a)
    out = sa.c_annotate(F, labels, G)
    check_moments((out["group_n"], out["sum"], out["rss"]), a)


@pytest.mark.parametrize("k", [1, 7, 64, 65, 130])
def test_resident_h_held_embedding_and_host_forms_agree(sa, k):
    n, G = 1000, 5
    F, labels = embedding(k, n, seed=3), labels_for(n, G, seed=3)
    want = ar.group_moments(F, labels, G)
    with sa.Context(0) as c:
        c.synth(300, n, 4)
        c.fit_init(k)
        c.set_factors(h=np.ascontiguousarray(F.T))
        check_moments(c.group_moments(labels, G), want)                     # the H of the fit, read in place
        assert same_bits(c.get_factors()[2], np.ascontiguousarray(F.T))
        check_moments(c.group_moments(labels, G, F), want)
        other = embedding(k, 257, seed=9)
        c.hold_embedding(other)                                             # a held embedding goes before the H of the fit
        l2 = labels_for(257, 2)
        check_moments(c.group_moments(l2, 2), ar.group_moments(other, l2, 2))
        c.hold_embedding(None)
        check_moments(c.group_moments(labels, G), want)
    with sa.Context(0) as c:                                                # no matrix, no fit: only the held embedding
        c.hold_embedding(F)
        check_moments(c.group_moments(labels, G), want)
        check_stats(c.annotate(labels, G), ar.annotate_stats(*want))


def test_all_cells_left_out_and_a_single_group(sa, ctx):
    F = embedding(7, 300)
    none = np.full(300, -1, dtype=np.int32)
    group_n, s, rss = ctx.group_moments(none, 3, F)
    assert group_n.tolist() == [0, 0, 0] and (s == 0).all() and not np.signbit(s).any() and (rss == 0).all()
    out = ctx.annotate(none, 3, F)
    assert all(np.isnan(out[k]).all() for k in ("coefficients", "t", "p_raw", "p_adj", "lods", "sigma", "Amean"))
    one = np.zeros(300, dtype=np.int32)
    check_moments(ctx.group_moments(one, None, F), ar.group_moments(F, one, 1))


# -------------------------------------------------------------------------------------------------------- gene moments --
def nonzero(r, k):
    v = np.round(r.normal(0.5, 1.5, size=k), 2)         # negatives and ties among them, no zero
    v[v == 0] = 0.25
    return v


def zero_tail(r, k, zeros):
    """k values whose last `zeros` are stored zeros of both signs: in the highest cells of the gene, where leaving them out
    (as the dense image does) moves no other entry to another lane, block or segment."""
    v = nonzero(r, k)
    v[k - zeros:] = np.where(np.arange(zeros) % 2 == 0, 0.0, -0.0)
    return v


def gene_matrix():
    """300 genes on 9000 cells: every kind of gene the residual pass can meet.  The stored zeros of THIS matrix end their
    genes, so that the image upload_dense builds (which stores no zero) holds every other entry at the same place and the
    stated order gives the same bits for both; zeros in mid-gene are the matter of mid_zero_matrix below."""
    n = 9000
    rng = np.random.default_rng(41)
    g = Genes(n)
    labels = rng.integers(-1, 5, size=n).astype(np.int32)
    labels[labels == 3] = 2                                                  # an empty group
    labels[[500, 4000]] = [0, 1]                                             # the cells of the two values of the gene of six below
    names = {
        "more than a segment": g.add_random(rng, 8800, lambda r, k: zero_tail(r, k, 30)),
        "exactly a segment": g.add_random(rng, 8192, nonzero),
        "empty": g.add(np.zeros(0), np.zeros(0, dtype=np.int64)),
    }
    out_cells = np.nonzero(labels == -1)[0]
    names["only in excluded cells"] = g.add(rng.random(out_cells.shape[0]) + 1.0, out_cells)
    names["zeros of both signs"] = g.add(np.array([2.5, -1.5, 0.0, -0.0, -0.0, 0.0]), np.array([500, 4000, 4001, 7000, 8000, 8999]))
    names["only zeros"] = g.add(np.array([0.0, -0.0, 0.0]), np.array([1, 2, 8000]))
    for q in range(294):
        length = int(rng.integers(0, 700))
        g.add_random(rng, length, nonzero if q % 2 or length < 8 else (lambda r, k: zero_tail(r, k, 5)))
    assert len(g.x) == 300
    return g, labels, names


def mid_zero_matrix():
    """40 genes on 3000 cells with stored zeros of both signs anywhere in a gene."""
    n = 3000
    rng = np.random.default_rng(43)
    g = Genes(n)
    for q in range(40):
        g.add_random(rng, int(rng.integers(1, 2900)), (signed, with_zeros)[q % 2])
    labels = rng.integers(-1, 4, size=n).astype(np.int32)
    return g, labels


@pytest.fixture(scope="module")
def gene_case():
    g, labels, names = gene_matrix()
    return g, labels, names, ar.gene_moments(*g.csc_t(), labels, 5)


def check_gene_moments(got, want):
    group_n, nz, s, rss = got
    assert np.array_equal(group_n, want[0]) and np.array_equal(nz, want[1])
    assert same_bits(np.ascontiguousarray(s), np.ascontiguousarray(want[2]))
    assert same_bits(np.ascontiguousarray(rss), np.ascontiguousarray(want[3])), np.abs(rss - want[3]).max()


def test_gene_moments_equal_the_restatement_and_the_marker_sums(sa, ctx, gene_case):
    g, labels, names, want = gene_case
    ctx.upload(g.dgc(sa))
    got = ctx.gene_group_moments(labels, 5)
    check_gene_moments(got, want)
    _, nz, s = ctx.op_marker_sums(labels, 5, "identity")
    assert np.array_equal(got[1], nz) and same_bits(np.ascontiguousarray(got[2]), np.ascontiguousarray(s))
    e = names["empty"]
    assert got[3][e] == 0.0 and got[3][names["only in excluded cells"]] == 0.0
    assert (got[1][names["zeros of both signs"]].sum() == 2) and got[3][names["zeros of both signs"]] > 0
    assert (got[1][names["only zeros"]] == 0).all() and got[3][names["only zeros"]] == 0.0
    x, i, p = g.csc_t()
    assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any() and (x < 0).any()
    assert np.diff(p).max() > ar.SEG and (np.diff(p) == ar.SEG).any()
    check_gene_moments(ctx.gene_group_moments(labels, 5), want)             # a second call: the same bits


def _dense_image(g):
    x, i, p = g.csc_t()
    return np.ascontiguousarray(np.asarray(sp.csc_matrix((x, i, p), shape=(g.n, len(g.x))).todense()).T)   # stored zeros become implicit


def test_gene_moments_of_the_upload_dense_image_agree(sa, ctx, gene_case):
    g, labels, names, want = gene_case
    ctx.upload(g.dgc(sa))
    resident = ctx.gene_group_moments(labels, 5)
    with sa.Context(0) as c:
        c.upload_dense(_dense_image(g))
        dense = c.gene_group_moments(labels, 5)
    check_gene_moments(dense, want)
    check_gene_moments(dense, resident)


def test_stored_zeros_in_mid_gene_join_the_implicit_ones(sa, ctx):
    """A stored zero holds a place in the stated order (its lane adds +0.0), so the image without it may sum in another order:
    each image equals the restatement of ITS entries bit for bit, the integers agree, and both stay inside the stated bound."""
    g, labels = mid_zero_matrix()
    x, i, p = g.csc_t()
    assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
    ctx.upload(g.dgc(sa))
    resident = ctx.gene_group_moments(labels, 4)
    check_gene_moments(resident, ar.gene_moments(x, i, p, labels, 4))
    T = sp.csc_matrix(_dense_image(g).T)
    T.sort_indices()
    with sa.Context(0) as c:
        c.upload_dense(_dense_image(g))
        dense = c.gene_group_moments(labels, 4)
    check_gene_moments(dense, ar.gene_moments(T.data, T.indices, T.indptr.astype(np.int64), labels, 4))
    assert np.array_equal(dense[1], resident[1])
    U = 2.0 ** -53
    longest = int(np.diff(p).max())
    assert np.abs(dense[3] - resident[3]).max() <= 2 * (longest + 3) * U * max(resident[3].max(), 1.0)


def test_the_whole_gene_call_equals_the_restated_statistics(sa, ctx, gene_case):
    g, labels, names, want = gene_case
    ctx.upload(g.dgc(sa))
    for tail, center, scale in (("pos", True, False), ("std", True, True), ("neg", False, False)):
        out = ctx.annotate_genes(labels, 5, center=center, scale=scale, tail=tail)
        check_gene_moments((out["group_n"], out["nz"], out["sum"], out["rss"]), want)
        check_stats(out, ar.annotate_stats(want[0], want[2], want[3], center=center, scale=scale, tail=tail))


# ------------------------------------------------------------------------------------------------------ the whole call --
@pytest.mark.parametrize("tail", ["pos", "neg", "std"])
def test_the_whole_call_equals_the_restated_statistics(sa, ctx, tail):
    for k, n, G, scale in ((7, 1000, 5, False), (65, 5000, 200, False), (1, 257, 2, True), (130, 1000, 5, True)):
        F, labels = embedding(k, n, seed=11), labels_for(n, G, seed=11)
        want = ar.group_moments(F, labels, G)
        out = ctx.annotate(labels, G, F, scale=scale, tail=tail)
        check_moments((out["group_n"], out["sum"], out["rss"]), want)
        check_stats(out, ar.annotate_stats(*want, scale=scale, tail=tail))


def test_any_output_pointer_may_be_null(sa, ctx):
    F, labels = embedding(7, 1000), labels_for(1000, 5)
    want = ctx.annotate(labels, 5, F)
    L = sa._lib.load()
    buf = np.ascontiguousarray(F.T)
    lods = np.empty((5, 7))
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = L.sgl_annotate(ctx._h, buf.ctypes.data_as(f64), 7, 1000, labels.ctypes.data_as(i32), 5, 1, 0, 0.01, 0, None, None, None,
                        *((None,) * 10), lods.ctypes.data_as(f64))
    assert rc == 0 and same_bits(np.ascontiguousarray(lods.T), np.ascontiguousarray(want["lods"]))
    assert L.sgl_group_moments(ctx._h, buf.ctypes.data_as(f64), 7, 1000, labels.ctypes.data_as(i32), 5, None, None, None) == 0


def test_planted_pairs_are_exactly_what_survives(sa):
    H, labels, pairs = pa.planted()
    model = {"h": H, "factor_names": ["NMF_%d" % (q + 1) for q in range(pa.K)]}
    meta = {"group": np.where(labels < 0, None, np.array(["g%d" % l for l in labels], dtype=object)), "noise": np.arange(pa.N_CELLS) * 0.5}
    tables = sa.AnnotateNMF(model, meta)
    assert list(tables) == ["group"]
    t = tables["group"]
    strong = {(int(g), int(f)) for g, f, p in zip(t["group"], t["factor"], t["p"]) if p < 1e-6}
    assert strong == set(pairs), (strong, pairs)
    assert (t["fc"] > 0).all() and t["group_names"][0].startswith("g") and t["factor_names"][0].startswith("NMF_")
    # the same through get_model_fit on a model and on a context that holds the embedding
    fit = sa.get_model_fit(labels, pa.G, model)
    with sa.Context(0) as c:
        c.hold_embedding(H)
        fit2 = sa.get_model_fit(labels, pa.G, c)
    for key in ("coefficients", "stdev_unscaled", "sigma", "df_residual", "Amean", "s2_prior", "df_prior", "s2_post", "df_total", "t",
                "p_value", "lods", "var_prior", "centered"):
        assert key in fit
        assert same_bits(np.ascontiguousarray(np.asarray(fit[key], dtype=np.float64)), np.ascontiguousarray(np.asarray(fit2[key], dtype=np.float64))), key
    rows = sa.get_model_results(fit)
    assert {(int(g), int(f)) for g, f, p in zip(rows["group"], rows["factor"], rows["p"]) if p < 1e-6} == set(pairs)
    assert fit["coefficients"].shape == (pa.K, pa.G) and fit["centered"] is True


# ------------------------------------------------------------------------------------------------------ fits, refusals --
def _same(fa, fb, what):
    for x, y in zip(fa, fb):
        assert same_bits(np.ascontiguousarray(x), np.ascontiguousarray(y)), what


def test_a_fit_continued_after_a_call_gives_the_same_bits(sa):
    m, n, k = 120, 6000, 12
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
                out = c.annotate(labels, 6)
                genes = c.annotate_genes(labels, 6)
                _same(c.get_factors(), before, "factors")
                _same(c.download(1), x0, "matrix")
                H = before[2].T
                check_moments((out["group_n"], out["sum"], out["rss"]), ar.group_moments(H, labels, 6))
                assert genes["lods"].shape == (m, 6)
            tols += [c.nmf_iterate(0.01, 0.01, 0.0, 0.0) for _ in range(2)]
            runs[with_call] = (c.get_factors(), tols, c.sweeps_get(reset=True))
    _same(runs[True][0], runs[False][0], "fit")
    assert runs[True][1] == runs[False][1]
    for key in ("h_sweeps", "w_sweeps"):
        assert runs[True][2][key] == runs[False][2][key], key


def test_refusals_return_their_code_and_leave_the_context_usable(sa):
    n, k, G = 600, 7, 4
    F, labels = embedding(k, n), labels_for(n, G)
    want = ar.group_moments(F, labels, G)
    A = sa.dgCMatrix.from_dense(np.round(embedding(30, n, seed=2), 1))

    def refused(c, code, match, fn):
        dims = c.dims()
        with pytest.raises(sa.SingletHipError, match=match) as e:
            fn()
        assert e.value.code == code and c.dims() == dims

    with sa.Context(0) as c:
        refused(c, ESTATE, "no fit is initialised", lambda: c.group_moments(labels[:0], G))
        refused(c, ESTATE, "no fit is initialised", lambda: c.annotate(labels[:0], G))
        refused(c, ESTATE, "no matrix resident", lambda: c.gene_group_moments(labels[:0], G))
        refused(c, ESTATE, "no matrix resident", lambda: c.annotate_genes(labels[:0], G))
        bad = labels.copy()
        bad[77], bad[500] = G, -2
        refused(c, EINVAL, r"sgl_group_moments: labels\[77\] = 4 is outside \[-1, 4\)", lambda: c.group_moments(bad, G, F))
        bad[77] = 0
        refused(c, EINVAL, r"sgl_annotate: labels\[500\] = -2 is outside \[-1, 4\)", lambda: c.annotate(bad, G, F))
        refused(c, EINVAL, r"n_groups = 0 is outside \[1, 1024\]", lambda: c.group_moments(np.zeros(n, dtype=np.int32), 0, F))
        refused(c, EINVAL, r"n_groups = 1025 is outside \[1, 1024\]", lambda: c.annotate(np.zeros(n, dtype=np.int32), 1025, F))
        refused(c, EINVAL, r"k = 1025 is outside \[1, 1024\]", lambda: c.group_moments(np.zeros(3, dtype=np.int32), 1, np.ones((1025, 3))))
        refused(c, EINVAL, r"proportion = 0 is outside \(0, 1\)", lambda: c.annotate(labels, G, F, proportion=0.0))
        L = sa._lib.load()
        f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        buf = np.ascontiguousarray(F.T)
        assert L.sgl_group_moments(c._h, buf.ctypes.data_as(f64), k, n, None, G, None, None, None) == EINVAL
        assert b"sgl_group_moments: NULL labels" in L.sgl_last_error()
        assert L.sgl_group_moments(c._h, buf.ctypes.data_as(f64), 0, n, labels.ctypes.data_as(i32), G, None, None, None) == EINVAL
        assert b"k = 0 is outside [1, 1024]" in L.sgl_last_error()
        assert L.sgl_annotate(c._h, buf.ctypes.data_as(f64), k, n, labels.ctypes.data_as(i32), G, 1, 0, 0.01, 3, *((None,) * 14)) == EINVAL
        assert b"tail = 3" in L.sgl_last_error()
        c.upload(A)
        refused(c, EINVAL, r"sgl_gene_group_moments: labels\[500\] = -2", lambda: c.gene_group_moments(bad, G))
        refused(c, EINVAL, r"sgl_annotate_genes: n_groups = 1025", lambda: c.annotate_genes(labels, 1025))
        c.fit_init(k)
        assert L.sgl_group_moments(c._h, None, k, 10, labels.ctypes.data_as(i32), G, None, None, None) == EINVAL
        assert b"are not the fit's" in L.sgl_last_error()
        c.set_allreduce(lambda dev_ptr, count: None)
        refused(c, ESTATE, "all-reduce hook", lambda: c.group_moments(labels, G, F))
        refused(c, ESTATE, "all-reduce hook", lambda: c.annotate_genes(labels, G))
        c.set_allreduce(None)
        c.upload(A, None, cell_offset=n, ncells_total=3 * n)
        refused(c, ESTATE, "shard", lambda: c.gene_group_moments(labels, G))
        c.fit_init(k)
        refused(c, ESTATE, "shard", lambda: c.group_moments(labels, G))
        # usable afterwards
        c.upload(A)
        check_moments(c.group_moments(labels, G, F), want)
        assert c.gene_group_moments(labels, G)[3].shape == (30,)
    with sa.Multi([0, 0]) as M:
        M.upload(A)
        r0 = M.rank_ctx(0)
        with pytest.raises(sa.SingletHipError, match="team") as e:
            r0.gene_group_moments(labels[:r0.dims()[1]], G)
        assert e.value.code == ESTATE
        with pytest.raises(sa.SingletHipError, match="team") as e:
            r0.group_moments(labels, G, F)
        assert e.value.code == ESTATE
    # the one-shot forms refuse their arguments before a context is made
    L = sa._lib.load()
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert L.sgl_c_group_moments(None, k, n, labels.ctypes.data_as(i32), G, None, None, None) == EINVAL
    assert b"sgl_c_group_moments: F is NULL" in L.sgl_last_error()
    assert L.sgl_c_annotate(None, k, n, labels.ctypes.data_as(i32), G, 1, 0, 0.01, 0, *((None,) * 14)) == EINVAL
    assert b"sgl_c_annotate: F is NULL" in L.sgl_last_error()
    with pytest.raises(sa.SingletHipError, match=r"sgl_c_group_moments: labels\[500\] = -2 is outside \[-1, 4\)") as e:
        sa.c_group_moments(F, bad, G)
    assert e.value.code == EINVAL
    with pytest.raises(sa.SingletHipError, match=r"sgl_c_group_moments: n_groups = 1025") as e:
        sa.c_group_moments(F, labels, 1025)
    assert e.value.code == EINVAL
    check_moments(sa.c_group_moments(F, labels, G), want)
    with pytest.raises(sa.SingletHipError, match=r"sgl_c_annotate: labels\[500\] = -2") as e:
        sa.c_annotate(F, bad, G)
    assert e.value.code == EINVAL
