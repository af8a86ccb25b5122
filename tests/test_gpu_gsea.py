"""Gene set enrichment on the device (sgl_c_gsea, its two stage operators and the Python layer above them; kernels_gsea.hip)
against the numpy restatement (gsea_restatement.py), BIT FOR BIT: every score, every null score, every p, NES and padj is
compared through its 64-bit image, every tally as an integer.  The restatement itself is held to independent yardsticks in
test_gsea_restatement.py; here only the end-to-end test adds a statistical check (planted sets at the floor of p, random sets
inside the calibration band 0.05 +- 0.045 derived there)."""
import os

import numpy as np
import pytest

import gsea_restatement as gr

pytestmark = pytest.mark.gpu

EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def make_sets(rng, m, sizes):
    sets = [np.sort(rng.choice(m, size=s, replace=False))[rng.permutation(s)] for s in sizes]
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return ptr, np.concatenate(sets).astype(np.int32)


def factors(rng, m):
    """Four factors: an L1-like one (65 % zeros), an all-zero one (NR == 0 everywhere), a constant one (one tie run), and a
    signed one with a few zeros of either sign."""
    w = np.zeros((m, 4))
    w[:, 0] = rng.random(m) * (rng.random(m) >= 0.65)
    w[:, 2] = 1.5
    w[:, 3] = np.round(rng.normal(size=m), 2)
    w[rng.random(m) < 0.05, 3] = -0.0
    return w


# --------------------------------------------------------------------------------------------------------- observed scores --
@pytest.mark.parametrize("m, sizes", [(4200, (1, 2, 63, 64, 65, 128, 129, 4096, 11, 37, 500)), (66, (1, 2, 63, 64, 65, 11))],
                         ids=["m=4200", "m=66"])
def test_observed_scores_at_the_loop_edges(ctx, m, sizes):
    """Set sizes at every edge of the block loop and of the LDS sort, the cap itself, s = m - 1 (at m = 66); all three score
    types on all four kinds of factor."""
    rng = np.random.default_rng(m)
    w = factors(rng, m)
    ptr, genes = make_sets(rng, m, sizes)
    got = ctx.op_gsea_es(w, ptr, genes)
    ref = gr.observed(w, ptr, genes)
    for name, g, r in zip(("pos", "neg", "std"), got, ref):
        assert same_bits(g, r), (name, np.argwhere(g != r)[:5])
    assert (got[0] >= 0).all() and (got[1] <= 0).all()
    info = ctx.gsea_info()
    assert info["sets"] == len(sizes) and info["s_max"] == max(sizes)


def test_a_set_above_the_cap_is_refused_and_the_context_stays_usable(sa, ctx):
    rng = np.random.default_rng(5)
    m = 4500
    w = factors(rng, m)[:, :1]
    ptr, genes = make_sets(rng, m, (12, gr.LDS_CAP + 1))
    with pytest.raises(sa.SingletHipError, match=r"set 1 holds 4097 genes, above the cap of 4096") as e:
        ctx.op_gsea_es(w, ptr, genes)
    assert e.value.code == EINVAL
    ptr, genes = make_sets(rng, m, (12, gr.LDS_CAP))
    assert same_bits(ctx.op_gsea_es(w, ptr, genes)[0], gr.observed(w, ptr, genes)[0])


# ------------------------------------------------------------------------------------------------- null scores and sample --
NULL_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200)


@pytest.fixture(scope="module")
def null_case():
    rng = np.random.default_rng(77)
    m = 700
    w = factors(rng, m)[:, [0, 3, 1]]
    ref = {}
    sample = gr.null_sample(9, 0, 130, m, NULL_SIZES[-1])
    for st in (0, 1, 2):
        ref[st] = gr.null_scores(w, NULL_SIZES, st, 9, 0, 130, sample=sample)
    return w, sample, ref


@pytest.mark.parametrize("nperm", [1, 7, 130])
def test_null_scores_do_not_depend_on_the_batch(ctx, null_case, nperm):
    """Distinct sizes straddling 64 and 128; forced batch sizes 1, 7 and nperm give the restatement's bits, and the sample is
    the prefix of the full sort by (key, gene)."""
    w, sample, ref = null_case
    for batch in sorted({1, 7, nperm, 0}):
        for st in ((0, 1, 2) if batch in (0, 7) else (0,)):
            null, got_sample = ctx.op_gsea_null(w, NULL_SIZES, st, seed=9, r0=0, r1=nperm, batch=batch, return_sample=True)
            assert np.array_equal(got_sample, sample[:nperm]), (nperm, batch)
            assert same_bits(null, ref[st][:, :, :nperm]), (nperm, batch, st)
            info = ctx.gsea_info()
            b = min(batch, nperm) if batch else nperm
            assert info["batch"] == b and info["batches"] == -(-nperm // b) and info["sizes"] == len(NULL_SIZES)


def test_null_scores_at_the_cap(ctx):
    """s_max = 4096: the sampled positions, the prefix sums and the compacted hits fill 80 KiB of LDS."""
    rng = np.random.default_rng(41)
    m = 4200
    w = factors(rng, m)[:, [0, 3]]
    sizes = (1, 4095, gr.LDS_CAP)
    null, sample = ctx.op_gsea_null(w, sizes, "std", seed=3, r0=0, r1=3, batch=2, return_sample=True)
    ref_sample = gr.null_sample(3, 0, 3, m, gr.LDS_CAP)
    assert np.array_equal(sample, ref_sample)
    assert same_bits(null, gr.null_scores(w, sizes, 2, 3, 0, 3, sample=ref_sample))


def test_null_scores_of_a_later_range_of_permutations(ctx, null_case):
    w, sample, ref = null_case
    null, got_sample = ctx.op_gsea_null(w, NULL_SIZES, "std", seed=9, r0=100, r1=130, batch=7, return_sample=True)
    assert np.array_equal(got_sample, sample[100:130]) and same_bits(null, ref[2][:, :, 100:130])


# --------------------------------------------------------------------------------------------------------------- the whole --
@pytest.fixture(scope="module")
def whole_case():
    rng = np.random.default_rng(31)
    m = 700
    w = factors(rng, m)[:, [0, 3, 1]]
    ptr, genes = make_sets(rng, m, [1, 2, 63, 64, 65, 128, 129] + rng.integers(11, 61, size=33).tolist())
    return w, ptr, genes


@pytest.mark.parametrize("score_type", ["pos", "neg", "std"])
def test_tallies_and_statistics_equal_the_restatement_whatever_the_batch(sa, whole_case, score_type):
    w, ptr, genes = whole_case
    nperm = 130
    ref = gr.gsea(w, ptr, genes, gr.SCORE_TYPES[score_type], nperm, seed=4)
    for batch in (1, 7, nperm, 0):
        got = sa.c_gsea(w, ptr, genes, score_type, nperm, seed=4, batch=batch)
        for name in ("n_ge", "n_le", "n_side"):
            assert np.array_equal(got[name], ref[name]), (name, batch)
        for name in ("es", "pval", "nes", "padj"):
            assert same_bits(got[name], ref[name]), (name, batch)
        assert np.array_equal(got["set_size"], ref["set_size"])
        b = batch or nperm
        assert got["info"] == {"sets": ptr.size - 1, "sizes": ref["sizes"].size, "s_max": int(ref["sizes"][-1]), "batches": -(-nperm // b), "batch": b}


# --------------------------------------------------------------------------------------------------------------- refusals --
def test_every_refusal_names_the_offender_and_leaves_the_device_usable(sa, ctx, whole_case):
    w, ptr, genes = whole_case
    m = w.shape[0]

    def refused(match, fn):
        with pytest.raises(sa.SingletHipError, match=match) as e:
            fn()
        assert e.value.code == EINVAL

    bad = w.copy()
    bad[17, 1] = np.inf
    refused(r"w\[17, 1\] is not finite", lambda: sa.c_gsea(bad, ptr, genes))
    bad[17, 1] = np.nan
    refused(r"w\[17, 1\] is not finite", lambda: ctx.op_gsea_es(bad, ptr, genes))
    refused(r"w\[17, 1\] is not finite", lambda: ctx.op_gsea_null(bad, [3], r1=2))
    p2 = ptr.copy()
    p2[3] = p2[2] - 1
    refused(r"set_ptr\[3\] = %d" % p2[3], lambda: sa.c_gsea(w, p2, genes))
    p2 = ptr.copy()
    p2[0] = 1
    refused(r"set_ptr\[0\] = 1", lambda: sa.c_gsea(w, p2, genes))
    p2 = ptr.copy()
    p2[5] = p2[4]
    refused(r"set 4 is empty", lambda: sa.c_gsea(w, p2, genes))
    g2 = genes.copy()
    g2[9] = m
    refused(r"set_genes\[9\] = %d is outside \[0, %d\)" % (m, m), lambda: sa.c_gsea(w, ptr, g2))
    g2[9] = -1
    refused(r"set_genes\[9\] = -1 is outside", lambda: ctx.op_gsea_es(w, ptr, g2))
    g2 = genes.copy()
    g2[ptr[4] + 1] = g2[ptr[4]]
    refused(r"set_genes\[%d\] = %d occurs twice" % (ptr[4] + 1, g2[ptr[4]]), lambda: sa.c_gsea(w, ptr, g2))
    small = w[:129]
    refused(r"set 0 holds 129 genes of 129", lambda: sa.c_gsea(small, [0, 129], np.arange(129)))
    refused(r"above the cap of 4096", lambda: sa.c_gsea(np.ones((5000, 1)), [0, 4097], np.arange(4097)))
    refused(r"nperm = 0 is outside", lambda: sa.c_gsea(w, ptr, genes, nperm=0))
    refused(r"nperm = %d is outside" % ((1 << 20) + 1), lambda: sa.c_gsea(w, ptr, genes, nperm=(1 << 20) + 1))
    refused(r"k = 1025 is outside \[1, 1024\]", lambda: sa.c_gsea(np.ones((40, 1025)), [0, 3], [0, 1, 2]))
    refused(r"batch = -1 is negative", lambda: sa.c_gsea(w, ptr, genes, batch=-1))
    refused(r"sizes\[1\] = 5", lambda: ctx.op_gsea_null(w, [5, 5], r1=2))
    refused(r"sizes\[0\] = %d" % m, lambda: ctx.op_gsea_null(w, [m], r1=2))
    refused(r"not 0 <= r0 < r1", lambda: ctx.op_gsea_null(w, [5], r0=3, r1=3))
    L = sa._lib.load()
    f64p, i64p, i32p = sa._lib.f64p, sa._lib.i64p, sa._lib.i32p
    wt = np.ascontiguousarray(w.T)
    args = (wt.ctypes.data_as(f64p), m, w.shape[1], ptr.ctypes.data_as(i64p), genes.ctypes.data_as(i32p), ptr.size - 1)
    none = (None,) * 10
    assert L.sgl_c_gsea(*args, 3, 10, 0, 0, *none) == EINVAL and b"score_type = 3" in L.sgl_last_error()
    assert L.sgl_c_gsea(*args, -1, 10, 0, 0, *none) == EINVAL
    assert L.sgl_c_gsea(None, *args[1:], 0, 10, 0, 0, *none) == EINVAL and b"NULL" in L.sgl_last_error()
    assert L.sgl_gsea_info(ctx._h, None) == EINVAL
    with pytest.raises(ValueError, match="score_type"):
        sa.c_gsea(w, ptr, genes, "both")
    # the device and the context work as before
    ref = gr.gsea(w, ptr, genes, 0, 5, seed=1)
    got = sa.c_gsea(w, ptr, genes, "pos", 5, seed=1)
    assert same_bits(got["pval"], ref["pval"]) and same_bits(ctx.op_gsea_es(w, ptr, genes)[0], ref["es"])
    assert L.sgl_c_gsea(*args, 0, 3, 0, 0, *none) == 0    # every output NULL


# ----------------------------------------------------------------------------------------------------------------- pbmc3k --
def _pbmc3k(sa):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pbmc3k_counts.npz"))
    p, dim = g["p"], g["dim"]
    i = g["di"].astype(np.int64)          # row indices are stored as within-column deltas
    for c in range(dim[1]):
        i[p[c]:p[c + 1]] = np.cumsum(i[p[c]:p[c + 1]])
    return sa.dgCMatrix(g["x"].astype(np.float64), i.astype(np.int32), p, (int(dim[0]), int(dim[1])))


def test_pbmc3k_end_to_end(sa):
    """Rank 10 on the fixture; a set planted from the top 40 genes of each factor reaches the floor of p in its own factor, 200
    random sets stay inside the calibration band in every factor (their shares of p <= 0.05 came out at 0.010 to 0.030 on an
    MI355X: the ten factors share their heavy genes, so they are far from ten independent draws), and run_gsea equals the
    restatement on the same input."""
    A = sa.PreprocessData(_pbmc3k(sa))
    fit = sa.run_nmf(A, rank=10, tol=1e-4, maxit=100, verbose=False, L1=0.01, seed=123)
    w = np.ascontiguousarray(fit["w"])
    m, k = w.shape
    assert k == 10
    names = ["g%d" % g for g in range(m)]
    rng = np.random.default_rng(2024)
    expressed = np.nonzero(w.sum(axis=1) != 0)[0]
    pathways = {}
    for f in range(k):
        pathways["planted%d" % f] = [names[g] for g in np.argsort(-w[:, f], kind="stable")[:40]]
    for q in range(200):
        pathways["random%d" % q] = [names[g] for g in rng.choice(expressed, size=int(rng.integers(11, 61)), replace=False)]
    nperm = 999
    out = sa.run_gsea(w, pathways, names, nperm=nperm, seed=7)
    assert out["pathways"] == list(pathways) and out["pval"].shape == (210, k)
    floor = -np.log10(1.0 / (nperm + 1))
    for f in range(k):
        assert out["pval"][f, f] == floor and abs(out["es"][f, f] - 1.0) <= 2 * 2.0**-52, (f, out["pval"][f, f], out["es"][f, f])
    share = (out["pval"][k:] >= -np.log10(0.05)).mean(axis=0)
    print("share of p <= 0.05 among the random sets, per factor:", share)
    assert (np.abs(share - 0.05) <= 0.045).all(), share
    # the same filtered input through the restatement
    pnames, rows, sets, tested = sa.api.gsea_filter(pathways, names, w)
    assert tested.all() and pnames == list(pathways)
    ptr = np.concatenate([[0], np.cumsum([s.size for s in sets])]).astype(np.int64)
    ref = gr.gsea(w[rows], ptr, np.concatenate(sets), 0, nperm, seed=7)
    assert same_bits(out["es"], ref["es"]) and same_bits(out["nes"], ref["nes"])
    with np.errstate(divide="ignore"):
        assert same_bits(out["pval"], -np.log10(ref["pval"])) and same_bits(out["padj"], -np.log10(ref["padj"]))
