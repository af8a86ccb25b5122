"""The ligand-receptor test on the device (sgl_ligrec, sgl_op_ligrec_sums, sgl_op_ligrec_tally and their forms; kernels_ligrec.hip)
against the numpy restatement (ligrec_restatement.py), bit for bit in nz, sum, mean, score, n_ge and the null tensor: genes of 0, 1,
63, 64, 65, 8192, 8193 and 16 385 stored entries in a matrix of 16 400 cells, a gene of explicit zeros, a gene with negative
values, an empty class; K = 1, 2, 20, 255, 256 and both sides of every K at which the vectors per wave change; nperm = 1, 63,
64, 65, 130 at batch 0, 64 and 1; both paths and every vectors_per_wave; lig == rec, a repeated pair, a gene in many pairs; the
label vectors of sgl_op_nhood_permute; one-shot against the context call; after a dense upload; beside a running fit; the
caller's-stream contract; every refusal.  References are computed once and shared."""
import numpy as np
import pytest

import ligrec_restatement as lr
from nhood_restatement import permuted
from test_gpu_caller_stream import Stalled, assert_same_bits, caller_stream, contexts

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -6
N_CELLS = 16400
LENGTHS = (0, 1, 63, 64, 65, 8192, 8193, 16385)          # genes 0 .. 7
M = 14                                                    # 8: explicit zeros; 9: negative values; 10 .. 13: sparse
GENES = np.array([7, 0, 1, 2, 3, 4, 5, 6, 8, 9, 12, 10], dtype=np.int32)   # any order; 11 and 13 are not listed
LIG = np.array([0, 5, 5, 6, 6, 9, 10, 0, 8, 3, 6], dtype=np.int32)        # indices into GENES; 6 = gene 5 in many pairs
REC = np.array([6, 6, 5, 7, 7, 6, 11, 0, 6, 4, 1], dtype=np.int32)        # (5, 5) and (0, 0): lig == rec; (6, 7) twice
K_EDGES = (1, 2, 20, 64, 65, 128, 129, 255, 256)
FIELDS = ("group_n", "nz", "sum", "mean", "score", "n_ge")
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def the_matrix(sa):
    """(x, i, p) cell-major with ascending rows, the dgCMatrix, and the gene-side image of the restatement."""
    def make():
        rng = np.random.default_rng(77)
        rows, cols, vals = [], [], []
        for g in range(M):
            ln = LENGTHS[g] if g < 8 else (300 if g == 8 else int(rng.integers(150, 400)))
            cells = np.sort(rng.choice(N_CELLS, ln, replace=False))
            if g == 8:
                x = np.zeros(ln)                                       # stored, all zero
            elif g == 9:
                x = rng.normal(0.0, 1.0, ln)                           # negative values
            else:
                x = np.exp(rng.normal(0.0, 2.0, ln))
                x[::7] = 0.0 if g == 6 else x[::7]                      # explicit zeros inside a long gene
            rows.append(np.full(ln, g))
            cols.append(cells)
            vals.append(x)
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        o = np.lexsort((rows, cols))
        x, i = vals[o], rows[o].astype(np.int32)
        p = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=N_CELLS)))).astype(np.int32)
        gx, gc, gp = lr.gene_major(x, i, p, M)
        assert np.diff(gp)[:8].tolist() == list(LENGTHS)
        return x, i, p, sa.dgCMatrix(x, i, p, (M, N_CELLS)), (gx, gc, gp)
    return cached("matrix", make)


def labels_of(nb, K, seed):
    labs = np.random.default_rng(seed).integers(0, K, (nb, N_CELLS)).astype(np.int32)
    if K > 3:
        labs[labs == 1] = 0                                  # class 1 has no cell
    return labs


def resident(sa):
    c = sa.Context(0)
    c.upload(the_matrix(sa)[3], None)
    return c


def info_fields(info):
    return {q: info[q] for q in ("path", "vectors_per_wave", "waves", "lds_bytes")}


def plan_fields(K, nvec, path=0, vpw=0):
    pl = lr.plan(N_CELLS, K, len(GENES), 0, nvec, path=path, vpw=vpw)
    return {q: pl[q] for q in ("path", "vectors_per_wave", "waves", "lds_bytes")}


# ------------------------------------------------------------------------------------------------------------- the sums
@pytest.mark.parametrize("K", (1, 2, 3))
def test_sums_equal_the_restatement_at_every_length_path_and_vectors_per_wave(sa, K):
    gx, gc, gp = the_matrix(sa)[4]
    labs = labels_of(130, K, 5 + K)
    want = cached(("sums", K), lambda: lr.sums(gx, gc, gp, GENES, labs, K))
    assert want.shape == (130, len(GENES), K)
    with resident(sa) as c:
        for nb in (1, 63, 64, 65, 130):
            for path in (0, 2):
                got = c.op_ligrec_sums(labs[:nb], K, GENES, path=path)
                assert same_bits(got, want[:nb]), (nb, path)
                info = c.ligrec_info()
                assert info_fields(info) == plan_fields(K, nb, path) and info["batches"] == 1 and info["batch"] == nb
                assert (info["lds_genes"], info["global_genes"]) == ((len(GENES), 0) if path == 0 else (0, len(GENES)))
        for path in (1, 2):
            for vpw in (1, 2, 4, 8, 16, 32, 64):
                assert same_bits(c.op_ligrec_sums(labs[:70], K, GENES, path=path, vectors_per_wave=vpw), want[:70]), (path, vpw)
                assert info_fields(c.ligrec_info()) == plan_fields(K, 70, path, vpw)
        # a single gene and its order in the list do not matter: the sums are a function of (gene, label vector) alone
        one = c.op_ligrec_sums(labs[:5], K, GENES[:1])
        assert same_bits(one[:, 0], want[:5, 0])
        rev = c.op_ligrec_sums(labs[:5], K, GENES[::-1].copy())
        assert same_bits(rev[:, ::-1], want[:5])
    assert not want[:, 1].any() and not want[:, 8].any()                      # the gene without entries, the gene of zeros


@pytest.mark.parametrize("K", K_EDGES)
def test_sums_at_both_sides_of_every_step_of_the_plan(sa, K):
    gx, gc, gp = the_matrix(sa)[4]
    nb = 70                                                                  # 2 groups at 64 vectors per wave, 3 at 32, 5 at 16
    labs = labels_of(nb, K, K)
    want = lr.sums(gx, gc, gp, GENES, labs, K)
    cap = lr.vpw_max(K)
    with resident(sa) as c:
        got = c.op_ligrec_sums(labs, K, GENES)
        assert info_fields(c.ligrec_info()) == plan_fields(K, nb) and c.ligrec_info()["vectors_per_wave"] == cap
        assert same_bits(got, want)
        if K > 3:
            assert not got[:, :, 1].any()                                     # the class without cells
        assert same_bits(c.op_ligrec_sums(labs, K, GENES, path=2), want) and c.ligrec_info()["path"] == 2
        for vpw in (1, 16, 32, 64):
            if vpw <= cap and vpw != cap:
                assert same_bits(c.op_ligrec_sums(labs[:33], K, GENES, vectors_per_wave=vpw), want[:33]), vpw
                assert c.ligrec_info()["vectors_per_wave"] == vpw
        if cap < 64:                                                          # one step above what a wave holds at this K
            for path in (1, 2):
                with pytest.raises(sa.SingletHipError, match="vectors_per_wave = %d" % (2 * cap)) as e:
                    c.op_ligrec_sums(labs, K, GENES, path=path, vectors_per_wave=2 * cap)
                assert e.value.code == EINVAL


# ------------------------------------------------------------------------------------------------------- the whole call
def whole(sa):
    def make():
        x, i, p, A, _ = the_matrix(sa)
        K, nperm, seed = 5, 130, 9
        lab = np.random.default_rng(1).integers(0, K, N_CELLS).astype(np.int32)
        lab[lab == 3] = 2                                                     # class 3 empty
        want = lr.ligrec(x, i, p, M, lab, K, GENES, LIG, REC, nperm, seed, threshold=0.002)
        return dict(A=A, K=K, nperm=nperm, seed=seed, lab=lab, want=want)
    return cached("whole", make)


def prefix(want, nperm):
    """The restated result at a smaller nperm: the relabellings are the first nperm of the same sequence."""
    out = dict(want, null=want["null"][:nperm])
    out["n_ge"] = (out["null"] >= want["score"][None]).sum(axis=0).astype(np.int64)
    return out


def test_whole_call_equals_the_restatement_whatever_nperm_and_batch(sa):
    fx = whole(sa)
    want = fx["want"]
    assert np.isnan(want["mean"][:, 3]).all() and not want["score"][:, 3].any() and not want["score"][:, :, 3].any()
    assert (want["nz"][8] == 0).all() and (want["sum"][8] == 0).all() and not want["score"][8].any()      # the gene of explicit zeros
    assert (want["mean"][9, [0, 1, 2, 4]] < 0).any() and (want["score"][5] == 0).any()                     # a negative mean scores +0.0
    assert same_bits(want["score"][3], want["score"][4]) and same_bits(want["n_ge"][3], want["n_ge"][4])   # the repeated pair
    assert want["nz"][7].sum() < 8193 and want["nz"][7].sum() > 6000                                        # explicit zeros are not counted
    with resident(sa) as c:
        for nperm in (1, 63, 64, 65, 130):
            ref = prefix(want, nperm)
            for batch in (0, 64, 1):
                got = c.ligrec(fx["lab"], GENES, LIG, REC, fx["K"], nperm=nperm, seed=fx["seed"], batch=batch, return_null=True)
                for q in FIELDS + ("null",):
                    assert same_bits(got[q], ref[q]) or (q == "mean" and np.array_equal(got[q], ref[q], equal_nan=True)), (nperm, batch, q)
                info = c.ligrec_info()
                b = min(batch or 64 * 999, nperm)
                assert info["path"] == 1 and info["vectors_per_wave"] == 64 and info["batches"] == -(-nperm // b)
        bare = c.ligrec(fx["lab"], GENES, LIG, REC, fx["K"], nperm=65, seed=fx["seed"])
        assert "null" not in bare and same_bits(bare["n_ge"], prefix(want, 65)["n_ge"])
        other = c.ligrec(fx["lab"], GENES, LIG, REC, fx["K"], nperm=65, seed=fx["seed"] + 1)
        assert same_bits(other["score"], want["score"]) and not same_bits(other["n_ge"], bare["n_ge"])


def test_the_label_vectors_are_those_of_the_neighbourhood_test_stage_by_stage(sa):
    fx = whole(sa)
    want, K = fx["want"], fx["K"]
    with resident(sa) as c:
        labs = c.op_nhood_permute(fx["lab"], seed=fx["seed"], r0=0, nb=70)
        assert np.array_equal(labs, permuted(fx["lab"], fx["seed"], 0, 70))
        s = c.op_ligrec_sums(labs, K, GENES)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = s / want["group_n"].astype(np.float64)[None, None, :]
        score, n_ge, null = c.op_ligrec_tally(want["mean"], m, LIG, REC, return_null=True)
        ref = prefix(want, 70)
        assert same_bits(score, ref["score"]) and same_bits(n_ge, ref["n_ge"]) and same_bits(null, ref["null"])
        obs = c.op_ligrec_sums(fx["lab"][None, :], K, GENES)
        assert same_bits(obs[0], want["sum"])


def test_one_shot_equals_the_context_call_and_the_statistics(sa):
    fx = whole(sa)
    want = fx["want"]
    one = sa.c_ligrec(fx["A"], fx["lab"], GENES, LIG, REC, fx["K"], threshold=0.002, nperm=fx["nperm"], seed=fx["seed"], batch=50, return_null=True)
    for q in FIELDS + ("null",):
        assert np.array_equal(one[q], want[q], equal_nan=True), q
    st = sa.ligrec_stats(fx["nperm"], one["group_n"], one["nz"], LIG, REC, one["n_ge"], 0.002)
    for q in ("expressed", "p", "padj"):
        assert np.array_equal(one[q], want[q], equal_nan=True) and np.array_equal(st[q], want[q], equal_nan=True), q
    assert not one["expressed"].all() and one["expressed"].any() and np.isnan(one["p"]).any() and not np.isnan(one["p"]).all()
    assert not one["expressed"][:, 3].any() and not one["expressed"][8].any()
    assert one["info"]["batches"] == 3 and one["info"]["batch"] == 50 and one["stage_ms"].shape == (3,) and (one["stage_ms"] > 0).all()
    per = sa.c_ligrec(fx["A"], fx["lab"], GENES, LIG, REC, fx["K"], threshold=0.002, nperm=64, seed=fx["seed"], per_interaction=True)
    ref = prefix(want, 64)
    assert np.array_equal(per["padj"], lr.stats(64, ref["group_n"], ref["nz"], LIG, REC, ref["n_ge"], 0.002, True)["padj"], equal_nan=True)


def test_after_a_dense_upload(sa):
    rng = np.random.default_rng(4)
    m, n, K = 9, 700, 3
    dense = np.where(rng.random((m, n)) < 0.3, rng.normal(0.5, 1.0, (m, n)), 0.0)
    dense[4] = 0.0
    rows, cols = np.nonzero(dense.T)
    x, i = dense.T[rows, cols], cols.astype(np.int32)
    p = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int32)
    lab = rng.integers(0, K, n).astype(np.int32)
    genes, lig, rec = np.array([8, 4, 0, 2], dtype=np.int32), np.array([0, 1, 2], dtype=np.int32), np.array([3, 0, 2], dtype=np.int32)
    want = lr.ligrec(x, i, p, m, lab, K, genes, lig, rec, 40, 2)
    with sa.Context(0) as c:
        c.upload_dense(dense)
        got = c.ligrec(lab, genes, lig, rec, K, nperm=40, seed=2, return_null=True)
    for q in FIELDS + ("null",):
        assert same_bits(got[q], want[q]), q


def test_a_fit_in_progress_continues_with_its_bits(sa, ora):
    A = ora.synth_csc(120, 400, 10)
    dA = sa.dgCMatrix(A.x, A.i, A.p, (A.nrow, A.ncol))
    lab = (np.arange(400) % 4).astype(np.int32)
    genes, lig, rec = np.arange(0, 120, 7, dtype=np.int32), np.array([0, 3, 5], dtype=np.int32), np.array([1, 3, 16], dtype=np.int32)
    want = lr.ligrec(A.x, A.i, A.p, 120, lab, 4, genes, lig, rec, 20, 5)

    def fit(with_call):
        with sa.Context(0) as c:
            c.upload(dA, None)
            c.fit_init(6, None)
            for _ in range(2):
                c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            out = None
            if with_call:
                out = c.ligrec(lab, genes, lig, rec, 4, nperm=20, seed=5, return_null=True)
                c.op_ligrec_sums(lab[None, :], 4, genes, path=2)
                c.op_ligrec_tally(out["mean"], out["mean"][None], lig, rec)
            for _ in range(2):
                c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            return out, c.get_factors(), c.dims()
    out, after, dims = fit(True)
    _, plain, dims0 = fit(False)
    assert all(same_bits(out[q], want[q]) for q in FIELDS + ("null",)) and dims == dims0
    assert all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(after, plain)), "the fit's iterate changed"


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched_and_the_context_usable(sa):
    from singlet_amd import _lib
    from singlet_amd._lib import f64p, i32p, i64p, ptr
    fx = whole(sa)
    K, lab, want = fx["K"], fx["lab"], fx["want"]
    L = _lib.load()
    G, P = len(GENES), len(LIG)

    def raw(c, lab_=lab, n=N_CELLS, k=K, genes=GENES, g=G, lig=LIG, rec=REC, pp=P, nperm=10, batch=0):
        outs = [np.full(K, -7, dtype=np.int64), np.full((G, K), -7, dtype=np.int64), np.full((G, K), -7.0), np.full((G, K), -7.0),
                np.full((K, K, P), -7.0), np.full((K, K, P), -7, dtype=np.int64), np.full((10, K, K, P), -7.0)]
        rc = L.sgl_ligrec(c._h, ptr(lab_, i32p), n, k, ptr(genes, i32p), g, ptr(lig, i32p), ptr(rec, i32p), pp, nperm, 0, batch, ptr(outs[0], i64p),
                          ptr(outs[1], i64p), ptr(outs[2], f64p), ptr(outs[3], f64p), ptr(outs[4], f64p), ptr(outs[5], i64p), ptr(outs[6], f64p))
        return rc, L.sgl_last_error().decode(), all((o == -7).all() for o in outs)

    def usable(c):
        assert same_bits(c.op_ligrec_sums(lab[None, :], K, GENES)[0], want["sum"])

    def refused(c, match, **kw):
        rc, msg, untouched = raw(c, **kw)
        assert rc == EINVAL and untouched, (kw.keys(), rc, msg)
        import re
        assert re.search(match, msg), (match, msg)
        usable(c)

    def at(a, pos, v):
        b = a.copy()
        b[pos] = v
        return b

    with resident(sa) as c:
        for name in ("lab_", "genes", "lig", "rec"):
            refused(c, "NULL", **{name: None})
        refused(c, r"K = 0 is outside \[1, 256\]", k=0)
        refused(c, r"K = 257", k=257)
        refused(c, r"G = 0 is outside \[1, 14\]", g=0)
        refused(c, r"G = 15", g=15)
        refused(c, r"P = 0", pp=0)
        refused(c, r"nperm = 0 is outside", nperm=0)
        refused(c, r"nperm = 1048577", nperm=(1 << 20) + 1)
        refused(c, r"lab\[123\] = 5 is outside \[0, 5\)", lab_=at(lab, 123, 5))
        refused(c, r"lab\[16399\] = -2", lab_=at(lab, N_CELLS - 1, -2))
        refused(c, r"genes\[2\] = 14 is outside \[0, 14\)", genes=at(GENES, 2, 14))
        refused(c, r"genes\[0\] = -1", genes=at(GENES, 0, -1))
        refused(c, r"genes\[4\] = 7 is listed twice", genes=at(GENES, 4, 7))
        refused(c, r"lig\[3\] = 12 is outside \[0, 12\)", lig=at(LIG, 3, 12))
        refused(c, r"rec\[10\] = -1", rec=at(REC, 10, -1))
        refused(c, r"batch = -1 is negative", batch=-1)
        refused(c, r"n = 16399 labels, the matrix has 16400 cells", n=N_CELLS - 1)
        # the stated order: the earlier defect is the one named
        refused(c, r"K = 0", k=0, g=0, nperm=0, batch=-1)
        refused(c, r"G = 0", g=0, pp=0, nperm=0)
        refused(c, r"nperm = 0", nperm=0, lab_=at(lab, 0, 9), batch=-1)
        refused(c, r"lab\[0\] = 9", lab_=at(lab, 0, 9), genes=at(GENES, 0, -1), n=N_CELLS - 1)
        refused(c, r"genes\[0\] = -1", genes=at(GENES, 0, -1), lig=at(LIG, 0, 99), batch=-1)
        refused(c, r"lig\[0\] = 99", lig=at(LIG, 0, 99), batch=-1, n=N_CELLS - 1)
        refused(c, r"batch = -1", batch=-1, n=N_CELLS - 1)
        # the threshold belongs to the one-shot call and to the statistics
        for thr in (-0.1, 1.5, float("nan")):
            with pytest.raises(sa.SingletHipError, match="threshold is outside") as e:
                sa.c_ligrec(fx["A"], lab, GENES, LIG, REC, K, threshold=thr, nperm=3)
            assert e.value.code == EINVAL
        with pytest.raises(sa.SingletHipError, match=r"lab\[123\] = -2") as e:
            sa.c_ligrec(fx["A"], at(lab, 123, -2), GENES, LIG, REC, K, nperm=3)       # before a context is made
        assert e.value.code == EINVAL
        # the stage operators
        for match, call in ((r"path = 3", lambda: c.op_ligrec_sums(lab[None, :], K, GENES, path=3)),
                            (r"vectors_per_wave = 3 ", lambda: c.op_ligrec_sums(lab[None, :], K, GENES, vectors_per_wave=3)),
                            (r"vectors_per_wave = 128", lambda: c.op_ligrec_sums(lab[None, :], K, GENES, path=2, vectors_per_wave=128)),
                            (r"vectors_per_wave = -1", lambda: c.op_ligrec_sums(lab[None, :], K, GENES, vectors_per_wave=-1)),
                            (r"nb = 0", lambda: c.op_ligrec_sums(lab[:0].reshape(0, N_CELLS), K, GENES)),
                            (r"lab\[%d\] = -2" % (N_CELLS + 5), lambda: c.op_ligrec_sums(np.stack([lab, at(lab, 5, -2)]), K, GENES)),
                            (r"genes\[1\] = 7 is listed twice", lambda: c.op_ligrec_sums(lab[None, :], K, np.array([7, 7], dtype=np.int32))),
                            (r"n = 100 labels", lambda: c.op_ligrec_sums(lab[None, :100], K, GENES)),
                            (r"rec\[0\] = 12", lambda: c.op_ligrec_tally(want["mean"], want["mean"][None], LIG[:1], np.array([12], dtype=np.int32)))):
            with pytest.raises(sa.SingletHipError, match=match) as e:
                call()
            assert e.value.code == EINVAL
            usable(c)
        with pytest.raises(ValueError, match="nb x n"):
            c.op_ligrec_sums(lab, K, GENES)
        with pytest.raises(ValueError, match="one index each per pair"):
            c.ligrec(lab, GENES, LIG, REC[:-1], K)
        # the states of sgl_markers
        c.set_allreduce(lambda dev_ptr, count: None)
        for call in (lambda: c.ligrec(lab, GENES, LIG, REC, K, nperm=3), lambda: c.op_ligrec_sums(lab[None, :], K, GENES)):
            with pytest.raises(sa.SingletHipError, match="all-reduce hook") as e:
                call()
            assert e.value.code == ESTATE
        c.set_allreduce(None)
        usable(c)
        small = sa.dgCMatrix(np.ones(3), np.array([0, 1, 2], dtype=np.int32), np.array([0, 1, 2, 3], dtype=np.int32), (5, 3))
        c.upload(small, None, cell_offset=3, ncells_total=9)
        with pytest.raises(sa.SingletHipError, match="shard") as e:
            c.ligrec(np.zeros(3, dtype=np.int32), [0], [0], [0], 1, nperm=3)
        assert e.value.code == ESTATE
        c.upload(small, None)
        got = c.ligrec(np.array([0, 1, 0], dtype=np.int32), [0, 2], [0], [1], 2, nperm=3)
        assert got["sum"].tolist() == [[1.0, 0.0], [1.0, 0.0]] and got["nz"].tolist() == [[1, 0], [1, 0]] and got["score"][0, 0, 0] == 0.5
    with sa.Context(0) as c:
        rc, msg, untouched = raw(c)
        assert rc == ESTATE and untouched and "no matrix resident" in msg


def test_a_team_member_is_refused(sa):
    A = sa.dgCMatrix.from_dense(np.random.default_rng(0).poisson(0.5, (30, 200)).astype(np.float64))
    lab = np.zeros(200, dtype=np.int32)
    with sa.Multi([0, 0]) as team:
        team.upload(A)
        rank = team.rank_ctx(0)
        for call in (lambda: rank.ligrec(lab, [0, 1], [0], [1], 1, nperm=3), lambda: rank.op_ligrec_sums(lab[None, :], 1, [0])):
            with pytest.raises(sa.SingletHipError, match="team") as e:
                call()
            assert e.value.code == ESTATE


# ------------------------------------------------------------------------------------------------- the caller's stream
def test_ligrec_on_a_stalled_caller_stream(sa):
    """sgl_set_stream's contract for sgl_ligrec, sgl_op_ligrec_sums (both paths) and sgl_op_ligrec_tally: all work goes to the
    caller's stream and the host reads wait for it, so a stall at the head of that stream changes no value."""
    fx = whole(sa)
    K, lab, want = fx["K"], fx["lab"], fx["want"]
    labs = labels_of(17, K, 4)
    calls = [("whole", lambda c: c.ligrec(lab, GENES, LIG, REC, K, nperm=65, seed=fx["seed"], batch=20, return_null=True)),
             ("sums, LDS", lambda c: c.op_ligrec_sums(labs, K, GENES, path=1)),
             ("sums, global", lambda c: c.op_ligrec_sums(labs, K, GENES, path=2)),
             ("tally", lambda c: c.op_ligrec_tally(want["mean"], np.stack([want["mean"]] * 3), LIG, REC, return_null=True))]
    A = fx["A"]
    with contexts(sa) as c:
        c.upload(A, None)
        ref = {name: call(c) for name, call in calls}
    assert all(same_bits(ref["whole"][q], prefix(want, 65)[q]) for q in FIELDS + ("null",))
    with contexts(sa) as c, caller_stream(c) as S:
        c.upload(A, None)
        sc = Stalled(c, S)
        got = {name: call(sc) for name, call in calls}
    for name, _ in calls:
        assert_same_bits(got[name], ref[name], name)
