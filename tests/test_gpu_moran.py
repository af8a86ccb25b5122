"""Spatial autocorrelation on the device (sgl_moran, sgl_op_moran_cross, sgl_moran_embedding and their forms;
kernels_moran.hip) against the numpy restatement (moran_restatement.py), bit for bit: the per-gene moments and the cross term
on genes of every stored-entry count at which a loop changes (0, 1, 63, 64, 65, 8191, 8192, 8193, every cell), the graph's
edge cases (empty columns, degree 1, hubs of 65 and 300, self-loops, asymmetric pairs, n no multiple of 64), the two paths of
the cross term against each other, the table's hygiene across batches, subsets and the one-shot form, the embedding form, the
refusals, the planted tissue end to end and the caller's-stream contract.  References are computed once and shared."""
import numpy as np
import pytest

import moran_restatement as mo
import variable_features_restatement as vf
from test_gpu_caller_stream import Stalled, assert_same_bits, caller_stream, contexts
from test_moran_restatement import planted_claims, planted_tables

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -6
N_BIG = 9000
COUNTS = (0, 1, 63, 64, 65, 8191, 8192, 8193, N_BIG)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def edge_graph(n, seed):
    """An asymmetric graph of mean degree about 8 with negative weights and: columns 0 and n - 1 empty, column 1 of degree 1,
    hubs of degree 65 (column 2) and 300 (column 3), self-loops on every 7th column."""
    rng = np.random.default_rng(seed)
    Gi, Gx, Gp = [], [], [0]
    for j in range(n):
        if j in (0, n - 1):
            rows = np.zeros(0, dtype=np.int64)
        else:
            deg = {1: 1, 2: min(65, n), 3: min(300, n)}.get(j, int(rng.integers(2, 15)))
            rows = np.sort(rng.choice(n, size=min(deg, n), replace=False))
            if j % 7 == 0 and j not in rows:
                rows = np.sort(np.append(rows[:-1], j))
        Gi.extend(rows.tolist())
        Gx.extend((rng.random(rows.shape[0]) * np.where(rng.random(rows.shape[0]) < 0.2, -1.0, 1.0)).tolist())
        Gp.append(len(Gi))
    return np.array(Gx), np.array(Gi, dtype=np.int32), np.array(Gp, dtype=np.int32)


def gene_matrix(n, counts, seed, extra=True):
    """Genes with the given stored-entry counts over n cells (Poisson counts >= 1 at random cells), then, with `extra`, a gene
    with explicit stored zeros, one with negative values and one disjoint from the first long gene.  Returns the per-gene
    (cells, values) lists."""
    rng = np.random.default_rng(seed)
    genes = []
    for c in counts:
        cells = np.sort(rng.choice(n, size=c, replace=False))
        genes.append((cells, 1.0 + rng.poisson(1.5, c)))
    if extra:
        cells = np.sort(rng.choice(n, size=min(500, n), replace=False))
        v = 1.0 + rng.poisson(1.0, cells.shape[0])
        v[::3] = 0.0                                                     # explicit zeros: stored entries
        genes.append((cells, v))
        cells = np.sort(rng.choice(n, size=min(700, n), replace=False))
        genes.append((cells, rng.normal(size=cells.shape[0])))           # negative values
        long_cells = max(genes, key=lambda g: g[0].shape[0] if g[0].shape[0] < n else -1)[0]
        free = np.setdiff1d(np.arange(n), long_cells)
        genes.append((free[:min(40, free.shape[0])], 2.0 + np.arange(min(40, free.shape[0]), dtype=np.float64)))
    return genes


def as_matrix(sa, genes, n):
    """(dgCMatrix genes x cells, (Tx, Ti, Tp) of its transpose)"""
    gi = np.concatenate([np.full(c.shape[0], q) for q, (c, _) in enumerate(genes)]).astype(np.int64)
    ci = np.concatenate([c for c, _ in genes]).astype(np.int64)
    v = np.concatenate([x for _, x in genes]).astype(np.float64)
    x, i, p = vf.csc_of_triplets(gi, ci, v, len(genes), n)
    Tp = np.concatenate(([0], np.cumsum([c.shape[0] for c, _ in genes]))).astype(np.int64)
    return sa.dgCMatrix(x, i, p, (len(genes), n)), (v, ci.astype(np.int32), Tp)


def big(sa):
    def make():
        genes = gene_matrix(N_BIG, COUNTS, 11)
        A, T = as_matrix(sa, genes, N_BIG)
        Gx, Gi, Gp = edge_graph(N_BIG, 12)
        S0, S1, S2, t = mo.graph_moments(Gx, Gi, Gp, N_BIG)
        want = mo.moran_moments(*T, N_BIG, Gx, Gi, Gp, t=t)
        return dict(A=A, T=T, G=sa.dgCMatrix(Gx, Gi, Gp, (N_BIG, N_BIG)), graph=(Gx, Gi, Gp), want=want, counts=np.diff(T[2]))
    return cached("big", make)


def small(sa, n=1000, seed=21):
    def make():
        genes = gene_matrix(n, (0, 1, 63, 64, 65, 200, n), seed)
        A, T = as_matrix(sa, genes, n)
        Gx, Gi, Gp = edge_graph(n, seed + 1)
        want = mo.moran_moments(*T, n, Gx, Gi, Gp)
        return dict(A=A, T=T, G=sa.dgCMatrix(Gx, Gi, Gp, (n, n)), graph=(Gx, Gi, Gp), want=want, counts=np.diff(T[2]), n=n)
    return cached(("small", n, seed), make)


# ------------------------------------------------------------------------------------------------ moments and cross term
def test_moments_and_cross_term_equal_the_restatement_bit_for_bit(sa):
    fx = big(sa)
    with sa.Context(0) as c:
        c.upload(fx["A"], None)
        got = c.moran(fx["G"])
        info = c.moran_info()
        again = c.moran(fx["G"])
    names = ("mean", "M2", "M4", "T", "P", "c")
    wrong = [(names[r], int(fx["counts"][g])) for r in range(6) for g in range(got.shape[1]) if not same_bits(got[r, g], fx["want"][r, g])]
    assert not wrong, "not the restatement's bits (row, stored entries of the gene): %r" % wrong
    assert same_bits(got, again)
    assert got[5].tolist() == fx["counts"].tolist()
    n_search = int((fx["counts"] <= mo.LDS_CAP).sum())
    assert (info["search_genes"], info["table_genes"], info["lds_cap"]) == (n_search, len(fx["counts"]) - n_search, mo.LDS_CAP)
    assert info["table_genes"] == 4 and info["batches"] == 1 and info["table_bytes"] == info["table_batch"] * N_BIG * 8


def test_paths_agree_and_the_split_follows_lds_cap(sa):
    fx = big(sa)
    P = fx["want"][4]
    with sa.Context(0) as c:
        c.upload(fx["A"], None)
        search = c.op_moran_cross(fx["G"], path=1)
        i1 = c.moran_info()
        table = c.op_moran_cross(fx["G"], path=2)
        i2 = c.moran_info()
        auto64 = c.op_moran_cross(fx["G"], lds_cap=64)
        i3 = c.moran_info()
    assert same_bits(search, P) and same_bits(table, P) and same_bits(auto64, P)
    n_fit = int((fx["counts"] <= mo.LDS_CAP).sum())
    assert i1["search_genes"] == n_fit and i1["table_genes"] == len(P) - n_fit           # a gene LDS cannot hold takes the table
    assert i2["search_genes"] == 0 and i2["table_genes"] == len(P)
    assert i3["lds_cap"] == 64 and i3["search_genes"] == int((fx["counts"] <= 64).sum())  # 64 on one side, 65 on the other
    assert [mo.gene_path(cn, 0, 64) for cn in (64, 65)] == [1, 2]


def test_table_hygiene_across_batches_and_gene_orders(sa):
    """The table path with a batch of 1 (every gene reuses slot 0 right after the gene before it) and with the largest batch;
    a long gene precedes a short one that shares no cell with it: a stale table entry would change P."""
    fx = big(sa)
    P = fx["want"][4]
    m = len(P)
    long_g = int(np.argmax(np.where(fx["counts"] < N_BIG, fx["counts"], -1)))
    order = np.array([N_BIG_GENE(fx), long_g, m - 1] + [g for g in range(m) if g not in (N_BIG_GENE(fx), long_g, m - 1)], dtype=np.int32)
    with sa.Context(0) as c:
        c.upload(fx["A"], None)
        for batch in (1, 2, m):
            got = c.op_moran_cross(fx["G"], genes=order, path=2, table_batch=batch)
            info = c.moran_info()
            assert same_bits(got, P[order]), batch
            assert info["table_batch"] == batch and info["batches"] == -(-m // batch)
            assert same_bits(c.op_moran_cross(fx["G"], genes=order, path=2, table_batch=batch), got)


def N_BIG_GENE(fx):
    return int(np.argmax(fx["counts"] == N_BIG))


def test_subsets_one_shot_dense_upload_and_log_normalised_values(sa):
    fx = small(sa)
    n, m = fx["n"], fx["want"].shape[1]
    sub = np.random.default_rng(5).permutation(m)[:6].astype(np.int32)
    with sa.Context(0) as c:
        c.upload(fx["A"], None)
        full = c.moran(fx["G"])
        assert same_bits(full, fx["want"])
        assert same_bits(c.moran(fx["G"], genes=sub), full[:, sub])
        assert c.moran(fx["G"], genes=np.zeros(0, dtype=np.int32)).shape == (6, 0)
        assert same_bits(sa.c_moran(fx["A"], fx["G"]), full)
        assert same_bits(sa.c_moran(fx["A"], fx["G"], genes=sub), full[:, sub])
        # log-normalised values of a counts-only matrix: the resident values are what the restatement is given
        counts, _ = as_matrix(sa, gene_matrix(n, (1, 63, 64, 65, 200, n), 31, extra=False), n)
        c.upload(counts, None)
        c.log_normalize(10000.0)
        x, i, p = c.download(1)                       # t(A): one column per gene
        assert np.isfinite(x).all() and not np.all(x == np.round(x))
        want = mo.moran_moments(x, i, p.astype(np.int64), n, *fx["graph"])
        got = c.moran(fx["G"])
        assert same_bits(got, want), [r for r in range(6) if not same_bits(got[r], want[r])]
    # after a dense upload: the CSC image holds the non-zeros
    rng = np.random.default_rng(6)
    D = rng.poisson(0.4, (9, 257)).astype(np.float64)
    D[3] = 2.0                                        # a constant gene, stored in every cell
    Gx, Gi, Gp = edge_graph(257, 8)
    G = sa.dgCMatrix(Gx, Gi, Gp, (257, 257))
    _, T = as_matrix(sa, [(np.nonzero(r)[0], r[np.nonzero(r)[0]]) for r in D], 257)
    with sa.Context(0) as c:
        c.upload_dense(D)
        got = c.moran(G)
    assert same_bits(got, mo.moran_moments(*T, 257, Gx, Gi, Gp))
    assert got[1, 3] == 0.0                           # M2 of the constant gene: I is NaN in the assembly
    S0, S1, S2, _ = mo.graph_moments(Gx, Gi, Gp, 257)
    st = sa.moran_stats(257, S0, S1, S2, got)
    assert np.isnan(st["I"][3]) and np.isnan(st["p"][3]) and np.isfinite(np.delete(st["I"], 3)).all()


# ----------------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("n", [5, 257, 3000])
@pytest.mark.parametrize("k", [1, 3, 50])
def test_embedding_form_equals_the_restatement_bit_for_bit(sa, k, n):
    rng = np.random.default_rng(1000 * k + n)
    F = rng.normal(size=(k, n)) * rng.random((k, 1)) * 3 + rng.random((k, 1)) * 5
    Gx, Gi, Gp = edge_graph(n, n + k)
    G = sa.dgCMatrix(Gx, Gi, Gp, (n, n))
    want, mean = mo.embedding_moments(F, Gx, Gi, Gp)
    got, gmean = sa.c_moran_embedding(F, G)
    assert same_bits(gmean, mean)
    assert same_bits(got, want), [r for r in range(6) if not same_bits(got[r], want[r])]
    with sa.Context(0) as c:
        r1 = c.moran_embedding(G, F)
        c.hold_embedding(F)
        r2 = c.moran_embedding(G)
        c.hold_embedding(None)
    assert same_bits(r1[0], want) and same_bits(r2[0], want) and same_bits(r2[1], mean)
    S0, S1, S2, _ = mo.graph_moments(Gx, Gi, Gp, n)
    assert same_bits(sa.moran_stats(n, S0, S1, S2, got)["I"], mo.stats(n, S0, S1, S2, want)["I"])


def test_embedding_of_the_fit_is_read_in_place_and_the_fit_continues_unchanged(sa, ora):
    A = ora.synth_csc(120, 400, 10)
    dA = sa.dgCMatrix(A.x, A.i, A.p, (A.nrow, A.ncol))
    Gx, Gi, Gp = edge_graph(400, 3)
    G = sa.dgCMatrix(Gx, Gi, Gp, (400, 400))

    def fit(with_call):
        with sa.Context(0) as c:
            c.upload(dA, None)
            c.fit_init(6, None)
            for _ in range(2):
                c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            H = c.get_factors()[2]
            out = (c.moran_embedding(G), c.moran(G), sa.moran_factors(c, G)) if with_call else None
            for _ in range(2):
                c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            return H, out, c.get_factors()
    H, out, after = fit(True)
    _, _, plain = fit(False)
    want, mean = mo.embedding_moments(H.T, Gx, Gi, Gp)
    assert same_bits(out[0][0], want) and same_bits(out[0][1], mean)
    assert all(same_bits(a, b) for a, b in zip(after, plain)), "the fit's iterate changed after the calls"
    assert out[2]["I"].shape == (6,) and same_bits(out[2]["mean"], mean)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable(sa):
    fx = small(sa)
    n, m = fx["n"], fx["want"].shape[1]
    G, (Gx, Gi, Gp) = fx["G"], fx["graph"]

    def refused(c, code, match, fn):
        dims = c.dims()
        with pytest.raises(sa.SingletHipError, match=match) as e:
            fn()
        assert e.value.code == code and c.dims() == dims

    with sa.Context(0) as c:
        refused(c, ESTATE, "no matrix resident", lambda: c.moran(G))
        refused(c, ESTATE, "no matrix resident", lambda: c.op_moran_cross(G))
        refused(c, ESTATE, "no fit is initialised", lambda: c.moran_embedding(G))
        c.upload(fx["A"], None)
        small_G = sa.dgCMatrix(Gx[:0], Gi[:0], np.zeros(n, dtype=np.int32), (n - 1, n - 1))
        refused(c, EINVAL, "must be n x n", lambda: c.moran(small_G))
        unsorted = sa.dgCMatrix(np.ones(2), np.array([5, 2], dtype=np.int32), np.concatenate(([0], np.full(n, 2))).astype(np.int32), (n, n))
        refused(c, EINVAL, "not strictly ascending", lambda: c.moran(unsorted))
        nonfinite = sa.dgCMatrix(np.array([np.nan]), np.array([5], dtype=np.int32), np.concatenate(([0], np.full(n, 1))).astype(np.int32), (n, n))
        refused(c, EINVAL, "non-finite", lambda: c.moran(nonfinite))
        zero = sa.dgCMatrix(np.array([1.0, -1.0]), np.array([2, 5], dtype=np.int32), np.concatenate(([0], np.full(n, 2))).astype(np.int32), (n, n))
        refused(c, EINVAL, "S0 = 0", lambda: c.moran(zero))
        assert c.op_moran_cross(zero).shape == (m,)                       # the cross term alone needs no S0
        refused(c, EINVAL, r"genes\[2\] = %d is outside" % m, lambda: c.moran(G, genes=[0, 1, m]))
        refused(c, EINVAL, r"genes\[1\] = -1 is outside", lambda: c.moran(G, genes=[0, -1]))
        refused(c, EINVAL, r"genes\[3\] = 1 is listed twice", lambda: c.moran(G, genes=[0, 1, 2, 1]))
        refused(c, EINVAL, "path = 3", lambda: c.op_moran_cross(G, path=3))
        refused(c, EINVAL, "negative", lambda: c.op_moran_cross(G, lds_cap=-1))
        refused(c, EINVAL, "negative", lambda: c.op_moran_cross(G, table_batch=-1))
        refused(c, EINVAL, "k = 1025", lambda: c.moran_embedding(G, np.zeros((1025, n))))
        with pytest.raises(ValueError, match="columns"):
            c.moran_embedding(G, np.zeros((2, n - 1)))
        c.set_allreduce(lambda dev_ptr, count: None)
        refused(c, ESTATE, "all-reduce hook", lambda: c.moran(G))
        refused(c, ESTATE, "all-reduce hook", lambda: c.moran_embedding(G, np.zeros((2, n))))
        c.set_allreduce(None)
        c.upload(fx["A"], None, cell_offset=n, ncells_total=3 * n)
        refused(c, ESTATE, "shard", lambda: c.moran(G))
        refused(c, ESTATE, "shard", lambda: c.op_moran_cross(G))
        # usable afterwards
        c.upload(fx["A"], None)
        assert same_bits(c.moran(G), fx["want"])
    tiny = sa.dgCMatrix(np.ones(2), np.array([1, 0], dtype=np.int32), np.array([0, 1, 2, 2], dtype=np.int32), (3, 3))
    with pytest.raises(sa.SingletHipError, match="at least 4") as e:
        sa.c_moran(sa.dgCMatrix(np.ones(1), np.zeros(1, dtype=np.int32), np.array([0, 1, 1, 1], dtype=np.int32), (2, 3)), tiny)
    assert e.value.code == EINVAL
    with pytest.raises(sa.SingletHipError, match="at least 4"):
        sa.c_moran_embedding(np.ones((2, 3)), tiny)


def test_a_team_member_is_refused(sa):
    fx = small(sa)
    with sa.Multi([0, 0]) as team:
        team.upload(fx["A"])
        rank = team.rank_ctx(0)
        for call in (lambda: rank.moran(fx["G"]), lambda: rank.op_moran_cross(fx["G"]),
                     lambda: rank.moran_embedding(fx["G"], np.zeros((2, fx["n"])))):
            with pytest.raises(sa.SingletHipError, match="team") as e:
                call()
            assert e.value.code == ESTATE


# ---------------------------------------------------------------------------------------------------------- end to end
def test_planted_tissue_end_to_end(sa):
    D, (Gx, Gi, Gp), which, (S0, S1, S2), mom, st = planted_tables()
    m, n = D.shape
    from scipy import sparse
    A = sa.as_dgCMatrix(sparse.csc_matrix(D))
    G = sa.dgCMatrix(Gx, Gi, Gp, (n, n))
    out = sa.find_spatially_variable_features(A, graph=G, nfeatures=10)
    assert same_bits(out["moments"], mom)
    for key in ("I", "EI", "sd", "z"):
        assert same_bits(out[key], st[key]), key
    assert np.allclose(out["p"], st["p"], rtol=2.2e-12, atol=0) and np.allclose(out["p_adj"], st["p_adj"], rtol=2.2e-12, atol=0)
    planted_claims(out, which, m)
    assert sorted(out["features"].tolist()) == which.tolist()
    # through coordinates: spatial_graph of the unit grid with a radius between 1 and sqrt 2 is the rook graph, weighted
    side = int(round(np.sqrt(n)))
    xy = np.stack([np.arange(n) % side, np.arange(n) // side], axis=1).astype(np.float64)
    with sa.Context(0) as c:
        c.upload(A, None)
        by_xy = sa.find_spatially_variable_features(c, coords=xy, max_dist=1.2, features=np.arange(m)[::-1].copy(), nfeatures=10)
    assert sorted(by_xy["features"].tolist()) == which.tolist()
    assert by_xy["genes"].tolist() == list(range(m))[::-1]


# ------------------------------------------------------------------------------------------------- the caller's stream
def test_moran_on_a_stalled_caller_stream(sa):
    """sgl_set_stream's contract for sgl_moran, sgl_op_moran_cross (both paths) and sgl_moran_embedding: all work goes to the
    caller's stream and the host reads wait for it, so a stall at the head of that stream changes no bit."""
    fx = small(sa)
    F = np.random.default_rng(2).normal(size=(3, fx["n"]))
    calls = [("moran", lambda c: c.moran(fx["G"])),
             ("cross, table", lambda c: c.op_moran_cross(fx["G"], path=2, table_batch=2)),
             ("cross, search", lambda c: c.op_moran_cross(fx["G"], path=1)),
             ("embedding", lambda c: c.moran_embedding(fx["G"], F))]
    with contexts(sa) as c:
        c.upload(fx["A"], None)
        want = {name: call(c) for name, call in calls}
    assert same_bits(want["moran"], fx["want"])
    with contexts(sa) as c, caller_stream(c) as S:
        sc = Stalled(c, S)
        sc.upload(fx["A"], None)
        got = {name: call(sc) for name, call in calls}
    for name, _ in calls:
        assert_same_bits(got[name], want[name], name)
