"""Neighbourhood enrichment on the device (sgl_nhood_enrichment, sgl_op_nhood_tally, sgl_op_nhood_permute and their forms;
kernels_nhood.hip) against the numpy restatement (nhood_restatement.py), equal in every integer: the tally at every size at which
a loop turns (n = 1, 2, 63, 64, 65, 9000; nb = 1, 15, 16, 17, 33), on the graph's edge cases (empty first and last columns,
degree 1, hubs of 65, 300 and 9000 entries, self-loops with and without drop_diagonal, repeated and unsorted rows, no counted
entry), at K = 1, 2, 3, at both sides of every step of the plan and at K = 256, the LDS path against the global path and every
admissible forced perms_per_group; the permutations at both sides of the sort switch and across sort chunks; the whole call
whatever the batch, one-shot and on a context, twice in a row, beside a running fit; every refusal; the planted fixture end to
end through coordinates; the caller's-stream contract.  References are computed once and shared."""
import numpy as np
import pytest

import nhood_restatement as nh
from test_gpu_caller_stream import Stalled, assert_same_bits, caller_stream, contexts

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -6
SIZES = (1, 2, 63, 64, 65, 9000)
K_EDGES = (45, 46, 64, 65, 90, 91, 128, 129, 181, 182, 256)
TALLIES = ("counts", "S1", "S2", "n_ge", "n_le")
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def edge_graph(n, seed):
    """Columns 0 and n - 1 empty (n >= 3), column 1 of degree 1, hubs of 65, 300 and 9000 entries in columns 2, 3, 4 (drawn with
    replacement, so rows repeat; the last spans three 4096-entry segments), every other column 1 - 12 rows in any order with
    repeats, a self-loop on every 7th.  (Gi, Gp) int32."""
    rng = np.random.default_rng(seed)
    Gi, Gp = [], [0]
    for j in range(n):
        if n >= 3 and j in (0, n - 1):
            rows = np.zeros(0, dtype=np.int64)
        else:
            deg = {1: 1, 2: 65, 3: 300, 4: 9000}.get(j, int(rng.integers(1, 13))) if n > 65 else int(rng.integers(1, 13))
            rows = rng.integers(0, n, deg)
            if j % 7 == 0:
                rows[0] = j
        Gi.extend(rows.tolist())
        Gp.append(len(Gi))
    return np.array(Gi, dtype=np.int32), np.array(Gp, dtype=np.int32)


def graph_of(sa, n):
    def make():
        Gi, Gp = edge_graph(n, 40 + n)
        return Gi, Gp, sa.dgCMatrix(np.ones(Gi.shape[0]), Gi, Gp, (n, n))
    return cached(("graph", n), make)


def labels_of(n, nb, K, seed):
    labs = np.random.default_rng(seed).integers(0, K, (nb, n)).astype(np.int32)
    if K > 3:
        labs[labs == 1] = 0                                  # class 1 has no cell
    return labs


def restated_tally(Gi, Gp, labs, K, drop):
    return np.stack([nh.tally(Gi, Gp, row, K, drop) for row in labs])


def info_fields(info):
    return {q: info[q] for q in ("path", "perms_per_group", "lds_bytes")}


# ------------------------------------------------------------------------------------------------------------ the tally
@pytest.mark.parametrize("n", SIZES)
def test_tally_equals_the_restatement_at_every_size_path_and_group(sa, n):
    Gi, Gp, G = graph_of(sa, n)
    if n == 9000:
        assert np.diff(Gp)[[0, 1, 2, 3, 4, n - 1]].tolist() == [0, 1, 65, 300, 9000, 0] and Gp[-1] > 3 * nh.SEG
    with sa.Context(0) as c:
        for K in (1, 2, 3):
            for nb in ((1, 15, 16, 17, 33) if n in (65, 9000) else (1, 17)):
                labs = labels_of(n, nb, K, 7 * n + nb + K)
                for drop in (True, False):
                    want = restated_tally(Gi, Gp, labs, K, drop)
                    lds = c.op_nhood_tally(G, labs, K, drop)
                    info = c.nhood_info()
                    glob = c.op_nhood_tally(G, labs, K, drop, path=2)
                    assert lds.dtype == np.int64 and np.array_equal(lds, want), (K, nb, drop)
                    assert np.array_equal(glob, want), (K, nb, drop)
                    assert info_fields(info) == {"path": 1, "perms_per_group": 16, "lds_bytes": 16 * K * K * 4}
                    assert info_fields(c.nhood_info()) == {"path": 2, "perms_per_group": 16, "lds_bytes": 0}
            if n in (65, 9000):
                labs = labels_of(n, 33, K, n + K)
                want = restated_tally(Gi, Gp, labs, K, True)
                for path in (1, 2):
                    for pg in (1, 2, 4, 8, 16):
                        assert np.array_equal(c.op_nhood_tally(G, labs, K, True, path=path, perms_per_group=pg), want), (K, path, pg)
                        assert c.nhood_info()["perms_per_group"] == pg and c.nhood_info()["path"] == path


@pytest.mark.parametrize("K", K_EDGES)
def test_tally_at_both_sides_of_every_step_of_the_plan(sa, K):
    n, nb = 9000, 33
    Gi, Gp, G = graph_of(sa, n)
    labs = labels_of(n, nb, K, K)
    want = cached(("want", K), lambda: restated_tally(Gi, Gp, labs, K, True))
    plan = nh.plan(n, K, nb)
    with sa.Context(0) as c:
        got = c.op_nhood_tally(G, labs, K)
        assert info_fields(c.nhood_info()) == {q: plan[q] for q in ("path", "perms_per_group", "lds_bytes")}
        assert np.array_equal(got, want)
        assert not got[:, 1, :].any() and not got[:, :, 1].any()                      # the class without cells
        assert np.array_equal(c.op_nhood_tally(G, labs, K, path=2), want)
        assert c.nhood_info()["path"] == 2
        assert np.array_equal(c.op_nhood_tally(G, labs, K, path=1), want)             # K >= 182: the global path all the same
        assert c.nhood_info()["path"] == plan["path"]
        cap = nh.pg_max(K)
        for pg in (1, 2, 4, 8, 16):
            if pg <= (cap or 16) and pg != plan["perms_per_group"]:
                assert np.array_equal(c.op_nhood_tally(G, labs[:17], K, perms_per_group=pg), want[:17]), pg
                assert c.nhood_info()["perms_per_group"] == pg
        if cap and cap < 16:                                                           # one step above what LDS holds at this K
            with pytest.raises(sa.SingletHipError, match="perms_per_group = %d" % (2 * cap)) as e:
                c.op_nhood_tally(G, labs, K, perms_per_group=2 * cap)
            assert e.value.code == EINVAL
            assert np.array_equal(c.op_nhood_tally(G, labs, K, path=2, perms_per_group=2 * cap), want)


def test_a_graph_without_a_counted_entry(sa):
    n = 100
    loops = sa.dgCMatrix(np.ones(n), np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32), (n, n))
    empty = sa.dgCMatrix(np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(n + 1, dtype=np.int32), (n, n))
    labs = labels_of(n, 5, 3, 1)
    with sa.Context(0) as c:
        for path in (1, 2):
            assert not c.op_nhood_tally(loops, labs, 3, True, path=path).any()
            assert not c.op_nhood_tally(empty, labs, 3, False, path=path).any()
            kept = c.op_nhood_tally(loops, labs, 3, False, path=path)
            assert np.array_equal(kept, restated_tally(np.arange(n), np.arange(n + 1), labs, 3, False)) and kept.sum() == 5 * n
        out = c.nhood_enrichment(loops, labs[0], 3, nperm=20, return_null=True)
        assert not out["counts"].any() and not out["null"].any() and (out["n_ge"] == 20).all() and (out["n_le"] == 20).all()
        st = sa.nhood_stats(20, *(out[q] for q in TALLIES))
        assert np.isnan(st["zscore"]).all() and (st["p_enriched"] == 1.0).all()


# ----------------------------------------------------------------------------------------------------- the permutations
@pytest.mark.parametrize("n", [1, 2, 65, 3000])
def test_permutations_equal_the_restatement_on_both_sides_of_the_sort_switch(sa, n, monkeypatch):
    lab = np.random.default_rng(n).integers(0, 256, n).astype(np.int32)
    want = cached(("perm", n), lambda: nh.permuted(lab, 5, 0, 35))
    with sa.Context(0) as c:
        for switch, sort in ((None, 0), ("64", int(n > 64)), ("1", int(n > 1))):
            if switch is None:
                monkeypatch.delenv("SGL_NHOOD_SORT_SWITCH", raising=False)
            else:
                monkeypatch.setenv("SGL_NHOOD_SORT_SWITCH", switch)
            got = c.op_nhood_permute(lab, seed=5, r0=0, nb=35)
            assert c.nhood_info()["sort"] == sort
            assert got.dtype == np.int32 and np.array_equal(got, want), (switch,)
            assert np.array_equal(c.op_nhood_permute(lab, seed=5, r0=16, nb=3), want[16:19])       # r0 is honoured
            assert np.array_equal(c.op_nhood_permute(lab, seed=5, r0=33, nb=1), want[33:34])
        monkeypatch.delenv("SGL_NHOOD_SORT_SWITCH", raising=False)
        if n >= 65:
            assert not np.array_equal(c.op_nhood_permute(lab, seed=6, r0=0, nb=1), want[:1])


def ring(sa, n):
    """Every cell with the two cells after it and the seventh: rows unsorted at the wrap."""
    c = np.arange(n, dtype=np.int64)
    Gi = np.stack([(c + 1) % n, (c + 7) % n, (c + 2) % n], axis=1).reshape(-1).astype(np.int32)
    Gp = (3 * np.arange(n + 1)).astype(np.int32)
    return Gi, Gp, sa.dgCMatrix(np.ones(Gi.shape[0]), Gi, Gp, (n, n))


def test_a_size_above_the_sort_switch_with_more_than_one_sort_chunk(sa):
    """600 000 cells: above the default switch (one device-wide sort per permutation), 16 permutations per sort chunk, so 19
    permutations take two chunks and two groups; the entries take several segments per workgroup."""
    n, K, nperm = 600_000, 5, 19
    lab = np.random.default_rng(3).integers(0, K, n).astype(np.int32)
    Gi, Gp, G = ring(sa, n)
    P = nh.permuted(lab, 9, 0, nperm)
    N = np.stack([nh.tally(Gi, Gp, row, K, True) for row in P])
    want = nh.tallies(nh.tally(Gi, Gp, lab, K, True), N)
    with sa.Context(0) as c:
        assert np.array_equal(c.op_nhood_permute(lab, seed=9, r0=2, nb=17), P[2:19])
        assert c.nhood_info()["sort"] == 1 and c.nhood_info()["batches"] == 2
        out = c.nhood_enrichment(G, lab, K, nperm=nperm, seed=9, return_null=True)
        info = c.nhood_info()
    assert np.array_equal(out["null"], N)
    for q in TALLIES:
        assert np.array_equal(out[q], want[q]), q
    assert (info["path"], info["perms_per_group"], info["sort"], info["batches"], info["batch"]) == (1, 16, 1, 1, 19)


# ------------------------------------------------------------------------------------------------------- the whole call
def whole(sa):
    def make():
        n, K, nperm, seed = 3000, 4, 40, 17
        Gi, Gp = edge_graph(n, 77)
        lab = np.random.default_rng(8).integers(0, K, n).astype(np.int32)
        lab[lab == 3] = 2                                    # class 3 has no cell: NaN in z
        return dict(n=n, K=K, nperm=nperm, seed=seed, Gi=Gi, Gp=Gp, lab=lab, G=sa.dgCMatrix(np.ones(Gi.shape[0]), Gi, Gp, (n, n)),
                    want=nh.enrichment(Gi, Gp, lab, K, nperm, seed, True), want_kept=nh.enrichment(Gi, Gp, lab, K, nperm, seed, False))
    return cached("whole", make)


def test_whole_call_equals_the_restatement_whatever_the_batch(sa, monkeypatch):
    fx = whole(sa)
    want = fx["want"]
    with sa.Context(0) as c:
        for batch, batches in ((1, 40), (7, 6), (40, 1), (0, 1)):
            out = c.nhood_enrichment(fx["G"], fx["lab"], fx["K"], nperm=fx["nperm"], seed=fx["seed"], batch=batch, return_null=True)
            info = c.nhood_info()
            for q in TALLIES + ("null",):
                assert out[q].dtype == np.int64 and np.array_equal(out[q], want[q]), (batch, q)
            assert (info["batches"], info["batch"], info["path"], info["perms_per_group"], info["sort"]) == (batches, batch or 40, 1, 16, 0)
        again = c.nhood_enrichment(fx["G"], fx["lab"], fx["K"], nperm=fx["nperm"], seed=fx["seed"], return_null=True)
        assert all(np.array_equal(again[q], out[q]) for q in out)
        monkeypatch.setenv("SGL_NHOOD_SORT_SWITCH", "100")                              # the device-wide sort: the same integers
        wide = c.nhood_enrichment(fx["G"], fx["lab"], fx["K"], nperm=fx["nperm"], seed=fx["seed"], batch=7, return_null=True)
        assert c.nhood_info()["sort"] == 1 and all(np.array_equal(wide[q], out[q]) for q in out)
        monkeypatch.delenv("SGL_NHOOD_SORT_SWITCH")
        kept = c.nhood_enrichment(fx["G"], fx["lab"], fx["K"], nperm=fx["nperm"], seed=fx["seed"], drop_diagonal=False)
        assert all(np.array_equal(kept[q], fx["want_kept"][q]) for q in TALLIES) and not np.array_equal(kept["counts"], out["counts"])
        assert c.nhood_enrichment(fx["G"], fx["lab"], 4, nperm=3, seed=1)["counts"].tolist() == want["counts"].tolist()
        other = c.nhood_enrichment(fx["G"], fx["lab"], fx["K"], nperm=fx["nperm"], seed=fx["seed"] + 1)
        assert np.array_equal(other["counts"], want["counts"]) and not np.array_equal(other["S2"], want["S2"])
    # the statistics: bit for bit nhood_stats on those integers, which is bit for bit the restatement
    st = sa.nhood_stats(fx["nperm"], *(out[q] for q in TALLIES))
    one = sa.c_nhood_enrichment(fx["G"], fx["lab"], fx["K"], nperm=fx["nperm"], seed=fx["seed"], batch=7, return_null=True, timing=True)
    for q in TALLIES + ("null",):
        assert np.array_equal(one[q], want[q]), q
    for q in st:
        assert st[q].tobytes() == one[q].tobytes(), q
        assert np.array_equal(st[q], want[q], equal_nan=True), q
    assert np.isnan(st["zscore"][3]).all() and np.isnan(st["zscore"][:, 3]).all() and np.isfinite(st["zscore"][:3, :3]).all()
    assert one["info"]["batches"] == 6 and one["stage_ms"].shape == (3,) and (one["stage_ms"] > 0).all()


def test_a_fit_in_progress_continues_with_its_bits(sa, ora):
    fx = whole(sa)
    A = ora.synth_csc(120, 400, 10)
    dA = sa.dgCMatrix(A.x, A.i, A.p, (A.nrow, A.ncol))

    def fit(with_call):
        with sa.Context(0) as c:
            c.upload(dA, None)
            c.fit_init(6, None)
            for _ in range(2):
                c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            out = c.nhood_enrichment(fx["G"], fx["lab"], fx["K"], nperm=fx["nperm"], seed=fx["seed"]) if with_call else None
            if with_call:
                c.op_nhood_permute(fx["lab"], nb=3)
                c.op_nhood_tally(fx["G"], fx["lab"][None, :], fx["K"])
            for _ in range(2):
                c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            return out, c.get_factors(), c.dims()
    out, after, dims = fit(True)
    _, plain, dims0 = fit(False)
    assert all(np.array_equal(out[q], fx["want"][q]) for q in TALLIES) and dims == dims0
    assert all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(after, plain)), "the fit's iterate changed"


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable(sa):
    from singlet_amd import _lib
    from singlet_amd._lib import i32p, i64p, ptr
    fx = whole(sa)
    n, K, G, lab, Gi, Gp = fx["n"], fx["K"], fx["G"], fx["lab"], fx["Gi"], fx["Gp"]
    L = _lib.load()

    def graph(i, p):
        return sa.dgCMatrix(np.ones(len(i)), np.asarray(i, dtype=np.int32), np.asarray(p, dtype=np.int32), (n, n))

    def refused(c, code, match, fn):
        with pytest.raises(sa.SingletHipError, match=match) as e:
            fn()
        assert e.value.code == code
        assert np.array_equal(c.op_nhood_tally(G, lab[None, :], K)[0], fx["want"]["counts"])      # usable afterwards

    def raw(c, gi, gp, nn, lb, k=K, nperm=10, batch=0):
        out = np.zeros((256, 256), dtype=np.int64)
        rc = L.sgl_nhood_enrichment(c._h, ptr(gi, i32p), ptr(gp, i32p), nn, ptr(lb, i32p), k, 1, nperm, 0, batch, ptr(out, i64p), None, None, None, None, None)
        return rc, L.sgl_last_error().decode()

    with sa.Context(0) as c:
        for args in ((None, Gp, n, lab), (Gi, None, n, lab), (Gi, Gp, n, None)):
            rc, msg = raw(c, *args)
            assert rc == EINVAL and "NULL" in msg
        for nn in (0, -3):
            rc, msg = raw(c, Gi, Gp, nn, lab)
            assert rc == EINVAL and "n = %d" % nn in msg
        p = Gp.copy()
        p[0] = 1
        refused(c, EINVAL, r"Gp\[0\] = 1", lambda: c.nhood_enrichment(graph(Gi, p), lab, K))
        p = Gp.copy()
        p[5] = p[4] - 1
        refused(c, EINVAL, r"Gp\[5\] = %d" % p[5], lambda: c.nhood_enrichment(graph(Gi[:Gp[-1]], p), lab, K))
        i = Gi.copy()
        i[11] = n
        refused(c, EINVAL, r"Gi\[11\] = %d is outside \[0, %d\)" % (n, n), lambda: c.nhood_enrichment(graph(i, Gp), lab, K))
        i[11] = -1
        refused(c, EINVAL, r"Gi\[11\] = -1", lambda: c.op_nhood_tally(graph(i, Gp), lab[None, :], K))
        refused(c, EINVAL, r"K = 0 is outside \[1, 256\]", lambda: c.nhood_enrichment(G, lab, 0))
        refused(c, EINVAL, r"K = 257", lambda: c.nhood_enrichment(G, lab, 257))
        refused(c, EINVAL, r"K = 257", lambda: c.op_nhood_tally(G, lab[None, :], 257))
        bad = lab.copy()
        bad[123] = K
        refused(c, EINVAL, r"lab\[123\] = %d is outside \[0, %d\)" % (K, K), lambda: c.nhood_enrichment(G, bad, K))
        bad[123] = -2
        refused(c, EINVAL, r"lab\[123\] = -2", lambda: c.nhood_enrichment(G, bad, K))
        refused(c, EINVAL, r"lab\[%d\] = -2" % (n + 123), lambda: c.op_nhood_tally(G, np.stack([lab, bad]), K))
        refused(c, EINVAL, r"nperm = 0 is outside", lambda: c.nhood_enrichment(G, lab, K, nperm=0))
        refused(c, EINVAL, r"nperm = 1048577", lambda: c.nhood_enrichment(G, lab, K, nperm=(1 << 20) + 1))
        refused(c, EINVAL, r"batch = -1 is negative", lambda: c.nhood_enrichment(G, lab, K, batch=-1))
        # nperm * nnz^2 at its boundary: 2^22 stored entries take nperm up to 2^19 - 1
        big_p = np.zeros(n + 1, dtype=np.int32)
        big_p[1:] = 1 << 22
        big = graph(np.ones(1 << 22, dtype=np.int32), big_p)                              # column 0 holds row 1 2^22 times: a hub, too
        refused(c, EINVAL, r"largest nperm that fits is 524287", lambda: c.nhood_enrichment(big, lab, K, nperm=1 << 19))
        hub = c.nhood_enrichment(big, lab, K, nperm=2, seed=0)
        assert hub["counts"][lab[0], lab[1]] == 1 << 22 and hub["counts"].sum() == 1 << 22 and hub["S1"].sum() == 2 << 22
        # the knobs of the stage operators
        refused(c, EINVAL, r"path = 3", lambda: c.op_nhood_tally(G, lab[None, :], K, path=3))
        refused(c, EINVAL, r"perms_per_group = 3", lambda: c.op_nhood_tally(G, lab[None, :], K, perms_per_group=3))
        refused(c, EINVAL, r"perms_per_group = 32", lambda: c.op_nhood_tally(G, lab[None, :], K, path=2, perms_per_group=32))
        refused(c, EINVAL, r"perms_per_group = -1", lambda: c.op_nhood_tally(G, lab[None, :], K, perms_per_group=-1))
        refused(c, EINVAL, r"nb = 0", lambda: c.op_nhood_tally(G, lab[:0].reshape(0, n), K))
        refused(c, EINVAL, r"not 0 <= r0", lambda: c.op_nhood_permute(lab, r0=-1, nb=1))
        refused(c, EINVAL, r"not 0 <= r0", lambda: c.op_nhood_permute(lab, r0=0, nb=0))
        refused(c, EINVAL, r"not 0 <= r0", lambda: c.op_nhood_permute(lab, r0=(1 << 20) - 1, nb=2))
        refused(c, EINVAL, r"lab\[123\] = 256 is outside \[0, 256\)", lambda: c.op_nhood_permute(np.where(np.arange(n) == 123, 256, lab)))
        with pytest.raises(ValueError, match="integer class"):
            c.nhood_enrichment(G, lab[:-1], K)
        with pytest.raises(ValueError, match="nb x n"):
            c.op_nhood_tally(G, lab, K)
        # the states of sgl_moran
        c.set_allreduce(lambda dev_ptr, count: None)
        refused_state = []
        for call in (lambda: c.nhood_enrichment(G, lab, K), lambda: c.op_nhood_tally(G, lab[None, :], K), lambda: c.op_nhood_permute(lab)):
            with pytest.raises(sa.SingletHipError, match="all-reduce hook") as e:
                call()
            refused_state.append(e.value.code)
        assert refused_state == [ESTATE] * 3
        c.set_allreduce(None)
        A = sa.dgCMatrix(np.ones(3), np.array([0, 1, 2], dtype=np.int32), np.array([0, 1, 2, 3], dtype=np.int32), (5, 3))
        c.upload(A, None, cell_offset=3, ncells_total=9)
        with pytest.raises(sa.SingletHipError, match="shard") as e:
            c.nhood_enrichment(G, lab, K)
        assert e.value.code == ESTATE
        c.upload(A, None)                                                               # a whole matrix resident: no obstacle
        out = c.nhood_enrichment(G, lab, K, nperm=fx["nperm"], seed=fx["seed"])
        assert all(np.array_equal(out[q], fx["want"][q]) for q in TALLIES) and c.dims()[:2] == (5, 3)
    # the one-shot form refuses before it makes a context
    with pytest.raises(sa.SingletHipError, match=r"lab\[123\] = -2") as e:
        sa.c_nhood_enrichment(G, bad, K)
    assert e.value.code == EINVAL


def test_a_team_member_is_refused(sa):
    fx = whole(sa)
    A = sa.dgCMatrix.from_dense(np.random.default_rng(0).poisson(0.5, (30, 200)).astype(np.float64))
    with sa.Multi([0, 0]) as team:
        team.upload(A)
        rank = team.rank_ctx(0)
        for call in (lambda: rank.nhood_enrichment(fx["G"], fx["lab"], fx["K"]), lambda: rank.op_nhood_tally(fx["G"], fx["lab"][None, :], fx["K"]),
                     lambda: rank.op_nhood_permute(fx["lab"])):
            with pytest.raises(sa.SingletHipError, match="team") as e:
                call()
            assert e.value.code == ESTATE


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("seed", [0, 1, 7])
def test_planted_fixture_end_to_end_through_coordinates(sa, seed):
    from test_nhood_restatement import planted_reference
    Gi, Gp, lab, want = planted_reference(seed)
    side = 24
    xy = np.stack([np.arange(side * side) % side, np.arange(side * side) // side], axis=1).astype(np.float64)
    out = sa.nhood_enrichment(lab, coords=xy, max_dist=1.5, nperm=200, seed=seed)                # spatial_graph: the 8 neighbours (and the diagonal, dropped)
    assert sorted(out) == sorted(("counts", "zscore", "mean", "sd", "p_enriched", "p_depleted", "p_adj_enriched", "p_adj_depleted", "n_ge", "n_le",
                                  "class_sizes"))
    nh.planted_claims(out, 200)
    for q in out:
        if q != "class_sizes":
            assert np.array_equal(out[q], want[q], equal_nan=True), q
    assert out["class_sizes"].tolist() == np.bincount(lab, minlength=3).tolist()
    if seed == 0:
        G = sa.dgCMatrix(np.ones(Gi.shape[0]), Gi, Gp, (side * side, side * side))
        by_graph = sa.nhood_enrichment(lab.reshape(-1, 1), graph={"snn": G}, nperm=200, seed=seed, batch=9)
        assert all(np.array_equal(by_graph[q], out[q], equal_nan=True) for q in out)
        im = sa.interaction_matrix(lab, G)
        assert im.dtype == np.int64 and im.tolist() == nh.PLANTED_COUNTS
        norm = sa.interaction_matrix(lab, G.to_scipy(), normalized=True)
        assert np.array_equal(norm, im / im.sum(axis=1, keepdims=True)) and np.allclose(norm.sum(axis=1), 1.0)
        four = sa.interaction_matrix(lab, G, normalized=True, n_classes=4)
        assert four.shape == (4, 4) and not four[3].any() and not four[:, 3].any()


# ------------------------------------------------------------------------------------------------- the caller's stream
def test_nhood_on_a_stalled_caller_stream(sa):
    """sgl_set_stream's contract for sgl_nhood_enrichment, sgl_op_nhood_tally (both paths) and sgl_op_nhood_permute: all work
    goes to the caller's stream and the host reads wait for it, so a stall at the head of that stream changes no value."""
    fx = whole(sa)
    G, lab, K = fx["G"], fx["lab"], fx["K"]
    labs = labels_of(fx["n"], 17, K, 4)
    calls = [("whole", lambda c: c.nhood_enrichment(G, lab, K, nperm=fx["nperm"], seed=fx["seed"], batch=7, return_null=True)),
             ("tally, LDS", lambda c: c.op_nhood_tally(G, labs, K, path=1)),
             ("tally, global", lambda c: c.op_nhood_tally(G, labs, K, path=2)),
             ("permute", lambda c: c.op_nhood_permute(lab, seed=3, r0=1, nb=18))]
    with contexts(sa) as c:
        want = {name: call(c) for name, call in calls}
    assert all(np.array_equal(want["whole"][q], fx["want"][q]) for q in TALLIES + ("null",))
    with contexts(sa) as c, caller_stream(c) as S:
        sc = Stalled(c, S)
        got = {name: call(sc) for name, call in calls}
    for name, _ in calls:
        assert_same_bits(got[name], want[name], name)
