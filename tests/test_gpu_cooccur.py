"""Co-occurrence by distance on the device (sgl_cooccur, sgl_op_cooccur_tally, sgl_c_cooccur; kernels_cooccur.hip) against the
numpy restatement (cooccur_restatement.py), equal in every integer: at every size at which a tile turns, in every grid mode and on
both bin paths; on exact ties, duplicated points and bucket borders; under coordinate offsets; on skewed bucket occupancy; at both
sides of the LDS / global switch; across early flushes; past the first pass of each capped launch; the whole call against the
operator and the one-shot form, beside a running fit, after every refusal, on a stalled caller's stream; the planted fixture and
the Poisson pattern end to end.  References are computed once and shared."""
import numpy as np
import pytest

import cooccur_restatement as co
from test_gpu_caller_stream import Stalled, assert_same_bits, caller_stream, contexts

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -6
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1500)
MODES = (0, 1, 2)
PATHS = (0, 1, 2)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def uniform(n, K, seed, scale=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    xy = offset + scale * rng.random((n, 2))
    lab = rng.integers(0, K, n).astype(np.int32)
    return xy, lab


def every_mode_and_path(c, xy, lab, K, r, want, modes=MODES, paths=PATHS, what=""):
    """The table on every grid mode and bin path, and what the info says ran."""
    for mode in modes:
        run = co.grid(xy[:, 0], xy[:, 1], float(r[-1]), mode)
        for path in paths:
            got = c.op_cooccur_tally(xy, lab, r, K, grid_mode=mode, bin_path=path)
            info = c.cooccur_info()
            assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (what, mode, path)
            plan = co.plan(xy.shape[0], K, len(r) - 1, run[0], path)
            assert (info["grid_mode"], info["W"], info["H"]) == run, (what, mode, info)
            assert (info["bin_path"], info["lds_bytes"], info["workgroups"]) == (plan["bin_path"], plan["lds_bytes"], plan["workgroups"]), (what, mode, path, info)
            assert info["flushes"] <= info["workgroups"] and (info["flushes"] == 0) == (plan["bin_path"] == 2 or info["pairs"] == 0)


# ----------------------------------------------------------------------------------------------------------- tile edges
@pytest.mark.parametrize("n", SIZES)
def test_tally_equals_the_restatement_at_every_size_mode_and_path(sa, n):
    K, T = 5, 7
    xy, lab = uniform(n, K, 100 + n)
    r = np.linspace(0.0, 0.15, T + 1)                              # side 0.15: a grid of 8 x 8 buckets by the plan, once the points span the square
    want = cached(("size", n), lambda: co.tally(xy[:, 0], xy[:, 1], lab, K, r))
    assert n < 65 or co.grid(xy[:, 0], xy[:, 1], 0.15)[0] == 2
    with sa.Context(0) as c:
        every_mode_and_path(c, xy, lab, K, r, want, what=n)
        wide = co.default_interval(xy[:, 0], xy[:, 1], T) if n > 1 else r       # squidpy's default regime: half the diagonal, one bucket by the plan
        got = c.op_cooccur_tally(xy, lab, wide, K)
        assert c.cooccur_info()["grid_mode"] == 1 and np.array_equal(got, co.tally(xy[:, 0], xy[:, 1], lab, K, wide))
        assert n <= 2 or got.sum() > 0
        assert np.array_equal(c.op_cooccur_tally(xy, lab, wide, K, grid_mode=2), got)


# ----------------------------------------------------------------------------------------------------------- exact ties
def lattice_with_duplicates():
    def make():
        ix, iy = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
        xy = np.stack([ix.reshape(-1), iy.reshape(-1)], axis=1).astype(np.float64)
        rng = np.random.default_rng(5)
        xy = np.concatenate([xy, xy[rng.integers(0, 1600, 60)]])                # 60 duplicated points: d2 == 0
        xy = xy[rng.permutation(xy.shape[0])]
        lab = rng.integers(0, 4, xy.shape[0]).astype(np.int32)
        d2 = co.d2_block(xy[:, 0], xy[:, 1], np.arange(xy.shape[0]))
        np.fill_diagonal(d2, -1.0)
        return xy, lab, d2
    return cached("lattice", make)


@pytest.mark.parametrize("r", [(0.0, 1.0, 2.0, 3.0, 5.0), (1.0, 2.0, 3.0, 5.0)])
def test_exact_ties_duplicates_and_bucket_borders(sa, r):
    """Integer coordinates and integer thresholds: many pairs have d2 == thr2[t] exactly; pairs at exactly r[T] = 5 straddle the
    borders of the buckets of side 5 (1 + 2^-10) (x = 5 and x = 10 are buckets 0 and 1).  d2 == thr2[t + 1] is in interval t, d2 ==
    thr2[0] is in none; duplicated points are in no interval when r[0] == 0 and in none when r[0] > 0 either."""
    xy, lab, d2 = lattice_with_duplicates()
    r = np.array(r)
    want = cached(("ties", len(r)), lambda: co.tally(xy[:, 0], xy[:, 1], lab, 4, r))
    assert (d2 == 0).sum() >= 120 and (d2 == 25.0).sum() > 0 and (d2 == 1.0).sum() > 0
    assert int(want[:, :, -1].sum()) == int(((d2 > 9.0) & (d2 <= 25.0)).sum())                 # boundary pairs are in
    assert int(want.sum()) == int(((d2 > r[0] ** 2) & (d2 <= 25.0)).sum())                     # d2 == thr2[0] is out (0 or 1)
    assert int(want[:, :, -3].sum()) == int(((d2 > 1.0) & (d2 <= 4.0)).sum())
    assert co.grid(xy[:, 0], xy[:, 1], 5.0) == (2, 9, 9)
    with sa.Context(0) as c:
        every_mode_and_path(c, xy, lab, 4, r, want, what="ties")


# --------------------------------------------------------------------------------------------------- coordinate offsets
@pytest.mark.parametrize("scale,offset", [(100.0, 1e9), (1e-3, 0.0), (1e-3, -1e9)])
def test_coordinate_offsets_keep_the_bits_of_dx(sa, scale, offset):
    """At 1e9 the coordinates carry 1.2e-7 of resolution and dx is exact where the stated d2 says so; at the 1e-3 scale the squares
    are ~1e-8; 1e-3 on top of -1e9 rounds the points onto a lattice of 1.2e-7, some 8000 nodes across: dx and dy are small integer
    multiples of 2^-23 there."""
    xy, lab = uniform(700, 3, 9, scale, offset)
    r = np.linspace(0.0, 0.12 * scale, 6)
    want = co.tally(xy[:, 0], xy[:, 1], lab, 3, r)
    assert want.sum() > 0
    with sa.Context(0) as c:
        every_mode_and_path(c, xy, lab, 3, r, want, what=(scale, offset))


# ----------------------------------------------------------------------------------------------------- skewed occupancy
def skewed(kind):
    rng = np.random.default_rng(21)
    if kind == "one bucket of a large grid":                      # 700 points in one bucket, one far point stretches the grid to ~10^4 x 10^4
        xy = np.concatenate([0.008 * rng.random((700, 2)), [[100.0, 100.0]]])
        reach = 0.01
    elif kind == "clump and field":
        xy = np.concatenate([0.5 + 0.01 * rng.standard_normal((600, 2)), rng.random((500, 2))])
        reach = 0.05
    elif kind == "one bucket row":
        xy = np.stack([rng.random(900), np.full(900, 0.5)], axis=1)
        reach = 0.02
    else:                                                          # one bucket column
        xy = np.stack([np.full(900, -3.0), rng.random(900)], axis=1)
        reach = 0.02
    xy = xy[rng.permutation(xy.shape[0])]
    return xy, rng.integers(0, 3, xy.shape[0]).astype(np.int32), np.linspace(0.0, reach, 5)


@pytest.mark.parametrize("kind", ["one bucket of a large grid", "clump and field", "one bucket row", "one bucket column"])
def test_skewed_bucket_occupancy(sa, kind):
    xy, lab, r = skewed(kind)
    want = co.tally(xy[:, 0], xy[:, 1], lab, 3, r)
    run = co.grid(xy[:, 0], xy[:, 1], float(r[-1]))
    assert run[0] == 2 and want.sum() > 0
    if kind == "one bucket of a large grid":
        assert run[1] > 9000 and run[2] > 9000
    if kind == "one bucket row":
        assert run[2] == 2 and run[1] > 40
    if kind == "one bucket column":
        assert run[1] == 2 and run[2] > 40
    with sa.Context(0) as c:
        every_mode_and_path(c, xy, lab, 3, r, want, what=kind)


# ------------------------------------------------------------------------------------------------------- bin-plan edges
@pytest.mark.parametrize("K,T", [(22, 64), (23, 64), (176, 1), (177, 1), (1, 1), (1, 64), (256, 1), (3, 64), (20, 50)])
def test_both_sides_of_the_lds_global_switch(sa, K, T):
    """T K^2 uint32 bins + 6144 bytes of staging against 128 KiB: (22, 64) and (176, 1) are the last that fit, (23, 64) and
    (177, 1) the first that do not."""
    assert co.lds_fits(K, T) == ((K, T) not in ((23, 64), (177, 1), (256, 1)))
    xy, lab = uniform(800, K, 3 * K + T)
    if K > 3:
        lab[lab == 1] = 0                                          # class 1 has no point
    r = np.linspace(0.0, 0.3, T + 1)
    want = cached(("switch", K, T), lambda: co.tally(xy[:, 0], xy[:, 1], lab, K, r))
    with sa.Context(0) as c:
        every_mode_and_path(c, xy, lab, K, r, want, what=(K, T))
        got = c.cooccur(xy, lab, r, K)
    assert np.array_equal(got, want)
    ratio = sa.cooccur_stats(got)
    assert np.array_equal(ratio, co.stats(want), equal_nan=True)
    if K > 3:
        assert not got[1].any() and not got[:, 1].any() and np.isnan(ratio[1]).all() and np.isnan(ratio[:, 1]).all()


# ------------------------------------------------------------------------------------------------------- flush crossing
def test_early_flushes_leave_the_table_unchanged(sa):
    """n = 1500 on the forced bucket grid: a workgroup stages several candidate tiles of up to 256 x 256 = 65 536 pairs, so a
    bound of 50 000 (and of 1) makes it flush before every stage after its first."""
    K, T = 5, 7
    xy, lab = uniform(1500, K, 100 + 1500)
    r = np.linspace(0.0, 0.15, T + 1)
    want = cached(("size", 1500), lambda: co.tally(xy[:, 0], xy[:, 1], lab, K, r))
    with sa.Context(0) as c:
        plain = c.op_cooccur_tally(xy, lab, r, K, grid_mode=2)
        base = c.cooccur_info()
        assert base["flushes"] == base["workgroups"] == 6 and np.array_equal(plain, want)
        for bound in (50000, 1):
            got = c.op_cooccur_tally(xy, lab, r, K, grid_mode=2, flush_pairs=bound)
            info = c.cooccur_info()
            assert np.array_equal(got, want), bound
            assert info["flushes"] > 1 and info["flushes"] > info["workgroups"] and info["pairs"] == base["pairs"], (bound, info)
            assert np.array_equal(c.op_cooccur_tally(xy, lab, r, K, grid_mode=1, flush_pairs=bound), want), bound
            assert np.array_equal(c.op_cooccur_tally(xy, lab, r, K, grid_mode=2, bin_path=2, flush_pairs=bound), want), bound
            assert c.cooccur_info()["flushes"] == 0                                             # the global path has nothing to flush


# ---------------------------------------------------------------------------------------------------------- capped grid
def jittered_lattice(n, h, seed, far_tail):
    """The first n nodes (e // h, e % h) of an integer lattice, each point jittered by < 0.1; with far_tail the last point sits
    alone at node (200, 200), far beyond the others."""
    e = np.arange(n)
    ix, iy = e // h, e % h
    if far_tail:
        ix[-1], iy[-1] = 200, 200
    rng = np.random.default_rng(seed)
    c1, c2 = ix + 0.1 * rng.random(n), iy + 0.1 * rng.random(n)
    return ix, iy, c1, c2, rng.integers(0, 3, n).astype(np.int32)


@pytest.mark.parametrize("n,h,far_tail", [(16385, 128, True), (262145, 512, False)])
def test_capped_launches_past_their_first_grid_pass(sa, n, h, far_tail):
    """The unit has two capped launches, each tested at the smallest n that gives it a second pass.  The extent reduction runs at
    most 64 workgroups of 256 threads, 16 384 points per pass: at n = 16 385 the stride loop's second pass holds exactly the last
    point, and that point alone sets xmax and ymax (node (200, 200) against 128 x 128 for the rest), so a skipped second pass gives
    W = H = 99 instead of 155.  The tally runs at most 1024 workgroups over the centre tiles of 256: n = 1024 x 256 + 1 = 262 145
    makes 1025 tiles, two per workgroup, the last workgroup taking tiles 1024 and 1025 (one point).  Points jittered by < 0.1
    around the nodes of an integer lattice with r[T] = 1.3 < 1.8: only the eight neighbouring nodes can hold a partner, so the
    restatement evaluates those pairs alone."""
    ix, iy, c1, c2, lab = jittered_lattice(n, h, n, far_tail)
    r = np.array([0.0, 0.95, 1.0, 1.05, 1.3])
    want = co.tally_offsets(ix, iy, c1, c2, lab, 3, r)
    run = co.grid(c1, c2, 1.3, 2)
    plan = co.plan(n, 3, 4, 2)
    assert plan["tiles_per_wg"] == (2 if n > 262144 else 1) and co.plan(n - 1, 3, 4, 2)["tiles_per_wg"] == 1 and run[0] == 2
    if far_tail:
        assert run[1:] == (155, 155) and co.grid(c1[:-1], c2[:-1], 1.3, 2)[1:] == (99, 99)
    with sa.Context(0) as c:
        for path in (1, 2):
            got = c.op_cooccur_tally((c1, c2), lab, r, 3, grid_mode=2, bin_path=path)
            info = c.cooccur_info()
            assert np.array_equal(got, want), path
            assert (info["grid_mode"], info["W"], info["H"]) == run and info["workgroups"] == plan["workgroups"]
    assert want.sum() > 3 * n                                                                    # the four axial neighbours of (almost) every node


# ------------------------------------------------------------------------------------------------------- the whole call
def whole():
    def make():
        K, T = 5, 7
        xy, lab = uniform(1500, K, 100 + 1500)
        r = np.linspace(0.0, 0.15, T + 1)
        return dict(xy=xy, lab=lab, K=K, T=T, r=r, want=cached(("size", 1500), lambda: co.tally(xy[:, 0], xy[:, 1], lab, K, r)))
    return cached("whole", make)


def test_whole_call_equals_the_operator_and_the_one_shot_call(sa):
    fx = whole()
    with sa.Context(0) as c:
        got = c.cooccur(fx["xy"], fx["lab"], fx["r"], fx["K"])
        info = c.cooccur_info()
        op = c.op_cooccur_tally(fx["xy"], fx["lab"], fx["r"], fx["K"])
        assert c.cooccur_info() == info and info["grid_mode"] == 2 and info["bin_path"] == 1
        again = c.cooccur((fx["xy"][:, 0], fx["xy"][:, 1]), fx["lab"].astype(np.int64), fx["r"])       # a pair of vectors, K from the labels
    one = sa.c_cooccur(fx["xy"], fx["lab"], fx["r"], fx["K"], timing=True)
    for t in (got, op, again, one["counts"]):
        assert t.dtype == np.int64 and np.array_equal(t, fx["want"])
    assert one["info"] == info and one["stage_ms"].shape == (3,) and (one["stage_ms"] > 0).all()
    assert one["ratio"].tobytes() == sa.cooccur_stats(got).tobytes() and np.array_equal(one["ratio"], co.stats(fx["want"]), equal_nan=True)
    assert np.array_equal(got, got.transpose(1, 0, 2)) and not (np.diagonal(got) % 2).any()


def test_a_fit_in_progress_continues_with_its_bits(sa, ora):
    fx = whole()
    A = ora.synth_csc(120, 400, 10)
    dA = sa.dgCMatrix(A.x, A.i, A.p, (A.nrow, A.ncol))

    def fit(with_call):
        with sa.Context(0) as c:
            c.upload(dA, None)
            c.fit_init(6, None)
            for _ in range(2):
                c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            out = c.cooccur(fx["xy"], fx["lab"], fx["r"], fx["K"]) if with_call else None
            if with_call:
                c.op_cooccur_tally(fx["xy"], fx["lab"], fx["r"], fx["K"], grid_mode=1, bin_path=2)
            for _ in range(2):
                c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            return out, c.get_factors(), c.dims()
    out, after, dims = fit(True)
    _, plain, dims0 = fit(False)
    assert np.array_equal(out, fx["want"]) and dims == dims0
    assert all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(after, plain)), "the fit's iterate changed"


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_usable(sa):
    from singlet_amd import _lib
    from singlet_amd._lib import f64p, i32p, i64p, ptr
    fx = whole()
    xy, lab, K, r, T = fx["xy"], fx["lab"], fx["K"], fx["r"], fx["T"]
    n = xy.shape[0]
    L = _lib.load()
    c1, c2 = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])

    def refused(c, code, match, fn):
        with pytest.raises(sa.SingletHipError, match=match) as e:
            fn()
        assert e.value.code == code
        assert np.array_equal(c.cooccur(xy, lab, r, K), fx["want"])                              # usable afterwards

    def raw(c, a1, a2, nn, lb, k, rr, tt):
        out = np.full((64, 8, 8), -7, dtype=np.int64)
        rc = L.sgl_cooccur(c._h, ptr(a1, f64p), ptr(a2, f64p), nn, ptr(lb, i32p), k, ptr(rr, f64p), tt, ptr(out, i64p))
        assert (out == -7).all()                                                                 # outputs stay untouched
        return rc, L.sgl_last_error().decode()

    with sa.Context(0) as c:
        for args in ((None, c2, n, lab, K, r, T), (c1, None, n, lab, K, r, T), (c1, c2, n, None, K, r, T), (c1, c2, n, lab, K, None, T)):
            rc, msg = raw(c, *args)
            assert rc == EINVAL and "NULL" in msg
        for nn in (0, -3):
            rc, msg = raw(c, c1, c2, nn, lab, K, r, T)
            assert rc == EINVAL and "n = %d" % nn in msg
        # the order: a bad coordinate is named before a bad K, a bad K before a bad label, a bad label before a bad T ...
        bad = xy.copy()
        bad[77, 1] = np.nan
        refused(c, EINVAL, r"c2\[77\] = nan is not finite", lambda: c.cooccur(bad, lab, r, 0))
        bad[5, 0] = -np.inf
        refused(c, EINVAL, r"c1\[5\] = -inf is not finite", lambda: c.cooccur(bad, lab, r, K))
        refused(c, EINVAL, r"K = 0 is outside \[1, 256\]", lambda: c.cooccur(xy, lab - 9, r, 0))
        refused(c, EINVAL, r"K = 257", lambda: c.op_cooccur_tally(xy, lab, r, 257))
        lb = lab.copy()
        lb[123] = K
        refused(c, EINVAL, r"lab\[123\] = %d is outside \[0, %d\)" % (K, K), lambda: c.cooccur(xy, lb, np.zeros(1), K))
        lb[123] = -2
        refused(c, EINVAL, r"lab\[123\] = -2", lambda: c.op_cooccur_tally(xy, lb, r, K))
        refused(c, EINVAL, r"T = 0 intervals", lambda: c.cooccur(xy, lab, np.array([-1.0]), K))
        refused(c, EINVAL, r"T = 65 intervals", lambda: c.cooccur(xy, lab, np.linspace(0, 1, 66), K))
        refused(c, EINVAL, r"r\[0\] = -0.5 is negative", lambda: c.cooccur(xy, lab, np.array([-0.5, 0.2, 0.1]), K))
        refused(c, EINVAL, r"r\[2\] = inf", lambda: c.cooccur(xy, lab, np.array([0.0, 0.2, np.inf]), K))
        refused(c, EINVAL, r"r\[1\] = nan", lambda: c.cooccur(xy, lab, np.array([0.0, np.nan, 0.3]), K))
        refused(c, EINVAL, r"square of r\[2\] = 0.2 is .* not above the square of r\[1\]", lambda: c.cooccur(xy, lab, np.array([0.0, 0.2, 0.2]), K))
        refused(c, EINVAL, r"square of r\[1\] = 1e\+200", lambda: c.cooccur(xy, lab, np.array([0.0, 1e200]), K))
        refused(c, EINVAL, r"square of r\[1\] = 2e-200", lambda: c.op_cooccur_tally(xy, lab, np.array([1e-200, 2e-200]), K, grid_mode=-1))
        refused(c, EINVAL, r"grid_mode = -1 is none of", lambda: c.op_cooccur_tally(xy, lab, r, K, grid_mode=-1, bin_path=7))
        refused(c, EINVAL, r"grid_mode = 3", lambda: c.op_cooccur_tally(xy, lab, r, K, grid_mode=3))
        refused(c, EINVAL, r"bin_path = -1", lambda: c.op_cooccur_tally(xy, lab, r, K, bin_path=-1, flush_pairs=-1))
        refused(c, EINVAL, r"bin_path = 3", lambda: c.op_cooccur_tally(xy, lab, r, K, bin_path=3))
        refused(c, EINVAL, r"flush_pairs = -1 is negative", lambda: c.op_cooccur_tally(xy, lab, r, K, flush_pairs=-1))
        refused(c, EINVAL, r"flush_pairs = 4294967296", lambda: c.op_cooccur_tally(xy, lab, r, K, flush_pairs=1 << 32))
        rc = L.sgl_cooccur(c._h, ptr(c1, f64p), ptr(c2, f64p), n, ptr(lab, i32p), K, ptr(r, f64p), T, None)
        assert rc == EINVAL and "NULL counts" in L.sgl_last_error().decode()
        with pytest.raises(ValueError, match="integer class"):
            c.cooccur(xy, lab[:-1], r, K)
        with pytest.raises(ValueError, match="n x 2"):
            c.cooccur(xy.T, lab, r, K)
        with pytest.raises(ValueError, match="one-dimensional"):
            c.cooccur(xy, lab, 5, K)
        # the states of sgl_nhood_enrichment
        c.set_allreduce(lambda dev_ptr, count: None)
        for call in (lambda: c.cooccur(xy, lab, r, K), lambda: c.op_cooccur_tally(xy, lab, r, K)):
            with pytest.raises(sa.SingletHipError, match="all-reduce hook") as e:
                call()
            assert e.value.code == ESTATE
        c.set_allreduce(None)
        A = sa.dgCMatrix(np.ones(3), np.array([0, 1, 2], dtype=np.int32), np.array([0, 1, 2, 3], dtype=np.int32), (5, 3))
        c.upload(A, None, cell_offset=3, ncells_total=9)
        with pytest.raises(sa.SingletHipError, match="shard") as e:
            c.cooccur(xy, lab, r, K)
        assert e.value.code == ESTATE
        c.upload(A, None)                                                                        # a whole matrix resident: no obstacle
        assert np.array_equal(c.cooccur(xy, lab, r, K), fx["want"]) and c.dims()[:2] == (5, 3)
    # the one-shot form refuses before it makes a context
    with pytest.raises(sa.SingletHipError, match=r"lab\[123\] = -2") as e:
        sa.c_cooccur(xy, lb, r, K)
    assert e.value.code == EINVAL


def test_a_team_member_is_refused(sa):
    fx = whole()
    A = sa.dgCMatrix.from_dense(np.random.default_rng(0).poisson(0.5, (30, 200)).astype(np.float64))
    with sa.Multi([0, 0]) as team:
        team.upload(A)
        rank = team.rank_ctx(0)
        for call in (lambda: rank.cooccur(fx["xy"], fx["lab"], fx["r"], fx["K"]), lambda: rank.op_cooccur_tally(fx["xy"], fx["lab"], fx["r"], fx["K"])):
            with pytest.raises(sa.SingletHipError, match="team") as e:
                call()
            assert e.value.code == ESTATE


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("seed", [0, 1, 7])
def test_planted_fixture_through_co_occurrence(sa, seed):
    """Classes 0 and 1 share clumps, class 2 is uniform: the device equals the restatement bit for bit, and the claims hold with
    the bar chosen on the CPU (test_cooccur_restatement.py: occ[0, 1, 0] = 1.7930, 1.7625, 1.6682 against occ[0, 2, 0] = 0.5316,
    0.4654, 0.5829 for the seeds 0, 1, 7; the bar is 1.4)."""
    from test_cooccur_restatement import PLANTED_BAR, planted_reference
    xy, lab, r, N, occ = planted_reference(seed)
    out = sa.co_occurrence(lab, xy, interval=10)
    assert sorted(out) == ["counts", "interval", "occ"]
    assert out["interval"].tobytes() == r.tobytes() and np.array_equal(out["counts"], N)
    assert out["occ"].shape == (3, 3, 10) and out["occ"].tobytes() == occ.tobytes()
    assert out["occ"][0, 1, 0] > out["occ"][0, 2, 0] and out["occ"][0, 1, 0] > PLANTED_BAR
    if seed == 0:
        cum = sa.co_occurrence(lab, (xy[:, 0], xy[:, 1]), interval=r, cumulative=True, n_classes=4)
        four = np.zeros((4, 4, 10), dtype=np.int64)
        four[:3, :3] = N
        assert np.array_equal(cum["counts"], four) and np.array_equal(cum["occ"], co.stats(four, True), equal_nan=True)
        assert np.isnan(cum["occ"][3]).all()


@pytest.mark.parametrize("seed", [0, 1, 7])
def test_ripley_on_a_poisson_pattern(sa, seed):
    """L(r) of a uniform pattern stays within the margin of r for r <= 0.1 of the unit box; the margin was set on the CPU
    (test_cooccur_restatement.py: max |L - r| = 0.00395, 0.00385, 0.00421 for the seeds 0, 1, 7; the margin is 0.008)."""
    from test_cooccur_restatement import POISSON_MARGIN, POISSON_R, poisson_reference
    xy, lab, N, (Kf, L) = poisson_reference(seed)
    got = sa.ripley(lab, xy, mode="L", interval=POISSON_R, area=1.0)
    assert got.shape == (2, 10) and got.tobytes() == L.tobytes()
    assert np.abs(got - POISSON_R[1:][None, :]).max() <= POISSON_MARGIN
    if seed == 0:
        assert sa.ripley(lab, xy, mode="K", interval=POISSON_R, area=1.0).tobytes() == Kf.tobytes()
        box = float((xy[:, 0].max() - xy[:, 0].min()) * (xy[:, 1].max() - xy[:, 1].min()))
        assert sa.ripley(lab, xy, mode="K", interval=POISSON_R).tobytes() == co.ripley(N, np.bincount(lab, minlength=2), box)[0].tobytes()


# ------------------------------------------------------------------------------------------------- the caller's stream
def test_cooccur_on_a_stalled_caller_stream(sa):
    """sgl_set_stream's contract for sgl_cooccur and sgl_op_cooccur_tally (both grid modes, both bin paths): all work goes to the
    caller's stream and the host reads wait for it, so a stall at the head of that stream changes no value."""
    fx = whole()
    xy, lab, r, K = fx["xy"], fx["lab"], fx["r"], fx["K"]
    calls = [("whole", lambda c: c.cooccur(xy, lab, r, K)),
             ("one bucket, LDS", lambda c: c.op_cooccur_tally(xy, lab, r, K, grid_mode=1, bin_path=1)),
             ("grid, global", lambda c: c.op_cooccur_tally(xy, lab, r, K, grid_mode=2, bin_path=2)),
             ("grid, flushing", lambda c: c.op_cooccur_tally(xy, lab, r, K, grid_mode=2, flush_pairs=1))]
    with contexts(sa) as c:
        want = {name: call(c) for name, call in calls}
    assert all(np.array_equal(want[name], fx["want"]) for name, _ in calls)
    with contexts(sa) as c, caller_stream(c) as S:
        sc = Stalled(c, S)
        got = {name: call(sc) for name, call in calls}
    for name, _ in calls:
        assert_same_bits(got[name], want[name], name)
