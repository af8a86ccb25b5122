"""The linked-NMF workflow on the device: group means (sgl_group_means and its one-shot, resident and team forms), the
grouped form of the link matrices (sgl_set_links_grouped) against the dense form and the oracle, and the Python mirror of
R/RunLNMF.R, R/MetadataSummary.R, R/GetSharedFactors.R and R/GetUniqueFactors.R above them."""
import numpy as np
import pytest

from conftest import rel_fro, same_zero_pattern, to_dgc

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CHUNK = 256   # SGL_GROUP_CHUNK: cells per chunk of a group's cell list
TOL = 1e-9    # the tolerance of tests/test_gpu_nmf.py::_check


def _check(got, ref, keys=("w", "h", "d")):
    """tests/test_gpu_nmf.py::_check: relative Frobenius error below 1e-9 and the same zero pattern."""
    for key in keys:
        g = got[key].T if got[key].ndim == 2 else got[key]
        assert rel_fro(g, ref[key]) < TOL, key
        if g.ndim == 2:
            assert same_zero_pattern(g, ref[key]), key


# ----------------------------------------------------------------------------------------------------- group means --
def _labels(rng, n, G):
    """Interleaved, unsorted labels; where the sizes allow it, one group left empty and one of a single cell."""
    g = rng.integers(0, G, n).astype(np.int32)
    if G >= 2 and n >= 2:
        g[g == G - 1] = 0                      # group G - 1: empty
    if G >= 3 and n >= 3:
        g[g == 1] = 0
        g[n // 2] = 1                          # group 1: one cell, in the middle of the list
    return g


def _ld_reference(F, g, G):
    """Long-double group sums of F (k x n) and of |F|, and the counts: one pass over the cells sorted by group."""
    k, n = F.shape
    order = np.argsort(g, kind="stable")
    counts = np.bincount(g, minlength=G).astype(np.int64)
    sums = np.zeros((k, G), dtype=np.longdouble)
    sabs = np.zeros((k, G), dtype=np.longdouble)
    Fs = F[:, order].astype(np.longdouble)
    start = 0
    for q in np.flatnonzero(counts):
        sums[:, q] = Fs[:, start:start + counts[q]].sum(axis=1)
        sabs[:, q] = np.abs(Fs[:, start:start + counts[q]]).sum(axis=1)
        start += counts[q]
    return sums, sabs, counts


def _assert_means_within_bound(means, F, g, G, what=""):
    """|err| <= 2 n_g 2^-53 mean_g |x|: the first-order bound of any summation order of n_g terms, doubled for the division
    and the second-order terms.  Empty groups must be NaN."""
    sums, sabs, counts = _ld_reference(F, g, G)
    full = counts > 0
    assert np.all(np.isnan(means[:, ~full])), what
    cnt = counts[full].astype(np.longdouble)
    ref = sums[:, full] / cnt
    bound = 2 * cnt * np.longdouble(U) * (sabs[:, full] / cnt)
    err = np.abs(means[:, full].astype(np.longdouble) - ref)
    assert np.all(err <= bound), (what, float((err - bound).max()))
    return counts


NS = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 4097, 10007)
GS = (1, 2, 7, 300)


@pytest.mark.parametrize("k", [1, 9, 50, 64, 65, 130])
def test_group_means_exact_and_within_the_bound(sa, ctx, k):
    """Every n (the wave width, the chunk size and their neighbours, several chunks) and every G at one rank k: integer F
    gives the exact means bit for bit, an all-zero (factor, group) gives 0.0, counts are exact, an empty group is NaN with
    count 0; random non-negative and signed F stay within the derived bound; a second call gives the same bits."""
    rng = np.random.default_rng(100 + k)
    for n in NS:
        for G in GS:
            g = _labels(rng, n, G)
            what = "k=%d n=%d G=%d" % (k, n, G)
            # small integers: every partial sum is exact in any order
            Fi = rng.integers(-8, 9, (k, n)).astype(np.float64)
            zero_g = int(g[0])
            Fi[k - 1, g == zero_g] = 0.0
            means, counts = ctx.group_means(g, G, F=Fi)
            cnt = np.bincount(g, minlength=G)
            assert means.shape == (k, G) and np.array_equal(counts, cnt), what
            exact = _ld_reference(Fi, g, G)[0].astype(np.float64)   # integers: exact in any format and order
            with np.errstate(invalid="ignore", divide="ignore"):
                want = exact / cnt.astype(np.float64)[None, :]
            assert np.array_equal(means, want, equal_nan=True), what
            assert np.all(np.isnan(means[:, cnt == 0])) and not np.any(np.isnan(means[:, cnt > 0])), what
            assert means[k - 1, zero_g] == 0.0 and not np.signbit(means[k - 1, zero_g]), what
            if G >= 3 and n >= 3:
                assert cnt[G - 1] == 0 and cnt[1] == 1 and np.array_equal(means[:, 1], Fi[:, n // 2]), what
            # random values against the long-double reference
            for F in (rng.random((k, n)), rng.standard_normal((k, n)) * np.exp(3 * rng.standard_normal((k, 1)))):
                means, counts = ctx.group_means(g, G, F=F)
                assert np.array_equal(_assert_means_within_bound(means, F, g, G, what), counts), what
            again, _ = ctx.group_means(g, G, F=F)
            assert np.array_equal(means, again, equal_nan=True), what


def test_group_means_forms_agree_bit_for_bit(sa, ora):
    """The resident form (F = None: the H of the fit, read in place) equals the host-F form on get_factors()'s H, and the
    one-shot form equals the context form."""
    m, n, k, G = 200, 1000, 12, 5
    A = ora.synth_csc(m, n, 15)
    g = _labels(np.random.default_rng(3), n, G)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A), None)
        c.fit_init(k, ora.synth_winit(k, m))
        c.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        _, _, H = c.get_factors()
        resident, cnt_r = c.group_means(g, G)
        host, cnt_h = c.group_means(g, G, F=H.T)
        _, _, H2 = c.get_factors()
    one_shot, cnt_o = sa.group_means(H.T, g, G)
    assert np.array_equal(H, H2)   # the fit's H is read, not touched
    assert np.array_equal(resident, host, equal_nan=True) and np.array_equal(host, one_shot, equal_nan=True)
    assert np.array_equal(cnt_r, cnt_h) and np.array_equal(cnt_h, cnt_o) and np.array_equal(cnt_o, np.bincount(g, minlength=G))
    _assert_means_within_bound(resident, H.T, g, G)


@pytest.mark.parametrize("ranks", [2, 3])
def test_group_means_on_a_team(sa, ora, ranks):
    """Multi.group_means: every rank sums its own cells, the host adds the partials in rank order: the counts of one
    context, means within the same bound."""
    m, n, k, G = 263, 530, 9, 7
    A = ora.synth_csc(m, n, 15)
    g = _labels(np.random.default_rng(5), n, G)
    with sa.Multi([0] * ranks) as M:
        M.upload(to_dgc(sa, A))
        with pytest.raises(sa.SingletHipError) as e:
            M.group_means(g, G)            # no fit yet
        assert e.value.code == -6
        M.fit_init(k, ora.synth_winit(k, m))
        M.nmf_run(0.0, 3, 0.01, 0.01, 0.0, 0.0)
        _, _, H = M.get_factors()
        means, counts = M.group_means(g, G)
        again, _ = M.group_means(g, G)
        with pytest.raises(sa.SingletHipError) as e:
            M.rank_ctx(0).group_means(g[:M.rank_ctx(0).dims()[1]], G)   # a team member refuses the one-context entry
        assert e.value.code == -6
    one, cnt_one = sa.group_means(H.T, g, G)
    assert np.array_equal(counts, cnt_one)
    assert np.array_equal(means, again, equal_nan=True)
    assert np.array_equal(_assert_means_within_bound(means, H.T, g, G), counts)


def test_group_means_refusals_leave_the_context_usable(sa, ora):
    n, k, G = 300, 7, 4
    rng = np.random.default_rng(9)
    F = rng.random((k, n))
    g = rng.integers(0, G, n).astype(np.int32)
    with sa.Context(0) as c:
        for pos, bad in ((17, -1), (n - 1, G)):
            gb = g.copy()
            gb[pos] = bad
            for call in (lambda: c.group_means(gb, G, F=F), lambda: sa.group_means(F, gb, G)):
                with pytest.raises(sa.SingletHipError) as e:
                    call()
                assert e.value.code == -1 and "group[%d] = %d" % (pos, bad) in str(e.value)
        for call in (lambda: c.group_means(g, 0, F=F), lambda: sa.group_means(F, g, 0)):
            with pytest.raises(sa.SingletHipError) as e:
                call()
            assert e.value.code == -1 and "n_groups" in str(e.value)
        with pytest.raises(sa.SingletHipError) as e:
            c.group_means(g, G)            # F = None without a fit
        assert e.value.code == -6
        c.set_allreduce(lambda p, cnt: None)
        with pytest.raises(sa.SingletHipError) as e:
            c.group_means(g, G, F=F)       # a shard's means are not the matrix's
        assert e.value.code == -6
        c.set_allreduce(None)
        means, counts = c.group_means(g, G, F=F)
        _assert_means_within_bound(means, F, g, G)
        # ... and still fits
        A = ora.synth_csc(120, 150, 15)
        c.upload(to_dgc(sa, A), None)
        c.fit_init(4, ora.synth_winit(4, 120))
        c.nmf_run(0.0, 1, 0.01, 0.01, 0.0, 0.0)
        means, counts = c.group_means(g[:150], G)
        assert means.shape == (4, G) and counts.sum() == 150


# --------------------------------------------------------------------------------------------------- grouped links --
def _tables(rng, rows, G, ncols):
    """A rows x G table with values (rand < 0.7) * (0.5 + rand) -- not only 0 / 1 -- and one group id per column."""
    T = (rng.random((rows, G)) < 0.7) * (0.5 + rng.random((rows, G)))
    grp = rng.integers(0, G, ncols).astype(np.int32)
    return T, grp


def _fit(c, sa, A, k, w0, links, iters=4):
    c.upload(to_dgc(sa, A), None)
    c.fit_init(k, w0)
    links(c)
    c.nmf_run(0.0, iters, 0.01, 0.01, 0.0, 0.0)
    return c.get_factors()


def _same_fit(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# k = 50: rows * G * 8 = 32 400 at G = 81 (the table is staged in LDS), 32 800 at G = 82 and 36 000 at G = 90 (past the 32 KiB budget)
@pytest.mark.parametrize("k,G,rows_h,w_side", [
    (9, 1, 9, False), (9, 3, 9, False), (9, 300, 9, False), (9, 1, 5, False), (9, 3, 5, True), (9, 300, 5, True),
    (9, 3, 9, True), (50, 81, 50, False), (50, 82, 50, True), (50, 90, 50, False), (50, 90, 37, True)])
def test_grouped_links_give_the_bits_of_the_dense_form(sa, ora, k, G, rows_h, w_side):
    m, n = 260, 330
    A = ora.synth_csc(m, n, 15)
    w0 = ora.synth_winit(k, m)
    rng = np.random.default_rng(4)
    Th, gh = _tables(rng, rows_h, G, n)
    Tw, gw = _tables(rng, rows_h if k == 9 else k, G, m) if w_side else (None, None)
    lh = Th[:, gh]
    lw = Tw[:, gw] if w_side else None
    with sa.Context(0) as c:
        grouped = _fit(c, sa, A, k, w0, lambda c: c.set_links_grouped(Th, gh, Tw, gw))
        dense = _fit(c, sa, A, k, w0, lambda c: c.set_links(lh, lw))
    assert _same_fit(grouped, dense)
    W, d, H = grouped
    assert np.all(H[:, :rows_h][lh.T == 0] == 0)   # a zero link pins the coefficient at zero
    if k == 9:
        ref = ora.c_linked_nmf(A, A.t(), 0.0, 4, 0.01, 0.0, 0, w0, lh, lw if w_side else np.ones((1, 1)))
        _check({"w": W.T, "d": d, "h": H.T}, ref)


@pytest.mark.parametrize("ranks", [2, 3])
def test_grouped_links_on_a_team(sa, ora, ranks):
    """group_h follows the cells to the ranks, group_w is read from every rank's first gene on (263 genes: an uneven last
    gene block); against the oracle at the team tolerance, W bit-identical on every rank."""
    m, n, k, G = 263, 530, 9, 3
    A = ora.synth_csc(m, n, 15)
    w0 = ora.synth_winit(k, m)
    rng = np.random.default_rng(4)
    Th, gh = _tables(rng, k, G, n)
    Tw, gw = _tables(rng, 5, 4, m)
    lh, lw = Th[:, gh], Tw[:, gw]
    ref = ora.c_linked_nmf(A, A.t(), 0.0, 4, 0.01, 0.0, 0, w0, lh, lw)
    with sa.Multi([0] * ranks) as M:
        M.upload(to_dgc(sa, A))
        M.fit_init(k, w0)
        gb = gh.copy()
        gb[n - 1] = G
        with pytest.raises(sa.SingletHipError) as e:
            M.set_links_grouped(Th, gb, Tw, gw)
        assert e.value.code == -1 and "group_h[%d] = %d" % (n - 1, G) in str(e.value)
        M.set_links_grouped(Th, gh, Tw, gw)
        M.nmf_run(0.0, 4, 0.01, 0.01, 0.0, 0.0)
        W, d, H = M.get_factors()
        Ws = [M.rank_ctx(r).get_factors(h=False)[0] for r in range(ranks)]
        M.fit_init(k, w0)
        M.set_links(lh, lw)
        M.nmf_run(0.0, 4, 0.01, 0.01, 0.0, 0.0)
        dense = M.get_factors()
    assert rel_fro(W, ref["w"]) < 1e-9 and rel_fro(H, ref["h"]) < 1e-9 and rel_fro(d, ref["d"]) < 1e-9
    assert same_zero_pattern(W, ref["w"]) and same_zero_pattern(H, ref["h"])
    assert all(np.array_equal(Wr, W) for Wr in Ws)
    assert np.all(H[lh.T == 0] == 0)
    assert _same_fit((W, d, H), dense)


def test_grouped_links_lifetime_and_refusals(sa, ora):
    m, n, k, G = 260, 330, 9, 3
    A = ora.synth_csc(m, n, 15)
    w0 = ora.synth_winit(k, m)
    rng = np.random.default_rng(11)
    T1, g1 = _tables(rng, k, G, n)
    T2, g2 = _tables(rng, 5, 7, n)
    Tw, gw = _tables(rng, k, G, m)
    l1, l2 = T1[:, g1], T2[:, g2]

    def bad_ids(c):
        gb = g1.copy()
        gb[n - 1] = -1
        with pytest.raises(sa.SingletHipError) as e:
            c.set_links_grouped(T2, g2, Tw, np.where(np.arange(m) == 3, 3, gw))
        assert e.value.code == -1 and "group_w[3] = 3" in str(e.value)
        with pytest.raises(sa.SingletHipError) as e:
            c.set_links_grouped(T1, gb)
        assert e.value.code == -1 and "group_h[%d] = -1" % (n - 1) in str(e.value)

    def too_many_rows(c):
        with pytest.raises(sa.SingletHipError) as e:
            c.set_links_grouped(np.ones((k + 1, G)), g1)
        assert e.value.code == -1 and "more rows" in str(e.value)

    def with_graph(c):
        c.set_graph(sa.dgCMatrix(np.ones(n), np.arange(n), np.arange(n + 1), (n, n)))
        with pytest.raises(sa.SingletHipError) as e:
            c.set_links_grouped(T1, g1)
        assert e.value.code == -1 and "graph" in str(e.value)
        c.set_graph(None)
        c.set_links_grouped(T1, g1)
        with pytest.raises(sa.SingletHipError) as e:
            c.set_graph(sa.dgCMatrix(np.ones(n), np.arange(n), np.arange(n + 1), (n, n)))
        assert e.value.code == -1 and "link" in str(e.value)

    with sa.Context(0) as c:
        plain = _fit(c, sa, A, k, w0, lambda c: None)
        only1 = _fit(c, sa, A, k, w0, lambda c: c.set_links(l1, None))
        only2 = _fit(c, sa, A, k, w0, lambda c: c.set_links(l2, None))
        assert not _same_fit(plain, only1) and not _same_fit(only1, only2)
        # each call replaces what the other set, on both sides
        assert _same_fit(only2, _fit(c, sa, A, k, w0, lambda c: (c.set_links_grouped(T1, g1, Tw, gw), c.set_links(l2, None))))
        assert _same_fit(only1, _fit(c, sa, A, k, w0, lambda c: (c.set_links(l2, Tw[:, gw]), c.set_links_grouped(T1, g1))))
        assert _same_fit(only2, _fit(c, sa, A, k, w0, lambda c: (c.set_links_grouped(T1, g1, Tw, gw), c.set_links_grouped(T2, g2))))
        # a NULL table switches the side off
        assert _same_fit(plain, _fit(c, sa, A, k, w0, lambda c: (c.set_links_grouped(T1, g1), c.set_links_grouped(None, None))))
        # fit_init drops it
        assert _same_fit(plain, _fit(c, sa, A, k, w0, lambda c: (c.set_links_grouped(T1, g1), c.fit_init(k, w0))))
        # a refused group list leaves the links set before in force; the rows refusal drops them, as sgl_set_links' does
        assert _same_fit(only1, _fit(c, sa, A, k, w0, lambda c: (c.set_links_grouped(T1, g1), bad_ids(c))))
        assert _same_fit(plain, _fit(c, sa, A, k, w0, lambda c: (c.set_links_grouped(T1, g1), too_many_rows(c))))
        assert _same_fit(only1, _fit(c, sa, A, k, w0, with_graph))
        c.upload(to_dgc(sa, A), None)
        with pytest.raises(sa.SingletHipError) as e:
            c.set_links_grouped(T1, g1)     # no fit
        assert e.value.code == -6
        with pytest.raises(ValueError):
            c.set_links_grouped(T1, g1[:-1])
        with pytest.raises(ValueError):
            c.set_links_grouped(T1, None)


# -------------------------------------------------------------------------------------------------------- workflow --
def test_run_linked_nmf_matches_the_oracle_sorted_by_d(sa, ora):
    m, n, k = 260, 330, 9
    A = ora.synth_csc(m, n, 15)
    w0 = ora.synth_winit(k, m)               # (m, k): the m x k `w` of run_linked_nmf
    rng = np.random.default_rng(4)
    lh = (rng.random((k, n)) < 0.7) * (0.5 + rng.random((k, n)))
    ref = ora.c_linked_nmf(A, A.t(), 0.0, 4, 0.01, 0.0, 0, w0, lh, np.zeros((1, 1)))
    idx = np.argsort(-ref["d"], kind="stable")
    got = sa.run_linked_nmf(to_dgc(sa, A), w0, link_h=lh, tol=0.0, maxit=4, verbose=False)
    assert got["w"].shape == (m, k) and got["h"].shape == (k, n)
    assert np.all(np.diff(got["d"]) <= 0)
    assert rel_fro(got["w"], ref["w"][:, idx]) < TOL and rel_fro(got["h"], ref["h"].T[idx]) < TOL and rel_fro(got["d"], ref["d"][idx]) < TOL
    assert same_zero_pattern(got["w"], ref["w"][:, idx]) and same_zero_pattern(got["h"], ref["h"].T[idx])
    # link_w m x k is ignored by c_linked_nmf unless k == m, as in the reference
    with_w = sa.run_linked_nmf(to_dgc(sa, A), w0, link_h=lh, link_w=np.zeros((m, k)), tol=0.0, maxit=4, verbose=False)
    assert np.array_equal(with_w["w"], got["w"]) and np.array_equal(with_w["h"], got["h"])
    dA = to_dgc(sa, A)
    for kwargs, msg in (
            (dict(), "both link_h and link_w cannot be NULL. Specify at least one linking matrix."),
            (dict(link_h=lh[:-1]), "number of rows in 'link_h' must be equal to the nubmer of columns in 'w'"),
            (dict(link_h=lh[:, :-1]), "number of columns in 'link_h' must be equal to the number of columns in 'A'"),
            (dict(link_w=np.ones((m, k + 1))), "number of columns in 'link_w' must be equal to the nubmer of columns in 'w'"),
            (dict(link_w=np.ones((m + 1, k))), "number of rows in 'link_w' must be equal to the number of rows in 'A'"),
            (dict(link_h=lh, L1=1.0), "L1 penalty must be strictly in the range (0, 1]")):
        with pytest.raises(ValueError) as e:
            sa.run_linked_nmf(dA, w0, verbose=False, **kwargs)
        assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        sa.run_linked_nmf(dA, w0[:-1], link_h=lh, verbose=False)
    assert str(e.value) == "number of rows in 'w' must be equal to the number of rows in 'A'"


@pytest.fixture(scope="module")
def planted(sa, ora):
    """The planted recipe: six gene blocks, factor 4 carried by group 0 alone, factor 5 by the others.  The model comes from
    the CPU oracle, so the input of RunLNMF does not depend on the device.  Shared by the tests below; left unchanged."""
    rng = np.random.default_rng(7)
    m, n, k, G = 240, 330, 6, 3
    sb = rng.integers(0, 3, n)
    Wt = np.zeros((m, k))
    for j in range(k):
        Wt[40 * j:40 * j + 40, j] = 0.5 + rng.random(40)
    Ht = rng.random((k, n)) * (rng.random((k, n)) < 0.6)
    Ht[4, sb != 0] = 0
    Ht[5, sb == 0] = 0
    D = np.log1p((Wt @ Ht) * (rng.random((m, n)) < 0.5))
    dA = sa.dgCMatrix.from_dense(D)
    A = ora.CSC(dA.x, dA.i, dA.p, m, n)
    fit = ora.c_nmf(A, A.t(), 0.0, 12, 0.01, 0.01, 0.0, 0.0, 0, ora.synth_winit(k, m))
    model = {"w": fit["w"].copy(), "d": fit["d"].copy(), "h": fit["h"].T.copy()}
    h = model["h"].astype(np.longdouble)
    means = np.stack([h[:, sb == q].sum(axis=1) / np.longdouble((sb == q).sum()) for q in range(G)], axis=1)
    share = means / means.sum(axis=1, keepdims=True) * G
    out = {}
    for cutoff in (0.5, 0.8):
        out[cutoff] = sa.RunLNMF(dA, model, sb, link_cutoff=cutoff, maxit=6, verbose=False)
    return dict(D=D, dA=dA, sb=sb, model=model, share=share, out=out, m=m, n=n, k=k, G=G)


@pytest.mark.parametrize("cutoff,unlinked", [(0.5, 3), (0.8, None)])
def test_RunLNMF_on_the_planted_recipe(sa, planted, cutoff, unlinked):
    P = planted
    share, sb, k, G = P["share"], P["sb"], P["k"], P["G"]
    assert float(np.abs(share - cutoff).min()) > 1e-6          # the precondition: no share near the cut-off
    table_ref = 1.0 - np.asarray(share < cutoff, dtype=np.float64)
    if unlinked is not None:
        assert int((table_ref == 0).sum()) == unlinked
    out = P["out"][cutoff]
    assert np.array_equal(out["link_table"], table_ref)
    assert np.array_equal(out["levels"], np.arange(G)) and out["factor_names"] == ["LNMF_%d" % (q + 1) for q in range(k)]
    assert np.all(np.diff(out["d"]) <= 0) and sorted(out["factor_order"]) == list(range(k))
    # the same fit through run_linked_nmf on the weighted matrix with the expanded dense link
    Aw = sa.weight_by_split(P["dA"], sb.astype(np.int32), G)
    link_h = table_ref[:, sb]
    dense = sa.run_linked_nmf(Aw, P["model"]["w"], link_h=link_h, tol=1e-5, maxit=6, verbose=False, L1=0.01, L2=0)
    for key in ("w", "d", "h"):
        assert np.array_equal(out[key], dense[key]), key
    assert out["iter"] == dense["iter"]
    # h is zero where unlinked (rows of link_table follow the input factors: factor_order maps the output back)
    assert np.all(out["h"][link_h[out["factor_order"]] == 0] == 0)
    # the 5 empty columns come back as the reference leaves them: never solved, h stays at its initial 0
    empty = np.flatnonzero(P["D"].sum(axis=0) == 0)
    assert empty.size == 5 and np.all(out["h"][:, empty] == 0)


def test_RunLNMF_refusals(sa, planted):
    P = planted
    with pytest.raises(ValueError, match="no value specified for 'split.by'"):
        sa.RunLNMF(P["dA"], P["model"], None)
    with pytest.raises(ValueError, match="per ROW of A"):
        sa.RunLNMF(P["dA"], P["model"], np.zeros(P["m"], dtype=int))
    with pytest.raises(ValueError, match="length of 'split.by' was not equal to one of the dimensions"):
        sa.RunLNMF(P["dA"], P["model"], P["sb"][:-1])
    dead = {"w": P["model"]["w"], "h": P["model"]["h"].copy()}
    dead["h"][2] = 0.0
    with pytest.raises(ValueError, match="factor 2 "):
        sa.RunLNMF(P["dA"], dead, P["sb"], verbose=False)


def test_MetadataSummary_and_the_factor_sets(sa, planted):
    P = planted
    out, sb, k, G = P["out"][0.5], P["sb"], P["k"], P["G"]
    h = out["h"]
    S = sa.MetadataSummary(h, sb)
    assert S["table"].shape == (G, k) and np.array_equal(S["levels"], np.arange(G))
    assert S["factors"] == ["factor%d" % (q + 1) for q in range(k)]

    def reference(labels):
        lv = np.unique(labels)
        hl = h.astype(np.longdouble)
        cnt = np.array([(labels == q).sum() for q in lv])
        mean = np.stack([hl[:, labels == q].sum(axis=1) / np.longdouble((labels == q).sum()) for q in lv], axis=1)
        return (mean / mean.sum(axis=1, keepdims=True)).T, cnt

    def bound(ref, cnt):
        # h >= 0: every mean has a relative error of at most e = 2 n_g 2^-53 (the bound above); their sum then e_max + G u,
        # the quotient one more rounding: |error of a share| <= share * (2 e_max + (G + 2) u), second-order terms included
        return ref * (2 * 2 * cnt.max() * U + (len(cnt) + 2) * U) * 1.01

    ref, cnt = reference(sb)
    assert np.all(np.abs(S["table"].astype(np.longdouble) - ref) <= bound(ref, cnt))
    # unique factors: those a group does not carry at all = the rows of link_table with a 0
    uniq = sa.GetUniqueFactors(h, sb)
    shared = sa.GetSharedFactors(h, sb)
    assert sorted(np.concatenate([uniq, shared]).tolist()) == list(range(k))
    assert set(out["factor_order"][uniq].tolist()) == set(np.flatnonzero((out["link_table"] == 0).any(axis=1)).tolist())
    assert len(uniq) > 0 and len(shared) > 0
    # a NaN column (a factor that is zero everywhere) counts as shared
    h0 = h.copy()
    h0[int(shared[0])] = 0.0
    assert int(shared[0]) in sa.GetSharedFactors(h0, sb).tolist() and int(shared[0]) not in sa.GetUniqueFactors(h0, sb).tolist()
    # two levels: rows ordered by their share of the first factor, decreasing (R/MetadataSummary.R:27-28)
    two = np.where(sb == 0, "a", "b")
    for h2 in (h, h[::-1]):
        S2 = sa.MetadataSummary(h2, two)
        assert S2["table"].shape == (2, k) and S2["table"][0, 0] >= S2["table"][1, 0]
        lv = np.unique(two)
        hl = h2.astype(np.longdouble)
        mean = np.stack([hl[:, two == q].sum(axis=1) / np.longdouble((two == q).sum()) for q in lv], axis=1)
        ref2 = (mean / mean.sum(axis=1, keepdims=True)).T
        order = np.argsort(-ref2[:, 0].astype(np.float64), kind="stable")
        assert list(S2["levels"]) == list(lv[order])
        cnt2 = np.array([(two == q).sum() for q in lv])
        assert np.all(np.abs(S2["table"].astype(np.longdouble) - ref2[order]) <= bound(ref2[order], cnt2))
