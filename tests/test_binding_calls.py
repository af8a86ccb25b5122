"""The Python binding's calls into the library, checked against _lib.SIGNATURES without the library or a device.

_lib.load is replaced by a recording stand-in: every attribute is a function that appends (name, args) to a list and
returns 0.  With a 7 x 5 sparse matrix, k = 3 and maxit = 4 the one-shot wrappers, Context and Multi are driven, and of
every recorded call the argument count, the ctypes type of every argument, the scalar positions (nrow, ncol, k, the maxit
cast, the penalties, seed, inv_density) and the buffers of matrices listed twice are checked; of every wrapper the keys,
their order, the shapes and the empty traces (the stand-in reports zero iterations)."""
import ctypes as C

import numpy as np
import pytest

M, N, K, MAXIT = 7, 5, 3, 4
TOL, L1W, L1H, L2W, L2H, THREADS = 1e-3, 0.01, 0.02, 0.03, 0.04, 2
SEED, INV_DENSITY, OVERFIT, TRACE = 11, 20, 1e-3, 2

CSC, CSCT = "Ax Ai Ap", "Tx Ti Tp"
NMF_TAIL = "w_out d_out h_out n_iter trace cb"
ARD_TAIL = "seed inv_density overfit trace_test_mse w_out d_out h_out tm itv ft so nt cb"
LISTS = "a_n a_x a_i a_p a_nc t_n t_x t_i t_p t_nc"
# the parameters of the calls below, in ABI order (include/singlet_hip.h)
LAYOUT = {name: text.split() for name, text in {
    "sgl_c_nmf": f"{CSC} {CSCT} nrow ncol tol maxit verbose L1_w L1_h L2_w L2_h threads w k {NMF_TAIL}",
    "sgl_c_nmf_dense": f"A nrow ncol tol maxit verbose L1_w L1_h L2_w L2_h threads w k {NMF_TAIL}",
    "sgl_c_nmf_sparse_list": f"{LISTS} nrow tol maxit verbose L1 L2 threads w k {NMF_TAIL}",
    "sgl_c_linked_nmf": f"{CSC} {CSCT} nrow ncol tol maxit verbose L1 L2 threads w k lh lh_rows lh_cols lw lw_rows lw_cols {NMF_TAIL}",
    "sgl_c_gcnmf": f"{CSC} {CSCT} nrow ncol Gx Gi Gp g_nrow g_ncol tol maxit verbose L1 L2 threads w w_rows w_cols k {NMF_TAIL}",
    "sgl_c_ard_nmf": f"{CSC} {CSCT} nrow ncol tol maxit verbose L1 L2 threads w k {ARD_TAIL}",
    "sgl_c_ard_nmf_dense": f"A nrow ncol tol maxit verbose L1 L2 threads w k {ARD_TAIL}",
    "sgl_c_ard_nmf_sparse_list": f"{LISTS} nrow tol maxit verbose L1 L2 threads w k {ARD_TAIL}",
    "sgl_c_project_model": f"{CSC} nrow ncol w w_rows w_cols L1 L2 threads h_out d_out",
    "sgl_rcpp_predict": f"{CSC} nrow ncol w w_rows w_cols L1 L2 threads h_out",
    "sgl_c_group_means": "F k n group n_groups means counts",
    "sgl_upload_csc": f"h {CSC} {CSCT} nrow ncol cell_offset ncells_total",
    "sgl_upload_csc_list": f"h {LISTS} nrow cell_offset ncells_total",
    "sgl_multi_upload_csc": f"h {CSC} nrow ncol",
    "sgl_fit_init": "h k w synth_seed",
    "sgl_multi_fit_init": "h k w synth_seed",
    "sgl_nmf_run": "h tol maxit L1_w L1_h L2_w L2_h n_iter trace cb",
    "sgl_multi_nmf_run": "h tol maxit L1_w L1_h L2_w L2_h n_iter trace cb",
    "sgl_ard_run": "h tol maxit L1 L2 seed inv_density overfit trace_test_mse tm itv ft so nt nit cb",
    "sgl_multi_ard_run": "h tol maxit L1 L2 seed inv_density overfit trace_test_mse tm itv ft so nt nit cb",
    "sgl_set_links": "h lh lh_rows lh_cols lw lw_rows lw_cols",
    "sgl_multi_set_links": "h lh lh_rows lh_cols lw lw_rows lw_cols",
    "sgl_set_links_grouped": "h th th_rows th_groups gh tw tw_rows tw_groups gw",
    "sgl_multi_set_links_grouped": "h th th_rows th_groups gh tw tw_rows tw_groups gw",
    "sgl_set_graph": "h Gx Gi Gp g_nrow g_ncol",
    "sgl_multi_set_graph": "h Gx Gi Gp g_nrow g_ncol",
    "sgl_group_means": "h F k n group n_groups means counts",
    "sgl_multi_group_means": "h group n_groups means counts",
    "sgl_evaluate": "h sse mse cell_loss gene_loss",
    "sgl_multi_evaluate": "h sse mse cell_loss gene_loss",
}.items()}

NMF_KEYS = ["w", "d", "h", "iter", "tol"]
ARD_KEYS = ["w", "d", "h", "test_mse", "iter", "tol", "score_overfit"]


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn

    def take(self, name):
        """The arguments of the one call of `name` recorded since the last take, by parameter name."""
        hits = [a for n, a in self.calls if n == name]
        assert len(hits) == 1, (name, [n for n, _ in self.calls])
        self.check_all()
        self.calls.clear()
        assert len(hits[0]) == len(LAYOUT[name]), name
        return dict(zip(LAYOUT[name], hits[0]))

    def check_all(self):
        from singlet_amd import _lib
        for name, args in self.calls:
            argtypes = _lib.SIGNATURES[name][1]
            assert len(args) == len(argtypes), "%s: %d arguments, the signature has %d" % (name, len(args), len(argtypes))
            for q, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except Exception as e:   # noqa: BLE001
                    pytest.fail("%s: argument %d (%r) is not a %s: %s" % (name, q, a, t.__name__, e))


def addr(p):
    return C.cast(p, C.c_void_p).value


def holds(got, **want):
    """Scalars compare by value and Python type (int stays int: the maxit cast), pointers by address; None is NULL."""
    for name, v in want.items():
        g = got[name]
        if isinstance(v, np.ndarray):
            assert addr(g) == v.ctypes.data, name
        elif v is None:
            assert g is None, name
        else:
            assert g == v and isinstance(g, type(v)), (name, g, v)


def csc(A, prefix="A"):
    return {prefix + "x": A.x, prefix + "i": A.i, prefix + "p": A.p}


def chunk_addrs(got, side, chunks):
    n = got[side + "_n"]
    assert n == len(chunks)
    for slot in "xip":
        assert [addr(got["%s_%s" % (side, slot)][q]) for q in range(n)] == [getattr(c, slot).ctypes.data for c in chunks], slot
    nc = C.cast(got[side + "_nc"], C.POINTER(C.c_int32 * n)).contents
    assert list(nc) == [c.ncol for c in chunks]


@pytest.fixture
def env(monkeypatch):
    """(package, recorder, data): _lib.load gives the recorder; Context.dims, which the stand-in would leave at zero,
    gives the test matrix's."""
    import singlet_amd as sa
    from singlet_amd import _lib
    rec = Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    rng = np.random.default_rng(5)
    D = rng.random((M, N)) * (rng.random((M, N)) < 0.6)
    D[0, :] = 1.0
    A = sa.dgCMatrix.from_dense(D)
    monkeypatch.setattr(sa.Context, "dims", lambda self: (M, N, A.nnz))
    data = dict(D=D, A=A, At=sa.dgCMatrix.from_dense(D.T), G=sa.dgCMatrix.from_dense(np.eye(N) + np.eye(N, k=1)),
                chunks=[A.col_slice(0, 2), A.col_slice(2, N)], w=rng.random((K, M)))
    yield sa, rec, data
    rec.check_all()   # whatever a test left unread


def check_fit(out, keys, w_shape=(K, M), n=N):
    assert list(out) == keys
    assert out["w"].shape == w_shape and out["d"].shape == (K,) and out["h"].shape == (K, n)
    if keys is NMF_KEYS:
        assert out["iter"] == 0 and isinstance(out["iter"], int) and out["tol"].shape == (0,)
    else:
        assert all(out[t].shape == (0,) for t in ("test_mse", "iter", "tol", "score_overfit"))
        assert out["iter"].dtype == np.int32


def test_sparse_one_shot_wrappers(env):
    sa, rec, d = env
    A, At, w = d["A"], d["At"], d["w"]
    fit = dict(nrow=M, ncol=N, tol=TOL, maxit=MAXIT, verbose=0, threads=THREADS, k=K)

    check_fit(sa.c_nmf(A, At, TOL, float(MAXIT), False, L1W, L1H, L2W, L2H, THREADS, w), NMF_KEYS)
    got = rec.take("sgl_c_nmf")
    holds(got, **fit, **csc(A), **csc(At, "T"), L1_w=L1W, L1_h=L1H, L2_w=L2W, L2_h=L2H)
    sa.c_nmf(A, None, TOL, MAXIT, True, L1W, L1H, L2W, L2H, THREADS, w)
    holds(rec.take("sgl_c_nmf"), Tx=None, Ti=None, Tp=None, verbose=1)
    sa.c_nmf(A, A, TOL, 0, False, L1W, L1H, L2W, L2H, THREADS, w)   # the same matrix twice: the same buffers twice
    holds(rec.take("sgl_c_nmf"), **csc(A), **csc(A, "T"), maxit=0)

    check_fit(sa.c_ard_nmf(A, At, TOL, float(MAXIT), False, L1W, L2W, THREADS, w, SEED, INV_DENSITY, OVERFIT, TRACE), ARD_KEYS)
    holds(rec.take("sgl_c_ard_nmf"), **fit, **csc(A), **csc(At, "T"), L1=L1W, L2=L2W, seed=SEED, inv_density=INV_DENSITY,
          overfit=OVERFIT, trace_test_mse=TRACE)

    link_h, link_w = np.ones((K, N)), np.ones((1, 1))
    check_fit(sa.c_linked_nmf(A, None, TOL, float(MAXIT), False, L1W, L2W, THREADS, w, link_h, link_w), NMF_KEYS)
    got = rec.take("sgl_c_linked_nmf")
    holds(got, **fit, **csc(A), Tx=None, L1=L1W, L2=L2W, lh_rows=K, lh_cols=N, lw_rows=1, lw_cols=1)
    assert got["lh"] is not None and got["lw"] is not None
    sa.c_linked_nmf(A, None, TOL, MAXIT, False, L1W, L2W, THREADS, w, None, link_w)
    holds(rec.take("sgl_c_linked_nmf"), lh=None, lh_rows=0, lh_cols=0, lw_rows=1)
    with pytest.raises(ValueError, match="link matrices must be 2-D"):
        sa.c_linked_nmf(A, None, TOL, MAXIT, False, L1W, L2W, THREADS, w, np.ones(3), None)

    G = d["G"]
    for w_in in (w, np.ascontiguousarray(w.T)):   # k x m and m x k: both are k = 3, and w comes back m x k
        check_fit(sa.c_gcnmf(A, At, G, TOL, float(MAXIT), False, L1W, L2W, THREADS, w_in), NMF_KEYS, w_shape=(M, K))
        holds(rec.take("sgl_c_gcnmf"), **fit, **csc(A), **csc(At, "T"), **csc(G, "G"), g_nrow=N, g_ncol=N, L1=L1W, L2=L2W,
              w_rows=w_in.shape[0], w_cols=w_in.shape[1])

    with pytest.raises(ValueError, match="w must be a k x nrow"):
        sa.c_nmf(A, None, TOL, MAXIT, True, L1W, L1H, L2W, L2H, THREADS, w.T)
    assert rec.calls == []


def test_validation_comes_before_the_log_header(env, capsys):
    sa, rec, d = env
    with pytest.raises(ValueError):
        sa.c_nmf(d["A"], None, TOL, MAXIT, True, L1W, L1H, L2W, L2H, THREADS, d["w"].T)
    with pytest.raises(ValueError):
        sa.c_ard_nmf_dense(d["D"], None, TOL, MAXIT, True, L1W, L2W, THREADS, d["w"].T, SEED, INV_DENSITY, OVERFIT, TRACE)
    with pytest.raises(ValueError):
        sa.c_nmf_sparse_list(d["chunks"], None, TOL, MAXIT, True, L1W, L2W, THREADS, d["w"].T)
    assert capsys.readouterr().out == "" and rec.calls == []
    sa.c_nmf(d["A"], None, TOL, MAXIT, True, L1W, L1H, L2W, L2H, THREADS, d["w"])
    assert capsys.readouterr().out == "\n%4s | %8s \n---------------\n" % ("iter", "tol")
    sa.c_ard_nmf(d["A"], None, TOL, MAXIT, True, L1W, L2W, THREADS, d["w"], SEED, INV_DENSITY, OVERFIT, TRACE)
    assert capsys.readouterr().out == "\n%4s | %8s | %8s \n---------------------------\n" % ("iter", "tol", "overfit")


def test_dense_and_list_one_shot_wrappers(env):
    sa, rec, d = env
    D, chunks, w = d["D"], d["chunks"], d["w"]
    fit = dict(nrow=M, tol=TOL, maxit=MAXIT, verbose=0, threads=THREADS, k=K)

    check_fit(sa.c_nmf_dense(D, None, TOL, float(MAXIT), False, L1W, L1H, L2W, L2H, THREADS, w), NMF_KEYS)
    holds(rec.take("sgl_c_nmf_dense"), **fit, ncol=N, L1_w=L1W, L1_h=L1H, L2_w=L2W, L2_h=L2H)
    check_fit(sa.c_ard_nmf_dense(D, None, TOL, float(MAXIT), False, L1W, L2W, THREADS, w, SEED, INV_DENSITY, OVERFIT, TRACE), ARD_KEYS)
    holds(rec.take("sgl_c_ard_nmf_dense"), **fit, ncol=N, L1=L1W, L2=L2W, seed=SEED, inv_density=INV_DENSITY, overfit=OVERFIT,
          trace_test_mse=TRACE)
    with pytest.raises(ValueError, match="A must be a matrix"):
        sa.c_nmf_dense(np.ones(4), None, TOL, MAXIT, False, L1W, L1H, L2W, L2H, THREADS, w)

    check_fit(sa.c_nmf_sparse_list(chunks, None, TOL, float(MAXIT), False, L1W, L2W, THREADS, w), NMF_KEYS)
    got = rec.take("sgl_c_nmf_sparse_list")
    holds(got, **fit, L1=L1W, L2=L2W, t_n=0, t_x=None, t_i=None, t_p=None, t_nc=None)
    chunk_addrs(got, "a", chunks)
    t_chunks = [d["At"]]
    check_fit(sa.c_ard_nmf_sparse_list(chunks, t_chunks, TOL, float(MAXIT), False, L1W, L2W, THREADS, w, SEED, INV_DENSITY,
                                       OVERFIT, TRACE), ARD_KEYS)
    got = rec.take("sgl_c_ard_nmf_sparse_list")
    holds(got, **fit, L1=L1W, L2=L2W, seed=SEED, inv_density=INV_DENSITY, overfit=OVERFIT, trace_test_mse=TRACE)
    chunk_addrs(got, "a", chunks)
    chunk_addrs(got, "t", t_chunks)
    twice = [chunks[0], chunks[0]]   # one chunk listed twice: the same buffers twice, h over the sum of the columns
    check_fit(sa.c_nmf_sparse_list(twice, [], TOL, MAXIT, False, L1W, L2W, THREADS, w), NMF_KEYS, n=4)
    chunk_addrs(rec.take("sgl_c_nmf_sparse_list"), "a", twice)
    with pytest.raises(ValueError, match="A_ must hold at least one matrix"):
        sa.c_nmf_sparse_list([], None, TOL, MAXIT, False, L1W, L2W, THREADS, w)
    with pytest.raises(ValueError, match="all chunks of A_ must have the same number of rows"):
        sa.c_nmf_sparse_list([chunks[0], d["At"]], None, TOL, MAXIT, False, L1W, L2W, THREADS, w)


def test_project_and_predict(env):
    sa, rec, d = env
    A, w = d["A"], d["w"]
    for w_in in (w, np.ascontiguousarray(w.T)):
        out = sa.c_project_model(A, w_in, L1W, L2W, THREADS)
        assert list(out) == ["h", "d"] and out["h"].shape == (K, N) and out["d"].shape == (K,)
        holds(rec.take("sgl_c_project_model"), **csc(A), nrow=M, ncol=N, w_rows=w_in.shape[0], w_cols=w_in.shape[1], L1=L1W,
              L2=L2W, threads=THREADS)
        assert sa.Rcpp_predict(A, w_in, L1W, L2W, THREADS).shape == (K, N)
        holds(rec.take("sgl_rcpp_predict"), **csc(A), nrow=M, ncol=N, w_rows=w_in.shape[0], w_cols=w_in.shape[1], L1=L1W,
              L2=L2W, threads=THREADS)
    assert sa.c_project_model(A, np.ones((M, 2)), L1W, L2W, 0)["h"].shape == (2, N)
    assert sa.Rcpp_predict(A, np.ones((M, 2)), L1W, L2W, 0).shape == (2, N)
    assert sa.c_project_model(A, np.ones((2, M)), L1W, L2W, 0)["h"].shape == (2, N)
    rec.check_all()


def drive_handle(sa, rec, d, h, prefix, is_multi):
    """The calls Context and Multi share; `prefix` is the symbol prefix of the handle's library functions."""
    A, G = d["A"], d["G"]
    wb = np.ascontiguousarray(d["w"].T)
    h.fit_init(K, wb)
    holds(rec.take(prefix + "fit_init"), h=h._h, k=K, w=wb)
    assert h.k == K

    n_iter, tr = h.nmf_run(TOL, float(MAXIT), L1W, L1H, L2W, L2H)
    assert n_iter == 0 and isinstance(n_iter, int) and tr.shape == (0,)
    holds(rec.take(prefix + "nmf_run"), h=h._h, tol=TOL, maxit=MAXIT, L1_w=L1W, L1_h=L1H, L2_w=L2W, L2_h=L2H)

    r = h.ard_run(TOL, float(MAXIT), L1W, L2W, SEED, INV_DENSITY, OVERFIT, TRACE)
    assert list(r) == ["test_mse", "iter", "tol", "score_overfit", "n_iter"] and r["n_iter"] == 0
    assert all(r[t].shape == (0,) for t in ("test_mse", "iter", "tol", "score_overfit")) and r["iter"].dtype == np.int32
    holds(rec.take(prefix + "ard_run"), h=h._h, tol=TOL, maxit=MAXIT, L1=L1W, L2=L2W, seed=SEED, inv_density=INV_DENSITY,
          overfit=OVERFIT, trace_test_mse=TRACE)

    h.set_links(np.ones((K, N)), None)
    got = rec.take(prefix + "set_links")
    holds(got, h=h._h, lh_rows=K, lh_cols=N, lw=None, lw_rows=0, lw_cols=0)
    assert got["lh"] is not None
    with pytest.raises(ValueError, match="link matrices must be 2-D"):
        h.set_links(np.ones(3))

    gh, gw = np.arange(N) % 2, np.arange(M) % 3
    h.set_links_grouped(np.ones((K, 2)), gh, np.ones((K, 3)), gw)
    got = rec.take(prefix + "set_links_grouped")
    holds(got, h=h._h, th_rows=K, th_groups=2, tw_rows=K, tw_groups=3)
    assert list(C.cast(got["gh"], C.POINTER(C.c_int32 * N)).contents) == list(gh)
    assert list(C.cast(got["gw"], C.POINTER(C.c_int32 * M)).contents) == list(gw)
    h.set_links_grouped(np.ones((K, 2)), gh)
    holds(rec.take(prefix + "set_links_grouped"), tw=None, tw_rows=0, tw_groups=0, gw=None)
    with pytest.raises(ValueError, match="group_h must hold one group id per column"):
        h.set_links_grouped(np.ones((K, 2)), gh[:-1])
    with pytest.raises(ValueError, match="table_h needs group_h"):
        h.set_links_grouped(np.ones((K, 2)), None)

    h.set_graph(G)
    holds(rec.take(prefix + "set_graph"), h=h._h, **csc(G, "G"), g_nrow=N, g_ncol=N)
    h.set_graph(None)
    holds(rec.take(prefix + "set_graph"), Gx=None, Gi=None, Gp=None, g_nrow=0, g_ncol=0)

    means, counts = h.group_means(gh, 2)
    assert means.shape == (K, 2) and counts.shape == (2,) and counts.dtype == np.int64
    got = rec.take(prefix + "group_means")
    holds(got, h=h._h, n_groups=2)
    if not is_multi:
        holds(got, F=None, k=K, n=N)
    assert list(C.cast(got["group"], C.POINTER(C.c_int32 * N)).contents) == list(gh)

    out = h.evaluate(cell_loss=True, gene_loss=True)
    assert list(out) == ["sse", "mse", "cell_loss", "gene_loss"] and out["cell_loss"].shape == (N,) and out["gene_loss"].shape == (M,)
    got = rec.take(prefix + "evaluate")
    assert got["cell_loss"] is not None and got["gene_loss"] is not None
    assert list(h.evaluate()) == ["sse", "mse"]
    holds(rec.take(prefix + "evaluate"), h=h._h, cell_loss=None, gene_loss=None)


def test_context_calls(env):
    sa, rec, d = env
    A, At, chunks = d["A"], d["At"], d["chunks"]
    with sa.Context(0) as c:
        assert [n for n, _ in rec.calls] == ["sgl_create"]
        rec.check_all()
        rec.calls.clear()
        c.upload(A, At, 3, 9)
        holds(rec.take("sgl_upload_csc"), h=c._h, **csc(A), **csc(At, "T"), nrow=M, ncol=N, cell_offset=3, ncells_total=9)
        c.upload(A)
        holds(rec.take("sgl_upload_csc"), **csc(A), Tx=None, Ti=None, Tp=None, cell_offset=0, ncells_total=0)
        with pytest.raises(ValueError, match="At must be the transpose of A"):
            c.upload(A, A)
        twice = [chunks[1], chunks[1]]
        c.upload_list(twice, None, 1, 8)
        got = rec.take("sgl_upload_csc_list")
        holds(got, h=c._h, nrow=M, cell_offset=1, ncells_total=8, t_n=0, t_x=None, t_nc=None)
        chunk_addrs(got, "a", twice)
        c.upload_list(chunks, [At])
        got = rec.take("sgl_upload_csc_list")
        chunk_addrs(got, "a", chunks)
        chunk_addrs(got, "t", [At])
        with pytest.raises(ValueError, match="the chunk list must hold at least one matrix"):
            c.upload_list([])
        with pytest.raises(ValueError, match="all chunks must have the same number of rows"):
            c.upload_list([chunks[0], At])
        drive_handle(sa, rec, d, c, "sgl_", False)
        F = np.arange(2.0 * N).reshape(2, N)
        means, counts = c.group_means(np.arange(N) % 2, 2, F=F)
        assert means.shape == (2, 2)
        got = rec.take("sgl_group_means")
        holds(got, k=2, n=N, n_groups=2)
        assert list(C.cast(got["F"], C.POINTER(C.c_double * (2 * N))).contents) == list(F.T.ravel())
        with pytest.raises(ValueError, match="F must be a k x n matrix"):
            c.group_means(np.arange(N) % 2, 2, F=np.ones(N))
    means, counts = sa.group_means(F, np.arange(N) % 2, 2)
    assert means.shape == (2, 2) and counts.shape == (2,) and counts.dtype == np.int64
    holds(rec.take("sgl_c_group_means"), k=2, n=N, n_groups=2)


def test_multi_calls(env):
    sa, rec, d = env
    with sa.Multi([0, 0]) as m:
        assert [n for n, _ in rec.calls] == ["sgl_multi_create"]
        rec.check_all()
        rec.calls.clear()
        m.upload(d["A"])
        holds(rec.take("sgl_multi_upload_csc"), h=m._h, **csc(d["A"]), nrow=M, ncol=N)
        drive_handle(sa, rec, d, m, "sgl_multi_", True)
        W, D, H = m.get_factors()
        assert W.shape == (M, K) and D.shape == (K,) and H.shape == (N, K)
        rec.check_all()


def test_resident_fits_return_the_one_shot_lists(env):
    from singlet_amd import api
    sa, rec, d = env
    with sa.Context(0) as c:
        rec.calls.clear()
        with api._ResidentFits(None, ctx=c, Dimnames=("g", "c")) as fits:
            assert fits.nrow == M and fits.Dimnames == ("g", "c")
            check_fit(fits.c_nmf(TOL, float(MAXIT), False, L1W, L1H, L2W, L2H, THREADS, d["w"]), NMF_KEYS)
            assert [n for n, _ in rec.calls] == ["sgl_fit_init", "sgl_nmf_run", "sgl_get_factors"]
            rec.check_all()
            holds(dict(zip(LAYOUT["sgl_nmf_run"], rec.calls[1][1])), tol=TOL, maxit=MAXIT, L1_w=L1W, L1_h=L1H, L2_w=L2W, L2_h=L2H)
            rec.calls.clear()
            check_fit(fits.c_ard_nmf(TOL, float(MAXIT), False, L1W, L2W, THREADS, d["w"], SEED, INV_DENSITY, OVERFIT, TRACE), ARD_KEYS)
            assert [n for n, _ in rec.calls] == ["sgl_fit_init", "sgl_ard_run", "sgl_get_factors"]
            rec.check_all()
            holds(dict(zip(LAYOUT["sgl_ard_run"], rec.calls[1][1])), tol=TOL, maxit=MAXIT, L1=L1W, L2=L2W, seed=SEED,
                  inv_density=INV_DENSITY, overfit=OVERFIT, trace_test_mse=TRACE)
        assert c._h is not None   # an adopted context stays the caller's to close
    rec.calls.clear()
    with api._ResidentFits(d["A"], 1) as fits:
        assert fits.nrow == M and fits.ctx.device == 1
        assert [n for n, _ in rec.calls] == ["sgl_create", "sgl_upload_csc"]
        rec.check_all()
