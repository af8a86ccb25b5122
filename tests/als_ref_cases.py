"""The case list shared by tests/golden/make_als_ref.py (which runs the reference build over it and writes
tests/golden/als_ref.npz), tests/test_reference_build.py (oracle against the reference build, CPU) and
tests/test_gpu_reference_pinned.py (product against the reference build, GPU).

A case is (entry, name, parameters).  run(case, L) runs it on L -- oracle.oracle, or a variant of oracle.reference: the
two carry the same functions with the same signatures -- and returns {output name: array}.  Outputs whose name starts
with "n_" or equals "iter" / "p" / "i" are integer / structural and compared exactly; the others are floating point.

Inputs are made from the oracle's hash generator (synth_csc / synth_winit: not reference code, deterministic C) and
numpy's default_rng by seed; nothing here depends on the reference tree."""
import numpy as np

NMF_RANKS = [1, 2, 10, 16, 17, 30, 32, 33, 40, 42, 50, 64, 65, 96, 100, 104, 105, 128, 129, 200, 256, 257]
NMF_PENALTIES = [(0.0, 0.0), (0.01, 0.0), (0.01, 0.01)]      # those of test_gpu_nmf.py::test_c_nmf_parity
ARD_RANKS = [6, 20, 44, 50, 85, 100, 116, 140]

EXACT = ("iter", "p", "i")
# the outputs whose exact zeros are results (a clamped coordinate, an empty column, a dead factor): their zero pattern is
# structural.  In the others (residuals, traces, sums) an exact zero is a coincidence of rounding; only NaN / Inf count.
PATTERNED = ("x", "w", "h", "s", "g", "res")


def is_exact(key):
    return key in EXACT or key.startswith("n_")


def ragged(ora, m, n, inv_density, seed=None):
    """Generator matrix made ragged: every 11th column (from 3) and every 13th row (from 5) empty, every 4th column
    (from 1) cut to its first two entries."""
    A = ora.synth_csc(m, n, inv_density) if seed is None else ora.synth_csc(m, n, inv_density, seed)
    keep = np.ones(A.nnz, dtype=bool)
    col = np.repeat(np.arange(n), np.diff(A.p))
    rank_in_col = np.arange(A.nnz) - A.p[:-1][col]
    keep &= col % 11 != 3
    keep &= A.i % 13 != 5
    keep &= ~((col % 4 == 1) & (rank_in_col >= 2))
    p = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(col[keep], minlength=n), out=p[1:])
    return ora.CSC(A.x[keep], A.i[keep], p, m, n)


def chunks(ora, A, widths):
    """Column chunks of A with the given widths (the last takes the rest)."""
    out, c0 = [], 0
    widths = list(widths) + [A.ncol - sum(widths)]
    for wd in widths:
        s, e = A.p[c0], A.p[c0 + wd]
        out.append(ora.CSC(A.x[s:e], A.i[s:e], A.p[c0:c0 + wd + 1] - s, A.nrow, wd))
        c0 += wd
    return out


def _nmf_size(k):
    return (230, 280, 3) if k <= 65 else (200, 240, 2) if k <= 129 else (280, 330, 2)


def cases():
    out = []
    # ---- functions
    for k, L1, L2 in [(7, 0.0, 0.0), (50, 0.01, 0.0), (100, 0.01, 0.02)]:
        out.append(("nnls", "k%d" % k, dict(k=k, L1=L1, L2=L2)))
    out.append(("nnls_quirks", "hand", {}))
    for k, cols in [(1, 1), (17, 63), (64, 64), (257, 65), (5, 100000)]:
        out.append(("scale_cor", "k%d_c%d" % (k, cols), dict(k=k, cols=cols)))
    out.append(("scale_cor", "zero_row", dict(k=6, cols=40, zero_row=2)))
    out.append(("aat", "k33", dict(k=33, cols=150)))
    for name, kw in [("cold", dict(k=12, L1=0.0, L2=0.0, warm=False)), ("warm_l1", dict(k=12, L1=0.02, L2=0.0, warm=True)),
                     ("warm_l1_l2_k70", dict(k=70, L1=0.01, L2=0.01, warm=True))]:
        out.append(("predict", name, dict(kw, mask_t=False)))
        out.append(("predict", name + "_t", dict(kw, mask_t=True)))       # the W side: t(A) against h
        out.append(("predict_mask", name, dict(kw, mask_t=False)))
        out.append(("predict_mask", name + "_t", dict(kw, mask_t=True)))
    for case in ("dead", "single"):
        for mask_t in (False, True):
            out.append(("predict_mask_degenerate", "%s_%d" % (case, mask_t), dict(k=44, case=case, mask_t=mask_t)))
    out.append(("predict_dense", "k9", dict(k=9)))
    out.append(("mse_test", "k8", dict(k=8, inv_density=8)))
    out.append(("mse_test", "k8_all", dict(k=8, inv_density=1)))
    # ---- plain drivers
    for q, k in enumerate(NMF_RANKS):
        m, n, maxit = _nmf_size(k)
        L1, L2 = NMF_PENALTIES[q % 3]
        out.append(("c_nmf", "k%d" % k, dict(m=m, n=n, k=k, tol=0.0, maxit=maxit, L1w=L1, L1h=L1, L2w=L2, L2h=L2)))
    # replacements for the ranks whose first input the two summation orders decide differently (kept above as candidates)
    for k, seed in [(129, 0xA11), (257, 0xA12)]:
        out.append(("c_nmf", "k%d_seed%x" % (k, seed), dict(m=280, n=330, k=k, tol=0.0, maxit=2, L1w=0.01, L1h=0.01, L2w=0.0, L2h=0.0, seed=seed)))
    # k = 257 exceeds what these matrices determine: the second iteration amplifies the last bit into a clamp decision under
    # either seed.  One iteration (as tests/test_gpu_high_rank.py runs its ranks) on a larger matrix holds.
    out.append(("c_nmf", "k257_one_iteration", dict(m=400, n=450, k=257, tol=0.0, maxit=1, L1w=0.01, L1h=0.01, L2w=0.0, L2h=0.0)))
    out.append(("c_nmf", "maxit0", dict(m=60, n=80, k=4, tol=0.0, maxit=0, L1w=0.0, L1h=0.0, L2w=0.0, L2h=0.0)))
    out.append(("c_nmf", "stop_by_tol", dict(m=150, n=200, k=6, tol=1e-3, maxit=40, L1w=0.01, L1h=0.01, L2w=0.0, L2h=0.0)))
    out.append(("c_nmf", "distinct_penalties", dict(m=150, n=200, k=9, tol=0.0, maxit=4, L1w=0.02, L1h=0.005, L2w=0.01, L2h=0.0)))
    out.append(("c_nmf_dense", "sparse_rhs", dict(m=90, n=110, k=7, inv_density=10, maxit=3)))     # < half non-zero
    out.append(("c_nmf_dense", "gemm_rhs", dict(m=90, n=110, k=7, inv_density=1, maxit=3)))        # > half non-zero
    out.append(("c_nmf_sparse_list", "uneven", dict(m=150, n=200, k=10, maxit=3, widths=(7, 90, 1), t_widths=(64, 5))))
    for name, kw in [("both", dict(lh="full", lw="full")), ("h_only", dict(lh="full", lw=None)),
                     ("w_only_one_by_one", dict(lh="1x1", lw="full")), ("mismatch", dict(lh="short", lw="short"))]:
        out.append(("c_linked_nmf", name, dict(m=120, n=150, k=8, maxit=3, L1=0.01, L2=0.0, **kw)))
    for name, orient in [("k_by_m", "km"), ("m_by_k", "mk"), ("square", "square")]:
        out.append(("c_project_model", name, dict(k=9, orient=orient, L1=0.01, L2=0.0)))
        out.append(("rcpp_predict", name, dict(k=9, orient=orient, L1=0.01, L2=0.0)))
    # ---- masked drivers
    for q, k in enumerate(ARD_RANKS):
        trace = 1 + q % 3
        out.append(("c_ard_nmf", "k%d" % k, dict(m=220, n=260, k=k, tol=0.0, maxit=3 if k <= 50 else 2, L1=0.01, L2=0.0, seed=77,
                                                 inv_density=20, thr=1e-3, trace=2 if k == 85 else trace)))
    out.append(("c_ard_nmf", "k100_seed%x" % 0xA13, dict(m=220, n=260, k=100, tol=0.0, maxit=2, L1=0.01, L2=0.0, seed=77, inv_density=20,
                                                         thr=1e-3, trace=1, mseed=0xA13)))
    for trace in (1, 2, 3):
        for maxit in (6, 5):
            out.append(("c_ard_nmf", "trace%d_maxit%d" % (trace, maxit), dict(m=110, n=140, k=5, tol=0.0, maxit=maxit, L1=0.01, L2=0.0,
                                                                             seed=31, inv_density=10, thr=1e-3, trace=trace)))
    out.append(("c_ard_nmf", "k86_dies", dict(m=220, n=260, k=86, tol=0.0, maxit=2, L1=0.01, L2=0.0, seed=77, inv_density=20, thr=1e-3, trace=2)))
    out.append(("c_ard_nmf", "overfit_break", dict(m=110, n=140, k=5, tol=0.0, maxit=9, L1=0.0, L2=0.0, seed=31, inv_density=10, thr=-1.0, trace=2)))
    out.append(("c_ard_nmf", "stop_by_tol", dict(m=110, n=140, k=5, tol=5e-3, maxit=40, L1=0.01, L2=0.0, seed=31, inv_density=10, thr=1.0, trace=3)))
    out.append(("c_ard_nmf", "maxit0", dict(m=60, n=80, k=4, tol=0.0, maxit=0, L1=0.0, L2=0.0, seed=31, inv_density=10, thr=1e-3, trace=2)))
    out.append(("c_ard_nmf", "inv_density1", dict(m=60, n=80, k=4, tol=0.0, maxit=2, L1=0.0, L2=0.0, seed=31, inv_density=1, thr=1e-3, trace=1)))
    out.append(("c_ard_nmf_dense", "k6", dict(m=70, n=90, k=6, maxit=3, trace=2)))
    out.append(("c_ard_nmf_sparse_list", "uneven", dict(m=110, n=140, k=6, maxit=4, trace=3, widths=(5, 70, 1), t_widths=(40, 3))))
    # ---- graph-convolutional fit, spatial graph, row-wise compression (restated in numpy under tests/)
    for name, orient, graph in [("lattice_km", "km", "lattice"), ("directed_mk", "mk", "directed"), ("odd_square", "square", "odd")]:
        out.append(("c_gcnmf", name, dict(k=6, orient=orient, graph=graph, maxit=3, L1=0.01, L2=0.0)))
    # columns of kNN length (20 entries) and one hub of 129: the stored-order sum on columns longer than a lattice's 9
    for k in (6, 34):
        out.append(("c_gcnmf", "knn_hub_k%d" % k, dict(k=k, orient="km", graph="knn_hub", side=14, maxit=3, L1=0.01, L2=0.0)))
    out.append(("spatial_graph", "lattice_max_k", dict(kind="lattice", side=9, max_dist=2.5, max_k=7)))
    out.append(("spatial_graph", "coincident", dict(kind="coincident", n=60, max_dist=0.2, max_k=100)))
    out.append(("spatial_graph", "random", dict(kind="random", n=150, max_dist=0.13, max_k=12)))
    out.append(("rowwise_sparse", "n10", dict(nrow=120, ncol=37, n=10)))
    out.append(("rowwise_sparse", "n7_empty_tail", dict(nrow=123, ncol=37, n=7)))
    out.append(("rowwise_dense", "n4", dict(nrow=48, ncol=9, n=4)))
    return out


def case_id(case):
    return "%s-%s" % (case[0], case[1])


def _w_oriented(w0, orient):
    """w0 is (m, k); R orientation k x m ("km"), m x k ("mk"), or square m == k ("square": not transposed by c_gcnmf /
    Rcpp_predict, transposed by c_project_model)."""
    return w0.T if orient == "km" else w0


def _proj_inputs(ora, p):
    m = p["k"] if p["orient"] == "square" else 130
    A = ragged(ora, m, 170, 10)
    return A, _w_oriented(ora.synth_winit(p["k"], m), p["orient"])


def inputs(ora, case):
    """The inputs of a case as a dict (also what the GPU test feeds the product)."""
    entry, name, p = case
    if entry in ("c_nmf", "c_ard_nmf"):
        A = ragged(ora, p["m"], p["n"], 20, p.get("seed" if entry == "c_nmf" else "mseed"))
        if entry == "c_ard_nmf" and name in ("k85", "k86_dies"):
            A = ora.synth_csc(p["m"], p["n"], 20)      # the fit of test_gpu_degenerate.py whose factor dies
        return dict(A=A, At=A.t(), w0=ora.synth_winit(p["k"], p["m"]))
    if entry in ("c_nmf_dense", "c_ard_nmf_dense"):
        A = ragged(ora, p["m"], p["n"], p.get("inv_density", 10))
        return dict(D=A.to_dense(), w0=ora.synth_winit(p["k"], p["m"]))
    if entry in ("c_nmf_sparse_list", "c_ard_nmf_sparse_list"):
        A = ragged(ora, p["m"], p["n"], 10)
        return dict(A=A, At=A.t(), A_=chunks(ora, A, p["widths"]), At_=chunks(ora, A.t(), p["t_widths"]), w0=ora.synth_winit(p["k"], p["m"]))
    if entry == "c_linked_nmf":
        A = ragged(ora, p["m"], p["n"], 10)
        rng = np.random.default_rng(3)
        k = p["k"]

        def link(kind, cols):
            if kind is None:
                return None
            if kind == "1x1":
                return np.ones((1, 1))
            if kind == "short":
                return (rng.random((k, cols - 1)) < 0.7).astype(np.float64)     # column count matches no side: ignored
            L = (rng.random((k, cols)) < 0.7).astype(np.float64)
            L[0] = 1.0
            return L
        return dict(A=A, At=A.t(), w0=ora.synth_winit(k, p["m"]), link_h=link(p["lh"], p["n"]), link_w=link(p["lw"], p["m"]))
    if entry in ("c_project_model", "rcpp_predict"):
        A, w = _proj_inputs(ora, p)
        return dict(A=A, w=w)
    if entry == "c_gcnmf":
        import gcnmf_restatement as gr
        side = p.get("side", 8)
        n = side * side
        m = p["k"] if p["orient"] == "square" else 90
        A = ragged(ora, m, n, 6)
        G = dict(lattice=lambda: gr.lattice_graph(ora, side), directed=lambda: gr.random_directed_graph(ora, n, 4, 9),
                 odd=lambda: gr.sparse_odd_graph(ora, n, 4),
                 knn_hub=lambda: gr.knn_hub_graph(ora, n, hubs=(77,), hub_len=129, seed=31))[p["graph"]]()
        return dict(A=A, At=A.t(), G=G, w0=ora.synth_winit(p["k"], m), w=_w_oriented(ora.synth_winit(p["k"], m), p["orient"]))
    if entry == "spatial_graph":
        rng = np.random.default_rng(21)
        if p["kind"] == "lattice":
            y, x = np.divmod(np.arange(p["side"] ** 2), p["side"])
            return dict(x=x.astype(np.float64), y=y.astype(np.float64))
        x, y = rng.random(p["n"]), rng.random(p["n"])
        if p["kind"] == "coincident":
            x[10:20], y[10:20] = x[3], y[3]       # eleven points in one place
        return dict(x=x, y=y)
    if entry in ("rowwise_sparse", "rowwise_dense"):
        A = ragged(ora, p["nrow"], p["ncol"], 4)
        if p["nrow"] % p["n"]:                     # the reference is defined only when the rows past the last whole bin are empty
            keep = A.i < (p["nrow"] // p["n"]) * p["n"]
            col = np.repeat(np.arange(A.ncol), np.diff(A.p))
            pp = np.zeros(A.ncol + 1, dtype=np.int32)
            np.cumsum(np.bincount(col[keep], minlength=A.ncol), out=pp[1:])
            A = ora.CSC(A.x[keep], A.i[keep], pp, A.nrow, A.ncol)
        return dict(A=A, D=A.to_dense())
    raise KeyError(entry)


def predict_inputs(ora, p):
    """(matrix whose columns are solved, factor, warm start) of a predict / predict_mask case: A and w on the H side,
    t(A) and h on the W side (mask_t)"""
    A = ragged(ora, 130, 170, 10)
    k = p["k"]
    M = A.t() if p["mask_t"] else A
    F = _factor(M.nrow, k, 5, ora)
    X0 = _factor(M.ncol, k, 6, ora) * (_factor(M.ncol, k, 7, ora) < 0.6) if p["warm"] else np.zeros((M.ncol, k))
    return M, F, X0


def mse_inputs(ora, p):
    k = p["k"]
    return ragged(ora, 130, 170, 10), _factor(130, k, 5, ora), 1.0 + np.arange(k) / 3.0, _factor(170, k, 6, ora)


def degenerate_inputs(ora, p):
    """tests/test_gpu_degenerate.py: a factor whose row is all zero ("dead"), or holds one entry ("single")"""
    A = ora.synth_csc(150, 200, 10)
    k = p["k"]
    M = A.t() if p["mask_t"] else A
    F = np.random.default_rng(5).random((M.nrow, k))
    F[:, k // 3] = 0.0
    if p["case"] == "single":
        F[17, k // 3] = 2.0
    return A, M, F


def scale_cor_inputs(p):
    rng = np.random.default_rng(11 + p["k"] + p["cols"])
    F = rng.random((p["cols"], p["k"]))
    if "zero_row" in p:
        F[:, p["zero_row"]] = 0.0
    return F, 0.7 * F + 0.3 * rng.random(F.shape)


def nnls_inputs(k):
    """the inputs of tests/test_gpu_ops.py::test_nnls (at k = 100, 17 of the 300 columns run into the 100-sweep cap)"""
    rng = np.random.default_rng(k)
    ncols = 300
    F = rng.random((4 * k + 5, k))
    B = rng.normal(size=(ncols, k)) * 3 + 1.0
    X0 = np.abs(rng.normal(size=(ncols, k))) * (rng.random((ncols, k)) < 0.6) * 1e-3
    return F, B, X0


def _factor(rows, k, seed, ora):
    return ora.synth_winit(k, rows, seed)


def run(case, L, ora):
    """Run a case on L (the oracle module, or a variant of oracle.reference).  ora: the oracle module, for inputs."""
    entry, name, p = case
    if entry == "nnls":
        F, B, X0 = nnls_inputs(p["k"])
        G = L.aat(F)
        X, R = np.empty_like(X0), np.empty_like(B)
        for c in range(B.shape[0]):
            X[c], R[c], _ = L.nnls(G, B[c], X0[c], p["L1"], p["L2"])
        return dict(x=X, b=R)
    if entry == "nnls_quirks":
        G = np.array([[2.0, 0.5], [0.5, 1.0]])
        Gb = np.array([[1.0, 0.999999], [0.999999, 1.0]])
        runs = [(G, [-1.0, -1.0], [0.0, 0.0], 0.0, 0.0),      # a negative step on x == 0 does nothing (rests at zero)
                (G, [1.0, 1.0], [0.0, 0.0], 0.01, 0.0),       # L1 subtracted from every step
                (G, [-5.0, 3.0], [1.0, 0.0], 0.0, 0.0),       # clamped from a positive value: tol overwritten with 1
                (G, [1.0, 1.0], [0.5, 0.25], 0.0, 0.3),       # L2 on a warm start
                (Gb, [1.0, 1.0000001], [0.0, 0.0], 0.0, 0.0)]  # runs into the 100-sweep cap
        xs, bs = [], []
        for g, b, x, L1, L2 in runs:
            xo, bo, _ = L.nnls(g, np.array(b), np.array(x), L1, L2)
            xs.append(xo)
            bs.append(bo)
        return dict(x=np.array(xs), b=np.array(bs))
    if entry == "scale_cor":
        F, y = scale_cor_inputs(p)
        S, d = L.scale(F)
        return dict(s=S, d=d, cor=np.array([L.cor(F, y)]))
    if entry == "aat":
        return dict(g=L.aat(np.random.default_rng(2).random((p["cols"], p["k"]))))
    if entry in ("predict", "predict_mask"):
        M, F, X0 = predict_inputs(ora, p)
        mask_t = p["mask_t"]
        if entry == "predict":
            X = L.predict(M, F, X0, p["L1"], p["L2"], 0)
        else:
            X = L.predict_mask(M, 99, 8, F, X0, p["L1"], p["L2"], 0, mask_t)
        return dict(x=X)
    if entry == "predict_mask_degenerate":
        k, mask_t = p["k"], p["mask_t"]
        _, M, F = degenerate_inputs(ora, p)
        return dict(x=L.predict_mask(M, 99, 8, F, np.zeros((M.ncol, k)), 0.01, 0.0, 0, mask_t))
    if entry == "predict_dense":
        D = ragged(ora, 40, 50, 3).to_dense()
        F = _factor(40, p["k"], 5, ora)
        if L is ora:       # the oracle has no dense predict of its own outside its drivers: densified == sparse with stored zeros
            full = ora.CSC(D.T.ravel(), np.tile(np.arange(40, dtype=np.int32), 50), np.arange(51, dtype=np.int32) * 40, 40, 50)
            return dict(x=ora.predict(full, F, np.zeros((50, p["k"])), 0.01, 0.0, 0))
        return dict(x=L.predict_dense(D, F, np.zeros((50, p["k"])), 0.01, 0.0, 0))
    if entry == "mse_test":
        A, w, d, h = mse_inputs(ora, p)
        return dict(mse=np.array([L.mse_test(A, w, d, h, 31, p["inv_density"], 0)]))
    I = inputs(ora, case)
    if entry == "c_nmf":
        r = L.c_nmf(I["A"], I["At"], p["tol"], p["maxit"], p["L1w"], p["L1h"], p["L2w"], p["L2h"], 0, I["w0"])
    elif entry == "c_nmf_dense":
        r = L.c_nmf_dense(I["D"], 0.0, p["maxit"], 0.01, 0.01, 0.0, 0.0, 0, I["w0"])
    elif entry == "c_nmf_sparse_list":
        r = L.c_nmf_sparse_list(I["A_"], I["At_"], 0.0, p["maxit"], 0.01, 0.0, 0, I["w0"])
    elif entry == "c_linked_nmf":
        r = L.c_linked_nmf(I["A"], I["At"], 0.0, p["maxit"], p["L1"], p["L2"], 0, I["w0"], I["link_h"], I["link_w"])
    elif entry == "c_project_model":
        return L.c_project_model(I["A"], I["w"], p["L1"], p["L2"], 0)
    elif entry == "rcpp_predict":
        return dict(h=L.rcpp_predict(I["A"], I["w"], p["L1"], p["L2"], 0))
    elif entry == "c_ard_nmf":
        r = L.c_ard_nmf(I["A"], I["At"], p["tol"], p["maxit"], p["L1"], p["L2"], 0, I["w0"], p["seed"], p["inv_density"], p["thr"], p["trace"])
    elif entry == "c_ard_nmf_dense":
        r = L.c_ard_nmf_dense(I["D"], 0.0, p["maxit"], 0.01, 0.0, 0, I["w0"], 31, 10, 1e-3, p["trace"])
    elif entry == "c_ard_nmf_sparse_list":
        r = L.c_ard_nmf_sparse_list(I["A_"], I["At_"], 0.0, p["maxit"], 0.01, 0.0, 0, I["w0"], 31, 10, 1e-3, p["trace"])
    elif entry == "c_gcnmf":
        if L is ora:
            import gcnmf_restatement as gr
            # a square w is taken as k x m as it stands: in the (m, k) convention of the restatement that is its transpose
            r = gr.c_gcnmf(ora, I["A"], I["At"], I["G"], 0.0, p["maxit"], p["L1"], p["L2"], I["w0"].T if p["orient"] == "square" else I["w0"])
        else:
            r = L.c_gcnmf(I["A"], I["At"], I["G"], 0.0, p["maxit"], p["L1"], p["L2"], I["w"])
    elif entry == "spatial_graph":
        if L is ora:
            import spatial_graph_restatement as sr
            pp, ii, xx = sr.brute(I["x"], I["y"], p["max_dist"], p["max_k"])
        else:
            pp, ii, xx = L.spatial_graph(I["x"], I["y"], p["max_dist"], p["max_k"])
        return dict(p=np.asarray(pp, dtype=np.int64), i=np.asarray(ii, dtype=np.int64), x=xx)
    elif entry in ("rowwise_sparse", "rowwise_dense"):
        if L is ora:
            import rowwise_compress_restatement as rr
            res = rr.vectorised_sparse(I["A"], p["n"]) if entry == "rowwise_sparse" else rr.vectorised_dense(I["D"], p["n"])
        else:
            res = L.rowwise_compress_sparse(I["A"], p["n"]) if entry == "rowwise_sparse" else L.rowwise_compress_dense(I["D"], p["n"])
            assert res is not None, "the reference indexes outside a matrix here"
        return dict(res=np.ascontiguousarray(res))
    else:
        raise KeyError(entry)
    out = dict(w=r["w"], d=r["d"], h=r["h"])
    if "test_mse" in r:
        out.update(test_mse=r["test_mse"], iter=np.asarray(r["iter"], dtype=np.int64), tol=r["tol"], score_overfit=r["score_overfit"])
    else:
        out["n_iter"] = np.array([r["iter"]], dtype=np.int64)
        out["tol_printed"] = np.array([float("%8.2e" % t) for t in r["tol"]])
    return out


def rel(a, b):
    """relative Frobenius distance over the entries finite in b (the NaN / Inf pattern is compared apart)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    nb = np.linalg.norm(b[fin])
    return float(np.linalg.norm(a[fin] - b[fin]) / (nb if nb > 0 else 1.0))


def same_structure(a, b, key="x"):
    """identical NaN and Inf patterns, and for the PATTERNED outputs identical zero patterns"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
            and (key not in PATTERNED or np.array_equal(a == 0, b == 0)))


# ---------------------------------------------------------------- the stored form (tests/golden/als_ref.npz)
FULL = 256      # outputs up to this many elements are stored whole
SAMPLE = 192    # larger ones: about this many elements at a fixed stride of the flattened array, the norm, the structure digest


def _digest(a, key):
    import hashlib
    a = np.ascontiguousarray(a, dtype=np.float64)
    zero = (a == 0) if key in PATTERNED else np.zeros(a.shape, dtype=bool)
    bits = np.concatenate([np.packbits(np.isnan(a).ravel()), np.packbits(np.isinf(a).ravel()), np.packbits(zero.ravel())])
    return np.frombuffer(hashlib.sha1(bits.tobytes()).digest(), dtype=np.uint8).copy()


def _norm(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.linalg.norm(a[np.isfinite(a)]))


def pack(prefix, out, store):
    """Put the outputs of one case into `store` (the dict that becomes the .npz) under prefix/..."""
    for key, a in out.items():
        a = np.asarray(a)
        if is_exact(key) or a.size <= FULL:
            store["%s/%s" % (prefix, key)] = a
        else:
            a = np.ascontiguousarray(a, dtype=np.float64)
            stride = -(-a.size // SAMPLE)
            store["%s/%s@sample" % (prefix, key)] = a.ravel()[::stride].copy()
            store["%s/%s@meta" % (prefix, key)] = np.array([a.size, stride, _norm(a)], dtype=np.float64)
            store["%s/%s@digest" % (prefix, key)] = _digest(a, key)


def against_stored(prefix, key, a, store):
    """(distance, structure equal) of output `a` to the stored reference output.  Exact keys: (0 or 1, equal)."""
    a = np.asarray(a)
    full = "%s/%s" % (prefix, key)
    if full in store:
        b = store[full]
        if is_exact(key):
            same = a.shape == b.shape and np.array_equal(a, b)
            return (0.0 if same else 1.0), same
        return rel(a, b), same_structure(a, b, key)
    size, stride, norm = store[full + "@meta"]
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.size != int(size):
        return 1.0, False
    dist = max(rel(a.ravel()[::int(stride)], store[full + "@sample"]), abs(_norm(a) - norm) / (norm if norm > 0 else 1.0))
    return dist, bool(np.array_equal(_digest(a, key), store[full + "@digest"]))


def same_bits(a, b):
    """equal bit for bit, every NaN equal to every NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    keep = ~np.isnan(a)
    return bool(np.array_equal(a[keep].view(np.uint64), b[keep].view(np.uint64)))
