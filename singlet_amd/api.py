"""Host-side mirror of singlet's R interface for the ALS hot path.

The reference's host language is R (absent from this image), so the functions
the R drivers call are mirrored here one-for-one in Python, with the same
names, argument order, defaults and return fields:

  c_nmf / c_ard_nmf / c_project_model   R/RcppExports.R:28-30, 78-80, 24-26
  c_gcnmf                               src/RcppExports.cpp:399-417
  run_nmf                               R/run_nmf.R:18-77
  run_gcnmf                             R/RunGCNMF.R:20-98
  c_LKNN / c_SNN                        src/singlet.cpp:1491-1665 (glue src/RcppExports.cpp:466-467)
  find_local_neighbors                  R/FindLocalNeighbors.R:32-101
  rescale_spatial                       R/RescaleSpatial.R:10-22
  RasterizeRowwise, rowwise_compress_*  R/rasterize_rowwise.R; src/singlet.cpp:146-180
  ard_nmf                               R/ard_nmf.R:31-193
  cross_validate_nmf                    R/cross_validate_nmf.R:18-105
  GetBestRank                           R/GetBestRank.R:8-46
  project_model                         R/ProjectData.R:11-19
  RunNMF (matrix steps), subset         R/RunNMF.R:61-151; A[features, ] (:72-81), R/ProjectData.R:68-69
  run_linked_nmf                        R/RunLNMF.R:18-66
  RunLNMF (matrix steps)                R/RunLNMF.R:111-159
  MetadataSummary                       R/MetadataSummary.R:15-36 (without the hclust display order)
  GetSharedFactors / GetUniqueFactors   R/GetSharedFactors.R:4-10, R/GetUniqueFactors.R:4-10
  group_means                           the k G calls of mean(h[which(...)]) of R/RunLNMF.R:136-143, R/MetadataSummary.R:18-26
  find_variable_features                Seurat::FindVariableFeatures(selection.method = "vst"), what R/RunNMF.R:73-74 reads as
                                        "var.features", under the rules stated in include/singlet_hip.h (the trend is an
                                        exact local fit at every gene, not R's interpolated loess)
  evaluate                              no R counterpart: the full-matrix error of a model (mse_test, src/singlet.cpp:536-568,
                                        with every entry drawn), per cell and per gene
  run_gsea                              RunGSEA (R/RunGSEA.R:27-138) with the gene sets given by the caller and a permutation
                                        null in place of fgseaMultilevel (include/singlet_hip.h, "Gene set enrichment")
  score_signatures                      UCell's ScoreSignatures_UCell: the rank-based score of gene signatures in every cell
                                        (include/singlet_hip.h, "Signature scores")
  score_doublets                        no R counterpart in the reference (it hands the object to Seurat): the scheme of Scrublet
                                        with the simulator on the device (include/singlet_hip.h, "Simulated doublets")
  find_all_markers / find_markers       Seurat::FindAllMarkers / FindMarkers(test.use = "wilcox") under the rules stated in
                                        include/singlet_hip.h, "Marker genes" (the filters are applied after the test)

Matrices follow R's orientation: w is returned k x m by c_nmf and m x k by
run_nmf / ard_nmf (they transpose and sort by d, R/run_nmf.R:65-68); h is
k x n.  All numerics run in libsinglet_hip.so on the GPU; nothing here computes
on the CPU beyond bookkeeping.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, ptr
from ._marshal import NHOOD_INFO, NHOOD_STATS, NHOOD_TALLIES, ligrec_call, ligrec_inputs, nhood_labels, ArdOutputs, NmfOutputs, annotate_call, annotate_tail, colmajor, csc_ptrs, gsea_inputs, gsea_score_type, knn_call, knn_ivf_shape, knn_method, knn_metric, knn_recall, knn_weighting, label_list, markers_call, signature_call
from .context import _chunk_lists, _link_image, make_callbacks
from .native import NativeMatrix
from .sparse import as_dgCMatrix, dgCMatrix


# ---------------------------------------------------------------------------
# RcppExports layer
# ---------------------------------------------------------------------------
def _w_in(w, nrow):
    """R matrix k x m (column-major) -> (m, k) C-contiguous buffer."""
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 2 or w.shape[1] != nrow:
        raise ValueError("w must be a k x nrow(A) matrix (got %r, nrow(A) = %d)" % (w.shape, nrow))
    return np.ascontiguousarray(w.T)


def _verbose_log(verbose, ard=False):
    if not verbose:
        return None
    if ard:
        print("\n%4s | %8s | %8s \n---------------------------" % ("iter", "tol", "overfit"))

        def log(it, tol, of):
            print("%4d | %8.2e | %s" % (it, tol, ("%8s" % "-") if math.isnan(of) else ("%8.2e" % of)))
    else:
        print("\n%4s | %8s \n---------------" % ("iter", "tol"))

        def log(it, tol, of):
            print("%4d | %8.2e" % (it, tol))
    return log


CALL_TIMES_KEYS = ("h2d_s", "validate_s", "transpose_s", "fit_init_s", "iterate_s", "d2h_s", "h2d_bytes", "cached", "total_s")


def call_times():
    """Host wall-clock split of this thread's last one-shot call (c_nmf / c_ard_nmf): sgl_call_times_get."""
    out = np.zeros(len(CALL_TIMES_KEYS))
    check(_lib.load().sgl_call_times_get(ptr(out, f64p), int(out.size)))
    return dict(zip(CALL_TIMES_KEYS, (float(v) for v in out)))


def _fit(fn, inp, tol, maxit, verbose, penalties, threads, extra=(), ard=False, w_m_by_k=False):
    """The body the one-shot fits share.  inp: (the matrix arguments, (m, n, k), the w arguments, what must stay alive) as
    _sparse_in / _dense_in / _list_in spell them; extra: what the entry point takes between k and its outputs.  The log
    header is printed here, after every check of the inputs."""
    matrix, shape, w, _keep = inp
    out = ArdOutputs(shape, maxit) if ard else NmfOutputs(shape, maxit, w_m_by_k)
    cb = make_callbacks(_verbose_log(verbose, ard))
    check(fn(*matrix, float(tol), int(maxit), int(bool(verbose)), *penalties, int(threads), *w, *extra, *out.args(), C.byref(cb)))
    return out.result()


def _ard_extra(seed, inv_density, overfit_threshold, trace_test_mse):
    return int(seed), int(inv_density), float(overfit_threshold), int(trace_test_mse)


def _sparse_in(A, At, w):
    A = as_dgCMatrix(A)
    At = None if At is None else as_dgCMatrix(At)
    wb = _w_in(w, A.nrow)
    k = wb.shape[1]
    return (*csc_ptrs(A), *csc_ptrs(At), A.nrow, A.ncol), (A.nrow, A.ncol, k), (ptr(wb, f64p), k), (A, At, wb)


def _dense_in(A, w):
    Af = colmajor(A, "A must be a matrix")
    n, m = Af.shape
    wb = _w_in(w, m)
    k = wb.shape[1]
    return (ptr(Af, f64p), m, n), (m, n, k), (ptr(wb, f64p), k), (Af, wb)


def _list_in(A_, At_, w):
    a, t, nrow, n, keep = _chunk_lists(A_, At_, "A_ must hold at least one matrix", "all chunks of A_ must have the same number of rows")
    wb = _w_in(w, nrow)
    k = wb.shape[1]
    return (*a, *t, nrow), (nrow, n, k), (ptr(wb, f64p), k), (keep, wb)


def c_nmf(A, At, tol, maxit, verbose, L1_w, L1_h, L2_w, L2_h, threads, w):
    """.Call(`_singlet_c_nmf`, ...) -> list(w = k x m, d = k, h = k x n)  (src/singlet.cpp:665)."""
    L = _lib.load()
    return _fit(L.sgl_c_nmf, _sparse_in(A, At, w), tol, maxit, verbose, (L1_w, L1_h, L2_w, L2_h), threads)


def c_nmf_dense(A, At, tol, maxit, verbose, L1_w, L1_h, L2_w, L2_h, threads, w):
    """.Call(`_singlet_c_nmf_dense`, ...) -> list(w, d, h)  (src/singlet.cpp:1052-1054).  A: dense m x n
    array; At is accepted for signature parity and ignored (the transpose is built on the device)."""
    L = _lib.load()
    return _fit(L.sgl_c_nmf_dense, _dense_in(A, w), tol, maxit, verbose, (L1_w, L1_h, L2_w, L2_h), threads)


def c_nmf_sparse_list(A_, At_, tol, maxit, verbose, L1, L2, threads, w):
    """.Call(`_singlet_c_nmf_sparse_list`, ...)  (src/singlet.cpp:715-743): A_ is a list of column chunks of A
    (the predict over chunks carries a running column offset, :384-402), At_ a list of column chunks of t(A)
    (None / empty: the transpose is built on the device).  The chunks are joined on the device."""
    L = _lib.load()
    return _fit(L.sgl_c_nmf_sparse_list, _list_in(A_, At_, w), tol, maxit, verbose, (L1, L2), threads)


def c_ard_nmf_sparse_list(A_, At_, tol, maxit, verbose, L1, L2, threads, w, rng_seed, inv_density, overfit_threshold,
                          trace_test_mse):
    """.Call(`_singlet_c_ard_nmf_sparse_list`, ...)  (src/singlet.cpp:1162-1234)."""
    L = _lib.load()
    return _fit(L.sgl_c_ard_nmf_sparse_list, _list_in(A_, At_, w), tol, maxit, verbose, (L1, L2), threads,
                _ard_extra(rng_seed, inv_density, overfit_threshold, trace_test_mse), ard=True)


def c_ard_nmf_dense(A, At, tol, maxit, verbose, L1, L2, threads, w, seed, inv_density, overfit_threshold, trace_test_mse):
    """.Call(`_singlet_c_ard_nmf_dense`, ...)  (src/singlet.cpp:1357-1361).  A: dense m x n array; At is accepted
    for signature parity and ignored."""
    L = _lib.load()
    return _fit(L.sgl_c_ard_nmf_dense, _dense_in(A, w), tol, maxit, verbose, (L1, L2), threads,
                _ard_extra(seed, inv_density, overfit_threshold, trace_test_mse), ard=True)


def c_linked_nmf(A, At, tol, maxit, verbose, L1, L2, threads, w, link_h, link_w):
    """.Call(`_singlet_c_linked_nmf`, ...) -> list(w, d, h)  (src/singlet.cpp:1059-1086).  link_h / link_w
    are R matrices (rows x cols); a link whose column count does not match its side is ignored, as in
    the reference (R/RunLNMF.R passes a 1 x 1 matrix to switch a side off)."""
    L = _lib.load()
    inp = _sparse_in(A, At, w)
    lh, lhr, lhc, keep_h = _link_image(link_h)
    lw, lwr, lwc, keep_w = _link_image(link_w)
    return _fit(L.sgl_c_linked_nmf, inp, tol, maxit, verbose, (L1, L2), threads, (lh, lhr, lhc, lw, lwr, lwc))


def _w_either(w, nrow, square_is_k_by_m):
    """A w that may come k x m or m x k -> (its column-major image, rows, cols, k).  The reference has two rules for which
    it is, and they stay two: c_project_model (src/singlet.cpp:406) reads w as m x k whenever nrow(w) == nrow(A);
    c_gcnmf (l.1713) and Rcpp_predict (l.350-367) only when w is not square as well (square_is_k_by_m)."""
    wf = colmajor(w, "w must be a matrix")
    w_cols, w_rows = wf.shape
    return wf, w_rows, w_cols, (w_cols if _w_is_m_by_k(w_rows, w_cols, nrow, square_is_k_by_m) else w_rows)


def _w_is_m_by_k(w_rows, w_cols, nrow, square_is_k_by_m):
    return w_rows == nrow and not (square_is_k_by_m and w_rows == w_cols)


def c_gcnmf(A, At, G, tol, maxit, verbose, L1, L2, threads, w):
    """.Call(`_singlet_c_gcnmf`, ...) -> list(w = m x k, d, h = k x n)  (src/singlet.cpp:1668-1730).  G: the n x n cell
    graph (may be asymmetric).  w: k x m or m x k, transposed iff nrow(w) == nrow(A) and w is not square (l.1713).
    Unlike c_nmf, w comes back m x k, as the reference returns it; "iter" / "tol" are extras of this mirror."""
    L = _lib.load()
    A = as_dgCMatrix(A)
    At = None if At is None else as_dgCMatrix(At)
    G = as_dgCMatrix(G)
    wf, w_rows, w_cols, k = _w_either(w, A.nrow, square_is_k_by_m=True)
    inp = ((*csc_ptrs(A), *csc_ptrs(At), A.nrow, A.ncol, *csc_ptrs(G), G.nrow, G.ncol), (A.nrow, A.ncol, k),
           (ptr(wf, f64p), w_rows, w_cols, k), (A, At, G, wf))
    return _fit(L.sgl_c_gcnmf, inp, tol, maxit, verbose, (float(L1), float(L2)), threads, w_m_by_k=True)   # w_out: m x k column-major


def c_ard_nmf(A, At, tol, maxit, verbose, L1, L2, threads, w, seed, inv_density, overfit_threshold, trace_test_mse):
    """.Call(`_singlet_c_ard_nmf`, ...) -> list(w, d, h, test_mse, iter, tol, score_overfit) (src/singlet.cpp:1144-1151)."""
    L = _lib.load()
    return _fit(L.sgl_c_ard_nmf, _sparse_in(A, At, w), tol, maxit, verbose, (L1, L2), threads,
                _ard_extra(seed, inv_density, overfit_threshold, trace_test_mse), ard=True)


def c_project_model(A, w, L1, L2, threads):
    """.Call(`_singlet_c_project_model`, ...) -> list(h = k x n, d = k)  (src/singlet.cpp:405-413)."""
    L = _lib.load()
    A = as_dgCMatrix(A)
    wf, w_rows, w_cols, k = _w_either(w, A.nrow, square_is_k_by_m=False)
    h_out, d_out = np.empty((A.ncol, k)), np.empty(k)
    check(L.sgl_c_project_model(*csc_ptrs(A), A.nrow, A.ncol, ptr(wf, f64p), w_rows, w_cols, L1, L2, int(threads),
                                ptr(h_out, f64p), ptr(d_out, f64p)))
    return {"h": h_out.T, "d": d_out}


def Rcpp_predict(A, w, L1, L2, threads):
    """.Call(`_singlet_Rcpp_predict`, ...) -> h (k x n)  (src/singlet.cpp:350-367)."""
    L = _lib.load()
    A = as_dgCMatrix(A)
    wf, w_rows, w_cols, k = _w_either(w, A.nrow, square_is_k_by_m=True)
    h_out = np.empty((A.ncol, k))
    check(L.sgl_rcpp_predict(*csc_ptrs(A), A.nrow, A.ncol, ptr(wf, f64p), w_rows, w_cols, L1, L2, int(threads), ptr(h_out, f64p)))
    return h_out.T


# ---------------------------------------------------------------------------
# R drivers
# ---------------------------------------------------------------------------
def _pair(v):
    v = list(np.atleast_1d(v))
    return (float(v[0]), float(v[0])) if len(v) != 2 else (float(v[0]), float(v[1]))


def _rng(seed):
    return seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)


def _sort_model(model, rn=None, cn=None):
    # sort_index <- order(model$d, decreasing = TRUE)   R/run_nmf.R:65-68
    idx = np.argsort(-model["d"], kind="stable")
    model["d"] = model["d"][idx]
    model["w"] = model["w"].T[:, idx]
    model["h"] = model["h"][idx, :]
    k = model["d"].shape[0]
    model["factor_names"] = ["NMF_%d" % (q + 1) for q in range(k)]
    model["rownames_w"] = rn
    model["colnames_h"] = cn
    return model


def _on_native(N, body):
    """body(ctx, fits) on one Context that holds the NativeMatrix N (native()), staged through the typed door
    (Context.upload_native); fits: the resident fits the drivers already run on (as RunNMF stages them).  The NativeMatrix
    case of every driver; what a driver checks before it stages, it checks before it calls this."""
    from .context import Context
    with Context(0) as ctx:
        ctx.upload_native(N)
        return body(ctx, _ResidentFits(None, ctx=ctx, Dimnames=N.Dimnames))


def run_nmf(A, rank, tol=1e-4, maxit=100, verbose=True, L1=0.01, L2=0, threads=0, seed=None, _fits=None):
    """R/run_nmf.R:18-77 (sparse, single-matrix branch).  `seed` replaces R's global RNG state
    (stats::runif, l.55): an int or numpy Generator.  A NativeMatrix (native()) is staged on the device as it is."""
    if _fits is None and isinstance(A, NativeMatrix):
        return _on_native(A, lambda ctx, fits: run_nmf(None, rank, tol, maxit, verbose, L1, L2, threads, seed, _fits=fits))
    if _fits is not None:   # RunNMF: the matrix is staged and resident already (A is not read)
        if verbose:
            print("running with sparse optimization")
        L1, L2 = _pair(L1), _pair(L2)
        w_init = _rng(seed).random((_fits.nrow, rank)).T
        model = _fits.c_nmf(tol, maxit, bool(verbose), L1[0], L1[1], L2[0], L2[1], threads, w_init)
        return _sort_model(model, _fits.Dimnames[0], _fits.Dimnames[1])
    dense_mode = isinstance(A, np.ndarray)   # R/run_nmf.R:41-46: a base matrix stays dense
    if not dense_mode:
        A = as_dgCMatrix(A)
        if verbose:
            print("running with sparse optimization")
    L1 = _pair(L1)
    L2 = _pair(L2)
    nrow = A.shape[0] if dense_mode else A.nrow
    # w_init <- matrix(stats::runif(nrow(A) * rank), rank, nrow(A))
    w_init = _rng(seed).random((nrow, rank)).T
    if dense_mode:
        model = c_nmf_dense(A, None, tol, maxit, bool(verbose), L1[0], L1[1], L2[0], L2[1], threads, w_init)
        return _sort_model(model, None, None)
    model = c_nmf(A, None, tol, maxit, bool(verbose), L1[0], L1[1], L2[0], L2[1], threads, w_init)
    return _sort_model(model, A.Dimnames[0], A.Dimnames[1])


def _gcnmf_on_team(A, G, tol, maxit, verbose, L1, L2, w, devices):
    """c_gcnmf's list from a fit on a one-process team (Multi): cells sharded over `devices`, the graph's crossing edges
    served by the halo exchange.  w as c_gcnmf takes it."""
    from .context import Multi
    A = as_dgCMatrix(A)
    G = as_dgCMatrix(G)
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError("w must be a matrix")
    given = w.shape
    if not _w_is_m_by_k(*w.shape, A.nrow, square_is_k_by_m=True):   # c_gcnmf's rule (l.1713): such a w is k x m; the team takes m x k
        w = w.T
    if w.shape[0] != A.nrow:
        raise ValueError("w is %d x %d; expected k x m or m x k with m = %d" % (given[0], given[1], A.nrow))
    with Multi([int(d) for d in devices]) as M:
        M.upload(A)
        M.fit_init(w.shape[1], w)
        M.set_graph(G)
        n_iter, tr = M.nmf_run(float(tol), int(maxit), float(L1), float(L1), float(L2), float(L2), log=_verbose_log(verbose))
        W, d, H = M.get_factors()
    return {"w": W, "d": d, "h": H.T, "iter": n_iter, "tol": tr}


def run_gcnmf(A, graph, k, split_by=None, tol=1e-5, L1=0.01, L2=0, verbose=2, maxit=100, threads=0, seed=None, devices=None):
    """The numeric steps of RunGCNMF.Seurat (R/RunGCNMF.R:20-98) on a genes x cells matrix: PreprocessData when every value
    is integral (l.42-45), weight_by_split when `split_by` (0-based group per cell) is given (l.62-68), w_init uniform k x
    nrow(A) (l.73-75; `seed` replaces R's RNG state: an int or numpy Generator), c_gcnmf, factor names GCNMF_1..k (l.78).
    There is NO sort by d (the reference has none).  Returns the c_gcnmf list (w m x k, d, h k x n) with "factor_names",
    "rownames_w" and "colnames_h".

    Two places follow the evident intent rather than the R code, which cannot run as written:
      - l.77 passes `G`, a name defined nowhere in the function, to c_gcnmf; here the `graph` argument is passed;
      - when `k` is a matrix, `w_init` is never assigned (l.71-76); here that matrix is the initial w (k x m or m x k,
        oriented by c_gcnmf's rule).

    devices: None runs c_gcnmf on the current device; a list of device ids (all distinct, or all equal: ranks sharing one
    device) runs the same fit cell-sharded on a Multi and returns the same dictionary."""
    A = as_dgCMatrix(A)
    rn, cn = A.Dimnames[0], A.Dimnames[1]
    v = A.x
    if np.sum(np.trunc(v)) == np.sum(v):   # sum(as.integer(v)) == sum(v)
        A = PreprocessData(A)
    if split_by is not None:
        sb = np.asarray(split_by)
        groups = np.unique(sb)
        sb = np.searchsorted(groups, sb).astype(np.int32)   # as.integer(as.numeric(as.factor(.))) - 1
        A = weight_by_split(A, sb, int(groups.size))
    At = None   # Matrix::t(A): built on the device
    if isinstance(k, np.ndarray) and k.ndim == 2:
        if A.nrow not in k.shape:
            raise ValueError("dimensions of matrix specified for 'k' are not compatible with number of rows in 'A'")
        w_init = k
    else:
        w_init = _rng(seed).random((A.nrow, int(k))).T   # matrix(runif(k * nrow(A)), k, nrow(A)), filled by column
    if devices is None:
        model = c_gcnmf(A, At, graph, tol, maxit, bool(verbose), L1, L2, threads, w_init)
    else:
        model = _gcnmf_on_team(A, graph, tol, maxit, bool(verbose), L1, L2, w_init, devices)
    kk = model["d"].shape[0]
    model["factor_names"] = ["GCNMF_%d" % (q + 1) for q in range(kk)]
    model["rownames_w"] = rn
    model["colnames_h"] = cn
    return model


def _staged(A, op, Dimnames=None):
    """Upload A (a NativeMatrix: through the typed door), run a staging operator on the device, return the transformed
    dgCMatrix (Dimnames: those of the result when the operator changes the shape)."""
    from .context import Context

    def body(c, fits=None):
        op(c)
        nrow, ncol, _ = c.dims()
        x, i, p = c.download(0)
        return dgCMatrix(x, i, p.astype(np.int32), (nrow, ncol), A.Dimnames if Dimnames is None else Dimnames)
    if isinstance(A, NativeMatrix):
        return _on_native(A, body)
    A = as_dgCMatrix(A)
    with Context(0) as c:
        c.upload(A, None)
        return body(c)


def PreprocessData(A, scale_factor=10000.0):
    """PreprocessData.dgCMatrix (R/PreprocessData.R:34-39): Seurat::LogNormalize of a counts matrix,
    log1p(x / colSums * scale_factor), computed on the device; dimnames kept."""
    return _staged(A, lambda c: c.log_normalize(scale_factor))


def _subset_index(sel, extent, names, what):
    """One axis of a subset as the library takes it: None, or a contiguous int32 array of 0-based indices.  sel: 0-based
    integers (any order, duplicates allowed), a boolean mask of the axis length, or names looked up in `names` (the
    first match, as R's `[` does).  R's negative "drop" indices are not mirrored: they raise."""
    if sel is None:
        return None
    a = np.asarray(sel)
    if a.ndim != 1:
        raise ValueError("subset: %s must be one-dimensional" % what)
    if a.size == 0:
        raise ValueError("subset: %s selects nothing (a matrix cannot be empty)" % what)
    if a.dtype == np.bool_:
        if a.shape[0] != extent:
            raise ValueError("subset: the boolean mask for %s has %d entries, the axis has %d" % (what, a.shape[0], extent))
        idx = np.flatnonzero(a)
    elif a.dtype.kind in "USO" and a.size and all(isinstance(v, (str, bytes, np.str_)) for v in a.tolist()):
        if names is None:
            raise ValueError("subset: %s are given by name, but that axis of A has no names" % what)
        first = {}
        for q, nm in enumerate(names):
            first.setdefault(nm, q)
        missing = [v for v in a.tolist() if v not in first]
        if missing:
            raise ValueError("subset: %d of the %s are not among the names of A (first: %r)" % (len(missing), what, missing[0]))
        idx = np.array([first[v] for v in a.tolist()], dtype=np.int64)
    elif a.dtype.kind in "iu":
        idx = a.astype(np.int64)
        if idx.size and int(idx.min()) < 0:
            raise ValueError("subset: negative index %d in %s (indices are 0-based; R's negative 'drop' indices are not "
                             "supported)" % (int(idx.min()), what))
        if idx.size and int(idx.max()) >= extent:
            raise ValueError("subset: index %d in %s is outside [0, %d)" % (int(idx.max()), what, extent))
    else:
        raise ValueError("subset: %s must be 0-based integers, a boolean mask or names" % what)
    if idx.size == 0:
        raise ValueError("subset: %s selects nothing (a matrix cannot be empty)" % what)
    return np.ascontiguousarray(idx, dtype=np.int32)


def _subset_names(names, idx):
    if names is None or idx is None:
        return names
    return [names[int(q)] for q in idx]


def subset(A, rows=None, cols=None):
    """A[rows, cols] computed on the device (sgl_subset): the A[features, ] of RunNMF.Seurat (R/RunNMF.R:72-81) and the
    gene alignment of ProjectData.Seurat (R/ProjectData.R:68-69).  rows / cols: 0-based integers in any order (duplicates
    allowed), a boolean mask of the axis length, names looked up in A.Dimnames, or None to keep the axis.  Returns a
    dgCMatrix with the selected Dimnames; the stored values, explicit zeros included, move bit for bit.  A NativeMatrix
    (native()) is staged through the typed door; the result is the same dgCMatrix (double values, sorted indices)."""
    if not isinstance(A, NativeMatrix):
        A = as_dgCMatrix(A)
    r = _subset_index(rows, A.nrow, A.Dimnames[0], "rows")
    c = _subset_index(cols, A.ncol, A.Dimnames[1], "cols")
    names = (_subset_names(A.Dimnames[0], r), _subset_names(A.Dimnames[1], c))
    return _staged(A, lambda ctx: ctx.subset(r, c), names)


def weight_by_split(A_, split_by, n_groups):
    """.Call(`_singlet_weight_by_split`, A_, split_by, n_groups)  (src/singlet.cpp:119-144):
    returns a rescaled copy; split_by is the 0-based group of every column (R/RunNMF.R:86)."""
    A = as_dgCMatrix(A_)
    sb = np.ascontiguousarray(split_by, dtype=np.int32)
    if sb.shape[0] != A.ncol:
        raise ValueError("split_by needs one entry per column of A")
    x = np.empty(A.nnz, dtype=np.float64)
    check(_lib.load().sgl_c_weight_by_split(*csc_ptrs(A), A.nrow, A.ncol, ptr(sb, i32p), int(n_groups), ptr(x, f64p)))
    return dgCMatrix(x, A.i, A.p, A.Dim, A.Dimnames)


# ---------------------------------------------------------------------------
# Row-wise rasterisation (RasterizeRowwise)
# ---------------------------------------------------------------------------
def _bin_size(n, who):
    """n as Rcpp's as<size_t> takes it: truncated toward zero.  NA is refused here; values below 1 by the library, with a
    message (include/singlet_hip.h: sgl_c_rowwise_compress_sparse)."""
    v = float(n)
    if math.isnan(v):
        raise _lib.SingletHipError(-1, "%s: n is NA: the bin size must be at least 1" % who)
    if v >= 2.0**63:
        return 2**63 - 1
    if v <= -2.0**63:
        return -2**63
    return int(v)


class RasterMatrix(np.ndarray):
    """The dense result of RasterizeRowwise: a Fortran-ordered float64 ndarray with R's dimnames, `rownames` and
    `colnames` (None where R's are NULL).  Arrays derived from it carry no names."""

    def __array_finalize__(self, obj):
        self.rownames = None
        self.colnames = None


def _raster_out(nb, ncol):
    return np.zeros((nb, ncol), dtype=np.float64, order="F")


def rowwise_compress_sparse(A, n=10, threads=0):
    """.Call(`_singlet_rowwise_compress_sparse`, A, n, threads)  (src/singlet.cpp:146-162): the floor(nrow / n) x ncol
    matrix of the means of every n consecutive rows of the dgCMatrix A (the last nrow mod n rows left out).  Rules:
    include/singlet_hip.h, sgl_c_rowwise_compress_sparse.  `threads` is ignored."""
    A = as_dgCMatrix(A)
    nn = _bin_size(n, "rowwise_compress_sparse")
    out = _raster_out(A.nrow // nn if 1 <= nn <= A.nrow else 0, A.ncol)
    check(_lib.load().sgl_c_rowwise_compress_sparse(*csc_ptrs(A), A.nrow, A.ncol, nn, ptr(out, f64p)))
    return out


def rowwise_compress_dense(A, n=10, threads=0):
    """.Call(`_singlet_rowwise_compress_dense`, A, n, threads)  (src/singlet.cpp:164-180): the same on a dense matrix,
    bit-identical to rowwise_compress_sparse on the same values.  `threads` is ignored."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 2:
        raise ValueError("rowwise_compress_dense: A must be a matrix")
    Af = np.asfortranarray(A)
    nrow, ncol = A.shape
    nn = _bin_size(n, "rowwise_compress_dense")
    out = _raster_out(nrow // nn if 1 <= nn <= nrow else 0, ncol)
    check(_lib.load().sgl_c_rowwise_compress_dense(ptr(Af, f64p) if Af.size else None, nrow, ncol, nn, ptr(out, f64p)))
    return out


def RasterizeRowwise(A, n=10, threads=0):
    """RasterizeRowwise (R/rasterize_rowwise.R): a dgCMatrix goes to rowwise_compress_sparse, anything else (as a dense
    matrix) to rowwise_compress_dense.  The result is a RasterMatrix with the names the R wrapper assigns: rownames
    rownames(A)[seq(1, floor(nrow / n) * n, n)], colnames colnames(A).  As in R, seq() fails when that range is empty
    (n > nrow)."""
    if isinstance(A, dgCMatrix):
        rn, cn = A.Dimnames
        B = rowwise_compress_sparse(A, n, threads)
        nrow = A.nrow
    else:
        rn = cn = None
        M = A.toarray() if hasattr(A, "toarray") else A   # as.matrix(A)
        B = rowwise_compress_dense(M, n, threads)
        nrow = np.shape(M)[0]
    to = math.floor(nrow / float(n)) * float(n)
    if to < 1:   # seq(1, to, n) with to < 1 and n > 0
        raise ValueError("RasterizeRowwise: wrong sign in 'by' argument (seq(1, %g, %g))" % (to, float(n)))
    steps = math.floor((to - 1) / float(n) + 1e-10)
    rows = [int(1 + q * float(n)) - 1 for q in range(steps + 1)]   # R truncates a double subscript
    out = B.view(RasterMatrix)
    if rn is not None:
        names = [rn[r] for r in rows]
        if len(names) != B.shape[0]:
            raise ValueError("RasterizeRowwise: length of 'dimnames' [1] not equal to array extent")
        out.rownames = names
    out.colnames = list(cn) if cn is not None else None
    return out


def project_model(A, w, L1=0.01, L2=0, threads=0):
    """R/ProjectData.R:11-19.  A NativeMatrix (native()) is staged through the typed door and projected on that context:
    scale(w) (Context.op_scale: the kernels of the one-shot call), fit_init(k, w), project_run -- the one-shot call's bits."""
    if isinstance(A, NativeMatrix):
        w = np.asarray(w, dtype=np.float64)
        if w.ndim != 2 or (w.shape[0] != A.nrow and w.shape[1] != A.nrow):
            raise ValueError("'w' must share a common edge with the rows of 'A'")
        wb = np.ascontiguousarray(w if w.shape[0] == A.nrow else w.T)   # (m, k), as c_project_model orients it (src/singlet.cpp:406)
        def body(ctx, fits):
            ws, _ = ctx.op_scale(wb)
            ctx.fit_init(ws.shape[1], ws)
            ctx.project_run(float(L1), float(L2))
            _, d, H = ctx.get_factors(w=False)
            return {"h": H.T, "d": d}
        return _on_native(A, body)
    A = as_dgCMatrix(A)
    w = np.asarray(w)
    if w.shape[0] != A.nrow and w.shape[1] != A.nrow:
        raise ValueError("'w' must share a common edge with the rows of 'A'")
    return c_project_model(A, w, L1, L2, threads)


class _Fits:
    """What the drivers fit through: c_ard_nmf / c_nmf without their two matrix arguments, and close(), also as a context
    manager."""

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _ResidentFits(_Fits):
    """One matrix kept in HBM across many fits (include/singlet_hip.h section 2): what R's ard_nmf /
    cross_validate_nmf do by calling c_ard_nmf / c_nmf again and again on the same A (R/ard_nmf.R:95-160,
    R/cross_validate_nmf.R:69-97), without re-uploading, re-transposing and re-validating it per call.
    Same arguments and return lists as c_ard_nmf / c_nmf; results are identical to the one-shot calls."""

    def __init__(self, A, device=0, ctx=None, Dimnames=(None, None)):
        """ctx: an already staged Context to adopt instead of uploading A (RunNMF); it stays the caller's to close, and
        Dimnames are the names of its resident matrix."""
        from .context import Context
        self._adopted = ctx is not None
        if self._adopted:
            self.ctx = ctx
            self.nrow = ctx.dims()[0]
            self.Dimnames = tuple(Dimnames)
            return
        A = as_dgCMatrix(A)
        self.nrow = A.nrow
        self.Dimnames = A.Dimnames
        self.ctx = Context(device)
        try:
            self.ctx.upload(A, None)
        except Exception:
            self.ctx.close()
            raise

    def close(self):
        if not self._adopted:
            self.ctx.close()

    def _run(self, w, run, verbose, ard, *args):
        wb = _w_in(w, self.nrow)
        self.ctx.fit_init(wb.shape[1], wb)
        out = run(*args, log=_verbose_log(verbose, ard))
        out.w, out.d, out.h = self.ctx.get_factors()
        return out.result()

    def c_ard_nmf(self, tol, maxit, verbose, L1, L2, threads, w, seed, inv_density, overfit_threshold, trace_test_mse):
        return self._run(w, self.ctx._ard_run, verbose, True, float(tol), int(maxit), L1, L2, int(seed), int(inv_density),
                         float(overfit_threshold), int(trace_test_mse))

    def c_nmf(self, tol, maxit, verbose, L1_w, L1_h, L2_w, L2_h, threads, w):
        return self._run(w, self.ctx._nmf_run, verbose, False, float(tol), int(maxit), L1_w, L1_h, L2_w, L2_h)


_ONE_SHOT = {"sparse": ("c_ard_nmf", "c_nmf"), "list": ("c_ard_nmf_sparse_list", "c_nmf_sparse_list"),
             "dense": ("c_ard_nmf_dense", "c_nmf_dense")}


class _OneShotFits(_Fits):
    """The same interface through the one-shot entry points of one branch of _classify_input (every call uploads A again):
      "sparse"  a dgCMatrix: c_ard_nmf / c_nmf;
      "list"    R's list branch (R/ard_nmf.R:45-76, 109-110, 176-178; R/cross_validate_nmf.R:27-50, 76-77): column chunks
                (dgCMatrix, same rows) through c_ard_nmf_sparse_list / c_nmf_sparse_list.  R builds a "distributed
                transpose" At on the host first (a list of row-block transposes); here At_ = None: the library joins the
                chunks into one resident matrix with 64-bit column pointers and builds t(A) on the device;
      "dense"   R's dense branch (class(A)[[1]] == "matrix": R/ard_nmf.R:79-86, 105-106, 172-173): c_ard_nmf_dense /
                c_nmf_dense (every column is solved, all-zero ones included: src/singlet.cpp:370-381).
    The entry points are looked up by name in this module when a fit is made, not when this object is."""

    def __init__(self, kind, A):
        self.A = A
        self.ard, self.nmf = _ONE_SHOT[kind]

    def c_ard_nmf(self, *args):
        return globals()[self.ard](self.A, None, *args)

    def c_nmf(self, tol, maxit, verbose, L1_w, L1_h, L2_w, L2_h, threads, w):
        if self.nmf == "c_nmf_sparse_list":
            # c_nmf_sparse_list(A, At, tol, maxit, verbose > 2, L1, L2, threads, w_init_this)   R/ard_nmf.R:178
            return globals()[self.nmf](self.A, None, tol, maxit, verbose, L1_w, L2_w, threads, w)
        # R/ard_nmf.R:173 calls c_nmf_dense(A, At, tol, maxit, verbose > 2, L1, L2, threads, w_init_this): nine arguments
        # for an eleven-argument wrapper (R/RcppExports.R: L1_w, L1_h, L2_w, L2_h) -- an error in R; mirrored as the call
        # the sparse branch makes (L1, L1, L2, L2), the only reading under which the dense branch returns a model
        return globals()[self.nmf](self.A, None, tol, maxit, verbose, L1_w, L1_h, L2_w, L2_h, threads, w)


def _classify_input(A):
    """-> ("list", chunks) | ("dense", array) | ("sparse", dgCMatrix): the three branches of R/ard_nmf.R:45-90 and
    R/cross_validate_nmf.R:27-63 (`"list" %in% class(A)`, `class(A)[[1]] == "matrix"`, everything else -> dgCMatrix)."""
    if isinstance(A, (list, tuple)):
        chunks = [as_dgCMatrix(a) for a in A]   # "you must provide a list of all 'dgCMatrix' objects"
        if not chunks:
            raise ValueError("A is an empty list")
        if len({c.nrow for c in chunks}) != 1:
            raise ValueError("number of rows in all provided 'A' matrices are not identical")
        rn0 = chunks[0].Dimnames[0]
        if rn0 is not None and any(c.Dimnames[0] is not None and list(c.Dimnames[0]) != list(rn0) for c in chunks[1:]):
            raise ValueError("rownames of all dgCMatrix objects in list must be identical")
        return "list", chunks
    if isinstance(A, np.ndarray) and A.ndim == 2:
        return "dense", A
    return "sparse", as_dgCMatrix(A)


class CVData(list):
    """cv_data rows: dicts with k, rep, test_error, iter, tol (+ overfit_score from ard_nmf);
    the column sets match R/ard_nmf.R:93,118 and R/cross_validate_nmf.R:90."""

    def columns(self):
        return list(self[0].keys()) if self else []

    def column(self, name):
        return [r[name] for r in self]


def GetBestRank(df, tol_overfit=1e-4):
    """R/GetBestRank.R:8-46, line for line."""
    df = list(df)
    best_ranks = []
    for replicate in sorted({r["rep"] for r in df}):
        df_rep = [r for r in df if r["rep"] == replicate]
        max_rank = max(r["k"] for r in df_rep) + 1
        seen = []
        for r in df_rep:
            if r["k"] not in seen:
                seen.append(r["k"])
        for rank in seen:
            if rank < max_rank:
                te = [r["test_error"] for r in df_rep if r["k"] == rank]
                if len(te) > 1:
                    v2 = te[1:]
                    v1 = te[:-1]
                    if len(v1) >= 2:
                        for pos in range(1, len(v1)):
                            if v1[pos] > v1[pos - 1]:
                                v1[pos] = v1[pos - 1]
                    if max([0.0] + [(b - a) / (b + a) for a, b in zip(v1, v2)]) > tol_overfit:
                        max_rank = rank
        df_rep = [r for r in df_rep if r["k"] < max_rank]
        if len(df_rep) == 0:
            best_ranks.append(2)
        elif len(df) == 1:
            best_ranks.append(df_rep[0]["k"])
        else:
            # group_by(rep, k) %>% slice(which.max(iter)): groups come out sorted by k
            last = {}
            for r in df_rep:
                cur = last.get(r["k"])
                if cur is None or r["iter"] > cur["iter"]:
                    last[r["k"]] = r
            rows = [last[kk] for kk in sorted(last)]
            errs = [r["test_error"] for r in rows]
            best_ranks.append(rows[errs.index(min(errs))]["k"])
    return int(math.floor(sum(best_ranks) / len(best_ranks)))


def ard_nmf(A, k_init=2, k_max=100, k_min=2, n_replicates=1, tol=1e-5, cv_tol=1e-4, maxit=100, verbose=1, L1=0.01,
            L2=0, threads=0, test_density=0.05, learning_rate=1, tol_overfit=1e-3, trace_test_mse=1, seed=None,
            resident=True, _fits=None):
    """R/ard_nmf.R:31-193: automatic rank search, then the final fit -- all three input branches: one dgCMatrix
    (:82-85), a list of dgCMatrix column chunks (:45-76 -> c_*_sparse_list), a dense matrix (:79-86 -> c_*_dense).
    resident = True keeps a single dgCMatrix in HBM across all fits of the search (False, and always for the list and
    dense branches: one-shot calls, as the R code makes them)."""
    if not L1 < 1:
        raise ValueError("L1 penalty must be strictly in the range (0, 1]")
    if k_init is None or (isinstance(k_init, float) and math.isnan(k_init)) or k_init < k_min:
        k_init = k_min
    if k_min < 2:
        raise ValueError("k_min cannot be less than 2")
    if _fits is None and isinstance(A, NativeMatrix):   # native(): staged through the typed door, then the resident way
        return _on_native(A, lambda ctx, fits: ard_nmf(None, k_init, k_max, k_min, n_replicates, tol, cv_tol, maxit, verbose, L1, L2,
                                                       threads, test_density, learning_rate, tol_overfit, trace_test_mse, seed,
                                                       resident, _fits=fits))
    kind, A = ("staged", None) if _fits is not None else _classify_input(A)
    if kind == "staged":   # RunNMF: the matrix is staged and resident already
        nrow, (rn, cn), fits = _fits.nrow, _fits.Dimnames, _fits
    elif kind == "list":
        nrow = A[0].nrow
        rn = A[0].Dimnames[0]
        cns = [c.Dimnames[1] for c in A]
        cn = None if any(c is None for c in cns) else [name for c in cns for name in c]   # rownames(At[[1]]): all cells
        fits = _OneShotFits(kind, A)
    elif kind == "dense":
        nrow, rn, cn = A.shape[0], None, None
        fits = _OneShotFits(kind, A)
    else:
        nrow, (rn, cn) = A.nrow, A.Dimnames
        fits = _ResidentFits(A) if resident else _OneShotFits(kind, A)
    if verbose > 0:
        print("running with dense optimization" if kind == "dense" else "running with sparse optimization")
    rng = _rng(seed)
    # w_init <- lapply(1:n_replicates, function(x) matrix(runif(nrow(A) * k_max), k_max, nrow(A)))
    w_init = [rng.random((nrow, k_max)).T for _ in range(n_replicates)]
    test_seed = int(rng.integers(1, 2 ** 31 - 1))  # abs(.Random.seed[[3]])
    inv_density = int(round(1 / test_density))
    df = CVData()
    try:
        return _ard_nmf_search(fits, (rn, cn), df, w_init, test_seed, inv_density, k_init, k_max, k_min, n_replicates, tol, cv_tol,
                               maxit, verbose, L1, L2, threads, learning_rate, tol_overfit, trace_test_mse)
    finally:
        fits.close()   # (an adopted context stays open: _ResidentFits.close)


def _ard_nmf_search(fits, dimnames, df, w_init, test_seed, inv_density, k_init, k_max, k_min, n_replicates, tol, cv_tol, maxit,
                    verbose, L1, L2, threads, learning_rate, tol_overfit, trace_test_mse):
    for curr_rep in range(1, n_replicates + 1):
        if verbose >= 1 and n_replicates > 1:
            print("\nREPLICATE ", curr_rep, "/", n_replicates)
        step_size = 1.0
        curr_rank = k_init
        while step_size >= 1 and curr_rank <= k_max and curr_rank >= k_min:
            if verbose > 0:
                print("k =", curr_rank, ", rep =", curr_rep)
            w_init_this = w_init[curr_rep - 1][:curr_rank, :]
            model = fits.c_ard_nmf(cv_tol, maxit, verbose > 2, L1, L2, threads, w_init_this, test_seed + curr_rep,
                                   inv_density, tol_overfit, trace_test_mse)
            overfit_score = float(model["score_overfit"][-1])
            for q in range(len(model["test_mse"])):
                df.append({"k": int(curr_rank), "rep": int(curr_rep), "test_error": float(model["test_mse"][q]),
                           "iter": int(model["iter"][q]), "tol": float(model["tol"][q]),
                           "overfit_score": overfit_score})
            if overfit_score >= tol_overfit:
                k_max = curr_rank
            df_rep = sorted([r for r in df if r["rep"] == curr_rep], key=lambda r: r["k"])
            best_rank = GetBestRank([r for r in df_rep if r["k"] < k_max])
            ks = sorted({r["k"] for r in df_rep})
            if best_rank not in ks:
                raise RuntimeError("argument is of length zero")  # what R's `if (rank_ind == ...)` does here
            rank_ind = ks.index(best_rank) + 1
            if rank_ind == len(ks):
                step_size = step_size * (1 + learning_rate)
                curr_rank = best_rank + int(math.floor(step_size))
            elif rank_ind == 1:
                if math.floor(step_size) < best_rank:
                    curr_rank = best_rank - int(math.floor(step_size))
                    step_size = step_size * (learning_rate + 1)
                else:
                    curr_rank = best_rank // 2
            else:
                next_lower_rank = ks[rank_ind - 2]
                next_higher_rank = ks[rank_ind]
                diff_lower = best_rank - next_lower_rank
                diff_higher = next_higher_rank - best_rank
                higher_option = best_rank + diff_higher // 2
                lower_option = best_rank - diff_lower // 2
                if diff_lower <= 1 and diff_higher <= 1:
                    break
                elif diff_lower >= diff_higher:
                    curr_rank = lower_option
                else:
                    curr_rank = higher_option
    best_rank = GetBestRank(df, tol_overfit)
    if verbose > 0:
        print("\nFitting final model at k =", best_rank)
    w_init_this = w_init[0][:best_rank, :]
    model = fits.c_nmf(tol, maxit, verbose > 2, L1, L1, L2, L2, threads, w_init_this)
    model["cv_data"] = df
    return _sort_model(model, dimnames[0], dimnames[1])


def _replica_devices(devices):
    """devices of the replica sweep: an explicit list, a count, or SINGLET_REPLICA_GPUS=N from the environment
    (None / unset: device 0 only)."""
    if devices is None:
        n = int(os.environ.get("SINGLET_REPLICA_GPUS", "1") or "1")
        return list(range(max(n, 1)))
    if isinstance(devices, (int, np.integer)):
        return list(range(max(int(devices), 1)))
    return [int(d) for d in devices]


def _run_grid_on_replicas(A, devices, jobs, run):
    """SURVEY.md 8(e) "rank-sweep alternative": the (rank, replicate) fits of a grid are independent, so every
    device keeps its OWN resident copy of A and pulls fits from a shared queue (largest rank first: the cost of a
    masked fit grows like k^2) -- no communication at all.  One host thread per device (the library calls release
    the GIL; a context is only ever used by its own thread).  jobs: list of argument tuples; run(fits, job) -> result.
    Results come back in job order and do not depend on which device ran which fit."""
    import threading
    order = sorted(range(len(jobs)), key=lambda q: -jobs[q][0])
    lock = threading.Lock()
    results = [None] * len(jobs)
    errors = []

    def worker(dev):
        try:
            with _ResidentFits(A, dev) as fits:
                while True:
                    with lock:
                        if errors or not order:
                            return
                        q = order.pop(0)
                    results[q] = run(fits, jobs[q])
        except BaseException as e:  # noqa: BLE001 -- re-raised on the calling thread
            with lock:
                errors.append(e)

    threads = [threading.Thread(target=worker, args=(d,), name="singlet-replica-%d" % i) for i, d in enumerate(devices)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return results


def cross_validate_nmf(A, ranks, n_replicates=3, tol=1e-4, maxit=100, verbose=1, L1=0.01, L2=0, threads=0,
                       test_density=0.05, tol_overfit=1e-4, trace_test_mse=5, seed=None, resident=True, devices=None,
                       _fits=None):
    """R/cross_validate_nmf.R:18-105 -> cv table with k, rep, test_error, iter, tol; one dgCMatrix, a list of dgCMatrix
    column chunks (:27-50 -> c_ard_nmf_sparse_list) or a dense matrix (:57-60 -> c_ard_nmf_dense).
    resident = True keeps a single dgCMatrix in HBM across the whole (rank, replicate) grid.  devices (a list, a count, or
    SINGLET_REPLICA_GPUS=N): deal the independent fits of the grid out over several GPUs, each with its own
    resident copy of A (BASELINE config 5 on one node); the table is the one-device table, row for row."""
    if L1 >= 1:
        raise ValueError("L1 penalty must be strictly in the range (0, 1]")
    if _fits is None and isinstance(A, NativeMatrix):   # native(): one staged context (no replica sweep over `devices`)
        return _on_native(A, lambda ctx, fits: cross_validate_nmf(None, ranks, n_replicates, tol, maxit, verbose, L1, L2, threads,
                                                                  test_density, tol_overfit, trace_test_mse, seed, resident, devices,
                                                                  _fits=fits))
    if _fits is not None:   # RunNMF: the matrix is staged and resident already (A is not read)
        kind, nrow = "sparse", _fits.nrow
    else:
        kind, A = _classify_input(A)
        nrow = A[0].nrow if kind == "list" else (A.shape[0] if kind == "dense" else A.nrow)
    ranks = [int(r) for r in np.atleast_1d(ranks)]
    rng = _rng(seed)
    w_init = [rng.random((nrow, max(ranks))).T for _ in range(n_replicates)]
    seeds = [int(rng.integers(1, 2 ** 31 - 1)) for _ in range(n_replicates)]  # abs(.Random.seed[[3 + rep]])
    inv_density = int(round(1 / test_density))
    df2 = CVData()
    grid = [(k, rep) for rep in range(1, n_replicates + 1) for k in ranks]  # expand.grid(k = ranks, rep = 1:n)

    def fit(fits, job):
        k, rep = job
        return fits.c_ard_nmf(tol, maxit, verbose > 1, L1, L2, threads, w_init[rep - 1][:k, :], seeds[rep - 1],
                              inv_density, tol_overfit, trace_test_mse)

    def rows(k, rep, model):
        for t in range(len(model["test_mse"])):
            df2.append({"k": k, "rep": rep, "test_error": float(model["test_mse"][t]), "iter": int(model["iter"][t]),
                        "tol": float(model["tol"][t])})

    devs = _replica_devices(devices)
    if kind != "sparse":
        fits = _OneShotFits(kind, A)
        for k, rep in grid:
            rows(k, rep, fit(fits, (k, rep)))
        return df2
    if _fits is None and resident and len(devs) > 1:
        for (k, rep), model in zip(grid, _run_grid_on_replicas(A, devs, grid, fit)):
            rows(k, rep, model)
        return df2
    fits = _fits if _fits is not None else (_ResidentFits(A, devs[0]) if resident else _OneShotFits(kind, A))
    try:
        for q, (k, rep) in enumerate(grid):
            if verbose > 1:
                print("k = %d, rep = %d (%d/%d):" % (k, rep, q + 1, len(grid)))
            model = fit(fits, (k, rep))
            rows(k, rep, model)
            if verbose > 1:
                print("test set error: %#.4e\n" % model["test_mse"][-1])
                if model["test_mse"][-1] / model["test_mse"][0] > (1 + tol_overfit):
                    print("overfitting detected, lower rank recommended")
    finally:
        fits.close()
    return df2


def RunNMF(A, k=None, features=None, split_by=None, reps=3, tol=1e-5, L1=0.01, L2=0, verbose=2, maxit=100, test_density=0.05,
           learning_rate=0.8, tol_overfit=1e-4, trace_test_mse=5, threads=0, seed=None, nfeatures=None):
    """The matrix steps of RunNMF.Seurat (R/RunNMF.R:61-151) on a genes x cells matrix, without the Seurat object, on ONE
    resident context -- the matrix is uploaded once and never comes back between the steps:
      1. LogNormalize when every value is integral (sum(as.integer(v)) == sum(v), l.66-69);
      2. A <- A[features, ] (l.72-81): `features` as subset() takes rows -- 0-based integers, names or a mask; the
         "var.features" of a Seurat object are the caller's to pass -- or `nfeatures` selects them here: the vst selection
         (Context.variable_features) runs on the resident COUNTS right after the upload, before step 1, and its genes, in
         rank order, are the rows of this step; the model then carries them as "var_features" (names, or indices when A
         has no row names).  Counts only: a matrix that is not integral is refused, and so is `features` next to it;
      3. weight_by_split when `split_by` (one label per cell, any type) is given (l.86-97);
      4. k a vector: cross_validate_nmf at tol * 10, GetBestRank, the final run_nmf (l.101-125); k None: ard_nmf with
         k_max = 1e4 (l.126-145), clipped to the library's rank limit of 1024; k a scalar: run_nmf (l.146-148).
    `seed` (an int or numpy Generator) replaces R's global RNG state: one stream, drawn from by the drivers in the order
    they run, each exactly as it draws for a matrix of the subset's shape.  Returns the model of the driver it
    dispatched to (w m x k, d, h k x n, names) plus "cv_data" (empty for a scalar k).
    A NativeMatrix (native()) is staged through the typed door; step 1 then takes its decision from the upload's report
    (`integral`: every stored value equals its truncation, found while the values are converted on the device) instead
    of scanning a host array -- for non-negative values that is the reference's sum(as.integer(v)) == sum(v)."""
    from .context import Context
    is_native = isinstance(A, NativeMatrix)
    if not is_native:
        A = as_dgCMatrix(A)
    rn, cn = A.Dimnames
    rows = None
    if nfeatures is not None:
        if features is not None:
            raise ValueError("pass either features or nfeatures (the variable features selected here), not both")
        if isinstance(nfeatures, bool) or int(nfeatures) != nfeatures or int(nfeatures) < 1:
            raise ValueError("nfeatures must be a whole number of at least 1")
        nfeatures = int(nfeatures)
    if features is not None:
        if isinstance(features, str):
            if features == "var.features":
                raise ValueError("features = 'var.features' reads a Seurat object's variable features: pass them as names or indices")
            features = [features]
        rows = _subset_index(features, A.nrow, rn, "features")
    sb = None
    if split_by is not None:
        sb = np.asarray(split_by)
        if sb.shape != (A.ncol,):
            raise ValueError("split_by needs one entry per column of A")
        groups = np.unique(sb)
        sb = np.searchsorted(groups, sb).astype(np.int32)   # as.integer(as.numeric(as.factor(.))) - 1
    scalar_k = k is not None and np.ndim(k) == 0
    if k is not None and not scalar_k and np.size(k) < 1:
        raise ValueError("value for 'k' was invalid")
    rng = _rng(seed)
    ctx = Context(0)
    try:
        if is_native:
            integral = bool(ctx.upload_native(A)["integral"])
        else:
            ctx.upload(A, None)
            v = A.x
            integral = np.sum(np.trunc(v)) == np.sum(v)   # sum(as.integer(v)) == sum(v)
        var_features = None
        if nfeatures is not None:
            if not integral:
                raise ValueError("variable features are selected on counts: A is not integral (select them elsewhere and pass features)")
            rows = ctx.variable_features(nfeatures)["features"]
            var_features = _subset_names(rn, rows) if rn is not None else rows
        if integral:
            ctx.log_normalize()
        if rows is not None:
            ctx.subset(rows=rows)
            rn = _subset_names(rn, rows)
        if sb is not None:
            ctx.weight_by_split(sb, int(groups.size))
        fits = _ResidentFits(None, ctx=ctx, Dimnames=(rn, cn))
        if k is not None and not scalar_k and np.size(k) > 1:
            cv_data = cross_validate_nmf(None, k, n_replicates=reps, tol=tol * 10, maxit=maxit, verbose=verbose, L1=L1, L2=L2,
                                         threads=threads, test_density=test_density, tol_overfit=tol_overfit,
                                         trace_test_mse=trace_test_mse, seed=rng, _fits=fits)
            best_rank = GetBestRank(cv_data, tol_overfit)
            if verbose >= 1:
                print("best rank: ", best_rank)
                print("\nfitting final model:")
            model = run_nmf(None, best_rank, tol, maxit, verbose > 1, L1, L2, threads, seed=rng, _fits=fits)
        elif k is None:
            k_max = 10000
            if k_max > 1024:
                if verbose >= 1:
                    print("k_max = 1e4 is above the library's rank limit: searching up to k = 1024")
                k_max = 1024
            model = ard_nmf(None, k_init=None, k_max=k_max, k_min=2, n_replicates=reps, tol=tol, maxit=maxit, verbose=verbose,
                            L1=L1, L2=L2, threads=threads, test_density=test_density, learning_rate=learning_rate,
                            tol_overfit=tol_overfit, trace_test_mse=trace_test_mse, seed=rng, _fits=fits)
            cv_data = model["cv_data"]
        else:
            rank = int(k if scalar_k else np.ravel(k)[0])
            model = run_nmf(None, rank, tol, maxit, verbose > 1, L1, L2, threads, seed=rng, _fits=fits)
            cv_data = CVData()
    finally:
        ctx.close()
    model["cv_data"] = cv_data
    if var_features is not None:
        model["var_features"] = var_features
    return model


# ---------------------------------------------------------------------------
# Variable features
# ---------------------------------------------------------------------------
def find_variable_features(A, nfeatures=2000, span=0.3, vmax=None, expected_var=None):
    """Seurat::FindVariableFeatures(selection.method = "vst") on a genes x cells COUNT matrix, on the device
    (sgl_c_variable_features; the rules are stated in include/singlet_hip.h, sgl_variable_features): {"features" (int32 gene
    indices, 0-based, in rank order: the rows of A[var.features, ]), "mean", "variance", "variance_expected",
    "variance_standardized"} plus "names" (the selected row names) when A has row names.  A: a dgCMatrix, anything
    as_dgCMatrix accepts, or a native(...) object, which is staged through the typed door.  vmax None: sqrt(ncol).
    expected_var: one expected variance per gene, used in place of the trend -- the trend here is an exact local fit at
    every gene, not R's interpolated loess; with R's fitted values passed in, everything else agrees with Seurat's rules."""
    from .context import _variable_features_call
    is_native = isinstance(A, NativeMatrix)
    if not is_native:
        A = as_dgCMatrix(A)
    if is_native:
        out = _on_native(A, lambda ctx, fits: ctx.variable_features(nfeatures, span, vmax, expected_var))
    else:
        L = _lib.load()
        out = _variable_features_call(lambda *a: L.sgl_c_variable_features(*csc_ptrs(A), A.nrow, A.ncol, *a), A.nrow, nfeatures, span,
                                      vmax, expected_var)
    rn = A.Dimnames[0]
    if rn is not None:
        out["names"] = _subset_names(rn, out["features"])
    return out


# ---------------------------------------------------------------------------
# Model error
# ---------------------------------------------------------------------------
def evaluate(A, model, cell_loss=False, gene_loss=False):
    """Error of a model against the matrix it explains: {"sse", "mse"} and, when asked for, "cell_loss" (one per column of A)
    and "gene_loss" (one per row) -- the sums of squared residuals of w diag(d) h over every entry, zeros included, formed on
    the device from the sparse structure (sgl_c_evaluate; include/singlet_hip.h, sgl_evaluate).  A: whatever run_nmf
    takes -- a dgCMatrix, anything as_dgCMatrix accepts, or a native(...) object, which is staged through the typed door.
    model: what the drivers return (w m x k, d k, h k x n).  Shapes are checked before anything is uploaded."""
    is_native = isinstance(A, NativeMatrix)
    if not is_native:
        A = as_dgCMatrix(A)
    w = np.asarray(model["w"], dtype=np.float64)
    d = np.asarray(model["d"], dtype=np.float64).reshape(-1)
    h = np.asarray(model["h"], dtype=np.float64)
    if w.ndim != 2 or h.ndim != 2:
        raise ValueError("evaluate: model['w'] must be m x k and model['h'] k x n")
    k = w.shape[1]
    if w.shape[0] != A.nrow or h.shape[1] != A.ncol or h.shape[0] != k or d.shape[0] != k:
        raise ValueError("evaluate: A is %d x %d, but w is %r, d %r and h %r (expected m x k, k, k x n)"
                         % (A.nrow, A.ncol, w.shape, d.shape, h.shape))
    if k < 1:
        raise ValueError("evaluate: the model has rank 0")
    wk = np.ascontiguousarray(w)        # m x k row-major = k x m column-major, the layout of sgl_set_factors
    hk = np.ascontiguousarray(h.T)
    dk = np.ascontiguousarray(d)
    from .context import _evaluate_call
    if is_native:
        def body(ctx, fits):
            ctx.fit_init(k)
            ctx.set_factors(wk, dk, hk)
            return ctx.evaluate(cell_loss, gene_loss)
        return _on_native(A, body)
    L = _lib.load()
    return _evaluate_call(lambda *o: L.sgl_c_evaluate(*csc_ptrs(A), A.nrow, A.ncol, ptr(wk, f64p), ptr(dk, f64p), ptr(hk, f64p),
                                                      int(k), *o), A.nrow, A.ncol, cell_loss, gene_loss)


# ---------------------------------------------------------------------------
# Linked NMF (R/RunLNMF.R, R/MetadataSummary.R, R/GetSharedFactors.R, R/GetUniqueFactors.R)
# ---------------------------------------------------------------------------
def group_means(F, group, n_groups):
    """(means, counts) of the columns of F (k x n, one column per cell) per group: means[f, g] = mean(F[f, which(group == g)])
    as k x n_groups, counts[g] the cells of group g (sgl_c_group_means, on the device).  group holds one 0-based id per
    column; an empty group gives a NaN column (R's mean(numeric(0))) and a count of 0.  The summation order depends on
    (n, group, n_groups) alone."""
    from .context import _group_list, _group_means_call
    buf = colmajor(F, "F must be a k x n matrix")
    n, k = buf.shape
    g = _group_list(group, n, "group")
    return _group_means_call(lambda *o: _lib.load().sgl_c_group_means(ptr(buf, f64p), int(k), int(n), *o), g, n_groups, k)


def _shares(means):
    """apply(m, 1, function(x) x / sum(x)), kept k x G: every factor's group means divided by their sum (added in group
    order).  A factor whose means are all zero gives a NaN row."""
    m = np.asarray(means, dtype=np.float64)
    if m.ndim != 2 or m.shape[1] < 1:
        raise ValueError("means must be a k x G matrix with at least one group")
    total = np.zeros(m.shape[0])
    for g in range(m.shape[1]):
        total = total + m[:, g]
    with np.errstate(invalid="ignore", divide="ignore"):
        return m / total[:, None]


def _share_table(means):
    """t(apply(m, 1, function(x) x / sum(x))) * length(levels) of R/RunLNMF.R:143 for the k x G table of group means."""
    s = _shares(means)
    return s * s.shape[1]


def _link_table(means, link_cutoff):
    """The k x G link table of R/RunLNMF.R:143-154: 0 where a group's share of a factor (_share_table) is below link_cutoff
    (strictly: a share equal to the cut-off stays linked), 1 elsewhere.  A NaN share raises, naming the factor: R stops
    there too, at `if (NA)` (l.149)."""
    share = _share_table(means)
    bad = np.flatnonzero(np.isnan(share).any(axis=1))
    if bad.size:
        raise ValueError("factor %d (0-based; factor %d of the reference) has no defined share of the groups (its group means "
                         "are all zero or not finite): the reference stops at `if (NA)` (R/RunLNMF.R:149)"
                         % (int(bad[0]), int(bad[0]) + 1))
    return 1.0 - (share < float(link_cutoff)).astype(np.float64)


def _dim2(x):
    return tuple(np.shape(x)) if np.ndim(x) == 2 else None


def _linked_checks(nrow_A, ncol_A, w_shape, link_h_shape, link_w_shape, L1):
    """The stop()s of run_linked_nmf (R/RunLNMF.R:19-53), in its order, with its messages (a shape is (rows, cols) or None)."""
    if link_h_shape is None and link_w_shape is None:
        raise ValueError("both link_h and link_w cannot be NULL. Specify at least one linking matrix.")
    if link_h_shape is not None and link_h_shape[0] != w_shape[1]:
        raise ValueError("number of rows in 'link_h' must be equal to the nubmer of columns in 'w'")
    if link_h_shape is not None and link_h_shape[1] != ncol_A:
        raise ValueError("number of columns in 'link_h' must be equal to the number of columns in 'A'")
    if link_w_shape is not None and link_w_shape[1] != w_shape[1]:
        raise ValueError("number of columns in 'link_w' must be equal to the nubmer of columns in 'w'")
    if link_w_shape is not None and link_w_shape[0] != nrow_A:
        raise ValueError("number of rows in 'link_w' must be equal to the number of rows in 'A'")
    if L1 >= 1:
        raise ValueError("L1 penalty must be strictly in the range (0, 1]")
    if w_shape[0] != nrow_A:
        raise ValueError("number of rows in 'w' must be equal to the number of rows in 'A'")


def _sort_linked(model):
    # sort_index <- order(model$d, decreasing = TRUE)   R/RunLNMF.R:61-64, as _sort_model
    idx = np.argsort(-model["d"], kind="stable")
    model["d"] = model["d"][idx]
    model["w"] = model["w"].T[:, idx]
    model["h"] = model["h"][idx, :]
    return idx


def run_linked_nmf(A, w, link_h=None, link_w=None, tol=1e-4, maxit=100, verbose=True, L1=0.01, L2=0, threads=0):
    """R/RunLNMF.R:18-66: linked NMF from an initial w (m x k).  link_h is k x n, link_w m x k, as the reference documents
    them.  The same checks in the same order (ValueError with the reference's messages), then c_linked_nmf on t(w) and the
    sort by d.  As in the reference, link_w reaches c_linked_nmf as it is, m x k, and is used only when its column count
    equals nrow(A) (src/singlet.cpp:1065), that is for k == m.  Returns w m x k, d, h k x n (plus "iter" / "tol")."""
    shp = getattr(A, "shape", None) or (A.nrow, A.ncol)
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError("w must be a matrix")
    for name, Lk in (("link_h", link_h), ("link_w", link_w)):
        if Lk is not None and np.ndim(Lk) != 2:
            raise ValueError("%s must be a matrix" % name)
    _linked_checks(int(shp[0]), int(shp[1]), w.shape, None if link_h is None else _dim2(link_h),
                   None if link_w is None else _dim2(link_w), L1)
    if link_h is None:
        link_h = np.zeros((1, 1))
    if link_w is None:
        link_w = np.zeros((1, 1))
    A = as_dgCMatrix(A)
    model = c_linked_nmf(A, None, tol, maxit, verbose, L1, L2, threads, w.T, link_h, link_w)
    _sort_linked(model)
    return model


def RunLNMF(A, model, split_by, link_cutoff=0.5, tol=1e-5, maxit=100, L1=0.01, L2=0, verbose=True, threads=0):
    """The matrix steps of RunLNMF.Seurat (R/RunLNMF.R:111-159) without the Seurat object, on ONE resident context: A is the
    assay's @data (the normalised genes x cells matrix), model what run_nmf / RunNMF returned (w m x k, h k x n), split_by one
    label per cell (any type).
      1. split_by -> as.factor codes (l.120), as RunNMF makes them; A uploaded once; weight_by_split (l.125);
      2. the k x G group means of model["h"] on the device (l.136-142: sgl_group_means);
      3. the share table m / rowSums(m) * G < link_cutoff (l.143) and the link table 1 - unlinked (l.146-154), k x G;
      4. fit_init(k, t(w)), the link set in its grouped form (the k x n matrix of l.146 is never built: column c of it is
         column codes[c] of the table), nmf_run(tol, maxit, L1, L1, L2, L2) -- what run_linked_nmf -> c_linked_nmf does
         (l.159), the same bits as with the expanded matrix;
      5. sort by d (l.61-64), factor names LNMF_i (l.164).
    link_w: the reference passes matrix(1, m, k) (l.157); c_linked_nmf ignores it unless k == m (src/singlet.cpp:1065), and
    then it multiplies by one -- no W-side link is set.
    Returns w m x k, d, h k x n, "iter", "tol", the names, and
      "link_table"    k x G, rows in the order of the INPUT factors -- the reference's misc$link_matrix (l.174) is not
                      re-sorted with the model either; the dense link matrix is link_table[:, codes];
      "levels"        the group levels (sorted unique labels; codes index them);
      "factor_order"  the sort index: output factor i is input factor factor_order[i].
    Refused (ValueError): a missing split_by, one of length nrow(A) -- the reference's transposed branch (l.121-123,
    161-163) hands t(A) to run_linked_nmf, whose own nrow(w) check (l.51) it cannot pass --, any other wrong length, the
    stop()s of run_linked_nmf, and a factor whose share row is NaN (all group means zero), where R stops at `if (NA)`."""
    from .context import Context
    A = as_dgCMatrix(A)
    rn, cn = A.Dimnames
    if split_by is None:
        raise ValueError("no value specified for 'split.by'")
    sb = np.asarray(split_by)
    if sb.ndim != 1:
        raise ValueError("split_by must be a vector")
    if sb.shape[0] == A.nrow:
        raise ValueError("split_by has one entry per ROW of A: the reference then factorises t(A) (R/RunLNMF.R:121-123), which its own "
                         "check of nrow(w) (l.51) refuses; pass one label per cell (column)")
    if sb.shape[0] != A.ncol:
        raise ValueError("length of 'split.by' was not equal to one of the dimensions of the input matrix")
    w = np.asarray(model["w"], dtype=np.float64)
    h = np.asarray(model["h"], dtype=np.float64)
    if w.ndim != 2 or h.ndim != 2:
        raise ValueError("model['w'] must be m x k and model['h'] k x n")
    # link_h <- matrix(1, ncol(h), nrow(h)) with h the n x k cell embeddings: its shape is that of model["h"]
    _linked_checks(A.nrow, A.ncol, w.shape, h.shape, (w.shape[0], w.shape[1]), L1)
    k = w.shape[1]
    levels = np.unique(sb)
    codes = np.searchsorted(levels, sb).astype(np.int32)   # as.integer(as.numeric(as.factor(.))) - 1
    G = int(levels.size)
    ctx = Context(0)
    try:
        ctx.upload(A, None)
        ctx.weight_by_split(codes, G)
        means, _ = ctx.group_means(codes, G, F=h)
        table = _link_table(means, link_cutoff)
        ctx.fit_init(k, w)
        ctx.set_links_grouped(table, codes)
        n_iter, tr = ctx.nmf_run(float(tol), int(maxit), L1, L1, L2, L2, log=_verbose_log(verbose))
        W, D, H = ctx.get_factors()
    finally:
        ctx.close()
    out = {"w": W.T, "d": D, "h": H.T, "iter": n_iter, "tol": tr}
    idx = _sort_linked(out)
    out["factor_names"] = ["LNMF_%d" % (q + 1) for q in range(k)]
    out["rownames_w"] = rn
    out["colnames_h"] = cn
    out["link_table"] = table
    out["levels"] = levels
    out["factor_order"] = idx
    return out


def MetadataSummary(h, factor_data):
    """R/MetadataSummary.R:15-36: the share of every group of cells in every factor.  h is k x n, factor_data one label per
    column; levels are the sorted unique labels (as.factor).  The k x G group means come from the device (group_means);
    each factor's means are divided by their sum (l.26).  Returns {"table": G x k, "levels": the row names in row order,
    "factors": the column names factor1 ... factork (l.17)}.  With two levels the rows are ordered by their share of the
    first factor, decreasing (l.27-28).  The hclust reordering of more than two levels (l.29-31) is display order only and is
    not mirrored: rows stay in level order, columns in factor order."""
    h = np.asarray(h, dtype=np.float64)
    fd = np.asarray(factor_data)
    if h.ndim != 2 or fd.shape != (h.shape[1],):
        raise ValueError("h must be k x n and factor_data hold one label per column of h")
    levels = np.unique(fd)
    codes = np.searchsorted(levels, fd).astype(np.int32)
    G = int(levels.size)
    means, _ = group_means(h, codes, G)
    table = _shares(means).T   # G x k: apply(m, 1, function(x) x / sum(x)) returns the transpose
    if G == 2:
        order = np.argsort(-table[:, 0], kind="stable")   # m[order(m[, 1], decreasing = TRUE), ]
        table, levels = table[order], levels[order]
    return {"table": table, "levels": levels, "factors": ["factor%d" % (q + 1) for q in range(h.shape[0])]}


def _unique_mask(h, split_by):
    t = MetadataSummary(h, split_by)["table"]
    with np.errstate(invalid="ignore"):
        return np.min(t, axis=0) == 0   # apply(., 2, function(x) min(x) == 0); NaN compares false, as which() drops NA


def GetUniqueFactors(h, split_by):
    """R/GetUniqueFactors.R:4-10 on a k x n embedding: the 0-based indices of the factors whose smallest share over the groups
    (MetadataSummary) is exactly 0 -- factors some group does not carry at all."""
    return np.flatnonzero(_unique_mask(h, split_by))


def GetSharedFactors(h, split_by):
    """R/GetSharedFactors.R:4-10: the 0-based indices of all other factors.  A factor whose shares are NaN counts as shared,
    as which() drops NA."""
    return np.flatnonzero(~_unique_mask(h, split_by))


# ---------------------------------------------------------------------------
# Spatial neighbour graphs (FindLocalNeighbors / RescaleSpatial)
# ---------------------------------------------------------------------------
def _two_call(fn, n):
    """Run a two-call sgl_c_lknn / sgl_c_snn / sgl_spatial_graph entry: counts first, then the slots."""
    p = np.empty(n + 1, dtype=np.int32)
    nnz = C.c_int64()
    check(fn(ptr(p, i32p), C.byref(nnz), None, None, 0))
    i = np.empty(max(nnz.value, 1), dtype=np.int32)
    x = np.empty(max(nnz.value, 1), dtype=np.float64)
    check(fn(ptr(p, i32p), C.byref(nnz), ptr(i, i32p), ptr(x, f64p), nnz.value))
    return p, i[:nnz.value], x[:nnz.value]


def c_LKNN(m, coord_x, coord_y, k, radius, metric, similarity, max_dist, verbose, threads):
    """.Call(`_singlet_c_LKNN`, ...) -> the n x n local k-nearest-neighbour dgCMatrix (src/singlet.cpp:1491-1603); column j
    holds the neighbours of point j, x their float distances.  Rules where the reference is undefined (ties, NaN distances,
    more neighbours than its slots per point): include/singlet_hip.h, sgl_c_lknn.  `threads` is ignored."""
    L = _lib.load()
    m = np.asarray(m, dtype=np.float64)
    if m.ndim == 1:
        m = m.reshape(-1, 1)
    if m.ndim != 2:
        raise ValueError("m must be a matrix")
    cx = np.ascontiguousarray(coord_x, dtype=np.float64).ravel()
    cy = np.ascontiguousarray(coord_y, dtype=np.float64).ravel()
    m_rows, m_cols = m.shape
    if m_cols != m_rows and m_rows == cx.size:
        m_cols_t = m_rows
    else:
        m_cols_t = m_cols
    if m_cols_t != cx.size:   # l.1493, in the reference's order
        raise _lib.SingletHipError(-1, "number of columns in 'm' must be equal to number of coordinates")
    if cx.size != cy.size:    # l.1494
        raise _lib.SingletHipError(-1, "length of coordinate vectors must be equivalent")
    mf = np.asfortranarray(m)
    n = int(cx.size)
    if verbose:
        base = np.float32(np.float32(radius) * np.float32(2) + np.float32(1))
        n_max_edges = int(math.ceil(float(base) * float(base))) - 1
        print("number of edges per node: %d" % (n_max_edges & 0xffffffff))
        print("filtering %d edges" % (n * n_max_edges))
    p, i, x = _two_call(lambda po, no, io, xo, cap: L.sgl_c_lknn(
        mf.ctypes.data_as(f64p), m_rows, m_cols, ptr(cx, f64p), ptr(cy, f64p), n, int(k), float(radius),
        str(metric).encode(), int(bool(similarity)), float(max_dist), po, no, io, xo, cap), n)
    if verbose:
        print("selected %d edges" % int(p[-1]))
    return dgCMatrix(x, i, p, (n, n))


def c_SNN(G, min_similarity, threads):
    """.Call(`_singlet_c_SNN`, ...) -> the ncol(G) x ncol(G) shared-nearest-neighbour dgCMatrix (src/singlet.cpp:1606-1665):
    the Jaccard index of the row sets of every two columns that share a row, kept when > min_similarity, and 1 on the
    diagonal of every non-empty column.  Only G's pattern is read.  `threads` is ignored."""
    L = _lib.load()
    G = as_dgCMatrix(G)
    n = G.ncol
    p, i, x = _two_call(lambda po, no, io, xo, cap: L.sgl_c_snn(ptr(G.i, i32p), ptr(G.p, i32p), G.nrow, G.ncol,
                                                                float(min_similarity), po, no, io, xo, cap), n)
    return dgCMatrix(x, i, p, (n, n))


def spatial_graph(c1, c2, max_dist, max_k=100, threads=0):
    """spatial_graph(c1, c2, max_dist, max_k, threads) (src/singlet.cpp:1365-1414) -> the n x n dgCMatrix whose column i
    holds, of the points within max_dist of point i (strict), the max_k lowest-numbered ones (i itself included), weighted
    (max_dist - d) * (1 / max_dist) and normalised to sum 1.  The selection is by index, not by distance.  Refusals, the column
    sum's order and what is bit-exact: include/singlet_hip.h, sgl_spatial_graph.  `threads` is ignored."""
    L = _lib.load()
    x = np.ascontiguousarray(c1, dtype=np.float64).ravel()
    y = np.ascontiguousarray(c2, dtype=np.float64).ravel()
    if x.size != y.size:   # the reference reads past the shorter one
        raise _lib.SingletHipError(-1, "spatial_graph: c1 (%d) and c2 (%d) differ in length" % (x.size, y.size))
    if x.size > 2**31 - 1:
        raise _lib.SingletHipError(-1, "spatial_graph: %d points do not fit a dgCMatrix" % x.size)
    n = int(x.size)
    k = min(int(max_k), 2**63 - 1)   # truncates toward zero; above n it acts as n
    p, i, v = _two_call(lambda po, no, io, xo, cap: L.sgl_spatial_graph(ptr(x, f64p), ptr(y, f64p), n, float(max_dist), k,
                                                                          po, no, io, xo, cap), n)
    return dgCMatrix(v, i, p, (n, n))


def rescale_spatial(coords):
    """RescaleSpatial.Seurat (R/RescaleSpatial.R:10-22) on an n x 2 coordinate matrix: each axis shifted to start at 0,
    scaled to [0, 1], divided by the median gap between its sorted unique values, and rounded half to even (R's round)."""
    df = np.array(coords, dtype=np.float64)
    if df.ndim != 2 or df.shape[1] < 2:
        raise ValueError("coords must be an n x 2 matrix")
    for a in (0, 1):
        c = df[:, a] - np.min(df[:, a])
        c = c / np.max(c)
        c = c * 1 / np.median(np.diff(np.sort(np.unique(c))))
        df[:, a] = c
    return np.round(df)


def find_local_neighbors(h, spatial, k_param=20, spatial_radius=4, nn_metric="jaccard", use_dist=False, compute_snn=True,
                         prune_snn=1 / 15, prune_knn=1 / 10, return_dist=False, verbose=False, dims=None, threads=0):
    """The numeric steps of FindLocalNeighbors.Seurat (R/FindLocalNeighbors.R:32-101): `h` is the reduction's embedding,
    cells x factors (as cell.embeddings), `spatial` the n x 2 spatial coordinates; `dims` are 1-based, as in R.
    Returns {"knn": c_LKNN graph (x = 1 unless return_dist), "snn": c_SNN of it or None}.

    The message of l.74 is R's own `stop(..., max(sp[,1], "or", max(sp[,2]), ...))`: its max() swallows the text.  Here it
    reads as intended."""
    sp = np.asarray(spatial, dtype=np.float64)
    if sp.ndim != 2 or sp.shape[1] < 2:
        raise ValueError("spatial must be an n x 2 matrix")
    if np.max(sp[:, 0]) == 1 and np.max(sp[:, 1]) == 1:   # l.64-65 (a warning in R)
        import warnings
        warnings.warn("maximum value in spatial.reduction is 1 in both dimensions. Double-check that your coordinates are "
                      "fixed and on the same scale in both dimensions.")
    hm = np.asarray(h, dtype=np.float64).T   # h <- t(cell.embeddings) (l.67)
    if hm.shape[1] != sp.shape[0]:
        raise ValueError("there were %d samples in reduction but %d samples in spatial reduction" % (hm.shape[1], sp.shape[0]))
    if dims is not None:
        dims = np.atleast_1d(np.asarray(dims, dtype=np.int64))
        if np.max(dims) > hm.shape[0]:
            raise ValueError("you requested up to %d dims but there are only %d dimensions in reduction" % (np.max(dims), hm.shape[0]))
        hm = hm[dims - 1, :]
    if spatial_radius > np.max(sp[:, 0]) or spatial_radius > np.max(sp[:, 1]):
        raise ValueError("your spatial radius of %s is greater than the maximum value of %s or %s in your spatial coordinates "
                         "reduction" % (spatial_radius, np.max(sp[:, 0]), np.max(sp[:, 1])))
    if nn_metric not in ("jaccard", "euclidean", "manhattan", "hamming", "kl", "cosine"):
        raise ValueError("specified nn.metric = %s is not one of c('jaccard', 'euclidean', 'manhattan', 'hamming', 'kl', or "
                         "'cosine')" % nn_metric)
    if use_dist and nn_metric not in ("jaccard", "cosine"):
        raise ValueError("it doesn't make sense to use dissimilarity (use.dist = FALSE) on a distance metric not strictly "
                         "bounded between 0 and 1. Try using 'cosine' or 'jaccard' distance instead.")
    if prune_knn >= 1:
        raise ValueError("prune.knn must be less than 1. You are currently asking to prune everything.")
    if prune_snn >= 1:
        raise ValueError("prune.snn must be less than 1. You are currently asking to prune everything.")
    knn = c_LKNN(hm, sp[:, 0], sp[:, 1], k_param, spatial_radius, nn_metric, not use_dist, prune_knn, verbose, threads)
    if not return_dist:
        knn.x = np.ones_like(knn.x)
    snn = c_SNN(knn, prune_snn, threads) if compute_snn else None
    return {"knn": knn, "snn": snn}


# ---------------------------------------------------------------------------
# Embedding neighbours (Seurat's FindNeighbors on the nmf reduction)
# ---------------------------------------------------------------------------
def knn(reference, query=None, n_neighbors=20, dims=None, metric="euclidean", method="exact", n_lists=None, n_probe=None, n_iter=10):
    """Exact nearest neighbours in an embedding, one-shot (sgl_c_knn): reference k x n, query k x n_query (R's orientation, one
    column per cell; None: the references themselves), dims 0-based rows -> (idx, dist), each n_query x n_neighbors, as
    Context.knn returns them.  The rules -- the sequential FP64 sum, the ranking by (squared distance, index) -- are in
    include/singlet_hip.h, sgl_knn.  metric "cosine" or "correlation" (sgl_c_knn_metric): as Context.knn; the rules are at
    sgl_knn_metric.  method "ivf" (sgl_c_knn_ivf): the approximate inverted-list search with n_lists, n_probe and n_iter as
    Context.knn takes them."""
    code = knn_metric(metric)
    if knn_method(method):
        return knn_call(_lib.load().sgl_c_knn_ivf, reference, query, dims, n_neighbors, metric=code,
                        extra=lambda n_ref, nd: (*knn_ivf_shape(n_ref, n_lists, n_probe), int(n_iter)))
    if code:
        return knn_call(_lib.load().sgl_c_knn_metric, reference, query, dims, n_neighbors, metric=code)
    return knn_call(_lib.load().sgl_c_knn, reference, query, dims, n_neighbors)


def _metric_kw(metric):
    """The keyword a composed call hands on: nothing for the default, so that it makes the very call it made before."""
    return {"metric": metric} if knn_metric(metric) else {}


def _nn_method_kw(nn_method, n_lists, n_probe):
    """The same for the search method: nothing for "exact"."""
    return {"method": nn_method, "n_lists": n_lists, "n_probe": n_probe} if knn_method(nn_method) else {}


def _refuse_short(who, idx):
    """A -1 of a short inverted-list result must not reach c_SNN or the fuzzy graph."""
    short = int((np.asarray(idx) < 0).any(axis=1).sum())
    if short:
        raise ValueError("%s: %d cells came back with fewer neighbours than asked for: the lists their n_probe probes reach hold too few "
                         "cells; raise n_probe (or lower n_lists)" % (who, short))


def find_neighbors(embedding, k_param=20, dims=None, compute_snn=True, prune_snn=1 / 15, return_dist=False, metric="euclidean",
                   nn_method="exact", n_lists=None, n_probe=None):
    """The numeric steps of Seurat's FindNeighbors on a reduction: the exact k.param nearest neighbours of every cell (itself
    included) in the embedding, and the shared-nearest-neighbour graph of them.  `embedding` is cells x factors (as
    cell.embeddings), or a Context with a fit, whose H is searched where it lies, in the fit's stored factor order; `dims`
    are 1-based, as in R.  Returns {"nn", "snn", "idx", "dist"}: idx / dist n x k.param as Context.knn returns them; nn the
    n x n dgCMatrix whose column j holds the neighbours of cell j (rows ascending; x = 1, or the distances with return_dist:
    the self entry is then an explicit 0); snn = c_SNN(nn, nextafter(prune_snn, -inf), 0) or None.  metric: Seurat's
    annoy.metric, "euclidean" (its default and ours), "cosine" or "correlation" as knn takes it; dist is then 1 - cos.
    nn_method "ivf": the approximate inverted-list search of knn (Seurat's own default, annoy, is approximate too) with n_lists
    and n_probe as knn takes them; a cell that comes back with fewer than k.param neighbours raises ValueError naming n_probe.

    Seurat's SNN zeroes the entries below prune.SNN and keeps equality; c_SNN keeps > strictly.  With k.param neighbours in
    every column, inter / (2 k.param - inter) is Seurat's Jaccard index and the diagonal 1 its k.param / k.param, and the
    next double below prune_snn as the strict threshold keeps exactly the entries >= prune_snn."""
    from .context import Context
    mkw = {**_metric_kw(metric), **_nn_method_kw(nn_method, n_lists, n_probe)}
    if prune_snn >= 1:
        raise ValueError("prune.snn must be less than 1. You are currently asking to prune everything.")
    if isinstance(embedding, Context):
        ctx, E = embedding, None
        _, n, _ = ctx.dims()
        k = ctx.k
    else:
        ctx, E = None, np.asarray(embedding, dtype=np.float64)
        if E.ndim != 2:
            raise ValueError("embedding must be a cells x factors matrix")
        n, k = E.shape
    d0 = None
    if dims is not None:
        d = np.atleast_1d(np.asarray(dims))
        if d.ndim != 1 or d.dtype.kind not in "iu":
            raise ValueError("dims must be a list of 1-based dimensions")
        d = d.astype(np.int64)
        if d.size and np.max(d) > k:
            raise ValueError("you requested up to %d dims but there are only %d dimensions in reduction" % (np.max(d), k))
        if d.size == 0 or np.min(d) < 1:
            raise ValueError("dims are 1-based: at least one, none below 1")
        d0 = d - 1
    K = int(k_param)
    if n * max(K, 0) > 2**31 - 1:
        raise ValueError("%d cells x %d neighbours do not fit a dgCMatrix" % (n, K))
    if ctx is not None:
        idx, dist = ctx.knn(K, dims=d0, **mkw)
    else:
        idx, dist = knn(E.T, None, K, d0, **mkw)
    _refuse_short("find_neighbors", idx)
    order = np.argsort(idx, axis=1, kind="stable")
    rows = np.take_along_axis(idx, order, axis=1).ravel()
    x = np.take_along_axis(dist, order, axis=1).ravel() if return_dist else np.ones(rows.size)
    nn = dgCMatrix(x, rows, np.arange(n + 1, dtype=np.int64) * K, (n, n))
    snn = c_SNN(nn, np.nextafter(prune_snn, -np.inf), 0) if compute_snn else None
    return {"nn": nn, "snn": snn, "idx": idx, "dist": dist}


# ---------------------------------------------------------------------------
# A neighbour index kept on the GPU, and label / value transfer to query cells (ProjectData followed by Seurat's TransferData /
# MapQuery; the rules are this library's own: include/singlet_hip.h, "Neighbour index and transfer")
# ---------------------------------------------------------------------------
class ReferenceIndex:
    """The reference cells of an embedding kept on the device for any number of searches (Context.knn_index_build), with the
    labels and values that are transferred to query cells.  `embedding_or_context` is cells x factors, or a Context with a fit,
    whose H is snapshotted (a fit continued afterwards does not change the index), as in find_neighbors; from an array the
    index owns a context of its own.  labels: one class in [-1, n_classes) per reference cell (-1: none); values: cells x
    n_values (layout coordinates, any covariate).  dims are 1-based, as in find_neighbors, and are applied to every query.
    method "ivf" (n_lists, n_iter as knn) or "exact".  A context manager; close() drops the index."""

    def __init__(self, embedding_or_context, labels=None, values=None, dims=None, metric="euclidean", method="ivf", n_lists=None, n_iter=10,
                 layout=None):
        from .context import Context
        knn_metric(metric)
        knn_method(method)
        self._own = not isinstance(embedding_or_context, Context)
        E = None
        if self._own:
            E = np.asarray(embedding_or_context, dtype=np.float64)
            if E.ndim != 2:
                raise ValueError("embedding must be a cells x factors matrix")
        d0 = None
        if dims is not None:
            d = np.atleast_1d(np.asarray(dims))
            if d.ndim != 1 or d.dtype.kind not in "iu" or d.size == 0 or np.min(d) < 1:
                raise ValueError("dims are 1-based: at least one, none below 1")
            d0 = d.astype(np.int64) - 1
        self._ctx = Context(0) if self._own else embedding_or_context
        try:
            self._ctx.knn_index_build(None if E is None else E.T, d0, metric, method, n_lists, n_iter)
            if labels is not None or values is not None:
                V = None
                if values is not None:
                    V = np.asarray(values, dtype=np.float64)
                    V = (V[:, None] if V.ndim == 1 else V).T
                self._ctx.knn_index_annotate(labels, None, V)
            self.has_layout = False
            if layout is not None:
                self.set_layout(layout)
        except Exception:
            self.close()
            raise

    def search(self, query, n_neighbors=20, n_probe=None, query_batch=0):
        """(idx, dist) of the query cells (cells x factors), as knn returns them."""
        return self._ctx.knn_index_search(np.asarray(query, dtype=np.float64).T, n_neighbors, n_probe, query_batch)

    def map(self, query, n_neighbors=20, n_probe=None, weighting="distance"):
        """Context.knn_index_map of the query cells (cells x factors); a query that comes back with fewer neighbours than
        asked for raises ValueError naming n_probe."""
        out = self._ctx.knn_index_map(np.asarray(query, dtype=np.float64).T, n_neighbors, n_probe, weighting)
        _refuse_short("ReferenceIndex.map", out["idx"])
        return out

    def set_layout(self, layout):
        """The layout of the reference cells (cells x dim, run_umap's positions), kept on the device with the index."""
        self._ctx.knn_index_set_layout(np.asarray(layout, dtype=np.float64).T)
        self.has_layout = True

    def project(self, query, a, b, n_neighbors=20, n_probe=None, n_epochs=None, alpha0=0.25, neg_rate=5, seed=42, query_batch=0):
        """Context.knn_index_project of the query cells (cells x factors): they are drawn in the reference's layout; a query
        that comes back with fewer neighbours than asked for raises ValueError naming n_probe, as map does."""
        out = self._ctx.knn_index_project(np.asarray(query, dtype=np.float64).T, a, b, n_neighbors, n_probe, n_epochs, alpha0, neg_rate, seed,
                                          query_batch)
        _refuse_short("ReferenceIndex.project", out["idx"])
        return out

    def info(self):
        return self._ctx.knn_index_info()

    def close(self):
        ctx, self._ctx = self._ctx, None
        if ctx is None:
            return
        if self._own:
            ctx.close()
        else:
            ctx.knn_index_drop()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _transfer(idx, dist, labels, n_classes, values, weighting):
    from .context import Context
    n_ref = np.asarray(labels).shape[0] if labels is not None else values.shape[1]
    with Context(0) as c:
        return c.op_knn_transfer(idx, dist, n_ref, labels, n_classes, values, weighting)


def transfer_labels(idx, dist, labels, n_classes=None, weighting="distance"):
    """The labels of the reference cells voted onto the query cells along their neighbour lists (sgl_op_knn_transfer): idx /
    dist n_query x n_neighbors as a search returns them, labels one class in [-1, n_classes) per reference cell ->
    {"predicted", "score", "scores"} as Context.knn_index_map returns them."""
    if labels is None:
        raise ValueError("labels must hold one class per reference cell")
    out = _transfer(idx, dist, labels, n_classes, None, weighting)
    return {k: out[k] for k in ("predicted", "score", "scores")}


def transfer_values(idx, dist, values, weighting="distance"):
    """The neighbour-weighted means of the reference cells' values (cells x n_values) for the query cells: n_query x
    n_values (sgl_op_knn_transfer)."""
    V = np.asarray(values, dtype=np.float64)
    if V.ndim not in (1, 2):
        raise ValueError("values must be a cells x n_values matrix")
    return _transfer(idx, dist, None, None, (V[:, None] if V.ndim == 1 else V).T, weighting)["values"]


def map_query(A, w, index, L1=0.01, L2=0, n_neighbors=20, n_probe=None, weighting="distance", layout=False, a=None, b=None, n_epochs=None,
              alpha0=0.25, neg_rate=5, seed=42):
    """New cells mapped onto a reference: project_model(A, w, L1, L2) and its h handed to index.map (a ReferenceIndex built on
    the reference's embedding in the same factor order).  A: anything project_model takes, native(...) included.  Returns
    {"h", "d", "idx", "dist", "predicted", "score", "scores", "values"}; a query that comes back short raises ValueError.
    layout=True (the index holds a layout; a, b the curve of the reference's run_umap, or a UmapModel as `a`) adds "layout"
    and "layout_init": index.project of the same h, the query cells drawn in the reference's picture."""
    if not isinstance(index, ReferenceIndex):
        raise ValueError("index must be a ReferenceIndex")
    knn_weighting(weighting)
    m = project_model(A, w, L1, L2)
    out = index.map(np.asarray(m["h"]).T, n_neighbors, n_probe, weighting)
    res = {"h": m["h"], "d": m["d"], **out}
    if layout:
        if isinstance(a, UmapModel):
            a, b = a.a, a.b
        if a is None or b is None:
            raise ValueError("map_query: layout=True needs the curve (a, b) of the reference's layout")
        pr = index.project(np.asarray(m["h"]).T, a, b, n_neighbors, n_probe, n_epochs, alpha0, neg_rate, seed)
        res["layout"], res["layout_init"] = pr["layout"], pr["layout_init"]
    return res


# ---------------------------------------------------------------------------
# Clustering (Seurat's FindClusters on the SNN graph; the rules are this library's own: include/singlet_hip.h, "Clustering")
# ---------------------------------------------------------------------------
LOUVAIN_MAX_LEVELS = 32


def _square_graph(G, what):
    G = as_dgCMatrix(G)
    if G.nrow != G.ncol:
        raise ValueError("%s: the graph must be square, not %d x %d" % (what, G.nrow, G.ncol))
    return G


def c_louvain(G, resolutions, tol=1e-7, max_sweeps=64, max_levels=32):
    """sgl_c_louvain: deterministic multi-level Louvain on the symmetric n x n graph G for every resolution of the list ->
    {"labels": n_res x n int32 (clusters numbered by descending size), "n_clusters", "n_levels": n_res, "q_levels",
    "sweeps_levels": n_res x 32}.  The graph is uploaded and validated once."""
    G = _square_graph(G, "c_louvain")
    res = np.ascontiguousarray(np.atleast_1d(np.asarray(resolutions, dtype=np.float64)).ravel())
    n, R = G.ncol, int(res.size)
    labels = np.zeros((max(R, 1), n), dtype=np.int32)
    ncl, nlev = np.zeros(max(R, 1), dtype=np.int32), np.zeros(max(R, 1), dtype=np.int32)
    q = np.zeros((max(R, 1), LOUVAIN_MAX_LEVELS))
    sw = np.zeros((max(R, 1), LOUVAIN_MAX_LEVELS), dtype=np.int32)
    check(_lib.load().sgl_c_louvain(ptr(G.x, f64p), ptr(G.i, i32p), ptr(G.p, i32p), n, ptr(res, f64p), R, float(tol), int(max_sweeps),
                                    int(max_levels), ptr(labels, i32p), ptr(ncl, i32p), ptr(nlev, i32p), ptr(q, f64p), ptr(sw, i32p)))
    return {"labels": labels[:R], "n_clusters": ncl[:R], "n_levels": nlev[:R], "q_levels": q[:R], "sweeps_levels": sw[:R]}


def op_louvain_sweep(G, labels, resolution=1.0):
    """sgl_op_louvain_sweep: one synchronous sweep on G from `labels` -> (labels_out, Q of labels, Q of labels_out, moved).
    No guard decision; G need not be symmetric (a coarse graph is a valid input)."""
    G = _square_graph(G, "op_louvain_sweep")
    n = G.ncol
    lab = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    if lab.size != n:
        raise ValueError("op_louvain_sweep: %d labels for %d vertices" % (lab.size, n))
    out = np.zeros(n, dtype=np.int32)
    q0, q1, moved = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
    check(_lib.load().sgl_op_louvain_sweep(ptr(G.x, f64p), ptr(G.i, i32p), ptr(G.p, i32p), n, ptr(lab, i32p), float(resolution),
                                           ptr(out, i32p), C.byref(q0), C.byref(q1), C.byref(moved)))
    return out, q0.value, q1.value, int(moved.value)


def louvain_info():
    """sgl_louvain_info: what the last clustering call of this process ran."""
    out = np.zeros(4, dtype=np.int64)
    check(_lib.load().sgl_louvain_info(ptr(out, _lib.i64p)))
    return dict(zip(("fast_degree", "slow_level0", "slow_coarse", "coarse_build"), (int(v) for v in out)))


def _without_diagonal(G):
    col = np.repeat(np.arange(G.ncol, dtype=np.int64), np.diff(G.p))
    keep = G.i != col
    p = np.concatenate(([0], np.cumsum(np.bincount(col[keep], minlength=G.ncol))))
    return dgCMatrix(G.x[keep], G.i[keep], p, G.Dim)


def find_clusters(graph, resolution=0.8, drop_diagonal=True, tol=1e-7, max_sweeps=64, max_levels=32):
    """The numeric step of Seurat's FindClusters on a neighbour graph: modularity clusters of the cells at every resolution
    asked for.  `graph` is a symmetric n x n dgCMatrix / SciPy matrix, or the dict find_neighbors returns (its "snn" is
    used); `resolution` a number or a list; drop_diagonal removes the stored diagonal first (the unit diagonal of an SNN
    graph says nothing about communities and only damps the moves).  Returns {"clusters": n x n_res int32, column r the
    clusters at resolution r numbered by descending size (0 the largest), "modularity": n_res, the Q reached,
    "n_clusters": n_res, "levels": n_res}.  The optimiser is this library's deterministic synchronous Louvain, not
    Seurat's seeded one: no parity of labels is claimed (include/singlet_hip.h, "Clustering")."""
    if isinstance(graph, dict):
        if graph.get("snn") is None:
            raise ValueError("find_clusters: the neighbours were computed without an SNN graph (compute_snn=False)")
        graph = graph["snn"]
    G = _square_graph(graph, "find_clusters")
    res = np.atleast_1d(np.asarray(resolution, dtype=np.float64))
    if res.ndim != 1 or res.size < 1:
        raise ValueError("find_clusters: resolution must be a number or a list of numbers")
    if not np.all(np.isfinite(res) & (res > 0)):
        raise ValueError("find_clusters: every resolution must be finite and > 0")
    if drop_diagonal:
        G = _without_diagonal(G)
    out = c_louvain(G, res, tol, max_sweeps, max_levels)
    last = np.maximum(out["n_levels"], 1) - 1
    return {"clusters": np.ascontiguousarray(out["labels"].T), "modularity": out["q_levels"][np.arange(res.size), last],
            "n_clusters": out["n_clusters"], "levels": out["n_levels"]}


# ---------------------------------------------------------------------------
# Layout (Seurat's RunUMAP on the nmf reduction; the rules are this library's own: include/singlet_hip.h, "Layout")
# ---------------------------------------------------------------------------
def fuzzy_simplicial_set(idx, dist, return_sigmas=False):
    """sgl_c_fuzzy_graph: the fuzzy neighbour graph of k-NN lists as knn returns them (idx, dist: n x K, row j the candidates
    of cell j in rank order) -> the symmetric n x n dgCMatrix (rows ascending, no diagonal, bitwise symmetric: what c_louvain
    and umap_layout take); with return_sigmas also (rho, sigma)."""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if idx.ndim != 2 or idx.shape != dist.shape:
        raise ValueError("fuzzy_simplicial_set: idx and dist must both be n x K")
    n, K = idx.shape
    L = _lib.load()
    rho, sigma = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    p, i, x = _two_call(lambda po, no, io, xo, cap: L.sgl_c_fuzzy_graph(ptr(idx, i32p), ptr(dist, f64p), n, K, po, no, io, xo, cap,
                                                                         ptr(rho, f64p), ptr(sigma, f64p)), n)
    G = dgCMatrix(x, i, p, (n, n))
    return (G, rho[:n], sigma[:n]) if return_sigmas else G


def _layout_args(G, Y, what):
    G = _square_graph(G, what)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[0] != G.ncol:
        raise ValueError("%s: the positions must be n x dim with one row per vertex of the graph" % what)
    return G, Y


def umap_layout(G, Y0, a, b, n_epochs, alpha0=1.0, neg_rate=5, seed=42):
    """sgl_c_umap_layout: n_epochs synchronous epochs on the graph G from the positions Y0 (n x dim) -> Y (n x dim)."""
    G, Y0 = _layout_args(G, Y0, "umap_layout")
    Y = np.empty_like(Y0)
    check(_lib.load().sgl_c_umap_layout(ptr(G.x, f64p), ptr(G.i, i32p), ptr(G.p, i32p), G.ncol, ptr(Y0, f64p), Y0.shape[1], float(a),
                                        float(b), int(n_epochs), float(alpha0), int(neg_rate), int(seed), ptr(Y, f64p)))
    return Y


def op_umap_epoch(G, Y, a, b, n_epochs, t, alpha0=1.0, neg_rate=5, seed=42):
    """sgl_op_umap_epoch: the ONE epoch t (1-based) of a layout of n_epochs epochs, from the positions Y -> the new positions."""
    G, Y = _layout_args(G, Y, "op_umap_epoch")
    out = np.empty_like(Y)
    check(_lib.load().sgl_op_umap_epoch(ptr(G.x, f64p), ptr(G.i, i32p), ptr(G.p, i32p), G.ncol, ptr(Y, f64p), Y.shape[1], float(a),
                                        float(b), int(n_epochs), float(alpha0), int(neg_rate), int(seed), int(t), ptr(out, f64p)))
    return out


def umap_info():
    """sgl_umap_info: what the last layout and the last fuzzy graph of this process ran."""
    out = np.zeros(4, dtype=np.int64)
    check(_lib.load().sgl_umap_info(ptr(out, _lib.i64p)))
    return dict(zip(("instance", "widest_column", "multi_chunk", "merge_fallback"), (int(v) for v in out)))


def find_ab_params(spread=1.0, min_dist=0.3):
    """(a, b) of the layout's curve 1 / (1 + a x^(2b)): the least-squares fit to umap-learn's target -- 1 up to min_dist,
    exp(-(x - min_dist) / spread) beyond -- on linspace(0, 3 spread, 300), by Levenberg-Marquardt from (1, 1)."""
    spread, min_dist = float(spread), float(min_dist)
    if not (spread > 0 and np.isfinite(spread)) or not (min_dist >= 0 and np.isfinite(min_dist)):
        raise ValueError("find_ab_params: spread must be > 0 and min_dist >= 0")
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    lx = np.log(np.where(x > 0, x, 1.0))

    def model(q):
        u = np.where(x > 0, np.exp(2.0 * q[1] * lx), 0.0)   # x^(2b)
        return u, 1.0 / (1.0 + q[0] * u)

    q = np.array([1.0, 1.0])
    u, f = model(q)
    r = f - y
    ss, lam = float(r @ r), 1e-3
    for _ in range(500):
        J = np.stack([-u * f * f, -q[0] * u * 2.0 * lx * f * f], axis=1)
        A, g = J.T @ J, J.T @ r
        step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        q2 = q + step
        if q2[0] > 0 and q2[1] > 0:
            u2, f2 = model(q2)
            r2 = f2 - y
            ss2 = float(r2 @ r2)
        else:
            ss2 = np.inf
        if ss2 <= ss:
            small = np.max(np.abs(step) / np.abs(q2)) < 1e-14
            q, u, f, r, ss, lam = q2, u2, f2, r2, ss2, max(lam / 10.0, 1e-12)
            if small:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return float(q[0]), float(q[1])


def _rand2(state, i, j):
    """The library's counter hash (sgl_op_rand) on numpy uint64 arrays: the bits the device and the oracle give."""
    M = np.uint64
    with np.errstate(over="ignore"):
        i = np.asarray(i, dtype=M).copy()
        j = np.asarray(j, dtype=M).copy()
        i ^= i << M(19)
        i ^= i >> M(7)
        i ^= i << M(36)
        x = M(state) + i
        x ^= x << M(38)
        x ^= x >> M(13)
        x ^= x << M(23)
        j ^= j >> M(7)
        j ^= j << M(23)
        j ^= j >> M(8)
        x = x + j
        x ^= x >> M(7)
        x ^= x << M(53)
        x ^= x >> M(4)
    return x


def _umap_init(E, n_components, init, seed):
    """The start positions (n x n_components) of run_umap from the k x n embedding E."""
    k, n = E.shape
    if isinstance(init, str):
        if init == "pca":
            if n_components > k:
                raise ValueError("run_umap: init='pca' gives at most %d components" % k)
            Ec = E - E.mean(axis=1, keepdims=True)
            lam, V = np.linalg.eigh(Ec @ Ec.T)                   # the k x k Gram on the host
            V = V[:, np.argsort(-lam, kind="stable")[:n_components]]
            top = np.argmax(np.abs(V), axis=0)
            V = V * np.where(V[top, np.arange(V.shape[1])] < 0, -1.0, 1.0)   # the largest-magnitude loading is positive
            Y = (V.T @ Ec).T
            m = np.max(np.abs(Y)) if Y.size else 0.0
            return np.ascontiguousarray(Y * (10.0 / m)) if m > 0 else np.ascontiguousarray(Y)
        if init == "random":
            c, f = np.meshgrid(np.arange(n, dtype=np.uint64), np.arange(n_components, dtype=np.uint64), indexing="ij")
            u = _rand2(int(seed) & (2**64 - 1), c, f)
            return (u >> np.uint64(11)).astype(np.float64) * (20.0 / 2.0**53) - 10.0
        raise ValueError("run_umap: init must be 'pca', 'random' or an n x n_components array")
    Y = np.ascontiguousarray(init, dtype=np.float64)
    if Y.shape != (n, n_components):
        raise ValueError("run_umap: the init array must be %d x %d" % (n, n_components))
    return Y


def run_umap(embedding, n_neighbors=30, n_components=2, min_dist=0.3, spread=1.0, n_epochs=None, learning_rate=1.0,
             negative_sample_rate=5, init="pca", seed=42, dims=None, return_graph=False, metric="euclidean", nn_method="exact", n_lists=None,
             n_probe=None, return_model=False):
    """The numeric steps of Seurat's RunUMAP(reduction = "nmf") on the device: exact k-NN, the fuzzy neighbour graph, and
    the synchronous layout (include/singlet_hip.h, "Layout").  `embedding` is k x n (R's orientation, one column per cell, as
    knn takes it) or a Context with a fit, whose H is searched where it lies; dims: 0-based rows.  n_epochs None: 500 up to
    10 000 cells, 200 above.  init: "pca" (the top components of the centred embedding, each signed so that its
    largest-magnitude loading is positive, scaled to max |y| = 10), "random" (uniform in [-10, 10) from the hash of
    (seed, cell, component)) or an n x n_components array.  Returns the n x n_components positions, with return_graph
    (positions, graph).  metric: "euclidean", "cosine" or "correlation", the metric of the neighbour search as knn takes it
    (the graph is then built on 1 - cos).  Seurat's RunUMAP defaults to metric = "cosine"; ours stays "euclidean", so that
    existing results stay.  nn_method "ivf", n_lists, n_probe: the approximate search, as find_neighbors takes them (a short
    result raises ValueError naming n_probe).  return_model: also a UmapModel, what project_umap needs to draw new cells into
    this picture (returned last).  No parity of coordinates with uwot or umap-learn is claimed."""
    from .context import Context
    mkw = {**_metric_kw(metric), **_nn_method_kw(nn_method, n_lists, n_probe)}
    if isinstance(embedding, Context):
        ctx = embedding
        E = np.ascontiguousarray(ctx.get_factors(w=False, d=False, h=True)[2].T)
    else:
        ctx, E = None, np.asarray(embedding, dtype=np.float64)
        if E.ndim != 2:
            raise ValueError("run_umap: embedding must be a k x n matrix or a Context")
    d0 = None
    if dims is not None:
        d0 = np.atleast_1d(np.asarray(dims))
        if d0.ndim != 1 or d0.dtype.kind not in "iu" or d0.size == 0 or d0.min() < 0 or d0.max() >= E.shape[0]:
            raise ValueError("run_umap: dims must be 0-based rows of the embedding")
    n = E.shape[1]
    n_components = int(n_components)
    if not 1 <= n_components <= 8:
        raise ValueError("run_umap: n_components must lie in [1, 8]")
    if n_epochs is None:
        n_epochs = 500 if n <= 10000 else 200
    a, b = find_ab_params(spread, min_dist)
    Y0 = _umap_init(E if d0 is None else E[d0], n_components, init, seed)
    idx, dist = ctx.knn(int(n_neighbors), dims=d0, **mkw) if ctx is not None else knn(E, None, int(n_neighbors), d0, **mkw)
    _refuse_short("run_umap", idx)
    G = fuzzy_simplicial_set(idx, dist)
    Y = umap_layout(G, Y0, a, b, n_epochs, learning_rate, negative_sample_rate, int(seed) & (2**64 - 1))
    if return_model:
        model = UmapModel(a, b, int(n_neighbors), metric, None if d0 is None else d0.astype(np.int64), Y, float(learning_rate),
                          int(negative_sample_rate), int(seed) & (2**64 - 1))
        return (Y, G, model) if return_graph else (Y, model)
    return (Y, G) if return_graph else Y


# ---------------------------------------------------------------------------
# Layout transform (Seurat's ProjectUMAP / MapQuery picture, umap-learn's transform; the rules are this library's own:
# include/singlet_hip.h, "Layout transform")
# ---------------------------------------------------------------------------
class UmapModel:
    """What a later projection needs of a run_umap(..., return_model=True): the curve (a, b), n_neighbors, the metric and the
    dims (0-based rows of the embedding, or None) of its neighbour search, the positions (n x n_components), the learning
    rate, the negative sample rate and the seed."""

    def __init__(self, a, b, n_neighbors, metric, dims, positions, learning_rate=1.0, negative_sample_rate=5, seed=42):
        self.a, self.b, self.n_neighbors, self.metric, self.dims = float(a), float(b), int(n_neighbors), metric, dims
        self.positions = np.ascontiguousarray(positions, dtype=np.float64)
        self.learning_rate, self.negative_sample_rate, self.seed = float(learning_rate), int(negative_sample_rate), int(seed)


def _transform_epochs(n_query, n_epochs):
    """umap-learn's transform: 100 epochs up to 10 000 queries, 30 above."""
    return int(n_epochs) if n_epochs is not None else (100 if n_query <= 10000 else 30)


def _query_lists(idx, second, what, name):
    from ._marshal import knn_lists_in
    i, d, nq, K = knn_lists_in(idx, second)
    if not 1 <= K <= 256:
        raise ValueError("%s: idx and %s must be n_query x K with K in [1, 256]" % (what, name))
    return i, d, nq, K


def _positions(Y, rows, what, name):
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    if Y.ndim != 2 or (rows is not None and Y.shape[0] != rows) or not 1 <= Y.shape[1] <= 8:
        raise ValueError("%s: %s must be %s x dim with dim in [1, 8]" % (what, name, "n" if rows is None else rows))
    return Y


def fuzzy_query(idx, dist, n_ref):
    """sgl_c_fuzzy_query: the memberships of query cells' neighbour lists against a reference of n_ref cells (idx, dist:
    n_query x K as the searches return them, padding -1 / +Inf behind the valid slots) -> (W n_query x K, rho, sigma)."""
    i, d, nq, K = _query_lists(idx, dist, "fuzzy_query", "dist")
    W, rho, sigma = np.zeros((max(nq, 1), K)), np.zeros(max(nq, 1)), np.zeros(max(nq, 1))
    check(_lib.load().sgl_c_fuzzy_query(ptr(i, i32p), ptr(d, f64p), nq, K, int(n_ref), ptr(W, f64p), ptr(rho, f64p), ptr(sigma, f64p)))
    return W[:nq], rho[:nq], sigma[:nq]


def umap_transform(idx, dist, layout, a, b, n_epochs=None, alpha0=0.25, neg_rate=5, seed=42, query_offset=0, return_init=False):
    """sgl_c_umap_transform: query cells placed in the fixed layout of the reference (n_ref x dim) from their neighbour lists
    against it (idx, dist: n_query x K) -> their positions (n_query x dim); with return_init (start, positions).  n_epochs
    None: 100 up to 10 000 queries, 30 above.  query_offset: the global index of the first query, with which a slice of a
    larger call reproduces that call's rows."""
    i, d, nq, K = _query_lists(idx, dist, "umap_transform", "dist")
    Yr = _positions(layout, None, "umap_transform", "layout")
    Y0, Y = np.empty((max(nq, 1), Yr.shape[1])), np.empty((max(nq, 1), Yr.shape[1]))
    check(_lib.load().sgl_c_umap_transform(ptr(i, i32p), ptr(d, f64p), nq, K, ptr(Yr, f64p), Yr.shape[1], Yr.shape[0], float(a), float(b),
                                           _transform_epochs(nq, n_epochs), float(alpha0), int(neg_rate), int(seed) & (2**64 - 1),
                                           int(query_offset), ptr(Y0, f64p), ptr(Y, f64p)))
    return (Y0[:nq], Y[:nq]) if return_init else Y[:nq]


def op_umap_transform_epochs(idx, W, layout, Y, a, b, n_epochs, t_first, t_last, alpha0=0.25, neg_rate=5, seed=42, query_offset=0):
    """sgl_op_umap_transform_epochs: the epochs t_first .. t_last (1-based) of a transform of n_epochs epochs from the
    caller's memberships W (n_query x K) and positions Y (n_query x dim) -> the new positions."""
    i, Wc, nq, K = _query_lists(idx, W, "op_umap_transform_epochs", "W")
    Yr = _positions(layout, None, "op_umap_transform_epochs", "layout")
    Yin = _positions(Y, nq, "op_umap_transform_epochs", "Y")
    if Yin.shape[1] != Yr.shape[1]:
        raise ValueError("op_umap_transform_epochs: Y and layout must have the same dim")
    out = np.empty((max(nq, 1), Yr.shape[1]))
    check(_lib.load().sgl_op_umap_transform_epochs(ptr(i, i32p), ptr(Wc, f64p), nq, K, ptr(Yr, f64p), Yr.shape[1], Yr.shape[0],
                                                   ptr(Yin if nq else out, f64p), float(a), float(b), int(n_epochs), float(alpha0), int(neg_rate),
                                                   int(seed) & (2**64 - 1), int(query_offset), int(t_first), int(t_last), ptr(out, f64p)))
    return out[:nq]


def umap_transform_info():
    """sgl_umap_transform_info: what the last layout transform of this process ran."""
    out = np.zeros(4, dtype=np.int64)
    check(_lib.load().sgl_umap_transform_info(ptr(out, _lib.i64p)))
    return dict(zip(("instance", "widest_list", "empty_queries", "launches"), (int(v) for v in out)))


def project_umap(model, index_or_reference_embedding, query_embedding, n_epochs=None, n_probe=None, return_init=False, query_batch=0):
    """The ProjectUMAP mirror: query cells (cells x factors) drawn in the picture of a run_umap(..., return_model=True).
    `index_or_reference_embedding`: a ReferenceIndex on the reference's embedding (it receives the model's positions as its
    layout when it holds none), or the reference embedding itself (cells x factors), on which an exact index is built for the
    call under the model's metric and dims.  alpha0 is a quarter of the model's learning rate.  -> positions (n_query x
    n_components); with return_init (start, positions)."""
    if not isinstance(model, UmapModel):
        raise ValueError("project_umap: model must come from run_umap(..., return_model=True)")
    own = not isinstance(index_or_reference_embedding, ReferenceIndex)
    index = index_or_reference_embedding
    if own:
        dims1 = None if model.dims is None else np.asarray(model.dims) + 1
        index = ReferenceIndex(index_or_reference_embedding, dims=dims1, metric=model.metric, method="exact", layout=model.positions)
    try:
        if not index.has_layout:
            index.set_layout(model.positions)
        out = index.project(query_embedding, model.a, model.b, model.n_neighbors, n_probe, n_epochs, 0.25 * model.learning_rate,
                            model.negative_sample_rate, model.seed, query_batch)
    finally:
        if own:
            index.close()
    return (out["layout_init"], out["layout"]) if return_init else out["layout"]


# ---------------------------------------------------------------------------
# Marker genes (Seurat's FindAllMarkers / FindMarkers, Wilcoxon rank-sum test)
# ---------------------------------------------------------------------------
def c_markers(A, labels, n_groups=None, transform="expm1", pseudocount=1.0):
    """The one-shot form of Context.markers (sgl_c_markers): A a dgCMatrix or anything as_dgCMatrix accepts, in a context of
    its own.  Returns the same dict of arrays."""
    A = as_dgCMatrix(A)
    g, G = label_list(labels, A.ncol, n_groups)
    L = _lib.load()
    return markers_call(lambda *a: L.sgl_c_markers(*csc_ptrs(A), A.nrow, A.ncol, *a), A.nrow, g, G, transform, pseudocount)


def _markers_of(A, labels, n_groups, transform, pseudocount):
    """(the dict of Context.markers, the row names or None) for whatever find_all_markers takes."""
    from .context import Context
    if isinstance(A, Context):
        return A.markers(labels, n_groups, transform, pseudocount), None
    if isinstance(A, NativeMatrix):
        return _on_native(A, lambda ctx, fits: ctx.markers(labels, n_groups, transform, pseudocount)), A.Dimnames[0]
    A = as_dgCMatrix(A)
    return c_markers(A, labels, n_groups, transform, pseudocount), A.Dimnames[0]


def _marker_table(st, c, names, min_pct, logfc_threshold, only_pos, return_thresh):
    """The rows of cluster c that pass the filters, in the stated order."""
    m = st["p"].shape[0]
    p, fc, p1, p2 = st["p"][:, c], st["log2fc"][:, c], st["pct_in"][:, c], st["pct_out"][:, c]
    with np.errstate(invalid="ignore"):
        keep = np.fmax(p1, p2) >= min_pct
        keep &= (fc >= logfc_threshold) if only_pos else (np.abs(fc) >= logfc_threshold)
        keep &= p < return_thresh
    genes = np.nonzero(keep)[0]
    genes = genes[np.lexsort((genes, -fc[genes], p[genes]))]   # (p_val asc, avg_log2FC desc, gene asc)
    out = {"gene": genes.astype(np.int32), "p_val": p[genes], "avg_log2FC": fc[genes], "pct_1": p1[genes], "pct_2": p2[genes],
           "p_val_adj": np.minimum(1.0, p[genes] * m)}
    if names is not None:
        out["names"] = _subset_names(names, out["gene"])
    return out


def find_all_markers(A, clusters, min_pct=0.1, logfc_threshold=0.25, only_pos=False, return_thresh=0.01, transform="expm1",
                     pseudocount=1.0):
    """Seurat::FindAllMarkers(test.use = "wilcox") on the device: for every cluster, the genes that mark it against all other
    cells (sgl_markers; the rules are stated in include/singlet_hip.h, "Marker genes").  A: a dgCMatrix, anything
    as_dgCMatrix accepts, a native(...) object, or a Context that holds the (normally log-normalised) matrix.  clusters: one
    id >= 0 per cell, -1 leaves the cell out.  Returns a list with one dict per cluster: "cluster", "gene" (int32 row
    indices), "names" (when A has row names), "p_val", "avg_log2FC", "pct_1", "pct_2", "p_val_adj" = min(1, p * nrow).
    The filters -- max(pct_1, pct_2) >= min_pct; |avg_log2FC| >= logfc_threshold (avg_log2FC >= it with only_pos);
    p_val < return_thresh -- are applied AFTER the test, to all genes; Seurat filters by pct and fold change BEFORE it tests:
    the retained rows are the same.  Rows are ordered by (p_val ascending, avg_log2FC descending, gene ascending)."""
    st, names = _markers_of(A, clusters, None, transform, pseudocount)
    out = []
    for c in range(st["group_n"].shape[0]):
        t = _marker_table(st, c, names, min_pct, logfc_threshold, only_pos, return_thresh)
        t["cluster"] = c
        out.append(t)
    return out


def find_markers(A, cells_1, cells_2=None, min_pct=0.1, logfc_threshold=0.25, only_pos=False, return_thresh=0.01,
                 transform="expm1", pseudocount=1.0):
    """Seurat::FindMarkers(ident.1, ident.2): the cells cells_1 (indices or a boolean mask) against cells_2 (None: all other
    cells), through the labels {0, 1, -1} of sgl_markers.  Returns the table of group 0 as find_all_markers lays it out."""
    from .context import Context
    if isinstance(A, Context):
        n = A.dims()[1]
    else:
        if not isinstance(A, NativeMatrix):
            A = as_dgCMatrix(A)
        n = A.ncol

    def mask(cells, what):
        c = np.asarray(cells)
        if c.dtype.kind == "b":
            if c.shape != (n,):
                raise ValueError("find_markers: a boolean %s needs one entry per cell (%d)" % (what, n))
            return c.copy()
        if c.ndim != 1 or c.dtype.kind not in "iu" or (c.size and (c.min() < 0 or c.max() >= n)):
            raise ValueError("find_markers: %s must hold cell indices in [0, %d)" % (what, n))
        mk = np.zeros(n, dtype=bool)
        mk[c] = True
        return mk
    m1 = mask(cells_1, "cells_1")
    m2 = ~m1 if cells_2 is None else mask(cells_2, "cells_2")
    if np.any(m1 & m2):
        raise ValueError("find_markers: a cell is in both groups")
    labels = np.full(n, -1, dtype=np.int32)
    labels[m2] = 1
    labels[m1] = 0
    st, names = _markers_of(A, labels, 2, transform, pseudocount)
    return _marker_table(st, 0, names, min_pct, logfc_threshold, only_pos, return_thresh)


# ---------------------------------------------------------------------------
# Signature scores of the cells (UCell's ScoreSignatures_UCell)
# ---------------------------------------------------------------------------
def c_signature_scores(A, sets, max_rank=1500, return_rank2=False):
    """The one-shot form of Context.signature_scores (sgl_c_signature_scores): A a dgCMatrix or anything as_dgCMatrix accepts,
    in a context of its own; the sets are checked before anything is uploaded.  Returns the same arrays."""
    A = as_dgCMatrix(A)
    L = _lib.load()
    return signature_call(lambda *a: L.sgl_c_signature_scores(*csc_ptrs(A), A.nrow, A.ncol, *a), A.ncol, sets, max_rank, return_rank2)


def signature_parse(signatures, gene_names=None, nrow=None, max_rank=1500, missing="skip"):
    """The host half of score_signatures.  signatures: dict name -> genes.  With gene_names the genes are names: a trailing
    "+" is stripped, a trailing "-" puts the gene into the signature's negative set; a name absent from gene_names is
    dropped and reported (missing="skip") or refused (missing="error").  Without gene_names they are 0-based int rows in
    [0, nrow), all positive.  Duplicates within a signature are dropped, the first occurrence kept.  A signature without a
    positive gene, or with more than max_rank genes on a side, is refused.  Returns (names, pos, neg, dropped): per
    signature its positive and negative rows as int32 arrays (neg may be empty), and dropped: dict name -> the names left
    out.  Pure host."""
    if missing not in ("skip", "error"):
        raise ValueError("score_signatures: missing must be 'skip' or 'error'")
    if not isinstance(signatures, dict) or not signatures:
        raise ValueError("score_signatures: signatures must be a dict name -> genes with at least one signature")
    index = None
    if gene_names is not None:
        index = {}
        for r, g in enumerate(gene_names):
            index.setdefault(g.decode() if isinstance(g, bytes) else str(g), r)   # a name that occurs twice: its first row
        nrow = len(gene_names)
    names, pos, neg, dropped = [], [], [], {}
    for name, genes in signatures.items():
        sides, gone = ([], []), []
        for g in ([genes] if isinstance(genes, (str, bytes)) else genes):
            side = 0
            if index is not None:
                g = g.decode() if isinstance(g, bytes) else str(g)
                if g.endswith("-"):
                    g, side = g[:-1], 1
                elif g.endswith("+"):
                    g = g[:-1]
                if g not in index:
                    if missing == "error":
                        raise ValueError("score_signatures: gene %r of signature %r is not among gene_names" % (g, name))
                    gone.append(g)
                    continue
                r = index[g]
            else:
                if isinstance(g, (str, bytes)) or int(g) != g:
                    raise ValueError("score_signatures: signature %r holds %r; without gene_names the genes are int rows" % (name, g))
                r = int(g)
                if nrow is not None and not 0 <= r < nrow:
                    raise ValueError("score_signatures: row %d of signature %r is outside [0, %d)" % (r, name, nrow))
            if r not in sides[0] and r not in sides[1]:
                sides[side].append(r)
        if not sides[0]:
            raise ValueError("score_signatures: signature %r has no positive gene%s" % (name, " left" if gone else ""))
        for what, side in zip(("", "negative "), sides):
            if len(side) > max_rank:
                raise ValueError("score_signatures: signature %r holds %d %sgenes, more than max_rank = %d" % (name, len(side), what, max_rank))
        names.append(name)
        pos.append(np.asarray(sides[0], dtype=np.int32))
        neg.append(np.asarray(sides[1], dtype=np.int32))
        if gone:
            dropped[name] = gone
    return names, pos, neg, dropped


def score_signatures(A, signatures, gene_names=None, max_rank=1500, w_neg=1.0, missing="skip"):
    """UCell's ScoreSignatures_UCell on the device: the rank-based score of every signature in every cell (sgl_signature_scores;
    the rules are stated in include/singlet_hip.h, "Signature scores").  A: a dgCMatrix, anything as_dgCMatrix accepts, a
    native(...) object, or a Context that holds the matrix (counts or normalised: only the order within a cell matters).
    signatures: a dict name -> gene names (int rows when gene_names is None), or the path of a GMT file (read_gmt).
    gene_names None: the row names of A when it has them.  A trailing "+" on a gene name is stripped, a trailing "-" puts
    the gene into the signature's negative set, scored as a device set of its own; the score is max(0, pos - w_neg * neg),
    computed on the host.  missing: "skip" drops the genes absent from gene_names and reports them, "error" refuses them.
    Everything is checked before anything is uploaded.  Returns {"scores" (n cells x S signatures), "names", "dropped"}."""
    from .context import Context
    if isinstance(signatures, (str, bytes, os.PathLike)):
        signatures = read_gmt(signatures)
    is_ctx, is_native = isinstance(A, Context), isinstance(A, NativeMatrix)
    if not is_ctx and not is_native:
        A = as_dgCMatrix(A)
    if gene_names is None and not is_ctx and A.Dimnames[0] is not None and isinstance(signatures, dict) and any(
            isinstance(g, (str, bytes)) for v in signatures.values() for g in ([v] if isinstance(v, (str, bytes)) else v)):
        gene_names = A.Dimnames[0]
    nrow = A.dims()[0] if is_ctx else A.nrow
    if gene_names is not None and len(gene_names) != nrow:
        raise ValueError("score_signatures: gene_names must name the %d rows of the matrix" % nrow)
    max_rank = int(max_rank)
    if not 1 <= max_rank <= nrow:
        raise ValueError("score_signatures: max_rank = %d is outside [1, %d] (the genes of the matrix)" % (max_rank, nrow))
    names, pos, neg, dropped = signature_parse(signatures, gene_names, nrow, max_rank, missing)
    has_neg = [j for j in range(len(names)) if neg[j].size]
    sets = pos + [neg[j] for j in has_neg]
    if is_ctx:
        sc = A.signature_scores(sets, max_rank)
    elif is_native:
        sc = _on_native(A, lambda ctx, fits: ctx.signature_scores(sets, max_rank))
    else:
        sc = c_signature_scores(A, sets, max_rank)
    S = len(names)
    scores = np.array(sc[:S].T)
    for t, j in enumerate(has_neg):
        scores[:, j] = np.maximum(0.0, scores[:, j] - float(w_neg) * sc[S + t])
    return {"scores": scores, "names": names, "dropped": dropped}


# ---------------------------------------------------------------------------
# Doublet scores (the scheme of Scrublet, Wolock, Lopez & Klein 2019; the rules are this library's own:
# include/singlet_hip.h, "Simulated doublets", DESIGN.md "Doublet scores")
# ---------------------------------------------------------------------------
DOUBLET_KNN_LIMIT = 256   # the neighbours one search returns (sgl_knn)


def doublet_parents(n_obs, n_sim, seed=0):
    """(parent_a, parent_b), int32, n_sim each: a = rng.integers(0, n_obs) and b = (a + 1 + rng.integers(0, n_obs - 1)) % n_obs
    from np.random.default_rng(seed), so the parents of a simulated cell are two DIFFERENT observed cells."""
    n_obs, n_sim = int(n_obs), int(n_sim)
    if n_obs < 2 or n_sim < 1:
        raise ValueError("doublet_parents: at least 2 observed cells and 1 simulated cell are needed")
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n_obs, size=n_sim)
    b = (a + 1 + rng.integers(0, n_obs - 1, size=n_sim)) % n_obs
    return a.astype(np.int32), b.astype(np.int32)


def doublet_scores(idx, n_obs, n_sim, expected_rate=0.1, stdev_rate=0.02):
    """Scrublet's doublet likelihood of every cell of the joint embedding [observed | simulated] from its neighbour lists:
    idx is (n_obs + n_sim) x (k_adj + 1), the search of the joint embedding against itself.  A cell's own index is removed from
    its list wherever it stands; when it is absent (duplicates pushed it out) the last entry is removed.  nd = the remaining
    entries >= n_obs (simulated neighbours); q = (nd + 1) / (k_adj + 2); r = n_sim / n_obs; rho = expected_rate;
      Ld = q rho / r / (1 - rho - q (1 - rho - rho / r));  se_q = sqrt(q (1 - q) / (k_adj + 3));
      se_Ld = q rho / r / (1 - rho - q (1 - rho - rho / r))^2 sqrt((se_q / q (1 - rho))^2 + (stdev_rate / rho (1 - q))^2).
    Host arithmetic.  Returns {"nd", "score", "se"} for the observed and {"sim_nd", "sim_score", "sim_se"} for the simulated."""
    idx = np.asarray(idx)
    n_obs, n_sim = int(n_obs), int(n_sim)
    if idx.ndim != 2 or idx.shape[0] != n_obs + n_sim or idx.shape[1] < 2 or n_obs < 1 or n_sim < 1:
        raise ValueError("doublet_scores: idx must be (n_obs + n_sim) x (k_adj + 1) with k_adj >= 1")
    rho, se_rho = float(expected_rate), float(stdev_rate)
    if not 0.0 < rho < 1.0 or not se_rho >= 0.0:
        raise ValueError("doublet_scores: expected_rate must lie in (0, 1) and stdev_rate must not be negative")
    n, k1 = idx.shape
    k_adj = k1 - 1
    own = idx == np.arange(n)[:, None]
    drop = np.where(own.any(axis=1), own.argmax(axis=1), k1 - 1)
    keep = np.ones((n, k1), dtype=bool)
    keep[np.arange(n), drop] = False
    nd = ((idx >= n_obs) & keep).sum(axis=1).astype(np.int64)
    q = (nd + 1) / float(k_adj + 2)
    r = n_sim / float(n_obs)
    den = 1 - rho - q * (1 - rho - rho / r)
    Ld = q * rho / r / den
    se_q = np.sqrt(q * (1 - q) / (k_adj + 3))
    se_Ld = q * rho / r / den ** 2 * np.sqrt((se_q / q * (1 - rho)) ** 2 + (se_rho / rho * (1 - q)) ** 2)
    return {"nd": nd[:n_obs], "score": Ld[:n_obs], "se": se_Ld[:n_obs], "sim_nd": nd[n_obs:], "sim_score": Ld[n_obs:], "sim_se": se_Ld[n_obs:]}


def _local_maxima(h):
    """Bins above their left neighbour and not below their right one, with empty bins beyond both ends: one per plateau, none
    among empty bins."""
    left, right = np.concatenate([[0.0], h[:-1]]), np.concatenate([h[1:], [0.0]])
    return np.flatnonzero((h > left) & (h >= right))


def doublet_threshold(sim_scores, bins=100):
    """The score that separates the two humps of the simulated cells' scores (doublets of two cell states against doublets
    within one): a histogram of `bins` bins on [0, max], smoothed by a 3-bin mean (empty bins beyond the ends) until at most
    two local maxima remain, at most 10 000 rounds; the threshold is the centre of the lowest bin between the two maxima (the
    first of several).  ValueError when two maxima are not there: the caller then passes a threshold."""
    s = np.asarray(sim_scores, dtype=np.float64).ravel()
    bins = int(bins)
    if s.size < 1 or bins < 3 or not np.all(np.isfinite(s)) or s.min() < 0 or not s.max() > 0:
        raise ValueError("doublet_threshold: needs finite non-negative scores with a positive maximum and at least 3 bins")
    top = float(s.max())
    h = np.histogram(s, bins=bins, range=(0.0, top))[0].astype(np.float64)
    peaks = _local_maxima(h)
    rounds = 0
    while peaks.size > 2 and rounds < 10000:
        h = (np.concatenate([[0.0], h[:-1]]) + h + np.concatenate([h[1:], [0.0]])) / 3.0
        peaks = _local_maxima(h)
        rounds += 1
    if peaks.size != 2:
        raise ValueError("doublet_threshold: the simulated scores show %d local maxima, not two; pass a threshold" % peaks.size)
    lo = int(peaks[0]) + 1 + int(np.argmin(h[peaks[0] + 1:peaks[1]]))
    return (lo + 0.5) * top / bins


def _whole(v, lo, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer, float, np.floating)) or int(v) != v or int(v) < lo:
        raise ValueError("score_doublets: %s must be a whole number of at least %d" % (what, lo))
    return int(v)


def score_doublets(A, w=None, rank=None, features=None, sim_ratio=2.0, n_neighbors=None, expected_rate=0.1, stdev_rate=0.02,
                   threshold=None, metric="euclidean", nn_method="exact", seed=0, sim_batch=0, L1=0.01, L2=0, scale_factor=1e4,
                   nfeatures=None, n_lists=None, n_probe=None, tol=1e-4, maxit=100, bins=100):
    """Doublet scores of the cells of a genes x cells COUNT matrix by the scheme of Scrublet, with the NMF projection as the
    reduction and every matrix step on the device.  A: anything RunNMF takes, native(...) included.
      1. one context holds the counts; `features` (as subset() takes rows) or `nfeatures` (Context.variable_features on the
         counts) selects the genes of the model;
      2. w None: the model is fitted first, run_nmf at `rank` (tol, maxit, L1, L2, seed) on the normalised observed matrix,
         and the counts are uploaded again; else w is the model (genes x k or k x genes, the selected genes in order);
      3. doublet_parents(n_obs, round(sim_ratio n_obs), seed); a second context receives the simulated cells in batches of
         sim_batch (0: all at once) through Context.simulate_doublets; each batch goes through log_normalize(scale_factor),
         subset(rows), fit_init(k, scale(w)) and the H-update of a projection (step_h; the row scaling of project_run is
         left out: it is taken over the cells of a batch, so it would tie a cell's coordinates to its batch and put the
         observed and the simulated cells on different scales);
      4. the first context is normalised, subset and projected the same way;
      5. Context.knn on [H_obs | H_sim] against itself with k_adj + 1 neighbours, k = n_neighbors (None:
         round(0.5 sqrt(n_obs))), k_adj = round(k (1 + n_sim / n_obs)); doublet_scores; the threshold (None:
         doublet_threshold of the simulated scores).
    Every argument is checked before the first upload; k_adj + 1 above the search's limit of 256 is refused there.  Returns
    {"scores", "se", "predicted", "threshold", "parent_a", "parent_b", "sim_scores", "sim_se", "nd", "sim_nd", "k_adj",
    "h_obs", "h_sim" (cells x k), "w"}."""
    from .context import Context
    is_native = isinstance(A, NativeMatrix)
    if not is_native:
        A = as_dgCMatrix(A)
    n_obs, nrow = int(A.ncol), int(A.nrow)
    if n_obs < 2:
        raise ValueError("score_doublets: at least 2 cells are needed")
    if not (isinstance(sim_ratio, (int, float, np.integer, np.floating)) and math.isfinite(sim_ratio) and sim_ratio > 0):
        raise ValueError("score_doublets: sim_ratio must be a positive number")
    n_sim = int(round(float(sim_ratio) * n_obs))
    if n_sim < 1 or n_sim > 2**31 - 1:
        raise ValueError("score_doublets: sim_ratio = %r gives %d simulated cells: between 1 and 2^31 - 1 are possible" % (sim_ratio, n_sim))
    k_nn = int(round(0.5 * math.sqrt(n_obs))) if n_neighbors is None else _whole(n_neighbors, 1, "n_neighbors")
    k_nn = max(k_nn, 1)
    k_adj = int(round(k_nn * (1 + n_sim / float(n_obs))))
    if k_adj + 1 > DOUBLET_KNN_LIMIT or k_adj + 1 > n_obs + n_sim:
        raise ValueError("score_doublets: sim_ratio = %r and n_neighbors = %d ask for k_adj + 1 = %d neighbours of %d joint cells; one "
                         "search returns at most %d: lower sim_ratio or n_neighbors" % (sim_ratio, k_nn, k_adj + 1, n_obs + n_sim,
                                                                                     DOUBLET_KNN_LIMIT))
    rho, se_rho = float(expected_rate), float(stdev_rate)
    if not 0.0 < rho < 1.0:
        raise ValueError("score_doublets: expected_rate must lie in (0, 1)")
    if not se_rho >= 0.0 or not math.isfinite(se_rho):
        raise ValueError("score_doublets: stdev_rate must be a finite number, not negative")
    if threshold is not None and not (isinstance(threshold, (int, float, np.integer, np.floating)) and math.isfinite(threshold)):
        raise ValueError("score_doublets: threshold must be a finite number or None")
    mkw = {**_metric_kw(metric), **_nn_method_kw(nn_method, n_lists, n_probe)}
    sim_batch = _whole(sim_batch, 0, "sim_batch")
    if not (isinstance(scale_factor, (int, float, np.integer, np.floating)) and math.isfinite(scale_factor) and scale_factor > 0):
        raise ValueError("score_doublets: scale_factor must be a positive number")
    L1f, L2f = float(_pair(L1)[1]), float(_pair(L2)[1])   # the H side of a pair, as run_nmf reads it
    if not (0 <= L1f < 1) or L2f < 0:
        raise ValueError("score_doublets: L1 must lie in [0, 1) and L2 must not be negative")
    rows = None
    if nfeatures is not None:
        if features is not None:
            raise ValueError("score_doublets: pass either features or nfeatures (the variable features selected here), not both")
        nfeatures = _whole(nfeatures, 1, "nfeatures")
        if nfeatures > nrow:
            raise ValueError("score_doublets: nfeatures = %d is above the %d genes of A" % (nfeatures, nrow))
    if features is not None:
        rows = _subset_index([features] if isinstance(features, str) else features, nrow, A.Dimnames[0], "features")
    m_sub = nfeatures if nfeatures is not None else (nrow if rows is None else int(np.asarray(rows).shape[0]))
    if (w is None) == (rank is None):
        raise ValueError("score_doublets: pass either w (a fitted model) or rank (the model is fitted here), not both and not neither")
    if w is not None:
        w = np.asarray(w, dtype=np.float64)
        if w.ndim != 2 or (w.shape[0] != m_sub and w.shape[1] != m_sub):
            raise ValueError("score_doublets: w must share an edge with the %d selected genes (got %r)" % (m_sub, w.shape))
        if not np.all(np.isfinite(w)):
            raise ValueError("score_doublets: w holds a non-finite value")
        wb = np.ascontiguousarray(w if w.shape[0] == m_sub else w.T)   # (genes, k)
        if not 1 <= wb.shape[1] <= 1024:
            raise ValueError("score_doublets: the rank of w must lie in [1, 1024]")
    else:
        rank = _whole(rank, 1, "rank")
        if rank > 1024:
            raise ValueError("score_doublets: rank must lie in [1, 1024]")
        _whole(maxit, 1, "maxit")
    pa, pb = doublet_parents(n_obs, n_sim, seed)

    def stage(c):
        if is_native:
            c.upload_native(A)
        else:
            c.upload(A, None)

    def embed(c, ws):
        c.log_normalize(float(scale_factor))
        if rows is not None:
            c.subset(rows=rows)
        c.fit_init(ws.shape[1], ws)
        c.step_h(L1f, L2f)
        return c.get_factors(w=False, d=False)[2]

    obs, sim = Context(0), None
    try:
        stage(obs)
        if nfeatures is not None:
            rows = obs.variable_features(nfeatures)["features"]
        if w is None:
            obs.log_normalize(float(scale_factor))
            if rows is not None:
                obs.subset(rows=rows)
            model = run_nmf(None, rank, tol, maxit, False, L1, L2, 0, seed=seed, _fits=_ResidentFits(None, ctx=obs))
            wb = np.ascontiguousarray(model["w"])
            stage(obs)   # the simulation needs the counts again
        ws, _ = obs.op_scale(wb)
        sim = Context(0)
        step = sim_batch if sim_batch else n_sim
        parts = []
        for s0 in range(0, n_sim, step):
            obs.simulate_doublets(sim, pa[s0:s0 + step], pb[s0:s0 + step])
            parts.append(np.array(embed(sim, ws)))
        H_sim = np.concatenate(parts, axis=0)
        H_obs = np.array(embed(obs, ws))
        E = np.ascontiguousarray(np.concatenate([H_obs, H_sim], axis=0).T)
        idx, _ = sim.knn(k_adj + 1, reference=E, **mkw)
    finally:
        obs.close()
        if sim is not None:
            sim.close()
    _refuse_short("score_doublets", idx)
    sc = doublet_scores(idx, n_obs, n_sim, rho, se_rho)
    if threshold is None:
        try:
            threshold = doublet_threshold(sc["sim_score"], bins)
        except ValueError as e:
            raise ValueError("score_doublets: no automatic threshold (%s)" % e) from e
    return {"scores": sc["score"], "se": sc["se"], "predicted": sc["score"] > float(threshold), "threshold": float(threshold),
            "parent_a": pa, "parent_b": pb, "sim_scores": sc["sim_score"], "sim_se": sc["sim_se"], "nd": sc["nd"],
            "sim_nd": sc["sim_nd"], "k_adj": k_adj, "h_obs": H_obs, "h_sim": H_sim, "w": wb}


# ---------------------------------------------------------------------------
# Gene set enrichment of the factors (RunGSEA, R/RunGSEA.R)
# ---------------------------------------------------------------------------
GSEA_SEED = 0x65EA


def c_gsea(w, set_ptr, set_genes, score_type="pos", nperm=1000, seed=GSEA_SEED, batch=0, timing=False):
    """The pre-ranked enrichment test of every gene set in every factor (sgl_c_gsea; the rules are stated in
    include/singlet_hip.h, "Gene set enrichment").  w: m genes x k factors; the sets as set_ptr (n_sets + 1 offsets) and
    set_genes (0-based gene indices).  Returns a dict of n_sets x k arrays "es", "nes", "pval", "padj", "n_ge", "n_le",
    "n_side", with "set_size" (n_sets), "info" ({"sets", "sizes", "s_max", "batches", "batch"}) and, with timing, "stage_ms"
    (rankings, observed scores, null sample, null scores, tallies).  batch: permutations per batch, 0 = by the memory budget;
    the results do not depend on it."""
    wt, m, k, sp, sg = gsea_inputs(w, set_ptr, set_genes)
    st = gsea_score_type(score_type)
    P = sp.shape[0] - 1
    shape = (max(k, 1), max(P, 1))
    f64s = {n: np.empty(shape) for n in ("es", "nes", "pval", "padj")}
    i64s = {n: np.zeros(shape, dtype=np.int64) for n in ("n_ge", "n_le", "n_side")}
    set_size = np.zeros(max(P, 1), dtype=np.int32)
    info = np.zeros(5, dtype=np.int64)
    stage_ms = np.zeros(5) if timing else None
    i64p = _lib.i64p
    check(_lib.load().sgl_c_gsea(ptr(wt, f64p), m, k, ptr(sp, i64p), ptr(sg, i32p), P, st, int(nperm), int(seed), int(batch),
                                 ptr(f64s["es"], f64p), ptr(f64s["nes"], f64p), ptr(f64s["pval"], f64p), ptr(f64s["padj"], f64p),
                                 ptr(i64s["n_ge"], i64p), ptr(i64s["n_le"], i64p), ptr(i64s["n_side"], i64p), ptr(set_size, i32p),
                                 ptr(info, i64p), ptr(stage_ms, f64p)))
    out = {n: a[:k, :P].T for n, a in {**f64s, **i64s}.items()}
    out["set_size"] = set_size[:P]
    out["info"] = dict(zip(("sets", "sizes", "s_max", "batches", "batch"), (int(v) for v in info)))
    if timing:
        out["stage_ms"] = stage_ms
    return out


def read_gmt(path):
    """A GMT file (one gene set per line: name, description, genes, tab-separated) as a dict name -> list of gene names, in
    file order; empty fields are dropped, a name that occurs twice keeps the genes of both lines.  Pure host."""
    sets = {}
    with open(path) as f:
        for line in f:
            cells = line.rstrip("\r\n").split("\t")
            if len(cells) < 2 or not cells[0]:
                continue
            sets.setdefault(cells[0], []).extend(g for g in cells[2:] if g)
    return sets


def gsea_filter(pathways, gene_names, w, min_size=10, max_size=500):
    """The filters of RunGSEA (R/RunGSEA.R:36-64) and of fgsea's own preparation, in their order.  pathways: dict name ->
    gene names; gene_names: the row names of w (m x k).  Returns (names, rows, sets, tested): the names of the sets RunGSEA
    hands to fgsea, the rows of w that stay (ascending), each set as indices into those rows (duplicates dropped, in order
    of first occurrence), and tested[j] = fgsea's own inclusive size filter min_size <= size <= max_size on what is left."""
    w = np.asarray(w)
    paths = {n: list(v) for n, v in pathways.items() if len(v) > min_size}                 # l.36: strictly longer
    in_paths = set(g for v in paths.values() for g in v)                                     # l.39
    keep = np.array([g in in_paths for g in gene_names], dtype=bool)                         # l.54
    kept_names = set(g for g, kk in zip(gene_names, keep) if kk)
    paths = {n: [g for g in v if g in kept_names] for n, v in paths.items()}                 # l.55
    paths = {n: v for n, v in paths.items() if min_size < len(v) < max_size}                 # l.56-57: both strict
    keep &= w.sum(axis=1) != 0                                                               # l.60-64: rows whose sum is 0 go
    rows = np.nonzero(keep)[0]
    index = {gene_names[g]: q for q, g in enumerate(rows.tolist())}
    names, sets, tested = [], [], []
    for n, v in paths.items():
        ids = list(dict.fromkeys(index[g] for g in v if g in index))                         # fgsea: unique genes of the ranking
        names.append(n)
        sets.append(np.asarray(ids, dtype=np.int32))
        tested.append(min_size <= len(ids) <= max_size)
    return names, rows, sets, np.asarray(tested, dtype=bool)


def run_gsea(w, pathways, gene_names, min_size=10, max_size=500, dims=None, score_type="pos", nperm=1000, seed=GSEA_SEED,
             padj_sig=0.01):
    """RunGSEA (R/RunGSEA.R:27-138) on the device: which gene sets are enriched in each factor.  w: m genes x k factors (a
    model's w); pathways: a dict name -> gene names, or the path of a GMT file (the reference fetches them from msigdbr, which
    needs a download); gene_names: the m row names of w; dims: the factors to test (0-based), None = all.  The filters are
    the reference's, in its order: keep the sets longer than min_size; restrict w to the genes of any kept set and the sets
    to those genes; keep the sets with min_size < size < max_size; drop the genes whose row of w sums to zero; then fgsea's
    own inclusive size filter on what is left -- a set failing it is a row of NaN, as padData leaves it.  Returns {"pval",
    "padj" (both as -log10), "es", "nes"}: sets x factors, with "pathways" (the row names), "dims", "significant" (the rows
    with a padj below padj_sig in some factor) and "genes" (the rows of w the test ran on).
    The test is the library's permutation test (sgl_c_gsea): ties of a factor go by gene index, the null is nperm random
    sets of each size.  NOT offered: the hclust display order of the rows and columns (as MetadataSummary leaves it out);
    add.noise (the tie rule removes its cause); remove.zeros.per.factor (a per-factor universe); fgseaMultilevel's p-values
    below 1 / (nperm + 1) -- the floor of this test is 1 / (nperm + 1): raise nperm to resolve smaller ones."""
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 2 or len(gene_names) != w.shape[0]:
        raise ValueError("run_gsea: gene_names must name the %s rows of w" % (w.shape[0] if w.ndim == 2 else "m"))
    if isinstance(pathways, (str, bytes)) or hasattr(pathways, "__fspath__"):
        pathways = read_gmt(pathways)
    st = gsea_score_type(score_type)
    gene_names = list(gene_names)
    dims = np.arange(w.shape[1]) if dims is None else np.asarray(dims, dtype=np.int64).ravel()
    w = w[:, dims]                                                                           # l.47
    names, rows, sets, tested = gsea_filter(pathways, gene_names, w, min_size, max_size)
    P, k = len(names), w.shape[1]
    out = {n: np.full((P, k), np.nan) for n in ("pval", "padj", "es", "nes")}
    run = np.nonzero(tested)[0]
    if run.size:
        set_ptr = np.concatenate([[0], np.cumsum([sets[j].size for j in run])]).astype(np.int64)
        res = c_gsea(w[rows], set_ptr, np.concatenate([sets[j] for j in run]), st, nperm, seed)
        for n in out:
            out[n][run] = res[n]
    with np.errstate(invalid="ignore"):
        sig = np.nonzero(np.nanmin(np.where(np.isnan(out["padj"]), np.inf, out["padj"]), axis=1, initial=np.inf) < padj_sig)[0]
        out["pval"], out["padj"] = -np.log10(out["pval"]), -np.log10(out["padj"])
    out.update(pathways=names, dims=dims, significant=sig, genes=rows)
    return out


# ---------------------------------------------------------------------------
# Factor annotation (R/AnnotateNMF.R, R/checkColumns.R, R/getDesigns.R, R/getModelMatrix.R, R/getModelFit.R, R/getModelResults.R)
# ---------------------------------------------------------------------------
def _meta_columns(meta):
    """{name: column} of a dict of arrays or a pandas DataFrame (recognised by its interface; pandas is not imported here)."""
    if isinstance(meta, dict):
        return dict(meta)
    if hasattr(meta, "columns") and hasattr(meta, "__getitem__"):
        return {c: meta[c] for c in meta.columns}
    raise ValueError("meta must be a dict of arrays or a pandas DataFrame, one value per cell in every column")


def _column_codes(col):
    """(int32 codes with -1 for a missing value, the level names) of one metadata column, or None when the column is not
    factor-like: a pandas Categorical (its categories, unused ones included, as nlevels counts them), strings / objects, booleans
    or integers -- levels: the sorted distinct values that are not missing (None, NaN, pandas NA), as as.factor orders them."""
    cat = getattr(col, "cat", None)
    if cat is None and hasattr(col, "categories") and hasattr(col, "codes"):
        cat = col
    if cat is not None:
        return np.asarray(cat.codes, dtype=np.int32), [c for c in cat.categories]
    a = np.asarray(col)
    if a.ndim != 1:
        return None
    if a.dtype.kind in "iub":
        levels, codes = np.unique(a, return_inverse=True)
        return codes.astype(np.int32), levels.tolist()
    if a.dtype.kind in "US":
        levels, codes = np.unique(a, return_inverse=True)
        return codes.astype(np.int32), levels.tolist()
    if a.dtype.kind == "O":
        missing = np.array([v is None or (isinstance(v, float) and v != v) or type(v).__name__ in ("NAType", "NaTType") for v in a], dtype=bool)
        vals = a[~missing]
        if any(isinstance(v, float) for v in vals):
            return None   # a numeric column that merely arrived as objects
        try:
            levels = sorted(set(vals.tolist()))
        except TypeError:
            return None
        index = {v: q for q, v in enumerate(levels)}
        codes = np.full(a.shape[0], -1, dtype=np.int32)
        codes[~missing] = [index[v] for v in vals.tolist()]
        return codes, levels
    return None   # floating point and everything else: not a factor


def check_columns(meta, columns=None, max_levels=200):
    """R/checkColumns.R: the names of the metadata columns an annotation can use -- present in meta, factor-like (categorical,
    string or integer-coded) and with 2 to max_levels levels.  The message about the discarded ones appears only when
    `columns` was given (l.10-19)."""
    cols = _meta_columns(meta)
    verbose = columns is not None
    if columns is None:
        columns = list(cols)
    elif isinstance(columns, str):
        columns = [columns]
    keep = []
    for name in columns:
        if name not in cols:
            continue
        coded = _column_codes(cols[name])
        if coded is None or len(coded[1]) < 2 or len(coded[1]) > max_levels:
            continue
        keep.append(name)
    discard = [c for c in columns if c not in keep]
    if verbose and discard:
        print("Some columns are not factors, or have only one level, or have more than max.levels levels.")
        print("Skipping `" + "`, `".join(str(c) for c in discard) + "`.")
    return keep


def get_designs(meta, columns=None, max_levels=200):
    """R/getDesigns.R + R/getModelMatrix.R in grouped form: {column: (labels, levels)} for every column check_columns keeps --
    labels int32, one per cell, the 0-based level of the cell or -1 where the value is missing (model.matrix drops those
    rows); levels the level names in code order.  A label list is to model.matrix(~ 0 + column) what set_links_grouped's
    group list is to a link matrix: column g of the design is labels == g."""
    cols = _meta_columns(meta)
    return {name: _column_codes(cols[name]) for name in check_columns(meta, columns, max_levels)}


def c_group_moments(F, labels, n_groups=None):
    """The one-shot form of Context.group_moments (sgl_c_group_moments): (group_n, sum k x G, rss k) of the means model over the
    columns of F (k x n on the host) under the labels, in a context of its own."""
    buf = colmajor(F, "F must be a k x n matrix")
    n, k = buf.shape
    g, G = label_list(labels, n, n_groups)
    kk, Gs = max(int(k), 1), max(min(G, 1024), 1)   # outside [1, 1024] the library refuses before it writes
    group_n, s, rss = np.zeros(Gs, dtype=np.int64), np.zeros((Gs, kk)), np.zeros(kk)
    check(_lib.load().sgl_c_group_moments(ptr(buf, f64p), int(k), int(n), ptr(g, i32p), G, ptr(group_n, _lib.i64p), ptr(s, f64p),
                                          ptr(rss, f64p)))
    return group_n, s[:, :k].T, rss[:k]


def annotate_stats(group_n, sums, rss, center=True, scale=False, proportion=0.01, tail="pos"):
    """The fit and the moderated statistics of a means model from its group moments (sgl_annotate_stats; host code of the
    library, no device needed): group_n G counts, sums rows x G, rss one value per row.  Returns the dict of the arrays:
    coefficients, t, p_raw, p_adj, lods (rows x G); Amean, sigma, s2_post (rows); stdev_unscaled, var_prior (G);
    df_residual, s2_prior, df_prior, df_total; the moments themselves."""
    s = np.asarray(sums, dtype=np.float64)
    if s.ndim != 2:
        raise ValueError("sums must be a rows x G matrix")
    L = _lib.load()
    return annotate_call(lambda *a: L.sgl_annotate_stats(s.shape[0], s.shape[1], *a), s.shape[0], s.shape[1], center, scale, proportion,
                         tail, moments=(group_n, s, rss))


def c_annotate(F, labels, n_groups=None, center=True, scale=False, proportion=0.01, tail="pos"):
    """The one-shot form of Context.annotate (sgl_c_annotate): F k x n on the host, in a context of its own."""
    buf = colmajor(F, "F must be a k x n matrix")
    n, k = buf.shape
    g, G = label_list(labels, n, n_groups)
    L = _lib.load()
    return annotate_call(lambda *a: L.sgl_c_annotate(ptr(buf, f64p), int(k), int(n), ptr(g, i32p), G, *a), k, G, center, scale,
                         proportion, tail)


def get_model_fit(labels, n_levels, obj, center=True, scale=False, genes=False):
    """R/getModelFit.R for the means model of one label list (get_designs): eBayes(lmFit(obj, design), proportion = 0.01) under
    the rules of include/singlet_hip.h ("Factor annotation"; not limma's robust = TRUE).  obj: a k x n array (transposed when
    it arrives n x k, l.36), a model dict (its "h"), a Context (its held embedding or the H of its fit; with genes = True the
    genes of its resident matrix), or a sparse matrix / native(...) object for the fit of every gene (l.27).  Returns a dict
    with limma's field names where they exist -- coefficients, stdev_unscaled, sigma, df_residual, Amean, s2_prior, df_prior,
    s2_post, df_total, t, p_value (two-sided), lods, var_prior, centered -- and the group moments the statistics came from."""
    from .context import Context
    labels = np.asarray(labels)
    kw = dict(center=center, scale=scale, proportion=0.01, tail="std")
    if isinstance(obj, Context):
        fit = obj.annotate_genes(labels, n_levels, **kw) if genes else obj.annotate(labels, n_levels, None, **kw)
    elif isinstance(obj, NativeMatrix):
        fit = _on_native(obj, lambda ctx, fits: ctx.annotate_genes(labels, n_levels, **kw))
    elif isinstance(obj, dgCMatrix) or hasattr(obj, "tocsc"):
        with Context(0) as ctx:
            ctx.upload(as_dgCMatrix(obj))
            fit = ctx.annotate_genes(labels, n_levels, **kw)
    else:
        F = np.asarray(obj["h"] if isinstance(obj, dict) else obj, dtype=np.float64)
        if F.ndim != 2:
            raise ValueError("obj must be a k x n matrix, a model, a Context or a sparse matrix")
        if F.shape[1] < labels.shape[0]:
            F = F.T   # if (ncol(dat) < nrow(design)) dat <- t(dat)
        fit = c_annotate(F, labels, n_levels, **kw)
    fit["p_value"] = fit.pop("p_raw")
    fit["_p_adj_std"] = fit.pop("p_adj")   # the two-sided table's adjusted p: get_model_results(tail = "std") reads it
    del fit["tail"]
    return fit


def get_model_results(fit, noneg=True, noint=True, tail="pos", names=None):
    """R/getModelResults.R:23-55: the long table (group, factor, fc, p) of a fit -- fc the log-odds, p the one-sided moderated p
    of `tail` ("pos", "neg" or "std": two-sided) adjusted by Benjamini-Hochberg over the WHOLE table before any filter; rows
    with lods <= 0 are dropped when noneg, a group named "(Intercept)" when noint (a means model has none).  Rows run over the
    groups, the factors ascending within a group (melt's order).  names: (group names, factor names), either may be None;
    they are added as "group_names" and "factor_names".  Returns a dict of equally long arrays."""
    annotate_tail(tail)   # "Invalid tail selection. Choose 'pos','neg', or 'std'"
    if tail == "std" and "_p_adj_std" in fit:   # the fit holds the two-sided p already; a one-sided tail is formed from the moments
        lods, p = fit["lods"], fit["_p_adj_std"]
    else:
        st = annotate_stats(fit["group_n"], fit["sum"], fit["rss"], fit["centered"], fit["scaled"], fit["proportion"], tail)
        lods, p = st["lods"], st["p_adj"]
    rows, G = lods.shape
    group, factor = np.repeat(np.arange(G), rows), np.tile(np.arange(rows), G)
    keep = np.ones(rows * G, dtype=bool)
    fc, pv = lods.T.reshape(-1), p.T.reshape(-1)
    if noneg:
        with np.errstate(invalid="ignore"):
            keep &= fc > 0
    gnames, fnames = names if names is not None else (None, None)
    if noint and gnames is not None:
        keep &= np.array([gnames[g] != "(Intercept)" for g in group], dtype=bool)
    if not keep.any():
        print("No associations after filtering.")
    out = {"group": group[keep].astype(np.int32), "factor": factor[keep].astype(np.int32), "fc": fc[keep], "p": pv[keep]}
    if gnames is not None:
        out["group_names"] = [gnames[g] for g in out["group"]]
    if fnames is not None:
        out["factor_names"] = [fnames[f] for f in out["factor"]]
    return out


def AnnotateNMF(model_or_context, meta, columns=None, center=True, scale=False, max_levels=200, tail="pos"):
    """R/AnnotateNMF.R:29-41 without the object around it: {column: table}, the content of misc$annotations -- for every usable
    metadata column (check_columns) the table get_model_results gives for the means-model fit of the factors against it.
    model_or_context: a model dict (its "h", k x n, uploaded ONCE and held on the device for all columns) or a Context (its
    held embedding or the H of its fit, read in place)."""
    from .context import Context
    annotate_tail(tail)
    designs = get_designs(meta, columns, max_levels)

    def run(ctx, fnames):
        out = {}
        for name, (labels, levels) in designs.items():
            fit = get_model_fit(labels, len(levels), ctx, center, scale)
            out[name] = get_model_results(fit, tail=tail, names=(levels, fnames))
        return out

    if isinstance(model_or_context, Context):
        return run(model_or_context, None)
    h = np.asarray(model_or_context["h"], dtype=np.float64)
    fnames = model_or_context.get("factor_names") if isinstance(model_or_context, dict) else None
    with Context(0) as ctx:
        ctx.hold_embedding(h)
        return run(ctx, fnames)


# ---------------------------------------------------------------------------
# Spatial autocorrelation (Moran's I of genes and factors over a cell graph)
# ---------------------------------------------------------------------------
MORAN_VARIANCES = ("randomisation", "normality")
MORAN_ALTERNATIVES = ("two.sided", "greater", "less")


def _moran_choice(value, choices, what):
    if value not in choices:
        raise ValueError("%s must be one of %s, not %r" % (what, ", ".join(repr(c) for c in choices), value))
    return choices.index(value)


def moran_graph_moments(G):
    """{"S0", "S1", "S2", "t"} of the n x n cell graph G (sgl_moran_graph_moments; host code of the library, no device
    needed): the sums of Cliff & Ord in the stated sequential orders, t[i] = rowsum_i + colsum_i.  The graph is used as given.
    A graph whose weights sum to zero is refused."""
    G = _square_graph(G, "moran_graph_moments")
    s, t = np.zeros(3), np.zeros(max(G.ncol, 1))
    f = lambda q: ptr(s[q:], f64p)
    check(_lib.load().sgl_moran_graph_moments(*csc_ptrs(G), G.ncol, f(0), f(1), f(2), ptr(t, f64p)))
    return {"S0": float(s[0]), "S1": float(s[1]), "S2": float(s[2]), "t": t[:G.ncol]}


def moran_stats(n, S0, S1, S2, moments, variance="randomisation", alternative="two.sided"):
    """Moran's I and its test from the graph moments and the per-row moments (sgl_moran_stats; host code of the library, no
    device needed).  moments: 6 x rows (mean, M2, M4, T, P, c) as Context.moran returns them.  Returns {"I", "EI", "sd", "z",
    "p", "p_adj"}, one value per row; a constant row has NaN for I, z and p; p_adj is Benjamini-Hochberg over the others."""
    v, a = _moran_choice(variance, MORAN_VARIANCES, "variance"), _moran_choice(alternative, MORAN_ALTERNATIVES, "alternative")
    mo = np.asarray(moments, dtype=np.float64)
    if mo.ndim != 2 or mo.shape[0] != 6:
        raise ValueError("moments must be a 6 x rows matrix (mean, M2, M4, T, P, c)")
    buf = np.ascontiguousarray(mo.T)
    rows = buf.shape[0]
    out = [np.zeros(max(rows, 1)) for _ in range(6)]
    check(_lib.load().sgl_moran_stats(int(n), float(S0), float(S1), float(S2), rows, ptr(buf, f64p), v, a, *(ptr(o, f64p) for o in out)))
    return dict(zip(("I", "EI", "sd", "z", "p", "p_adj"), (o[:rows] for o in out)))


def c_moran(A, G, genes=None):
    """The one-shot form of Context.moran (sgl_c_moran): A a dgCMatrix or anything as_dgCMatrix accepts, in a context of its
    own.  Returns the 6 x n_genes moments."""
    from .context import Context
    A, G = as_dgCMatrix(A), _square_graph(G, "c_moran")
    g, ng = Context._gene_list(genes, "c_moran")
    rows = ng if genes is not None else A.nrow
    out = np.zeros((max(rows, 1), 6))
    check(_lib.load().sgl_c_moran(*csc_ptrs(A), A.nrow, A.ncol, *csc_ptrs(G), G.ncol, ptr(g, i32p), ng, ptr(out, f64p)))
    return out[:rows].T


def c_moran_embedding(F, G):
    """The one-shot form of Context.moran_embedding (sgl_c_moran_embedding): F k x n on the host, in a context of its own.
    Returns (moments 6 x k, mean k)."""
    G = _square_graph(G, "c_moran_embedding")
    buf = colmajor(F, "F must be a k x n matrix")
    n, k = buf.shape
    if n != G.ncol:
        raise ValueError("c_moran_embedding: F has %d columns, the graph %d cells" % (n, G.ncol))
    kk = max(min(int(k), 1024), 1)
    out, mean = np.zeros((kk, 6)), np.zeros(kk)
    check(_lib.load().sgl_c_moran_embedding(*csc_ptrs(G), G.ncol, ptr(buf, f64p), int(k), ptr(out, f64p), ptr(mean, f64p)))
    return out[:k].T, mean[:k]


def _moran_front(who, n, graph, coords, max_dist, max_k, variance, alternative, nfeatures):
    """The refusals of the front-ends, all before the first upload; returns a function that builds the graph."""
    _moran_choice(variance, MORAN_VARIANCES, "%s: variance" % who)
    _moran_choice(alternative, MORAN_ALTERNATIVES, "%s: alternative" % who)
    if nfeatures is not None and (int(nfeatures) != nfeatures or nfeatures < 1):
        raise ValueError("%s: nfeatures = %r: at least one feature is ranked" % (who, nfeatures))
    if (graph is None) == (coords is None):
        raise ValueError("%s: exactly one of graph and coords (+ max_dist) must be given" % who)
    if n < 4:
        raise ValueError("%s: %d cells: the variance of Moran's I needs at least 4" % (who, n))
    if graph is not None:
        if max_dist is not None:
            raise ValueError("%s: max_dist belongs to coords; a graph is used as it is" % who)
        G = _square_graph(graph, who)
        if G.ncol != n:
            raise ValueError("%s: the graph has %d cells, the data %d" % (who, G.ncol, n))
        return lambda: G
    xy = np.asarray(coords, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] != n:
        raise ValueError("%s: coords must be an n x 2 matrix with one row per cell (%d), not %r" % (who, n, xy.shape))
    if max_dist is None or not max_dist > 0:
        raise ValueError("%s: coords needs a positive max_dist" % who)
    return lambda: spatial_graph(xy[:, 0], xy[:, 1], max_dist, max_k)


def _moran_table(n, G, moments, variance, alternative):
    gm = moran_graph_moments(G)
    st = moran_stats(n, gm["S0"], gm["S1"], gm["S2"], moments, variance, alternative)
    st["moments"] = moments
    st["graph_moments"] = {q: gm[q] for q in ("S0", "S1", "S2")}
    return st


def moran_rank(p, I, genes):
    """The order of find_spatially_variable_features: p ascending, I descending, gene index ascending; NaN rows last."""
    p, I, genes = np.asarray(p), np.asarray(I), np.asarray(genes)
    bad = np.isnan(p) | np.isnan(I)
    return np.lexsort((genes, np.where(bad, 0.0, -I), np.where(bad, np.inf, p), bad))


def find_spatially_variable_features(A, graph=None, coords=None, max_dist=None, max_k=100, features=None, nfeatures=2000,
                                     variance="randomisation", alternative="two.sided", drop_diagonal=True):
    """Seurat::FindSpatiallyVariableFeatures(selection.method = "moransi") on the device: Moran's I of every gene (or of
    `features`, distinct 0-based gene indices) over a cell graph, with its expectation, standard deviation, z, p and
    Benjamini-Hochberg p_adj (sgl_moran; the rules are stated in include/singlet_hip.h, "Spatial autocorrelation" -- this
    library's own statement of the published definitions, no parity with ape is claimed).  A: anything RunNMF takes, or a
    Context that holds the matrix.  Exactly one of graph (an n x n sparse matrix, used as it is but for its diagonal, which
    drop_diagonal removes) and coords (n x 2, turned into spatial_graph(coords, max_dist, max_k)).  Returns {"genes" (the tested
    gene indices), "I", "EI", "sd", "z", "p", "p_adj", "moments", "graph_moments", "features": the first nfeatures tested genes
    ranked by (p ascending, I descending, gene index ascending), NaN rows last}.  Every argument is refused before the first
    upload."""
    from .context import Context
    who = "find_spatially_variable_features"
    is_ctx = isinstance(A, Context)
    if not is_ctx and not isinstance(A, NativeMatrix):
        A = as_dgCMatrix(A)
    m, n = A.dims()[:2] if is_ctx else (A.nrow, A.ncol)
    build = _moran_front(who, n, graph, coords, max_dist, max_k, variance, alternative, nfeatures)
    g, ng = Context._gene_list(features, who)
    if features is not None:
        if ng and (g[:ng].min() < 0 or g[:ng].max() >= m):
            raise ValueError("%s: a feature index is outside [0, %d)" % (who, m))
        if np.unique(g[:ng]).shape[0] != ng:
            raise ValueError("%s: features holds a gene twice" % who)
    G = build()
    if drop_diagonal:
        G = _without_diagonal(G)
    genes = np.arange(m, dtype=np.int32) if features is None else g[:ng].copy()
    if is_ctx:
        moments = A.moran(G, features)
    elif isinstance(A, NativeMatrix):
        moments = _on_native(A, lambda ctx, fits: ctx.moran(G, features))
    else:
        moments = c_moran(A, G, features)
    out = _moran_table(n, G, moments, variance, alternative)
    out["genes"] = genes
    out["features"] = genes[moran_rank(out["p"], out["I"], genes)][:int(nfeatures)]
    return out


def moran_factors(h_or_context, graph, variance="randomisation", alternative="two.sided", drop_diagonal=True):
    """The table of find_spatially_variable_features for the factors: Moran's I of every row of h (k x n, or a model dict's
    "h") or, for a Context, of its held embedding or else the H of its fit, read in place (sgl_moran_embedding).  Returns
    {"I", "EI", "sd", "z", "p", "p_adj", "mean", "moments", "graph_moments"}, one value per factor."""
    from .context import Context
    who = "moran_factors"
    is_ctx = isinstance(h_or_context, Context)
    G = _square_graph(graph, who)
    _moran_front(who, G.ncol, G, None, None, None, variance, alternative, None)
    if not is_ctx:
        h = h_or_context["h"] if isinstance(h_or_context, dict) else h_or_context
        h = np.asarray(h, dtype=np.float64)
        if h.ndim != 2 or h.shape[1] != G.ncol:
            raise ValueError("%s: h must be k x n with one column per cell of the graph (%d), not %r" % (who, G.ncol, h.shape))
    if drop_diagonal:
        G = _without_diagonal(G)
    moments, mean = h_or_context.moran_embedding(G, None) if is_ctx else c_moran_embedding(h, G)
    out = _moran_table(G.ncol, G, moments, variance, alternative)
    out["mean"] = mean
    return out


# ---------------------------------------------------------------------------
# Neighbourhood enrichment (which clusters sit next to which on a cell graph; include/singlet_hip.h, "Neighbourhood enrichment")
# ---------------------------------------------------------------------------
def nhood_stats(nperm, counts, S1, S2, n_ge, n_le):
    """z, mean, sd, the two p and their Benjamini-Hochberg adjustments from the integer tallies of a neighbourhood enrichment
    call (sgl_nhood_stats; host code of the library, no device needed).  Every table is K x K, [a, b] = centre class a, neighbour
    class b.  Returns {"zscore", "mean", "sd", "p_enriched", "p_depleted", "p_adj_enriched", "p_adj_depleted"}; z is NaN where
    every permutation gave the same count."""
    t = [np.asarray(a) for a in (counts, S1, S2, n_ge, n_le)]
    K = t[0].shape[0] if t[0].ndim == 2 else 0
    if K < 1 or any(a.shape != (K, K) or a.dtype.kind not in "iu" for a in t):
        raise ValueError("nhood_stats: counts, S1, S2, n_ge and n_le must be K x K integer tables")
    t = [np.ascontiguousarray(a.T, dtype=np.int64) for a in t]
    out = [np.zeros((K, K)) for _ in NHOOD_STATS]
    check(_lib.load().sgl_nhood_stats(K, int(nperm), *(ptr(a, _lib.i64p) for a in t), *(ptr(o, f64p) for o in out)))
    return {name: np.ascontiguousarray(o.T) for name, o in zip(NHOOD_STATS, out)}


def c_nhood_enrichment(G, labels, n_classes=None, nperm=1000, seed=0, drop_diagonal=True, batch=0, return_null=False, timing=False):
    """The one-shot form of Context.nhood_enrichment (sgl_c_nhood_enrichment), in a context of its own: the tallies and the
    statistics of nhood_stats in one dict, plus "info" (Context.nhood_info's fields); with return_null "null" (nperm x K x K),
    with timing "stage_ms" (keys + sort + gather, tallies, reduction)."""
    G = _square_graph(G, "c_nhood_enrichment")
    lab, K = nhood_labels(labels, G.ncol, n_classes, "c_nhood_enrichment")
    kk = max(min(K, 256), 1)
    t = [np.zeros((kk, kk), dtype=np.int64) for _ in NHOOD_TALLIES]
    st = [np.zeros((kk, kk)) for _ in NHOOD_STATS]
    null = np.zeros((max(min(int(nperm), 1 << 20), 1), kk, kk), dtype=np.int64) if return_null else None
    info, ms = np.zeros(6, dtype=np.int64), (np.zeros(3) if timing else None)
    i64p = _lib.i64p
    check(_lib.load().sgl_c_nhood_enrichment(ptr(G.i, i32p), ptr(G.p, i32p), G.ncol, ptr(lab, i32p), K, int(bool(drop_diagonal)), int(nperm), int(seed),
                                             int(batch), *(ptr(a, i64p) for a in t), ptr(null, i64p), *(ptr(o, f64p) for o in st), ptr(info, i64p),
                                             ptr(ms, f64p)))
    out = {name: np.ascontiguousarray(a.T) for name, a in zip(NHOOD_TALLIES + NHOOD_STATS, t + st)}
    out["info"] = dict(zip(NHOOD_INFO, (int(v) for v in info)))
    if return_null:
        out["null"] = np.ascontiguousarray(null.transpose(0, 2, 1))
    if timing:
        out["stage_ms"] = ms
    return out


def _nhood_graph(who, n, graph, coords, max_dist, max_k):
    """The refusals of the graph arguments; returns a function that builds the graph (the first upload happens there)."""
    if (graph is None) == (coords is None):
        raise ValueError("%s: exactly one of graph and coords (+ max_dist) must be given" % who)
    if graph is not None:
        if max_dist is not None:
            raise ValueError("%s: max_dist belongs to coords; a graph is used as it is" % who)
        if isinstance(graph, dict):
            if graph.get("snn") is None:
                raise ValueError("%s: the neighbours were computed without an SNN graph (compute_snn=False)" % who)
            graph = graph["snn"]
        G = _square_graph(graph, who)
        if G.ncol != n:
            raise ValueError("%s: the graph has %d cells, the labels %d" % (who, G.ncol, n))
        return lambda: G
    xy = np.asarray(coords, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] != n:
        raise ValueError("%s: coords must be an n x 2 matrix with one row per cell (%d), not %r" % (who, n, xy.shape))
    if max_dist is None or not max_dist > 0:
        raise ValueError("%s: coords needs a positive max_dist" % who)
    return lambda: spatial_graph(xy[:, 0], xy[:, 1], max_dist, max_k)


def _nhood_classes(who, labels, n_classes):
    lab, K = nhood_labels(labels, None, n_classes, who)
    if not 1 <= K <= 256:
        raise ValueError("%s: %d classes: between 1 and 256 are taken" % (who, K))
    if lab.min() < 0 or lab.max() >= K:
        at = int(np.nonzero((lab < 0) | (lab >= K))[0][0])
        raise ValueError("%s: labels[%d] = %d is outside [0, %d)" % (who, at, int(lab[at]), K))
    return lab, K


def nhood_enrichment(labels, graph=None, coords=None, max_dist=None, max_k=100, n_classes=None, nperm=1000, seed=0, drop_diagonal=True,
                     batch=0):
    """Which clusters sit next to which on a cell graph, more or less often than under a random relabelling: the permutation
    test of squidpy's gr.nhood_enrichment / Giotto's cellProximityEnrichment on the device (sgl_c_nhood_enrichment; the rules are
    stated in include/singlet_hip.h, "Neighbourhood enrichment" -- this library's own statement of the published scheme with its
    own permutations, NO parity with squidpy's seeded shuffles is claimed).  labels: one integer class in [0, n_classes) per cell
    (a column of find_clusters' "clusters"); n_classes None: 1 + the largest label.  Exactly one of graph (any SciPy matrix or
    dgCMatrix, or the dict find_neighbors returns, whose "snn" is used; the stored entries count, not their values) and coords
    (n x 2, turned into spatial_graph(coords, max_dist, max_k)).  drop_diagonal leaves self-loops out.  Returns {"counts",
    "zscore", "mean", "sd", "p_enriched", "p_depleted", "p_adj_enriched", "p_adj_depleted", "n_ge", "n_le", "class_sizes"}, K x K
    tables with [a, b] = centre class a, neighbour class b.  Every argument is refused before the first upload."""
    who = "nhood_enrichment"
    lab, K = _nhood_classes(who, labels, n_classes)
    if int(nperm) != nperm or not 1 <= nperm <= 1 << 20:
        raise ValueError("%s: nperm = %r is outside [1, 2^20]" % (who, nperm))
    if int(batch) != batch or batch < 0:
        raise ValueError("%s: batch = %r is negative" % (who, batch))
    if int(seed) != seed or not 0 <= seed < 2**64:
        raise ValueError("%s: seed = %r is no unsigned 64-bit integer" % (who, seed))
    build = _nhood_graph(who, lab.shape[0], graph, coords, max_dist, max_k)
    res = c_nhood_enrichment(build(), lab, K, nperm, seed, drop_diagonal, batch)
    out = {name: res[name] for name in ("counts",) + NHOOD_STATS + ("n_ge", "n_le")}
    out["class_sizes"] = np.bincount(lab, minlength=K).astype(np.int64)
    return out


def interaction_matrix(labels, graph, normalized=False, n_classes=None, drop_diagonal=True):
    """squidpy's gr.interaction_matrix: the observed class-pair counts of the stored entries of `graph` alone, K x K with [a, b] =
    centre class a, neighbour class b (sgl_op_nhood_tally on the labels as they are; no permutation is drawn).  graph as in
    nhood_enrichment.  normalized divides every row by its sum on the host (a row without entries stays 0) and returns doubles."""
    from .context import Context
    who = "interaction_matrix"
    lab, K = _nhood_classes(who, labels, n_classes)
    G = _nhood_graph(who, lab.shape[0], graph, None, None, None)()
    with Context(0) as ctx:
        counts = ctx.op_nhood_tally(G, lab[None, :], K, drop_diagonal)[0]
    if not normalized:
        return counts
    rows = counts.sum(axis=1, keepdims=True)
    return np.divide(counts, rows, out=np.zeros(counts.shape), where=rows > 0)


# ---------------------------------------------------------------------------
# Ligand-receptor interactions between clusters (CellPhoneDB's / squidpy's gr.ligrec permutation test; include/singlet_hip.h,
# "Ligand-receptor interactions")
# ---------------------------------------------------------------------------
def ligrec_stats(nperm, group_n, nz, lig, rec, n_ge, threshold=0.01, per_interaction=False):
    """The expressed mask, p and its Benjamini-Hochberg adjustment from the tallies of a ligand-receptor call (sgl_ligrec_stats;
    host code of the library, no device needed).  group_n K, nz G x K, n_ge P x K x K ([q, a, b] = ligand class a, receptor class
    b), lig / rec indices into the G genes.  p = (1 + n_ge) / (1 + nperm) where ligand and receptor are expressed (nz / n_c >=
    threshold), NaN elsewhere; padj over all P K^2 values, or with per_interaction over the K^2 of every pair alone.  Returns
    {"expressed" (G x K bool), "p", "padj" (P x K x K)}."""
    gn, z, ge = np.asarray(group_n), np.asarray(nz), np.asarray(n_ge)
    lg, rc = np.asarray(lig), np.asarray(rec)
    if gn.ndim != 1 or z.ndim != 2 or ge.ndim != 3 or lg.ndim != 1 or lg.shape != rc.shape or any(a.dtype.kind not in "iu" for a in (gn, z, ge, lg, rc)):
        raise ValueError("ligrec_stats: group_n (K), nz (G x K), n_ge (P x K x K), lig and rec (P) must be integer arrays")
    K, G, P = int(gn.shape[0]), int(z.shape[0]), int(lg.shape[0])
    if K < 1 or G < 1 or P < 1 or z.shape != (G, K) or ge.shape != (P, K, K):
        raise ValueError("ligrec_stats: group_n (K), nz (G x K), n_ge (P x K x K), lig and rec (P) must agree in K, G and P")
    gn, z = np.ascontiguousarray(gn, dtype=np.int64), np.ascontiguousarray(z, dtype=np.int64)
    ge = np.ascontiguousarray(ge.transpose(2, 1, 0), dtype=np.int64)
    lg, rc = np.ascontiguousarray(lg, dtype=np.int32), np.ascontiguousarray(rc, dtype=np.int32)
    ex, p, padj = np.zeros((G, K), dtype=np.uint8), np.zeros((K, K, P)), np.zeros((K, K, P))
    i64p = _lib.i64p
    check(_lib.load().sgl_ligrec_stats(K, G, P, int(nperm), ptr(gn, i64p), ptr(z, i64p), ptr(lg, i32p), ptr(rc, i32p), ptr(ge, i64p), float(threshold),
                                       int(bool(per_interaction)), ptr(ex, _lib.u8p), ptr(p, f64p), ptr(padj, f64p)))
    return {"expressed": ex.astype(bool), "p": np.ascontiguousarray(p.transpose(2, 1, 0)), "padj": np.ascontiguousarray(padj.transpose(2, 1, 0))}


def c_ligrec(A, labels, genes, lig, rec, n_classes=None, threshold=0.01, nperm=1000, seed=0, batch=0, per_interaction=False, return_null=False):
    """The one-shot form of Context.ligrec (sgl_c_ligrec): A a dgCMatrix or anything as_dgCMatrix accepts, in a context of its
    own.  The dict of Context.ligrec plus the statistics of ligrec_stats, "info" (Context.ligrec_info's fields) and "stage_ms"
    (labels, sums, tally)."""
    A = as_dgCMatrix(A)
    lab, K, g, G, lg, rc, P = ligrec_inputs(labels, A.ncol, n_classes, genes, lig, rec, "c_ligrec")
    L = _lib.load()
    return ligrec_call(lambda *a: L.sgl_c_ligrec(*csc_ptrs(A), A.nrow, A.ncol, ptr(lab, i32p), K, ptr(g, i32p), G, ptr(lg, i32p), ptr(rc, i32p), P,
                                                 int(nperm), int(seed), int(batch), float(threshold), int(bool(per_interaction)), *a),
                       K, G, P, nperm, return_null, with_stats=True)


def read_interactions(path):
    """The (ligand, receptor) name pairs of a two-column tab-separated file: one pair per line; empty lines and lines that
    start with '#' are skipped; a line without exactly two non-empty columns is refused with its number."""
    pairs = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            cols = [c.strip() for c in line.split("\t")]
            if len(cols) != 2 or not cols[0] or not cols[1]:
                raise ValueError("read_interactions: %s line %d: a ligand and a receptor separated by one tab" % (path, no))
            pairs.append((cols[0], cols[1]))
    return pairs


def ligrec_parse(interactions, gene_names=None, nrow=None, missing="error"):
    """The host half of ligrec: interactions = a list of (ligand, receptor) -- names looked up in gene_names (the first row of a
    name that occurs twice), or 0-based int rows in [0, nrow) when gene_names is None.  A pair with a name absent from
    gene_names is dropped and reported (missing="skip") or refused (missing="error").  Returns (genes, lig, rec, pairs,
    dropped): the distinct rows in order of first use, the pairs as indices into them, the kept pairs as given."""
    if missing not in ("skip", "error"):
        raise ValueError("ligrec: missing must be 'skip' or 'error'")
    try:
        given = [tuple(p) for p in interactions]
    except TypeError:
        given = None
    if not given or any(len(p) != 2 for p in given):
        raise ValueError("ligrec: interactions must be a non-empty list of (ligand, receptor) pairs")
    index = None
    if gene_names is not None:
        index = {}
        for r, g in enumerate(gene_names):
            index.setdefault(g.decode() if isinstance(g, bytes) else str(g), r)
        nrow = len(gene_names)
    rows, slot, lig, rec, kept, dropped = [], {}, [], [], [], []
    for pair in given:
        at = []
        for g in pair:
            if index is not None:
                r = index.get(g.decode() if isinstance(g, bytes) else str(g))
            else:
                if isinstance(g, (str, bytes)) or int(g) != g or not 0 <= int(g) < nrow:
                    raise ValueError("ligrec: %r is no gene row in [0, %d) (give gene_names to use names)" % (g, nrow))
                r = int(g)
            at.append(r)
        if None in at:
            if missing == "error":
                raise ValueError("ligrec: %r of the pair %r is not among the genes of the matrix (missing='skip' drops such pairs)"
                                 % (pair[at.index(None)], pair))
            dropped.append(pair)
            continue
        for r in at:
            if r not in slot:
                slot[r] = len(rows)
                rows.append(r)
        lig.append(slot[at[0]])
        rec.append(slot[at[1]])
        kept.append(pair)
    if not kept:
        raise ValueError("ligrec: no pair is left: none has both genes in the matrix")
    return np.array(rows, dtype=np.int32), np.array(lig, dtype=np.int32), np.array(rec, dtype=np.int32), kept, dropped


def ligrec(A, labels, interactions, gene_names=None, threshold=0.01, nperm=1000, seed=0, n_classes=None, missing="error", per_interaction=False,
           batch=0):
    """Which ligand-receptor pairs are expressed between which pairs of clusters more strongly than under a random relabelling
    of the cells: the permutation test of CellPhoneDB and of squidpy's gr.ligrec on the device (sgl_ligrec; the rules are stated in
    include/singlet_hip.h, "Ligand-receptor interactions" -- this library's own statement with its own relabellings, NO parity with
    squidpy's or CellPhoneDB's seeded shuffles, no multi-subunit complexes, no interaction database).  A: a dgCMatrix, anything
    as_dgCMatrix accepts, a native(...) object, or a Context that holds the (normally log-normalised) matrix.  labels: one integer
    class in [0, n_classes) per cell.  interactions: a list of (ligand, receptor) gene names (int rows when there are no
    gene_names), or the path of a two-column TSV file (read_interactions).  gene_names None: the row names of A when it has
    them.  missing "error" refuses a pair with a name that is not in the matrix, "skip" drops and reports it.  Every argument is
    refused before the first upload.  Returns {"means", "p", "padj" (P x K x K; [q, a, b] = ligand in class a, receptor in class b;
    means is the score, p is NaN where ligand or receptor is expressed in less than `threshold` of the class), "expressed"
    (P x K x K bool), "pairs", "dropped", "n_ge", "class_sizes"}."""
    from .context import Context
    who = "ligrec"
    if isinstance(interactions, (str, bytes, os.PathLike)):
        interactions = read_interactions(interactions)
    is_ctx, is_native = isinstance(A, Context), isinstance(A, NativeMatrix)
    if not is_ctx and not is_native:
        A = as_dgCMatrix(A)
    if gene_names is None and not is_ctx and A.Dimnames[0] is not None:
        gene_names = A.Dimnames[0]
    nrow, ncol = (A.dims()[0], A.dims()[1]) if is_ctx else (A.nrow, A.ncol)
    if gene_names is not None and len(gene_names) != nrow:
        raise ValueError("%s: gene_names must name the %d rows of the matrix" % (who, nrow))
    lab, K = _nhood_classes(who, labels, n_classes)
    if lab.shape[0] != ncol:
        raise ValueError("%s: %d labels, the matrix has %d cells" % (who, lab.shape[0], ncol))
    if int(nperm) != nperm or not 1 <= nperm <= 1 << 20:
        raise ValueError("%s: nperm = %r is outside [1, 2^20]" % (who, nperm))
    if int(batch) != batch or batch < 0:
        raise ValueError("%s: batch = %r is negative" % (who, batch))
    if int(seed) != seed or not 0 <= seed < 2**64:
        raise ValueError("%s: seed = %r is no unsigned 64-bit integer" % (who, seed))
    if not 0.0 <= float(threshold) <= 1.0:
        raise ValueError("%s: threshold = %r is outside [0, 1]" % (who, threshold))
    genes, lg, rc, kept, dropped = ligrec_parse(interactions, gene_names, nrow, missing)

    def on(ctx):
        t = ctx.ligrec(lab, genes, lg, rc, K, nperm, seed, batch)
        t.update(ligrec_stats(nperm, t["group_n"], t["nz"], lg, rc, t["n_ge"], threshold, per_interaction))
        return t
    if is_ctx:
        t = on(A)
    elif is_native:
        t = _on_native(A, lambda ctx, fits: on(ctx))
    else:
        t = c_ligrec(A, lab, genes, lg, rc, K, threshold, nperm, seed, batch, per_interaction)
    ex = t["expressed"]
    return {"means": t["score"], "p": t["p"], "padj": t["padj"], "expressed": ex[lg][:, :, None] & ex[rc][:, None, :], "pairs": kept,
            "dropped": dropped, "n_ge": t["n_ge"], "class_sizes": t["group_n"]}


# ---------------------------------------------------------------------------
# Co-occurrence of clusters by distance (squidpy's gr.co_occurrence score, Ripley's K / L; include/singlet_hip.h, "Co-occurrence by
# distance")
# ---------------------------------------------------------------------------
def _cooccur_table(counts, who):
    t = np.asarray(counts)
    if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[0] < 1 or t.shape[2] < 1 or t.dtype.kind not in "iu":
        raise ValueError("%s: counts must be a K x K x T integer table" % who)
    from ._cooccur import tba
    return tba(t.astype(np.int64)), int(t.shape[0]), int(t.shape[2])


def cooccur_stats(counts, cumulative=False):
    """The co-occurrence ratio of a K x K x T tally (sgl_cooccur_stats; host code of the library, no device needed): [a, b, t] =
    P(b | within interval t of an a) / P(b among all pairs of interval t), of the intervals or with `cumulative` of their running
    sums; NaN where class a or b has no pair.  A table that is not symmetric with an even diagonal is refused."""
    from ._cooccur import abt, table_shape
    buf, K, T = _cooccur_table(counts, "cooccur_stats")
    out = np.zeros(table_shape(K, T))
    check(_lib.load().sgl_cooccur_stats(K, T, ptr(buf, _lib.i64p), int(bool(cumulative)), ptr(out, f64p)))
    return abt(out, K, T)


def ripley_stats(counts, group_n, area):
    """Ripley's K and L of every class from the cumulative diagonal of a K x K x T tally (sgl_ripley_stats; host code):
    {"K", "L"}, K x T each; NaN for a class of fewer than two points.  No edge correction."""
    buf, K, T = _cooccur_table(counts, "ripley_stats")
    g = np.asarray(group_n)
    if g.shape != (K,) or g.dtype.kind not in "iu":
        raise ValueError("ripley_stats: group_n must hold one integer count per class (%d)" % K)
    g = np.ascontiguousarray(g, dtype=np.int64)
    kk, tt = max(min(K, 256), 1), max(min(T, 64), 1)
    Kf, L = np.zeros((tt, kk)), np.zeros((tt, kk))
    check(_lib.load().sgl_ripley_stats(K, T, ptr(buf, _lib.i64p), ptr(g, _lib.i64p), float(area), ptr(Kf, f64p), ptr(L, f64p)))
    return {"K": np.ascontiguousarray(Kf[:T, :K].T), "L": np.ascontiguousarray(L[:T, :K].T)}


def c_cooccur(coords, labels, interval, n_classes=None, timing=False):
    """The one-shot form of Context.cooccur (sgl_c_cooccur), in a context of its own: {"counts" (K x K x T int64), "ratio" (the
    per-interval statistic of cooccur_stats), "info" (Context.cooccur_info's fields)}; with timing "stage_ms" (sort + gather,
    tally, epilogue + download).  The arguments come in Context.cooccur's order, the coordinates before the labels; co_occurrence
    and ripley take the labels first."""
    from ._cooccur import COOCCUR_INFO, abt, cooccur_inputs, table_shape
    c1, c2, n, lab, K, r, T = cooccur_inputs(coords, labels, interval, n_classes, "c_cooccur")
    counts, ratio = np.zeros(table_shape(K, T), dtype=np.int64), np.zeros(table_shape(K, T))
    info, ms = np.zeros(8, dtype=np.int64), (np.zeros(3) if timing else None)
    check(_lib.load().sgl_c_cooccur(ptr(c1, f64p), ptr(c2, f64p), n, ptr(lab, i32p), K, ptr(r, f64p), T, ptr(counts, _lib.i64p), ptr(ratio, f64p),
                                    ptr(info, _lib.i64p), ptr(ms, f64p)))
    out = {"counts": abt(counts, K, T), "ratio": abt(ratio, K, T), "info": dict(zip(COOCCUR_INFO, (int(v) for v in info)))}
    if timing:
        out["stage_ms"] = ms
    return out


def _cooccur_front(who, labels, coords, interval, n_classes):
    """Every refusal of co_occurrence / ripley, before the first upload: (c1, c2, lab, K, r)."""
    from ._cooccur import MAX_INTERVALS, cooccur_coords, cooccur_thresholds, default_interval
    c1, c2 = cooccur_coords(coords, who)
    lab, K = _nhood_classes(who, labels, n_classes)
    if lab.shape[0] != c1.shape[0]:
        raise ValueError("%s: %d labels, %d points" % (who, lab.shape[0], c1.shape[0]))
    for name, v in (("first", c1), ("second", c2)):
        if not np.isfinite(v).all():
            at = int(np.nonzero(~np.isfinite(v))[0][0])
            raise ValueError("%s: the %s coordinate of point %d is not finite" % (who, name, at))
    if np.ndim(interval) == 0:
        r = default_interval(c1, c2, interval, who)
    else:
        r = cooccur_thresholds(interval, who)
        if not 2 <= r.shape[0] <= MAX_INTERVALS + 1:
            raise ValueError("%s: %d thresholds: between 2 and %d are taken (at most %d intervals)" % (who, r.shape[0], MAX_INTERVALS + 1, MAX_INTERVALS))
        if not np.isfinite(r).all() or r[0] < 0:
            raise ValueError("%s: the thresholds must be finite and start at 0 or above" % who)
    with np.errstate(over="ignore", under="ignore"):
        sq = r * r
    if not np.isfinite(sq).all() or not (np.diff(sq) > 0).all():
        raise ValueError("%s: the thresholds must ascend strictly, and so must their squares" % who)
    return c1, c2, lab, K, r


def co_occurrence(labels, coords, interval=50, n_classes=None, cumulative=False):
    """How the presence of class b changes with the distance from a cell of class a: the co-occurrence score of squidpy's
    gr.co_occurrence on the device (sgl_c_cooccur; the rules are stated in include/singlet_hip.h, "Co-occurrence by distance" --
    this library's own statement of the published score in FP64, NO parity with squidpy is claimed).  labels: one integer class
    in [0, n_classes) per cell; coords: n x 2, or a pair of vectors.  interval: an ascending array of distance thresholds (at
    most 65), or a count T <= 64, which means np.linspace(0, 0.5 * hypot(extent_x, extent_y), T + 1) -- the library's own rule.
    Returns {"occ" (K x K x T doubles, [a, b, t]; of the running sums with cumulative), "counts" (K x K x T int64 ordered pairs
    per interval), "interval" (the thresholds)}.  Every argument is refused before the first upload.  The labels come first, as in
    nhood_enrichment; the calls below this one (c_cooccur, Context.cooccur) take the coordinates first."""
    who = "co_occurrence"
    c1, c2, lab, K, r = _cooccur_front(who, labels, coords, interval, n_classes)
    res = c_cooccur((c1, c2), lab, r, K)
    return {"occ": cooccur_stats(res["counts"], True) if cumulative else res["ratio"], "counts": res["counts"], "interval": r}


def ripley(labels, coords, mode="L", interval=50, area=None, n_classes=None):
    """Ripley's K or L function of every class (squidpy's gr.ripley without edge correction or simulations), from the same
    tally as co_occurrence: K x T, [a, t] at radius interval[t + 1].  mode "K" or "L"; area None: the bounding box of the
    points.  interval as in co_occurrence; a first threshold above 0 leaves the closer pairs out of the cumulative count."""
    who = "ripley"
    if mode not in ("K", "L"):
        raise ValueError("%s: mode = %r is none of 'K', 'L'" % (who, mode))
    c1, c2, lab, K, r = _cooccur_front(who, labels, coords, interval, n_classes)
    if area is None:
        area = float((c1.max() - c1.min()) * (c2.max() - c2.min()))
    if not (np.isfinite(area) and area > 0):
        raise ValueError("%s: area = %r is not a positive finite number" % (who, area))
    res = c_cooccur((c1, c2), lab, r, K)
    return ripley_stats(res["counts"], np.bincount(lab, minlength=K).astype(np.int64), area)[mode]
