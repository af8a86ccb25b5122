"""Marshalling shared by the fit calls of api.py and the handles of context.py: pointer triples, column-major images and
the output buffers of the two fit families, each yielding its trailing ctypes arguments in ABI order, and the one call of the
embedding k-NN."""
import ctypes as C
import math

import numpy as np

from ._lib import check, f64p, i32p, i64p, ptr, u64p


def csc_ptrs(A):
    """The (x, i, p) pointers of a dgCMatrix; three NULLs for None."""
    return (None, None, None) if A is None else (ptr(A.x, f64p), ptr(A.i, i32p), ptr(A.p, i32p))


def colmajor(X, message):
    """Column-major image of a 2-D array, as the library reads an R matrix: shape (cols, rows), float64, contiguous.
    message: the caller's ValueError text for anything that is not 2-D."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError(message)
    return np.ascontiguousarray(X.T)


class _FitOutputs:
    """shape = (m, n, k): w_out (m, k) -- (k, m) with w_m_by_k, the m x k column-major image c_gcnmf writes --, h_out
    (n, k) and d_out; shape = None: no factor buffers (the run loops of a handle: get_factors fills w, d, h later)."""

    def __init__(self, shape, w_m_by_k=False):
        self.w = self.d = self.h = None
        if shape is not None:
            m, n, k = shape
            self.w, self.h, self.d = np.empty((k, m) if w_m_by_k else (m, k)), np.empty((n, k)), np.empty(k)

    def _factor_args(self):
        return () if self.w is None else (ptr(self.w, f64p), ptr(self.d, f64p), ptr(self.h, f64p))


class NmfOutputs(_FitOutputs):
    """What a fit of the c_nmf family writes: the factors, n_iter and the tol trace of max(maxit, 1) entries."""

    def __init__(self, shape, maxit, w_m_by_k=False):
        super().__init__(shape, w_m_by_k)
        self.n_iter = C.c_int32()
        self.trace = np.zeros(max(int(maxit), 1))

    def args(self):
        return (*self._factor_args(), C.byref(self.n_iter), ptr(self.trace, f64p))

    def run(self):
        """(iterations, their tol) as nmf_run returns them."""
        return self.n_iter.value, self.trace[:self.n_iter.value].copy()

    def result(self):
        n_iter, tol = self.run()
        return {"w": self.w.T, "d": self.d, "h": self.h.T, "iter": n_iter, "tol": tol}


class ArdOutputs(_FitOutputs):
    """What a fit of the ARD family writes: the factors, four traces of maxit + 2 entries, nt (the entries written) and,
    with nit (the run loops), the iterations run."""

    def __init__(self, shape, maxit, nit=False):
        super().__init__(shape)
        cap = int(maxit) + 2
        self.test_mse, self.tol, self.score_overfit = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        self.iter = np.zeros(cap, dtype=np.int32)
        self.nt = C.c_int32()
        self.nit = C.c_int32() if nit else None

    def args(self):
        tail = (C.byref(self.nt),) if self.nit is None else (C.byref(self.nt), C.byref(self.nit))
        return (*self._factor_args(), ptr(self.test_mse, f64p), ptr(self.iter, i32p), ptr(self.tol, f64p),
                ptr(self.score_overfit, f64p), *tail)

    def traces(self):
        q = self.nt.value
        return {"test_mse": self.test_mse[:q].copy(), "iter": self.iter[:q].copy(), "tol": self.tol[:q].copy(),
                "score_overfit": self.score_overfit[:q].copy()}

    def result(self):
        return {"w": self.w.T, "d": self.d, "h": self.h.T, **self.traces()}


MARKER_TRANSFORMS = {"identity": 0, "expm1": 1, 0: 0, 1: 1}


def label_list(labels, n, n_groups):
    """(int32 labels, G) of sgl_markers: one label in [-1, G) per cell; n_groups None: 1 + the largest label (at least 1).
    The library checks the range."""
    g = np.asarray(labels)
    if g.ndim != 1 or (n is not None and g.shape[0] != n):
        raise ValueError("labels must hold one cluster id per cell" + ("" if n is None else " (%d)" % n))
    if g.dtype.kind not in "iub":
        raise ValueError("labels must hold integer cluster ids (-1: the cell is left out)")
    if g.size and (g.min() < -2**31 or g.max() >= 2**31):
        raise ValueError("labels holds an id outside the 32-bit range")
    g = np.ascontiguousarray(g, dtype=np.int32)
    G = int(n_groups) if n_groups is not None else max(int(g.max()) + 1 if g.size else 1, 1)
    return g, G


NHOOD_TALLIES = ("counts", "S1", "S2", "n_ge", "n_le")
NHOOD_STATS = ("zscore", "mean", "sd", "p_enriched", "p_depleted", "p_adj_enriched", "p_adj_depleted")
NHOOD_INFO = ("path", "perms_per_group", "batches", "batch", "lds_bytes", "sort")


def nhood_labels(labels, n, n_classes, who):
    """(int32 labels, K) of the neighbourhood enrichment calls: one integer class per cell (a column of find_clusters'
    "clusters" is one); n_classes None: 1 + the largest label.  The library checks the range and names the offender."""
    g = np.asarray(labels)
    if g.ndim == 2 and 1 in g.shape:
        g = g.reshape(-1)
    if g.ndim != 1 or g.size < 1 or g.dtype.kind not in "iub" or (n is not None and g.shape[0] != n):
        raise ValueError("%s: labels must hold one integer class per cell%s" % (who, "" if n is None else " (%d)" % n))
    if g.min() < -2**31 or g.max() >= 2**31:
        raise ValueError("%s: a label is outside the 32-bit range" % who)
    K = int(n_classes) if n_classes is not None else max(int(g.max()) + 1, 1)
    if not -2**31 <= K < 2**31:
        raise ValueError("%s: n_classes is outside the 32-bit range" % who)
    return np.ascontiguousarray(g, dtype=np.int32), K


LIGREC_INFO = ("path", "vectors_per_wave", "batches", "batch", "lds_bytes", "waves", "lds_genes", "global_genes")


def _index_list(a, who, name):
    a = np.asarray(a)
    if a.size == 0:
        a = np.zeros(0, dtype=np.int32)
    if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < -2**31 or a.max() >= 2**31)):
        raise ValueError("%s: %s must be a one-dimensional list of 32-bit indices" % (who, name))
    return np.ascontiguousarray(a, dtype=np.int32) if a.size else np.zeros(1, dtype=np.int32)[:0]


def ligrec_inputs(labels, n, n_classes, genes, lig, rec, who):
    """(lab, K, genes, G, lig, rec, P) of the ligand-receptor calls: one integer class per cell, distinct 0-based gene indices,
    and the pairs as indices into genes.  The library checks the content and names the offender; only what cannot be marshalled
    is refused here."""
    lab, K = nhood_labels(labels, n, n_classes, who)
    g, lg, rc = _index_list(genes, who, "genes"), _index_list(lig, who, "lig"), _index_list(rec, who, "rec")
    if lg.shape != rc.shape:
        raise ValueError("%s: lig and rec must hold one index each per pair" % who)
    return lab, K, g, int(g.shape[0]), lg, rc, int(lg.shape[0])


def ligrec_call(fn, K, G, P, nperm, return_null, with_stats=False):
    """Shared by Context.ligrec and api.c_ligrec: fn(group_n, nz, sum, mean, score, n_ge, null_out[, expressed, p, padj, info,
    stage_ms]) is the library call with everything before the outputs bound.  Returns the dict of the arrays: "group_n" (K),
    "nz", "sum", "mean" (G x K), "score", "n_ge" (P x K x K, [q, a, b] = ligand class a, receptor class b), with return_null
    "null" (nperm x P x K x K); with_stats also "expressed" (G x K bool), "p", "padj", "info" and "stage_ms"."""
    kk, gg, pp = max(min(K, 256), 1), max(G, 1), max(P, 1)   # outside the legal ranges the library refuses before it writes
    group_n, nz = np.zeros(kk, dtype=np.int64), np.zeros((gg, kk), dtype=np.int64)
    s, mean = np.zeros((gg, kk)), np.zeros((gg, kk))
    score, n_ge = np.zeros((kk, kk, pp)), np.zeros((kk, kk, pp), dtype=np.int64)
    null = np.zeros((max(min(int(nperm), 1 << 20), 1), kk, kk, pp)) if return_null else None
    args = [ptr(group_n, i64p), ptr(nz, i64p), ptr(s, f64p), ptr(mean, f64p), ptr(score, f64p), ptr(n_ge, i64p), ptr(null, f64p)]
    if with_stats:
        ex, p, padj = np.zeros((gg, kk), dtype=np.uint8), np.zeros((kk, kk, pp)), np.zeros((kk, kk, pp))
        info, ms = np.zeros(8, dtype=np.int64), np.zeros(3)
        args += [ptr(ex, C.POINTER(C.c_uint8)), ptr(p, f64p), ptr(padj, f64p), ptr(info, i64p), ptr(ms, f64p)]
    check(fn(*args))
    out = {"group_n": group_n, "nz": nz, "sum": s, "mean": mean, "score": np.ascontiguousarray(score.transpose(2, 1, 0)),
           "n_ge": np.ascontiguousarray(n_ge.transpose(2, 1, 0))}
    if return_null:
        out["null"] = np.ascontiguousarray(null.transpose(0, 3, 2, 1))
    if with_stats:
        out.update(expressed=ex.astype(bool), p=np.ascontiguousarray(p.transpose(2, 1, 0)), padj=np.ascontiguousarray(padj.transpose(2, 1, 0)),
                   info=dict(zip(LIGREC_INFO, (int(v) for v in info))), stage_ms=ms)
    return out


def markers_call(fn, nrow, labels, G, transform, pseudocount):
    """Shared by Context.markers and api.c_markers: fn(labels, n_groups, transform, pseudocount, group_n, pos, sum, rank2, tie,
    pct_in, pct_out, log2fc, z, p) is the library call.  Returns the dict of the arrays, the per-(gene, cluster) ones as
    nrow x G."""
    if transform not in MARKER_TRANSFORMS:
        raise ValueError("transform must be 'expm1' or 'identity'")
    m, Gs = max(int(nrow), 1), max(min(G, 1024), 1)   # outside [1, 1024] the library refuses before it writes
    group_n = np.zeros(Gs, dtype=np.int64)
    i64s = {k: np.zeros((Gs, m), dtype=np.int64) for k in ("pos", "rank2")}
    f64s = {k: np.empty((Gs, m)) for k in ("sum", "pct_in", "pct_out", "log2fc", "z", "p")}
    tie = np.zeros(m, dtype=np.uint64)
    check(fn(ptr(labels, i32p), int(G), MARKER_TRANSFORMS[transform], float(pseudocount), ptr(group_n, i64p), ptr(i64s["pos"], i64p),
             ptr(f64s["sum"], f64p), ptr(i64s["rank2"], i64p), ptr(tie, u64p), ptr(f64s["pct_in"], f64p), ptr(f64s["pct_out"], f64p),
             ptr(f64s["log2fc"], f64p), ptr(f64s["z"], f64p), ptr(f64s["p"], f64p)))
    out = {"group_n": group_n, "tie": tie[:int(nrow)]}
    for k, a in {**i64s, **f64s}.items():
        out[k] = a[:, :int(nrow)].T
    return out


ANNOTATE_TAILS = {"pos": 0, "neg": 1, "std": 2}
ANNOTATE_ROW_GROUP = ("coefficients", "t", "p_raw", "p_adj", "lods")      # rows x G
ANNOTATE_ROW = ("Amean", "sigma", "s2_post")                              # rows
ANNOTATE_GROUP = ("stdev_unscaled", "var_prior")                          # G
ANNOTATE_SCALARS = ("df_residual", "s2_prior", "df_prior", "df_total")


def annotate_tail(tail):
    if tail not in ANNOTATE_TAILS:
        raise ValueError("Invalid tail selection. Choose 'pos','neg', or 'std'")
    return ANNOTATE_TAILS[tail]


def annotate_call(fn, rows, G, center, scale, proportion, tail, moments=None, with_nz=False):
    """Shared by annotate_stats, Context.annotate, Context.annotate_genes and api.c_annotate: fn(center, scale, proportion, tail,
    [group_n, (nz,) sum, rss,] the eleven outputs) is the library call.  moments: (group_n, sum rows x G, rss) when the call
    takes them as inputs (sgl_annotate_stats), else they are outputs.  Returns the dict of the arrays, the per-(row, group)
    ones as rows x G, with the moments among them."""
    r, Gs = max(int(rows), 1), max(min(int(G), 1024), 1)   # outside [1, 1024] the library refuses before it writes
    tl = annotate_tail(tail)
    rg = {k: np.full((Gs, r), np.nan) for k in ANNOTATE_ROW_GROUP}
    rw = {k: np.full(r, np.nan) for k in ANNOTATE_ROW}
    gr = {k: np.full(Gs, np.nan) for k in ANNOTATE_GROUP}
    sc = np.full(4, np.nan)
    outs = [ptr(rg["coefficients"], f64p), ptr(gr["stdev_unscaled"], f64p), ptr(rw["Amean"], f64p), ptr(rw["sigma"], f64p),
            ptr(rw["s2_post"], f64p), ptr(sc, f64p), ptr(gr["var_prior"], f64p), ptr(rg["t"], f64p), ptr(rg["p_raw"], f64p),
            ptr(rg["p_adj"], f64p), ptr(rg["lods"], f64p)]
    nz = None
    if moments is None:
        group_n, s, rss = np.zeros(Gs, dtype=np.int64), np.zeros((Gs, r)), np.zeros(r)
        mom = [ptr(group_n, i64p)]
        if with_nz:
            nz = np.zeros((Gs, r), dtype=np.int64)
            mom.append(ptr(nz, i64p))
        mom += [ptr(s, f64p), ptr(rss, f64p)]
        check(fn(int(bool(center)), int(bool(scale)), float(proportion), tl, *mom, *outs))
    else:
        group_n = np.ascontiguousarray(moments[0], dtype=np.int64)
        given = np.asarray(moments[1], dtype=np.float64)
        rss = np.ascontiguousarray(moments[2], dtype=np.float64) if rows else np.zeros(r)
        if group_n.shape != (int(G),) or given.shape != (int(rows), int(G)) or (rows and rss.shape != (int(rows),)):
            raise ValueError("group_n must hold G counts, sum rows x G values and rss one value per row")
        s = np.ascontiguousarray(given.T) if rows else np.zeros((max(int(G), 1), r))   # (G outside [1, 1024]: the library refuses)
        check(fn(ptr(group_n, i64p), ptr(s, f64p), ptr(rss, f64p), int(bool(center)), int(bool(scale)), float(proportion), tl, *outs))
    n = int(rows)
    out = {"group_n": group_n, "sum": s[:, :n].T, "rss": rss[:n], "centered": bool(center), "scaled": bool(scale),
           "proportion": float(proportion), "tail": tail}
    if nz is not None:
        out["nz"] = nz[:, :n].T
    for k, a in rg.items():
        out[k] = a[:, :n].T
    for k, a in rw.items():
        out[k] = a[:n]
    out.update(gr)
    out.update(dict(zip(ANNOTATE_SCALARS, (float(v) for v in sc))))
    return out


GSEA_SCORE_TYPES = {"pos": 0, "neg": 1, "std": 2, 0: 0, 1: 1, 2: 2}


def gsea_inputs(w, set_ptr, set_genes):
    """(w column-major as its (k, m) image, m, k, int64 set_ptr, int32 set_genes) of the enrichment calls.  w: m genes x k
    factors.  The library checks the content; only what cannot be marshalled is refused here."""
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError("w must be a matrix, m genes x k factors")
    sp, sg = np.asarray(set_ptr), np.asarray(set_genes)
    if sg.size == 0:
        sg = np.zeros(0, dtype=np.int32)
    if sp.ndim != 1 or sp.size < 1 or sp.dtype.kind not in "iu":
        raise ValueError("set_ptr must hold the n_sets + 1 integer offsets of the gene sets")
    if sg.ndim != 1 or sg.dtype.kind not in "iu" or (sg.size and (sg.min() < -2**31 or sg.max() >= 2**31)):
        raise ValueError("set_genes must hold 0-based integer gene indices")
    sp = np.ascontiguousarray(sp, dtype=np.int64)
    if sp[-1] > sg.size or (sp.size > 1 and sp.max() > sg.size):
        raise ValueError("set_ptr points past the end of set_genes (%d entries)" % sg.size)
    return np.ascontiguousarray(w.T), w.shape[0], w.shape[1], sp, np.ascontiguousarray(sg, dtype=np.int32)


def gsea_score_type(score_type):
    if score_type not in GSEA_SCORE_TYPES:
        raise ValueError("score_type must be 'pos', 'neg' or 'std'")
    return GSEA_SCORE_TYPES[score_type]


def signature_sets(sets):
    """(int64 set_ptr, int32 set_genes) of the signature calls from a list of gene-index sequences, one per set.  The library
    checks the content; only what cannot be marshalled is refused here."""
    if isinstance(sets, np.ndarray) and sets.ndim == 1 and sets.dtype.kind in "iu":
        sets = [sets]
    rows = []
    for j, v in enumerate(sets):
        a = np.asarray(v)
        if a.size == 0:
            a = np.zeros(0, dtype=np.int32)
        if a.ndim != 1 or a.dtype.kind not in "iu" or (a.size and (a.min() < -2**31 or a.max() >= 2**31)):
            raise ValueError("set %d must hold 0-based integer gene indices" % j)
        rows.append(a.astype(np.int32))
    sp = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        sp[1:] = np.cumsum([r.size for r in rows])
    sg = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0), dtype=np.int32)
    if sg.size == 0:
        sg = np.zeros(1, dtype=np.int32)[:0]
    return sp, sg


def signature_call(fn, ncol, sets, max_rank, return_rank2):
    """Shared by Context.signature_scores, Context.op_signature_scores and api.c_signature_scores: fn(set_ptr, set_genes,
    n_sets, max_rank, rank2, score) is the library call.  Returns score (n_sets x ncol), with return_rank2 (rank2, score)."""
    sp, sg = signature_sets(sets)
    P, n = sp.shape[0] - 1, max(int(ncol), 1)
    if not -2**31 <= int(max_rank) < 2**31:
        raise ValueError("max_rank is outside the 32-bit range")
    score = np.empty((n, max(P, 1)))
    rank2 = np.zeros((n, max(P, 1)), dtype=np.uint64) if return_rank2 else None
    keep = sg if sg.size else np.zeros(1, dtype=np.int32)   # (an empty list still needs an address: the library names the defect)
    check(fn(ptr(sp, i64p), ptr(keep, i32p), P, int(max_rank), ptr(rank2, u64p), ptr(score, f64p)))
    score = score[:int(ncol), :P].T
    return (rank2[:int(ncol), :P].T, score) if return_rank2 else score


KNN_METRICS = {"euclidean": 0, "cosine": 1, "correlation": 2}


def knn_metric(metric):
    """The metric code of sgl_knn_metric for a name; anything else is refused here, by name."""
    if not isinstance(metric, str) or metric not in KNN_METRICS:
        raise ValueError("metric must be 'euclidean', 'cosine' or 'correlation'")
    return KNN_METRICS[metric]


KNN_IVF_DEFAULT_PROBES = 8   # KNN_IVF_DEFAULT_PROBES of csrc/knn_ivf_host.h (tests/test_knn_ivf_restatement.py holds the two together)
KNN_METHODS = ("exact", "ivf")


def knn_method(method):
    """True for the inverted-list search, False for the exact one; anything else is refused here, by name."""
    if not isinstance(method, str) or method not in KNN_METHODS:
        raise ValueError("method must be 'exact' or 'ivf'")
    return method == "ivf"


def knn_ivf_shape(n_ref, n_lists=None, n_probe=None):
    """(n_lists, n_probe) of an inverted-list search.  n_lists None: ceil(sqrt(n_ref)) clamped to the legal [1, min(n_ref,
    65536)]; n_probe None: the default of knn_ivf_host.h clamped to min(n_lists, 64).  A given value goes to the library as it
    is, which refuses what is out of range."""
    n_ref = int(n_ref)
    if n_lists is None:
        r = math.isqrt(max(n_ref, 0))
        n_lists = max(1, min(r + (r * r < n_ref), n_ref, 65536))
    if n_probe is None:
        n_probe = max(1, min(KNN_IVF_DEFAULT_PROBES, int(n_lists), 64))
    return int(n_lists), int(n_probe)


def knn_recall(idx, idx_exact):
    """The mean, over the rows, of the share of a row's exact neighbours (idx_exact, n x K) that the same row of idx holds;
    entries of -1 (a short result) match nothing."""
    a, b = np.asarray(idx), np.asarray(idx_exact)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("idx and idx_exact must be matrices with one row per query")
    if b.size == 0:
        raise ValueError("idx_exact is empty")
    hit = (b[:, :, None] == a[:, None, :]) & (b[:, :, None] >= 0)
    return float(hit.any(axis=2).mean(axis=1).mean())


def knn_call(fn, reference, query, dims, n_neighbors, resident=None, metric=None, extra=None):
    """Shared by Context.knn and api.knn: fn(R, k, n_ref, Q, n_query, dims, n_dims, n_neighbors, idx_out, dist_out) is the
    library call -- with a metric code, fn(..., n_neighbors, metric, idx_out, dist_out), the sgl_knn_metric form; extra: a
    function of n_ref giving the arguments between the metric and idx_out (the inverted-list forms).  reference / query: k x n matrices (R's orientation, one column per cell); a None reference stands for the
    H of a fit of shape resident = (k, n), a None query for the references themselves; dims: 0-based rows or None.
    Returns (idx, dist), each n_query x n_neighbors: row j holds the neighbours of query j in rank order."""
    if reference is None:
        if resident is None:
            raise ValueError("reference must be a k x n matrix")
        k, n_ref = resident
        Rb = None
    else:
        Rb = colmajor(reference, "reference must be a k x n matrix")
        n_ref, k = Rb.shape
    Qb, nq = None, n_ref
    if query is not None:
        Qb = colmajor(query, "query must be a k x n matrix")
        nq = Qb.shape[0]
        if Qb.shape[1] != k:
            raise ValueError("query has %d rows, the reference has %d" % (Qb.shape[1], k))
    d, nd = None, 0
    if dims is not None:
        d = np.asarray(dims)
        if d.size == 0:   # (an empty list has no integer type of its own; the library refuses it by name)
            d = np.zeros(0, dtype=np.int32)
        if d.ndim != 1 or d.dtype.kind not in "iu" or (d.size and (d.min() < -2**31 or d.max() >= 2**31)):
            raise ValueError("dims must be a list of 32-bit row indices")
        d = np.ascontiguousarray(d, dtype=np.int32)
        nd = int(d.size)
    K = int(n_neighbors)
    shape = (int(nq), K) if 1 <= K <= 256 else (1, 1)   # outside it the library refuses before it writes
    idx, dist = np.empty(shape, dtype=np.int32), np.empty(shape)
    code = () if metric is None else (int(metric),)
    more = () if extra is None else tuple(extra(int(n_ref), nd if d is not None else int(k)))
    check(fn(ptr(Rb, f64p), int(k), int(n_ref), ptr(Qb, f64p), int(nq), ptr(d, i32p), nd, K, *code, *more, ptr(idx, i32p), ptr(dist, f64p)))
    return idx, dist


KNN_WEIGHTINGS = {"uniform": 0, "distance": 1}
KNN_INDEX_FIELDS = ("present", "method", "metric", "k", "n_dims", "n_ref", "n_lists", "train_cells", "shortest_list", "longest_list",
                    "empty_lists", "bytes", "searches", "last_queries", "last_short_queries", "instance")


def knn_weighting(weighting):
    """The weighting code of the transfer for a name: "uniform" (every neighbour votes 1) or "distance" (Dudani's weights)."""
    if not isinstance(weighting, str) or weighting not in KNN_WEIGHTINGS:
        raise ValueError("weighting must be 'uniform' or 'distance'")
    return KNN_WEIGHTINGS[weighting]


def knn_lists_in(idx, dist):
    """(idx int32, dist float64, n_query, n_neighbors) of neighbour lists as the searches return them, n_query x n_neighbors: in
    memory the n_neighbors x n_query column-major image the library reads."""
    i, d = np.asarray(idx), np.asarray(dist, dtype=np.float64)
    if i.ndim != 2 or d.shape != i.shape:
        raise ValueError("idx and dist must be matrices of one shape, n_query x n_neighbors")
    if i.dtype.kind not in "iu" or (i.size and (i.min() < -2**31 or i.max() >= 2**31)):
        raise ValueError("idx must hold 32-bit reference indices (-1: padding)")
    return np.ascontiguousarray(i, dtype=np.int32), np.ascontiguousarray(d), int(i.shape[0]), int(i.shape[1])


def transfer_call(fn, nq, labelled, n_classes, n_values):
    """Shared by Context.knn_index_map and Context.op_knn_transfer: fn(pred_out, best_out, scores_out, values_out) is the
    library call with everything before the outputs bound.  labelled: the label outputs are asked for; n_values 0: no values.
    Returns {"predicted", "score", "scores" (n_query x n_classes), "values" (n_query x n_values)}, None where not asked for."""
    nq = max(int(nq), 0)
    pred = np.empty(nq, dtype=np.int32) if labelled else None
    best = np.empty(nq) if labelled else None
    scores = np.empty((nq, int(n_classes))) if labelled and 1 <= int(n_classes) <= 65536 else None
    values = np.empty((nq, int(n_values))) if 1 <= int(n_values) <= 1024 else None
    check(fn(ptr(pred, i32p), ptr(best, f64p), ptr(scores, f64p), ptr(values, f64p)))
    return {"predicted": pred, "score": best, "scores": scores, "values": values}
