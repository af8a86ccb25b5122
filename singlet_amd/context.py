"""Device context: one resident shard of cells on one MI355X (sgl_ctx of
include/singlet_hip.h section 2).  Thin object wrapper over the C ABI."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f64p, i32p, i64p, ptr, u64p, u8p
from ._marshal import (KNN_INDEX_FIELDS, LIGREC_INFO, ligrec_call, ligrec_inputs, MARKER_TRANSFORMS, NHOOD_INFO, NHOOD_TALLIES, ArdOutputs, NmfOutputs, annotate_call, colmajor, csc_ptrs, gsea_inputs,
                       gsea_score_type, knn_call, knn_ivf_shape, knn_lists_in, knn_method, knn_metric, knn_weighting, label_list, markers_call, nhood_labels,
                       signature_call, transfer_call)
from .sparse import as_dgCMatrix

SYNTH_SEED = 0x5EED
# 16 value levels of the synthetic generator: log1p(1 + level)
LEVELS16 = np.log1p(1.0 + np.arange(16, dtype=np.float64))


def skew_weights16(sigma):
    """16 log-normal quantile levels exp(sigma * z_q), z_q the normal quantile of (q + 1/2) / 16, scaled to mean 1."""
    # normal quantiles of (q + 0.5) / 16, q = 0..15 (symmetric)
    z = np.array([-1.8627318674, -1.3180108973, -1.0099901692, -0.7764217611, -0.5791321623, -0.4022500653, -0.2372021093, -0.0784124127])
    z = np.concatenate([z, -z[::-1]])
    w = np.exp(float(sigma) * z)
    return w / w.mean()


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def make_callbacks(log=None, poll=None):
    """Builds an sgl_callbacks struct; keep the returned object alive during the call."""
    cb = _lib.Callbacks()
    keep = []
    if log is not None:
        fn = _lib.LOG_FN(lambda user, it, tol, of: log(it, tol, of))
        cb.log = fn
        keep.append(fn)
    if poll is not None:
        fn = _lib.POLL_FN(lambda user: int(bool(poll())))
        cb.poll = fn
        keep.append(fn)
    cb._keep = keep
    return cb


COMM_ID_BYTES = 128


def comm_unique_id():
    """RCCL unique id (bytes) for Context.comm_init_rank: rank 0 makes it, the host broadcasts it."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(_lib.load().sgl_comm_unique_id(buf))
    return buf.raw


def device_count():
    """gfx950 devices this process can use (sgl_device_count; 0 without the HIP runtime or a device)."""
    return int(_lib.load().sgl_device_count())


def comm_available():
    """(ok, path): can RCCL be bound in this process (no communication), and which library was opened.
    Ranks agree on this BEFORE comm_init_rank, which is collective and would otherwise hang on a rank
    that cannot join."""
    buf = C.create_string_buffer(512)
    rc = _lib.load().sgl_comm_available(buf, 512)
    return rc == 0, buf.value.decode("utf-8", "replace")


def split_cells_by_nnz(p, n):
    """The cell split of Multi.upload (sgl_multi_upload_csc): n + 1 boundaries of contiguous blocks of
    nearly equal non-zero count, each at least one cell."""
    p = np.ascontiguousarray(p, dtype=np.int32)
    lo = np.zeros(n + 1, dtype=np.int64)
    check(_lib.load().sgl_split_cells_by_nnz(ptr(p, i32p), int(p.shape[0] - 1), int(n), ptr(lo, i64p)))
    return lo


def graph_halo_plan(p, i, cell_lo):
    """The halo plan of Multi.set_graph (sgl_graph_halo_plan; host only, no device): for an n x n cell graph given by its
    dgCMatrix slots p, i and the block boundaries cell_lo (ranks + 1 values from 0 to n) a dict with
      "export":   per rank, the cells (global indices, ascending) that columns of other ranks read,
      "i_local":  i with every row rewritten for its column's rank r: row - cell_lo[r] for a cell of r, n_local_r + s * E +
                  (position in export[s]) for a cell of rank s,
      "edges", "crossing" (entries whose row and column live on different ranks), "E" (longest export list)."""
    p = np.ascontiguousarray(p, dtype=np.int32)
    i = np.ascontiguousarray(i, dtype=np.int32)
    lo = np.ascontiguousarray(cell_lo, dtype=np.int64)
    n, nr = int(p.shape[0] - 1), int(lo.shape[0] - 1)
    if n < 1 or nr < 1 or i.shape[0] < int(p[-1]):
        raise ValueError("graph_halo_plan: p, i, cell_lo do not describe a graph and its blocks")
    i_local = np.zeros(max(int(p[-1]), 1), dtype=np.int32)
    eptr = np.zeros(nr + 1, dtype=np.int64)
    eidx = np.zeros(n, dtype=np.int32)
    info = np.zeros(4, dtype=np.int64)
    check(_lib.load().sgl_graph_halo_plan(ptr(i, i32p), ptr(p, i32p), n, nr, ptr(lo, i64p), ptr(i_local, i32p), ptr(eptr, i64p),
                                          ptr(eidx, i32p), ptr(info, i64p)))
    return dict(export=[eidx[eptr[r]:eptr[r + 1]].copy() for r in range(nr)], i_local=i_local[:int(p[-1])],
                edges=int(info[0]), crossing=int(info[1]), E=int(info[2]))


def _chunk_list(chunks):
    """ctypes image of a list of dgCMatrix column chunks: (n, x**, i**, p**, ncol*) and what must stay alive.  A chunk
    that already is a dgCMatrix is not copied: a chunk listed twice passes the same host pointers twice."""
    chunks = [as_dgCMatrix(a) for a in chunks]
    n = len(chunks)
    xs = (f64p * n)(*[ptr(a.x, f64p) for a in chunks])
    is_ = (i32p * n)(*[ptr(a.i, i32p) for a in chunks])
    ps = (i32p * n)(*[ptr(a.p, i32p) for a in chunks])
    nc = np.array([a.ncol for a in chunks], dtype=np.int32)
    return (n, xs, is_, ps, ptr(nc, i32p)), (chunks, xs, is_, ps, nc)


def _chunk_lists(chunks, t_chunks, empty_message, rows_message):
    """The images of the column chunks of A and of t(A) (None / empty: the transpose is built on the device) for the list
    entry points: (a, t, nrow, total columns, what must stay alive).  The caller words the two refusals."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError(empty_message)
    a, keep_a = _chunk_list(chunks)
    nrow = keep_a[0][0].nrow
    if any(c.nrow != nrow for c in keep_a[0]):
        raise ValueError(rows_message)
    if t_chunks is None or len(t_chunks) == 0:
        t, keep_t = (0, None, None, None, None), None
    else:
        t, keep_t = _chunk_list(t_chunks)
    return a, t, nrow, sum(c.ncol for c in keep_a[0]), (keep_a, keep_t)


def _link_image(Lk):
    """ctypes image of an R link matrix (rows x cols): (pointer, rows, cols, the buffer to keep alive); None switches the side off."""
    if Lk is None:
        return None, 0, 0, None
    buf = colmajor(Lk, "link matrices must be 2-D")
    return ptr(buf, f64p), buf.shape[1], buf.shape[0], buf


def _group_list(group, n, what):
    """int32 image of a list of group ids, one per cell (gene); the library checks their range."""
    g = np.asarray(group)
    if g.ndim != 1 or (n is not None and g.shape[0] != n):
        raise ValueError("%s must hold one group id per %s" % (what, "entry" if n is None else "column (%d)" % n))
    if g.dtype.kind not in "iu" and g.dtype.kind != "b":
        raise ValueError("%s must hold integer group ids" % what)
    if g.size and (g.min() < -2**31 or g.max() >= 2**31):
        raise ValueError("%s holds an id outside the 32-bit range" % what)
    return np.ascontiguousarray(g, dtype=np.int32)


def _grouped_side(table, group, n, side):
    """(pointer, rows, groups, group pointer, what to keep alive) of one side of set_links_grouped; a None table is off."""
    if table is None:
        return None, 0, 0, None, None
    buf = colmajor(table, "table_%s must be a rows x groups matrix" % side)
    if group is None:
        raise ValueError("table_%s needs group_%s" % (side, side))
    g = _group_list(group, n, "group_" + side)
    return ptr(buf, f64p), buf.shape[1], buf.shape[0], ptr(g, i32p), (buf, g)


def _group_means_call(fn, g, n_groups, k):
    """Shared by Context.group_means, Multi.group_means and api.group_means: fn(group, n_groups, means, counts) is the
    library call; g the int32 group list (_group_list)."""
    G = int(n_groups)
    means = np.empty((max(G, 0), k))
    counts = np.zeros(max(G, 0), dtype=np.int64)
    check(fn(ptr(g, i32p), G, ptr(means, f64p), ptr(counts, i64p)))
    return means.T, counts


def _evaluate_call(fn, nrow, ncol, cell_loss, gene_loss):
    """Shared by Context.evaluate, Multi.evaluate and api.evaluate: fn(sse, mse, cell_loss, gene_loss) is the library call."""
    sse, mse = np.zeros(1), np.zeros(1)
    cl = np.empty(max(int(ncol), 1)) if cell_loss else None
    gl = np.empty(max(int(nrow), 1)) if gene_loss else None
    check(fn(ptr(sse, f64p), ptr(mse, f64p), ptr(cl, f64p), ptr(gl, f64p)))
    out = {"sse": float(sse[0]), "mse": float(mse[0])}
    if cell_loss:
        out["cell_loss"] = cl[:int(ncol)]
    if gene_loss:
        out["gene_loss"] = gl[:int(nrow)]
    return out


def _variable_features_call(fn, nrow, nfeatures, span, vmax, expected_var):
    """Shared by Context.variable_features and api.find_variable_features: fn(nfeatures, span, vmax, expected_var, features,
    n_out, info) is the library call."""
    nrow = int(nrow)
    ev = None
    if expected_var is not None:
        ev = np.ascontiguousarray(expected_var, dtype=np.float64)
        if ev.shape != (nrow,):
            raise ValueError("expected_var needs one entry per gene (row) of A")
    nf = int(nfeatures)
    feats = np.zeros(max(min(nf, nrow), 1), dtype=np.int32)
    n_out = C.c_int32()
    info = np.empty((max(nrow, 1), 4))
    check(fn(nf, float(span), 0.0 if vmax is None else float(vmax), ptr(ev, f64p), ptr(feats, i32p), C.byref(n_out), ptr(info, f64p)))
    info = info[:nrow]
    return {"features": feats[:n_out.value].copy(), "mean": info[:, 0].copy(), "variance": info[:, 1].copy(),
            "variance_expected": info[:, 2].copy(), "variance_standardized": info[:, 3].copy()}


class _Handle:
    """One handle of the library -- a context (sgl_*) or a team (sgl_multi_*) -- its lifetime, and the calls both take
    alike: _fn picks the symbol by the class's prefix, _shape gives (nrow, ncol) of the whole resident matrix."""
    _PREFIX = "sgl_"
    _owned = True

    def _fn(self, name):
        return getattr(self._L, self._PREFIX + name)

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_links(self, link_h=None, link_w=None):
        """c_linked_nmf's link matrices (sgl_set_links; rows x cols, as R holds them: link_h rows x cells -- of this shard
        on a Context, of the whole matrix on a Multi --, link_w rows x genes); a matrix whose column count does not match
        its side is ignored, None switches a side off.  Call after fit_init (which drops them)."""
        lh, lhr, lhc, k1 = _link_image(link_h)
        lw, lwr, lwc, k2 = _link_image(link_w)
        check(self._fn("set_links")(self._h, lh, lhr, lhc, lw, lwr, lwc))

    def set_links_grouped(self, table_h, group_h, table_w=None, group_w=None):
        """The grouped form of the links (sgl_set_links_grouped): exactly set_links(table_h[:, group_h], table_w[:, group_w])
        without the expanded matrices -- table_* rows x groups, group_* one 0-based id per cell (gene).  Same bits, same
        lifetime; a None table switches its side off; either call replaces what the other set.  On a Multi group_h holds
        one id per cell of ALL cells and follows them to the ranks; the tables and group_w go to every rank."""
        nr, nc = self._shape()
        th, rh, gh, ph, k1 = _grouped_side(table_h, group_h, nc, "h")
        tw, rw, gw, pw, k2 = _grouped_side(table_w, group_w, nr, "w")
        check(self._fn("set_links_grouped")(self._h, th, rh, gh, ph, tw, rw, gw, pw))

    def set_graph(self, G):
        """c_gcnmf's cell graph (sgl_set_graph): an n x n dgCMatrix-like or scipy sparse matrix over the resident cells (on
        a Multi: over ALL cells), or None to clear it.  Call after fit_init (which drops it).  On a Multi every rank keeps
        the columns of its cells; the columns of B and h that other ranks read travel in a halo exchange per
        half-iteration (graph_info())."""
        G = None if G is None else as_dgCMatrix(G)
        check(self._fn("set_graph")(self._h, *csc_ptrs(G), *((0, 0) if G is None else (G.nrow, G.ncol))))

    def evaluate(self, cell_loss=False, gene_loss=False):
        """Error of the current factors against the resident matrix (sgl_evaluate): {"sse", "mse"} plus, when asked for,
        "cell_loss" (one per cell) and "gene_loss" (one per gene) -- sums of squared residuals of w^T diag(d) h over every
        entry of the column / row, zeros included.  Links and a cell graph on the fit are ignored; the fit is not changed.
        On a Multi cell_loss covers all cells in global order; the ranks' sums and gene partials are added on the host in
        rank order."""
        nr, nc = self._shape() or (0, 0)
        return _evaluate_call(lambda *o: self._fn("evaluate")(self._h, *o), nr, nc, cell_loss, gene_loss)

    def _nmf_run(self, tol, maxit, L1_w, L1_h, L2_w, L2_h, log=None, poll=None):
        out = NmfOutputs(None, maxit)
        cb = make_callbacks(log, poll)
        check(self._fn("nmf_run")(self._h, tol, int(maxit), L1_w, L1_h, L2_w, L2_h, *out.args(), C.byref(cb)))
        return out

    def nmf_run(self, tol, maxit, L1_w, L1_h, L2_w, L2_h, log=None, poll=None):
        return self._nmf_run(tol, maxit, L1_w, L1_h, L2_w, L2_h, log, poll).run()

    def _ard_run(self, tol, maxit, L1, L2, seed, inv_density, overfit_threshold, trace_test_mse, log=None, poll=None):
        out = ArdOutputs(None, maxit, nit=True)
        cb = make_callbacks(log, poll)
        check(self._fn("ard_run")(self._h, tol, int(maxit), L1, L2, int(seed), int(inv_density), overfit_threshold,
                                  int(trace_test_mse), *out.args(), C.byref(cb)))
        return out

    def ard_run(self, tol, maxit, L1, L2, seed, inv_density, overfit_threshold, trace_test_mse, log=None, poll=None):
        out = self._ard_run(tol, maxit, L1, L2, seed, inv_density, overfit_threshold, trace_test_mse, log, poll)
        return dict(out.traces(), n_iter=out.nit.value)


class Context(_Handle):
    def __init__(self, device=0, _borrowed=None):
        self._L = _lib.load()
        if _borrowed is not None:   # a rank of a Multi: owned by it
            self._h = _borrowed
            self._owned = False
            self.device = None
        else:
            h = C.c_void_p()
            check(self._L.sgl_create(int(device), C.byref(h)))
            self._h = h
            self._owned = True
            self.device = int(device)
        self._keep = []
        self.k = 0

    def _shape(self):
        return self.dims()[:2]

    def comm_init_rank(self, nranks, rank, comm_id):
        """Join the native team of `nranks` processes (one per GPU) with the id rank 0 made
        (comm_unique_id); call before fit_init.  nmf_iterate / nmf_run then exchange over RCCL."""
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError("comm_id must be %d bytes" % COMM_ID_BYTES)
        buf = C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        check(self._L.sgl_comm_init_rank(self._h, int(nranks), int(rank), buf))

    def comm_info(self):
        """What the library's own communicator reports: ranks (ncclCommCount), whether it is RCCL, the library bound."""
        n, r = C.c_int32(), C.c_int32()
        buf = C.create_string_buffer(512)
        check(self._L.sgl_comm_info(self._h, C.byref(n), C.byref(r), buf, 512))
        return {"nranks": n.value, "is_rccl": bool(r.value), "path": buf.value.decode("utf-8", "replace")}

    def nmf_iterate(self, L1_w, L1_h, L2_w, L2_h):
        """One ALS iteration (any exchange mode); returns tol."""
        t = C.c_double()
        check(self._L.sgl_nmf_iterate(self._h, L1_w, L1_h, L2_w, L2_h, C.byref(t)))
        return t.value

    # -- matrix -----------------------------------------------------------
    def upload(self, A, At=None, cell_offset=0, ncells_total=0):
        if At is not None and At.Dim != (A.Dim[1], A.Dim[0]):
            raise ValueError("At must be the transpose of A")
        check(self._L.sgl_upload_csc(self._h, *csc_ptrs(A), *csc_ptrs(At), A.nrow, A.ncol, int(cell_offset), int(ncells_total)))
        self.k = 0

    def upload_list(self, chunks, t_chunks=None, cell_offset=0, ncells_total=0):
        """sgl_upload_csc_list: a list of column chunks of A joined into one resident shard (64-bit column pointers);
        t_chunks: the column chunks of t(A), or None / empty to build the transpose on the device."""
        a, t, nrow, _, keep = _chunk_lists(chunks, t_chunks, "the chunk list must hold at least one matrix",
                                           "all chunks must have the same number of rows")
        check(self._L.sgl_upload_csc_list(self._h, *a, *t, nrow, int(cell_offset), int(ncells_total)))
        self.k = 0

    def upload_native(self, N, sort=True, cell_offset=0, ncells_total=0):
        """sgl_upload_typed: a NativeMatrix (native()) goes in as its owner holds it -- converted, validated, sorted (sort =
        True: the indices of a slice may come in any order) and transposed on the device; the resident image is bit for
        bit that of upload(as_dgCMatrix(...)).  A torch GPU tensor is read where it lies (its device must be this
        context's; its current stream is synchronised first), everything else is copied once from host memory.
        Returns the report: nnz, sorted_lds / sorted_long (slices sorted by either path), integral (every stored value
        equals its truncation), bytes_copied, lds_capacity."""
        from .native import NativeMatrix, REPORT_KEYS, SGL_SPACE_DEVICE, SGL_UP_SORT
        if not isinstance(N, NativeMatrix):
            raise TypeError("upload_native takes what native() returns")
        if N.space == SGL_SPACE_DEVICE:
            if N.device != self.device:
                raise ValueError("upload_native: the tensors live on GPU %r, this context on GPU %r" % (N.device, self.device))
            import torch
            torch.cuda.current_stream(N.device).synchronize()
        try:
            N.check_entry_count()
        except ValueError:
            # the library cannot see the arrays' length, so this refusal is made here; like every refused upload it
            # leaves no matrix resident (a call without arrays is refused by the library after it dropped the matrix)
            self._L.sgl_upload_typed(self._h, None, 0, None, 0, None, 0, 0, 0, 0, 0, 0, 0, 0, None)
            self.k = 0
            raise
        report = np.zeros(8, dtype=np.int64)
        x, i, p = (C.c_void_p(a) for a in N.addresses())
        check(self._L.sgl_upload_typed(self._h, x, N.x_type, i, N.idx_type, p, N.ptr_type, N.n_major, N.n_minor, N.major_is_genes,
                                       N.space, SGL_UP_SORT if sort else 0, int(cell_offset), int(ncells_total), ptr(report, i64p)))
        self.k = 0
        return dict(zip(REPORT_KEYS, (int(v) for v in report)))

    def upload_dense(self, A):
        """A: dense (nrow, ncol) array (sgl_upload_dense: CSC image built on the device, GEMM right-hand sides when
        more than half of it is non-zero)."""
        A = np.asarray(A, dtype=np.float64)
        Af = np.ascontiguousarray(A.T)   # column-major image
        check(self._L.sgl_upload_dense(self._h, ptr(Af, f64p), A.shape[0], A.shape[1]))
        self.k = 0

    def synth(self, ngenes, ncells_local, inv_density=20, seed=SYNTH_SEED, cell_offset=0, ncells_total=0, skew=None):
        """skew = (sigma_cells, sigma_genes): the skewed generator (log-normal weights per cell and per gene)."""
        lv = _f(LEVELS16)
        if skew is None:
            check(self._L.sgl_synth_csc(self._h, seed, inv_density, ptr(lv, f64p), int(ngenes), int(cell_offset),
                                        int(ncells_local), int(ncells_total)))
        else:
            cw, gw = _f(skew_weights16(skew[0])), _f(skew_weights16(skew[1]))
            check(self._L.sgl_synth_csc_skewed(self._h, seed, inv_density, ptr(lv, f64p), int(ngenes), int(cell_offset),
                                               int(ncells_local), int(ncells_total), ptr(cw, f64p), ptr(gw, f64p)))
        self.k = 0

    def dims(self):
        nr, nc, nz = C.c_int32(), C.c_int32(), C.c_int64()
        check(self._L.sgl_dims(self._h, C.byref(nr), C.byref(nc), C.byref(nz)))
        return nr.value, nc.value, nz.value

    def download(self, which=0):
        nr, nc, nz = self.dims()
        ncol = nr if which else nc
        x = np.empty(nz)
        i = np.empty(nz, dtype=np.int32)
        p = np.empty(ncol + 1, dtype=np.int64)
        check(self._L.sgl_download_csc(self._h, int(which), ptr(x, f64p), ptr(i, i32p), ptr(p, i64p)))
        return x, i, p

    def col_counts(self, which=0):
        """Non-zeros per column of the resident A (which = 0: per cell) or t(A) (which = 1: per gene): the column
        pointers only (sgl_download_csc with NULL value / index buffers)."""
        nr, nc, _ = self.dims()
        p = np.empty((nr if which else nc) + 1, dtype=np.int64)
        check(self._L.sgl_download_csc(self._h, int(which), None, None, ptr(p, i64p)))
        return np.diff(p)

    # -- fit ----------------------------------------------------------------
    def log_normalize(self, scale_factor=10000.0):
        """Seurat::LogNormalize on the resident shard (R/PreprocessData.R:34-39)."""
        check(self._L.sgl_log_normalize(self._h, float(scale_factor)))
        self.k = 0

    def rasterize_rowwise(self, n):
        """RasterizeRowwise on the resident matrix (sgl_rasterize_rowwise): it becomes the floor(nrow / n) x ncol matrix of
        the means of every n consecutive rows, resident as upload_dense leaves a dense matrix; a running fit is dropped."""
        from .api import _bin_size
        check(self._L.sgl_rasterize_rowwise(self._h, _bin_size(n, "rasterize_rowwise")))
        self.k = 0

    def subset(self, rows=None, cols=None):
        """A <- A[rows, cols] on the resident matrix (sgl_subset): 0-based int32 index lists in any order, duplicates
        allowed; None keeps the axis.  Both orientations are rebuilt on the device; a running fit is dropped."""
        def lst(v):
            if v is None:
                return None, 0
            a = np.ascontiguousarray(v, dtype=np.int32)
            if a.ndim != 1:
                raise ValueError("subset: an index list must be one-dimensional")
            n = int(a.shape[0])
            # an empty list is not None: it goes down as a non-NULL pointer with n = 0, which the library refuses
            return (a if n else np.zeros(1, dtype=np.int32)), n
        r, nr = lst(rows)
        cl, nc = lst(cols)
        check(self._L.sgl_subset(self._h, ptr(r, i32p), nr, ptr(cl, i32p), nc))
        self.k = 0

    @staticmethod
    def _parent_lists(parent_a, parent_b, who):
        """The two parent lists as int32 arrays of one length (an empty list still goes down with an address: the library
        refuses n_sim = 0 itself); None stays None, which the library refuses as a NULL list."""
        out = []
        for v in (parent_a, parent_b):
            if v is None:
                out.append(None)
                continue
            a = np.asarray(v)
            if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
                raise ValueError("%s: a parent list must be a one-dimensional list of 0-based cell indices" % who)
            if a.size and (a.min() < -2**31 or a.max() >= 2**31):
                raise ValueError("%s: a parent index is outside the 32-bit range" % who)
            out.append(np.ascontiguousarray(a, dtype=np.int32))
        sizes = {a.shape[0] for a in out if a is not None}
        if len(sizes) > 1:
            raise ValueError("%s: parent_a and parent_b must have the same length" % who)
        n = sizes.pop() if sizes else 0
        return [a if a is None or n else np.zeros(1, dtype=np.int32) for a in out] + [n]

    def simulate_doublets(self, dst, parent_a, parent_b):
        """The resident matrix of `dst` (another Context on this device) becomes S, S[:, s] = A[:, parent_a[s]] +
        A[:, parent_b[s]] over this context's resident matrix, which is only read (sgl_simulate_doublets; the rules are in
        include/singlet_hip.h, "Simulated doublets").  A fit of dst is dropped; this context keeps its matrix and its fit."""
        if not isinstance(dst, Context):
            raise TypeError("simulate_doublets: dst must be a Context")
        a, b, n = self._parent_lists(parent_a, parent_b, "simulate_doublets")
        check(self._L.sgl_simulate_doublets(self._h, dst._h, ptr(a, i32p), ptr(b, i32p), n))
        dst.k = 0

    def doublets_info(self):
        """What the last simulate_doublets INTO this context, or the last op_pair_columns on it, ran (sgl_doublets_info):
        {"lds_pairs", "long_pairs", "entries" (stored entries of S), "shared_rows" (rows stored in both parents)}."""
        out = np.zeros(4, dtype=np.int64)
        check(self._L.sgl_doublets_info(self._h, ptr(out, i64p)))
        return dict(zip(("lds_pairs", "long_pairs", "entries", "shared_rows"), (int(v) for v in out)))

    def weight_by_split(self, split_by, n_groups):
        """weight_by_split (src/singlet.cpp:119-144) on the resident shard; split_by: 0-based group per local cell."""
        sb = np.ascontiguousarray(split_by, dtype=np.int32)
        _, nc, _ = self.dims()
        if sb.shape != (nc,):
            raise ValueError("split_by must have one entry per cell (column) of A")
        check(self._L.sgl_weight_by_split(self._h, ptr(sb, i32p), int(n_groups)))
        self.k = 0

    def fit_init(self, k, w_init=None, synth_seed=SYNTH_SEED):
        """w_init: (m, k) C-contiguous (== k x m column-major) or None for the synthetic init."""
        w = None
        if w_init is not None:
            w = _f(w_init)
            nr, _, _ = self.dims()
            if w.shape != (nr, k):
                raise ValueError("w_init must be k x nrow(A) (got %r for k=%d, nrow=%d)" % (w.shape[::-1], k, nr))
        check(self._L.sgl_fit_init(self._h, int(k), ptr(w, f64p), synth_seed))
        self.k = int(k)

    def group_means(self, group, n_groups, F=None):
        """(means k x n_groups, counts) of the columns of F (k x n, R's orientation) per group (sgl_group_means); F = None:
        of the H of the current fit, read where it is.  An empty group gives a NaN column and a count of 0."""
        if F is None:
            _, n, _ = self.dims()
            k, Fp = self.k, None
            if k == 0:   # no fit: the library refuses (SGL_ESTATE) before it reads the list
                n = None
        else:
            buf = colmajor(F, "F must be a k x n matrix")
            n, k = buf.shape
            Fp = ptr(buf, f64p)
        g = _group_list(group, n, "group")
        return _group_means_call(lambda *o: self._L.sgl_group_means(self._h, Fp, int(k), int(g.shape[0]), *o), g, n_groups, k)

    def _embedding_in(self, F):
        """(the column-major image kept alive or None, its pointer or None, k, n) of the embedding argument of the annotation
        calls; F = None: the held embedding, else the H of the current fit."""
        if F is None:
            held = getattr(self, "_held_embedding", None)
            if held is not None:
                return None, None, held[0], held[1]
            _, n, _ = self.dims()
            return None, None, self.k, (n if self.k else None)   # no fit: the library refuses (SGL_ESTATE) before it reads the list
        buf = colmajor(F, "F must be a k x n matrix")
        return buf, ptr(buf, f64p), buf.shape[1], buf.shape[0]

    def hold_embedding(self, F):
        """Keeps a device copy of F (k x n) for the annotation calls, which read it when their F is None (sgl_annotate_hold);
        F = None drops it."""
        if F is None:
            check(self._L.sgl_annotate_hold(self._h, None, 0, 0))
            self._held_embedding = None
            return
        buf = colmajor(F, "F must be a k x n matrix")
        self._held_embedding = None
        check(self._L.sgl_annotate_hold(self._h, ptr(buf, f64p), buf.shape[1], buf.shape[0]))
        self._held_embedding = (buf.shape[1], buf.shape[0])

    def group_moments(self, labels, n_groups=None, F=None):
        """(group_n, sum k x G, rss k) of a means model over the columns of F (k x n, R's orientation) under the labels (one in
        [-1, G) per cell, -1: left out) (sgl_group_moments); F = None: of the H of the current fit, read where it is."""
        _buf, Fp, k, n = self._embedding_in(F)
        g, G = label_list(labels, n, n_groups)
        kk, Gs = max(int(k), 1), max(min(G, 1024), 1)
        group_n, s, rss = np.zeros(Gs, dtype=np.int64), np.zeros((Gs, kk)), np.zeros(kk)
        check(self._L.sgl_group_moments(self._h, Fp, int(k), int(g.shape[0]), ptr(g, i32p), G, ptr(group_n, i64p), ptr(s, f64p), ptr(rss, f64p)))
        return group_n, s[:, :k].T, rss[:k]

    def gene_group_moments(self, labels, n_groups=None):
        """(group_n, nz m x G, sum m x G, rss m) of the same model over the genes of the resident matrix (sgl_gene_group_moments)."""
        nr, nc, _ = self.dims()
        g, G = label_list(labels, nc or None, n_groups)   # (no matrix: the library refuses)
        m, Gs = max(nr, 1), max(min(G, 1024), 1)
        group_n, nz, s, rss = np.zeros(Gs, dtype=np.int64), np.zeros((Gs, m), dtype=np.int64), np.zeros((Gs, m)), np.zeros(m)
        check(self._L.sgl_gene_group_moments(self._h, ptr(g, i32p), G, ptr(group_n, i64p), ptr(nz, i64p), ptr(s, f64p), ptr(rss, f64p)))
        return group_n, nz[:, :nr].T, s[:, :nr].T, rss[:nr]

    def annotate(self, labels, n_groups=None, F=None, center=True, scale=False, proportion=0.01, tail="pos"):
        """The means-model fit of every row of F (k x n; None: the resident H) against the labels with the moderated statistics
        (sgl_annotate; the rules: include/singlet_hip.h, "Factor annotation"): the dict of annotate_stats."""
        _buf, Fp, k, n = self._embedding_in(F)
        g, G = label_list(labels, n, n_groups)
        return annotate_call(lambda *a: self._L.sgl_annotate(self._h, Fp, int(k), int(g.shape[0]), ptr(g, i32p), G, *a), k, G, center, scale,
                             proportion, tail)

    def annotate_genes(self, labels, n_groups=None, center=True, scale=False, proportion=0.01, tail="pos"):
        """The same fit of every gene of the resident matrix (sgl_annotate_genes); the dict also holds "nz"."""
        nr, nc, _ = self.dims()
        g, G = label_list(labels, nc or None, n_groups)   # (no matrix: the library refuses)
        return annotate_call(lambda *a: self._L.sgl_annotate_genes(self._h, ptr(g, i32p), G, *a), nr, G, center, scale, proportion, tail,
                             with_nz=True)

    @staticmethod
    def _gene_list(genes, who):
        """(the int32 array kept alive or None, its length) of a list of distinct 0-based gene indices; None: all genes.  The
        library checks the range and the repeats itself and names the offender."""
        if genes is None:
            return None, 0
        a = np.asarray(genes)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("%s: genes must be a one-dimensional list of 0-based gene indices" % who)
        if a.size and (a.min() < -2**31 or a.max() >= 2**31):
            raise ValueError("%s: a gene index is outside the 32-bit range" % who)
        n = int(a.shape[0])
        return (np.ascontiguousarray(a, dtype=np.int32) if n else np.zeros(1, dtype=np.int32)), n

    @staticmethod
    def _square_graph(G, who):
        G = as_dgCMatrix(G)
        if G.nrow != G.ncol:
            raise ValueError("%s: the graph is %d x %d, not square" % (who, G.nrow, G.ncol))
        return G

    def moran(self, G, genes=None):
        """The per-gene moments behind Moran's I of the resident matrix over the n x n cell graph G (sgl_moran; the rules:
        include/singlet_hip.h, "Spatial autocorrelation"): a 6 x n_genes array with the rows mean, M2, M4, T, P, c_g, in the
        order of `genes` (None: all genes).  The graph is used as given.  The matrix and a running fit are only read."""
        G = self._square_graph(G, "moran")
        g, ng = self._gene_list(genes, "moran")
        nr, _, _ = self.dims()
        rows = ng if genes is not None else nr
        out = np.zeros((max(rows, 1), 6))
        check(self._L.sgl_moran(self._h, *csc_ptrs(G), G.ncol, ptr(g, i32p), ng, ptr(out, f64p)))
        return out[:rows].T

    def op_moran_cross(self, G, genes=None, path=0, lds_cap=0, table_batch=0):
        """P of sgl_moran alone (sgl_op_moran_cross): one value per listed gene.  path 0 automatic, 1 the search path, 2 the
        table path; lds_cap and table_batch 0: the defaults.  The result does not depend on any of them; moran_info() says
        what ran."""
        G = self._square_graph(G, "op_moran_cross")
        g, ng = self._gene_list(genes, "op_moran_cross")
        nr, _, _ = self.dims()
        rows = ng if genes is not None else nr
        out = np.zeros(max(rows, 1))
        check(self._L.sgl_op_moran_cross(self._h, *csc_ptrs(G), G.ncol, ptr(g, i32p), ng, int(path), int(lds_cap), int(table_batch),
                                         ptr(out, f64p)))
        return out[:rows]

    def moran_info(self):
        """What the last moran / op_moran_cross on this context ran (sgl_moran_info): {"search_genes", "table_genes",
        "batches", "table_batch", "table_bytes", "lds_cap"}."""
        out = np.zeros(6, dtype=np.int64)
        check(self._L.sgl_moran_info(self._h, ptr(out, i64p)))
        return dict(zip(("search_genes", "table_genes", "batches", "table_batch", "table_bytes", "lds_cap"), (int(v) for v in out)))

    def moran_embedding(self, G, F=None):
        """(moments 6 x k, mean k) behind Moran's I of the rows of F (k x n; None: the held embedding, else the H of the current
        fit, read where it is) over the cell graph G (sgl_moran_embedding).  The rows of the moments are +0.0, M2, M4, +0.0,
        C, n: the embedding is centred before the sums, so moran_stats takes them as they are."""
        G = self._square_graph(G, "moran_embedding")
        _buf, Fp, k, n = self._embedding_in(F)
        if F is not None and n != G.ncol:
            raise ValueError("moran_embedding: F has %d columns, the graph %d cells" % (n, G.ncol))
        kk = max(min(int(k), 1024), 1)
        out, mean = np.zeros((kk, 6)), np.zeros(kk)
        check(self._L.sgl_moran_embedding(self._h, *csc_ptrs(G), G.ncol, Fp, int(k), ptr(out, f64p), ptr(mean, f64p)))
        return out[:k].T, mean[:k]

    def nhood_enrichment(self, G, labels, n_classes=None, nperm=1000, seed=0, drop_diagonal=True, batch=0, return_null=False):
        """The integer tallies of the neighbourhood enrichment test of the classes `labels` on the n x n cell graph G
        (sgl_nhood_enrichment; the rules: include/singlet_hip.h, "Neighbourhood enrichment"): {"counts", "S1", "S2", "n_ge",
        "n_le"}, K x K int64 each, [a, b] = centre class a, neighbour class b; with return_null also "null", nperm x K x K.
        n_classes None: 1 + the largest label.  The stored values of G are not read.  Nothing of the context is touched;
        nhood_info() says what ran; nhood_stats turns the tallies into z, p and p_adj."""
        G = self._square_graph(G, "nhood_enrichment")
        lab, K = nhood_labels(labels, G.ncol, n_classes, "nhood_enrichment")
        kk = max(min(K, 256), 1)
        t = [np.zeros((kk, kk), dtype=np.int64) for _ in NHOOD_TALLIES]
        null = np.zeros((max(min(int(nperm), 1 << 20), 1), kk, kk), dtype=np.int64) if return_null else None
        check(self._L.sgl_nhood_enrichment(self._h, ptr(G.i, i32p), ptr(G.p, i32p), G.ncol, ptr(lab, i32p), K, int(bool(drop_diagonal)), int(nperm),
                                           int(seed), int(batch), *(ptr(a, i64p) for a in t), ptr(null, i64p)))
        out = {name: np.ascontiguousarray(a.T) for name, a in zip(NHOOD_TALLIES, t)}
        if return_null:
            out["null"] = np.ascontiguousarray(null.transpose(0, 2, 1))
        return out

    def op_nhood_permute(self, labels, seed=0, r0=0, nb=1):
        """lab_r of the permutations [r0, r0 + nb) of the neighbourhood enrichment null (sgl_op_nhood_permute): nb x n int32."""
        lab, _ = nhood_labels(labels, None, None, "op_nhood_permute")
        n = int(lab.shape[0])
        out = np.zeros((max(int(nb), 1), max(n, 1)), dtype=np.int32)
        check(self._L.sgl_op_nhood_permute(self._h, n, ptr(lab, i32p), int(seed), int(r0), int(nb), ptr(out, i32p)))
        return out[:, :n]

    def op_nhood_tally(self, G, labs, n_classes, drop_diagonal=True, path=0, perms_per_group=0):
        """The class-pair counts of G under each of nb given label vectors (labs nb x n; sgl_op_nhood_tally): nb x K x K int64,
        [q, a, b] = centre class a, neighbour class b.  path 0 automatic, 1 the LDS path, 2 the global path; perms_per_group 0:
        the plan's value.  The result depends on neither; nhood_info() says what ran."""
        G = self._square_graph(G, "op_nhood_tally")
        L = np.asarray(labs)
        if L.ndim != 2 or L.shape[1] != G.ncol or (L.size and L.dtype.kind not in "iub"):
            raise ValueError("op_nhood_tally: labs must be an nb x n integer matrix with one column per cell (%d)" % G.ncol)
        nb, K = int(L.shape[0]), int(n_classes)
        L = np.ascontiguousarray(L, dtype=np.int32)
        kk = max(min(K, 256), 1)
        out = np.zeros((max(nb, 1), kk, kk), dtype=np.int64)
        check(self._L.sgl_op_nhood_tally(self._h, ptr(G.i, i32p), ptr(G.p, i32p), G.ncol, ptr(L, i32p), nb, K, int(bool(drop_diagonal)), int(path),
                                         int(perms_per_group), ptr(out, i64p)))
        return np.ascontiguousarray(out[:nb].transpose(0, 2, 1))

    def nhood_info(self):
        """What the last neighbourhood enrichment call on this context ran (sgl_nhood_info): {"path" (1 LDS, 2 global, 0 no
        tally), "perms_per_group", "batches", "batch", "lds_bytes", "sort" (0 segmented, 1 device-wide)}."""
        out = np.zeros(6, dtype=np.int64)
        check(self._L.sgl_nhood_info(self._h, ptr(out, i64p)))
        return dict(zip(NHOOD_INFO, (int(v) for v in out)))

    def ligrec(self, labels, genes, lig, rec, n_classes=None, nperm=1000, seed=0, batch=0, return_null=False):
        """The ligand-receptor permutation test of the resident matrix (sgl_ligrec; the rules: include/singlet_hip.h,
        "Ligand-receptor interactions"): genes = distinct 0-based gene indices, lig / rec = indices into genes, one pair each.
        Returns {"group_n" (K), "nz", "sum", "mean" (G x K), "score", "n_ge" (P x K x K, [q, a, b] = ligand class a, receptor
        class b)}; with return_null also "null", nperm x P x K x K.  The matrix and a running fit are only read; ligrec_info()
        says what ran; ligrec_stats turns the tallies into p and padj."""
        lab, K, g, G, lg, rc, P = ligrec_inputs(labels, None, n_classes, genes, lig, rec, "ligrec")
        return ligrec_call(lambda *a: self._L.sgl_ligrec(self._h, ptr(lab, i32p), int(lab.shape[0]), K, ptr(g, i32p), G, ptr(lg, i32p), ptr(rc, i32p), P,
                                                         int(nperm), int(seed), int(batch), *a), K, G, P, nperm, return_null)

    def op_ligrec_sums(self, labs, n_classes, genes, path=0, vectors_per_wave=0):
        """The per-class sums of the listed genes under each of nb given label vectors (labs nb x n; sgl_op_ligrec_sums):
        nb x G x K doubles.  path 0 automatic, 1 the LDS path, 2 the global path; vectors_per_wave 0: the plan's value.  The
        result depends on neither; ligrec_info() says what ran."""
        L = np.asarray(labs)
        if L.ndim != 2 or (L.size and L.dtype.kind not in "iub"):
            raise ValueError("op_ligrec_sums: labs must be an nb x n integer matrix with one column per cell")
        L = np.ascontiguousarray(L, dtype=np.int32)
        g = np.ascontiguousarray(np.asarray(genes), dtype=np.int32)
        nb, n, K, G = int(L.shape[0]), int(L.shape[1]), int(n_classes), int(g.shape[0])
        out = np.zeros((max(nb, 1), max(G, 1), max(min(K, 256), 1)))
        check(self._L.sgl_op_ligrec_sums(self._h, ptr(L, i32p), n, nb, K, ptr(g, i32p), G, int(path), int(vectors_per_wave), ptr(out, f64p)))
        return out[:nb]

    def op_ligrec_tally(self, mean_obs, means, lig, rec, return_null=False):
        """The scores and the tallies from mean tables alone (sgl_op_ligrec_tally): mean_obs G x K, means nb x G x K.  Returns
        (score, n_ge), P x K x K each; with return_null also the s_r, nb x P x K x K."""
        mo, mm = np.ascontiguousarray(mean_obs, dtype=np.float64), np.ascontiguousarray(means, dtype=np.float64)
        if mo.ndim != 2 or mm.ndim != 3 or mm.shape[1:] != mo.shape:
            raise ValueError("op_ligrec_tally: mean_obs must be G x K and means nb x G x K")
        lg, rc = np.ascontiguousarray(lig, dtype=np.int32), np.ascontiguousarray(rec, dtype=np.int32)
        if lg.ndim != 1 or lg.shape != rc.shape:
            raise ValueError("op_ligrec_tally: lig and rec must hold one index each per pair")
        G, K, nb, P = int(mo.shape[0]), int(mo.shape[1]), int(mm.shape[0]), int(lg.shape[0])
        kk, pp = max(min(K, 256), 1), max(P, 1)
        score, n_ge = np.zeros((kk, kk, pp)), np.zeros((kk, kk, pp), dtype=np.int64)
        null = np.zeros((max(nb, 1), kk, kk, pp)) if return_null else None
        check(self._L.sgl_op_ligrec_tally(self._h, ptr(mo, f64p), ptr(mm, f64p), nb, K, G, ptr(lg, i32p), ptr(rc, i32p), P, ptr(score, f64p),
                                          ptr(n_ge, i64p), ptr(null, f64p)))
        out = (np.ascontiguousarray(score.transpose(2, 1, 0)), np.ascontiguousarray(n_ge.transpose(2, 1, 0)))
        return out + (np.ascontiguousarray(null.transpose(0, 3, 2, 1)),) if return_null else out

    def ligrec_info(self):
        """What the last ligand-receptor call on this context ran (sgl_ligrec_info): {"path" (1 LDS, 2 global, 0 none),
        "vectors_per_wave", "batches", "batch", "lds_bytes", "waves", "lds_genes", "global_genes"}."""
        out = np.zeros(8, dtype=np.int64)
        check(self._L.sgl_ligrec_info(self._h, ptr(out, i64p)))
        return dict(zip(LIGREC_INFO, (int(v) for v in out)))

    def cooccur(self, coords, labels, interval, n_classes=None):
        """The co-occurrence tally of the classes `labels` of the points `coords` (n x 2, or a pair of vectors) over the distance
        intervals (interval[t], interval[t + 1]] (sgl_cooccur; the rules: include/singlet_hip.h, "Co-occurrence by distance"):
        K x K x T int64, [a, b, t] = the ordered pairs (i, j), i != j, of classes a, b whose distance lies in interval t.
        n_classes None: 1 + the largest label.  Nothing of the context is touched; cooccur_info() says what ran.  ARGUMENT ORDER:
        the data first, then the labels, as every call on a context (nhood_enrichment(G, labels), ...) and c_cooccur; the
        user-facing co_occurrence / ripley take the labels first, as nhood_enrichment(labels, ...) does."""
        return self.op_cooccur_tally(coords, labels, interval, n_classes, _whole=True)

    def op_cooccur_tally(self, coords, labels, interval, n_classes=None, grid_mode=0, bin_path=0, flush_pairs=0, _whole=False):
        """Context.cooccur with the knobs of its plan (sgl_op_cooccur_tally): grid_mode 0 the plan, 1 one bucket (all pairs), 2
        the bucket grid; bin_path 0 the plan, 1 the LDS path, 2 the global path; flush_pairs 0 the plan's bound, otherwise a
        smaller one.  The result depends on none of them; cooccur_info() says what ran."""
        from ._cooccur import abt, cooccur_inputs, table_shape
        who = "cooccur" if _whole else "op_cooccur_tally"
        c1, c2, n, lab, K, r, T = cooccur_inputs(coords, labels, interval, n_classes, who)
        out = np.zeros(table_shape(K, T), dtype=np.int64)
        if _whole:
            check(self._L.sgl_cooccur(self._h, ptr(c1, f64p), ptr(c2, f64p), n, ptr(lab, i32p), K, ptr(r, f64p), T, ptr(out, i64p)))
        else:
            check(self._L.sgl_op_cooccur_tally(self._h, ptr(c1, f64p), ptr(c2, f64p), n, ptr(lab, i32p), K, ptr(r, f64p), T, int(grid_mode),
                                               int(bin_path), int(flush_pairs), ptr(out, i64p)))
        return abt(out, K, T)

    def cooccur_info(self):
        """What the last co-occurrence call on this context ran (sgl_cooccur_info): {"grid_mode" (1 one bucket, 2 the bucket
        grid, 0 none ran), "W", "H", "bin_path" (1 LDS, 2 global), "lds_bytes", "workgroups", "flushes", "pairs"}."""
        from ._cooccur import COOCCUR_INFO
        out = np.zeros(8, dtype=np.int64)
        check(self._L.sgl_cooccur_info(self._h, ptr(out, i64p)))
        return dict(zip(COOCCUR_INFO, (int(v) for v in out)))

    def variable_features(self, nfeatures=2000, span=0.3, vmax=None, expected_var=None):
        """Variable features of the resident counts (sgl_variable_features; Seurat's vst selection under this library's
        stated rules): {"features" (int32 gene indices in rank order), "mean", "variance", "variance_expected",
        "variance_standardized"} (one value per gene).  vmax None: sqrt(ncol).  expected_var: one expected variance per
        gene, used instead of the trend (another loess's, for parity with it).  The matrix and a running fit are only read."""
        nr, _, _ = self.dims()
        return _variable_features_call(lambda *a: self._L.sgl_variable_features(self._h, *a), nr, nfeatures, span, vmax, expected_var)

    def markers(self, labels, n_groups=None, transform="expm1", pseudocount=1.0):
        """The one-vs-rest Wilcoxon rank-sum test of every gene against every cluster of the resident matrix (sgl_markers;
        the rules are stated in include/singlet_hip.h, "Marker genes").  labels: one cluster id in [-1, G) per cell, -1
        leaves the cell out; n_groups None: 1 + the largest label.  transform: "expm1" (Seurat's mean of log-normalised
        data) or "identity".  Returns {"group_n" (G), "tie" (m), and m x G arrays "pos", "sum", "rank2", "pct_in",
        "pct_out", "log2fc", "z", "p"}.  The matrix and a running fit are only read."""
        nr, nc, _ = self.dims()
        g, G = label_list(labels, nc or None, n_groups)   # (no matrix: the library refuses)
        return markers_call(lambda *a: self._L.sgl_markers(self._h, *a), nr, g, G, transform, pseudocount)

    def markers_info(self):
        """What the last rank pass on this context ran (sgl_markers_info): {"lds_genes", "long_genes", "batches", "lds_cap"}."""
        out = np.zeros(4, dtype=np.int64)
        check(self._L.sgl_markers_info(self._h, ptr(out, i64p)))
        return dict(zip(("lds_genes", "long_genes", "batches", "lds_cap"), (int(v) for v in out)))

    def signature_scores(self, sets, max_rank=1500, return_rank2=False):
        """The rank-based UCell score of every gene set in every cell of the resident matrix (sgl_signature_scores; the rules
        are stated in include/singlet_hip.h, "Signature scores").  sets: a list of sequences of 0-based gene indices, one per
        set (no gene twice in a set, at most max_rank genes).  Returns score, n_sets x ncol; with return_rank2 (rank2, score),
        rank2 the uint64 sums of the doubled capped midranks.  The matrix and a running fit are only read."""
        _, nc, _ = self.dims()
        return signature_call(lambda *a: self._L.sgl_signature_scores(self._h, *a), nc, sets, max_rank, return_rank2)

    def signature_info(self):
        """What the last signature call on this context ran (sgl_signature_info): {"lds_small", "lds_large", "long_cells",
        "batches", "passes", "lds_cap", "batch_cap", "pass_sets"}."""
        out = np.zeros(8, dtype=np.int64)
        check(self._L.sgl_signature_info(self._h, ptr(out, i64p)))
        return dict(zip(("lds_small", "lds_large", "long_cells", "batches", "passes", "lds_cap", "batch_cap", "pass_sets"), (int(v) for v in out)))

    def knn(self, n_neighbors=20, reference=None, query=None, dims=None, metric="euclidean", method="exact", n_lists=None, n_probe=None,
            n_iter=10):
        """Exact nearest neighbours in an embedding (sgl_knn): (idx, dist), each n_query x n_neighbors, row j = the
        n_neighbors nearest reference columns of query column j in rank order -- by (squared distance, index), ties to
        the lower index -- and their Euclidean distances.  reference: k x n (R's orientation); None: the H of the current
        fit, read where it is, in the fit's stored factor order.  query: k x n_query; None: the references themselves (a
        cell is then its own first neighbour unless n_neighbors identical columns precede it).  dims: 0-based rows.  The
        context and a running fit are only read.  metric: "euclidean"; "cosine" or "correlation" (sgl_knn_metric) rank by
        1 - the dot of the unit columns (for correlation of the columns centred by their own mean) and return that key as
        the distance, exactly +0.0 between a cell and its duplicates or power-of-two multiples.  method "ivf" (sgl_knn_ivf):
        the approximate inverted-list search -- n_lists lists from n_iter Lloyd steps of a coarse k-means (None:
        ceil(sqrt(n_ref))), of which a query scans the n_probe nearest (None: the default of knn_ivf_host.h); a query whose
        probed lists hold fewer than n_neighbors cells has -1 / +Inf in its last slots (knn_ivf_info counts them), and
        n_probe == n_lists is the exact search bit for bit.  The rules are in include/singlet_hip.h."""
        code = knn_metric(metric)
        resident = None
        if reference is None:
            _, n, _ = self.dims()
            resident = (self.k, n)
        if knn_method(method):
            return knn_call(lambda *a: self._L.sgl_knn_ivf(self._h, *a), reference, query, dims, n_neighbors, resident, code,
                            lambda n_ref, nd: (*knn_ivf_shape(n_ref, n_lists, n_probe), int(n_iter)))
        if code:
            return knn_call(lambda *a: self._L.sgl_knn_metric(self._h, *a), reference, query, dims, n_neighbors, resident, code)
        return knn_call(lambda *a: self._L.sgl_knn(self._h, *a), reference, query, dims, n_neighbors, resident)

    def knn_info(self):
        """What the last knn() on this context ran (sgl_knn_info): {"instance" (0 .. 3: coordinates in registers up to 8,
        16, 32, 64 dimensions; 4: the generic kernel), "segments" (pieces of the references, merged afterwards),
        "queries_per_workgroup", "lists_global" (0: candidate lists in LDS, 1: in global scratch)}."""
        out = np.zeros(4, dtype=np.int64)
        check(self._L.sgl_knn_info(self._h, ptr(out, i64p)))
        return dict(zip(("instance", "segments", "queries_per_workgroup", "lists_global"), (int(v) for v in out)))

    def knn_ivf_info(self):
        """What the last inverted-list search on this context ran (sgl_knn_ivf_info): {"n_lists", "n_probe", "train_cells" (0
        after op_ivf_search), "shortest_list", "longest_list", "empty_lists", "short_queries" (queries with -1 / +Inf slots),
        "instance" (of the list scan, as knn_info)}."""
        out = np.zeros(8, dtype=np.int64)
        check(self._L.sgl_knn_ivf_info(self._h, ptr(out, i64p)))
        return dict(zip(("n_lists", "n_probe", "train_cells", "shortest_list", "longest_list", "empty_lists", "short_queries", "instance"),
                        (int(v) for v in out)))

    def knn_ivf_stage_ms(self):
        """With timing on, the milliseconds of the stages of the last inverted-list call (sgl_knn_ivf_stage_ms)."""
        out = np.zeros(8)
        check(self._L.sgl_knn_ivf_stage_ms(self._h, ptr(out, f64p)))
        return dict(zip(("operands", "lloyd", "assign", "bucket", "probes", "tasks", "scan", "merge"), (float(v) for v in out)))

    def op_ivf_train(self, n_lists, reference=None, dims=None, metric="euclidean", n_iter=10):
        """The training of the inverted-list search alone (sgl_op_ivf_train): (centroids n_dims x n_lists, assign int32[n_ref],
        the list of every reference).  reference / dims / metric as knn."""
        code = knn_metric(metric)
        if reference is None:
            _, n_ref, _ = self.dims()
            k, Rb = self.k, None
        else:
            Rb = colmajor(reference, "reference must be a k x n matrix")
            n_ref, k = Rb.shape
        d = None if dims is None else np.ascontiguousarray(np.asarray(dims), dtype=np.int32)
        nd = int(k) if d is None else int(d.size)
        L = int(n_lists)
        cent = np.empty((max(L, 1), max(nd, 1)))
        assign = np.empty(max(int(n_ref), 1), dtype=np.int32)
        check(self._L.sgl_op_ivf_train(self._h, ptr(Rb, f64p), int(k), int(n_ref), ptr(d, i32p), 0 if d is None else nd, code, L, int(n_iter),
                                       ptr(cent, f64p), ptr(assign, i32p)))
        return cent[:L, :nd].T, assign[:int(n_ref)]

    def op_ivf_search(self, centroids, assign, n_probe, n_neighbors=20, reference=None, query=None, dims=None, metric="euclidean",
                      query_batch=0):
        """The inverted-list search under the caller's centroids (n_dims x n_lists) and assignment (one list per reference,
        any value in [0, n_lists)) (sgl_op_ivf_search): (idx, dist) as knn.  query_batch: 0 automatic, positive: that many
        queries per pass -- the result does not depend on it."""
        code = knn_metric(metric)
        cent = colmajor(centroids, "centroids must be an n_dims x n_lists matrix")
        a = np.ascontiguousarray(np.asarray(assign), dtype=np.int32)
        resident = None
        if reference is None:
            _, n, _ = self.dims()
            resident = (self.k, n)

        def extra(n_ref, nd):
            if cent.shape[1] != nd:
                raise ValueError("centroids has %d rows, the search has %d dimensions" % (cent.shape[1], nd))
            if a.ndim != 1 or a.shape[0] != n_ref:
                raise ValueError("assign must hold one list per reference (%d)" % n_ref)
            return (ptr(cent, f64p), int(cent.shape[0]), ptr(a, i32p), int(n_probe), int(query_batch))
        return knn_call(lambda *x: self._L.sgl_op_ivf_search(self._h, *x), reference, query, dims, n_neighbors, resident, code, extra)

    def knn_index_build(self, reference=None, dims=None, metric="euclidean", method="ivf", n_lists=None, n_iter=10):
        """Builds the neighbour index of this context and keeps it on the device (sgl_knn_index_build): the packed references
        of knn() -- for method "ivf" trained and cut into n_lists lists (None: ceil(sqrt(n_ref))) by n_iter Lloyd steps, for
        "exact" as they are.  reference: k x n (R's orientation); None: a snapshot of the H of the current fit.  dims / metric
        as knn; the dims are applied to every later query.  A second build replaces the first and its annotations."""
        code = knn_metric(metric)
        ivf = knn_method(method)
        if reference is None:
            _, n_ref, _ = self.dims()
            k, Rb = self.k, None
        else:
            Rb = colmajor(reference, "reference must be a k x n matrix")
            n_ref, k = Rb.shape
        d, nd = None, 0
        if dims is not None:
            d = np.ascontiguousarray(np.asarray(dims), dtype=np.int32)
            nd = int(d.size)
        L = knn_ivf_shape(n_ref, n_lists, None)[0] if ivf else 0
        check(self._L.sgl_knn_index_build(self._h, ptr(Rb, f64p), int(k), int(n_ref), ptr(d, i32p), nd, code, int(ivf), L, int(n_iter)))
        self._knn_annotations = [0, 0]
        self._knn_layout_dim = 0

    def _knn_index_query(self, query, n_probe):
        """(the k x n_query image of the query, n_query, n_probe as the library takes it) for a call against the index."""
        info = self.knn_index_info()
        Qb = colmajor(query, "query must be a k x n matrix")
        if info["present"] and Qb.shape[1] != info["k"]:
            raise ValueError("query has %d rows, the index was built on %d" % (Qb.shape[1], info["k"]))
        if n_probe is None:
            n_probe = knn_ivf_shape(info["n_ref"], info["n_lists"], None)[1] if info["method"] == 1 else 0
        nq = int(Qb.shape[0])
        if nq == 0:
            Qb = np.zeros((1, Qb.shape[1]))   # (no query: a buffer that is there, so that the pointer is not NULL)
        return Qb, nq, int(n_probe)

    def knn_index_search(self, query, n_neighbors=20, n_probe=None, query_batch=0):
        """The neighbours of the query columns (k x n_query) among the references of the index (sgl_knn_index_search): (idx,
        dist) as knn returns them -- bit for bit what knn(method=...) gives for the same references and queries.  n_probe
        (inverted lists only; None: the default of knn) may differ from search to search; query_batch as op_ivf_search."""
        Qb, nq, n_probe = self._knn_index_query(query, n_probe)
        K = int(n_neighbors)
        shape = (nq, K) if 1 <= K <= 256 else (1, 1)   # outside it the library refuses before it writes
        idx, dist = np.empty(shape, dtype=np.int32), np.empty(shape)
        check(self._L.sgl_knn_index_search(self._h, ptr(Qb, f64p), nq, K, n_probe, int(query_batch), ptr(idx, i32p), ptr(dist, f64p)))
        return idx, dist

    def knn_index_annotate(self, labels=None, n_classes=None, values=None):
        """Puts labels (one class in [-1, n_classes) per reference cell, -1: none; n_classes None: 1 + the largest) and / or
        values (n_values x n_ref, R's orientation: one column per reference cell) onto the index (sgl_knn_index_annotate);
        what is None stays as it is."""
        n_ref = self.knn_index_info()["n_ref"]
        g, G, Vb, nv = None, 0, None, 0
        if labels is not None:
            g, G = label_list(labels, n_ref or None, n_classes)
        if values is not None:
            Vb = colmajor(values, "values must be an n_values x n_ref matrix")
            if n_ref and Vb.shape[0] != n_ref:
                raise ValueError("values has %d columns, the index has %d references" % (Vb.shape[0], n_ref))
            nv = int(Vb.shape[1])
        check(self._L.sgl_knn_index_annotate(self._h, ptr(g, i32p), int(G), ptr(Vb, f64p), nv))
        a = getattr(self, "_knn_annotations", [0, 0])
        self._knn_annotations = [G if g is not None else a[0], nv if Vb is not None else a[1]]

    def knn_index_map(self, query, n_neighbors=20, n_probe=None, weighting="distance"):
        """One search against the index with the transfer of its annotations run on the device (sgl_knn_index_map): {"idx",
        "dist"} as knn_index_search, and for the annotations the index holds {"predicted" (int32 per query, -1: no vote),
        "score" (the winning share), "scores" (n_query x n_classes), "values" (n_query x n_values)}, None for what it does
        not hold.  weighting: "distance" (Dudani's weights: the nearest neighbour votes 1, the farthest 0) or "uniform"."""
        w = knn_weighting(weighting)
        Qb, nq, n_probe = self._knn_index_query(query, n_probe)
        K = int(n_neighbors)
        shape = (nq, K) if 1 <= K <= 256 else (1, 1)
        idx, dist = np.empty(shape, dtype=np.int32), np.empty(shape)
        G, nv = getattr(self, "_knn_annotations", [0, 0])
        out = transfer_call(lambda *o: self._L.sgl_knn_index_map(self._h, ptr(Qb, f64p), nq, K, n_probe, w, ptr(idx, i32p), ptr(dist, f64p), *o),
                            nq, G > 0, G, nv)
        return {"idx": idx, "dist": dist, **out}

    def knn_index_set_layout(self, layout):
        """Puts the layout of the reference cells (dim x n_ref, R's orientation: one column per reference cell; finite, dim in
        [1, 8]) onto the index, resident with it (sgl_knn_index_set_layout).  A second call replaces it; a rebuild and
        knn_index_drop release it."""
        Yb = colmajor(layout, "layout must be a dim x n_ref matrix")
        n_ref = self.knn_index_info()["n_ref"]
        if n_ref and Yb.shape[0] != n_ref:
            raise ValueError("layout has %d columns, the index has %d references" % (Yb.shape[0], n_ref))
        check(self._L.sgl_knn_index_set_layout(self._h, ptr(Yb, f64p), int(Yb.shape[1])))
        self._knn_layout_dim = int(Yb.shape[1])

    def knn_index_project(self, query, a, b, n_neighbors=20, n_probe=None, n_epochs=None, alpha0=0.25, neg_rate=5, seed=42, query_batch=0):
        """One search against the index with the memberships, the start and the layout transform of every batch run on the
        device (sgl_knn_index_project): {"idx", "dist"} as knn_index_search, "layout_init" (the start) and "layout" (after
        n_epochs epochs), each n_query x dim.  Bit for bit knn_index_search followed by umap_transform.  n_epochs None: 100
        up to 10 000 queries, 30 above."""
        Qb, nq, n_probe = self._knn_index_query(query, n_probe)
        K = int(n_neighbors)
        dim = getattr(self, "_knn_layout_dim", 0)
        shape = (nq, K) if 1 <= K <= 256 else (1, 1)   # outside it the library refuses before it writes
        idx, dist = np.empty(shape, dtype=np.int32), np.empty(shape)
        Y0, Y = np.empty((max(nq, 1), max(dim, 1))), np.empty((max(nq, 1), max(dim, 1)))
        if n_epochs is None:
            n_epochs = 100 if nq <= 10000 else 30
        check(self._L.sgl_knn_index_project(self._h, ptr(Qb, f64p), nq, K, n_probe, int(query_batch), float(a), float(b), int(n_epochs),
                                            float(alpha0), int(neg_rate), int(seed) & (2**64 - 1), ptr(idx, i32p), ptr(dist, f64p),
                                            ptr(Y0, f64p), ptr(Y, f64p)))
        return {"idx": idx, "dist": dist, "layout_init": Y0[:nq], "layout": Y[:nq]}

    def knn_index_drop(self):
        """Releases the index and its annotations (sgl_knn_index_drop); nothing happens without one."""
        check(self._L.sgl_knn_index_drop(self._h))
        self._knn_annotations = [0, 0]
        self._knn_layout_dim = 0

    def knn_index_info(self):
        """The index of this context (sgl_knn_index_info): {"present" (0 / 1), "method" (0 exact, 1 ivf), "metric", "k",
        "n_dims", "n_ref", "n_lists", "train_cells", "shortest_list", "longest_list", "empty_lists", "bytes" (resident),
        "searches" (served since the build), "last_queries", "last_short_queries" (of the last search), "instance" (of its
        scan, as knn_info)}."""
        out = np.zeros(16, dtype=np.int64)
        check(self._L.sgl_knn_index_info(self._h, ptr(out, i64p)))
        return dict(zip(KNN_INDEX_FIELDS, (int(v) for v in out)))

    def op_knn_transfer(self, idx, dist, n_ref, labels=None, n_classes=None, values=None, weighting="distance"):
        """The transfer stage alone on the caller's neighbour lists (sgl_op_knn_transfer): idx / dist n_query x n_neighbors as
        the searches return them, labels and values as knn_index_annotate takes them -> the transfer outputs of
        knn_index_map."""
        w = knn_weighting(weighting)
        i, d, nq, K = knn_lists_in(idx, dist)
        g, G, Vb, nv = None, 0, None, 0
        if labels is not None:
            g, G = label_list(labels, None, n_classes)
        if values is not None:
            Vb = colmajor(values, "values must be an n_values x n_ref matrix")
            nv = int(Vb.shape[1])
        for name, a in (("labels", g), ("values", Vb)):
            if a is not None and a.shape[0] != int(n_ref):
                raise ValueError("%s must hold one entry per reference cell (%d)" % (name, int(n_ref)))
        return transfer_call(lambda *o: self._L.sgl_op_knn_transfer(self._h, ptr(i, i32p), ptr(d, f64p), K, nq, int(n_ref), ptr(g, i32p), int(G),
                                                                    ptr(Vb, f64p), nv, w, *o), nq, g is not None, G, nv)

    def knn_metric_info(self):
        """knn_info() of the last search on this context (sgl_knn_metric_info) with "metric" (0 euclidean, 1 cosine,
        2 correlation) and "no_direction": the columns among its operands whose unit column is all zeros (a zero or a
        constant column, a norm that overflows or underflows); 0 for euclidean."""
        out = np.zeros(6, dtype=np.int64)
        check(self._L.sgl_knn_metric_info(self._h, ptr(out, i64p)))
        return dict(zip(("instance", "segments", "queries_per_workgroup", "lists_global", "metric", "no_direction"), (int(v) for v in out)))

    def set_stream(self, stream_ptr):
        """Launch all work of this context on the HIP stream with this handle (sgl_set_stream; e.g. the cuda_stream of a
        torch.cuda.Stream); host reads wait for it, and an all-reduce hook enqueues on it without a host sync.  Handle 0 /
        None = the context's private stream -- torch's default stream, whose handle is 0, cannot be chosen --, and a hook
        on the private stream must have finished its writes when it returns."""
        check(self._L.sgl_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def set_allreduce(self, fn):
        """fn(dev_ptr: int, count: int) -> None; sums `count` doubles at dev_ptr over all shards."""
        if fn is None:
            cfn = C.cast(None, _lib.ALLREDUCE_FN)
        else:
            def tramp(user, dev_ptr, count):
                try:
                    fn(int(dev_ptr), int(count))
                    return 0
                except Exception:  # noqa: BLE001 - must not unwind through C
                    import traceback
                    traceback.print_exc()
                    return 1
            cfn = _lib.ALLREDUCE_FN(tramp)
        self._keep = [cfn]
        check(self._L.sgl_set_allreduce(self._h, cfn, None))

    def step_begin(self):
        check(self._L.sgl_step_begin(self._h))

    def step_h(self, L1, L2):
        check(self._L.sgl_step_h(self._h, L1, L2))

    def step_scale_h(self):
        check(self._L.sgl_step_scale_h(self._h))

    def step_w(self, L1, L2):
        check(self._L.sgl_step_w(self._h, L1, L2))

    def step_h_masked(self, L1, L2, seed, inv_density):
        """predict_mask(A, ...) on the resident fit: the masked H-update (unscaled h)."""
        check(self._L.sgl_step_h_masked(self._h, L1, L2, int(seed), int(inv_density)))

    def step_w_masked(self, L1, L2, seed, inv_density):
        """predict_mask(At, ..., mask_t = true) on the resident fit: the masked W-update (unscaled w)."""
        check(self._L.sgl_step_w_masked(self._h, L1, L2, int(seed), int(inv_density)))

    def step_scale_w(self):
        t = C.c_double()
        check(self._L.sgl_step_scale_w(self._h, C.byref(t)))
        return t.value

    def project_run(self, L1, L2):
        check(self._L.sgl_project_run(self._h, L1, L2))

    def get_factors(self, w=True, d=True, h=True):
        nr, nc, _ = self.dims()
        k = self.k
        W = np.empty((nr, k)) if w else None
        D = np.empty(k) if d else None
        H = np.empty((nc, k)) if h else None
        check(self._L.sgl_get_factors(self._h, ptr(W, f64p), ptr(D, f64p), ptr(H, f64p)))
        return W, D, H

    def set_factors(self, w=None, d=None, h=None):
        w = None if w is None else _f(w)
        d = None if d is None else _f(d)
        h = None if h is None else _f(h)
        check(self._L.sgl_set_factors(self._h, ptr(w, f64p), ptr(d, f64p), ptr(h, f64p)))

    # -- single operators ---------------------------------------------------
    def op_rand(self, state, i, j):
        i = np.ascontiguousarray(i, dtype=np.uint64)
        j = np.ascontiguousarray(j, dtype=np.uint64)
        out = np.empty(i.shape, dtype=np.uint64)
        check(self._L.sgl_op_rand(self._h, int(state), ptr(i, u64p), ptr(j, u64p), i.size, ptr(out, u64p)))
        return out

    def op_mask(self, state, inv_density, cell0, ncells, ngenes):
        out = np.empty((ncells, ngenes), dtype=np.uint8)
        check(self._L.sgl_op_mask(self._h, int(state), int(inv_density), int(cell0), ncells, ngenes, ptr(out, u8p)))
        return out

    def op_gram(self, F):
        F = _f(F)
        cols, k = F.shape
        G = np.empty((k, k))
        check(self._L.sgl_op_gram(self._h, ptr(F, f64p), k, cols, ptr(G, f64p)))
        return G

    def _rhs_buffers(self, which, F):
        """(F, k, B) of op_rhs / op_rhs_masked: which & 1 selects t(A); which & 2 the LDS-tiled kernel."""
        F = _f(F)
        nr, nc, _ = self.dims()
        ncol, nrow = (nr, nc) if (which & 1) else (nc, nr)
        if F.shape[0] != nrow:
            raise ValueError("F must have %d rows" % nrow)
        return F, F.shape[1], np.empty((ncol, F.shape[1]))

    def op_rhs(self, which, F):
        F, k, B = self._rhs_buffers(which, F)
        check(self._L.sgl_op_rhs(self._h, int(which), ptr(F, f64p), k, ptr(B, f64p)))
        return B

    def op_nnls(self, G, B, X, L1=0.0, L2=0.0):
        G, B = _f(G), _f(B)
        X = np.array(X, dtype=np.float64, order="C")
        ncols, k = B.shape
        sw = C.c_int32()
        check(self._L.sgl_op_nnls(self._h, ptr(G, f64p), ptr(B, f64p), ptr(X, f64p), k, ncols, L1, L2, C.byref(sw)))
        return X, sw.value

    def op_mask_gram(self, F, G, ncols, seed, inv_density, mask_t=0, col_offset=0, row_offset=0, use_lists=False):
        """Per-column Gram downdates of predict_mask for columns 0 .. ncols-1: F is nrow x k, G k x k or None (raw sums)."""
        F = _f(F)
        nrow, k = F.shape
        out = np.empty((ncols, k, k))
        Gp = ptr(_f(G), f64p) if G is not None else None
        check(self._L.sgl_op_mask_gram(self._h, ptr(F, f64p), Gp, k, nrow, ncols, int(seed), int(inv_density), int(mask_t),
                                       int(col_offset), int(row_offset), 1 if use_lists else 0, ptr(out, f64p)))
        return out

    def op_transpose(self, max_batch_entries=0):
        """Rebuild the resident t(A) from A on the device, at most max_batch_entries non-zeros per sort (0: the
        default).  Drops a running fit."""
        check(self._L.sgl_op_transpose(self._h, int(max_batch_entries)))
        self.k = 0

    def op_scale(self, F):
        F = np.array(F, dtype=np.float64, order="C")
        cols, k = F.shape
        d = np.empty(k)
        check(self._L.sgl_op_scale(self._h, ptr(F, f64p), k, cols, ptr(d, f64p)))
        return F, d

    def op_cor(self, x, y):
        x, y = _f(x), _f(y)
        out = C.c_double()
        check(self._L.sgl_op_cor(self._h, ptr(x, f64p), ptr(y, f64p), x.size, C.byref(out)))
        return out.value

    def op_graph_conv(self, X, out=None):
        """Y = X G over the graph of the current fit (set_graph): X (n, k) C-contiguous (== k x n column-major), k the fit's
        rank.  out: an (n, k) float64 C-contiguous array to write into (a fresh one otherwise)."""
        X = _f(X)
        n, k = X.shape
        _, nc, _ = self.dims()
        if n != nc:
            raise ValueError("X must have %d rows (the cells of the resident matrix)" % nc)
        Y = np.empty((n, k)) if out is None else out
        if Y.shape != (n, k) or Y.dtype != np.float64 or not Y.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous float64 array of X's shape")
        check(self._L.sgl_op_graph_conv(self._h, ptr(X, f64p), k, ptr(Y, f64p)))
        return Y

    def op_mse_test(self, seed, inv_density):
        out = C.c_double()
        check(self._L.sgl_op_mse_test(self._h, int(seed), int(inv_density), C.byref(out)))
        return out.value

    # the stages of variable_features, one at a time (mu, sd: one value per gene)
    def _gene_vec(self, v, what):
        a = np.ascontiguousarray(v, dtype=np.float64)
        if a.shape != (self.dims()[0],):
            raise ValueError("%s needs one entry per gene (row) of A" % what)
        return a

    def op_gene_mean(self):
        """(mean, count) per gene of the resident matrix (sgl_op_gene_mean): sum of the stored values / ncol, stored entries."""
        nr = self.dims()[0]
        mean, count = np.empty(max(nr, 1)), np.zeros(max(nr, 1), dtype=np.int64)
        check(self._L.sgl_op_gene_mean(self._h, ptr(mean, f64p), ptr(count, i64p)))
        return mean[:nr], count[:nr]

    def op_gene_var(self, mu):
        mu = self._gene_vec(mu, "mu")
        out = np.empty(max(mu.shape[0], 1))
        check(self._L.sgl_op_gene_var(self._h, ptr(mu, f64p), ptr(out, f64p)))
        return out[:mu.shape[0]]

    def op_gene_var_std(self, mu, sd, vmax):
        mu, sd = self._gene_vec(mu, "mu"), self._gene_vec(sd, "sd")
        out = np.empty(max(mu.shape[0], 1))
        check(self._L.sgl_op_gene_var_std(self._h, ptr(mu, f64p), ptr(sd, f64p), float(vmax), ptr(out, f64p)))
        return out[:mu.shape[0]]

    def op_loess_direct(self, x, y, q):
        """The trend of variable_features (sgl_op_loess_direct): the local fit of y on the ascending x at every x[i], windows of q."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if x.ndim != 1 or x.shape != y.shape:
            raise ValueError("x and y must be vectors of one length")
        out = np.empty(max(x.shape[0], 1))
        check(self._L.sgl_op_loess_direct(self._h, ptr(x, f64p), ptr(y, f64p), x.shape[0], int(q), ptr(out, f64p)))
        return out[:x.shape[0]]

    # the stages of markers, one at a time
    def op_marker_sums(self, labels, n_groups=None, transform="expm1"):
        """(pos, nz, sum), each m x G, of the resident matrix under the labels (sgl_op_marker_sums)."""
        nr, nc, _ = self.dims()
        g, G = label_list(labels, nc or None, n_groups)   # (no matrix: the library refuses)
        if transform not in MARKER_TRANSFORMS:
            raise ValueError("transform must be 'expm1' or 'identity'")
        shape = (max(min(G, 1024), 1), max(nr, 1))
        pos, nz, s = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64), np.empty(shape)
        check(self._L.sgl_op_marker_sums(self._h, ptr(g, i32p), G, MARKER_TRANSFORMS[transform], ptr(pos, i64p), ptr(nz, i64p), ptr(s, f64p)))
        return pos[:, :nr].T, nz[:, :nr].T, s[:, :nr].T

    def op_marker_ranks(self, labels, n_groups=None, max_batch_entries=0):
        """(rank2 m x G, tie m) of the resident matrix under the labels (sgl_op_marker_ranks); max_batch_entries 0: the default."""
        nr, nc, _ = self.dims()
        g, G = label_list(labels, nc or None, n_groups)   # (no matrix: the library refuses)
        rank2 = np.zeros((max(min(G, 1024), 1), max(nr, 1)), dtype=np.int64)
        tie = np.zeros(max(nr, 1), dtype=np.uint64)
        check(self._L.sgl_op_marker_ranks(self._h, ptr(g, i32p), G, int(max_batch_entries), ptr(rank2, i64p), ptr(tie, u64p)))
        return rank2[:, :nr].T, tie[:nr]

    # the stages of signature_scores, with the knobs that force every path (0: the default)
    def op_cell_ranks(self, max_rank=1500, lds_cap=0, max_batch_entries=0):
        """(rank2_entry, zero2): the doubled capped midrank of every stored entry of the resident matrix within its cell, in
        storage order, and of every cell's zero block (0: the cell has none) (sgl_op_cell_ranks)."""
        _, nc, nnz = self.dims()
        entry, zero2 = np.zeros(max(nnz, 1), dtype=np.uint64), np.zeros(max(nc, 1), dtype=np.uint64)
        check(self._L.sgl_op_cell_ranks(self._h, int(max_rank), int(lds_cap), int(max_batch_entries), ptr(entry, u64p), ptr(zero2, u64p)))
        return entry[:nnz], zero2[:nc]

    def op_signature_scores(self, sets, max_rank=1500, lds_cap=0, max_batch_entries=0, pass_sets=0):
        """(rank2, score), each n_sets x ncol, as signature_scores gives them, with the LDS cap, the batch size of the long
        path and the sets of a pass forced (sgl_op_signature_scores); the results do not depend on them."""
        _, nc, _ = self.dims()
        return signature_call(lambda sp, sg, P, R, r2, sc: self._L.sgl_op_signature_scores(
            self._h, sp, sg, P, R, int(lds_cap), int(max_batch_entries), int(pass_sets), r2, sc), nc, sets, max_rank, True)

    # the merge of simulate_doublets alone, with the knob that forces either path (0: the default)
    def op_pair_columns(self, parent_a, parent_b, lds_cap=0):
        """(x, i, p) of S, S[:, s] = A[:, parent_a[s]] + A[:, parent_b[s]] over the resident matrix, as CSC slots with 64-bit
        offsets (sgl_op_pair_columns, called twice: the offsets, then the entries).  A pair whose row indices together fit
        lds_cap is merged in LDS, a longer one in global memory; the result does not depend on it."""
        a, b, n = self._parent_lists(parent_a, parent_b, "op_pair_columns")
        p = np.zeros(n + 1, dtype=np.int64)
        check(self._L.sgl_op_pair_columns(self._h, ptr(a, i32p), ptr(b, i32p), n, int(lds_cap), ptr(p, i64p), None, None))
        nnz = int(p[n])
        x, i = np.empty(max(nnz, 1)), np.empty(max(nnz, 1), dtype=np.int32)
        check(self._L.sgl_op_pair_columns(self._h, ptr(a, i32p), ptr(b, i32p), n, int(lds_cap), ptr(p, i64p), ptr(i, i32p), ptr(x, f64p)))
        return x[:nnz], i[:nnz], p

    # the stages of the gene set enrichment test, one at a time (no resident matrix is needed)
    def op_gsea_es(self, w, set_ptr, set_genes):
        """(es_pos, es_neg, es_std), each n_sets x k: the observed enrichment scores of the gene sets in every column of w (m genes
        x k factors) under the three score types (sgl_op_gsea_es; the rules: include/singlet_hip.h, "Gene set enrichment")."""
        wt, m, k, sp, sg = gsea_inputs(w, set_ptr, set_genes)
        P = sp.shape[0] - 1
        out = [np.empty((max(k, 1), max(P, 1))) for _ in range(3)]
        check(self._L.sgl_op_gsea_es(self._h, ptr(wt, f64p), m, k, ptr(sp, i64p), ptr(sg, i32p), P, *(ptr(o, f64p) for o in out)))
        return tuple(o[:k, :P].T for o in out)

    def op_gsea_null(self, w, sizes, score_type="pos", seed=0, r0=0, r1=1, batch=0, return_sample=False):
        """null (k x n_sizes x (r1 - r0)): the scores of the null sets of the given sizes (strictly ascending) for the permutations
        [r0, r1) in batches of `batch` permutations (0: by the memory budget); with return_sample also the (r1 - r0) x s_max
        genes of every permutation in their order by (key, gene) (sgl_op_gsea_null)."""
        wt, m, k, _, _ = gsea_inputs(w, [0], [])
        sz = np.ascontiguousarray(np.asarray(sizes).ravel(), dtype=np.int32)
        st, n = gsea_score_type(score_type), max(int(r1) - int(r0), 1)
        s_max = int(min(max(int(sz.max()) if sz.size else 1, 1), 4096))   # (outside the range the library refuses before it writes)
        null = np.empty((max(k, 1), max(sz.size, 1), n))
        sample = np.zeros((n, s_max), dtype=np.int32) if return_sample else None
        check(self._L.sgl_op_gsea_null(self._h, ptr(wt, f64p), m, k, ptr(sz, i32p), sz.size, st, int(seed), int(r0), int(r1), int(batch),
                                       ptr(null, f64p), ptr(sample, i32p)))
        null = null[:k, :sz.size]
        return (null, sample) if return_sample else null

    def gsea_info(self):
        """What the last enrichment call on this context ran (sgl_gsea_info): {"sets", "sizes", "s_max", "batches", "batch"}."""
        out = np.zeros(5, dtype=np.int64)
        check(self._L.sgl_gsea_info(self._h, ptr(out, i64p)))
        return dict(zip(("sets", "sizes", "s_max", "batches", "batch"), (int(v) for v in out)))

    def op_rhs_masked(self, which, F, seed, inv_density):
        """op_rhs with the entries the mask (seed, inv_density) draws left out (sgl_op_rhs_masked): which = 0 / 1 hash every
        entry in the plain kernel, 2 / 3 run the LDS-tiled kernel on a masked value array."""
        F, k, B = self._rhs_buffers(which, F)
        check(self._L.sgl_op_rhs_masked(self._h, int(which), ptr(F, f64p), k, int(seed), int(inv_density), ptr(B, f64p)))
        return B

    def op_nnls_percol(self, Gcols, B, X, col_nnz=None, L1=0.0, L2=0.0):
        """nnls of every column against its own Gram (sgl_op_nnls_percol): Gcols (ncols, k, k), B / X (ncols, k); col_nnz:
        int64 per column, a zero skips the column.  Returns (X, total sweeps)."""
        Gcols, B = _f(Gcols), _f(B)
        X = np.array(X, dtype=np.float64, order="C")
        ncols, k = B.shape
        if Gcols.shape != (ncols, k, k) or X.shape != (ncols, k):
            raise ValueError("Gcols must be (ncols, k, k) and X (ncols, k)")
        nz = None if col_nnz is None else np.ascontiguousarray(col_nnz, dtype=np.int64)
        if nz is not None and nz.shape != (ncols,):
            raise ValueError("col_nnz must have one entry per column")
        sw = C.c_int32()
        check(self._L.sgl_op_nnls_percol(self._h, ptr(Gcols, f64p), ptr(B, f64p), ptr(X, f64p), ptr(nz, i64p), k, ncols, L1, L2,
                                         C.byref(sw)))
        return X, sw.value

    def op_mse_test_cells(self, seed, inv_density, variant=0):
        """The per-cell losses of mse_test (sgl_op_mse_test_cells) by one kernel family: variant 0 hashing, 1 mask lists with
        the sliding window, 2 mask lists with listed matrix values."""
        _, nc, _ = self.dims()
        out = np.empty(nc)
        check(self._L.sgl_op_mse_test_cells(self._h, int(seed), int(inv_density), int(variant), ptr(out, f64p)))
        return out

    # -- timing -------------------------------------------------------------
    def timing_enable(self, on=True):
        check(self._L.sgl_timing_enable(self._h, int(bool(on))))

    def timing_get(self, reset=False):
        ms = np.zeros(_lib.SGL_PH_COUNT)
        calls = np.zeros(_lib.SGL_PH_COUNT, dtype=np.int64)
        check(self._L.sgl_timing_get(self._h, ptr(ms, f64p), ptr(calls, i64p), int(reset)))
        return {n: (float(ms[q]), int(calls[q])) for q, n in enumerate(_lib.SGL_PH_NAMES)}

    def sweeps_get(self, reset=False):
        out = np.zeros(4, dtype=np.int64)
        check(self._L.sgl_sweeps_get(self._h, ptr(out, i64p), int(reset)))
        return dict(h_sweeps=int(out[0]), w_sweeps=int(out[1]), h_wave_sweeps=int(out[2]), w_wave_sweeps=int(out[3]))

    def layout_get(self):
        """Entry-stream layout of the current fit: {'A': {...}, 'At': {...}} (all zero on the plain CSC path)."""
        out = np.zeros(10, dtype=np.int64)
        check(self._L.sgl_layout_get(self._h, ptr(out, i64p)))
        keys = ("entries", "tiles", "tile_rows", "tile_ranges", "col_blocks")
        return {name: dict(zip(keys, (int(v) for v in out[5 * o:5 * o + 5]))) for o, name in enumerate(("A", "At"))}

    def mask_pairs(self):
        """(pairs listed per cell, per gene) of the mask the current fit runs under (sgl_mask_pairs; 0 where no lists are built)."""
        out = np.zeros(2, dtype=np.int64)
        check(self._L.sgl_mask_pairs(self._h, ptr(out, i64p)))
        return int(out[0]), int(out[1])

    def layout_builds(self):
        """(stream of A, of At, mask lists of the cell side, of the gene side): times each has been written on this context
        (a re-init at an unchanged rank adds no stream, a masked fit under a recently used seed no lists)."""
        out = np.zeros(4, dtype=np.int64)
        check(self._L.sgl_layout_builds(self._h, ptr(out, i64p)))
        return tuple(int(v) for v in out)


class Multi(_Handle):
    """sgl_multi: ONE process driving several devices, cells sharded, exchange over RCCL inside the
    library (include/singlet_hip.h section 2b).  devices: list of device ids -- all distinct (RCCL) or
    all equal (ranks share one device and exchange through a HIP kernel: the test configuration)."""
    _PREFIX = "sgl_multi_"

    def __init__(self, devices):
        self._L = _lib.load()
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        check(self._L.sgl_multi_create(int(dev.size), ptr(dev, i32p), C.byref(h)))
        self._h = h
        self.n = int(dev.size)
        self.k = 0
        self._dims = None

    def _shape(self):
        return self._dims

    def rank_ctx(self, r):
        h = C.c_void_p()
        check(self._L.sgl_multi_ctx(self._h, int(r), C.byref(h)))
        c = Context(_borrowed=h)
        c.k = self.k
        return c

    def upload(self, A):
        check(self._L.sgl_multi_upload_csc(self._h, *csc_ptrs(A), A.nrow, A.ncol))
        self._dims = (A.nrow, A.ncol)
        self.k = 0

    def synth(self, ngenes, ncells_total, inv_density=20, seed=SYNTH_SEED):
        lv = _f(LEVELS16)
        check(self._L.sgl_multi_synth_csc(self._h, seed, inv_density, ptr(lv, f64p), int(ngenes), int(ncells_total)))
        self._dims = (int(ngenes), int(ncells_total))
        self.k = 0

    def fit_init(self, k, w_init=None, synth_seed=SYNTH_SEED):
        w = None
        if w_init is not None:
            w = _f(w_init)
            if w.shape != (self._dims[0], k):
                raise ValueError("w_init must be k x nrow(A)")
        check(self._L.sgl_multi_fit_init(self._h, int(k), ptr(w, f64p), synth_seed))
        self.k = int(k)

    def group_means(self, group, n_groups):
        """(means k x n_groups, counts) of the H of the team's fit per group of cells (sgl_multi_group_means): every rank sums
        its cells, the rank partials are added in rank order and divided by the counts over all ranks."""
        g = _group_list(group, self._dims[1], "group")
        return _group_means_call(lambda *o: self._L.sgl_multi_group_means(self._h, *o), g, n_groups, self.k)

    def graph_info(self):
        """dict(edges, crossing, E, exported, halo_bytes) of the graph set by set_graph (all 0 without one): entries of G,
        entries whose row lives on another rank than their column, the longest export list, the sum of the export list
        lengths, and the bytes one rank contributes to one halo all-gather (8 k E)."""
        out = np.zeros(5, dtype=np.int64)
        check(self._L.sgl_multi_graph_info(self._h, ptr(out, i64p)))
        return dict(zip(("edges", "crossing", "E", "exported", "halo_bytes"), (int(v) for v in out)))

    def iterate(self, L1_w, L1_h, L2_w, L2_h):
        t = C.c_double()
        check(self._L.sgl_multi_iterate(self._h, L1_w, L1_h, L2_w, L2_h, C.byref(t)))
        return t.value

    def get_factors(self):
        nr, nc = self._dims
        W, D, H = np.empty((nr, self.k)), np.empty(self.k), np.empty((nc, self.k))
        check(self._L.sgl_multi_get_factors(self._h, ptr(W, f64p), ptr(D, f64p), ptr(H, f64p)))
        return W, D, H
