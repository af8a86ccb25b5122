"""native(): a SciPy / AnnData / torch CSR or CSC handed to the library as it is (sgl_upload_typed, include/singlet_hip.h).

No array is copied or converted here: the three arrays are checked (one-dimensional, contiguous, a dtype the library
converts on the device) and referenced.  Widening to double, narrowing the indices to int32, sorting the indices of a
slice and building the other orientation all happen on the GPU (Context.upload_native).  SciPy is never imported -- a
SciPy object is recognised by its `.format`, `.data`, `.indices`, `.indptr` -- and torch only when a torch object is passed.

  (format, cells_by_genes) -> major_is_genes      CSR cells x genes -> 0      CSC genes x cells -> 0
                                                  CSR genes x cells -> 1      CSC cells x genes -> 1
"""
import numpy as np

SGL_T_F64, SGL_T_F32, SGL_T_I32, SGL_T_I64 = 0, 1, 2, 3
SGL_SPACE_HOST, SGL_SPACE_DEVICE = 0, 1
SGL_UP_SORT = 1

_VALUE_TYPES = {"float64": SGL_T_F64, "float32": SGL_T_F32, "int32": SGL_T_I32, "int64": SGL_T_I64}
_INDEX_TYPES = {"int32": SGL_T_I32, "int64": SGL_T_I64}
REPORT_KEYS = ("nnz", "sorted_lds", "sorted_long", "integral", "bytes_copied", "lds_capacity")


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def major_is_genes(fmt, cells_by_genes):
    """The layout table of the module docstring; fmt is "csr" or "csc"."""
    if fmt not in ("csr", "csc"):
        raise ValueError("native: the format must be 'csr' or 'csc' (got %r); COO input is not taken" % (fmt,))
    return int((fmt == "csr") != bool(cells_by_genes))


class _Array:
    """One of the three arrays: the object (kept alive), its dtype name, length, address, and where it lives."""
    __slots__ = ("obj", "dtype", "n", "device")

    def __init__(self, a, what, types):
        if _is_torch(a):
            if a.dim() != 1:
                raise ValueError("native: %s must be one-dimensional" % what)
            if not a.is_contiguous():
                raise ValueError("native: %s is not contiguous (it is not copied here: pass a contiguous tensor)" % what)
            self.dtype = str(a.dtype).replace("torch.", "")
            self.n = int(a.numel())
            self.device = None if a.device.type == "cpu" else (a.device.index if a.device.index is not None else 0)
        elif isinstance(a, np.ndarray):
            if a.ndim != 1:
                raise ValueError("native: %s must be one-dimensional" % what)
            if not (a.flags.c_contiguous and a.flags.aligned and a.dtype.isnative):
                raise ValueError("native: %s is not a contiguous, aligned array in native byte order (it is not copied here)" % what)
            self.dtype = a.dtype.name
            self.n = int(a.shape[0])
            self.device = None
        else:
            raise TypeError("native: %s must be a NumPy array or a torch tensor (got %s)" % (what, type(a).__name__))
        if self.dtype not in types:
            raise TypeError("native: %s has dtype %s; the library takes %s (nothing is cast here)" % (what, self.dtype, " / ".join(types)))
        self.obj = a

    def address(self):
        return int(self.obj.data_ptr()) if _is_torch(self.obj) else int(self.obj.ctypes.data)

    def last(self):
        return int(self.obj[-1])


class NativeMatrix:
    """What native() returns: references to the caller's arrays plus the layout.  nrow / ncol are genes / cells of A."""

    def __init__(self, data, indices, indptr, shape, fmt, cells_by_genes=False, Dimnames=(None, None)):
        self.major_is_genes = major_is_genes(fmt, cells_by_genes)
        rows, cols = (int(shape[0]), int(shape[1]))
        self.n_major, self.n_minor = (rows, cols) if fmt == "csr" else (cols, rows)
        self.nrow, self.ncol = (cols, rows) if cells_by_genes else (rows, cols)
        self.format, self.cells_by_genes = fmt, bool(cells_by_genes)
        self._x = _Array(data, "data", _VALUE_TYPES)
        self._i = _Array(indices, "indices", _INDEX_TYPES)
        self._p = _Array(indptr, "indptr", _INDEX_TYPES)
        if self._p.n != self.n_major + 1:
            raise ValueError("native: indptr holds %d offsets, a %s of shape %r has %d" % (self._p.n, fmt, (rows, cols), self.n_major + 1))
        if self._x.n != self._i.n:
            raise ValueError("native: data holds %d entries, indices %d" % (self._x.n, self._i.n))
        kinds = {(_is_torch(a.obj), a.device) for a in (self._x, self._i, self._p)}
        if len(kinds) != 1:
            raise ValueError("native: data, indices and indptr must live in the same place (all NumPy, or torch tensors of one device)")
        self.device = self._x.device                     # None: host memory (a CPU tensor travels as HOST)
        self.space = SGL_SPACE_HOST if self.device is None else SGL_SPACE_DEVICE
        self.Dimnames = tuple(Dimnames)

    data = property(lambda self: self._x.obj)
    indices = property(lambda self: self._i.obj)
    indptr = property(lambda self: self._p.obj)
    nnz = property(lambda self: self._x.n)
    x_type = property(lambda self: _VALUE_TYPES[self._x.dtype])
    idx_type = property(lambda self: _INDEX_TYPES[self._i.dtype])
    ptr_type = property(lambda self: _INDEX_TYPES[self._p.dtype])

    def addresses(self):
        return self._x.address(), self._i.address(), self._p.address()

    def check_entry_count(self):
        """indptr[n_major] against the arrays' length (one element read back for a device tensor): the library takes the
        entry count from the offsets and cannot see how long the arrays are."""
        last = self._p.last()
        if last != self._x.n:
            raise ValueError("native: indptr[%d] = %d, but data and indices hold %d entries" % (self.n_major, last, self._x.n))


def native(A, cells_by_genes=False, Dimnames=(None, None)):
    """A as the library's typed door takes it, nothing copied.  A: a SciPy csr / csc matrix or array (float64 / float32 /
    int32 / int64 values), a torch sparse_csr / sparse_csc tensor on the CPU or a GPU, or a tuple (data, indices, indptr,
    shape, "csr" | "csc") of NumPy arrays or torch tensors.  cells_by_genes = True: the object is laid out as AnnData's X
    (cells x genes); otherwise genes x cells, as everywhere in this package.  Dimnames: (gene names, cell names)."""
    if isinstance(A, NativeMatrix):
        return A
    if isinstance(A, tuple) and len(A) == 5:
        data, indices, indptr, shape, fmt = A
    elif _is_torch(A):
        import torch
        if A.layout == torch.sparse_csr:
            data, indices, indptr, fmt = A.values(), A.col_indices(), A.crow_indices(), "csr"
        elif A.layout == torch.sparse_csc:
            data, indices, indptr, fmt = A.values(), A.row_indices(), A.ccol_indices(), "csc"
        else:
            raise TypeError("native: a torch tensor must have the sparse_csr or sparse_csc layout (got %s)" % (A.layout,))
        if A.dim() != 2:
            raise ValueError("native: a torch sparse tensor must be two-dimensional")
        shape = tuple(A.shape)
    elif all(hasattr(A, s) for s in ("format", "data", "indices", "indptr", "shape")):
        data, indices, indptr, shape, fmt = A.data, A.indices, A.indptr, A.shape, A.format
    else:
        raise TypeError("native: expected a SciPy csr / csc object, a torch sparse_csr / sparse_csc tensor or a "
                        "(data, indices, indptr, shape, format) tuple")
    return NativeMatrix(data, indices, indptr, shape, fmt, cells_by_genes, Dimnames)
