"""Test-side numpy restatement of rowwise_compress_sparse / rowwise_compress_dense (src/singlet.cpp:146-180), the natives of
RasterizeRowwise (R/rasterize_rowwise.R).  Two forms:

  * literal(): the reference's loops transcribed entry by entry.  Defined only where the reference is (nrow % n == 0,
    n >= 1): elsewhere it would write res(n_rows, col), an alias of the next column's first bin.
  * vectorised(): this build's rule for every n >= 1 -- entry (b, j) = (A[b n, j] + A[b n + 1, j] + ... in order, from
    +0.0) / n over the first floor(nrow / n) n rows -- as one running sum per bin, all bins at once.  np.add.reduce and
    reduceat sum pairwise, in another order, and are not used.

Inputs are dgCMatrix-like objects (x, i, p, nrow, ncol) or dense 2-D arrays."""
import numpy as np

np_quiet = np.errstate(over="ignore", invalid="ignore")   # overflow to Inf and Inf - Inf are part of the rule


def _slots(A):
    return np.asarray(A.x, dtype=np.float64), np.asarray(A.i, dtype=np.int64), np.asarray(A.p, dtype=np.int64)


def _dims(A):
    return (A.nrow, A.ncol) if hasattr(A, "nrow") else (A.Dim[0], A.Dim[1])


@np_quiet
def literal_sparse(A, n):
    """rowwise_compress_sparse, l.147-161: res(row / n, col) += value for every stored entry, then res /= n."""
    nrow, ncol = _dims(A)
    assert n >= 1 and nrow % n == 0, "the reference is undefined here"
    x, i, p = _slots(A)
    n_rows = nrow // n
    res = np.zeros((n_rows, ncol), order="F")
    for col in range(ncol):
        for e in range(p[col], p[col + 1]):
            res[i[e] // n, col] += x[e]
    for j in range(ncol):
        for r in range(n_rows):
            res[r, j] /= n
    return res


@np_quiet
def literal_dense(A, n):
    """rowwise_compress_dense, l.165-179: for every column, res_row += A(row + i, col) for i < n, then /= n."""
    A = np.asarray(A, dtype=np.float64)
    nrow, ncol = A.shape
    assert n >= 1 and nrow % n == 0, "the reference is undefined here"
    res = np.zeros((nrow // n, ncol), order="F")
    for col in range(ncol):
        res_row = 0
        for row in range(0, nrow, n):
            for t in range(n):
                res[res_row, col] += A[row + t, col]
            res[res_row, col] /= n
            res_row += 1
    return res


@np_quiet
def vectorised_dense(A, n):
    """This build's rule on a dense matrix, for any n >= 1 (the last nrow mod n rows left out)."""
    A = np.asarray(A, dtype=np.float64)
    nrow, ncol = A.shape
    nb = nrow // n
    acc = np.zeros((nb, ncol))
    for t in range(n):   # acc += A[b n + t, :] for every bin b at once: one sequential sum per bin
        acc += A[t:nb * n:n, :]
    return np.asfortranarray(acc / float(n))


def densify(A):
    """The dense matrix of a dgCMatrix-like (unstored entries +0.0)."""
    nrow, ncol = _dims(A)
    x, i, p = _slots(A)
    D = np.zeros((nrow, ncol), order="F")
    col = np.repeat(np.arange(ncol), np.diff(p))
    D[i, col] = x
    return D


def vectorised_sparse(A, n):
    """This build's rule on a dgCMatrix-like: the dense form over its densified matrix (stored zeros and skipped zeros
    are the same +0.0 additions; see kernels_raster.hip for why they change no sum)."""
    return vectorised_dense(densify(A), n)


def columns(A, n, cols):
    """vectorised_sparse restricted to the listed columns of A: a floor(nrow / n) x len(cols) array."""
    nrow, _ = _dims(A)
    x, i, p = _slots(A)
    out = np.zeros((nrow // n, len(cols)), order="F")
    for q, c in enumerate(cols):
        d = np.zeros((nrow, 1))
        d[i[p[c]:p[c + 1]], 0] = x[p[c]:p[c + 1]]
        out[:, q] = vectorised_dense(d, n)[:, 0]
    return out


def same_bits(a, b):
    """Equal bit for bit, except that every NaN equals every NaN (the payload of a NaN made by an operation differs
    between the CPU and the GPU)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return bool(np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
