"""Model error by its definition (include/singlet_hip.h, sgl_evaluate), restated in numpy for the tests: per cell and per
gene the sum of the squared residuals of w diag(d) h over EVERY entry of the dense matrix, zeros included.

Orientation: D is the dense m x n matrix (genes x cells), w is m x k, d has k entries, h is k x n -- what the drivers return.

  losses_int64      integer inputs, int64 arithmetic: exact, the reference of the bit-exact device tests
  losses_longdouble np.longdouble arithmetic, plus per column (row) the sum of the absolute values of the terms of the
                    sparse identity  ||a_j||^2 + 2 |h_j| . |b_j| + |h_j|^T |Gw| |h_j|  =  sum_i (|A_ij| + sum_f |w_if d_f h_fj|)^2,
                    the quantity every first-order rounding bound of the device result is relative to
"""
import numpy as np

U = 2.0 ** -53


def dense_of(A):
    """The dense m x n image of a dgCMatrix-like (x, i, p, nrow, ncol)."""
    D = np.zeros((A.nrow, A.ncol))
    for c in range(A.ncol):
        s = slice(A.p[c], A.p[c + 1])
        D[A.i[s], c] = A.x[s]
    return D


def losses_int64(D, w, d, h):
    """(cell_loss n, gene_loss m, sse) as int64 for integer-valued inputs."""
    D, w, d, h = (np.asarray(a) for a in (D, w, d, h))
    for a in (D, w, d, h):
        assert np.array_equal(a, np.rint(a)), "losses_int64 takes integer values"
    Di, wi, di, hi = (a.astype(np.int64) for a in (D, w, d, h))
    R = Di - (wi * di[None, :]) @ hi
    R2 = R * R
    cell, gene = R2.sum(axis=0), R2.sum(axis=1)
    return cell, gene, int(cell.sum())


def losses_longdouble(D, w, d, h):
    """dict(cell, gene, sse, cell_abs, gene_abs) in np.longdouble."""
    L = np.longdouble
    D, w, d, h = (np.asarray(a, dtype=np.float64).astype(L) for a in (D, w, d, h))
    rec = (w * d[None, :]) @ h
    R2 = (D - rec) ** 2
    T2 = (np.abs(D) + (np.abs(w) * np.abs(d)[None, :]) @ np.abs(h)) ** 2   # = the identity's terms, all taken positive
    cell = R2.sum(axis=0)
    return dict(cell=cell, gene=R2.sum(axis=1), sse=cell.sum(), cell_abs=T2.sum(axis=0), gene_abs=T2.sum(axis=1))


def identity_float64(D, w, d, h):
    """The sparse identity in plain float64 (numpy's own summation order): (cell, gene) -- what the device computes, up to order."""
    D, w, d, h = (np.asarray(a, dtype=np.float64) for a in (D, w, d, h))
    Wd = w * d[None, :]            # m x k
    Hd = h * d[:, None]            # k x n
    cell = (D * D).sum(axis=0) - 2.0 * (h * (Wd.T @ D)).sum(axis=0) + (h * ((Wd.T @ Wd) @ h)).sum(axis=0)
    gene = (D * D).sum(axis=1) - 2.0 * (w * (D @ Hd.T)).sum(axis=1) + (w * (w @ (Hd @ Hd.T))).sum(axis=1)
    return cell, gene


def gamma(max_nnz, length, k, extra=0):
    """(max column nnz + length + k^2 + 4 + extra) 2^-53: the first-order factor of the three sums of the identity -- ||a||^2
    (nnz terms), x . b (k terms, each b a sum of nnz products against a factor that was rounded once when scaled by d) and
    x^T G x (k^2 terms, each G a sum of `length` products) -- plus the four roundings that join them."""
    return (max_nnz + length + k * k + 4 + extra) * U
