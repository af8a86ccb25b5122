"""Test-side restatement of c_gcnmf (src/singlet.cpp:1668-1730) from the oracle's own pieces (ora.aat, ora.rhs, ora.nnls
per column, ora.scale, ora.cor), plus the cell graphs the GCNMF tests and scripts/gcnmf_rate.py use.

Matrices follow the oracle's convention: factors are (cols, k) C-contiguous arrays (== k x cols column-major); sparse
matrices are ora.CSC (genes x cells for A, cells x cells for G, G(r, c) = weight of neighbour r in cell c's convolution).
"""
import numpy as np


def _csc_from_coo(ora, rows, cols, vals, n):
    order = np.lexsort((rows, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    p = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=p[1:])
    return ora.CSC(vals, rows.astype(np.int32), p.astype(np.int32), n, n)


def lattice_graph(ora, side, perm=None):
    """side x side lattice, cell id y * side + x (row-major); column j holds its 3 x 3 neighbourhood including itself with
    weights (1.5 - distance) / 1.5, normalised to sum 1 per column (the weighting and normalisation of the reference's
    spatial_graph).  perm: optional relabelling, cell c -> perm[c] (P G P^T)."""
    n = side * side
    y, x = np.divmod(np.arange(n, dtype=np.int64), side)
    rows, cols, vals = [], [], []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ok = (y + dy >= 0) & (y + dy < side) & (x + dx >= 0) & (x + dx < side)
            c = np.nonzero(ok)[0]
            rows.append(c + dy * side + dx)
            cols.append(c)
            vals.append(np.full(c.size, (1.5 - np.hypot(dy, dx)) / 1.5))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    colsum = np.bincount(cols, weights=vals, minlength=n)
    vals = vals / colsum[cols]
    if perm is not None:
        rows, cols = perm[rows], perm[cols]
    return _csc_from_coo(ora, rows, cols, vals, n)


def random_directed_graph(ora, n, per_col, seed):
    """Asymmetric directed graph, no self-loops: every column draws `per_col` distinct other cells with positive weights."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for c in range(n):
        r = rng.choice(n - 1, size=per_col, replace=False)
        r[r >= c] += 1   # skip c itself
        rows.append(r)
        cols.append(np.full(per_col, c))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc_from_coo(ora, rows, cols, rng.uniform(0.1, 1.0, rows.size), n)


def sparse_odd_graph(ora, n, seed):
    """Empty columns (every 5th cell), self-loop-only columns (every 7th that is not empty), the rest 1 - 4 random entries."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for c in range(n):
        if c % 5 == 0:
            continue
        if c % 7 == 0:
            r = np.array([c])
        else:
            r = rng.choice(n, size=int(rng.integers(1, 5)), replace=False)
        rows.append(r)
        cols.append(np.full(r.size, c))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc_from_coo(ora, rows, cols, rng.uniform(0.1, 1.0, rows.size), n)


def hub_graph(ora, n, hub, hub_len, seed):
    """Column `hub` holds hub_len entries; every other column 0 - 3."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for c in range(n):
        r = rng.choice(n, size=hub_len if c == hub else int(rng.integers(0, 4)), replace=False)
        rows.append(r)
        cols.append(np.full(r.size, c))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc_from_coo(ora, rows, cols, rng.uniform(0.1, 1.0, rows.size), n)


EDGE_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 127, 128, 129, 130, 131, 191, 192, 193, 256, 257, 320]


def edge_length_graph(ora, n=320, seed=17, weights=None):
    """Column lengths at every edge of the convolution's loops: the four-deep main loop and its 1 - 3 entry tail, the
    largest non-hub column (128), the smallest hub (129: segments of 64 + 64 + 1), hubs that are whole multiples of the
    segment length (192, 256, 320) and one entry either side.  Column c holds EDGE_LENGTHS[c % 20] entries, except: column
    0 holds 129 and column n - 1 holds n (every row: rows 0 and n - 1 occur), columns 100 and 101 hold 192 and 193
    (adjacent hubs).  A column of one entry is a self-loop; every other column draws sorted distinct rows.
    weights = None: entry q (its position in the stored order) weighs s * j / 8 with j = q % 15 + 1, s = -1 where q % 3 ==
    0, else +1 -- exact in eighths, both signs.  Otherwise weights(nnz) supplies them (same structure)."""
    rng = np.random.default_rng(seed)
    lens = np.array([EDGE_LENGTHS[c % len(EDGE_LENGTHS)] for c in range(n)])
    lens[0], lens[n - 1], lens[100], lens[101] = 129, n, 192, 193
    assert lens.max() <= n
    rows = []
    for c in range(n):
        rows.append(np.array([c]) if lens[c] == 1 else np.sort(rng.choice(n, size=lens[c], replace=False)))
    rows = np.concatenate(rows).astype(np.int32)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    q = np.arange(rows.size)
    x = np.where(q % 3 == 0, -1.0, 1.0) * (q % 15 + 1) / 8.0 if weights is None else np.asarray(weights(rows.size), dtype=np.float64)
    return ora.CSC(x, rows, p, n, n)


def knn_hub_graph(ora, n, per_col=20, hubs=(), hub_len=129, seed=23):
    """A kNN-sized graph: every column holds per_col distinct rows with uniform(0.1, 1.0) weights, the columns listed in
    `hubs` hold hub_len (> 128: the segment pass sums them)."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for c in range(n):
        r = rng.choice(n, size=hub_len if c in hubs else per_col, replace=False)
        rows.append(r)
        cols.append(np.full(r.size, c))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return _csc_from_coo(ora, rows, cols, rng.uniform(0.1, 1.0, rows.size), n)


def identity_graph(ora, n):
    return ora.CSC(np.ones(n), np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32), n, n)


def transpose_graph(ora, G):
    return ora.transpose(G)


def convolve(G, X, cols=None):
    """(X G) as (cols, k): out[j] = sum over G's column j, in stored order, of G(r, j) * X[r]  (l.1684-1686)."""
    cols = range(G.ncol) if cols is None else cols
    out = np.zeros((len(cols), X.shape[1]))
    for o, j in enumerate(cols):
        b = np.zeros(X.shape[1])
        for q in range(G.p[j], G.p[j + 1]):
            b += G.x[q] * X[G.i[q]]
        out[o] = b
    return out


def update_h(ora, A, w, h, G, L1, L2):
    """gcnmf_update_h (l.1668-1691): B = rhs(A, w) (0 on empty columns), Bc = B G column by column, nnls for EVERY column."""
    a = ora.aat(w)
    B = ora.rhs(A, w)
    h = np.array(h, dtype=np.float64)
    for j in range(A.ncol):
        b_ = convolve(G, B, [j])[0]
        h[j] = ora.nnls(a, b_, h[j], L1, L2)[0]
    return h


def update_w(ora, At, w, h, G, L1, L2, pairwise=True):
    """gcnmf_update_w (l.1693-1710): a = AAt(h) of the plain h; b_j = sum over t(A)'s column j and over G's column c of
    (A(j, c) G(c', c)) h(c').  pairwise = True loops exactly so (l.1703-1706); False forms rhs(At, H G) (large sizes)."""
    a = ora.aat(h)
    w = np.array(w, dtype=np.float64)
    if pairwise:
        B = np.zeros((At.ncol, h.shape[1]))
        for j in range(At.ncol):
            b = np.zeros(h.shape[1])
            for q in range(At.p[j], At.p[j + 1]):
                c = At.i[q]
                for q2 in range(G.p[c], G.p[c + 1]):
                    b += (At.x[q] * G.x[q2]) * h[G.i[q2]]
            B[j] = b
    else:
        B = ora.rhs(At, convolve(G, h))
    for j in range(At.ncol):
        w[j] = ora.nnls(a, B[j], w[j], L1, L2)[0]
    return w


def c_gcnmf(ora, A, At, G, tol, maxit, L1, L2, w, pairwise=True):
    """c_gcnmf (l.1712-1730).  w: (m, k) (== k x m column-major).  Returns w (m, k), d, h (n, k), iter, tol."""
    w = np.array(w, dtype=np.float64)
    k = w.shape[1]
    h = np.zeros((A.ncol, k))
    d = np.ones(k)
    tol_, it, trace = 1.0, 0, []
    while it < maxit and tol_ > tol:
        w_it = w.copy()
        h = update_h(ora, A, w, h, G, L1, L2)
        h, d = ora.scale(h)
        w = update_w(ora, At, w, h, G, L1, L2, pairwise)
        w, d = ora.scale(w)
        tol_ = ora.cor(w, w_it)
        trace.append(tol_)
        it += 1
    return dict(w=w, d=d, h=h, iter=it, tol=np.array(trace))
