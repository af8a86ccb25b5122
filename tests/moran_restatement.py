"""The rules of the spatial autocorrelation calls (include/singlet_hip.h, "Spatial autocorrelation") restated in numpy,
operation by operation and in the stated summation orders; no device.  The graph moments, the per-gene moments, the cross
term, the embedding form and the assembly are written from the header, not from the library's code; the primitives of the
orders they share with older calls are those calls' restatements (variable_features_restatement: lanes, butterfly, segments;
markers_restatement: the block butterfly; annotate_restatement: the chunk sums of sgl_group_means, Benjamini-Hochberg).
direct_* are the definitions themselves on the dense n x n weight matrix in long double, any order: what the tests hold the
restatement against.  Nothing here is tuned to the device's output."""
import math

import numpy as np

import annotate_restatement as ar
import markers_restatement as mr
import variable_features_restatement as vf

SEG = 8192
BLOCK = 64
LDS_CAP = 5120
LD = np.longdouble
VARIANCES = ("randomisation", "normality")
ALTERNATIVES = ("two.sided", "greater", "less")


# ---------------------------------------------------------------------------------------------------------- graph moments
def graph_moments(Gx, Gi, Gp, n):
    """(S0, S1, S2, t) of the n x n CSC graph, every sum sequential in the stated order (Python floats: IEEE double, one
    rounding per operation)."""
    Gx, Gi, Gp = [float(v) for v in Gx], [int(v) for v in Gi], [int(v) for v in Gp]
    rows = [[] for _ in range(n)]                     # the counting transpose: row i as (column, weight), columns ascending
    for j in range(n):
        for q in range(Gp[j], Gp[j + 1]):
            rows[Gi[q]].append((j, Gx[q]))
    S0, t = 0.0, []
    for j in range(n):
        cs = 0.0
        for q in range(Gp[j], Gp[j + 1]):
            S0 = S0 + Gx[q]
            cs = cs + Gx[q]
        rs = 0.0
        for _, w in rows[j]:
            rs = rs + w
        t.append(rs + cs)
    S2 = 0.0
    for i in range(n):
        S2 = S2 + t[i] * t[i]
    S1 = 0.0
    for j in range(n):
        col = {Gi[q]: Gx[q] for q in range(Gp[j], Gp[j + 1])}      # w_rj
        row = dict(rows[j])                                       # w_jr
        for r in sorted(set(col) | set(row)):                     # the union pattern, rows ascending
            s = col.get(r, 0.0) + row.get(r, 0.0)
            S1 = S1 + s * s
    return S0, 0.5 * S1, S2, np.array(t, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------- per-gene moments
def gene_moments(x, cells, n, t):
    """(mean, M2, M4, T, c) of one gene given as its stored entries in stored order (ascending cells)."""
    x = np.asarray(x, dtype=np.float64)
    c = x.shape[0]
    m = vf.gene_sum(x) / np.float64(n)
    d = x - m
    d2 = d * d
    mm = m * m
    zeros = np.float64(n - c)
    M2 = vf.gene_sum(d2) + zeros * mm
    M4 = vf.gene_sum(d2 * d2) + zeros * (mm * mm)
    T = vf.gene_sum(x * np.asarray(t)[cells])
    return np.float64(m), np.float64(M2), np.float64(M4), np.float64(T), c


def entry_terms(x, cells, Gx, Gi, Gp, n):
    """p_e of every stored entry of one gene: x_j * q_e, q_e the stored-order sum from +0.0 over column j of G of w * x_r for
    the rows r the gene stores (an absent r adds nothing).  The columns are walked together, one stored position per round."""
    x, cells = np.asarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    Gp = np.asarray(Gp, dtype=np.int64)
    where = np.full(n, -1, dtype=np.int64)
    where[cells] = np.arange(cells.shape[0])
    lo, deg = Gp[cells], Gp[cells + 1] - Gp[cells]
    q = np.zeros(cells.shape[0])
    for step in range(int(deg.max()) if deg.size else 0):
        live = np.nonzero(deg > step)[0]
        at = lo[live] + step
        src = where[np.asarray(Gi)[at]]
        have = src >= 0
        live, at, src = live[have], at[have], src[have]
        q[live] = q[live] + np.asarray(Gx, dtype=np.float64)[at] * x[src]
    return x * q


def block_sum(terms):
    """The sum of per-entry terms in the block order of sgl_gene_group_moments' E[g]: segments of 8192, blocks of 64, a lane
    past the end holds +0.0, one butterfly per block, block sums ascending from +0.0, segment sums ascending from +0.0."""
    terms = np.asarray(terms, dtype=np.float64)
    total = np.float64(0.0)
    for a in range(0, terms.shape[0], SEG):
        seg_terms = terms[a:a + SEG]
        nb = -(-seg_terms.shape[0] // BLOCK)
        V = np.zeros(nb * BLOCK)
        V[:seg_terms.shape[0]] = seg_terms
        part = mr._butterfly(V.reshape(nb, BLOCK))
        seg = np.float64(0.0)
        for b in range(nb):
            seg = seg + part[b]
        total = total + seg
    return total


def cross_term(x, cells, Gx, Gi, Gp, n):
    return block_sum(entry_terms(x, cells, Gx, Gi, Gp, n))


def gene_path(c, path=0, lds_cap=0):
    """1 search, 2 table: the path a gene of c stored entries takes."""
    cap = LDS_CAP if lds_cap <= 0 or lds_cap > LDS_CAP else lds_cap
    if path == 2:
        return 2
    if path == 1:
        return 1 if c <= LDS_CAP else 2
    return 1 if c <= cap else 2


def moran_moments(Tx, Ti, Tp, n, Gx, Gi, Gp, genes=None, t=None):
    """The 6 x n_genes table of sgl_moran (mean, M2, M4, T, P, c_g) from the CSC arrays of t(A) (one column per gene)."""
    if t is None:
        t = graph_moments(Gx, Gi, Gp, n)[3]
    genes = range(len(Tp) - 1) if genes is None else genes
    out = np.zeros((6, len(genes)))
    for q, g in enumerate(genes):
        x, cells = mr.gene_entries(Tx, Ti, Tp, g)
        m, M2, M4, T, c = gene_moments(x, cells, n, t)
        out[:, q] = (m, M2, M4, T, cross_term(x, cells, Gx, Gi, Gp, n), c)
    return out


# --------------------------------------------------------------------------------------------------------- embedding form
def _all_cells_sum(M):
    """Row sums of M (k x n) in sgl_group_means' order over all cells: the chunk sums ascending from +0.0."""
    cs = ar._chunk_sums(np.asarray(M, dtype=np.float64))
    s = np.zeros(M.shape[0])
    for ch in range(cs.shape[1]):
        s = s + cs[:, ch]
    return s


def embedding_moments(F, Gx, Gi, Gp):
    """(moments 6 x k: +0.0, M2, M4, +0.0, C, n; mean k) of the rows of F (k x n)."""
    F = np.asarray(F, dtype=np.float64)
    k, n = F.shape
    Gp, Gi, Gx = np.asarray(Gp, dtype=np.int64), np.asarray(Gi), np.asarray(Gx, dtype=np.float64)
    mean = _all_cells_sum(F) / np.float64(n)
    Z = F - mean[:, None]
    Y = np.zeros((k, n))
    deg = np.diff(Gp)
    for step in range(int(deg.max()) if n else 0):
        live = np.nonzero(deg > step)[0]
        at = Gp[live] + step
        Y[:, live] = Y[:, live] + Gx[at][None, :] * Z[:, Gi[at]]
    Z2 = Z * Z
    out = np.zeros((6, k))
    out[1], out[2], out[4], out[5] = _all_cells_sum(Z2), _all_cells_sum(Z2 * Z2), _all_cells_sum(Z * Y), n
    return out, mean


# ----------------------------------------------------------------------------------------------------------- the assembly
def cross_product(moments, S0):
    """C = (P - m * T) + (m * m) * S0, one value per row."""
    m, T, P = moments[0], moments[3], moments[4]
    return (P - m * T) + (m * m) * np.float64(S0)


def stats(n, S0, S1, S2, moments, variance="randomisation", alternative="two.sided"):
    """{"I", "EI", "sd", "z", "p", "p_adj"} of sgl_moran_stats; moments 6 x rows."""
    moments = np.asarray(moments, dtype=np.float64)
    nn, S0, S1, S2 = np.float64(n), np.float64(S0), np.float64(S1), np.float64(S2)
    M2, M4 = moments[1], moments[2]
    EI = np.float64(-1.0) / np.float64(n - 1)
    s02 = S0 * S0
    with np.errstate(all="ignore"):
        C = cross_product(moments, S0)
        I = (nn / S0) * (C / M2)
        if VARIANCES.index(variance) == 1:
            V = ((nn * nn) * S1 - nn * S2 + 3.0 * s02) / (((nn * nn) - 1.0) * s02) - EI * EI
            V = np.full(moments.shape[1], V)
        else:
            b2 = (nn * M4) / (M2 * M2)
            a = nn * (((nn * nn) - 3.0 * nn + 3.0) * S1 - nn * S2 + 3.0 * s02)
            b = b2 * ((nn * (nn - 1.0)) * S1 - (2.0 * nn) * S2 + 6.0 * s02)
            V = (a - b) / (((nn - 1.0) * (nn - 2.0) * (nn - 3.0)) * s02) - EI * EI
        sd = np.sqrt(V)
        z = (I - EI) / sd
    const = M2 == 0
    I, z = np.where(const, np.nan, I), np.where(const, np.nan, z)
    alt = ALTERNATIVES.index(alternative)
    root2 = math.sqrt(2.0)
    p = np.full(z.shape, np.nan)
    for r in range(z.shape[0]):
        if np.isnan(z[r]):
            continue
        zz = float(z[r])
        p[r] = math.erfc(abs(zz) / root2) if alt == 0 else 0.5 * math.erfc(zz / root2) if alt == 1 else 0.5 * math.erfc(-zz / root2)
    return {"I": I, "EI": np.full(z.shape, EI), "sd": sd, "z": z, "p": p, "p_adj": ar.bh(p)}


def rank(p, I, genes):
    """(p ascending, I descending, gene index ascending), NaN rows last."""
    bad = np.isnan(p) | np.isnan(I)
    return np.lexsort((np.asarray(genes), np.where(bad, 0.0, -np.asarray(I)), np.where(bad, np.inf, p), bad))


# ------------------------------------------------------------------------------------- the definitions, dense, long double
def dense_weights(Gx, Gi, Gp, n):
    W = np.zeros((n, n))
    for j in range(n):
        W[np.asarray(Gi)[Gp[j]:Gp[j + 1]], j] = np.asarray(Gx)[Gp[j]:Gp[j + 1]]
    return W


def direct(xfull, W, variance="randomisation"):
    """Moran's I of one dense vector over the dense W by the definitions in long double: dict of C, scale (the magnitude the
    error of C is measured against), M2, M4, I, EI, sd, z, S0, S1, S2."""
    x, W = np.asarray(xfull, dtype=LD), np.asarray(W, dtype=LD)
    n = x.shape[0]
    nn = LD(n)
    m = x.sum() / nn
    d = x - m
    C = (W * np.outer(d, d)).sum()
    t = W.sum(axis=0) + W.sum(axis=1)
    S0, S1, S2 = W.sum(), LD(0.5) * ((W + W.T) ** 2).sum(), (t * t).sum()
    scale = (np.abs(W) * np.outer(np.abs(d), np.abs(d))).sum() + np.abs(m) * np.abs(x * t).sum() + m * m * np.abs(S0)
    M2, M4 = (d ** 2).sum(), (d ** 4).sum()
    EI = LD(-1.0) / (nn - 1)
    out = dict(C=C, scale=scale, M2=M2, M4=M4, EI=EI, S0=S0, S1=S1, S2=S2, t=t, mean=m)
    with np.errstate(all="ignore"):
        I = (nn / S0) * (C / M2)
        if variance == "normality":
            V = (nn * nn * S1 - nn * S2 + 3 * S0 * S0) / ((nn * nn - 1) * S0 * S0) - EI * EI
        else:
            b2 = nn * M4 / (M2 * M2)
            V = (nn * ((nn * nn - 3 * nn + 3) * S1 - nn * S2 + 3 * S0 * S0) - b2 * (nn * (nn - 1) * S1 - 2 * nn * S2 + 6 * S0 * S0)) / (
                (nn - 1) * (nn - 2) * (nn - 3) * S0 * S0) - EI * EI
        sd = np.sqrt(V)
        out.update(I=I, sd=sd, z=(I - EI) / sd)
    return out


# ---------------------------------------------------------------------------------------------------------------- fixtures
def csc_graph(W):
    """(Gx, Gi, Gp) of the stored pattern of the dense W (its non-zeros), rows ascending."""
    n = W.shape[0]
    Gi, Gx, Gp = [], [], [0]
    for j in range(n):
        r = np.nonzero(W[:, j])[0]
        Gi.extend(r.tolist())
        Gx.extend(W[r, j].tolist())
        Gp.append(len(Gi))
    return np.array(Gx, dtype=np.float64), np.array(Gi, dtype=np.int32), np.array(Gp, dtype=np.int32)


def grid_graph(side_x, side_y):
    """Rook neighbours on a side_x x side_y grid, unit weights, no diagonal: (Gx, Gi, Gp), cell = y * side_x + x."""
    n = side_x * side_y
    Gi, Gp = [], [0]
    for c in range(n):
        x, y = c % side_x, c // side_x
        nb = [c - side_x] * (y > 0) + [c - 1] * (x > 0) + [c + 1] * (x < side_x - 1) + [c + side_x] * (y < side_y - 1)
        Gi.extend(nb)
        Gp.append(len(Gi))
    return np.ones(len(Gi)), np.array(Gi, dtype=np.int32), np.array(Gp, dtype=np.int32)


def planted_tissue(side=40, m=300, planted=10, seed=0):
    """The fixture of examples/spatial_variable_features.py: a side x side grid of cells; `planted` genes expressed in a
    rectangular domain each (Poisson 6 inside, 0.3 outside), the other genes the same values with the cells shuffled.
    Returns (D genes x cells dense counts, (Gx, Gi, Gp) rook graph, the planted gene indices)."""
    rng = np.random.default_rng(seed)
    n = side * side
    D = np.zeros((m, n))
    xs, ys = np.arange(n) % side, np.arange(n) // side
    which = np.sort(rng.permutation(m)[:planted])
    for q in range(m):
        x0, y0 = rng.integers(0, side // 2, 2)
        w, h = rng.integers(side // 4, side // 2, 2)
        inside = (xs >= x0) & (xs < x0 + w) & (ys >= y0) & (ys < y0 + h)
        v = rng.poisson(np.where(inside, 6.0, 0.3)).astype(np.float64)
        D[q] = v
    for q in range(m):
        if q not in set(which.tolist()):
            D[q] = D[q][rng.permutation(n)]
    return D, grid_graph(side, side), which
