"""The rules of the factor annotation (include/singlet_hip.h, "Factor annotation") restated in numpy and scipy: the group
moments of a means model in their stated summation orders, on the embedding side and on the gene side, and the fit, the
prior, the moderated t, its p-values, the log-odds and Benjamini-Hochberg from those moments.  The statistics are written
from the header's formulae with scipy's special functions (digamma, polygamma, the t distribution, brentq for the inverse
trigamma), not from the library's host code.  Nothing here is tuned to the device's output."""
import math

import numpy as np
from scipy import optimize, special, stats

import markers_restatement as mr

CHUNK = 256
THREADS = 256
SEG = 8192
BLOCK = 64
MAX_GROUPS = 1024
MAX_K = 1024


# ------------------------------------------------------------------------------------------------------ embedding moments
def _chunk_sums(M):
    """The chunk sums (nd x chunks) of the columns of M (nd x count, in position order) in sgl_group_means' order: chunks of
    256 positions; slot s of S = 256 / min(64, nd rounded up to a power of two) adds the positions s, s + S, ... in turn from
    +0.0, the slot sums go through the binary tree (slot s += slot s + stride, stride = S / 2 ... 1)."""
    nd, count = M.shape
    shift = 0
    while (1 << shift) < nd and shift < 6:
        shift += 1
    S = THREADS >> shift
    out = []
    for c0 in range(0, count, CHUNK):
        chunk = M[:, c0:c0 + CHUNK]
        rounds = -(-chunk.shape[1] // S)
        pad = np.zeros((nd, rounds * S))          # a position that does not exist adds +0.0: no partial sum is -0.0
        pad[:, :chunk.shape[1]] = chunk
        pad = pad.reshape(nd, rounds, S)
        acc = np.zeros((nd, S))
        for r in range(rounds):
            acc = acc + pad[:, r, :]
        stride = S >> 1
        while stride > 0:
            acc[:, :stride] = acc[:, :stride] + acc[:, stride:2 * stride]
            stride >>= 1
        out.append(acc[:, 0].copy())
    return np.array(out).T.reshape(nd, len(out))


def group_moments(F, labels, G):
    """(group_n, sum k x G, rss k) of the k x n matrix F under the labels (-1: left out)."""
    F = np.asarray(F, dtype=np.float64)
    labels = np.asarray(labels)
    k = F.shape[0]
    group_n = np.bincount(labels[labels >= 0], minlength=G).astype(np.int64)
    sums = np.zeros((k, G))
    rss = np.zeros(k)
    for g in range(G):
        cells = np.nonzero(labels == g)[0]           # ascending cell index
        if cells.size == 0:
            continue
        cs = _chunk_sums(F[:, cells])
        s = np.zeros(k)
        for ch in range(cs.shape[1]):
            s = s + cs[:, ch]
        sums[:, g] = s
        mean = s / np.float64(group_n[g])
        d = F[:, cells] - mean[:, None]
        rs = _chunk_sums(d * d)
        for ch in range(rs.shape[1]):                # the chunks of all groups in ascending order: one chain per factor
            rss = rss + rs[:, ch]
    return group_n, sums, rss


# ------------------------------------------------------------------------------------------------------------ gene moments
def gene_rss(x, cells, labels, G, group_n, nz, sums, skip_empty_blocks=False):
    """rss of one gene given as its stored entries in stored order; nz and sums (G values) as the marker sums give them."""
    l = np.asarray(labels)[cells]
    n = x.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.asarray(sums, dtype=np.float64) / np.asarray(group_n, dtype=np.float64)
    nb = (n + BLOCK - 1) // BLOCK
    T = np.zeros(nb * BLOCK)
    live = (l >= 0) & (x != 0)                       # an excluded cell, a stored zero, a place past the end: +0.0
    d = x[live] - mean[l[live]]
    T[np.nonzero(live)[0]] = d * d
    T = T.reshape(nb, BLOCK)
    part = mr._butterfly(T) if nb else np.zeros(0)
    present = (T != 0).any(axis=1) if nb else np.zeros(0, dtype=bool)
    per_seg = SEG // BLOCK
    E = 0.0
    for s0 in range(0, nb, per_seg):
        seg = 0.0
        for blk in range(s0, min(s0 + per_seg, nb)):
            if skip_empty_blocks and not present[blk]:
                continue
            seg = seg + part[blk]
        E = E + seg
    Z = 0.0
    for c in range(G):
        if group_n[c] == 0:
            continue
        Z = Z + np.float64(int(group_n[c]) - int(nz[c])) * (mean[c] * mean[c])
    return E + Z


def gene_moments(Tx, Ti, Tp, labels, G):
    """(group_n, nz m x G, sum m x G, rss m) from the CSC arrays of t(A) (one column per gene)."""
    m = len(Tp) - 1
    group_n, _ = mr.group_counts(labels, G)
    nz = np.zeros((m, G), dtype=np.int64)
    sums = np.zeros((m, G))
    rss = np.zeros(m)
    for g in range(m):
        x, cells = mr.gene_entries(Tx, Ti, Tp, g)
        _, nz[g] = mr.entry_counts(x, cells, labels, G)
        sums[g] = mr.group_sums(x, cells, labels, G, 0, skip_empty_blocks=True)
        rss[g] = gene_rss(x, cells, labels, G, group_n, nz[g], sums[g], skip_empty_blocks=True)
    return group_n, nz, sums, rss


# -------------------------------------------------------------------------------------------------------------- the statistics
def trigamma_inverse(x):
    """The y > 0 with polygamma(1, y) = x, by bracketing."""
    if not (x > 0):
        return math.nan
    if math.isinf(x):
        return 0.0
    f = lambda ly: math.log(special.polygamma(1, math.exp(ly))) - math.log(x)   # decreasing in log y
    lo, hi = -1.0, 1.0
    while f(lo) < 0:
        lo -= 4.0
    while f(hi) > 0:
        hi += 4.0
    return math.exp(optimize.brentq(f, lo, hi, xtol=1e-300, rtol=8.9e-16, maxiter=500))


def t_sf(t, df):
    """P(T > t), T Student's t with df degrees of freedom, the normal distribution for df = +Inf."""
    return stats.norm.sf(t) if np.isinf(df) else stats.t.sf(t, df)


def t_isf(p, df):
    return stats.norm.isf(p) if np.isinf(df) else stats.t.isf(p, df)


def bh(p):
    """Benjamini-Hochberg over the values that are not NaN (a NaN stays NaN); ties in ascending index order."""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    idx = np.nonzero(~np.isnan(p))[0]
    order = idx[np.argsort(p[idx], kind="stable")]
    nv = order.shape[0]
    run = math.inf
    for i in range(nv, 0, -1):
        v = (np.float64(nv) / np.float64(i)) * p[order[i - 1]]
        run = min(run, v)
        out[order[i - 1]] = min(run, 1.0)
    return out


def annotate_stats(group_n, sums, rss, center=True, scale=False, proportion=0.01, tail="pos"):
    """Everything sgl_annotate_stats returns, as a dict; sums rows x G, rss rows."""
    group_n = np.asarray(group_n, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    rss = np.asarray(rss, dtype=np.float64)
    rows, G = sums.shape
    nan_rg, nan_r, nan_g = (lambda: np.full((rows, G), np.nan)), (lambda: np.full(rows, np.nan)), (lambda: np.full(G, np.nan))
    out = {"coefficients": nan_rg(), "t": nan_rg(), "p_raw": nan_rg(), "p_adj": nan_rg(), "lods": nan_rg(), "Amean": nan_r(),
           "sigma": nan_r(), "s2_post": nan_r(), "stdev_unscaled": nan_g(), "var_prior": nan_g(), "s2_prior": math.nan,
           "df_prior": math.nan, "df_total": math.nan}
    N = int(group_n.sum())
    live = group_n > 0
    df = N - int(live.sum())
    out["df_residual"] = float(df)
    if df <= 0:
        return out
    gn = group_n.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = sums / gn[None, :]
        su = np.where(live, 1.0 / np.sqrt(gn), np.nan)
    grand = np.zeros(rows)
    for g in range(G):
        grand = grand + sums[:, g]
    amean = grand / np.float64(N)
    coef = mean - (amean[:, None] if center else 0.0)
    s2 = rss / np.float64(df)
    with np.errstate(invalid="ignore", divide="ignore"):
        if scale:
            tss = rss.copy()
            for g in range(G):
                if live[g]:
                    d = mean[:, g] - amean
                    tss = tss + gn[g] * (d * d)
            sd = np.sqrt(tss / (np.float64(N) - 1.0))
            coef = coef / sd[:, None]
            s2 = s2 / (sd * sd)
        coef[:, ~live] = np.nan
        out.update({"coefficients": coef, "Amean": amean, "sigma": np.sqrt(s2), "stdev_unscaled": su})
        usable = np.isfinite(s2) & (s2 >= 0)
        nu = int(usable.sum())
        if nu >= 2:
            x = s2[usable]
            med = np.median(x)
            if med == 0:
                med = 1.0
            x = np.maximum(x, 1e-5 * med)
            e = np.log(x) - special.digamma(df / 2.0) + math.log(df / 2.0)
            emean = e.mean()
            evar = e.var(ddof=1) - special.polygamma(1, df / 2.0)
            if evar > 0:
                df_prior = 2.0 * trigamma_inverse(float(evar))
                s2_prior = math.exp(emean + special.digamma(df_prior / 2.0) - math.log(df_prior / 2.0))
            else:
                df_prior, s2_prior = math.inf, math.exp(emean)
        else:
            df_prior, s2_prior = 0.0, math.nan
        df_total = min(df + df_prior, nu * df) if nu else math.nan
        if df_prior == 0.0:
            post = s2.copy()
        elif math.isinf(df_prior):
            post = np.full(rows, s2_prior)
        else:
            post = (df * s2 + df_prior * s2_prior) / (df + df_prior)
        post[~usable] = np.nan
        out.update({"s2_post": post, "s2_prior": s2_prior, "df_prior": df_prior, "df_total": df_total})
        t = coef / (su[None, :] * np.sqrt(post)[:, None])
        out["t"] = t
        if tail == "pos":
            p = t_sf(t, df_total)
        elif tail == "neg":
            p = t_sf(-t, df_total)
        elif tail == "std":
            p = 2.0 * t_sf(np.abs(t), df_total)
        else:
            raise ValueError("Invalid tail selection. Choose 'pos','neg', or 'std'")
        p = np.where(np.isnan(t), np.nan, p)
        out["p_raw"] = p
        lods = np.full((rows, G), np.nan)
        var_prior = np.full(G, np.nan)
        for g in range(G):
            if not live[g]:
                continue
            tg = t[:, g]
            ok = np.nonzero(~np.isnan(tg))[0]
            nr = ok.shape[0]
            if nr == 0:
                continue
            at = np.abs(tg)
            ntarget = int(math.ceil(proportion / 2.0 * nr))
            order = ok[np.lexsort((ok, -at[ok]))][:ntarget]   # |t| descending, ties by row index
            pp = max(ntarget / nr, proportion)
            v = []
            for i, r in enumerate(order, start=1):
                p0 = 2.0 * t_sf(at[r], df_total)
                ptarget = ((i - 0.5) / nr - (1.0 - pp) * p0) / pp
                v0 = 0.0
                if ptarget > p0:
                    q = t_isf(ptarget / 2.0, df_total)
                    v0 = su[g] ** 2 * ((at[r] / q) ** 2 - 1.0)
                v.append(min(max(v0, 0.01), 16.0))
            var_prior[g] = float(np.mean(v))
            r_ = (su[g] ** 2 + var_prior[g]) / su[g] ** 2
            t2 = tg * tg
            if df_prior > 1e6:
                kernel = t2 * (1.0 - 1.0 / r_) / 2.0
            else:
                kernel = (1.0 + df_total) / 2.0 * np.log((t2 + df_total) / (t2 / r_ + df_total))
            lods[:, g] = math.log(proportion / (1.0 - proportion)) - math.log(r_) / 2.0 + kernel
        out["lods"], out["var_prior"] = lods, var_prior
        out["p_adj"] = bh(p.T.reshape(-1)).reshape(G, rows).T   # column-major, as the library lays the table out
    return out


def model_results(st, noneg=True):
    """The (group, factor, fc, p) rows get_model_results keeps, in its order (groups, the factors ascending within one)."""
    rows, G = st["lods"].shape
    out = []
    for g in range(G):
        for f in range(rows):
            fc = st["lods"][f, g]
            if noneg and not fc > 0:
                continue
            out.append((g, f, fc, st["p_adj"][f, g]))
    return out


def check_args(labels, n, G, k):
    """None when the library accepts the arguments, else (what, position, value) of the first refusal in its order."""
    if labels is None:
        return ("null", -1, 0)
    if G < 1 or G > MAX_GROUPS:
        return ("groups", -1, 0)
    if k < 1 or k > MAX_K:
        return ("k", -1, 0)
    for j in range(n):
        if labels[j] < -1 or labels[j] >= G:
            return ("label", j, int(labels[j]))
    return None
