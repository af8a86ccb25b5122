"""The rules of the ligand-receptor test (include/singlet_hip.h, "Ligand-receptor interactions") restated in numpy: TEST
INFRASTRUCTURE ONLY.  Every sum is formed by np.add.at, which adds the values one by one in the order given, segment by segment;
one division and one 0.5 * (a + b) follow, each a numpy ufunc on doubles (no fused multiply-add), so a correct kernel gives the
same bits.

Layouts follow the Python layer: nz, sum, mean are G x K; score, n_ge, p, padj are P x K x K with [q, a, b] = ligand in class a,
receptor in class b; the null tensor is nperm x P x K x K."""
import numpy as np

from gsea_restatement import bh
from nhood_restatement import permuted

SEG = 8192
MAX_K = 256
MAX_NPERM = 1 << 20
MAX_VPW = 64
WAVE_LDS_BYTES = 32 << 10
WG_LDS_BYTES = 64 << 10
MAX_WAVES = 8
BATCH_BYTES = 256 << 20


def gene_major(x, i, p, m):
    """The gene-side image of a CSC matrix (m genes x n cells, rows ascending within a column): (x, cells, ptr) with the entries
    of gene g at ptr[g] .. ptr[g + 1] in ascending cell order -- the stored order of the rules."""
    x, i, p = np.asarray(x, dtype=np.float64), np.asarray(i, dtype=np.int64), np.asarray(p, dtype=np.int64)
    cell = np.repeat(np.arange(p.shape[0] - 1, dtype=np.int64), np.diff(p))
    o = np.argsort(i, kind="stable")
    ptr = np.concatenate(([0], np.cumsum(np.bincount(i, minlength=m)))).astype(np.int64)
    return x[o], cell[o], ptr


def class_sums(x, cells, lab, K):
    """sum[c] of one gene under one label vector: segments of SEG entries, np.add.at within a segment (sequential from +0.0),
    the segment partials added in ascending order from +0.0."""
    out = np.zeros(K)
    for s0 in range(0, x.shape[0], SEG):
        part = np.zeros(K)
        np.add.at(part, lab[cells[s0:s0 + SEG]], x[s0:s0 + SEG])
        out = out + part
    return out


def sums(gx, gcells, gptr, genes, labs, K):
    """nb x G x K: the sums of the listed genes under each of the nb label vectors."""
    labs = np.asarray(labs, dtype=np.int64)
    out = np.zeros((labs.shape[0], len(genes), K))
    for gi, g in enumerate(genes):
        a, b = int(gptr[g]), int(gptr[g + 1])
        for r in range(labs.shape[0]):
            out[r, gi] = class_sums(gx[a:b], gcells[a:b], labs[r], K)
    return out


def nonzeros(gx, gcells, gptr, genes, lab, K):
    """nz[g, c]: the stored x != 0 of gene g in class c; int64."""
    lab = np.asarray(lab, dtype=np.int64)
    out = np.zeros((len(genes), K), dtype=np.int64)
    for gi, g in enumerate(genes):
        a, b = int(gptr[g]), int(gptr[g + 1])
        out[gi] = np.bincount(lab[gcells[a:b]][gx[a:b] != 0], minlength=K)
    return out


def means(sum_, group_n):
    """sum / (double)n_c, one division; 0 / 0 = NaN for a class without cells."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return sum_ / np.asarray(group_n, dtype=np.float64)


def scores(mean, lig, rec):
    """P x K x K of one mean table (G x K): 0.5 * (mean[lig, a] + mean[rec, b]) when both are > 0, else +0.0."""
    ma, mb = mean[np.asarray(lig)][:, :, None], mean[np.asarray(rec)][:, None, :]
    with np.errstate(invalid="ignore"):
        both = (ma > 0) & (mb > 0)
        return np.where(both, 0.5 * (ma + mb), 0.0)


def stats(nperm, group_n, nz, lig, rec, n_ge, threshold=0.01, per_interaction=False):
    """{"expressed" (G x K bool), "p", "padj" (P x K x K)}."""
    group_n = np.asarray(group_n, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ex = (group_n[None, :] > 0) & (nz.astype(np.float64) / group_n.astype(np.float64)[None, :] >= threshold)
    on = ex[np.asarray(lig)][:, :, None] & ex[np.asarray(rec)][:, None, :]
    p = np.where(on, (1.0 + n_ge.astype(np.float64)) / (1.0 + float(nperm)), np.nan)
    P, K = p.shape[0], p.shape[1]
    if per_interaction:
        # the library's order of the pairs of one interaction: a + K b ascending
        padj = np.stack([bh(p[q].T.reshape(-1)).reshape(K, K).T for q in range(P)])
    else:
        # the library's order: q + P (a + K b) ascending
        padj = bh(p.transpose(2, 1, 0).reshape(-1)).reshape(K, K, P).transpose(2, 1, 0)
    return {"expressed": ex, "p": p, "padj": padj}


def ligrec(x, i, p, m, lab, K, genes, lig, rec, nperm, seed, threshold=0.01, per_interaction=False):
    """The whole call on a CSC matrix (m genes x n cells): the dict of Context.ligrec with "null", and the statistics."""
    lab = np.asarray(lab, dtype=np.int64)
    gx, gc, gp = gene_major(x, i, p, m)
    group_n = np.bincount(lab, minlength=K).astype(np.int64)
    s = sums(gx, gc, gp, genes, lab[None, :], K)[0]
    mean = means(s, group_n)
    score = scores(mean, lig, rec)
    labs = permuted(lab, seed, 0, nperm)
    null = np.stack([scores(means(sr, group_n), lig, rec) for sr in sums(gx, gc, gp, genes, labs, K)])
    n_ge = (null >= score[None]).sum(axis=0).astype(np.int64)
    out = {"group_n": group_n, "nz": nonzeros(gx, gc, gp, genes, lab, K), "sum": s, "mean": mean, "score": score, "n_ge": n_ge, "null": null}
    out.update(stats(nperm, group_n, out["nz"], lig, rec, n_ge, threshold, per_interaction))
    return out


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def vpw_max(K):
    for v in (64, 32, 16, 8, 4, 2, 1):
        if v * K * 8 <= WAVE_LDS_BYTES:
            return v
    return 0


def plan(n, K, G, segs, nvec, batch=0, path=0, vpw=0):
    """{"path", "vectors_per_wave", "waves", "lds_bytes", "batch"} as ligrec_host.h plans it."""
    v = vpw or vpw_max(K)
    p = 2 if path == 2 else 1
    waves = min(max(WG_LDS_BYTES // (v * K * 8), 1), MAX_WAVES)
    if batch == 0:
        batch = max(BATCH_BYTES // (n + (segs + 2 * G) * K * 8) // MAX_VPW * MAX_VPW, MAX_VPW)
    return {"path": p, "vectors_per_wave": v, "waves": waves, "lds_bytes": v * K * 8 * waves if p == 1 else 0, "batch": min(batch, nvec)}


def segments(lengths):
    return int(sum((int(v) + SEG - 1) // SEG for v in lengths))
