"""The planted fixture of the ligand-receptor test, shared by the CPU and the GPU tests: 320 cells in 4 clusters of 80, 14 genes.
Gene "LIG" is up in cluster 0, gene "REC" up in cluster 1; the other twelve genes ("G02" .. "G13") carry no structure.  Values
are log1p of Poisson counts, as after log-normalisation.  Pair 0 is (LIG, REC); the other pairs join unstructured genes, one of
them a gene with itself and one listed twice."""
import numpy as np

N_CELLS, N_CLUSTERS, N_GENES = 320, 4, 14
NAMES = ["LIG", "REC"] + ["G%02d" % g for g in range(2, N_GENES)]
PAIRS = [("LIG", "REC"), ("G02", "G03"), ("G04", "G05"), ("G06", "G07"), ("G08", "G09"), ("G10", "G11"), ("G12", "G12"), ("G02", "G03"),
         ("G13", "G04")]
NPERM = 200


def matrix(seed=0):
    """(x, i, p) of the CSC matrix, 14 genes x 320 cells (rows ascending in every column), and the labels."""
    rng = np.random.default_rng(1000 + seed)
    lab = (np.arange(N_CELLS) % N_CLUSTERS).astype(np.int32)
    rate = np.full((N_GENES, N_CELLS), 0.8)
    rate[0] = np.where(lab == 0, 5.0, 0.2)
    rate[1] = np.where(lab == 1, 4.0, 0.3)
    dense = np.log1p(rng.poisson(rate).astype(np.float64))
    rows, cols = np.nonzero(dense.T)                        # cell-major: rows of dense.T are the cells
    x, i = dense.T[rows, cols], cols.astype(np.int32)
    p = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=N_CELLS)))).astype(np.int32)
    return x, i, p, lab


def planted_claims(out, nperm=NPERM):
    """What the fixture must show, on the restatement and on the device alike: no relabelling reaches the planted pair's score
    between cluster 0 (ligand) and cluster 1 (receptor), so its p is the floor 1 / (nperm + 1); the reverse direction is
    nothing special."""
    assert out["n_ge"][0, 0, 1] == 0 and out["p"][0, 0, 1] == 1.0 / (nperm + 1.0)
    assert out["p"][0, 0, 1] == np.nanmin(out["p"]) and out["n_ge"][0, 1, 0] > nperm // 2
    assert out["padj"][0, 0, 1] == np.nanmin(out["padj"])
