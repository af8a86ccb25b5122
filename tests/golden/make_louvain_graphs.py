"""Writes tests/golden/louvain_graphs.npz: the fixture graphs of the clustering tests, their planted labels, and the
modularity that networkx's louvain_communities reaches on each of them with seeds 0 .. 9 (networkx is the yardstick of the
quality criterion and is needed only here; the tests read the file).

    python tests/golden/make_louvain_graphs.py

Every graph is a symmetric dgCMatrix (p, i, x) with bitwise equal A_ij and A_ji.  The modularity stored for a networkx
partition is this library's formula (diagonal entries counted once) evaluated on that partition; without a diagonal it
agrees with networkx's own figure to 1e-13, which is asserted here."""
import os
import sys

import networkx as nx
import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import louvain_restatement as lr  # noqa: E402


def snn_graph(X, K, keep_diagonal, prune=1 / 15):
    """Seurat's SNN of the exact K nearest neighbours (self included): Jaccard index inter / (2K - inter), kept at >= prune."""
    n = X.shape[0]
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2) if n <= 1600 else None
    M = np.zeros((n, n), dtype=np.int32)
    for a in range(n):
        row = d2[a] if d2 is not None else ((X - X[a]) ** 2).sum(axis=1)
        M[a, np.argsort(row, kind="stable")[:K]] = 1
    inter = (M @ M.T).astype(np.float64)
    J = inter / (2.0 * K - inter)
    J[J < prune] = 0.0
    np.fill_diagonal(J, 1.0 if keep_diagonal else 0.0)
    assert np.array_equal(J, J.T)
    return sp.csc_matrix(J)


def blobs(rng, n, centres, dim, spread, K, keep_diagonal):
    C = rng.standard_normal((centres, dim)) * 4.0
    lab = rng.integers(0, centres, n)
    X = C[lab] + spread * rng.standard_normal((n, dim))
    return snn_graph(X, K, keep_diagonal), lab


def ring_of_cliques(cliques, size):
    n = cliques * size
    A = np.zeros((n, n))
    lab = np.repeat(np.arange(cliques), size)
    for c in range(cliques):
        s = c * size
        A[s:s + size, s:s + size] = 1.0
        a, b = s + size - 1, ((c + 1) % cliques) * size
        A[a, b] = A[b, a] = 1.0
    np.fill_diagonal(A, 0.0)
    return sp.csc_matrix(A), lab


def block_model(rng, blocks, per, p_in, p_out):
    n = blocks * per
    lab = np.repeat(np.arange(blocks), per)
    P = np.where(lab[:, None] == lab[None, :], p_in, p_out)
    U = np.triu(rng.random((n, n)) < P, 1)
    A = (U | U.T).astype(np.float64)
    return sp.csc_matrix(A), lab


def nx_modularities(G, gammas):
    """Ten seeds per gamma -> array (len(gammas), 10), in this library's formula."""
    G = sp.csc_matrix(G)
    G.sort_indices()
    p, i, x = lr.as_graph(G.indptr, G.indices, G.data)
    g = nx.from_scipy_sparse_array(G)
    has_diag = G.diagonal().any()
    out = np.zeros((len(gammas), 10))
    for a, gamma in enumerate(gammas):
        for seed in range(10):
            parts = nx.community.louvain_communities(g, weight="weight", resolution=gamma, seed=seed)
            lab = np.zeros(G.shape[0], dtype=np.int64)
            for c, mem in enumerate(parts):
                lab[list(mem)] = c
            out[a, seed] = lr.modularity(p, i, x, lab, gamma)[0]
            if not has_diag:
                assert abs(out[a, seed] - nx.community.modularity(g, parts, weight="weight", resolution=gamma)) < 1e-13
    return out


def main():
    rng = np.random.default_rng(20261019)
    graphs = {
        "snn_noisy": blobs(rng, 1500, 8, 6, 2.5, 20, False) + ([0.5, 1.0, 2.0],),
        "snn_weak20": blobs(rng, 2000, 20, 4, 1.6, 10, False) + ([1.0],),
        "snn_diag": blobs(rng, 3000, 12, 8, 1.5, 10, True) + ([1.0],),
        "cliques": ring_of_cliques(30, 6) + ([1.0],),
        "sbm": block_model(rng, 8, 100, 0.2, 0.02) + ([1.0],),
    }
    out = {"names": np.array(list(graphs))}
    for name, (G, lab, gammas) in graphs.items():
        G.sort_indices()
        out[name + "_p"] = G.indptr.astype(np.int32)
        out[name + "_i"] = G.indices.astype(np.int32)
        out[name + "_x"] = G.data.astype(np.float64)
        out[name + "_planted"] = lab.astype(np.int32)
        out[name + "_gammas"] = np.array(gammas)
        out[name + "_nx_q"] = nx_modularities(G, gammas)
        print(name, G.shape[0], G.nnz, out[name + "_nx_q"].min(axis=1), out[name + "_nx_q"].max(axis=1), flush=True)
    path = os.path.join(HERE, "louvain_graphs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
