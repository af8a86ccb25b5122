"""The rules of sgl_knn (include/singlet_hip.h) restated in numpy, without a device.

For query column q and reference column r, over the selected dimensions f in the listed order: s = +0.0; t = q_f - r_f;
s = s + t * t, in double.  numpy neither contracts a product into the addition that follows nor reorders these element-wise
operations, so the n_ref x n_query accumulator below holds the stated sums bit for bit.  The references rank by
(s, reference index) ascending -- np.lexsort with the index as the secondary key --, the first n_neighbors are the result,
and the distance is np.sqrt(s), the IEEE root.

Seconds on one CPU core: 50 x 1025 against itself 0.3, 3 x 4097 against itself 2, 130 x 130 against itself 0.01."""
import numpy as np


def knn(R, Q=None, n_neighbors=20, dims=None):
    """R k x n_ref, Q k x n_query (None: R itself), dims 0-based rows (None: all, in stored order) -> (idx int32, dist), each
    n_query x n_neighbors, row j = the neighbours of query j in rank order."""
    R = np.asarray(R, dtype=np.float64)
    Q = R if Q is None else np.asarray(Q, dtype=np.float64)
    if dims is not None:
        R, Q = R[np.asarray(dims)], Q[np.asarray(dims)]
    n_ref, nq, K = R.shape[1], Q.shape[1], int(n_neighbors)
    acc = np.zeros((n_ref, nq))
    with np.errstate(over="ignore"):
        for f in range(R.shape[0]):
            diff = Q[f][None, :] - R[f][:, None]
            acc = acc + diff * diff
    index = np.arange(n_ref)
    idx = np.empty((nq, K), dtype=np.int32)
    s = np.empty((nq, K))
    for j in range(nq):
        order = np.lexsort((index, acc[:, j]))[:K]
        idx[j] = order
        s[j] = acc[order, j]
    return idx, np.sqrt(s)


def nn_graph(idx, n):
    """(p, i) of the n x n pattern whose column j holds the rows idx[j], ascending."""
    idx = np.asarray(idx)
    return np.arange(idx.shape[0] + 1, dtype=np.int64) * idx.shape[1], np.sort(idx, axis=1).ravel().astype(np.int32)


def seurat_snn(idx, n, prune):
    """Seurat's ComputeSNN rule on the neighbour lists idx (n x K): shared = NN NN^T, value = shared / (2 K - shared), entries
    below prune zeroed (equality stays).  Dense n x n, [i, j] = the value between cells i and j."""
    K = idx.shape[1]
    NN = np.zeros((n, n))
    NN[np.repeat(np.arange(n), K), np.asarray(idx).ravel()] = 1.0
    shared = NN @ NN.T
    v = shared / (2.0 * K - shared)
    v[v < prune] = 0.0
    return v
