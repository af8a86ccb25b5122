"""The rules of sgl_knn_metric (include/singlet_hip.h) restated in numpy, without a device.

Unit columns, per column x of an operand after dims, over the nd selected rows, in double and in the listed order:
correlation m = (+0.0 + x_0 + x_1 + ...) / nd and y = x - m, cosine y = x; s2 = +0.0, s2 = s2 + y_f * y_f; nrm = sqrt(s2);
u = y / nrm where nrm != 0 and +0.0 everywhere where nrm == 0.  A column whose nrm is 0 or +Inf has no direction: all its u
are zeros.  Key of a pair: dot = +0.0, dot = dot + uq_f * ur_f; key = 1.0 - dot; key < 2^-40 -> +0.0.  The references rank
by (key, reference index) ascending and the distance is the key itself.  numpy neither contracts a product into the addition
that follows nor reorders these element-wise operations, so the arrays below hold the stated values bit for bit.

metric "euclidean" is tests/embedding_knn_restatement.py, unchanged."""
import numpy as np

import embedding_knn_restatement as euclid

METRICS = {"euclidean": 0, "cosine": 1, "correlation": 2}
SNAP = 2.0 ** -40


def unit_columns(X, metric):
    """X nd x n (dims already applied) -> (U nd x n, no_direction bool[n])."""
    X = np.asarray(X, dtype=np.float64)
    nd, n = X.shape
    with np.errstate(all="ignore"):
        Y = X
        if metric == "correlation":
            m = np.zeros(n)
            for f in range(nd):
                m = m + X[f]
            m = m / float(nd)
            Y = X - m[None, :]
        else:
            assert metric == "cosine", metric
        s2 = np.zeros(n)
        for f in range(nd):
            s2 = s2 + Y[f] * Y[f]
        nrm = np.sqrt(s2)
        U = np.where(nrm[None, :] != 0.0, Y / nrm[None, :], 0.0)
    return U, (nrm == 0.0) | (nrm == np.inf)


def raw_dots(UR, UQ):
    """dot[r, q] of the unit columns, n_ref x n_query."""
    acc = np.zeros((UR.shape[1], UQ.shape[1]))
    for f in range(UR.shape[0]):
        acc = acc + UQ[f][None, :] * UR[f][:, None]
    return acc


def keys(R, Q, metric, dims=None):
    """(key n_ref x n_query, the number of columns without direction among R and -- when given -- Q)."""
    R = np.asarray(R, dtype=np.float64)
    if dims is not None:
        R = R[np.asarray(dims)]
    UR, zr = unit_columns(R, metric)
    count = int(zr.sum())
    UQ = UR
    if Q is not None:
        Q = np.asarray(Q, dtype=np.float64)
        if dims is not None:
            Q = Q[np.asarray(dims)]
        UQ, zq = unit_columns(Q, metric)
        count += int(zq.sum())
    key = 1.0 - raw_dots(UR, UQ)
    key[key < SNAP] = 0.0
    return key, count


def knn(R, Q=None, n_neighbors=20, dims=None, metric="cosine", with_count=False):
    """As embedding_knn_restatement.knn: (idx int32, dist), each n_query x n_neighbors; dist is the key."""
    if metric == "euclidean":
        out = euclid.knn(R, Q, n_neighbors, dims)
        return out + (0,) if with_count else out
    key, count = keys(R, Q, metric, dims)
    n_ref, nq = key.shape
    K = int(n_neighbors)
    index = np.arange(n_ref)
    idx = np.empty((nq, K), dtype=np.int32)
    dist = np.empty((nq, K))
    for j in range(nq):
        order = np.lexsort((index, key[:, j]))[:K]
        idx[j] = order
        dist[j] = key[order, j]
    return (idx, dist, count) if with_count else (idx, dist)


def rays(k=10, n=600, n_labels=6, seed=20250101):
    """The fixture "rays": cells on n_labels close rays with magnitudes over three decades -> (X k x n, label[n])."""
    rng = np.random.default_rng(seed)
    label = np.arange(n) % n_labels
    dirs = 1 + 0.5 * rng.random((k, n_labels))
    scale = 10 ** rng.uniform(-1.5, 1.5, n)
    X = dirs[:, label] * scale * (1 + 0.02 * rng.random((k, n)))
    return X, label


def purity(idx, label):
    """The share of listed neighbours that carry the query cell's label."""
    return float((label[idx] == label[:, None]).mean())
