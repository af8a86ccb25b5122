"""The rules of the inverted-list neighbour search (include/singlet_hip.h, "Approximate embedding neighbours") restated in
numpy, without a device.  The distance and key rules are those of embedding_knn_restatement and knn_metric_restatement.

Operands: R, Q after dims; for cosine / correlation their unit columns (knn_metric_restatement.unit_columns).  Q None: the
references themselves.
Coarse quantiser, for every metric: the Euclidean sum of sgl_knn between a column and a centroid, and "nearest" by
(s, centroid index) -- embedding_knn_restatement.knn with the centroids as the references.
Training set: T = min(n_ref, 64 n_lists); training cell t is reference floor(t n_ref / T).  Seeds: centroid g is training cell
floor(g T / n_lists).  A Lloyd step: every training cell to its nearest centroid; every centroid becomes the mean of its cells
in sgl_group_means' order (group_sum below), over the training positions in ascending order; a centroid without cells stays.
Lists: every reference to its nearest centroid; members in ascending cell index.  Probes: the n_probe nearest centroids of a
query.  Result: among the members of the probed lists the n_neighbors best by (key, cell index), key the Euclidean sum or
1 - dot with the snap; the Euclidean distance is the root; missing slots are idx -1, dist +Inf.

Seconds on one CPU core: 2000 cells x 20 dimensions, 45 lists, 10 steps: about 1."""
import numpy as np

import embedding_knn_restatement as euclid
import knn_metric_restatement as km

TRAIN_PER_LIST = 64
GROUP_CHUNK = 256     # SGL_GROUP_CHUNK: cells per chunk of a group's cell list
GROUP_THREADS = 256   # lanes of a chunk's workgroup


def operands(R, Q=None, dims=None, metric="euclidean"):
    """(Rs nd x n_ref, Qs nd x n_query) as the search reads them."""
    R = np.asarray(R, dtype=np.float64)
    Q = None if Q is None else np.asarray(Q, dtype=np.float64)
    if dims is not None:
        R = R[np.asarray(dims)]
        Q = None if Q is None else Q[np.asarray(dims)]
    if metric != "euclidean":
        R = km.unit_columns(R, metric)[0]
        Q = None if Q is None else km.unit_columns(Q, metric)[0]
    return R, (R if Q is None else Q)


def train_count(n_ref, n_lists):
    return min(int(n_ref), TRAIN_PER_LIST * int(n_lists))


def train_picks(n_ref, n_lists):
    """The references that train, in training order."""
    T = train_count(n_ref, n_lists)
    return np.array([(t * int(n_ref)) // T for t in range(T)], dtype=np.int64)


def seed_picks(T, n_lists):
    """The training cells the centroids start as."""
    return np.array([(g * int(T)) // int(n_lists) for g in range(int(n_lists))], dtype=np.int64)


def group_sum(M):
    """The sum of the columns of M (nd x count, in position order) in sgl_group_means' order: chunks of 256 positions; inside a
    chunk FL = min(64, nd rounded up to a power of two) lanes run over the factors and S = 256 / FL slots over the positions:
    slot s adds the positions s, s + S, ... in that order, starting from +0.0; the slot sums are added by a binary tree
    (slot s += slot s + stride, stride = S / 2 ... 1); the chunk sums are added in chunk order, starting from +0.0.  (A
    position that does not exist adds +0.0, which changes no bit: no partial sum is -0.0.)"""
    nd, count = M.shape
    shift = 0
    while (1 << shift) < nd and shift < 6:
        shift += 1
    S = GROUP_THREADS >> shift
    total = np.zeros(nd)
    for c0 in range(0, count, GROUP_CHUNK):
        chunk = M[:, c0:c0 + GROUP_CHUNK]
        rounds = -(-chunk.shape[1] // S)
        pad = np.zeros((nd, rounds * S))
        pad[:, :chunk.shape[1]] = chunk
        pad = pad.reshape(nd, rounds, S)
        acc = np.zeros((nd, S))
        for r in range(rounds):
            acc = acc + pad[:, r, :]
        stride = S >> 1
        while stride > 0:
            acc[:, :stride] = acc[:, :stride] + acc[:, stride:2 * stride]
            stride >>= 1
        total = total + acc[:, 0]
    return total


def nearest(C, X, K=1):
    """idx n x K: the K centroids nearest to every column of X by (Euclidean sum, centroid index)."""
    return euclid.knn(C, X, K)[0]


def train(Rs, n_lists, n_iter=10):
    """(centroids nd x n_lists, assign int32[n_ref]) of the packed references Rs."""
    nd, n_ref = Rs.shape
    Tr = Rs[:, train_picks(n_ref, n_lists)]
    C = Tr[:, seed_picks(Tr.shape[1], n_lists)].copy()
    for _ in range(int(n_iter)):
        a = nearest(C, Tr)[:, 0]
        for g in range(n_lists):
            members = np.flatnonzero(a == g)
            if members.size:
                C[:, g] = group_sum(Tr[:, members]) / float(members.size)
    return C, nearest(C, Rs)[:, 0].astype(np.int32)


def pair_keys(Rs, Qs, metric):
    """key[r, q], n_ref x n_query: the Euclidean sum of sgl_knn, or 1 - dot with the snap of sgl_knn_metric."""
    if metric == "euclidean":
        acc = np.zeros((Rs.shape[1], Qs.shape[1]))
        with np.errstate(over="ignore"):
            for f in range(Rs.shape[0]):
                diff = Qs[f][None, :] - Rs[f][:, None]
                acc = acc + diff * diff
        return acc
    key = 1.0 - km.raw_dots(Rs, Qs)
    key[key < km.SNAP] = 0.0
    return key


def search(Rs, Qs, metric, C, assign, n_probe, n_neighbors):
    """(idx int32, dist), each n_query x n_neighbors, under the centroids C and the assignment assign."""
    K = int(n_neighbors)
    assign = np.asarray(assign)
    probes = nearest(C, Qs, int(n_probe))
    key = pair_keys(Rs, Qs, metric)
    nq = Qs.shape[1]
    idx = np.full((nq, K), -1, dtype=np.int32)
    dist = np.full((nq, K), np.inf)
    for j in range(nq):
        members = np.flatnonzero(np.isin(assign, probes[j]))   # ascending cell index
        order = members[np.lexsort((members, key[members, j]))][:K]
        idx[j, :order.size] = order
        dist[j, :order.size] = np.sqrt(key[order, j]) if metric == "euclidean" else key[order, j]
    return idx, dist


def knn_ivf(R, Q=None, n_neighbors=20, dims=None, metric="euclidean", n_lists=1, n_probe=1, n_iter=10):
    """The whole call: (idx, dist, centroids, assign)."""
    Rs, Qs = operands(R, Q, dims, metric)
    C, assign = train(Rs, n_lists, n_iter)
    idx, dist = search(Rs, Qs, metric, C, assign, n_probe, n_neighbors)
    return idx, dist, C, assign


def recall(idx, idx_exact):
    """The mean over the rows of the share of a row's exact neighbours that the same row of idx holds (-1 matches nothing)."""
    idx, idx_exact = np.asarray(idx), np.asarray(idx_exact)
    share = [np.isin(e[e >= 0], a).sum() / float(e.size) for a, e in zip(idx, idx_exact)]
    return float(np.mean(share))


def clustered(n=2000, k=20, n_profiles=12, seed=20261020):
    """The fixture "clustered": a mixture of n_profiles sparse non-negative profiles with multiplicative gamma noise -> (X k x n,
    label[n]).  A profile has about a third of its k entries non-zero, uniform in [0.5, 2); a cell is its profile times a
    per-entry gamma(shape 20, scale 1 / 20) factor (mean 1, coefficient of variation 0.22) times a per-cell size factor
    uniform in [0.8, 1.25), plus a floor of 0.01 gamma noise on every entry so that no two cells coincide."""
    rng = np.random.default_rng(seed)
    profiles = np.where(rng.random((k, n_profiles)) < 1.0 / 3.0, rng.uniform(0.5, 2.0, (k, n_profiles)), 0.0)
    label = rng.integers(0, n_profiles, n)
    X = profiles[:, label] * rng.gamma(20.0, 1.0 / 20.0, (k, n)) * rng.uniform(0.8, 1.25, n)[None, :]
    X = X + 0.01 * rng.gamma(2.0, 0.5, (k, n))
    return X, label
