"""Writes tests/golden/umap_transform_fixtures.npz: the quality criterion of the layout transform
(tests/test_umap_transform_restatement.py, tests/test_gpu_umap_transform.py) on the two data sets of umap_fixtures.npz with
every fourth point held out as a query.  Stored: which points are queries, their exact neighbour lists against the rest, the
layout of the rest (the device's umap_layout of its fuzzy graph from the PCA start: existing code), the score of the start,
and the scores the SEQUENTIAL transform (umap_transform_restatement.sequential_transform: umap-learn's manner, one slot after
the other, only the query moving) reaches for the seeds 0 .. 9.  No program text is stored.

Two steps, because the layout of the rest needs the device and the yardstick does not:

    python tests/golden/make_umap_transform_fixtures.py --layout-only layouts.npz      (on the GPU)
    python tests/golden/make_umap_transform_fixtures.py --layout layouts.npz           (anywhere; a plain Python loop)

Without an argument both run here."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import umap_restatement as ur  # noqa: E402
import umap_transform_restatement as tr  # noqa: E402

T_EPOCHS, ALPHA0, SHARE_K, LAYOUT_SEED = 100, 0.25, 15, 42
SEEDS = range(10)


def split(z, name):
    X = z[name + "_X"]
    query = np.arange(X.shape[0]) % 4 == 0
    return X[~query], X[query], z[name + "_labels"][~query], z[name + "_labels"][query], query


def query_lists(R, Q, K):
    """Exact lists of the queries against the references by (squared distance, index), the roots as distances."""
    D = np.zeros((Q.shape[0], R.shape[0]))
    for f in range(R.shape[1]):
        t = Q[:, None, f] - R[None, :, f]
        D = D + t * t
    idx = np.argsort(D, axis=1, kind="stable")[:, :K]
    return idx.astype(np.int32), np.sqrt(np.take_along_axis(D, idx, axis=1))


def device_layouts(z):
    import singlet_amd as sa
    K, epochs, neg, _ = (int(v) for v in z["settings"])
    a, b = z["ab"]
    out = {}
    for name in z["names"]:
        R = split(z, name)[0]
        idx, dist = ur.knn_lists(R, K)
        G = sa.fuzzy_simplicial_set(idx, dist)
        out[name + "_Yref"] = sa.umap_layout(G, ur.pca_start(R, 2), a, b, epochs, 1.0, neg, LAYOUT_SEED)
    return out


def main(argv):
    z = np.load(os.path.join(HERE, "umap_fixtures.npz"))
    if len(argv) == 2 and argv[0] == "--layout-only":
        np.savez_compressed(argv[1], **device_layouts(z))
        return
    layouts = np.load(argv[1]) if len(argv) == 2 and argv[0] == "--layout" else device_layouts(z)
    K, _, neg, _ = (int(v) for v in z["settings"])
    a, b = z["ab"]
    out = {"names": z["names"], "settings": np.array([K, T_EPOCHS, neg, SHARE_K], dtype=np.int64), "ab": z["ab"], "alpha0": np.array(ALPHA0)}
    for name in z["names"]:
        R, Q, _, _, query = split(z, name)
        Yref = layouts[name + "_Yref"]
        idx, dist = query_lists(R, Q, K)
        _, _, W = tr.fuzzy_query(idx, dist)
        Y0 = tr.start(idx, W, Yref)
        s_seq = []
        for seed in SEEDS:
            t0 = time.time()
            Y = tr.sequential_transform(idx, W, Yref, Y0, a, b, T_EPOCHS, ALPHA0, neg, seed)
            s_seq.append(tr.neighbour_share(R, Q, Yref, Y, SHARE_K))
            print(name, "seed", seed, "share", s_seq[-1], "%.0f s" % (time.time() - t0), flush=True)
        out.update({name + "_query": query, name + "_idx": idx, name + "_dist": dist, name + "_Yref": Yref,
                    name + "_S_start": np.array(tr.neighbour_share(R, Q, Yref, Y0, SHARE_K)), name + "_S_seq": np.array(s_seq)})
        print(name, "start", float(out[name + "_S_start"]), "sequential", min(s_seq), "to", max(s_seq), flush=True)
    np.savez_compressed(os.path.join(HERE, "umap_transform_fixtures.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1:])
