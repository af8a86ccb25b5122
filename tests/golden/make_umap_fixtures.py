"""Writes tests/golden/umap_fixtures.npz: the two data sets of the layout's quality criterion (tests/test_umap_restatement.py,
tests/test_gpu_umap.py) with what the tests must not recompute -- the points, their exact k-NN lists, the PCA start, the
trustworthiness of the start, and the trustworthiness the SEQUENTIAL optimiser (umap_restatement.sequential_layout: umap-learn's
edge order, head and tail both moving) reaches for the seeds 0 .. 9.  Deterministic; takes some minutes (the sequential
optimiser is a plain Python loop).

    python tests/golden/make_umap_fixtures.py
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import umap_restatement as ur  # noqa: E402

K, EPOCHS, A, B, NEG, TRUST_K = 15, 200, 1.577, 0.8951, 5, 15
SEEDS = range(10)


def blobs():
    """800 points in 6 blobs of 10 dimensions (unit noise around centres of scale 3: a PCA start of trustworthiness 0.94)."""
    rng = np.random.default_rng(20240601)
    centres = rng.standard_normal((6, 10)) * 3.0
    labels = np.arange(800) % 6
    return centres[labels] + rng.standard_normal((800, 10)), labels


def weak():
    """1 200 points around 20 weakly separated centres (scale 2.5: a PCA start of trustworthiness 0.85)."""
    rng = np.random.default_rng(20240602)
    centres = rng.standard_normal((20, 10)) * 2.5
    labels = np.arange(1200) % 20
    return centres[labels] + rng.standard_normal((1200, 10)), labels


def main():
    out = {"names": np.array(["blobs", "weak"]), "settings": np.array([K, EPOCHS, NEG, TRUST_K], dtype=np.int64),
           "ab": np.array([A, B])}
    for name, make in (("blobs", blobs), ("weak", weak)):
        X, labels = make()
        idx, dist = ur.knn_lists(X, K)
        Y0 = ur.pca_start(X, 2)
        p, i, x, _, _ = ur.fuzzy_graph(idx, dist)
        t_seq = []
        for seed in SEEDS:
            t0 = time.time()
            Y = ur.sequential_layout(p, i, x, Y0, A, B, EPOCHS, 1.0, NEG, seed)
            t_seq.append(ur.trustworthiness(X, Y, TRUST_K))
            print(name, "seed", seed, "T", t_seq[-1], "%.0f s" % (time.time() - t0), flush=True)
        out.update({name + "_X": X, name + "_labels": labels.astype(np.int32), name + "_idx": idx, name + "_dist": dist,
                    name + "_Y0": Y0, name + "_T_start": np.array(ur.trustworthiness(X, Y0, TRUST_K)),
                    name + "_T_seq": np.array(t_seq)})
        print(name, "T_start", float(out[name + "_T_start"]), "sequential", min(t_seq), "to", max(t_seq), flush=True)
    np.savez_compressed(os.path.join(HERE, "umap_fixtures.npz"), **out)


if __name__ == "__main__":
    main()
