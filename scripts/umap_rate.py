"""Rate of run_umap's stages (sgl_knn, sgl_c_fuzzy_graph, sgl_c_umap_layout) on synthetic cells -> one JSON document
(profiles/umap_rate.json).

    python scripts/umap_rate.py [out.json] [cells ...]

The cells are Gaussian blobs in a 20-dimensional embedding; 30 neighbours, 2 components, a and b of min_dist = 0.3, five
negative samples, PCA start.  Timed by wall clock around the one-shot calls (upload, validation, every epoch, download).  The
cost of one epoch is the difference of the whole layout and a layout of 1 epoch, over the other epochs (also with b = 1,
the instance without pow; the first launches of a call run slower than the later ones, so a short layout overstates it); it
is set against the bytes of one pass over the stored entries -- 12 per entry, plus the positions gathered by the terms of the
firing entries -- at the HBM rate.  The CPU column is the numpy restatement of one epoch (tests/umap_restatement.py).  No test asserts a time."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import singlet_amd as sa  # noqa: E402
import umap_restatement as ur  # noqa: E402

HBM_BYTES_PER_S = 8.0e12     # MI355X specification
K, DIM, NEG, SEED = 30, 2, 5, 42


def timed(fn, repeats=3):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return out, {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}


def cells(n):
    rng = np.random.default_rng(n)
    centres = rng.standard_normal((25, 20)) * 3.0
    return np.ascontiguousarray((centres[rng.integers(0, 25, n)] + rng.standard_normal((n, 20))).T)   # k x n


def measure(n):
    E = cells(n)
    a, b = sa.find_ab_params(1.0, 0.3)
    n_epochs = 500 if n <= 10000 else 200
    repeats = 3 if n <= 200000 else 1
    t0 = time.perf_counter()
    idx, dist = sa.knn(E, None, K)
    t_knn = 1e3 * (time.perf_counter() - t0)
    G, t_fuzzy = timed(lambda: sa.fuzzy_simplicial_set(idx, dist), repeats)
    info_fuzzy = sa.umap_info()
    Y0 = sa.api._umap_init(E, DIM, "pca", SEED)
    Y, t_whole = timed(lambda: sa.umap_layout(G, Y0, a, b, n_epochs, 1.0, NEG, SEED), repeats)
    info = sa.umap_info()
    _, t_1 = timed(lambda: sa.umap_layout(G, Y0, a, b, 1, 1.0, NEG, SEED), repeats)
    per_epoch = (t_whole["median"] - t_1["median"]) / (n_epochs - 1)
    _, b1_whole = timed(lambda: sa.umap_layout(G, Y0, a, 1.0, n_epochs, 1.0, NEG, SEED), repeats)     # b == 1: the instance without pow
    _, b1_1 = timed(lambda: sa.umap_layout(G, Y0, a, 1.0, 1, 1.0, NEG, SEED), repeats)
    per_epoch_b1 = (b1_whole["median"] - b1_1["median"]) / (n_epochs - 1)
    # firing entries of an average epoch: the sum of w / w_max over the entries that ever fire
    r = G.x / G.x.max()
    firing = float(r[r >= 1.0 / n_epochs].sum())
    bytes_pass = 12.0 * G.nnz + firing * (1 + NEG) * DIM * 8.0
    t0 = time.perf_counter()
    ur.epoch(G.p, G.i, G.x, Y0, a, b, n_epochs, 1.0, NEG, SEED, 1)
    t_numpy = 1e3 * (time.perf_counter() - t0)
    return {"cells": n, "neighbours": K, "entries": int(G.nnz), "entries_per_column": G.nnz / n, "n_epochs": n_epochs, "a": a, "b": b,
            "knn_ms": t_knn, "fuzzy_graph_ms": t_fuzzy, "merge_fallback_vertices": info_fuzzy["merge_fallback"],
            "layout_whole_call_ms": t_whole, "layout_1_epoch_ms": t_1, "per_epoch_ms": per_epoch,
            "layout_whole_call_without_pow_ms": b1_whole,
            "per_epoch_without_pow_ms": per_epoch_b1,
            "instance": info["instance"], "widest_column": info["widest_column"], "multi_chunk_vertices": info["multi_chunk"],
            "firing_entries_per_epoch": firing, "firing_share": firing / max(G.nnz, 1), "terms_per_epoch": firing * (1 + NEG),
            "bytes_of_one_pass": bytes_pass, "pass_at_hbm_rate_ms": 1e3 * bytes_pass / HBM_BYTES_PER_S,
            "share_of_hbm_rate": (1e3 * bytes_pass / HBM_BYTES_PER_S) / per_epoch if per_epoch > 0 else None,
            "ns_per_term": 1e6 * per_epoch / max(firing * (1 + NEG), 1.0), "numpy_restatement_epoch_1_ms": t_numpy,
            "finite": bool(np.isfinite(Y).all())}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "umap_rate.json")
    sizes = [int(v) for v in sys.argv[2:]] or [2700, 200000, 1000000]
    doc = {"what": "run_umap's stages on Gaussian blobs in 20 dimensions; wall clock around the one-shot calls, ms",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "runs": []}
    for n in sizes:
        doc["runs"].append(measure(n))
        print(json.dumps(doc["runs"][-1]), flush=True)
        with open(out, "w") as f:
            json.dump(doc, f)
    print("wrote", out)


if __name__ == "__main__":
    main()
