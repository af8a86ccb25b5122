#!/usr/bin/env python3
"""Time the five stages of the gene set enrichment test (sgl_c_gsea: rankings, observed scores, null sample, null scores,
tallies) and the whole call.  Writes one JSON line to profiles/gsea_rate.json (or the path in GSEA_RATE_OUT) and prints it.

  pbmc3k shape   m = 13 714 genes, k = 15 factors, P = 5 000 sets of sizes 11 to 499, nperm = 1 000
  the same with nperm = 10 000
  large          m = 30 000, k = 50, P = 15 000, nperm = 1 000
The loadings are synthetic (uniform, 65 % zeros, as an L1 fit leaves them), the sets uniform draws: the times depend on the
shapes and the size table alone.  After one warm-up call, REPEATS timed calls: the stages by hipEvent (the library's own
events around every stage of every batch, sgl_c_gsea's stage_ms) and the whole call by the wall clock (validation, uploads,
context, kernels, the host's statistics).  Beside them the host time of the vectorised numpy restatement
(tests/gsea_restatement.py) on the smallest shape, the only baseline at hand: its null scores are timed on one factor and
every tenth size and scaled to all, the rest in full.  No time is a pass condition."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.environ.get("GSEA_RATE_OUT", os.path.join(ROOT, "profiles", "gsea_rate.json"))
REPEATS = int(os.environ.get("GSEA_RATE_REPEATS", "3"))
STAGES = ("rankings", "observed", "null_sample", "null_scores", "tallies")
SHAPES = (("pbmc3k_shape", 13714, 15, 5000, 1000), ("pbmc3k_shape_nperm_10000", 13714, 15, 5000, 10000), ("large", 30000, 50, 15000, 1000))


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def inputs(m, k, P, seed):
    rng = np.random.default_rng(seed)
    w = rng.random((m, k)) * (rng.random((m, k)) >= 0.65)
    sizes = rng.integers(11, 500, size=P)
    genes = np.concatenate([rng.choice(m, size=int(s), replace=False) for s in sizes]).astype(np.int32)
    return w, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), genes


def device(sa, w, ptr, genes, nperm):
    stage, wall, info = [], [], None
    for rep in range(REPEATS + 1):
        t0 = time.perf_counter()
        out = sa.c_gsea(w, ptr, genes, "pos", nperm, seed=1, timing=True)
        t1 = time.perf_counter()
        if rep:
            stage.append(out["stage_ms"].copy())
            wall.append(1e3 * (t1 - t0))
        info = out["info"]
        print("  call %d: %.1f ms, stages %s" % (rep, 1e3 * (t1 - t0), np.round(out["stage_ms"], 2)), file=sys.stderr, flush=True)
    res = {"info": info, "call_wall_ms": stats(wall), "stages_sum_ms": stats([s.sum() for s in stage])}
    for i, name in enumerate(STAGES):
        res[name + "_ms"] = stats([s[i] for s in stage])
    return res, out


def host(w, ptr, genes, nperm, got):
    import gsea_restatement as gr
    m, k = w.shape
    sizes = np.unique(np.diff(ptr))
    t0 = time.perf_counter()
    es = gr.observed(w, ptr, genes)[0]
    t1 = time.perf_counter()
    sample = gr.null_sample(1, 0, nperm, m, int(sizes[-1]))
    t2 = time.perf_counter()
    part = sizes[::10]
    null = gr.null_scores(w[:, :1], part, 0, 1, 0, nperm, sample=sample)
    t3 = time.perf_counter()
    assert np.array_equal(es.view(np.uint64), np.ascontiguousarray(got["es"]).view(np.uint64)), "the device's scores are not the restatement's"
    j = int(np.nonzero(np.diff(ptr) == part[0])[0][0])
    assert int((null[0, 0] >= es[j, 0]).sum()) == int(got["n_ge"][j, 0]), "the device's tally is not the restatement's"
    scale = k * sizes.size / part.size
    return {"observed_s": t1 - t0, "null_sample_s": t2 - t1, "null_scores_timed_s": t3 - t2, "null_scores_timed_sizes": int(part.size),
            "null_scores_timed_factors": 1, "null_scores_scaled_s": (t3 - t2) * scale,
            "total_scaled_s": (t1 - t0) + (t2 - t1) + (t3 - t2) * scale}


def main():
    import singlet_amd as sa
    res = {"repeats": REPEATS, "shapes": {}}
    for name, m, k, P, nperm in SHAPES:
        print("%s: m = %d, k = %d, P = %d, nperm = %d" % (name, m, k, P, nperm), file=sys.stderr, flush=True)
        w, ptr, genes = inputs(m, k, P, 7)
        r, out = device(sa, w, ptr, genes, nperm)
        r.update(m=m, k=k, sets=P, nperm=nperm)
        if name == "pbmc3k_shape":
            r["numpy_restatement"] = host(w, ptr, genes, nperm, out)
        res["shapes"][name] = r
    line = json.dumps(res)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
