#!/usr/bin/env python3
"""Time the device passes of the factor annotation (Context.group_moments, Context.gene_group_moments) and the whole calls
(Context.annotate, Context.annotate_genes) beside their yardsticks from the same session.  Writes one JSON line to
profiles/annotate_rate.json (or the path in ANNOTATE_RATE_OUT) and prints it.

  config 3   sgl_synth_csc 30 000 genes x 1 000 000 cells at 5 %, LogNormalized; a rank-50 fit (one iteration, so that H holds
             numbers); 20 groups dealt out by a hash of the cell, one cell in 64 left out.
After one warm-up call each, REPEATS timed calls: the kernels by hipEvent (the "scale" phase, which nothing else of these calls
is booked under) and the whole call by the wall clock.
  embedding  group_means of the resident H (the sums pass alone) against group_moments (the sums pass, the k x G division and the
             residual pass): the residual pass is their difference, and reads what the sums pass reads.
  genes      the gene-mean pass of the variable features (8 bytes per stored entry) and op_marker_sums (identity) against
             gene_group_moments (the marker sums, then the residual pass): the residual pass is the difference, and does one
             butterfly per block where the marker sums do up to G.
With ANNOTATE_RATE_PARENT set to a built tree of the parent commit, the three yardsticks (group_means, the gene-mean pass,
op_marker_sums) are also timed with THAT tree's library, in a child process of the same session on the same matrix and labels
("parent_commit" in the result).  No time is a pass condition."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("ANNOTATE_RATE_TREE", ROOT))   # (the child process of the parent's yardsticks: that tree's package)
OUT = os.environ.get("ANNOTATE_RATE_OUT", os.path.join(ROOT, "profiles", "annotate_rate.json"))
GENES = int(os.environ.get("ANNOTATE_RATE_GENES", "30000"))
CELLS = int(os.environ.get("ANNOTATE_RATE_CELLS", "1000000"))
RANK = int(os.environ.get("ANNOTATE_RATE_RANK", "50"))
GROUPS = int(os.environ.get("ANNOTATE_RATE_GROUPS", "20"))
REPEATS = int(os.environ.get("ANNOTATE_RATE_REPEATS", "3"))


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def timed(c, fn):
    """(kernel ms by hipEvent, wall ms) of REPEATS calls of fn after one warm-up."""
    kern, wall = [], []
    for rep in range(REPEATS + 1):
        c.timing_get(reset=True)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if rep:
            wall.append(1e3 * (t1 - t0))
            kern.append(c.timing_get(reset=True)["scale"][0])
        print("  call %d: %.1f ms" % (rep, 1e3 * (t1 - t0)), file=sys.stderr, flush=True)
    return {"kernel_ms": stats(kern), "call_wall_ms": stats(wall)}


def stage(c):
    """The matrix, the fit and the labels; (labels, labels without -1)."""
    c.synth(GENES, CELLS, 20)
    c.log_normalize()
    c.fit_init(RANK)
    c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
    cell = np.arange(CELLS, dtype=np.uint64)
    h = (cell * np.uint64(2654435761)) >> np.uint64(7)
    labels = (h % np.uint64(GROUPS)).astype(np.int32)
    labels[(h >> np.uint64(9)) % np.uint64(64) == 0] = -1
    return labels, np.where(labels < 0, 0, labels).astype(np.int32)   # group_means takes no -1


def yardsticks_only():
    """The yardsticks alone, with whatever tree ANNOTATE_RATE_TREE names: one JSON line on stdout."""
    import singlet_amd as sa
    with sa.Context(0) as c:
        labels, groups_only = stage(c)
        c.timing_enable(True)
        res = {"tree_has_the_annotation_entries": "sgl_annotate" in sa._lib.SIGNATURES,
               "group_means": timed(c, lambda: c.group_means(groups_only, GROUPS)),
               "hvg_mean_pass": timed(c, c.op_gene_mean),
               "marker_sums_identity": timed(c, lambda: c.op_marker_sums(labels, GROUPS, "identity"))}
    print(json.dumps(res))


def main():
    if "--yardsticks-only" in sys.argv:
        return yardsticks_only()
    import singlet_amd as sa
    res = {"repeats": REPEATS}
    parent = os.environ.get("ANNOTATE_RATE_PARENT")
    if parent:   # first, and in a process of its own: one matrix of this size at a time
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--yardsticks-only"], env=dict(os.environ, ANNOTATE_RATE_TREE=parent),
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("the parent tree's yardsticks failed:\n" + r.stderr[-2000:])
        res["parent_commit"] = json.loads(r.stdout.strip().splitlines()[-1])
    with sa.Context(0) as c:
        labels, groups_only = stage(c)
        m, n, nnz = c.dims()
        res.update({"genes": m, "cells": n, "nnz": nnz, "rank": RANK, "groups": GROUPS, "cells_left_out": int((labels < 0).sum())})
        c.timing_enable(True)
        e = {"group_means": timed(c, lambda: c.group_means(groups_only, GROUPS)),
             "group_moments": timed(c, lambda: c.group_moments(labels, GROUPS)),
             "annotate_whole_call": timed(c, lambda: c.annotate(labels, GROUPS))}
        e["residual_pass_kernel_ms"] = e["group_moments"]["kernel_ms"]["median"] - e["group_means"]["kernel_ms"]["median"]
        e["residual_over_sums_pass"] = e["residual_pass_kernel_ms"] / e["group_means"]["kernel_ms"]["median"]
        e["h_bytes"] = 8 * RANK * n
        res["embedding"] = e
        g = {"hvg_mean_pass": timed(c, c.op_gene_mean),
             "marker_sums_identity": timed(c, lambda: c.op_marker_sums(labels, GROUPS, "identity")),
             "gene_group_moments": timed(c, lambda: c.gene_group_moments(labels, GROUPS))}
        g["residual_pass_kernel_ms"] = g["gene_group_moments"]["kernel_ms"]["median"] - g["marker_sums_identity"]["kernel_ms"]["median"]
        g["residual_over_marker_sums"] = g["residual_pass_kernel_ms"] / g["marker_sums_identity"]["kernel_ms"]["median"]
        g["residual_over_hvg_pass"] = g["residual_pass_kernel_ms"] / g["hvg_mean_pass"]["kernel_ms"]["median"]
        g["residual_entries_per_s"] = nnz / (1e-3 * g["residual_pass_kernel_ms"])
        t0 = time.perf_counter()
        out = c.annotate_genes(labels, GROUPS)
        g["annotate_genes_whole_call_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        g["rows_with_positive_lods"] = int((out["lods"] > 0).sum())
        res["genes_side"] = g
    line = json.dumps(res)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
