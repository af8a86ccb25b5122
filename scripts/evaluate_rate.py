#!/usr/bin/env python3
"""Time Context.evaluate against one ALS iteration on the same resident matrix.  Writes one JSON line to
profiles/evaluate_rate.json (or the path in EVAL_RATE_OUT) and prints it.

On sgl_synth_csc 30 000 genes at 5 %, k = 50, at config 3's 1 000 000 cells and at the 125 000 cells of one rank of an
8-GPU team: two warm-up iterations, then REPEATS timed iterations (wall clock and the phases bench.py prints), then one
warm-up evaluation and REPEATS timed ones with both sides (wall clock of the whole call -- scratch allocation, kernels,
the losses back on the host -- and the rhs_h / rhs_w / gram phases its accumulate and Gram passes are booked under), and
the same for the cell side alone (sse only).  The factors are compared before and after: the evaluations must not move them.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.environ.get("EVAL_RATE_OUT", os.path.join(ROOT, "profiles", "evaluate_rate.json"))
GENES, K, REPEATS = 30000, 50, 5
SIZES = [int(v) for v in os.environ.get("EVAL_RATE_CELLS", "1000000,125000").split(",")]


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v)}


def phases(t):
    return {name: float(val[0]) for name, val in t.items() if val[0] > 0}


def measure(sa, cells):
    res = {"cells": cells}
    with sa.Context(0) as c:
        c.synth(GENES, cells, 20)
        res["nnz"] = c.dims()[2]
        c.fit_init(K)
        c.timing_enable(True)
        for _ in range(2):
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        it_wall, it_ph = [], []
        for _ in range(REPEATS):
            c.timing_get(reset=True)
            t0 = time.perf_counter()
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
            it_wall.append(1e3 * (time.perf_counter() - t0))
            it_ph.append(phases(c.timing_get(reset=True)))
        before = c.get_factors()
        for name, args in (("both_sides", (True, True)), ("cell_side_sse_only", (False, False))):
            wall, ph = [], []
            for rep in range(REPEATS + 1):
                c.timing_get(reset=True)
                t0 = time.perf_counter()
                out = c.evaluate(*args)
                t1 = time.perf_counter()
                if rep:
                    wall.append(1e3 * (t1 - t0))
                    ph.append(phases(c.timing_get(reset=True)))
            res["evaluate_%s_wall_ms" % name] = stats(wall)
            res["evaluate_%s_phase_ms" % name] = {k: stats([p.get(k, 0.0) for p in ph]) for k in sorted(set().union(*ph))}
            res["mse"] = out["mse"]
        after = c.get_factors()
        res["factors_untouched"] = bool(all(np.array_equal(a, b) for a, b in zip(before, after)))
    res["iteration_wall_ms"] = stats(it_wall)
    res["iteration_phase_ms"] = {k: stats([p.get(k, 0.0) for p in it_ph]) for k in sorted(set().union(*it_ph))}
    res["evaluate_over_iteration"] = res["evaluate_both_sides_wall_ms"]["median"] / res["iteration_wall_ms"]["median"]
    return res


def main():
    import singlet_amd as sa
    res = {"genes": GENES, "k": K, "repeats": REPEATS, "sizes": [measure(sa, n) for n in SIZES]}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
