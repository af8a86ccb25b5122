#!/usr/bin/env python3
"""Generates tests/golden/als_ref.npz from the REFERENCE's own ALS functions.

oracle/make_ref.sh cuts the functions out of the reference tree at build time (git-ignored oracle/_ref/) and compiles
them twice against oracle/standin/: variant A (stand-in reductions ascending, no contraction) and variant B (descending,
contraction on).  This script runs both over the case list of tests/als_ref_cases.py and stores variant A's outputs
(small ones whole; large ones as a strided sample, their norm and a digest of their NaN / Inf / zero structure) and, per
floating-point output, `spread`: the relative Frobenius distance between A and B -- the measured size of what the
stand-in cannot pin (Eigen's own summation order and contraction).

A case is ADMITTED when A and B agree in every integer / structural output (iter vectors, iteration counts, NaN / Inf /
zero patterns, graph patterns) and every spread is <= 1e-12; only admitted cases are asserted by the tests.  A case
that is not admitted is one where a discrete event (a sweep cap, a clamp, a stop) is decided differently by the two
summation orders, which says nothing about the code under test.  At most one candidate in twenty may be dropped, and no
entry point may lose all its cases: the script fails otherwise.

Authoring container only (needs the reference tree); the committed fixture is data.  Prints the report that belongs
in the pull request description.
"""
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ADMIT = 1e-12


def main():
    subprocess.check_call(["sh", os.path.join(ROOT, "oracle", "make_ref.sh")])
    from oracle import oracle as ora, reference
    import als_ref_cases as rc
    ora.build()
    a, b = reference.variant("a"), reference.variant("b")
    store, admitted, dropped, by_entry = {}, [], [], {}
    for case in rc.cases():
        cid = rc.case_id(case)
        t0 = time.time()
        ra, rb = rc.run(case, a, ora), rc.run(case, b, ora)
        ok, spreads = True, {}
        for key in ra:
            if rc.is_exact(key):
                ok &= np.asarray(ra[key]).shape == np.asarray(rb[key]).shape and np.array_equal(ra[key], rb[key])
            else:
                same = np.asarray(ra[key]).shape == np.asarray(rb[key]).shape and rc.same_structure(ra[key], rb[key], key)
                ok &= same
                spreads[key] = rc.rel(rb[key], ra[key]) if same else float("inf")
                ok &= spreads[key] <= ADMIT
        by_entry.setdefault(case[0], []).append(ok)
        line = "%-42s %s  %5.1fs  %s" % (cid, "admitted" if ok else "DROPPED ", time.time() - t0,
                                        " ".join("%s=%.1e" % kv for kv in spreads.items()))
        print(line, flush=True)
        if not ok:
            dropped.append(cid)
            continue
        admitted.append(cid)
        rc.pack(cid, ra, store)
        for key, s in spreads.items():
            store["%s/%s@spread" % (cid, key)] = np.float64(s)
    total = len(admitted) + len(dropped)
    print("%d candidates, %d admitted, %d dropped: %s" % (total, len(admitted), len(dropped), dropped))
    worst = max(float(v) for k, v in store.items() if k.endswith("@spread"))
    print("largest spread among admitted cases: %.2e" % worst)
    assert len(dropped) * 20 <= total, "more than one candidate in twenty dropped"
    lost = [e for e, oks in by_entry.items() if not any(oks)]
    assert not lost, "entry points without an admitted case: %s" % lost
    for entry, ranks in (("c_nmf", rc.NMF_RANKS), ("c_ard_nmf", rc.ARD_RANKS)):
        lost_ranks = [k for k in ranks if not any(c.startswith("%s-k%d" % (entry, k)) and c.split("-k")[1].split("_")[0] == str(k)
                                                  for c in admitted)]
        assert not lost_ranks, "%s: listed ranks without an admitted case (add another input): %s" % (entry, lost_ranks)
    store["admitted"] = np.array(admitted)
    store["dropped"] = np.array(dropped, dtype="U64")
    path = os.path.join(HERE, "als_ref.npz")
    np.savez_compressed(path, **store)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    sys.exit(main())
