#!/usr/bin/env python3
"""How the presence of one cell type changes with the distance from another in a synthetic tissue (co_occurrence, ripley): two
cell types that share small clumps, a third that fills the tissue uniformly and a fourth that keeps a ring of a fixed radius
around every clump.  The co-occurrence score of the clumped pair must be above 1 at short distances and fall towards 1, the ring type
must peak against the clumped ones at the ring's radius, and the uniform type must have Ripley's L(r) close to r while the
clumped types sit far above it.  Makes no download.  Needs an MI355X.

  python examples/spatial_co_occurrence.py [cells] [intervals]        defaults: 40000, 25
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import singlet_amd as sa  # noqa: E402

n, T = (int(v) for v in sys.argv[1:3]) if len(sys.argv) >= 3 else (40000, 25)
rng = np.random.default_rng(0)
clumps, ring = 60, 0.04
centres = rng.random((clumps, 2)) * 0.9 + 0.05
per = n // (8 * clumps)
pts, lab = [], []
for cls in (0, 1):
    pts.append(np.repeat(centres, per, axis=0) + 0.006 * rng.standard_normal((clumps * per, 2)))
    lab.append(np.full(clumps * per, cls))
ang = rng.random(clumps * per) * 2 * np.pi
pts.append(np.repeat(centres, per, axis=0) + ring * np.stack([np.cos(ang), np.sin(ang)], axis=1) + 0.003 * rng.standard_normal((clumps * per, 2)))
lab.append(np.full(clumps * per, 3))
rest = n - 3 * clumps * per
pts.append(rng.random((rest, 2)))
lab.append(np.full(rest, 2))
xy, labels = np.concatenate(pts), np.concatenate(lab).astype(np.int32)
names = ["clump A", "clump B", "uniform", "ring"]
print("tissue: %d cells, class sizes %s" % (xy.shape[0], np.bincount(labels).tolist()))

r = np.linspace(0.0, 0.1, T + 1)
t0 = time.perf_counter()
res = sa.co_occurrence(labels, xy, interval=r)
t1 = time.perf_counter()
print("co_occurrence: %d ordered pairs within %.2f tallied into %d intervals in %.3f s (upload and host statistics included)"
      % (int(res["counts"].sum()), r[-1], T, t1 - t0))
occ = res["occ"]
mid = 0.5 * (r[1:] + r[:-1])
print("score of class b around clump A, by distance:")
print("%10s %s" % ("distance", " ".join("%9s" % s for s in names)))
for t in range(0, T, max(T // 8, 1)):
    print("%10.4f %s" % (mid[t], " ".join("%9.2f" % occ[0, b, t] for b in range(4))))
peak = int(np.nanargmax(occ[0, 3]))
print("clump B is enriched next to clump A: %s; the score falls with distance: %s; the ring type peaks at %.4f (planted %.2f): %s"
      % (occ[0, 1, 0] > 1.2, occ[0, 1, 0] > occ[0, 1, -1], mid[peak], ring, abs(mid[peak] - ring) < 0.01))

L = sa.ripley(labels, xy, mode="L", interval=r, area=1.0)
print("Ripley's L(r) - r at r = %.3f (no edge correction): %s" % (r[T // 2 + 1], " ".join("%s %+.4f" % (s, L[a, T // 2] - r[T // 2 + 1]) for a, s in enumerate(names))))
print("the uniform type is close to complete spatial randomness: %s; the clumped types are far above it: %s"
      % (bool(np.abs(L[2] - r[1:]).max() < 0.01), bool(L[0, T // 2] - r[T // 2 + 1] > 0.02)))

wide = sa.co_occurrence(labels, xy, interval=10)          # the default thresholds: up to half the diagonal, all pairs
print("default thresholds up to %.3f (all %d x %d pairs): score of clump B around clump A %.2f in the first interval, %.2f in the last"
      % (wide["interval"][-1], xy.shape[0], xy.shape[0], wide["occ"][0, 1, 0], wide["occ"][0, 1, -1]))
