"""The planted fixture of the doublet tests: counts with known doublets, from one fixed seed.

600 genes, 4 cell types.  A shared gamma(2, 1) base profile; type t multiplies its own block of 100 genes (genes 100 t ..
100 t + 99) by 6.  A cell of type t at depth D = 1500 x lognormal(0, 0.25) has Poisson counts with mean D x profile_t /
sum(profile_t).  1080 singlets (270 per type) and 120 true doublets, each the sum of two FRESH cells (not among the singlets)
of two different types.  The columns are shuffled.  Dense in, CSC out: the matrix is small."""
import numpy as np

SEED = 20191
N_GENES, N_TYPES, BLOCK, FOLD = 600, 4, 100, 6.0
N_SINGLETS, N_DOUBLETS = 1080, 120
DEPTH, DEPTH_SIGMA = 1500.0, 0.25
_CACHE = {}


def _cells(rng, profiles, types):
    depth = DEPTH * rng.lognormal(0.0, DEPTH_SIGMA, size=types.shape[0])
    return rng.poisson(profiles[:, types] * depth[None, :]).astype(np.float64)


def planted():
    """{"dense" (genes x cells counts), "x", "i", "p" (its CSC slots, int32 offsets), "is_doublet" (bool per cell), "types"
    (the type of a singlet, -1 for a doublet)}; computed once, never written to."""
    if "fx" in _CACHE:
        return _CACHE["fx"]
    rng = np.random.default_rng(SEED)
    base = rng.gamma(2.0, 1.0, size=N_GENES)
    profiles = np.repeat(base[:, None], N_TYPES, axis=1)
    for t in range(N_TYPES):
        profiles[BLOCK * t:BLOCK * (t + 1), t] *= FOLD
    profiles /= profiles.sum(axis=0, keepdims=True)
    st = np.repeat(np.arange(N_TYPES), N_SINGLETS // N_TYPES)
    singles = _cells(rng, profiles, st)
    ta = rng.integers(0, N_TYPES, size=N_DOUBLETS)
    tb = (ta + 1 + rng.integers(0, N_TYPES - 1, size=N_DOUBLETS)) % N_TYPES
    doubles = _cells(rng, profiles, ta) + _cells(rng, profiles, tb)
    dense = np.concatenate([singles, doubles], axis=1)
    types = np.concatenate([st, np.full(N_DOUBLETS, -1)])
    perm = rng.permutation(dense.shape[1])
    dense, types = np.ascontiguousarray(dense[:, perm]), types[perm]
    x, i, p = dense_to_csc(dense)
    for a in (dense, types, x, i, p):
        a.setflags(write=False)
    _CACHE["fx"] = {"dense": dense, "x": x, "i": i, "p": p, "is_doublet": types < 0, "types": types}
    return _CACHE["fx"]


def dense_to_csc(D):
    """(x, i, p) of the non-zero entries of D, columns in order, rows ascending; p int32."""
    nz = D.T != 0
    cols, rows = np.nonzero(nz)
    p = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int32)
    return np.ascontiguousarray(D.T[nz], dtype=np.float64), rows.astype(np.int32), p
