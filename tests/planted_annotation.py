"""The planted embedding shared by tests/test_annotate_restatement.py (CPU: the restatement alone recovers the pairs) and
tests/test_gpu_annotate.py (the device does): H 12 x 3000 of non-negative noise, 4 groups, and three (factor, group) pairs
whose cells are shifted by 20 residual standard deviations."""
import numpy as np

K, N_CELLS, G = 12, 3000, 4
SEED = 20240611
PAIRS = ((0, 2), (1, 5), (3, 9))   # (group, factor)
SIGMA = 0.25
SHIFT = 20.0


def planted():
    """(H k x n, labels with a few cells left out, the planted (group, factor) pairs)."""
    rng = np.random.default_rng(SEED)
    labels = rng.integers(0, G, size=N_CELLS)
    labels[rng.random(N_CELLS) < 0.03] = -1
    H = 8.0 + SIGMA * rng.normal(size=(K, N_CELLS))
    for g, f in PAIRS:
        H[f, labels == g] += SHIFT * SIGMA
    return H, labels.astype(np.int32), PAIRS
