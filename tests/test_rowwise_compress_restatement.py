"""The two forms of tests/rowwise_compress_restatement.py agree bit for bit where the reference is defined (nrow % n == 0):
the literal transcription of the reference's loops (sparse and dense) and the vectorised running sum, on random matrices
with integer counts, empty and full columns, NaN, +-Inf and -0.0, and on hand-worked cases.  CPU only."""
import numpy as np
import pytest

import rowwise_compress_restatement as rr
from singlet_amd.sparse import dgCMatrix


def _random(rng, nrow, ncol, density, special=False, counts=False):
    D = np.where(rng.random((nrow, ncol)) < density, rng.standard_normal((nrow, ncol)) * 10.0 ** rng.integers(-3, 4, (nrow, ncol)), 0.0)
    if counts:
        D = np.where(D != 0, rng.integers(1, 50, (nrow, ncol)).astype(np.float64), 0.0)
    if ncol > 2:
        D[:, 0] = 0.0                                   # an empty column
        D[:, 1] = rng.integers(1, 9, nrow)             # a full column
    if special:
        flat = D.reshape(-1, order="F")
        pos = rng.choice(flat.size, min(flat.size, 12), replace=False)
        flat[pos] = np.array([np.nan, np.inf, -np.inf, -0.0] * 3)[:pos.size]
        D = flat.reshape(D.shape, order="F")
    return D


def _sparse(D, keep_neg_zero=True):
    """dgCMatrix of D storing every entry that is not +0.0 (so stored -0.0 entries survive)."""
    mask = (D != 0) | (np.signbit(D) & keep_neg_zero) | np.isnan(D)
    return _from_mask(D, mask)


def _from_mask(D, mask):
    nrow, ncol = D.shape
    cols = [np.nonzero(mask[:, j])[0] for j in range(ncol)]
    p = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int32)
    i = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    x = np.concatenate([D[c, j] for j, c in enumerate(cols)]) if cols else np.zeros(0)
    return dgCMatrix(x, i, p, (nrow, ncol))


@pytest.mark.parametrize("nrow,ncol,n", [(10, 4, 1), (10, 4, 2), (12, 5, 3), (21, 3, 7), (40, 6, 10), (128, 3, 64), (60, 4, 60)])
@pytest.mark.parametrize("special", [False, True])
def test_literal_and_vectorised_agree(nrow, ncol, n, special):
    rng = np.random.default_rng(nrow * 100 + ncol * 10 + n + special)
    D = _random(rng, nrow, ncol, 0.3, special)
    S = _sparse(D)
    ld, ls = rr.literal_dense(D, n), rr.literal_sparse(S, n)
    vd, vs = rr.vectorised_dense(D, n), rr.vectorised_sparse(S, n)
    assert rr.same_bits(ld, vd)
    assert rr.same_bits(ls, vs)
    assert rr.same_bits(ld, ls)          # sparse and densified: one result
    assert vd.flags.f_contiguous and vd.shape == (nrow // n, ncol)


def test_counts_are_exact_means():
    rng = np.random.default_rng(7)
    D = _random(rng, 100, 8, 0.2, counts=True)
    got = rr.vectorised_dense(D, 10)
    want = D.reshape(10, 10, 8, order="F").sum(axis=0) / 10.0   # integer sums are exact in any order
    assert rr.same_bits(got, want)


def test_hand_worked():
    D = np.array([[1.0, 0.0], [2.0, -0.0], [0.0, np.inf], [0.0, -np.inf], [1e308, 5.0], [1e308, 0.0]])
    got = rr.vectorised_dense(D, 2)
    assert got.shape == (3, 2)
    assert got[0, 0] == 1.5 and got[1, 0] == 0.0 and got[2, 0] == np.inf   # 1e308 + 1e308 overflows
    assert got[0, 1] == 0.0 and not np.signbit(got[0, 1])                  # +0.0 + -0.0 = +0.0
    assert np.isnan(got[1, 1])                                             # +Inf + -Inf
    assert got[2, 1] == 2.5
    assert rr.same_bits(rr.literal_dense(D, 2), got)
    assert rr.same_bits(rr.literal_sparse(_sparse(D), 2), got)


def test_order_is_sequential_not_pairwise():
    # 1 + 2^-53 + ... in row order: each 2^-53 is half an ulp of 1 and rounds away; summed first they would count
    col = np.array([1.0] + [2.0 ** -53] * 7)
    got = rr.vectorised_dense(col[:, None], 8)
    assert got[0, 0] == 1.0 / 8
    other = 0.0
    for v in col[::-1]:
        other += v
    assert other != 1.0 and got[0, 0] != other / 8


def test_true_division_not_reciprocal():
    # a sum s with s / 3 != s * (1 / 3)
    s = 5.0
    assert s / 3.0 != s * (1.0 / 3.0)
    D = np.array([[s], [0.0], [0.0]])
    assert rr.vectorised_dense(D, 3)[0, 0] == s / 3.0


def test_remainder_rows_are_left_out():
    rng = np.random.default_rng(3)
    D = _random(rng, 23, 4, 0.5)
    got = rr.vectorised_dense(D, 5)
    assert got.shape == (4, 4)
    D2 = D.copy()
    D2[20:, :] = 12345.0
    assert rr.same_bits(rr.vectorised_dense(D2, 5), got)
    assert rr.same_bits(rr.vectorised_sparse(_sparse(D), 5), got)
    assert rr.same_bits(rr.columns(_sparse(D), 5, [3, 0]), got[:, [3, 0]])


def test_n_above_nrow_is_empty():
    D = np.ones((4, 3))
    assert rr.vectorised_dense(D, 5).shape == (0, 3)
