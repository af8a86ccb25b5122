"""The numpy restatement of the model error (tests/evaluate_restatement.py) against the oracle: ora.mse_test with
inv_density = 1 draws every entry (rand % 1 == 0, src/singlet.cpp:92-95, 536-568), so it IS the full-matrix MSE in the
reference's own arithmetic -- per cell a sequential sum over the m genes divided by m, then the sum over the cells divided
by n."""
import numpy as np
import pytest

import evaluate_restatement as er

U = er.U
SHAPES = [(300, 1000, 8, 20), (257, 700, 50, 20), (130, 900, 70, 4), (64, 65, 1, 3), (500, 640, 130, 20)]


@pytest.fixture(scope="module")
def fits(ora):
    """The factors after four oracle c_nmf iterations from synth_winit, once per shape: (A, D, w m x k, d, h k x n)."""
    out = {}
    for m, n, k, inv in SHAPES:
        A = ora.synth_csc(m, n, inv)
        r = ora.c_nmf(A, A.t(), 0.0, 4, 0.01, 0.01, 0.0, 0.0, 0, ora.synth_winit(k, m))
        out[(m, n, k, inv)] = (A, er.dense_of(A), r["w"], r["d"], np.ascontiguousarray(r["h"].T))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_longdouble_restatement_is_the_oracles_full_matrix_mse(ora, fits, shape):
    """|oracle - exact| <= (m + n + 2 k + 8) 2^-53 sum_ij (|A_ij| + sum_f |w d h|)^2 / (m n): every squared residual carries
    (2 k + 5) roundings of its k-term product sum, subtraction and square relative to (|a| + reconstruction)^2, the cell's
    sequential sum m more, its division one, the sum over the cells n, the last division one."""
    m, n, k, inv = shape
    A, D, w, d, h = fits[shape]
    ld = er.losses_longdouble(D, w, d, h)
    got = ora.mse_test(A, w, d, np.ascontiguousarray(h.T), 12345, 1)
    exact = ld["sse"] / (np.longdouble(m) * n)
    bound = (m + n + 2 * k + 8) * U * ld["cell_abs"].sum() / (np.longdouble(m) * n)
    print("shape", shape, "oracle", got, "rel. diff", float(abs(got - exact) / exact), "bound / mse", float(bound / exact))
    assert abs(np.longdouble(got) - exact) <= bound
    # the seed is irrelevant when everything is drawn
    assert ora.mse_test(A, w, d, np.ascontiguousarray(h.T), 7, 1) == got
    # both sides of the restatement sum the same residuals
    assert abs(ld["gene"].sum() - ld["sse"]) <= (m + n) * np.finfo(np.longdouble).eps * ld["sse"]
    assert ld["cell"].shape == (n,) and ld["gene"].shape == (m,)
    assert np.all(ld["cell"] <= ld["cell_abs"]) and np.all(ld["gene"] <= ld["gene_abs"])


@pytest.mark.parametrize("shape", SHAPES)
def test_float64_sparse_identity_stays_within_the_device_bound(fits, shape):
    """The identity ||a||^2 - 2 x . b + x^T G x in plain float64 against the long-double definition, held to the bound the
    device tests use: |err| <= 4 gamma A_j, gamma = (max column nnz + m + k^2 + 4) 2^-53 (n for m on the gene side)."""
    m, n, k, inv = shape
    A, D, w, d, h = fits[shape]
    ld = er.losses_longdouble(D, w, d, h)
    cell, gene = er.identity_float64(D, w, d, h)
    g_cell = er.gamma(int((D != 0).sum(axis=0).max()), m, k)
    g_gene = er.gamma(int((D != 0).sum(axis=1).max()), n, k)
    assert np.all(np.abs(cell - ld["cell"]) <= 4 * g_cell * ld["cell_abs"])
    assert np.all(np.abs(gene - ld["gene"]) <= 4 * g_gene * ld["gene_abs"])


def test_int64_form_is_exact_and_agrees_with_the_longdouble_form():
    rng = np.random.default_rng(5)
    m, n, k = 37, 53, 9
    D = rng.integers(0, 8, (m, n)) * (rng.random((m, n)) < 0.3)
    w, h, d = rng.integers(0, 4, (m, k)), rng.integers(0, 4, (k, n)), rng.integers(1, 3, k)
    cell, gene, sse = er.losses_int64(D, w, d, h)
    assert cell.dtype == np.int64 and cell.sum() == gene.sum() == sse
    # by hand, entry by entry
    want = np.zeros((m, n), dtype=np.int64)
    for i in range(m):
        for j in range(n):
            want[i, j] = (int(D[i, j]) - sum(int(w[i, f]) * int(d[f]) * int(h[f, j]) for f in range(k))) ** 2
    assert np.array_equal(cell, want.sum(axis=0)) and np.array_equal(gene, want.sum(axis=1))
    ld = er.losses_longdouble(D, w, d, h)
    assert np.array_equal(ld["cell"], cell.astype(np.longdouble)) and np.array_equal(ld["gene"], gene.astype(np.longdouble))
    assert np.array_equal(np.array(er.identity_float64(D, w, d, h)[0]), cell.astype(np.float64))
    with pytest.raises(AssertionError):
        er.losses_int64(D + 0.5, w, d, h)
