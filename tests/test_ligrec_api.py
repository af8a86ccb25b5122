"""The user-level ligrec() on the device: pairs by gene names, from a TSV file, dropped and refused names, everything
find_all_markers takes as the matrix, and the planted fixture through the public call, equal to the restatement's result."""
import numpy as np
import pytest

import ligrec_restatement as lr
import planted_ligrec as pl
from test_ligrec_restatement import planted_reference

pytestmark = pytest.mark.gpu
KEYS = ("means", "p", "padj", "expressed", "pairs", "dropped", "n_ge", "class_sizes")


def the_matrix(sa, names=True):
    x, i, p, lab = pl.matrix(0)
    return sa.dgCMatrix(x, i, p, (pl.N_GENES, pl.N_CELLS), (pl.NAMES if names else None, None)), lab


def assert_is_the_restatement(out, want, pairs=pl.PAIRS):
    assert sorted(out) == sorted(KEYS) and out["pairs"] == list(pairs)
    assert np.array_equal(out["means"], want["score"]) and np.array_equal(out["n_ge"], want["n_ge"])
    assert np.array_equal(out["p"], want["p"], equal_nan=True) and np.array_equal(out["padj"], want["padj"], equal_nan=True)
    assert out["class_sizes"].tolist() == [80] * 4 and out["expressed"].shape == out["p"].shape and out["expressed"].dtype == bool
    assert np.array_equal(out["expressed"], ~np.isnan(out["p"]))


@pytest.mark.parametrize("seed", [0, 7])
def test_planted_fixture_through_the_public_call_equals_the_restatement(sa, seed):
    want = planted_reference(seed)[7]
    A, lab = the_matrix(sa)
    out = sa.ligrec(A, lab, pl.PAIRS, nperm=pl.NPERM, seed=seed)                  # the names are the row names of A
    assert_is_the_restatement(out, want)
    pl.planted_claims(out)
    assert out["dropped"] == [] and out["means"].shape == (9, 4, 4)
    if seed == 0:
        assert_is_the_restatement(sa.ligrec(A, lab, pl.PAIRS, nperm=pl.NPERM, seed=seed, batch=7), want)


def test_names_files_rows_and_every_kind_of_matrix(sa, tmp_path):
    want = planted_reference(0)[7]
    A, lab = the_matrix(sa)
    bare, _ = the_matrix(sa, names=False)
    # a TSV file
    path = tmp_path / "pairs.tsv"
    path.write_text("# ligand\treceptor\n" + "".join("%s\t%s\n" % pair for pair in pl.PAIRS))
    assert_is_the_restatement(sa.ligrec(A, lab, str(path), nperm=pl.NPERM), want)
    # gene_names given, and rows as integers when there are none
    assert_is_the_restatement(sa.ligrec(bare, lab, pl.PAIRS, gene_names=pl.NAMES, nperm=pl.NPERM), want)
    index = {name: g for g, name in enumerate(pl.NAMES)}
    rows = [(index[a], index[b]) for a, b in pl.PAIRS]
    assert_is_the_restatement(sa.ligrec(bare, lab, rows, nperm=pl.NPERM), want, rows)
    # a SciPy matrix and a Context that holds the matrix
    assert_is_the_restatement(sa.ligrec(bare.to_scipy(), lab, rows, nperm=pl.NPERM), want, rows)
    with sa.Context(0) as c:
        c.upload(bare, None)
        assert_is_the_restatement(sa.ligrec(c, lab, pl.PAIRS, gene_names=pl.NAMES, nperm=pl.NPERM), want)
        assert c.ligrec_info()["path"] == 1 and c.ligrec_info()["vectors_per_wave"] == 64 and c.dims()[:2] == (pl.N_GENES, pl.N_CELLS)
    assert_is_the_restatement(sa.ligrec(sa.native(bare.to_scipy()), lab, rows, nperm=pl.NPERM), want, rows)
    # names that are not in the matrix: dropped on request, otherwise refused
    more = [("LIG", "REC"), ("NOPE", "REC"), ("G02", "G03"), ("G04", "ALSO_NOT")]
    out = sa.ligrec(A, lab, more, nperm=pl.NPERM, missing="skip")
    assert out["pairs"] == [("LIG", "REC"), ("G02", "G03")] and out["dropped"] == [("NOPE", "REC"), ("G04", "ALSO_NOT")]
    assert np.array_equal(out["means"], want["score"][:2]) and np.array_equal(out["n_ge"], want["n_ge"][:2])
    with pytest.raises(ValueError, match="'NOPE' of the pair"):
        sa.ligrec(A, lab, more, nperm=pl.NPERM)
    # the adjustment per interaction, and the threshold's mask
    per = sa.ligrec(A, lab, pl.PAIRS, nperm=pl.NPERM, per_interaction=True)
    ref = lr.stats(pl.NPERM, want["group_n"], want["nz"], planted_reference(0)[5], planted_reference(0)[6], want["n_ge"], 0.01, True)
    assert np.array_equal(per["p"], want["p"]) and np.array_equal(per["padj"], ref["padj"], equal_nan=True)
    assert not np.array_equal(per["padj"], want["padj"])
    strict = sa.ligrec(A, lab, pl.PAIRS, nperm=pl.NPERM, threshold=0.5)
    assert np.isnan(strict["p"][0, 1, 0]) and strict["p"][0, 0, 1] == want["p"][0, 0, 1] and not strict["expressed"][0, 1, 0]

