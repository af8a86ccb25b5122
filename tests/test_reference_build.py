"""The CPU oracle (oracle/singlet_oracle.c) and the numpy restatements under tests/ held to a BUILD OF THE REFERENCE'S OWN
STATEMENTS: oracle/make_ref.sh cuts the ALS functions out of the reference tree at build time and compiles them against
oracle/standin/ (DESIGN.md "Oracle status").  Two ways, over the case list of tests/als_ref_cases.py:

  * always, against tests/golden/als_ref.npz, the outputs of that build stored by tests/golden/make_als_ref.py;
  * live, against oracle/_ref/libals_ref.so, wherever it exists -- which it must wherever the reference tree does.

Bounds (none chosen from what the oracle gives): integer and structural outputs exactly; floating-point outputs at the
project's parity bar, 1e-9 relative Frobenius with identical NaN / Inf / zero patterns, on the cases the fixture admits
(the reference build against its own second variant within 1e-12: make_als_ref.py).  On top of that the oracle is
expected to equal variant A BIT FOR BIT, because both sum in the same order (NOT_BITWISE below would list an exception).
"""
import os

import numpy as np
import pytest

import als_ref_cases as rc
from oracle import reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "als_ref.npz")
REFERENCE_TREE = os.environ.get("SINGLET_REFERENCE", "/root/reference")
PARITY = 1e-9       # DESIGN.md "Parity bar"
ADMIT = 1e-12       # make_als_ref.py: variant A against variant B

CASES = rc.cases()

# The cases the fixture admits (make_als_ref.py drops a case whose discrete events the reference build's two variants
# decide differently; test_fixture_covers_the_case_list keeps the account of them).
_admitted = set(np.load(GOLD)["admitted"].tolist())
ADMITTED = [c for c in CASES if rc.case_id(c) in _admitted]

# Entries where the oracle side is NOT expected to give variant A's bits.  None: the C oracle and the numpy restatements
# (c_gcnmf from the oracle's pieces, spatial_graph and the row-wise compression element by element) sum in variant A's
# order, and every entry is asserted bit for bit.  An exception would be written down here, with its reason.
NOT_BITWISE = set()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _check(case, got, ref_of, bitwise):
    """got: outputs of the oracle side; ref_of(key) -> (distance, structure equal, bits equal or None)"""
    for key, a in got.items():
        dist, same, bits = ref_of(key, a)
        if rc.is_exact(key):
            assert same, (rc.case_id(case), key, a)
            continue
        assert same, "%s %s: NaN / Inf / zero pattern differs from the reference build" % (rc.case_id(case), key)
        assert dist <= PARITY, "%s %s: %.3e from the reference build" % (rc.case_id(case), key, dist)
        if bitwise and bits is not None:
            assert bits, "%s %s: within %.1e of the reference build but not its bits" % (rc.case_id(case), key, dist)


def test_fixture_covers_the_case_list(gold):
    """Every case of the list is in the fixture, admitted or dropped; at most one in twenty is dropped; every entry
    point and every listed rank keeps an admitted case; every stored spread is within the admission bound."""
    admitted, dropped = set(gold["admitted"].tolist()), set(gold["dropped"].tolist())
    ids = [rc.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert set(ids) == admitted | dropped and not admitted & dropped
    assert len(dropped) * 20 <= len(ids)
    for entry in set(c[0] for c in CASES):
        assert any(i.startswith(entry + "-") for i in admitted), entry
    for entry, ranks in (("c_nmf", rc.NMF_RANKS), ("c_ard_nmf", rc.ARD_RANKS)):
        for k in ranks:
            assert any(c[0] == entry and c[2].get("k") == k and rc.case_id(c) in admitted for c in CASES), (entry, k)
    spreads = [float(v) for key, v in gold.items() if key.endswith("@spread")]
    assert spreads and max(spreads) <= ADMIT


def test_reference_libraries_are_built_where_the_reference_tree_is():
    """A missing library next to the reference tree is a failure of build() (oracle/make_ref.sh), not a skip."""
    if not os.path.exists(os.path.join(REFERENCE_TREE, "src", "singlet.cpp")):
        pytest.skip("no reference tree here: the fixture stands in")
    assert reference.available("a") and reference.available("b"), "run oracle/make_ref.sh (build() does)"


@pytest.mark.parametrize("case", ADMITTED, ids=rc.case_id)
def test_oracle_against_the_stored_reference_build(ora, gold, case):
    cid = rc.case_id(case)
    got = rc.run(case, ora, ora)
    assert set(got) == set(k.split("/")[1].split("@")[0] for k in gold if k.startswith(cid + "/"))

    def ref_of(key, a):
        dist, same = rc.against_stored(cid, key, a, gold)
        full = "%s/%s" % (cid, key)
        if full in gold:
            bits = rc.same_bits(a, gold[full])
        else:
            bits = rc.same_bits(np.ascontiguousarray(a, dtype=np.float64).ravel()[::int(gold[full + "@meta"][1])], gold[full + "@sample"])
        return dist, same, bits
    _check(case, got, ref_of, case[0] not in NOT_BITWISE)


@pytest.mark.parametrize("case", ADMITTED, ids=rc.case_id)
def test_oracle_against_the_live_reference_build(ora, case):
    if not reference.available("a"):
        pytest.skip("oracle/_ref/libals_ref.so is not built here")
    ref = rc.run(case, reference.variant("a"), ora)
    got = rc.run(case, ora, ora)
    assert set(got) == set(ref)

    def ref_of(key, a):
        b = ref[key]
        if rc.is_exact(key):
            same = np.asarray(a).shape == np.asarray(b).shape and np.array_equal(a, b)
            return 0.0, same, None
        return rc.rel(a, b), rc.same_structure(a, b, key), rc.same_bits(a, b)
    _check(case, got, ref_of, case[0] not in NOT_BITWISE)


def test_live_reference_build_reproduces_the_fixture(gold):
    """The libraries built here give what the fixture stores (same cut, same stand-in, same flags): bit for bit."""
    if not reference.available("a"):
        pytest.skip("oracle/_ref/libals_ref.so is not built here")
    from oracle import oracle as ora
    ora.build()
    a = reference.variant("a")
    for case in CASES:
        cid = rc.case_id(case)
        if case[0] not in ("nnls", "scale_cor", "predict_mask", "c_linked_nmf", "c_ard_nmf_sparse_list", "c_gcnmf") or cid not in gold["admitted"].tolist():
            continue
        for key, arr in rc.run(case, a, ora).items():
            dist, same = rc.against_stored(cid, key, arr, gold)
            assert same and dist == 0.0, (cid, key, dist)


def test_variant_b_is_the_other_arithmetic(ora):
    """Variant B is a different summation order of the same text: it differs from A in the last bits (else the spread
    measures nothing) and agrees within the admission bound."""
    if not (reference.available("a") and reference.available("b")):
        pytest.skip("oracle/_ref/libals_ref*.so are not built here")
    case = next(c for c in CASES if rc.case_id(c) == "c_nmf-k30")
    ra, rb = rc.run(case, reference.variant("a"), ora), rc.run(case, reference.variant("b"), ora)
    assert not np.array_equal(ra["w"], rb["w"])
    for key in ("w", "d", "h"):
        assert rc.rel(rb[key], ra[key]) <= ADMIT and rc.same_structure(ra[key], rb[key], key)
    assert np.array_equal(ra["n_iter"], rb["n_iter"])


def test_reference_refuses_nothing_silently_in_the_rowwise_compression(ora):
    """Where the bin size does not divide the row count and the tail rows hold entries, the reference indexes outside
    its result (R does not check); the stand-in's matrix does, and the binding reports None instead of a value.  The
    restatement's rule for that case (tail rows left out) is this build's, not the reference's."""
    if not reference.available("a"):
        pytest.skip("oracle/_ref/libals_ref.so is not built here")
    a = reference.variant("a")
    A = rc.ragged(ora, 123, 20, 3)
    assert (A.i >= 119).any()
    assert a.rowwise_compress_sparse(A, 7) is None
    assert a.rowwise_compress_dense(A.to_dense(), 7) is None
    assert a.rowwise_compress_sparse(A, 3) is not None


def test_spatial_graph_on_a_non_finite_coordinate_is_where_this_build_refuses():
    """A point with a NaN coordinate keeps nothing, not even itself: its column of zeros is divided by its sum 0, and the
    reference stores max_k NaN entries of row 0 (include/singlet_hip.h says so of the reference and refuses the input;
    the restatement asserts finite coordinates).  Shown on the reference build."""
    if not reference.available("a"):
        pytest.skip("oracle/_ref/libals_ref.so is not built here")
    p, i, x = reference.variant("a").spatial_graph([0.0, 1.0, np.nan, 3.0], np.zeros(4), 1.5, 3)
    assert p.tolist() == [0, 2, 4, 7, 8]
    assert i[4:7].tolist() == [0, 0, 0] and np.isnan(x[4:7]).all() and np.isfinite(np.delete(x, [4, 5, 6])).all()


def test_the_sweep_cap_is_reached_in_the_nnls_cases(ora):
    """The case list must reach the 100-sweep cap and the clamp: of the 300 columns at k = 100, some run all 100 sweeps
    (tests/test_gpu_ops.py::test_nnls counts 17), and solutions hold exact zeros next to warm-started coordinates."""
    F, B, X0 = rc.nnls_inputs(100)
    G = ora.aat(F)
    sweeps = [ora.nnls(G, B[c], X0[c], 0.01, 0.02)[2] for c in range(B.shape[0])]
    assert sum(s == 100 for s in sweeps) >= 10 and min(sweeps) < 100
    x = np.array([ora.nnls(G, B[c], X0[c], 0.01, 0.02)[0] for c in range(40)])
    assert ((x == 0) & (X0[:40] > 0)).any() and ((x == 0) & (X0[:40] == 0)).any()
