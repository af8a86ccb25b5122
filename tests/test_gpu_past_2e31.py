"""Oracle parity past 2^31 and past 2^32 stored non-zeros: the sizes the chunk-list entry points (sgl_c_nmf_sparse_list,
sgl_upload_csc_list: 64-bit column pointers) are there for, and that one dgCMatrix cannot hold.

Past 2^31 (about 2.25e9 non-zeros, generated on the device): slices of h at the first cells, at the last ones and around
the cell whose entries in A straddle entry 2^31; whole gene columns of w for the first, last, heaviest, lightest genes
and the gene whose entries in t(A) straddle entry 2^31 -- against ora.predict / ora.predict_mask on the regenerated
slices (ora.synth_csc(cell0=...), ora.synth_gene_columns), as tests/test_gpu_fullsize_oracle.py does at 1.5e9.

Past 2^32 (about 4.3e9 non-zeros): ONE host chunk listed R times, uploaded with the transpose built on the device
(n_t_chunks = 0: the column-batched sort of kernels_transpose.hip).  Host memory stays at one chunk, and the repetition
checks every column without a full-size oracle: the plain CSC accumulate sums each cell's entries in row order, so its
right-hand sides of every copy equal copy 0's bit for bit; a gene's column of t(A) is the chunk's row tiled R times with
cell offsets.  The fit's LDS-tiled accumulate is NOT position-independent to the bit: its sliding-window layout places
each column by its non-zero count, next to a neighbour in that order, so a column's place -- and with it how its sum is
grouped -- depends on the other columns.  Measured on this matrix: a few dozen cells per copy differ from copy 0 in the
last bits (at most 3.5e-15 relative in the tiled right-hand sides; the plain ones are bit-equal).  The tiled h of the
copies is therefore held to rounding (1e-12), and to the oracle on slices.

Device memory in use is printed at the peaks (pytest -s shows it)."""
import ctypes

import numpy as np
import pytest

from conftest import rel_fro, same_zero_pattern, to_dgc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

GENES, INV = 30000, 20
L1 = 0.01
SEED, INV_MASK = 4711, 20
E31, E32 = 2 ** 31, 2 ** 32


def _release(sa):
    from singlet_amd import _lib
    _lib.check(_lib.load().sgl_cache_release())


def _mem(tag):
    """Device memory in use (hipMemGetInfo) and the part of it the library's pool keeps (sgl_pool_info)."""
    from singlet_amd import _lib
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    cached = ctypes.c_int64()
    _lib.check(_lib.load().sgl_pool_info(ctypes.byref(cached)))
    print("\n[mem] %-40s used %6.1f GB of %6.1f GB (pool cache %5.1f GB)"
          % (tag, (total.value - free.value) / 1e9, total.value / 1e9, cached.value / 1e9), flush=True)


def _straddle(counts, e):
    """Index of the column whose entries hold entry number e (0-based) of the matrix."""
    cum = np.cumsum(counts, dtype=np.int64)
    j = int(np.searchsorted(cum, e, side="right"))
    assert (cum[j - 1] if j else 0) <= e < cum[j]
    return j


def _assert_copies_equal(blocks, tol=None):
    """Every copy's block equals copy 0's: bit for bit (tol None), or to rounding with the same zero pattern."""
    for q in range(1, blocks.shape[0]):
        if tol is None:
            assert np.array_equal(blocks[q].view(np.uint64), blocks[0].view(np.uint64)), q
        else:
            assert rel_fro(blocks[q], blocks[0]) < tol, (q, rel_fro(blocks[q], blocks[0]))
            assert same_zero_pattern(blocks[q], blocks[0]), q


def _check_h_slices(H, slices, width, k, oracle_slice):
    for s0, local in slices:
        ref = oracle_slice(local, width, k)
        got = H[s0:s0 + width]
        assert rel_fro(got, ref) < 1e-9, (k, s0, rel_fro(got, ref))
        assert same_zero_pattern(got, ref), (k, s0)


def _check_scales_and_w(c, ora, H, W0, W_ref_fn, groups):
    """scale(h, d), the W-update on the whole gene columns of `groups`, scale(w, d) and tol = cor(w, w_it)
    (src/singlet.cpp:651-659) against the oracle, as the config-3 test checks them."""
    c.step_scale_h()
    _, dh, Hs = c.get_factors(w=False)
    d_host = H.sum(axis=0) + 1e-15
    assert rel_fro(dh, d_host) < 1e-12
    assert rel_fro(Hs[:4096], H[:4096] / d_host) < 1e-12 and rel_fro(Hs[-4096:], H[-4096:] / d_host) < 1e-12
    c.step_w(L1, 0.0)
    W1, _, _ = c.get_factors(h=False)
    for genes in groups:
        ref = W_ref_fn(genes, Hs)
        got = W1[genes]
        assert rel_fro(got, ref) < 1e-9, (genes, rel_fro(got, ref))
        assert same_zero_pattern(got, ref), genes
    tol = c.step_scale_w()
    W2, dw, _ = c.get_factors(h=False)
    Ws, d_ref = ora.scale(W1)
    assert rel_fro(dw, d_ref) < 1e-12 and rel_fro(W2, Ws) < 1e-12
    tol_ref = ora.cor(Ws, W0)
    assert abs(tol - tol_ref) <= 1e-8 * abs(tol_ref), (tol, tol_ref)


# ---- past 2^31: 30 000 x 1 500 000, generated on the device ----------------------------------------------------------

class TestPast2e31:
    CELLS = 1500000

    @pytest.fixture(scope="class")
    def big(self, sa):
        _release(sa)
        c = sa.Context(0)
        try:
            c.synth(GENES, self.CELLS, INV)
            _mem("2^31 leg: A and t(A) resident")
            yield c
        finally:
            c.close()
            _release(sa)

    def _cell_slices(self, c, width):
        j = _straddle(c.col_counts(0), E31)
        s = j - width // 2 - 3                                           # not aligned to a 64-column block
        return [(0, 0), (s, s), (self.CELLS - width, self.CELLS - width)]

    def _gene_groups(self, c):
        cnt = c.col_counts(1)
        assert cnt.shape == (GENES,) and int(cnt.sum()) == c.dims()[2]
        g31 = _straddle(cnt, E31)
        return [[0, 1, 2], [GENES - 2, GENES - 1], [int(np.argmax(cnt))], [int(np.argmin(cnt))], [g31]]

    def test_size(self, big):
        nr, nc, nnz = big.dims()
        assert (nr, nc) == (GENES, self.CELLS)
        assert nnz > E31 + 10 ** 8, nnz
        print("\n[nnz] 2^31 leg: %d non-zeros (%d x %d)" % (nnz, nr, nc))

    @pytest.mark.parametrize("k", [50, 20])
    def test_h_and_w_update_equal_the_oracle(self, big, ora, k):
        width = 512
        big.fit_init(k, None)
        W0 = ora.synth_winit(k, GENES)
        Wdev, _, _ = big.get_factors(h=False)
        assert np.array_equal(Wdev, W0)
        big.step_begin()
        big.step_h(L1, 0.0)
        _mem("2^31 leg: fit at k = %d, after the H-update" % k)
        _, _, H = big.get_factors(w=False, d=False)

        def h_ref(s0, width, k):
            return ora.predict(ora.synth_csc(GENES, width, INV, cell0=s0), W0, np.zeros((width, k)), L1, 0.0)

        _check_h_slices(H, self._cell_slices(big, width), width, k, h_ref)
        assert np.all(np.isfinite(H)) and np.all(H >= 0)

        def w_ref(genes, Hs):
            G = ora.synth_gene_columns(genes, self.CELLS, INV)
            assert np.array_equal(np.diff(G.p), big.col_counts(1)[genes])
            return ora.predict(G, Hs, W0[genes].copy(), L1, 0.0)

        _check_scales_and_w(big, ora, H, W0, w_ref, self._gene_groups(big))

    def test_masked_h_and_w_update_equal_the_oracle(self, big, ora):
        """predict_mask (src/singlet.cpp:436-466) at k = 50: the mask lists run to about 2.25e9 entries; the GLOBAL cell
        index goes into the hash (col_offset), the gene index on the W side (mask_t = true)."""
        k, width = 50, 256
        big.fit_init(k, None)
        W0 = ora.synth_winit(k, GENES)
        big.step_begin()
        big.step_h_masked(L1, 0.0, SEED, INV_MASK)
        _mem("2^31 leg: masked fit at k = 50, after the H-update")
        _, _, H = big.get_factors(w=False, d=False)
        for s0, _ in self._cell_slices(big, width):
            A_s = ora.synth_csc(GENES, width, INV, cell0=s0)
            ref = ora.predict_mask(A_s, SEED, INV_MASK, W0, np.zeros((width, k)), L1, 0.0, col_offset=s0)
            got = H[s0:s0 + width]
            assert rel_fro(got, ref) < 1e-9, (s0, rel_fro(got, ref))
            assert same_zero_pattern(got, ref), s0
        big.step_scale_h()
        _, _, Hs = big.get_factors(w=False, d=False)
        big.step_w_masked(L1, 0.0, SEED, INV_MASK)
        _mem("2^31 leg: masked fit at k = 50, after the W-update")
        W1, _, _ = big.get_factors(h=False)
        for genes in self._gene_groups(big):
            G = ora.synth_gene_columns(genes, self.CELLS, INV)
            ref = ora.predict_mask(G, SEED, INV_MASK, Hs, W0[genes].copy(), L1, 0.0, mask_t=True, col_offset=genes[0])
            got = W1[genes]
            assert rel_fro(got, ref) < 1e-9, (genes, rel_fro(got, ref))
            assert same_zero_pattern(got, ref), genes


# ---- past 2^32: one 30 000 x 100 000 chunk listed R times, t(A) built on the device ----------------------------------

NC = 100000


@pytest.fixture(scope="module")
def chunk(sa, ora):
    """The chunk (as a dgCMatrix, converted once) and R: copies enough for the total to pass 2^32 by a quarter chunk."""
    C = ora.synth_csc(GENES, NC, INV)
    R = E32 // C.nnz + 1
    if R * C.nnz - E32 < C.nnz // 4:
        R += 1
    for e in (E31, E32):                                                # the entries of interest lie inside a copy
        off = e % C.nnz
        assert off != 0
        lc = _straddle(np.diff(C.p), off)
        assert 256 <= lc < NC - 256, (e, lc)
    return C, to_dgc(sa, C), R


class TestPast2e32:
    @pytest.fixture(scope="class")
    def lst(self, sa, chunk):
        C, Cd, R = chunk
        _release(sa)
        c = sa.Context(0)
        try:
            c.upload_list(R * [Cd])
            _mem("2^32 leg: A and t(A) resident")
            yield c
        finally:
            c.close()
            _release(sa)

    def test_size_and_counts(self, lst, chunk):
        C, _, R = chunk
        nr, nc, nnz = lst.dims()
        assert (nr, nc, nnz) == (GENES, R * NC, R * C.nnz)
        assert nnz > E32 + C.nnz // 4, nnz
        print("\n[nnz] 2^32 leg: %d non-zeros (%d x %d, %d copies of a %d-entry chunk)" % (nnz, nr, nc, R, C.nnz))
        assert np.array_equal(lst.col_counts(0), np.tile(np.diff(C.p), R))
        assert np.array_equal(lst.col_counts(1), R * np.bincount(C.i, minlength=GENES))

    def test_plain_rhs_copies_bit_equal(self, lst, ora, chunk):
        """B = w A through the plain CSC accumulate (sgl_op_rhs which = 0) over all R * NC cells: every copy's block
        equals copy 0's bit for bit -- the 64-bit column pointers and entry offsets past 2^31 and 2^32 read the right
        entries -- and copy 0 equals the oracle's right-hand sides on slices."""
        C, _, R = chunk
        W0 = ora.synth_winit(10, GENES)
        B = lst.op_rhs(0, W0)
        _assert_copies_equal(B.reshape(R, NC, 10))
        for s0 in (0, NC // 2 + 17, NC - 256):
            ref = ora.rhs(ora.synth_csc(GENES, 256, INV, cell0=s0), W0)
            assert rel_fro(B[s0:s0 + 256], ref) < 1e-13, s0

    @pytest.mark.parametrize("k", [10, 50])
    def test_h_and_w_update(self, lst, ora, chunk, k):
        C, _, R = chunk
        width = 256
        lst.fit_init(k, None)
        W0 = ora.synth_winit(k, GENES)
        lst.step_begin()
        lst.step_h(L1, 0.0)
        _mem("2^32 leg: fit at k = %d, after the H-update" % k)
        _, _, H = lst.get_factors(w=False, d=False)
        _assert_copies_equal(H.reshape(R, NC, k), 1e-12)                  # every cell, every copy (tiled: to rounding)
        slices = [(0, 0), (NC // 2 + 17, NC // 2 + 17), (NC - width, NC - width)]
        for e in (E31, E32):                                              # the copies holding entries 2^31 and 2^32
            j = _straddle(lst.col_counts(0), e)
            s = j - width // 2
            slices.append((s, s % NC))
            assert s // NC == (s + width - 1) // NC

        def h_ref(s0, width, k):
            return ora.predict(ora.synth_csc(GENES, width, INV, cell0=s0), W0, np.zeros((width, k)), L1, 0.0)

        _check_h_slices(H, slices, width, k, h_ref)
        assert np.all(np.isfinite(H)) and np.all(H >= 0)

        cnt = np.bincount(C.i, minlength=GENES)

        def w_ref(genes, Hs):
            Gc = ora.synth_gene_columns(genes, NC, INV)                   # the genes' rows of the chunk
            xs, is_, p = [], [], [0]
            for b in range(len(genes)):
                s = slice(Gc.p[b], Gc.p[b + 1])
                is_.append(np.concatenate([Gc.i[s] + q * NC for q in range(R)]))
                xs.append(np.tile(Gc.x[s], R))
                p.append(p[-1] + is_[-1].size)
            G = ora.CSC(np.concatenate(xs), np.concatenate(is_), p, R * NC, len(genes))
            assert np.array_equal(np.diff(G.p), R * cnt[genes])
            return ora.predict(G, Hs, W0[genes].copy(), L1, 0.0)          # the Gram over all R * NC cells inside

        groups = [[0, 1, 2], [GENES - 2, GENES - 1], [int(np.argmax(cnt))], [int(np.argmin(cnt))]]
        _check_scales_and_w(lst, ora, H, W0, w_ref, groups)
        _mem("2^32 leg: fit at k = %d, after the W-update" % k)

    def test_one_shot_call_equals_the_step_sequence(self, sa, lst, ora, chunk):
        """sgl_c_nmf_sparse_list on the repeated chunk (n_t_chunks = 0), maxit = 2, in a fresh context: its h copies agree
        to rounding, and h and w equal the step-API sequence on the resident list bit for bit.  Last in its class: it
        closes the resident context to make room."""
        C, Cd, R = chunk
        k = 10
        W0 = ora.synth_winit(k, GENES)
        lst.fit_init(k, W0)
        for _ in range(2):
            lst.step_begin()
            lst.step_h(L1, 0.0)
            lst.step_scale_h()
            lst.step_w(L1, 0.0)
            lst.step_scale_w()
        W, d, H = lst.get_factors()
        lst.close()
        _release(sa)
        try:
            got = sa.c_nmf_sparse_list(R * [Cd], None, 0.0, 2, False, L1, 0.0, 0, W0.T)
            _mem("2^32 leg: after the one-shot call")
        finally:
            _release(sa)
        assert got["iter"] == 2
        h = np.ascontiguousarray(got["h"].T)
        _assert_copies_equal(h.reshape(R, NC, k), 1e-12)
        assert np.array_equal(h.view(np.uint64), H.view(np.uint64))
        assert np.array_equal(np.ascontiguousarray(got["w"].T).view(np.uint64), W.view(np.uint64))
        assert rel_fro(got["d"], d) < 1e-12
