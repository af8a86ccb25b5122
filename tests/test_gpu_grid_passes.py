"""Kernels on a capped grid, past their first grid pass.

Almost every element-wise, per-column or per-cell kernel of singlet_amd/csrc is launched on a capped grid and walks the rest
of its work in a grid-stride loop.  A test on a few hundred columns runs the first pass only; the per-workgroup state that is
re-used across passes (a table staged in LDS, the register rows of a solve, a running `best`) can only go wrong on the second
lap.  The table has one row per capped launch site: where the cap is, how much one pass holds, the smallest shape that makes
a second pass, and the test that crosses it -- an existing one where there is one, a test of this file otherwise.  The tests
of this file use the smallest shape that makes the second pass; where the work items are independent, the second-pass items
are copies of first-pass items and must carry their bits, and a handful of them meets the oracle or a longdouble reference.
test_every_test_named_in_the_table_exists (no device needed) keeps the names in the table real.

site                       one pass holds                          second pass from        crossed by
-------------------------  --------------------------------------  ----------------------  ------------------------------------
-- the fit: right-hand sides, solves, scaling --
kernels_acc.hip:108        8192 x 4 waves = 32 768 columns         32 769 columns          test_gpu_grid_passes.py::test_rhs_above_256_past_the_first_grid_pass
                             (acc_kernel<8 / 16, 0>: 32 773 cells at k = 257 / 641); acc_kernel<1, 0>:
                             test_gpu_past_2e31.py::test_plain_rhs_copies_bit_equal (k = 10 over all cells of the 2^32 leg)
kernels_nnls.hip:712       8192 x 4 waves = 32 768 columns         32 769 columns          test_gpu_grid_passes.py::test_nnls_above_256_past_the_first_grid_pass
                             (nnls_wave_kernel<8 / 16>: 32 773 columns at k = 257 / 641).  The instances <1> .. <4> take
                             32 769 .. 65 535 columns only with per-column Grams at k = 113 .. 128 and 209 .. 256: see the end of the table
kernels_nnls.hip:594       2048 x 4 waves x 4 = 32 768 columns     32 769 columns          test_gpu_grid_passes.py::test_quad_shared_solve_past_the_first_grid_pass
                             (k = 50, 32 773 columns; the fit takes this solve for short launches only)
kernels_nnls.hip:619       256 x per_cu x 4 waves x 4 columns,     65 537 columns at       test_gpu_fullsize_oracle.py::test_config5_masked_h_and_w_update_slices_equal_the_oracle
                             per_cu = 16 up to k = 24                k = 10                  (k = 10: 10^6 cells, per-column Grams in LDS)
nnls_quad_global.h:175     8192 waves x 4 = 32 768 columns         32 769 columns          test_gpu_fullsize_oracle.py::test_config5_masked_h_and_w_update_slices_equal_the_oracle
                             (k = 50 and 100: chunks of the 10^6 cells far above 32 768 columns)
nnls_quarter.h:133         256 or 512 x 4 waves x 16 columns       16 385 / 32 769 col.    test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
                             (k = 160: 10^6 columns on 512 workgroups)
kernels_prep.hip:50        16 384 x 4 waves = 65 536 columns       65 537 columns          test_gpu_ingest.py::test_log_normalize_per_element and
                             test_gpu_ingest.py::test_weight_by_split_per_element (`wide`: 65 543 columns; colsum_kernel and cell_factor_kernel by column)
kernels_prep.hip:70        16 384 x 256 = 4 194 304 entries        4 194 305 entries       test_gpu_ingest.py::test_log_normalize_per_element (`long`: 4 500 000 entries, by row index)
kernels_prep.hip:92        8192 x 256 = 2 097 152 elements         cell 41 943 at 50 rows  test_gpu_grid_passes.py::test_links_past_the_first_grid_pass (42 000 cells x 50 rows)
kernels_prep.hip:132       2048 x (256 >> fl_shift) cells:         cell 8192 / 32 768      test_gpu_grid_passes.py::test_links_past_the_first_grid_pass (both instances: G = 81
                             8192 at rows 33 - 64, 32 768 at 9 - 16                          in LDS, G = 90 cached; 9 rows x 33 000 cells; the W side over 8200 genes)
kernels_dense.hip:405      1024 / 512 / 128 workgroups of whole    262 145 / 131 073 /     test_gpu_high_rank.py::test_gram_many_partial_blocks (k <= 256: 278 523 / 139 259
                             16-column steps (256 columns each)      32 769 columns          columns); above 256: test_gpu_grid_passes.py::test_gram_above_256_past_its_block_cap
kernels_dense.hip:516      512 workgroups x 512 columns            262 145 columns         test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
kernels_dense.hip:531        (as :516: the same arithmetic on the host, which decides where the ridge is added)          (the row sums of h over 10^6 cells)
kernels_dense.hip:558      4096 x 256 = 1 048 576 elements         1 048 577 elements      test_gpu_high_rank.py::test_scale_high_rank (k = 257 x 20 000 columns and more)
kernels_dense.hip:618      512 workgroups x 4096 elements          2 097 153 elements      test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
                             (k = 160: cor over 160 x 30 000 = 4 800 000 elements of w)
kernels_dense.hip:659      1024 x 256 = 262 144 elements           --                      k_transpose_dense has no caller
kernels_dense.hip:674      4096 x 256 = 1 048 576 elements         1 048 577 elements      test_gpu_high_rank.py::test_c_ard_nmf_parity_high_rank (k = 1024 x 1100 genes = 1 126 400)
kernels_dense.hip:706      4096 x 256 = 1 048 576 genes            1 048 577 genes         test_gpu_grid_passes.py::test_hooked_gene_counts_past_the_first_grid_pass
kernels_dense.hip:712        (as :706: the way back, doubles to counts)                      (1 048 583 genes, an empty one in the second pass)
dense_frontend.hip:57      4096 x 4 waves = 16 384 columns         16 385 columns          test_gpu_ingest.py::test_dense_image_past_the_first_grid_pass (16 387 columns;
dense_frontend.hip:65        (as :57: the fill after the count)                              count and fill)
dense_frontend.hip:80      4096 x 256 = 1 048 576 elements         k x genes = 1 048 577   test_gpu_grid_passes.py::test_dense_w_side_slab_sum_past_the_first_grid_pass (50 x 21 000)
-- the synthetic generator, the mask, validation --
kernels_hash.hip:34        64 x 256 = 16 384 genes of a cell       16 385 genes            test_gpu_grid_passes.py::test_mask_rows_past_the_first_grid_pass (16 390 genes)
kernels_hash.hip:107       4096 x 4 waves = 16 384 columns         16 385 columns          synth_kernel: test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
                             (10^6 cells, slices regenerated on the host); validate_csc_kernel:
                             test_gpu_ingest.py::test_refused_upload_names_the_defect_and_leaves_the_context_empty (position `pass2`)
kernels_hash.hip:144       1024 x 256 = 262 144 elements           262 145 elements        test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
                             (winit_kernel: k = 50 x 30 000 genes, bit for bit the oracle's generator)
kernels_hash.hip:219       8192 x 256 = 2 097 152 (tile, column)   2 097 153 items         test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
                             (75 x 10^6 segment starts on the H side)
kernels_hash.hip:258       8192 x 256 = 2 097 152 values           2 097 153 values        test_gpu_ingest.py::test_non_finite_value_in_the_second_grid_pass_is_refused (2 100 000 values)
-- the transpose and the entry streams --
kernels_transpose.hip:69   8192 x 256 = 2 097 152 entries          2 097 153 entries       row_hist_kernel, gather_kernel: test_gpu_ingest.py::test_log_normalize_per_element
                             (`long`, device-built transpose: 4 500 000 entries); run_start / gather_batch / advance_kernel:
                             test_gpu_past_2e31.py::test_h_and_w_update (the column-batched sort of the 2^32 leg)
kernels_transpose.hip:145  8192 x 4 waves = 32 768 columns         32 769 columns          test_gpu_ingest.py::test_log_normalize_per_element (`wide`, device-built transpose: 65 543 columns)
kernels_tiled.hip:342      4096 x 256 = 1 048 576 columns          1 048 577 columns       test_gpu_past_2e31.py::test_h_and_w_update_equal_the_oracle (1 500 000 cells)
kernels_tiled.hip:552      16 384 x 4 waves = 65 536 chunks        65 537 chunks           test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
kernels_tiled.hip:566        (as :552: the schedule table of the same chunks)                (15 625 wave blocks x the row blocks of 30 000 genes)
kernels_tiled.hip:603        (as :552: the masked value array)                             test_gpu_fullsize_oracle.py::test_config5_masked_h_and_w_update_slices_equal_the_oracle
kernels_tiled.hip:1032     4096 x 256 = 1 048 576 elements         tail columns x k        test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
                                                                     = 1 048 577             (k = 50, H side: 162 tail workgroups x 512 columns x 50)
kernels_tiled.hip:1039     4096 x 256 = 1 048 576 elements         k x columns = 1 048 577 test_gpu_fullsize_oracle.py::test_config3_h_and_w_update_slices_equal_the_oracle
                             (k = 50, W side: 13 or more tile ranges over 30 000 genes, 1 500 000 elements)
-- the masked fit --
kernels_mask.hip:493       8192 x 256 = 2 097 152 elements         k^2 x genes of a rank   test_gpu_grid_passes.py::test_team_full_downdate_blocks_past_the_first_grid_pass
                                                                     = 2 097 153             (130^2 x 210)
kernels_mask.hip:516       8192 x 256 = 2 097 152 elements         k (k + 1) / 2 x genes   test_gpu_high_rank.py::test_sharded_masked_path_high_rank (k = 130: 8515 x 420)
kernels_mask.hip:536       8192 x 256 = 2 097 152 elements         k^2 x genes of a rank   test_gpu_high_rank.py::test_sharded_masked_path_high_rank (k = 130: 16 900 x 210)
kernels_mask.hip:807       4096 x 4 waves = 16 384 cells           16 385 cells            test_gpu_grid_passes.py::test_mse_test_families_up_to_128_past_the_first_grid_pass
kernels_mask.hip:839       4096 x 4 waves = 16 384 cells           16 385 cells            test_gpu_grid_passes.py::test_mse_test_above_128_past_the_first_grid_pass (<4>, <16>),
                             test_gpu_grid_passes.py::test_mse_test_families_up_to_128_past_the_first_grid_pass (<1>, <2>, the list and the value kernels)
kernels_mask.hip:895       256 x 256 x 16 = 1 048 576 cells        1 048 577 cells         test_gpu_grid_passes.py::test_mse_test_total_past_the_first_pass_of_its_partial_sums
-- upload doors --
kernels_ingest.hip:94      8192 x 256 = 2 097 152 values           2 097 153 values        test_gpu_native_ingest.py::test_one_entry_past_the_convert_kernels_first_pass
kernels_ingest.hip:204     4096 x 4 waves = 16 384 slices          16 385 slices           test_gpu_native_ingest.py::test_out_of_order_slice_in_the_mark_kernels_second_pass
kernels_ingest.hip:230     8192 x 256 = 2 097 152 offsets          2 097 152 slices        test_gpu_grid_passes.py::test_native_upload_past_the_first_pass_of_the_offset_and_list_kernels
kernels_ingest.hip:263     8192 x 256 = 2 097 152 slices           2 097 153 slices          (2 097 157 slices, both offset types)
-- analysis --
kernels_knn.hip:369        4096 x 256 = 1 048 576 elements         1 048 577 elements      test_gpu_grid_passes.py::test_knn_refuses_a_non_finite_value_in_the_second_grid_pass
kernels_doublet.hip:176    4096 workgroups, one pair each          4097 pairs              test_gpu_doublets.py::test_merge_bit_for_bit_on_both_paths (5000 pairs)
ligrec_host.h:21           4096 waves (1024 on the global path)    4097 (segment, group)   test_gpu_grid_passes.py::test_ligrec_sums_past_the_first_grid_pass (14 x 300 items)
kernels_raster.hip:114     65 536 workgroups: columns (sparse),    65 537 columns / tiles  sparse: test_gpu_rasterize.py::test_resident_config3 (10^6 columns); dense:
                             tiles of 256 bins (dense)                                       test_gpu_grid_passes.py::test_dense_rasterisation_past_the_first_grid_pass
kernels_neighbors.hip:24   65 535 workgroups of 1, 4 or 256 items  65 536 points           test_gpu_spatial_graph.py::test_million_point_sets and
                             test_gpu_local_neighbors.py::test_million_cell_lattice_on_a_sample (10^6 points)
kernels_umap.hip:34        2^20 workgroups of 1 or 256 items       1 048 577 cells         the fuzzy graph's merge (one cell a workgroup):
                             test_gpu_grid_passes.py::test_fuzzy_graph_past_the_first_grid_pass (1 048 583 cells, K = 2); the layout: see below
multi.hip:276              2048 x 256 = 524 288 elements           524 289 elements        test_gpu_grid_passes.py::test_team_exchange_past_the_first_pass_of_the_loopback_kernels
                             (524 295 genes: the 64-bit all-reduce, the reduce-scatter and the all-gather);
                             test_gpu_high_rank.py::test_sharded_masked_path_high_rank (reduce-scatter of 8515 x 210 doubles a rank)

Not crossed, each with its arithmetic.  Crossing needs more than 2 GB of device memory, or a CPU reference of more than about
20 s, or a switch that only A/B measurements set:
kernels_graph.hip:136      2^20 workgroups x 256 / LPC columns     2^28 / LPC + 1 columns  LPC lanes serve a column of k >= LPC / 2 + 1 rows (LPC = 1 .. 64): X and Y together hold
                             at least 2 x 8 x (2^28 / LPC) x (LPC / 2 + 1) > 2^31 bytes at every LPC, and at LPC = 1 the graph's 2^28 column pointers alone are 2 GiB
kernels_graph.hip:214        (as :136, for the exported columns of a team's halo: they are columns of X)
kernels_subset.hip:78      2^20 tiles x 4096 entries               2^32 + 1 entries        12 bytes an entry: 51 GB
kernels_ingest.hip:301     65 535 long slices a launch             65 536 slices longer than the LDS sort's capacity (4096 entries): 268 M entries x 12 bytes = 3.2 GB
kernels_cluster.hip:30     2^20 workgroups of 1, 4 or 256 items    1 048 577 vertices      one sweep of the restatement (louvain_restatement.op_sweep) takes 0.36 s at 20 000
                             vertices of degree 20 (measured): 19 s at 1 048 577 before the graph is built and a level aggregated; the launches of 256 items a workgroup need 2^28 vertices (2 GiB of column pointers)
kernels_umap.hip:34        the layout's epoch kernel (one cell a workgroup) past 1 048 576 cells: one epoch of the restatement takes 0.31 s at 20 000 cells, K = 10
                             (measured), 16 s at 1 048 577, on top of the 10 s of its fuzzy graph; the launches of 256 items a workgroup need 2^28 cells (2 GiB of lists at K = 2)
kernels_umap_transform.hip:29  (as kernels_umap.hip:34, on the query cells: 2^20 workgroups, the same restatement at the same cost)
kernels_nnls.hip:712       nnls_wave_kernel<1> .. <4> past 32 768 columns: the fit sends them launches of 32 769 .. 65 535 columns only with per-column Grams at
                             k = 113 .. 128 and 209 .. 256 (other ranks and longer launches take the four-column solves, a shared Gram the four-lane solve unless
                             SGL_NNLS_NO_QUARTER / SGL_NNLS_NO_QUAD_BIG of the A/B runs are set): 32 769 Grams of 113^2 doubles are 3.3 GB, of 209^2 11.4 GB
multi.hip:276              lb_allreduce_kernel<double> moves k^2 + k doubles: past 524 288 from k = 724, and the oracle's fit at that rank takes minutes
                             (test_gpu_high_rank.py::test_c_nmf_parity_high_rank at k = 513 runs under a 900 s limit); the <long long> instance is crossed above
"""
import os
import re

import numpy as np
import pytest

from conftest import rel_fro, same_zero_pattern, to_dgc

gpu = pytest.mark.gpu   # per test, not module-wide: test_every_test_named_in_the_table_exists runs without a device
HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -1


# ----------------------------------------------------------------------------------------------------------- the table --
def test_every_test_named_in_the_table_exists():
    """Every `file.py::test_name` of the table above is a `def` (or a method) of that file, every row that names a test of
    this file names a test of this file, and every row's `file.hip:line` / `file.h:line` is a line of that source file."""
    named = sorted(set(re.findall(r"(test_\w+\.py)::(test_\w+)", __doc__)))
    assert named, "the table names no test"
    for fname, test in named:
        with open(os.path.join(HERE, fname)) as f:
            assert re.search(r"^\s*def %s\(" % re.escape(test), f.read(), re.M), (fname, test)
    with open(os.path.abspath(__file__)) as f:
        mine = set(re.findall(r"^def (test_\w+)\(", f.read(), re.M)) - {"test_every_test_named_in_the_table_exists"}
    unnamed = mine - {test for fname, test in named if fname == os.path.basename(__file__)}
    assert not unnamed, "tests of this file that no row of the table names: %s" % sorted(unnamed)
    csrc = os.path.join(os.path.dirname(HERE), "singlet_amd", "csrc")
    sites = re.findall(r"^(\w+\.(?:hip|h)):(\d+)", __doc__, re.M)
    assert sites, "the table has no row"
    for fname, line in sites:
        with open(os.path.join(csrc, fname)) as f:
            assert 1 <= int(line) <= len(f.readlines()), (fname, line)


# ---------------------------------------------------------------------------------------- links past their first pass --
def _grouped_cells_per_pass(rows):
    """k_link_mul_grouped's arithmetic: FL = min(64, rows rounded up to a power of two) lanes per cell, 256 / FL cells per
    workgroup, 2048 workgroups."""
    fl_shift = 0
    while (1 << fl_shift) < rows and fl_shift < 6:
        fl_shift += 1
    return 2048 * (256 >> fl_shift)


def _edge_tables(rng, rows, G, ncols):
    """_tables of test_gpu_linked_workflow.py with group 0 holding a zero in its first and its last row, and the columns on
    either side of each kernel's pass edge, and the last column, put into group 0."""
    from test_gpu_linked_workflow import _tables
    T, grp = _tables(rng, rows, G, ncols)
    T[:, 0] = 0.5 + rng.random(rows)
    T[0, 0] = T[rows - 1, 0] = 0.0
    dense_edge = (8192 * 256) // rows            # the column that holds element 2 097 152, the dense kernel's second pass
    edges = [e for e in (_grouped_cells_per_pass(rows), dense_edge, dense_edge + 1) if e < ncols] + [ncols - 1]
    grp[edges] = 0
    return T, grp, edges


@gpu
@pytest.mark.parametrize("k,rows,G,cells,genes,w_side", [
    (50, 50, 81, 42000, 200, False), (50, 50, 90, 42000, 200, False), (9, 9, 3, 33000, 200, False), (50, 50, 81, 300, 8200, True)])
def test_links_past_the_first_grid_pass(sa, ora, k, rows, G, cells, genes, w_side):
    """link_mul_kernel's second pass starts at element 2 097 152 (row 2 of cell 41 943 at 50 rows), link_mul_grouped_kernel's
    at cell 8192 (rows 33 - 64: 4 cells x 2048 workgroups) or 32 768 (rows 9 - 16); at G = 81 the table (32 400 B) is staged
    in LDS and re-used by the second round, at G = 90 it is read through the cache.  The W side runs the same kernels over
    the 8200 genes.  Group 0 has a zero in its first and last row and owns the cells (genes) at the pass edges and the last.
    (a) grouped fit == dense-link fit bit for bit; (b) a zero link pins the coefficient at zero; (c) the oracle's
    c_linked_nmf on the WHOLE matrix, two iterations, at the tolerance of tests/test_gpu_nmf.py::_check.
    Oracle seconds on one CPU core (measured): 0.87 at 200 x 42 000 k = 50, 0.02 at 200 x 33 000 k = 9, 0.08 at 8200 x 300."""
    from test_gpu_linked_workflow import _check, _fit, _same_fit, _tables
    A = ora.synth_csc(genes, cells, 15)
    w0 = ora.synth_winit(k, genes)
    rng = np.random.default_rng(4)
    if w_side:
        Th, gh = _tables(rng, rows, G, cells)
        Tw, gw, edges = _edge_tables(rng, k, G, genes)
        assert edges == [8192, genes - 1]
        lw = Tw[:, gw]
    else:
        Th, gh, edges = _edge_tables(rng, rows, G, cells)
        assert edges[0] == (8192 if rows == 50 else 32768) and (rows != 50 or edges[1] == 41943)
        Tw = gw = lw = None
    lh = Th[:, gh]
    assert (lw if w_side else lh)[0, edges].tolist() == [0.0] * len(edges)
    with sa.Context(0) as c:
        grouped = _fit(c, sa, A, k, w0, lambda c: c.set_links_grouped(Th, gh, Tw, gw), iters=2)
        dense = _fit(c, sa, A, k, w0, lambda c: c.set_links(lh, lw), iters=2)
    assert _same_fit(grouped, dense)                                   # (a)
    W, d, H = grouped
    assert np.all(H[:, :rows][lh.T == 0] == 0)                         # (b)
    if w_side:
        assert np.all(W[lw.T == 0] == 0) and np.count_nonzero(W[8192:]) > 0
    else:
        assert np.count_nonzero(H[edges[0]:, :rows]) > 0               # (the second pass is not zero throughout)
    ref = ora.c_linked_nmf(A, A.t(), 0.0, 2, 0.01, 0.0, 0, w0, lh, lw if w_side else np.ones((1, 1)))
    _check({"w": W.T, "d": d, "h": H.T}, ref)                          # (c)


# ------------------------------------------------------------------------ ranks above 256 past 32 768 columns: solve --
NCOLS = 32768 + 5      # 8192 workgroups x 4 waves, and five columns of a second pass
DISTINCT = 16


@gpu
@pytest.mark.parametrize("k", [257, 641])
def test_nnls_above_256_past_the_first_grid_pass(ctx, ora, k):
    """nnls_wave_kernel<8> (k = 257) and <16> (k = 641) on 32 773 columns: 16 distinct (b, x0) tiled, so that each of the five
    second-pass columns has 2048 twins in the first pass.  Every column carries the bits of its twin, the 16 agree with
    ora.nnls at test_nnls_high_rank's bar, the sweep total is the oracle's weighted by multiplicity.
    Oracle seconds (measured): aat 0.03 / 0.31, the 16 solves 0.01 / 0.03."""
    rng = np.random.default_rng(k)
    L1, L2 = 0.01, 0.05
    G = ora.aat(rng.random((4 * k + 5, k)))
    B16 = rng.normal(size=(DISTINCT, k)) * 3 + 1.0
    X16 = np.abs(rng.normal(size=(DISTINCT, k))) * (rng.random((DISTINCT, k)) < 0.6) * 1e-3
    twin = np.arange(NCOLS) % DISTINCT
    X, sweeps = ctx.op_nnls(G, B16[twin], X16[twin], L1, L2)
    assert np.array_equal(X, X[:DISTINCT][twin])
    E = np.empty_like(X16)
    its = np.empty(DISTINCT, dtype=np.int64)
    for c in range(DISTINCT):
        E[c], _, its[c] = ora.nnls(G, B16[c], X16[c], L1, L2)
    assert rel_fro(X[:DISTINCT], E) < 1e-10
    assert np.array_equal(X[:DISTINCT] == 0, E == 0)
    assert rel_fro(X[-DISTINCT:], E[twin[-DISTINCT:]]) < 1e-10     # the last columns against the oracle directly
    assert sweeps == int((its * np.bincount(twin, minlength=DISTINCT)).sum())


# ------------------------------------------------------------------- ranks above 256 past 32 768 columns: accumulate --
@pytest.fixture(scope="module")
def wide_a(ora):
    """200 genes x 32 773 cells, shared by the accumulate cases and left unchanged."""
    return ora.synth_csc(200, NCOLS, 12)


@gpu
@pytest.mark.parametrize("k", [257, 641])
def test_rhs_above_256_past_the_first_grid_pass(ctx, sa, ora, wide_a, k):
    """acc_kernel<8, 0> (k = 257) and <16, 0> (k = 641), one wave per column on 8192 x 4 waves: 32 773 columns against
    ora.rhs at the bar of test_rhs_high_rank_plain_and_tiled, and the last 64 columns against the oracle on the slice
    regenerated from its first cell.  Oracle seconds (measured): 0.10 / 0.22."""
    A = wide_a
    ctx.upload(to_dgc(sa, A), None)
    W = np.random.default_rng(k).random((A.nrow, k))
    B = ctx.op_rhs(0, W)
    assert B.shape == (NCOLS, k)
    assert rel_fro(B, ora.rhs(A, W)) < 1e-14
    tail = ora.synth_csc(200, 64, 12, cell0=NCOLS - 64)
    assert np.count_nonzero(B[-64:]) > 0
    assert rel_fro(B[-64:], ora.rhs(tail, W)) < 1e-14
    assert rel_fro(B[32768:], ora.rhs(tail, W)[-5:]) < 1e-14


# --------------------------------------------------------------------------------- mse_test past 16 384 cells, k > 128 --
def _last_cells_reference(ora, A, W, d, H, seed, inv, last):
    """The losses of the last `last` cells as tests/test_gpu_masked_ops.py::_mse_reference forms them: longdouble
    `(W * d) @ H[c]` against the dense column, squared, averaged over the genes ora.rng_mask draws (0 where it draws none)."""
    m, n = A.nrow, A.ncol
    M = ora.rng_mask(seed, n - last, last, m, inv).astype(bool)
    assert M.shape == (last, m)
    D = np.zeros((last, m), dtype=np.longdouble)
    for q in range(last):
        lo, hi = A.p[n - last + q], A.p[n - last + q + 1]
        D[q, A.i[lo:hi]] = A.x[lo:hi]
    Wd = (W * d).astype(np.longdouble)
    ref = np.zeros(last)
    for q in range(last):
        pred = (Wd * H[n - last + q].astype(np.longdouble)).sum(axis=1)
        if M[q].any():
            ref[q] = float(((pred - D[q]) ** 2)[M[q]].sum() / M[q].sum())
    return ref, M


@gpu
@pytest.mark.parametrize("k", [130, 257])
def test_mse_test_above_128_past_the_first_grid_pass(sa, ora, k):
    """mse_test_kernel<4> (k = 130) and <16> (k = 257), one wave per cell on 4096 x 4 waves: 60 genes x 16 391 cells, the
    set-up and tolerance of test_mse_test_op_high_rank; the losses of the last seven cells (all in the second pass) against
    the per-cell terms of the reference of test_gpu_masked_ops.py -- longdouble, over the genes ora.rng_mask draws -- at that
    file's bar.  Oracle seconds (measured): below 0.01."""
    m, n, seed, inv = 60, 16384 + 7, 99, 7
    A = ora.synth_csc(m, n, 9)
    rng = np.random.default_rng(k)
    W = np.abs(rng.standard_normal((m, k)))
    H = np.abs(rng.standard_normal((n, k))) * (rng.random((n, k)) < 0.8)
    d = 0.5 + rng.random(k)
    exp = ora.mse_test(A, W, d, H, seed, inv)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A), None)
        c.fit_init(k, W)
        c.set_factors(W, d, H)
        got = c.op_mse_test(seed, inv)
        cells = c.op_mse_test_cells(seed, inv, variant=0)
    assert abs(got - exp) <= 1e-11 * abs(exp), (got, exp)
    assert cells.shape == (n,) and abs(cells.sum() / n - exp) <= 1e-11 * abs(exp)
    ref, M = _last_cells_reference(ora, A, W, d, H, seed, inv, 7)
    assert M.any(axis=1).all()
    last = cells[n - 7:]
    assert np.all(np.abs(last - ref) <= 1e-11 * np.maximum(ref, exp)), (last, ref)
    assert np.all(last[~M.any(axis=1)] == 0.0)


@gpu
@pytest.mark.parametrize("k", [50, 100])
def test_mse_test_families_up_to_128_past_the_first_grid_pass(sa, ora, k):
    """The same 16 391 cells at the ranks that have mask lists: mse_test_kernel<1> / <2> (hashing), mse_test_list_kernel<4> /
    <7>, mask_vals_kernel and mse_test_vals_kernel<4> / <7>, all on 4096 x 4 waves.  The three families agree on the last
    seven cells with the longdouble reference, the two list families bit for bit on every cell, and the total equals
    ora.mse_test before the lists exist (hashing) and after (listed values).  Oracle seconds (measured): below 0.01."""
    m, n, seed, inv = 60, 16384 + 7, 99, 7
    A = ora.synth_csc(m, n, 9)
    rng = np.random.default_rng(k)
    W = np.abs(rng.standard_normal((m, k)))
    H = np.abs(rng.standard_normal((n, k))) * (rng.random((n, k)) < 0.8)
    d = 0.5 + rng.random(k)
    exp = ora.mse_test(A, W, d, H, seed, inv)
    ref, M = _last_cells_reference(ora, A, W, d, H, seed, inv, 7)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A), None)
        c.fit_init(k, W)
        c.set_factors(W, d, H)
        before = c.op_mse_test(seed, inv)
        cells = [c.op_mse_test_cells(seed, inv, variant=v) for v in (0, 1, 2)]
        after = c.op_mse_test(seed, inv)
    assert abs(before - exp) <= 1e-11 * abs(exp) and abs(after - exp) <= 1e-11 * abs(exp), (before, after, exp)
    assert np.array_equal(cells[1], cells[2])
    for v in (0, 1, 2):
        last = cells[v][n - 7:]
        assert np.all(np.abs(last - ref) <= 1e-11 * np.maximum(ref, exp)), (v, last, ref)
        assert abs(cells[v].sum() / n - exp) <= 1e-11 * abs(exp), v
    assert np.all(np.abs(cells[0] - cells[1]) <= 1e-11 * np.maximum(cells[1], exp))


@gpu
def test_mse_test_total_past_the_first_pass_of_its_partial_sums(sa, ora):
    """sum_partial_kernel adds the per-cell losses on 256 workgroups x 256 threads x 16 cells = 1 048 576 cells a pass: 8 genes
    x 1 048 583 cells at k = 3.  The total against ora.mse_test at test_mse_test_op's bar, and against math.fsum of the
    device's own per-cell losses: a thread adds at most 17 terms in turn, the workgroup's tree has 8 levels, the last stage
    adds 256 partials in turn, one division -- non-negative terms, so the relative error is below (17 + 8 + 256 + 1) 2^-53,
    taken as 300 x 2^-53.  The last seven cells against the longdouble reference.  Oracle seconds (measured): 0.03."""
    import math
    m, n, k, seed, inv = 8, 256 * 4096 + 7, 3, 99, 3
    A = ora.synth_csc(m, n, 3)
    rng = np.random.default_rng(11)
    W = np.abs(rng.standard_normal((m, k)))
    H = np.abs(rng.standard_normal((n, k))) * (rng.random((n, k)) < 0.8)
    d = 0.5 + rng.random(k)
    exp = ora.mse_test(A, W, d, H, seed, inv)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A), None)
        c.fit_init(k, W)
        c.set_factors(W, d, H)
        got = c.op_mse_test(seed, inv)
        cells = c.op_mse_test_cells(seed, inv, variant=0)
    assert abs(got - exp) <= 1e-11 * abs(exp), (got, exp)
    exact = math.fsum(cells) / n
    assert abs(got - exact) <= 300 * 2.0 ** -53 * exact, (got, exact)
    ref, M = _last_cells_reference(ora, A, W, d, H, seed, inv, 7)
    assert M.any(axis=1).sum() == 6       # one of the seven draws no gene: its loss is exactly 0
    last = cells[n - 7:]
    assert np.all(np.abs(last - ref) <= 1e-11 * np.maximum(ref, exp)), (last, ref)
    assert np.all(last[~M.any(axis=1)] == 0.0)


# ------------------------------------------------------------------------------------------ further sites of the table --
@gpu
def test_quad_shared_solve_past_the_first_grid_pass(ctx, ora, monkeypatch):
    """nnls_quad_shared_kernel<4> (k = 50, SGL_OP_NNLS_QUAD_SHARED=1 as in test_gpu_ops.py) on 2048 workgroups x 4 waves x 4
    columns = 32 768 columns a pass; the Gram is staged in LDS once per workgroup and serves the second round too.  32 773
    columns tiled from 16: every column has the bits of its twin and of the lane kernel, the 16 agree with ora.nnls at that
    test's bar (1e-9 per column, equal zero pattern), the sweep total is the oracle's by multiplicity."""
    k, L1, L2 = 50, 0.02, 0.01
    rng = np.random.default_rng(750)
    F = rng.random((3 * k + 5, k))
    G = F.T @ F + 1e-15 * np.eye(k)
    B16 = (rng.normal(size=(DISTINCT, k)) * 3 + 1.0) * np.exp(rng.normal(size=(DISTINCT, 1)) * 2)
    X16 = np.abs(rng.normal(size=(DISTINCT, k))) * (rng.random((DISTINCT, k)) < 0.5) * 1e-3
    twin = np.arange(NCOLS) % DISTINCT
    monkeypatch.delenv("SGL_OP_NNLS_QUAD_SHARED", raising=False)
    Xl, sl = ctx.op_nnls(G, B16[twin], X16[twin], L1, L2)
    monkeypatch.setenv("SGL_OP_NNLS_QUAD_SHARED", "1")
    Xq, sq = ctx.op_nnls(G, B16[twin], X16[twin], L1, L2)
    assert np.array_equal(Xq, Xq[:DISTINCT][twin]) and np.array_equal(Xq, Xl) and sq == sl
    tot = 0
    for c in range(DISTINCT):
        xo, _, it = ora.nnls(G, B16[c], X16[c], L1, L2)
        tot += it * int((twin == c).sum())
        assert np.linalg.norm(Xq[c] - xo) <= 1e-9 * max(np.linalg.norm(xo), 1e-300) and np.array_equal(Xq[c] == 0, xo == 0)
    assert sq == tot


@gpu
def test_mask_rows_past_the_first_grid_pass(ctx, ora):
    """mask_kernel: 64 workgroups x 256 lanes = 16 384 genes a pass along a cell's row; 16 390 genes, bit for bit."""
    ngenes = 64 * 256 + 6
    for inv in (7, 1, 2 ** 20 + 7):
        assert np.array_equal(ctx.op_mask(42, inv, 1000, 5, ngenes), ora.rng_mask(42, 1000, 5, ngenes, inv)), inv


@gpu
def test_native_upload_past_the_first_pass_of_the_offset_and_list_kernels(sa):
    """offsets_kernel and lists_kernel walk 8192 x 256 = 2 097 152 slices a pass: 2 097 157 columns of two entries, columns
    7, 2 097 152 and the last stored in descending order (sorted by the LDS sort, so listed by lists_kernel), through both
    offset types; then an offset below its predecessor in the second pass.  The expected arrays are written down directly."""
    from test_gpu_native_ingest import F64, I32, I64, Csc, assert_empty, assert_same_csc, typed
    n = 8192 * 256 + 5
    i = np.tile(np.array([1, 4], dtype=np.int32), n)
    x = 1.0 + np.arange(2 * n) % 13
    wi, wx = i.copy(), x.copy()
    for col in (7, 8192 * 256, n - 1):
        i[2 * col:2 * col + 2] = [4, 1]
        wx[2 * col:2 * col + 2] = x[2 * col:2 * col + 2][::-1]
    M = Csc(x, i, 2 * np.arange(n + 1), 6)
    with sa.Context(0) as c:
        for pt in (I32, I64):
            rep = c.upload_native(typed(sa, M, 0, F64, I32, pt))
            assert (rep["sorted_lds"], rep["sorted_long"], rep["nnz"]) == (3, 0, 2 * n)
            assert c.dims() == (6, n, 2 * n)
            assert_same_csc(c.download(0), (wx, wi, M.p), "offsets of type %d" % pt)
            p = M.p.copy()
            p[n - 2] = p[n - 3] - 1
            with pytest.raises(sa.SingletHipError, match="offset"):
                c.upload_native(typed(sa, Csc(x, i, p, 6), 0, F64, I32, pt))
            assert_empty(sa, c)


@gpu
def test_dense_rasterisation_past_the_first_grid_pass(sa):
    """raster_dense_kernel: one workgroup per tile of 256 bins of a column, 65 536 workgroups: 515 rows in bins of 2 are 257
    bins = 2 tiles a column, 32 771 columns 65 542 tiles (and a remainder row).  Bit for bit the restatement."""
    import rowwise_compress_restatement as rr
    from test_gpu_rasterize import _same
    rng = np.random.default_rng(21)
    nrow, ncol, n = 515, 32768 + 3, 2
    D = np.where(rng.random((nrow, ncol)) < 0.2, rng.integers(1, 60, (nrow, ncol)), 0).astype(np.float64)
    D[:, ncol - 1] = np.arange(1.0, nrow + 1.0)
    D[:, ncol - 2] = 0.0
    got = sa.rowwise_compress_dense(D, n)
    assert got.shape == (257, ncol) and got[256, ncol - 1] == (513.0 + 514.0) / 2
    _same(got, rr.vectorised_dense(D, n))


@gpu
def test_fuzzy_graph_past_the_first_grid_pass(sa):
    """fz_merge_fast_kernel merges one cell's K slots and incoming entries per workgroup, 2^20 workgroups a pass: 1 048 583
    cells on a ring (K = 2: the cell itself and its successor at a random distance).  check_fuzzy of tests/test_gpu_umap.py:
    pattern, symmetry and rho bit for bit, sigma and the weights within that file's measured bound.  The restatement takes
    2.3 s (measured)."""
    from test_gpu_umap import check_fuzzy
    n = (1 << 20) + 7
    idx = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1).astype(np.int32)
    dist = np.stack([np.zeros(n), 0.1 + np.random.default_rng(3).random(n)], axis=1)
    G = check_fuzzy(sa, idx, dist, "ring", fallback=0)
    assert G.nnz == 2 * n and G.p[n] - G.p[n - 7] == 14


@gpu
def test_ligrec_sums_past_the_first_grid_pass(sa):
    """lr_sums_kernel walks (segment, vector group) items on at most 4096 waves (LDS path) or 1024 (global path): the matrix
    of test_gpu_ligrec.py has 14 segments, 300 label vectors at one vector per wave are 4200 items.  The vectors are 10
    distinct ones tiled: every result has the bits of its twin, the 10 those of the restatement."""
    import ligrec_restatement as lr
    from test_gpu_ligrec import GENES, labels_of, resident, same_bits, the_matrix
    K = 3
    gx, gc, gp = the_matrix(sa)[4]
    labs10 = labels_of(10, K, 8)
    want = lr.sums(gx, gc, gp, GENES, labs10, K)
    twin = np.arange(300) % 10
    labs = np.ascontiguousarray(labs10[twin])
    with resident(sa) as c:
        for path in (1, 2):
            got = c.op_ligrec_sums(labs, K, GENES, path=path, vectors_per_wave=1)
            info = c.ligrec_info()
            assert (info["path"], info["vectors_per_wave"], info["batches"]) == (path, 1, 1)
            assert same_bits(got, want[twin]), path


@gpu
def test_dense_w_side_slab_sum_past_the_first_grid_pass(sa, ora):
    """dense_sum_slabs_kernel adds the partial products of the W side's batched GEMM on 4096 x 256 = 1 048 576 elements of
    k x genes a pass: 21 000 genes at k = 50 are 1 050 000.  One iteration of c_nmf_dense on a matrix that is dense (the GEMM
    path, as test_c_nmf_dense_gemm_path) against the oracle's dense loop at _check's tolerance.  Oracle seconds (measured): 1.4."""
    from test_gpu_linked_workflow import _check
    m, n, k = 21000, 520, 50
    D = np.random.default_rng(7).random((m, n)) + 0.05
    w0 = ora.synth_winit(k, m)
    ref = ora.c_nmf_dense(D, 0.0, 1, 0.01, 0.01, 0.0, 0.0, 0, w0)
    got = sa.c_nmf_dense(D, None, 0.0, 1, False, 0.01, 0.01, 0.0, 0.0, 0, w0.T)
    _check(got, ref)
    assert np.count_nonzero(got["w"].T[20972:]) > 0


@gpu
def test_team_exchange_past_the_first_pass_of_the_loopback_kernels(sa, ora):
    """The loopback exchange of a team on one device runs on 2048 x 256 = 524 288 elements a pass: 524 295 genes make the
    64-bit all-reduce of the gene counts, the reduce-scatter of the W side's right-hand sides (k x genes) and the all-gather
    of W cross it at k = 2.  Two ranks against the oracle and the one-context fit, as
    test_team_on_one_device_high_rank.  Oracle seconds (measured): 0.6 (and 0.9 to generate and transpose the matrix)."""
    m, n, k, ranks = 2048 * 256 + 7, 64, 2, 2
    A = ora.synth_csc(m, n, 4)
    w0 = ora.synth_winit(k, m)
    ref = ora.c_nmf(A, A.t(), 0.0, 2, 0.01, 0.01, 0.0, 0.0, 0, w0)
    one = sa.c_nmf(to_dgc(sa, A), None, 0.0, 2, False, 0.01, 0.01, 0.0, 0.0, 0, w0.T)
    with sa.Multi([0] * ranks) as M:
        M.upload(to_dgc(sa, A))
        M.fit_init(k, w0)
        it, tols = M.nmf_run(0.0, 2, 0.01, 0.01, 0.0, 0.0)
        W, d, H = M.get_factors()
        W1, d1, _ = M.rank_ctx(1).get_factors(h=False)
    assert it == 2 and np.array_equal(W1, W) and np.array_equal(d1, d)
    assert rel_fro(W, ref["w"]) < 1e-9 and rel_fro(H, ref["h"]) < 1e-9 and rel_fro(d, ref["d"]) < 1e-9
    assert same_zero_pattern(W, ref["w"]) and same_zero_pattern(H, ref["h"])
    assert rel_fro(W[524288:], ref["w"][524288:]) < 1e-9 and np.count_nonzero(W[524288:]) > 0
    assert rel_fro(W, one["w"].T) < 1e-11 and rel_fro(H, one["h"].T) < 1e-11
    assert np.allclose(tols, one["tol"], rtol=1e-9, atol=0)


@gpu
def test_team_full_downdate_blocks_past_the_first_grid_pass(sa, ora, monkeypatch):
    """mask_gram_finalize_kernel (the k x k blocks of SGL_TEAM_FULL_S=1) on 8192 x 256 = 2 097 152 elements a pass: a rank's
    210 genes at k = 130 are 3 549 000.  The invariant of test_sharded_masked_path_moves_triangles_with_the_same_bits at the
    shape of test_sharded_masked_path_high_rank, whose triangles (tri_pack_kernel, mask_gram_finalize_tri_kernel) cross the
    same cap and are held to the oracle there: the full blocks must give their bits."""
    m, n, k, ranks = 420, 640, 130, 2
    A = to_dgc(sa, ora.synth_csc(m, n, 10))
    w0 = ora.synth_winit(k, m)
    out = {}
    for full in (True, False):
        if full:
            monkeypatch.setenv("SGL_TEAM_FULL_S", "1")
        else:
            monkeypatch.delenv("SGL_TEAM_FULL_S", raising=False)
        with sa.Multi([0] * ranks) as M:
            M.upload(A)
            M.fit_init(k, w0)
            r = M.ard_run(0.0, 2, 0.01, 0.0, 977, 10, 1e9, 1)
            out[full] = (M.get_factors(), (r["test_mse"], r["tol"], r["iter"]))
    for part in (0, 1):
        for a, b in zip(out[True][part], out[False][part]):
            assert np.array_equal(a, b)


@gpu
def test_gram_above_256_past_its_block_cap(ctx, ora):
    """The VALU Gram above k = 256 runs on at most 128 workgroups of whole 16-column steps (gram_chunks): up to 32 768 columns
    a workgroup has 256, beyond them its column loop grows instead.  32 773 columns at k = 257 at test_gram_high_rank's bar.
    Oracle seconds (measured): 1.1."""
    k = 257
    F = np.random.default_rng(k).random((NCOLS, k))
    G = ctx.op_gram(F)
    assert rel_fro(G, ora.aat(F)) < 1e-13
    assert np.array_equal(G, G.T)


@gpu
def test_hooked_gene_counts_past_the_first_grid_pass(sa, ora):
    """With an all-reduce hook the per-gene counts travel as doubles: i64_to_f64_kernel and f64_to_i64_kernel on 4096 x 256 =
    1 048 576 genes a pass.  1 048 583 genes x 16 cells at k = 2, one shard that holds every cell (the hook of a team of one
    adds nothing); gene 1 048 578 has no entry, so a count that is wrong in the second pass changes which genes are solved.
    Against the oracle and the fit without a hook.  Oracle seconds (measured on the 524 295-gene case, twice the size here):
    below 2."""
    m, n, k = 4096 * 256 + 7, 16, 2
    A = ora.synth_csc(m, n, 2)
    empty = 4096 * 256 + 2
    keep = A.i != empty
    cnt = np.bincount(np.repeat(np.arange(n), np.diff(A.p))[keep], minlength=n)
    A = ora.CSC(A.x[keep], A.i[keep], np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), m, n)
    per_gene = np.bincount(A.i, minlength=m)
    assert per_gene[empty] == 0 and np.all(per_gene[[m - 1, empty - 1, empty + 1]] > 0)
    w0 = ora.synth_winit(k, m)
    ref = ora.c_nmf(A, A.t(), 0.0, 2, 0.01, 0.01, 0.0, 0.0, 0, w0)
    one = sa.c_nmf(to_dgc(sa, A), None, 0.0, 2, False, 0.01, 0.01, 0.0, 0.0, 0, w0.T)
    with sa.Context(0) as c:
        c.upload(to_dgc(sa, A), None, cell_offset=0, ncells_total=n)
        c.set_allreduce(lambda ptr, count: None)
        c.fit_init(k, w0)
        for _ in range(2):
            c.nmf_iterate(0.01, 0.01, 0.0, 0.0)
        W, d, H = c.get_factors()
        c.set_allreduce(None)
    assert rel_fro(W, ref["w"]) < 1e-9 and rel_fro(H, ref["h"]) < 1e-9 and rel_fro(d, ref["d"]) < 1e-9
    assert same_zero_pattern(W, ref["w"]) and same_zero_pattern(H, ref["h"])
    assert rel_fro(W[4096 * 256:], ref["w"][4096 * 256:]) < 1e-9
    assert rel_fro(W, one["w"].T) < 1e-11 and rel_fro(H, one["h"].T) < 1e-11


# ---------------------------------------------------------------- a non-finite value in a later pass of the kNN check --
@gpu
def test_knn_refuses_a_non_finite_value_in_the_second_grid_pass(sa):
    """knn_first_nonfinite walks 4096 x 256 = 1 048 576 elements per pass; Q is 64 x 16 400 = 1 049 600: column 16 384 opens
    the second pass.  The refusal names the first non-finite value in column-major order, wherever the passes put it, and
    the context goes on to give the restatement's neighbours.  The restatement takes 0.15 s (measured)."""
    import embedding_knn_restatement as rs
    from test_gpu_embedding_knn import _refused, _same
    rng = np.random.default_rng(5)
    R, Q = rng.standard_normal((64, 50)), rng.standard_normal((64, 16400))
    want = rs.knn(R, Q, 4)
    bad = Q.copy()
    with sa.Context(0) as c:
        for (row, col), value in (((63, 16399), np.nan), ((0, 16390), -np.inf), ((5, 8), np.inf)):
            assert (col * 64 + row >= 4096 * 256) == (col >= 16384)
            bad[row, col] = value
            _refused(sa, EINVAL, r"sgl_knn: Q holds a non-finite value in column %d, row %d " % (col, row), lambda: c.knn(4, R, bad))
            _same(c.knn(4, R, Q), want, "after the refusal of (%d, %d)" % (row, col))
