// Internal declarations shared by the translation units of libsinglet_hip.so.
// gfx950 (MI355X, CDNA4) only: wave = 64 lanes, no other target is supported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>
#include <functional>
#include <vector>
#include <algorithm>

#include "../../include/singlet_hip.h"

#define SGL_WAVE 64
#define SGL_MAX_K 1024         // rank limit of the library: above 128 (plain fit) / 128 (masked fit) the generic kernels run
#define SGL_LANE_NNLS_MAX_K 128  // lane-per-column NNLS: one lane per column up to k = 64, two above; all in registers, no scratch

void sgl_set_error(const char* fmt, ...);

// device-memory pool (pool.hip): every allocation of the library goes through these; blocks >= 64 MB are cached on free
hipError_t sgl_pool_malloc_raw(void** p, size_t bytes);
template <typename T_>
inline hipError_t sgl_pool_malloc(T_** p, size_t bytes) { return sgl_pool_malloc_raw(reinterpret_cast<void**>(p), bytes); }
hipError_t sgl_pool_free(void* p);
hipError_t sgl_pool_mem_info(size_t* free_b, size_t* total_b);
void sgl_pool_release(void);
size_t sgl_pool_cached_bytes(void);

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (expr);                                                                       \
        if (e__ != hipSuccess) {                                                                       \
            sgl_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return SGL_EHIP;                                                                           \
        }                                                                                              \
    } while (0)

#define SGLCHK(expr)              \
    do {                          \
        int r__ = (expr);         \
        if (r__ != SGL_OK) return r__; \
    } while (0)

// Lets kernel F take `bytes` of dynamic LDS (above the default 48 KiB): the attribute belongs to the (function, device) pair, so it
// is set once per device; several host threads may drive devices at once.  SGL_OK, or SGL_EHIP as HIPCHK returns it.
template <auto* F>
int sgl_allow_dynamic_lds(int bytes) {
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(F), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    return SGL_OK;
}

// One orientation of the resident shard: CSC with 64-bit column pointers.
struct DevCSC {
    double* x = nullptr;
    int32_t* i = nullptr;
    int64_t* p = nullptr;
    int32_t nrow = 0, ncol = 0;
    int64_t nnz = 0;
    // Tiling of the row range into L2-sized pieces for the sparse accumulate:
    // seg[t * ncol + c] = first non-zero of column c with row >= t * tile_rows
    // (t = 0..ntiles), so tile t of column c is [seg[t][c], seg[t+1][c]).
    int64_t* seg = nullptr;
    int32_t tile_rows = 0, ntiles = 0;
};

// Re-blocked non-zero stream for the LDS-tiled accumulate (kernels_tiled.hip).
struct DevTiled {
    uint32_t* roff = nullptr;   // byte offset of the row inside the LDS tile, per entry
    double* x = nullptr;        // value per entry (0 for pads)
    int64_t* cstart = nullptr;  // [nwb * NB + 1] first entry of chunk (wb, b): wave block wb, stage = row block b
    uint8_t* cnt = nullptr;     // [nwb * NB * 32] 4-entry groups of column unit p in chunk (wb, b)
    uint16_t* ahead = nullptr;  // [nwb * NB * CW] entries of block b a column slot already took in stage b - 1 (run-ahead)
    uint16_t* gtab = nullptr;   // [E / (4 NSL) + slack] schedule: the M0 word (0x8000 | 4 * column unit) of every group of 4 entry tuples
    size_t cap_gtab = 0;
    double* part = nullptr;     // [R][k * ncol] partial slabs when the tile range is split
    double* xm = nullptr;       // value per entry with the cross-validation mask applied (0 at drawn entries), per fit
    uint64_t xm_seed = 0, xm_inv = 0;
    int xm_mask_t = -1;
    int64_t* seg = nullptr;     // [(NB + 1) * ncol] first non-zero of column c at or below row b * TR / 2 (kept for the masked values)
    int32_t* perm = nullptr;    // [ncol] column at position pos of the descending-non-zero-count order (nullptr: matrix order)
    size_t cap_perm = 0;
    int64_t perm_nnz = -1;      // the matrix (by its non-zero count) perm was computed for
    bool balance = true;        // the waves' chunks of a stage levelled by run-ahead (tiled_count_kernel; SGL_TILED_NO_BALANCE)
    bool range_fastest = false; // work units ordered (column group, tile range) instead of (tile range, column group)
    double top_share = 0.0;     // share of the non-zeros in the first 512 columns of that order (the heaviest workgroup)
    double top_share4 = 0.0;    // ... in the first 1024 (the heaviest workgroup of the quad layout)
    // The buffers outlive a fit: a rank sweep re-inits the fit tens of times on one matrix, and hipMalloc / hipFree of
    // tens of GB cost up to seconds each at config-5 size.  cap_* = allocated element counts; `built` = the stream
    // content is valid for (k, src_nnz); any change of the matrix frees everything (sgl_tiled_free).
    size_t cap_roff = 0, cap_x = 0, cap_cstart = 0, cap_cnt = 0, cap_part = 0, cap_xm = 0, cap_seg = 0, cap_ahead = 0;
    bool built = false;
    int64_t builds = 0;         // times the stream content was (re)written on this context (sgl_layout_builds)
    int64_t src_nnz = -1;
    int32_t TR = 0, T = 0, CW = 0, k = 0, R = 1, tiles_per_range = 0;
    int32_t NB = 0;             // row blocks of TR / 2 rows (the LDS tile is a ring of two): stages of the chunk loop
    int64_t tail_wg0 = -1;      // tail split (R == 1): first workgroup (x) of the last, partly filled round of 256 (-1: none)
    int32_t tail_R = 1;         //   its workgroups' tile ranges are cut into this many pieces (own slabs, summed in order)
    int32_t NSL = 2;            // column slots per LDS instruction: 2 (pairs, k <= 64) or 4 (quads, k <= 32); CW = 32 * NSL
    int32_t KS = 0;             // LDS row stride in doubles the row offsets were built for
    int64_t nwb = 0, E = 0, ncol = 0, nrow = 0;
};

struct PhaseEvent {
    int phase;
    hipEvent_t e0, e1;
};

// one pass of the re-packing lane solves (protocol: nnls_static_for.h): columns come from `list` (count at *count)
// or are 0..ncols-1 when list == nullptr; unfinished columns go to next_list (nullptr: run to the end)
struct NnlsPass {
    const int32_t* list;
    const uint32_t* count;
    int32_t* next_list;
    uint32_t* next_count;
    uint8_t* it_state;    // sweeps done so far, per column
    double* tol_state;    // running tol, per column
    int32_t final_below;  // a pass over at most this many columns runs them to the end
    int32_t fresh;        // list != nullptr but nothing to resume: a first pass over columns given in packing order (below)
    uint8_t* prev_it;     // sweeps a column needed, written when it stops: the packing key of the NEXT solve (nullptr: not kept)
    // the bounded-tol solve (kernels_nnls_asm_bounded.hip): the columns whose stop test it could not decide, for the exact kernel
    int32_t* redo_list;
    uint32_t* redo_count;
};
// device scratch of the multi-pass solve, sized for `cap` columns (owned by the caller)
struct NnlsScratch {
    int32_t* list[2] = {nullptr, nullptr};
    uint32_t* counts = nullptr;   // SGL_NNLS_MAX_PASSES + 1
    uint8_t* it_state = nullptr;
    double* tol_state = nullptr;
    int64_t cap = 0;
    // packing by sweep count (H side of a plain fit): per column the sweeps of the previous solve, the columns in descending
    // order of it, and the counting sort's workspace
    uint8_t* prev_it = nullptr;
    int32_t* packed = nullptr;
    uint32_t* sort_ws = nullptr;  // [128 * nblocks + 4 + 128]: counts / offsets, the list length, the 128 bin totals
    int64_t pack_cap = 0;
    // the redo list of the bounded-tol solve and its length (a device word)
    int32_t* redo_list = nullptr;
    uint32_t* redo_count = nullptr;
    int64_t redo_cap = 0;
};

// The cross-validation mask of one orientation as lists: idx[ptr[c] .. ptr[c + 1]) = the rows r (ascending) with
// draw(cell, gene) true for column c -- built once per (seed, inv_density, shape, offsets) by two hashing passes and
// read by mask_gram_list_kernel every iteration instead of hashing all rows x columns again (kernels_mask.hip).
#define SGL_ML_KEEP 3
struct DevMaskList {
    int64_t* ptr = nullptr;    // ncol + 1
    int32_t* idx = nullptr;
    double* val = nullptr;     // cell side, on the first mse_test of a mask: the matrix value at every listed (gene, cell), 0 where A has none
    bool val_ok = false, val_refused = false;
    size_t cap_ptr = 0, cap_idx = 0, cap_val = 0;
    int64_t ncol = 0, total = 0;
    int32_t nrow = 0;
    uint64_t seed = 0, inv = 0;
    int mask_t = -1;           // -1: nothing built
    int64_t col_off = 0, row_off = 0;
    bool refused = false;      // too large for the memory budget under this key: the hashing kernel runs
};

// Cell graph of graph-convolutional NMF (c_gcnmf, src/singlet.cpp:1668-1730): n x n CSC, 64-bit offsets, uploaded by
// sgl_set_graph.  Columns with more than SGL_GRAPH_HUB entries ("hubs") are cut into segments of SGL_GRAPH_SEG entries that
// separate waves sum into partials, added afterwards in segment order (kernels_graph.hip).
#define SGL_GRAPH_HUB 128
#define SGL_GRAPH_SEG 64
struct DevGraph {
    double* x = nullptr;
    int32_t* i = nullptr;
    int64_t* p = nullptr;
    int64_t nnz = 0;
    int32_t n = 0;              // 0: no graph set
    int32_t* seg_col = nullptr; // [nseg] hub column of each segment (segments of one hub are contiguous, in entry order)
    int64_t* seg_q0 = nullptr;  // [nseg] first entry of each segment
    int32_t* hub_col = nullptr; // [nhub] the hub columns
    int32_t* hub_seg0 = nullptr;// [nhub + 1] first segment of each hub
    double* part = nullptr;     // [nseg * k] partial sums of the segments
    int32_t nseg = 0, nhub = 0;
    double* buf = nullptr;      // k x n (+ 2): the convolved right-hand sides of the H-update
    // rank of a team (sgl_multi_set_graph): n = the rank's own cells; a row index below n_src names a column of the rank's
    // factor block, n_src + s * E + e names entry e of rank s's export list, held in the halo slab
    int32_t n_src = 0;
    int32_t E = 0;              // longest export list of the team (0: no edge crosses a rank boundary, no halo step)
    int32_t n_exp = 0;          // this rank's export list: its cells that other ranks read, ascending (local indices)
    int32_t* exp = nullptr;
    double* halo = nullptr;     // [team size * E * k] block s = the exported columns of rank s (all-gathered in place)
};

// The grouped form of one side's link matrix (sgl_set_links_grouped): column c of the link is column group[c] of a
// rows x groups table, so rows * groups doubles and 4 bytes per cell / gene are resident instead of rows x cols doubles.
struct DevGroupLink {
    double* table = nullptr;   // rows x groups, column-major (nullptr: this side has no grouped link)
    int32_t* group = nullptr;  // one id in [0, groups) per local cell (H side) / per gene (W side)
    int rows = 0, groups = 0;
};

struct sgl_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    DevCSC A, At;  // A: genes x local cells; At: local cells x genes
    DevTiled TA, TAt;  // re-blocked streams of A / At for the current k (k <= 64)
    bool use_tiled = false;
    int64_t cell_offset = 0, ncells_total = 0;
    int64_t* col_nnz_A = nullptr;   // n_local: nnz per cell (skip rule of predict, l.340)
    int64_t* col_nnz_At = nullptr;  // m: nnz per gene of THIS shard
    int64_t* col_nnz_At_global = nullptr;  // m: nnz per gene over all shards (valid while gene_nnz_global)
    bool gene_nnz_global = false;

    int k = 0;
    double *W = nullptr, *Wprev = nullptr, *H = nullptr, *d = nullptr;
    double* B = nullptr;    // k x ncol_local right-hand sides of the H-update
    double* red = nullptr;  // [k*m right-hand sides of the W-update | k*k Gram of H | k row sums]
    double* G = nullptr;    // k x k Gram (+1e-15 diagonal)
    double* Gpad = nullptr; // KP x KP zero-padded copy for the lane NNLS kernel
    NnlsScratch nnls_scr;   // lists / per-column state of the multi-pass lane NNLS
    bool solve_empty = false;  // dense front-end (src/singlet.cpp:370-381): no empty-column skip
    // dense front-end (dense_frontend.hip): the matrix as R holds it (nrow x ncol, column-major) next to its CSC image;
    // dense_gemm: more than half of it is non-zero -> the right-hand sides of predict are GEMMs (rocBLAS)
    double* Adense = nullptr;
    bool dense_gemm = false;
    void* rocblas = nullptr;
    double* link_h = nullptr;  // c_linked_nmf: link_rows x ncol / x nrow multipliers of the right-hand sides
    double* link_w = nullptr;
    int link_h_rows = 0, link_w_rows = 0;
    DevGroupLink glink_h, glink_w;   // the grouped form: a side holds the dense matrix, the grouped table or nothing
    DevGraph graph;            // c_gcnmf: right-hand sides convolved over the cell graph (sgl_set_graph); dropped with the fit
    bool dense_input = false;  // the resident matrix came from sgl_upload_dense (a graph is refused there)
    DevMaskList ML[2];         // masked path: the drawn rows of every column, per orientation (kernels_mask.hip); live with the entry streams
    int64_t ml_builds[2] = {0, 0};        // times the lists of an orientation were hashed out on this context (sgl_layout_builds)
    DevMaskList MLkeep[2][SGL_ML_KEEP];   // the lists of the masks used before this one, most recent first (sgl_mask_list_select)
    double* Gcols = nullptr;   // masked path: per-column Grams of one chunk of columns (gcols_chunk * k * k)
    int64_t gcols_chunk = 0;
    double* Wd = nullptr;      // mse_test: W' = W^T diag(d) as k x m
    double* Sbuf = nullptr;    // team masked W-update: per-gene downdate partials, (gene blocks x team size) x k x k
    double* Stri = nullptr;    // ... their lower triangles, what the reduce-scatter moves: (gene blocks x team size) x k (k + 1) / 2
    struct sgl_team* team = nullptr;   // native collective (multi.hip): the team this context is a rank of
    int team_rank = 0;
    double* ws = nullptr;   // partial-reduction workspace
    size_t ws_bytes = 0;
    double* scalars = nullptr;       // device scratch for cor / mse results
    unsigned long long* sweep_counters = nullptr;   // device: [0] H sweeps, [1] W sweeps
    int64_t sweeps_acc[4] = {0, 0, 0, 0};
    int64_t wave_sweeps_acc[2] = {0, 0};
    double* pinned = nullptr;        // host pinned scratch (8 doubles)
    // sgl_knn_info / sgl_knn_metric_info: instance, segments, queries per workgroup, list home, metric and columns without
    // direction of the last search
    int64_t knn_last[6] = {0, 0, 0, 0, 0, 0};
    // sgl_knn_ivf_info: lists, probes, training cells, shortest and longest list, empty lists, short queries, scan instance of
    // the last inverted-list search; sgl_knn_ivf_stage_ms: its stage times (timing on)
    int64_t knn_ivf_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double knn_ivf_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    struct KnnIndex* knn_index = nullptr;   // the neighbour index kept on the device (kernels_knn_ivf.hip: sgl_knn_index_build); one per context
    int64_t markers_last[4] = {0, 0, 0, 0};   // sgl_markers_info: genes sorted in LDS, long genes, batches, the LDS cap of the last rank pass
    double* ann_F = nullptr;   // sgl_annotate_hold: a k x n embedding kept for the annotation calls (F == NULL reads it)
    int32_t ann_k = 0;
    int64_t ann_n = 0;
    int64_t gsea_last[5] = {0, 0, 0, 0, 0};   // sgl_gsea_info: sets, distinct sizes, s_max, batches, batch size of the last enrichment call
    // sgl_signature_info: cells sorted by the small and by the large LDS instance, long cells, batches, set passes, and the
    // caps in force (LDS entries, batch entries, sets per pass) of the last signature call
    int64_t signature_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // sgl_doublets_info: pairs merged on the LDS path and on the long path, stored entries of S, rows stored in both parents,
    // of the last sgl_simulate_doublets into / sgl_op_pair_columns on this context
    int64_t doublet_last[4] = {0, 0, 0, 0};
    // sgl_moran_info: genes on the search path and on the table path, table batches, the table batch B, the table's bytes and
    // the LDS cap in force, of the last sgl_moran / sgl_op_moran_cross on this context
    int64_t moran_last[6] = {0, 0, 0, 0, 0, 0};
    // sgl_nhood_info: the tally's path (1 LDS, 2 global; 0: none ran), the permutations per group, the batches, the permutations
    // per batch, the LDS bytes per workgroup and the sort (0 segmented, 1 device-wide) of the last neighbourhood enrichment call
    int64_t nhood_last[6] = {0, 0, 0, 0, 0, 0};
    // sgl_ligrec_info: the sums' path (1 LDS, 2 global; 0: none ran), the label vectors per wave, the batches, the vectors per
    // batch, the LDS bytes per workgroup, the waves per workgroup and the listed genes on the LDS and on the global path, of the
    // last ligand-receptor call on this context
    int64_t ligrec_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // sgl_cooccur_info: the grid mode run (1 one bucket, 2 the bucket grid; 0: none ran), W, H, the bin path (1 LDS, 2 global), the
    // LDS bytes per workgroup, the workgroups, the flushes and the candidate pairs evaluated, of the last co-occurrence call
    int64_t cooccur_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    sgl_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;

    bool timing = false;
    std::vector<PhaseEvent> pending;
    std::vector<hipEvent_t> event_pool;
    double phase_ms[SGL_PH_COUNT] = {0};
    int64_t phase_calls[SGL_PH_COUNT] = {0};
};

// native team (multi.hip): ranks of a cell-sharded fit that exchange through RCCL (or, for ranks that
// share one device inside one process, through a HIP kernel)
int sgl_team_size(const sgl_ctx* c);   // 1 without a team
// internals of singlet_hip.hip used by multi.hip
int sgl_nnls_shared(sgl_ctx* c, const double* G, double* B, double* X, const int64_t* col_nnz, int64_t ncols,
                    double L1, double L2, unsigned long long* counter, bool h_side = false);
// the two halves of sgl_step_h: Gram of w and right-hand sides B (convolved over the graph into graph.buf when
// `convolve`), then the solve (which convolves first when `convolve`): a team puts its halo exchange between them
int sgl_step_h_rhs(sgl_ctx* c, bool convolve);
int sgl_step_h_solve(sgl_ctx* c, double L1, double L2, bool convolve);
// cell graph of a context (singlet_hip.hip): checks of sgl_set_graph (messages start with `who`), upload of the columns
// [0, ncol) described by Gp[0 .. ncol] (entries Gx / Gi [Gp[0], Gp[ncol])), release
int sgl_graph_check(const char* who, const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t G_nrow, int32_t G_ncol, int64_t n);
int sgl_graph_upload(sgl_ctx* c, const char* who, const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t ncol);
void sgl_graph_clear(sgl_ctx* c);
// links of either form on either side (a graph is refused next to them)
inline bool sgl_has_links(const sgl_ctx* c) { return c->link_h || c->link_w || c->glink_h.table || c->glink_w.table; }
int sgl_scale_w_enqueue(sgl_ctx* c);            // scale(w, d); cor(w, w_prev) -> device scalar
int sgl_scale_w_fetch(sgl_ctx* c, double* tol); // copy it out (synchronises the stream)
// masked path pieces (singlet_hip.hip) used by the team's sharded c_ard_nmf (multi.hip)
int sgl_mask_workspace(sgl_ctx* c);
int sgl_predict_mask_dev(sgl_ctx* c, const DevCSC& M, const int64_t* col_nnz, const double* F, double* X, double* Bbuf,
                         uint64_t seed, uint64_t inv_density, double L1, double L2, int mask_t, int rhs_phase, int nnls_phase,
                         unsigned long long* counter);
int sgl_mse_test_enqueue(sgl_ctx* c, uint64_t seed, uint64_t inv_density);   // local loss sum -> c->scalars[1]
#define SGL_MASK_MAX_K SGL_MAX_K   // the masked (ARD) path: MFMA Gram downdates up to k = 128, the generic VALU kernel above
void sgl_team_detach(sgl_ctx* c);               // called by sgl_destroy
void sgl_knn_index_free(sgl_ctx* c);            // called by sgl_destroy and sgl_knn_index_drop (kernels_knn_ivf.hip)

// RAII-free phase timer helpers (driver side).
int sgl_phase_begin(sgl_ctx* c, int phase, PhaseEvent* pe);
int sgl_phase_end(sgl_ctx* c, PhaseEvent* pe);
int sgl_ws_reserve(sgl_ctx* c, size_t bytes);
struct Phase {  // scope guard: the phase ends on every exit (a failing hipEventRecord only loses the sample, never the call)
    sgl_ctx* c;
    PhaseEvent pe;
    Phase(sgl_ctx* c_, int phase) : c(c_) { (void)sgl_phase_begin(c, phase, &pe); }
    ~Phase() { (void)sgl_phase_end(c, &pe); }
};

// ---- host-side helpers every unit shares ------------------------------------
template <typename T>
inline int dev_alloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = sgl_pool_malloc(p, count * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        sgl_set_error("hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
        return SGL_ENOMEM;
    }
    return SGL_OK;
}
template <typename T>
inline void dev_free(T*& p) {
    if (p) (void)sgl_pool_free(p);
    p = nullptr;
}
// device buffer released on every return path (alloc on a held buffer frees it first)
template <typename T>
struct DevBuf {
    T* p = nullptr;
    ~DevBuf() { dev_free(p); }
    int alloc(size_t n) { dev_free(p); return dev_alloc(&p, n); }
};
// the context of a one-shot call, destroyed on every return path
struct CtxHolder {
    sgl_ctx* c = nullptr;
    ~CtxHolder() { if (c) sgl_destroy(c); }
};
inline int current_device_or_zero() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; }
    return d;
}

// ---- the ALS loops (singlet_hip.hip), shared with the team (multi.hip) -------
// what c_ard_nmf_base (src/singlet.cpp:1090-1152) takes and returns beyond c_nmf_base: the mask, the trace schedule, the traces
struct ArdArgs {
    uint64_t seed, inv_density;
    double overfit_threshold;
    int32_t trace_test_mse;
    double* test_mse;
    int32_t* iter;
    double* tol_out;
    double* score_overfit;
    int32_t* n_trace;
};
int sgl_ard_args_check(const ArdArgs& a, const char* who);   // SGL_EINVAL "<who>: bad arguments"
int sgl_mask_rank_check(int k);                               // SGL_EINVAL above SGL_MASK_MAX_K
// THE loop of c_nmf_base l.647-664 (ard == nullptr: tol_trace[it]) and c_ard_nmf_base l.1090-1152 (ard + mse_test: a trace row
// every trace_test_mse iterations and after the last one, the overfit break).  iterate: one iteration, returns tol.  The sweep
// counters of ctxs[0 .. nctx) are fetched at the end.  log gets NAN as the score of an untraced iteration; poll ends an iteration.
int sgl_als_loop(double tol, int32_t maxit, const std::function<int(double*)>& iterate, const ArdArgs* ard,
                 const std::function<int(double*)>& mse_test, sgl_ctx* const* ctxs, int nctx, double* tol_trace, int32_t* n_iter,
                 const sgl_callbacks* cb);
// one iteration on ONE shard (no team): step_begin, step_h, scale_h, step_w, scale_w -- the masked steps with `mask`; cb (may be
// NULL) is polled after scale_h
int sgl_iterate_shard(sgl_ctx* c, double L1_w, double L1_h, double L2_w, double L2_h, const ArdArgs* mask, const sgl_callbacks* cb,
                      double* tol);
int sgl_ard_run_team(sgl_ctx* c, double tol, int32_t maxit, double L1, double L2, const ArdArgs& a, int32_t* n_iter,
                     const sgl_callbacks* cb);

// ---- kernel launchers (each enqueues on `s`, returns SGL_* code) ----------
// hash / synthetic generator / mask
int k_rand(hipStream_t s, uint64_t state, const uint64_t* i, const uint64_t* j, int64_t n, uint64_t* out);
int k_mask(hipStream_t s, uint64_t state, uint64_t inv_density, int64_t cell0, int32_t ncells, int32_t ngenes, uint8_t* out);
// counts per column of the synthetic matrix.  transposed = 0: column = cell
// (rows = genes); 1: column = gene (rows = local cells).
int k_synth_count(hipStream_t s, uint64_t S, uint64_t inv_density, int transposed, int64_t cell_offset,
                  int32_t ncells, int32_t ngenes, int64_t* counts, const double* skew_dev = nullptr);
int k_synth_fill(hipStream_t s, uint64_t S, uint64_t inv_density, const double* levels16_dev, int transposed,
                 int64_t cell_offset, int32_t ncells, int32_t ngenes, const int64_t* p, int32_t* idx, double* x,
                 const double* skew_dev = nullptr);
int k_synth_winit(hipStream_t s, uint64_t S, int k, int32_t ngenes, double* W);
int k_exclusive_scan(sgl_ctx* c, const int64_t* in, int64_t* out, int64_t n);  // out has n+1 entries
int k_scan_total(hipStream_t s, const int64_t* in, int64_t* out, int64_t n);
int k_col_counts(hipStream_t s, const int64_t* p, int64_t ncol, int64_t* counts);
int k_validate_csc(hipStream_t s, const int32_t* idx, const int64_t* p, int64_t ncol, int32_t nrow, int* flag_dev);
int k_all_finite(hipStream_t s, const double* x, int64_t n, int* flag_dev);   // flag |= 4 on NaN / Inf (after k_validate_csc)
int k_widen_p(hipStream_t s, const int32_t* p32, int64_t n1, int64_t* p64);
int k_build_segments(hipStream_t s, const DevCSC& M);

// dense helpers
int k_gram(sgl_ctx* c, const double* F, int k, int64_t cols, double* G, double diag_add);
int k_gram_add_diag(hipStream_t s, double* G, int k, double v);
int k_rowsum(sgl_ctx* c, const double* F, int k, int64_t cols, double* d_out, int add_eps = 0);  // add_eps: + 1e-15 in the final stage
bool k_rowsum_can_add_eps(int k, int64_t cols);
int k_scale_apply(hipStream_t s, double* F, int k, int64_t cols, double* d, int add_eps);
int k_add_eps(hipStream_t s, double* d, int k);   // d += 1e-15, the kernel of k_scale_apply(add_eps = 1)
// k_scale_apply(add_eps = 0) and k_gram of the scaled F in one pass over F, bit for bit (k <= 64)
int k_scale_gram(sgl_ctx* c, double* F, int k, int64_t cols, const double* d, double* G, double diag_add);
int k_cor(sgl_ctx* c, const double* x, const double* y, int64_t n, double* out_dev);
int k_pad_gram(hipStream_t s, const double* G, int k, int KP, int GS, double* Gpad);
int k_gram_rescale(hipStream_t s, double* G, int k, const double* d, double diag_add);  // G[i,j] = G[i,j] / d_i / d_j (+ diag_add)
int k_i64_to_f64(hipStream_t s, const int64_t* in, double* out, int64_t n);
int k_f64_to_i64(hipStream_t s, const double* in, int64_t* out, int64_t n);
int k_transpose_dense(hipStream_t s, const double* in, int rows, int cols, double* out);

// sparse accumulate: B[:, c] (+)= sum_{nz in tile t of column c} x * F[:, row]
int k_acc(hipStream_t s, const DevCSC& M, const double* F, int k, double* B,
          uint64_t mask_seed, uint64_t inv_density, int mask_mode, int64_t mask_col_offset, int64_t mask_row_offset);

// LDS-tiled accumulate
void sgl_tiled_free(DevTiled& S);
int sgl_tiled_build(sgl_ctx* c, const DevCSC& M, int k, DevTiled& S);
int k_acc_tiled(hipStream_t s, const DevTiled& S, const double* F, int ldf, double* B, int ldb, int kf, const double* xvals = nullptr);
int k_acc_tiled_all(hipStream_t s, const DevTiled& S, const double* F, double* B, int k, const double* xvals = nullptr);
int sgl_tiled_mask_values(sgl_ctx* c, const DevCSC& M, DevTiled& S, uint64_t seed, uint64_t inv_density, int mask_t,
                          int64_t col_off, int64_t row_off);
// masked right-hand sides of predict_mask for one orientation (0: A, 1: At), through the tiled kernel when the fit has one
int sgl_masked_rhs(sgl_ctx* c, int orientation, const double* F, double* Bbuf, uint64_t seed, uint64_t inv_density);
int tiled_part_size(int k);

// dense front-end (dense_frontend.hip)
int k_dense_count(hipStream_t s, const double* A, int32_t nrow, int64_t ncol, int64_t* counts);
int k_dense_fill(hipStream_t s, const double* A, int32_t nrow, int64_t ncol, const int64_t* p, int32_t* idx, double* x);
int k_dense_rhs(sgl_ctx* c, int which, const double* F, int k, double* B);
void sgl_dense_release(sgl_ctx* c);
bool sgl_dense_gemm_available();

// input staging (kernels_prep.hip)
int k_colsum(hipStream_t s, const DevCSC& M, double* sums);
int k_cell_factor(hipStream_t s, DevCSC& A, DevCSC& At, const double* f, int mode, double scale);
int k_link_mul(hipStream_t s, double* B, const double* L, int k, int link_rows, int64_t ncols);
// the same multiplication with the link column looked up by group: B[j, c] *= T[j, group[c]], j < rows (T rows x n_groups)
int k_link_mul_grouped(hipStream_t s, double* B, const double* T, const int32_t* group, int k, int rows, int n_groups, int64_t ncols);
#define SGL_GLINK_LDS_BYTES (32 * 1024)   // a table of up to this many bytes is staged in LDS; a larger one is read through the cache

// group sums (kernels_group.hip): F k x n column-major on the device, group[c] in [0, n_groups) on the HOST (checked by the
// caller).  out (k x n_groups, host) = the sums of F's columns per group -- divided by the group's cell count when
// `divide` (0 / 0 = NaN for an empty group) -- and counts (n_groups, host).  The summation order depends on (n, group,
// n_groups) alone.  Synchronises the stream.
#define SGL_GROUP_CHUNK 256   // cells per chunk of a group's cell list
int sgl_group_sums_dev(sgl_ctx* c, const double* F, int k, int64_t n, const int32_t* group, int32_t n_groups, bool divide,
                       double* out, int64_t* counts);
// its two halves, for a caller that makes a second pass over the same cell lists (kernels_annotate.hip): the plan -- the
// cells by group in ascending index (a NEGATIVE id leaves its cell out), cut into chunks -- and the two kernels, launched in
// the "scale" phase on device arrays (part: nchunks x k, out: k x n_groups); NEITHER half synchronises: as before the split,
// one call queues the uploads, the kernels and the copy back, and waits once at its end
struct GroupPlan {
    DevBuf<int32_t> perm, cgroup;       // the included cells by group; the group of every chunk
    DevBuf<int64_t> cbeg, gfirst, goff; // chunk -> first position; group -> first chunk; group -> first position
    std::vector<int64_t> counts;        // host: cells per group
    std::vector<int32_t> h_perm, h_cgroup;          // the host images the asynchronous uploads read: they live as long as the
    std::vector<int64_t> h_cbeg, h_gfirst, h_goff;  // plan, and the caller synchronises the stream before the plan goes
    int64_t nchunks = 0, n_in = 0;
};
int sgl_group_plan(sgl_ctx* c, GroupPlan& P, int64_t n, const int32_t* group, int32_t n_groups);
int sgl_group_sums_on(sgl_ctx* c, GroupPlan& P, const double* F, int k, int32_t n_groups, bool divide, double* part, double* out);
// SGL_EINVAL naming the list, the position and the value of the first id outside [0, n_groups)
int sgl_group_ids_check(const char* who, const char* name, const int32_t* group, int64_t n, int32_t n_groups);

// model error (kernels_eval.hip; include/singlet_hip.h, sgl_evaluate) of the shard of a context with a fit: *cell_sum (host) = the
// order-fixed sum of the clamped losses of its cells; cell_loss (host, ncol; may be NULL); gene_loss (host, nrow; NULL: the
// gene side is skipped) = the losses of the genes over THIS shard's cells, clamped only when `clamp_genes` (a team adds the
// unclamped rank partials first).  Uses red, B, G and the workspace as scratch; synchronises the stream.
int sgl_eval_shard(sgl_ctx* c, bool clamp_genes, double* cell_sum, double* cell_loss, double* gene_loss);

// variable features (kernels_hvg.hip; include/singlet_hip.h, sgl_variable_features).  All arrays are the HOST's; every call
// only reads the context, allocates its own temporaries and synchronises the stream before it returns.
// one gene pass over c->At: mode 0 mean (out = mean, count = c_g), 1 variance about mu, 2 standardised variance (mu, sd, vmax)
int sgl_hvg_pass(sgl_ctx* c, int mode, const double* mu, const double* sd, double vmax, double* out, int64_t* count);
int sgl_loess_direct(sgl_ctx* c, const double* x, const double* y, int64_t n, int64_t q, double* fitted);   // arguments checked by the caller
int sgl_hvg_args_check(const char* who, int32_t nrow, int32_t ncol, int32_t nfeatures, double span, const double* expected_var,
                       const int32_t* features, const int32_t* n_out);
int sgl_hvg_select(sgl_ctx* c, int32_t nfeatures, double span, double vmax, const double* expected_var, int32_t* features,
                   int32_t* n_out, double* info);   // the composite after its refusals

// marker genes (kernels_markers.hip; include/singlet_hip.h, "Marker genes").  All arrays are the HOST's; every call only reads the
// context, allocates its own temporaries and synchronises the stream before it returns.
int sgl_markers_args_check(const char* who, const int32_t* labels, int64_t ncol, int32_t n_groups, int transform, double pseudocount);
// the device passes over c->At (labels checked before): the group sums with their counts (`sums`) and / or the rank pass
// (`ranks`; max_batch_entries <= 0: the default); m x G column-major outputs, any may be NULL
int sgl_markers_core(sgl_ctx* c, const int32_t* labels, int32_t G, int transform, int64_t max_batch_entries, bool sums, bool ranks,
                     int64_t* group_n, int64_t* pos, int64_t* nz, double* sum, int64_t* rank2, uint64_t* tie);
// both passes and the derived statistics (markers_host.h)
int sgl_markers_all(sgl_ctx* c, const int32_t* labels, int32_t G, int transform, double pseudocount, int64_t* group_n, int64_t* pos,
                    double* sum, int64_t* rank2, uint64_t* tie, double* pct_in, double* pct_out, double* log2fc, double* z, double* p);

// factor annotation (kernels_annotate.hip; include/singlet_hip.h, "Factor annotation").  Host arrays except F, which is the
// DEVICE's (k x n column-major); every call only reads the context, allocates its own temporaries and synchronises the stream
// before it returns.  k = 1 on the gene side, which has no rank to refuse.
int sgl_annotate_args_check(const char* who, const int32_t* labels, int64_t n, int32_t n_groups, int32_t k);
int sgl_group_moments_dev(sgl_ctx* c, const double* F, int k, int64_t n, const int32_t* labels, int32_t G, int64_t* group_n, double* sum,
                          double* rss);
// over c->At: nz and sum from sgl_markers_core (transform 0), rss = E + Z; m x G column-major, rss m values; any may be NULL
int sgl_gene_moments_core(sgl_ctx* c, const int32_t* labels, int32_t G, int64_t* group_n, int64_t* nz, double* sum, double* rss);

// signature scores (kernels_signature.hip; include/singlet_hip.h, "Signature scores").  All arrays are the HOST's; every call only
// reads the context (it records what it ran in signature_last), allocates its own temporaries and synchronises the stream
// before it returns.  The args check holds every refusal of the arguments and launches nothing (m = the genes of the matrix).
int sgl_signature_args_check(const char* who, const int64_t* set_ptr, const int32_t* set_genes, int64_t n_sets, int64_t m, int64_t max_rank,
                             int64_t lds_cap, int64_t max_batch_entries, int64_t pass_sets);
// over c->A (arguments checked before): rank2 / score n_sets x ncol, set fastest; either may be NULL; a knob of 0: the default
int sgl_signature_scores_core(sgl_ctx* c, const int64_t* set_ptr, const int32_t* set_genes, int32_t n_sets, int64_t max_rank, int64_t lds_cap,
                              int64_t max_batch_entries, int64_t pass_sets, uint64_t* rank2_out, double* score_out);
// the doubled capped midrank of every stored entry (nnz values) and of every cell's zero block (ncol values; 0: no zero block)
int sgl_cell_ranks_core(sgl_ctx* c, int64_t max_rank, int64_t lds_cap, int64_t max_batch_entries, uint64_t* entry_out, uint64_t* zero2_out);

// simulated doublets (kernels_doublet.hip; include/singlet_hip.h, "Simulated doublets"): S = the pair sums of A's columns, built
// on c's stream from c's pool; the parent lists are the HOST's and have been checked (doublet_host.h).  S comes in empty; on a
// failure the caller frees what it holds.  info: LDS pairs, long pairs, entries of S, shared rows; *bad_col: the lowest
// simulated column with a non-finite sum, or -1.  count_only: S.p alone.  Synchronises the stream.
int sgl_pair_columns_core(sgl_ctx* c, const DevCSC& A, const int32_t* parent_a, const int32_t* parent_b, int64_t n, int64_t lds_cap,
                          bool count_only, DevCSC& S, int64_t info[4], int64_t* bad_col);

// spatial autocorrelation (kernels_moran.hip; include/singlet_hip.h, "Spatial autocorrelation").  All arrays are the HOST's but
// F, which is the DEVICE's (k x n column-major); every call only reads the context (the gene form records what it ran in
// moran_last), allocates its own temporaries and synchronises the stream before it returns.  The args check holds every refusal
// of the arguments (the graph through sgl_graph_check, n, the gene list, the knobs) and launches nothing.
int sgl_moran_args_check(const char* who, const double* Gx, const int32_t* Gi, const int32_t* Gp, int64_t G_n, int64_t ncells, const int32_t* genes,
                         int64_t n_genes, int64_t m, int64_t path, int64_t lds_cap, int64_t table_batch);
// over c->At: moments_out 6 x n_genes (mean, M2, M4, T, P, c_g) with want_moments (a graph without weight is then refused),
// P_out n_genes; either may be NULL; a knob of 0: the default
int sgl_moran_genes_core(sgl_ctx* c, const double* Gx, const int32_t* Gi, const int32_t* Gp, const int32_t* genes, int64_t n_genes, int path,
                         int64_t lds_cap, int64_t table_batch, bool want_moments, double* moments_out, double* P_out);
// moments_out 6 x k (+0.0, M2, M4, +0.0, C, n: the rows are centred), mean_out k; either may be NULL
int sgl_moran_embedding_core(sgl_ctx* c, const double* Gx, const int32_t* Gi, const int32_t* Gp, const double* F, int k, int64_t n,
                             double* moments_out, double* mean_out);

// neighbourhood enrichment (kernels_nhood.hip; include/singlet_hip.h, "Neighbourhood enrichment").  All arrays are the HOST's;
// every call reads nothing of the context but its device, stream and pool (it records what it ran in nhood_last), allocates its
// own temporaries and synchronises the stream before it returns.  The *_args_check functions hold every refusal and launch nothing.
int sgl_nhood_args_check(const char* who, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* lab, int64_t K, int64_t nperm, int64_t batch);
int sgl_nhood_permute_args_check(const char* who, int64_t n, const int32_t* lab, int64_t r0, int64_t nb);
int sgl_nhood_tally_args_check(const char* who, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* labs, int64_t nb, int64_t K, int path,
                               int64_t pg);
// lab_out nb x n: lab_r of the permutations [r0, r0 + nb)
int sgl_nhood_permute_core(sgl_ctx* c, int64_t n, const int32_t* lab, uint64_t seed, int64_t r0, int64_t nb, int32_t* lab_out);
// counts_out nb x K x K: the tally of nb label vectors; path 0 / 1 / 2, pg 0: the plan's
int sgl_nhood_tally_core(sgl_ctx* c, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* labs, int64_t nb, int K, int drop, int path,
                         int64_t pg, int64_t* counts_out);
// the whole call: any output may be NULL; null_out nperm x K x K; stage_ms (3 values, may be NULL): the stages timed by events
int sgl_nhood_all(sgl_ctx* c, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* lab, int K, int drop, int64_t nperm, uint64_t seed,
                  int64_t batch, int64_t* counts, int64_t* S1, int64_t* S2, int64_t* n_ge, int64_t* n_le, int64_t* null_out, double* stage_ms);

// the interleaved label tables of the permutation tests, made by the neighbourhood unit's keys, sorts and gather in groups of 16
// (kernels_nhood.hip): vector l of a table is out8[((l / 16) n + c) 16 + l % 16]; a slot past the last vector holds label 0.
// dlab / dlabs and out8 are the DEVICE's; nothing synchronises.  A labeller holds the sort buffers of batches of up to `batch`.
struct sgl_nhood_labeller;
int sgl_nhood_labeller_create(sgl_ctx* c, int64_t n, int64_t batch, sgl_nhood_labeller** out);
void sgl_nhood_labeller_free(sgl_nhood_labeller* h);
// lab_r of the permutations [r0, r0 + nb)
int sgl_nhood_labels_permuted(sgl_ctx* c, sgl_nhood_labeller* h, const int32_t* dlab, int64_t n, uint64_t seed, int64_t r0, int64_t nb, uint8_t* out8);
// np given label vectors, vector l at dlabs + l * lab_stride
int sgl_nhood_labels_given(sgl_ctx* c, const int32_t* dlabs, int64_t lab_stride, int64_t n, int64_t np, uint8_t* out8);

// ligand-receptor interactions (kernels_ligrec.hip; include/singlet_hip.h, "Ligand-receptor interactions").  All arrays are the
// HOST's; every call only reads the context (it records what it ran in ligrec_last), allocates its own temporaries and
// synchronises the stream before it returns.  The *_args_check functions hold every refusal and launch nothing.
int sgl_ligrec_args_check(const char* who, const int32_t* lab, int64_t n, int64_t K, const int32_t* genes, int64_t G, int64_t m, const int32_t* lig,
                          const int32_t* rec, int64_t P, int64_t nperm, double threshold, int64_t batch, int64_t ncol);
int sgl_ligrec_sums_args_check(const char* who, const int32_t* labs, int64_t n, int64_t nb, int64_t K, const int32_t* genes, int64_t G, int64_t m,
                               int path, int64_t vpw, int64_t ncol);
int sgl_ligrec_tally_args_check(const char* who, const double* mean_obs, const double* means, int64_t nb, int64_t K, int64_t G, const int32_t* lig,
                                const int32_t* rec, int64_t P);
// the whole call over c->At: any output may be NULL; group_n K; nz, sum, mean G x K (class fastest); score, n_ge P x K x K at
// q + P (a + K b); null_out nperm x P x K x K; stage_ms (3 values, may be NULL): the stages timed by events
int sgl_ligrec_all(sgl_ctx* c, const int32_t* lab, int K, const int32_t* genes, int64_t G, const int32_t* lig, const int32_t* rec, int64_t P,
                   int64_t nperm, uint64_t seed, int64_t batch, int64_t* group_n, int64_t* nz, double* sum, double* mean, double* score, int64_t* n_ge,
                   double* null_out, double* stage_ms);
// sum_out nb x G x K: the sums of nb given label vectors; path 0 / 1 / 2, vpw 0: the plan's
int sgl_ligrec_sums_core(sgl_ctx* c, const int32_t* labs, int64_t nb, int K, const int32_t* genes, int64_t G, int path, int64_t vpw, double* sum_out);
// score_out, n_ge_out P x K x K, null_out nb x P x K x K from the means alone (no matrix is read); any output may be NULL
int sgl_ligrec_tally_core(sgl_ctx* c, const double* mean_obs, const double* means, int64_t nb, int K, int64_t G, const int32_t* lig,
                          const int32_t* rec, int64_t P, double* score_out, int64_t* n_ge_out, double* null_out);

// co-occurrence by distance (kernels_cooccur.hip; include/singlet_hip.h, "Co-occurrence by distance").  All arrays are the HOST's;
// the call reads nothing of the context but its device, stream and pool (it records what it ran in cooccur_last), allocates its
// own temporaries and synchronises the stream before it returns.  The args check holds every refusal, launches nothing and fills
// thr2 (T + 1 doubles) with the squared thresholds.
int sgl_cooccur_args_check(const char* who, const double* c1, const double* c2, int64_t n, const int32_t* lab, int64_t K, const double* r, int64_t T,
                           int64_t grid_mode, int64_t bin_path, int64_t flush_pairs, double* thr2);
// counts T x K x K at a + K b + K^2 t; a knob of 0: the plan's; stage_ms (3 values, may be NULL): the stages timed by events
int sgl_cooccur_core(sgl_ctx* c, const double* c1, const double* c2, int64_t n, const int32_t* lab, int K, const double* r, const double* thr2, int T,
                     int grid_mode, int bin_path, int64_t flush_pairs, int64_t* counts, double* stage_ms);

// gene set enrichment (kernels_gsea.hip; include/singlet_hip.h, "Gene set enrichment").  All arrays are the HOST's; every call
// only reads the context (it records what it ran in gsea_last), allocates its own temporaries and synchronises the stream
// before it returns.  The *_args_check functions hold every refusal and launch nothing.
int sgl_gsea_args_check(const char* who, const double* w, int64_t m, int64_t k, const int64_t* set_ptr, const int32_t* set_genes, int64_t P,
                        int score_type, int64_t nperm, int64_t batch);
int sgl_gsea_null_args_check(const char* who, const double* w, int64_t m, int64_t k, const int32_t* sizes, int64_t n_sizes, int score_type,
                             int64_t r0, int64_t r1, int64_t batch);
// es3: the three planes (pos, neg, std) of P x k observed scores
int sgl_gsea_es(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int64_t* set_ptr, const int32_t* set_genes, int64_t P, double* es3);
// null_out[(f S + si) (r1 - r0) + (r - r0)]; sample[(r - r0) s_max + t]; either may be NULL; batch 0: by the memory budget
int sgl_gsea_null(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int32_t* sizes, int64_t S, int score_type, uint64_t seed, int64_t r0,
                  int64_t r1, int64_t batch, double* null_out, int32_t* sample);
// the five stages and the derived statistics (gsea_host.h); stage_ms (5 values, may be NULL): the stages timed by events
int sgl_gsea_all(sgl_ctx* c, const double* w, int64_t m, int64_t k, const int64_t* set_ptr, const int32_t* set_genes, int64_t P, int score_type,
                 int64_t nperm, uint64_t seed, int64_t batch, double* es, double* nes, double* pval, double* padj, int64_t* n_ge, int64_t* n_le,
                 int64_t* n_side, int32_t* set_size, double* stage_ms);

// label / value transfer along neighbour lists (kernels_knn_transfer.hip; include/singlet_hip.h, "Neighbour index and transfer").
// The refusals of the arguments and of a label list under the caller's name (host arrays), and the transfer itself: every
// pointer is the DEVICE's, idx / dist n_neighbors x nq, any output may be nullptr (labels nullptr: no label outputs; V nullptr:
// no values); it only launches, in the "scale" phase.
int sgl_knn_transfer_args(const char* who, int32_t weighting, int32_t n_neighbors, int64_t n_query, int64_t n_ref, bool has_labels,
                          int32_t n_classes, bool has_values, int32_t n_values);
int sgl_knn_transfer_labels_check(const char* who, const int32_t* labels, int64_t n_ref, int32_t n_classes);
int sgl_knn_transfer_dev(sgl_ctx* c, const int32_t* idx, const double* dist, int K, int64_t nq, const int32_t* labels, int n_classes,
                         const double* V, int n_values, int weighting, int32_t* pred, double* best, double* scores, double* values);

// row-wise rasterisation (kernels_raster.hip): out (nb x ncol, column-major) = means of rows [b n, b n + n), nb >= 1
int k_raster_sparse(hipStream_t s, const DevCSC& A, int64_t n, int64_t nb, double* out);
int k_raster_dense(hipStream_t s, const double* A, int64_t nrow, int64_t ncol, int64_t n, int64_t nb, double* out);
// column gather of a CSC (kernels_subset.hip): D = S[:, sel], sel on the device and checked by the caller, D empty on entry
int k_subset_gather(sgl_ctx* c, const DevCSC& S, const int32_t* sel, int64_t n, DevCSC& D);
// typed ingest (kernels_ingest.hip, sgl_upload_typed): what a convert kernel ORs into its flag word (RANGE / ORDER / FINITE
// are the validator's bits), the LDS sort's capacity in entries (8 LDS bytes per entry: four workgroups fit a CU's
// 160 KiB, two were asked for), and the launchers
#define SGL_INGEST_RANGE 1
#define SGL_INGEST_ORDER 2
#define SGL_INGEST_FINITE 4
#define SGL_INGEST_INEXACT 8     // an int64 value beyond +-2^53
#define SGL_INGEST_OFFSETS 16    // ptr[0] != 0 or ptr decreases (device-space offsets)
#define SGL_INGEST_FRACTION 32   // not a defect: some value has a fraction (report[3] = 0)
#define SGL_INGEST_LDS_CAP 4096
int k_ingest_values(hipStream_t s, const void* src, int x_type, double* dst, int64_t n, int* flag);   // src may be dst for F64
int k_ingest_narrow_index(hipStream_t s, const int64_t* src, int32_t* dst, int64_t n, int64_t extent, int* flag);
int k_ingest_offsets(hipStream_t s, const void* src, int ptr_type, int64_t n1, int64_t* dst, int check, int* flag);
int k_ingest_sort_slices(sgl_ctx* c, DevCSC& M, int64_t* n_short, int64_t* n_long);
// device transpose (kernels_transpose.hip): T (empty on entry) = t(A), rows ascending; <= 0: the default batch size
int sgl_device_transpose_into(sgl_ctx* c, const DevCSC& A, DevCSC& T, int64_t max_batch_entries);
// upload of A alone (an empty At) validating the structure only, the values as they are (singlet_hip.hip)
void sgl_matrix_clear(sgl_ctx* c);   // drops the fit and the resident matrix (the team upload, after one rank refused)
int sgl_upload_A_structure(sgl_ctx* c, const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol);

// graph convolution (kernels_graph.hip): Y = X G, X and Y k x n column-major (Y must not alias X)
int k_graph_conv(hipStream_t s, DevGraph& g, const double* X, double* Y, int k);
int k_graph_pack(hipStream_t s, DevGraph& g, const double* X, int k, int rank);   // X(:, g.exp) -> block `rank` of g.halo

// NNLS
#define SGL_NNLS_MAX_PASSES 10
// below this many columns the GPU is not full anyway: one pass; 2^18, 2^17 for the two-lane solve (env SGL_NNLS_REPACK_MIN_COLS overrides, tests)
int64_t nnls_repack_min_cols(bool two_lane);
int nnls_gram_stride(int KP);  // row stride of the padded Gram the lane kernel expects
int nnls_lane_kp(int k, double L1);   // padded rank of the lane solve serving rank k <= SGL_LANE_NNLS_MAX_K
int nnls_scratch_alloc(NnlsScratch& sc, int64_t cap, int k);
void nnls_scratch_free(NnlsScratch& sc);
// B is destroyed (and used as the spill space of b between passes).  scr == nullptr: one pass.
int k_nnls_lane(hipStream_t s, const double* Gpad, int KP, double* B, double* X, const int64_t* col_nnz,
                int k, int64_t ncols, double L1, double L2, unsigned long long* sweep_counter, const NnlsScratch* scr,
                bool pack_by_sweeps = false);
int nnls_pack_alloc(NnlsScratch& sc, int64_t ncols);
// ranks 129 - 256, shared Gram, all columns of the shard: four lanes per column, waves packed by the previous solve's sweep counts
int k_nnls_quarter_packed(hipStream_t s, const double* G, const double* B, double* X, const int64_t* col_nnz, int k, int64_t ncols, double L1,
                          double L2, unsigned long long* sweep_counter, const NnlsScratch* scr);
// few columns against a shared Gram (k <= 64): four columns per wave, the Gram staged in LDS; B is read only
int k_nnls_quad_shared(hipStream_t s, const double* G, const double* B, double* X, const int64_t* col_nnz, int k, int64_t ncols,
                       double L1, double L2, unsigned long long* sweep_counter);
// THE DISPATCH of every solve that is not the lane / two-lane / shared-quad kernel (until round 6 named k_nnls_wave, after its
// last resort): per-column Grams (gstride = k * k: the masked path, one GPU AND the gene blocks of a team, multi.hip) run four
// columns per wave -- nnls_quad_kernel (triangles in LDS, k < 40 / 47) or nnls_quad_global_kernel (k <= 112 / 128) -- and only
// above that, or with a shared Gram above k = 128 (gstride = 0), the wave-per-column kernel
int k_nnls_percol(hipStream_t s, const double* G, int64_t gstride, const double* B, double* X, const int64_t* col_nnz,
                int k, int64_t ncols, double L1, double L2, unsigned long long* sweep_counter);

// masked path
int k_mask_gram_cols(hipStream_t s, int64_t col0, int64_t ncols, int32_t nrow, const int64_t* col_nnz,
                     const double* F, const double* G, int k, uint64_t seed, uint64_t inv_density, int mask_t,
                     int64_t col_offset, int64_t row_offset, double* Gcols, const DevMaskList* L = nullptr);
int sgl_mask_list_build(sgl_ctx* c, DevMaskList& L, int64_t ncol, int32_t nrow, uint64_t seed, uint64_t inv_density, int mask_t,
                        int64_t col_offset, int64_t row_offset);
void sgl_mask_list_free(DevMaskList& L);
// the lists of orientation `which` (0: cells, 1: genes) under this key in c->ML[which]: the current ones, ones kept from an
// earlier fit, or built now -- the lists they replace are kept (R's rank search refits one matrix with the seeds
// seed + 1 .. seed + n_replicates over and over, R/ard_nmf.R:95-160; the mask does not depend on the rank)
int sgl_mask_list_select(sgl_ctx* c, int which, int64_t ncol, int32_t nrow, uint64_t seed, uint64_t inv_density, int mask_t,
                         int64_t col_offset, int64_t row_offset);
void sgl_mask_lists_free_all(sgl_ctx* c);
bool sgl_mask_lists_release_kept(sgl_ctx* c);   // memory pressure: drop the kept (not the current) masks; true if anything was freed
int k_mask_gram_finalize(hipStream_t s, const double* G, const double* S, int k, int64_t ncols, double* out);
int k_tri_pack(hipStream_t s, const double* S, int k, int64_t ncols, double* tri);   // lower triangles of ncols symmetric k x k blocks
int k_mask_gram_finalize_tri(hipStream_t s, const double* G, const double* tri, int k, int64_t ncols, double* out);
int k_mse_test(sgl_ctx* c, const double* Wd, const double* H, int k, uint64_t seed, uint64_t inv_density,
               double* out_dev);
// its two halves, shared with sgl_op_mse_test_cells: the matrix values at the listed entries of the cell-side lists (no-op once
// there or refused), and the per-cell losses by the named kernel family (0 hashing, 1 lists + window, 2 listed values)
int k_mask_vals(sgl_ctx* c, DevMaskList& L);
int k_mse_test_cells(sgl_ctx* c, const double* Wd, const double* H, int k, uint64_t seed, uint64_t inv_density, int variant,
                     const DevMaskList* L, double* losses);
int k_wd(hipStream_t s, const double* W, const double* d, int k, int64_t cols, double* Wd);

// ---- device-side hash (rng::rand, src/singlet.cpp:30-64) ------------------
__device__ __forceinline__ uint64_t sgl_rand2(uint64_t state, uint64_t i, uint64_t j) {
    i ^= i << 19;
    i ^= i >> 7;
    i ^= i << 36;
    uint64_t x = state + i;
    x ^= x << 38;
    x ^= x >> 13;
    x ^= x << 23;
    j ^= j >> 7;
    j ^= j << 23;
    j ^= j >> 8;
    x += j;
    x ^= x >> 7;
    x ^= x << 53;
    x ^= x >> 4;
    return x;
}
// the i-only half of the hash, hoistable out of loops over j
__device__ __forceinline__ uint64_t sgl_rand_i(uint64_t state, uint64_t i) {
    i ^= i << 19;
    i ^= i >> 7;
    i ^= i << 36;
    uint64_t x = state + i;
    x ^= x << 38;
    x ^= x >> 13;
    x ^= x << 23;
    return x;
}
__device__ __forceinline__ uint64_t sgl_rand_j(uint64_t xi, uint64_t j) {
    j ^= j >> 7;
    j ^= j << 23;
    j ^= j >> 8;
    uint64_t x = xi + j;
    x ^= x >> 7;
    x ^= x << 53;
    x ^= x >> 4;
    return x;
}
// `x % d == 0` for a kernel-uniform divisor without a 64-bit division per test (hipcc expands a runtime u64
// modulo into a long software routine, the bulk of the hashing cost of the masked path).  With d = 2^s * o
// (o odd):  d | x  <=>  the low s bits of x are zero  and  o | (x >> s);  and for odd o (Granlund-Montgomery)
// o | y  <=>  y * o^-1 (mod 2^64) <= floor((2^64 - 1) / o).  One 64-bit low multiply and a compare instead of
// round 1's multiply-high + multiply-low + two corrections.  Exact for every x and d >= 1 (d = 0 is rejected
// on the host); tests/test_gpu_ops.py::test_mask_bit_exact holds it against the oracle's `%`.
struct SglDiv {
    uint64_t d, low_mask, inv, lim;
    int shift;
};
static inline SglDiv sgl_div_make(uint64_t d) {
    SglDiv v{d, 0ull, 1ull, ~0ull, 0};
    if (d <= 1) return v;
    uint64_t o = d;
    while ((o & 1ull) == 0) { o >>= 1; ++v.shift; }
    v.low_mask = (1ull << v.shift) - 1ull;
    uint64_t inv = o;                       // Newton: doubles the correct low bits each step (3 -> 6 -> ... -> 96)
    for (int q = 0; q < 6; ++q) inv *= 2ull - o * inv;
    v.inv = inv;
    v.lim = ~0ull / o;
    return v;
}
__device__ __forceinline__ bool sgl_divides(uint64_t x, SglDiv dv) {
    if (dv.d <= 1) return true;
    if ((x & dv.low_mask) != 0ull) return false;
    return (x >> dv.shift) * dv.inv <= dv.lim;
}
__device__ __forceinline__ bool sgl_draw(uint64_t state, uint64_t i, uint64_t j, SglDiv inv_density) {
    return sgl_divides(sgl_rand2(state, i, j), inv_density);
}
