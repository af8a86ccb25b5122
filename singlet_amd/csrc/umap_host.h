// Host logic of the layout stage (include/singlet_hip.h, "Layout") that makes no HIP call: the argument rules and the
// validation of the k-NN lists (sgl_c_fuzzy_graph) and of the graph (sgl_c_umap_layout), the exact maximum weight, the
// learning rate of an epoch, the firing rule, the choice of the kernel instance, the chunk plan of the columns and the split
// of the fuzzy graph's vertices into the LDS merge and its fallback.  Plain C++ over plain pointers, so
// tests/umap_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define UMAP_MAX_NEIGHBORS 256
#define UMAP_MAX_DIM 8
#define UMAP_MAX_EPOCHS (1 << 20)
#define UMAP_MAX_NEG_RATE 255
#define UMAP_CHUNK 64             // stored entries of a column one wave looks at per step (one per lane)
#define UMAP_MERGE_WIDTH 512      // own slots plus incoming entries of a vertex that one wave sorts in LDS (4 KiB of keys, as Clustering)
#define UMAP_SUM_BLOCK 1024       // the global distance sum runs sequentially inside blocks of this many terms (as Clustering)

// ------------------------------------------------------------------------------------------------------- the fuzzy graph
enum FuzzyDefect {
    FUZZY_OK = 0,
    FUZZY_ARGS_NULL,       // a NULL input or count output
    FUZZY_ARGS_K,          // K outside [2, 256]
    FUZZY_ARGS_N,          // n outside [1, 2^31)
    FUZZY_INDEX_RANGE,     // an index outside [0, n)
    FUZZY_INDEX_REPEATED,  // an index twice in one list
    FUZZY_DIST_NOT_FINITE,
    FUZZY_DIST_NEGATIVE,
    FUZZY_DIST_ORDER,      // below the distance before it in its list
};

// The refusals of sgl_c_fuzzy_graph, in the order of the enum per entry, the lists in ascending cell; *cell / *slot name the
// first offending entry.
inline FuzzyDefect fuzzy_check(const int32_t* idx, const double* dist, int64_t n, int32_t K, int64_t* cell, int32_t* slot) {
    *cell = -1;
    *slot = -1;
    if (!idx || !dist) return FUZZY_ARGS_NULL;
    if (K < 2 || K > UMAP_MAX_NEIGHBORS) return FUZZY_ARGS_K;
    if (n < 1 || n > (int64_t)INT32_MAX) return FUZZY_ARGS_N;
    std::vector<int32_t> stamp((size_t)n, -1);   // the last cell whose list held this index
    for (int64_t j = 0; j < n; ++j) {
        for (int32_t q = 0; q < K; ++q) {
            const int64_t r = idx[j * K + q];
            const double d = dist[j * K + q];
            FuzzyDefect f = FUZZY_OK;
            if (r < 0 || r >= n) f = FUZZY_INDEX_RANGE;
            else if (stamp[(size_t)r] == (int32_t)j) f = FUZZY_INDEX_REPEATED;
            else if (!(d - d == 0.0)) f = FUZZY_DIST_NOT_FINITE;
            else if (d < 0.0) f = FUZZY_DIST_NEGATIVE;
            else if (q > 0 && d < dist[j * K + q - 1]) f = FUZZY_DIST_ORDER;
            if (f != FUZZY_OK) { *cell = j; *slot = q; return f; }
            stamp[(size_t)r] = (int32_t)j;
        }
    }
    return FUZZY_OK;
}

inline const char* fuzzy_defect_text(FuzzyDefect f) {
    switch (f) {
        case FUZZY_ARGS_NULL: return "a NULL array";
        case FUZZY_ARGS_K: return "the number of neighbours must lie in [2, 256]";
        case FUZZY_ARGS_N: return "the number of cells must lie in [1, 2^31)";
        case FUZZY_INDEX_RANGE: return "index outside [0, n)";
        case FUZZY_INDEX_REPEATED: return "index repeated in the list";
        case FUZZY_DIST_NOT_FINITE: return "distance is not finite";
        case FUZZY_DIST_NEGATIVE: return "distance is negative";
        case FUZZY_DIST_ORDER: return "distances not ascending within the list";
        default: return "ok";
    }
}

// The vertices whose merged list (the K slots of the own list plus the incoming entries) fits the LDS merge, and those that
// take the fallback; soff = the offsets of the fallback vertices' keys.  Every vertex is in one of the two.
inline void fuzzy_split(const int64_t* indeg, int64_t n, int32_t K, std::vector<int32_t>& fast, std::vector<int32_t>& slow,
                        std::vector<int64_t>& soff) {
    fast.clear();
    slow.clear();
    soff.assign(1, 0);
    for (int64_t v = 0; v < n; ++v) {
        const int64_t len = (int64_t)K + indeg[v];
        if (len <= UMAP_MERGE_WIDTH) {
            fast.push_back((int32_t)v);
        } else {
            slow.push_back((int32_t)v);
            soff.push_back(soff.back() + len);
        }
    }
}

// Column counts -> 32-bit column pointers; false when the graph would hold 2^31 entries or more (*nnz is set all the same).
inline bool fuzzy_pointers(const int32_t* cnt, int64_t n, int32_t* p_out, int64_t* nnz) {
    int64_t total = 0;
    for (int64_t v = 0; v < n; ++v) total += cnt[v];
    *nnz = total;
    if (total > (int64_t)INT32_MAX) return false;
    p_out[0] = 0;
    for (int64_t v = 0; v < n; ++v) p_out[v + 1] = p_out[v] + cnt[v];
    return true;
}

// ------------------------------------------------------------------------------------------------------------ the layout
enum UmapDefect {
    UMAP_OK = 0,
    UMAP_ARGS_NULL,
    UMAP_ARGS_N,           // n outside [1, 2^31)
    UMAP_ARGS_DIM,         // dim outside [1, 8]
    UMAP_ARGS_AB,          // a or b not finite or not > 0
    UMAP_ARGS_EPOCHS,      // n_epochs outside [1, 2^20]
    UMAP_ARGS_EPOCH,       // (operator) t outside [1, n_epochs]
    UMAP_ARGS_ALPHA,       // alpha0 not finite or not > 0
    UMAP_ARGS_NEG,         // neg_rate outside [0, 255]
    UMAP_ARGS_P0,
    UMAP_ARGS_P_DECREASES, // p[*pos + 1] < p[*pos]
    UMAP_Y_NOT_FINITE,     // Y0[*pos] (column-major position) is not finite
    UMAP_ROW_RANGE,        // entry *pos of column *col
    UMAP_ROW_ORDER,
    UMAP_WEIGHT_NOT_FINITE,
    UMAP_WEIGHT_NEGATIVE,
};

inline bool umap_positive_finite(double v) { return v > 0.0 && v < INFINITY; }

// The refusals of sgl_c_umap_layout and sgl_op_umap_epoch (t = 0: the whole layout, no epoch to check), in the order of the
// enum; the graph's entries in column-major order.  *pos / *col name the offender.
inline UmapDefect umap_check(const double* Gx, const int32_t* Gi, const int32_t* Gp, int64_t n, const double* Y0, int32_t dim, double a,
                             double b, int32_t n_epochs, double alpha0, int32_t neg_rate, int64_t t, bool is_op, int64_t* pos,
                             int64_t* col) {
    *pos = -1;
    *col = -1;
    if (!Gp || !Y0) return UMAP_ARGS_NULL;
    if (n < 1 || n > (int64_t)INT32_MAX) return UMAP_ARGS_N;
    if (dim < 1 || dim > UMAP_MAX_DIM) return UMAP_ARGS_DIM;
    if (!umap_positive_finite(a) || !umap_positive_finite(b)) return UMAP_ARGS_AB;
    if (n_epochs < 1 || n_epochs > UMAP_MAX_EPOCHS) return UMAP_ARGS_EPOCHS;
    if (is_op && (t < 1 || t > n_epochs)) return UMAP_ARGS_EPOCH;
    if (!umap_positive_finite(alpha0)) return UMAP_ARGS_ALPHA;
    if (neg_rate < 0 || neg_rate > UMAP_MAX_NEG_RATE) return UMAP_ARGS_NEG;
    if (Gp[0] != 0) return UMAP_ARGS_P0;
    for (int64_t c = 0; c < n; ++c)
        if (Gp[c + 1] < Gp[c]) { *pos = c; return UMAP_ARGS_P_DECREASES; }
    if (Gp[n] > 0 && (!Gi || !Gx)) return UMAP_ARGS_NULL;
    for (int64_t q = 0; q < n * dim; ++q)
        if (!(Y0[q] - Y0[q] == 0.0)) { *pos = q; return UMAP_Y_NOT_FINITE; }
    for (int64_t c = 0; c < n; ++c)
        for (int64_t e = Gp[c]; e < Gp[c + 1]; ++e) {
            UmapDefect f = UMAP_OK;
            if (Gi[e] < 0 || Gi[e] >= n) f = UMAP_ROW_RANGE;
            else if (e > Gp[c] && Gi[e - 1] >= Gi[e]) f = UMAP_ROW_ORDER;
            else if (!(Gx[e] - Gx[e] == 0.0)) f = UMAP_WEIGHT_NOT_FINITE;
            else if (Gx[e] < 0.0) f = UMAP_WEIGHT_NEGATIVE;
            if (f != UMAP_OK) { *pos = e; *col = c; return f; }
        }
    return UMAP_OK;
}

inline const char* umap_defect_text(UmapDefect f) {
    switch (f) {
        case UMAP_ARGS_NULL: return "a NULL array";
        case UMAP_ARGS_N: return "the number of vertices must lie in [1, 2^31)";
        case UMAP_ARGS_DIM: return "dim must lie in [1, 8]";
        case UMAP_ARGS_AB: return "a and b must be finite and > 0";
        case UMAP_ARGS_EPOCHS: return "n_epochs must lie in [1, 2^20]";
        case UMAP_ARGS_EPOCH: return "the epoch must lie in [1, n_epochs]";
        case UMAP_ARGS_ALPHA: return "alpha0 must be finite and > 0";
        case UMAP_ARGS_NEG: return "neg_rate must lie in [0, 255]";
        case UMAP_ARGS_P0: return "invalid column pointer array (p[0] is not 0)";
        case UMAP_ARGS_P_DECREASES: return "invalid column pointer array: p decreases";
        case UMAP_Y_NOT_FINITE: return "a start position is not finite";
        case UMAP_ROW_RANGE: return "row index outside [0, n)";
        case UMAP_ROW_ORDER: return "row indices not strictly ascending within the column";
        case UMAP_WEIGHT_NOT_FINITE: return "weight is not finite";
        case UMAP_WEIGHT_NEGATIVE: return "weight is negative";
        default: return "ok";
    }
}

// The exact maximum of the stored weights (+0.0 without entries); the weights are finite and >= 0.
inline double umap_w_max(const double* Gx, int64_t nnz) {
    double m = 0.0;
    for (int64_t e = 0; e < nnz; ++e)
        if (Gx[e] > m) m = Gx[e];
    return m;
}

// alpha_t = alpha0 * (1.0 - (t - 1) / n_epochs), t 1-based: one division, one subtraction, one product.
inline double umap_alpha(double alpha0, int64_t t, int32_t n_epochs) {
    return alpha0 * (1.0 - (double)(t - 1) / (double)n_epochs);
}

// Entry of weight w fires in epoch t (1-based) iff floor(t * r) > floor((t - 1) * r) with r = w / w_max (w_max > 0).
inline bool umap_fires(double w, double w_max, int64_t t) {
    const double r = w / w_max;
    return floor((double)t * r) > floor((double)(t - 1) * r);
}

// The kernel instance: 2 * (0: dim 2, 1: dim 3, 2: the generic loop) + (b == 1.0 exactly: no pow).
inline int umap_instance(int32_t dim, double b) { return 2 * (dim == 2 ? 0 : dim == 3 ? 1 : 2) + (b == 1.0 ? 1 : 0); }

// The chunk plan: a wave takes a column in steps of UMAP_CHUNK stored entries and carries the sums from step to step.
struct UmapPlan {
    int64_t widest = 0;        // stored entries of the widest column
    int64_t multi_chunk = 0;   // columns of more than one step
    int64_t epochs = 0;
    int instance = 0;
};
inline UmapPlan umap_plan(const int32_t* Gp, int64_t n, int32_t dim, double b, int32_t n_epochs) {
    UmapPlan P;
    for (int64_t c = 0; c < n; ++c) {
        const int64_t len = (int64_t)Gp[c + 1] - Gp[c];
        P.widest = std::max(P.widest, len);
        if (len > UMAP_CHUNK) ++P.multi_chunk;
    }
    P.epochs = n_epochs;
    P.instance = umap_instance(dim, b);
    return P;
}

// The epoch loop of the whole layout: epoch(t, alpha_t, from, to) for t = 1 .. n_epochs with the two position buffers
// swapping; returns the buffer (0 or 1) that holds the result.  A failing epoch ends the loop with its status in *rc.
template <typename F>
inline int umap_run_epochs(int32_t n_epochs, double alpha0, F epoch, int* rc) {
    int cur = 0;
    *rc = 0;
    for (int64_t t = 1; t <= n_epochs; ++t) {
        *rc = epoch(t, umap_alpha(alpha0, t, n_epochs), cur, 1 - cur);
        if (*rc != 0) return cur;
        cur = 1 - cur;
    }
    return cur;
}
