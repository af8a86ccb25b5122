// Host logic of the layout transform (include/singlet_hip.h, "Layout transform") that makes no HIP call: the argument rules,
// the validation of the query lists, of the memberships and of the positions, the kernel instance, the report of
// sgl_umap_transform_info and the cut of a call's epochs into launches.  Plain C++ over plain pointers, so
// tests/umap_transform_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include "umap_host.h"

#define UMAP_TRANSFORM_EPOCHS_PER_LAUNCH 128      // a call's epochs are cut into launches of at most this many
#define UMAP_TRANSFORM_MAX_OFFSET (1ll << 55)     // query_offset + n_query stays at or below it: 256 * index + slot fits 63 bits

enum UtDefect {
    UT_OK = 0,
    UT_ARGS_NULL,
    UT_ARGS_NQ,            // n_query < 0
    UT_ARGS_K,             // K outside [1, 256]
    UT_ARGS_NREF,          // n_ref outside [1, 2^31)
    UT_ARGS_DIM,
    UT_ARGS_AB,
    UT_ARGS_EPOCHS,
    UT_ARGS_RANGE,         // not 1 <= t_first <= t_last <= n_epochs
    UT_ARGS_ALPHA,
    UT_ARGS_NEG,
    UT_ARGS_OFFSET,        // query_offset < 0 or query_offset + n_query > 2^55
    UT_INDEX_RANGE,        // an index outside [-1, n_ref)
    UT_VALID_AFTER_PAD,    // a valid slot behind a padding slot
    UT_INDEX_REPEATED,
    UT_DIST_NOT_FINITE,
    UT_DIST_NEGATIVE,
    UT_DIST_ORDER,
    UT_W_RANGE,            // a membership of a valid slot outside [0, 1]
    UT_YREF_NOT_FINITE,    // Yref[*query] (column-major position)
    UT_YIN_NOT_FINITE,     // Yin of query *query, component *slot
};

inline const char* ut_defect_text(UtDefect f) {
    switch (f) {
        case UT_ARGS_NULL: return "a NULL array";
        case UT_ARGS_NQ: return "n_query must be >= 0";
        case UT_ARGS_K: return "the number of neighbours must lie in [1, 256]";
        case UT_ARGS_NREF: return "n_ref must lie in [1, 2^31)";
        case UT_ARGS_DIM: return "dim must lie in [1, 8]";
        case UT_ARGS_AB: return "a and b must be finite and > 0";
        case UT_ARGS_EPOCHS: return "n_epochs must lie in [1, 2^20]";
        case UT_ARGS_RANGE: return "the epochs must satisfy 1 <= t_first <= t_last <= n_epochs";
        case UT_ARGS_ALPHA: return "alpha0 must be finite and > 0";
        case UT_ARGS_NEG: return "neg_rate must lie in [0, 255]";
        case UT_ARGS_OFFSET: return "query_offset must be >= 0 and query_offset + n_query at most 2^55";
        case UT_INDEX_RANGE: return "index outside [-1, n_ref)";
        case UT_VALID_AFTER_PAD: return "a valid slot behind a padding slot";
        case UT_INDEX_REPEATED: return "index repeated in the list";
        case UT_DIST_NOT_FINITE: return "distance is not finite";
        case UT_DIST_NEGATIVE: return "distance is negative";
        case UT_DIST_ORDER: return "distances not ascending within the list";
        case UT_W_RANGE: return "membership outside [0, 1]";
        case UT_YREF_NOT_FINITE: return "a reference position is not finite";
        case UT_YIN_NOT_FINITE: return "a query position is not finite";
        default: return "ok";
    }
}

// The scalar arguments, in the order of the enum.  `layout`: dim, a, b, n_epochs, alpha0, neg_rate, the epoch range and the
// offset are checked too (sgl_c_fuzzy_query has none of them).
inline UtDefect ut_check_scalars(int64_t n_query, int32_t K, int64_t n_ref, bool layout, int32_t dim, double a, double b, int32_t n_epochs,
                                 int64_t t_first, int64_t t_last, double alpha0, int32_t neg_rate, int64_t query_offset) {
    if (n_query < 0) return UT_ARGS_NQ;
    if (K < 1 || K > UMAP_MAX_NEIGHBORS) return UT_ARGS_K;
    if (n_ref < 1 || n_ref > (int64_t)INT32_MAX) return UT_ARGS_NREF;
    if (!layout) return UT_OK;
    if (dim < 1 || dim > UMAP_MAX_DIM) return UT_ARGS_DIM;
    if (!umap_positive_finite(a) || !umap_positive_finite(b)) return UT_ARGS_AB;
    if (n_epochs < 1 || n_epochs > UMAP_MAX_EPOCHS) return UT_ARGS_EPOCHS;
    if (t_first < 1 || t_first > t_last || t_last > n_epochs) return UT_ARGS_RANGE;
    if (!umap_positive_finite(alpha0)) return UT_ARGS_ALPHA;
    if (neg_rate < 0 || neg_rate > UMAP_MAX_NEG_RATE) return UT_ARGS_NEG;
    if (query_offset < 0 || query_offset > UMAP_TRANSFORM_MAX_OFFSET || n_query > UMAP_TRANSFORM_MAX_OFFSET - query_offset) return UT_ARGS_OFFSET;
    return UT_OK;
}

// The lists, K x n_query column-major; dist == NULL (the stage operator) checks the indices only, W != NULL the memberships
// of the valid slots.  Per slot in the order of the enum, the queries ascending; *query / *slot name the first offender.
inline UtDefect ut_check_lists(const int32_t* idx, const double* dist, const double* W, int64_t n_query, int32_t K, int64_t n_ref,
                               int64_t* query, int32_t* slot) {
    *query = -1;
    *slot = -1;
    std::vector<int32_t> seen((size_t)K);
    for (int64_t q = 0; q < n_query; ++q) {
        const int32_t* li = idx + q * K;
        int32_t valid = 0;
        bool padded = false;
        for (int32_t s = 0; s < K; ++s) {
            const int64_t r = li[s];
            UtDefect f = UT_OK;
            if (r < -1 || r >= n_ref) f = UT_INDEX_RANGE;
            else if (r == -1) padded = true;
            else if (padded) f = UT_VALID_AFTER_PAD;
            else if (dist) {
                const double d = dist[q * K + s];
                if (!(d - d == 0.0)) f = UT_DIST_NOT_FINITE;
                else if (d < 0.0) f = UT_DIST_NEGATIVE;
                else if (s > 0 && d < dist[q * K + s - 1]) f = UT_DIST_ORDER;
            }
            if (f == UT_OK && r >= 0 && W) {
                const double w = W[q * K + s];
                if (!(w >= 0.0 && w <= 1.0)) f = UT_W_RANGE;
            }
            if (f != UT_OK) { *query = q; *slot = s; return f; }
            if (r >= 0) seen[(size_t)valid++] = (int32_t)r;
        }
        // a repeated index: named by the later of the two slots
        if (valid > 1) {
            std::vector<int32_t> srt(seen.begin(), seen.begin() + valid);
            std::sort(srt.begin(), srt.end());
            if (std::adjacent_find(srt.begin(), srt.end()) != srt.end()) {
                for (int32_t s = 1; s < valid; ++s)
                    for (int32_t u = 0; u < s; ++u)
                        if (li[u] == li[s]) { *query = q; *slot = s; return UT_INDEX_REPEATED; }
            }
        }
    }
    return UT_OK;
}

// count doubles, all finite?  *pos names the first that is not.
inline bool ut_all_finite(const double* v, int64_t count, int64_t* pos) {
    for (int64_t q = 0; q < count; ++q)
        if (!(v[q] - v[q] == 0.0)) { *pos = q; return false; }
    *pos = -1;
    return true;
}

// Yin (dim x n_query): the columns of the queries with a valid slot must be finite; the others are not read.
inline bool ut_yin_finite(const double* Yin, const int32_t* idx, int64_t n_query, int32_t K, int32_t dim, int64_t* query, int32_t* comp) {
    for (int64_t q = 0; q < n_query; ++q) {
        if (idx[q * K] < 0) continue;
        for (int32_t f = 0; f < dim; ++f)
            if (!(Yin[q * dim + f] - Yin[q * dim + f] == 0.0)) { *query = q; *comp = f; return false; }
    }
    *query = -1;
    *comp = -1;
    return true;
}

// What sgl_umap_transform_info reports of a call.
struct UtPlan {
    int instance = 0;
    int64_t widest = 0;      // valid slots of the widest list
    int64_t empty = 0;       // queries without a valid slot
    int64_t launches = 0;    // of the transform kernel
};

// The epochs of one launch: UMAP_TRANSFORM_EPOCHS_PER_LAUNCH, or what the profiling switch
// SGL_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH asks for (text; a whole number in [1, UMAP_TRANSFORM_EPOCHS_PER_LAUNCH], anything else
// is ignored).  The result of a call does not depend on it.
inline int64_t ut_epochs_per_launch(const char* text) {
    if (!text || !*text) return UMAP_TRANSFORM_EPOCHS_PER_LAUNCH;
    int64_t v = 0;
    for (const char* c = text; *c; ++c) {
        if (*c < '0' || *c > '9' || v > UMAP_TRANSFORM_EPOCHS_PER_LAUNCH) return UMAP_TRANSFORM_EPOCHS_PER_LAUNCH;
        v = 10 * v + (*c - '0');
    }
    return v >= 1 && v <= UMAP_TRANSFORM_EPOCHS_PER_LAUNCH ? v : UMAP_TRANSFORM_EPOCHS_PER_LAUNCH;
}

inline int64_t ut_launch_count(int64_t t_first, int64_t t_last, int64_t per = UMAP_TRANSFORM_EPOCHS_PER_LAUNCH) {
    return (t_last - t_first + per) / per;
}

inline UtPlan ut_plan(const int32_t* idx, int64_t n_query, int32_t K, int32_t dim, double b, int64_t t_first, int64_t t_last) {
    UtPlan P;
    for (int64_t q = 0; q < n_query; ++q) {
        int32_t valid = 0;
        while (valid < K && idx[q * K + valid] >= 0) ++valid;
        P.widest = std::max<int64_t>(P.widest, valid);
        if (valid == 0) ++P.empty;
    }
    P.instance = umap_instance(dim, b);
    P.launches = ut_launch_count(t_first, t_last);
    return P;
}

// The launches of the epochs t_first .. t_last: launch(first, last) with last - first < per, in ascending order, each epoch
// in exactly one.  A failing launch ends the loop with its status; returns the number issued.
template <typename F>
inline int64_t ut_run_launches(int64_t t_first, int64_t t_last, F launch, int* rc, int64_t per = UMAP_TRANSFORM_EPOCHS_PER_LAUNCH) {
    int64_t issued = 0;
    *rc = 0;
    for (int64_t t = t_first; t <= t_last; t += per) {
        const int64_t last = std::min<int64_t>(t + per - 1, t_last);
        *rc = launch(t, last);
        if (*rc != 0) return issued;
        ++issued;
    }
    return issued;
}
