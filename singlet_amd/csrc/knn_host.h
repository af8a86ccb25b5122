// Host logic of sgl_knn and sgl_knn_metric (include/singlet_hip.h) that makes no HIP call: the argument rules, the check of
// `dims`, the metric's rule and the launch plan -- kernel instance, queries per workgroup, reference segments, where the
// candidate lists live.  Plain C++ over plain pointers, so tests/knn_host_main.cpp and tests/knn_metric_host_main.cpp compile
// it alone under -fsanitize=address,undefined and run it on the CPU.
#pragma once
#include <stdint.h>

#define KNN_MAX_RANK 1024        // SGL_MAX_K, restated so that this header stands alone
#define KNN_MAX_NEIGHBORS 256
#define KNN_REG_MAX_DIMS 64      // up to here a lane keeps its queries' coordinates in registers
#define KNN_LDS_MAX_NEIGHBORS 32 // up to here the candidate lists live in LDS, above in global scratch
#define KNN_MAX_SEGMENTS 64
#define KNN_TARGET_WAVES 1024    // one wave per SIMD of 256 CUs: with fewer query blocks the references are cut into segments
#define KNN_MIN_SEGMENT_REFS 1024
#define KNN_GENERIC_INSTANCE 4

enum KnnArgError {
    KNN_ARGS_OK = 0,
    KNN_ARGS_RANK,         // k outside [1, 1024]
    KNN_ARGS_NREF,         // n_ref < 1 or >= 2^31
    KNN_ARGS_NQUERY,       // n_query < 0
    KNN_ARGS_NEIGHBORS,    // n_neighbors < 1, > 256 or > n_ref
    KNN_ARGS_NDIMS,        // dims given with n_dims outside [1, k]
    KNN_ARGS_DIM_RANGE,    // dims[*pos] = *value outside [0, k)
    KNN_ARGS_DIM_REPEAT,   // dims[*pos] = *value occurred at a lower position
};

// The refusals of sgl_knn that need no device, in the order the header lists them; *pos / *value name the offending entry
// of dims (first in list order).  dims == nullptr: all k dimensions in stored order, n_dims is not read.
inline KnnArgError knn_check_args(int32_t k, int64_t n_ref, int64_t n_query, const int32_t* dims, int32_t n_dims, int32_t n_neighbors,
                                  int32_t* pos, int32_t* value) {
    *pos = -1;
    *value = 0;
    if (n_neighbors < 1 || n_neighbors > KNN_MAX_NEIGHBORS) return KNN_ARGS_NEIGHBORS;
    if (k < 1 || k > KNN_MAX_RANK) return KNN_ARGS_RANK;
    if (n_ref < 1 || n_ref > (int64_t)INT32_MAX) return KNN_ARGS_NREF;
    if ((int64_t)n_neighbors > n_ref) return KNN_ARGS_NEIGHBORS;
    if (n_query < 0) return KNN_ARGS_NQUERY;
    if (!dims) return KNN_ARGS_OK;
    if (n_dims < 1 || n_dims > k) return KNN_ARGS_NDIMS;
    uint64_t seen[KNN_MAX_RANK / 64] = {0};
    for (int32_t q = 0; q < n_dims; ++q) {
        const int32_t d = dims[q];
        *pos = q;
        *value = d;
        if (d < 0 || d >= k) return KNN_ARGS_DIM_RANGE;
        if (seen[d >> 6] & (1ull << (d & 63))) return KNN_ARGS_DIM_REPEAT;
        seen[d >> 6] |= 1ull << (d & 63);
    }
    *pos = -1;
    *value = 0;
    return KNN_ARGS_OK;
}

// The metric of sgl_knn_metric: 0 is sgl_knn's own code, 1 and 2 rank by 1 - the dot of the unit columns.
#define KNN_METRIC_EUCLIDEAN 0
#define KNN_METRIC_COSINE 1
#define KNN_METRIC_CORRELATION 2   // cosine of the columns centred by their own mean
#define KNN_METRIC_MAX 2

// The one refusal sgl_knn_metric adds: it comes after knn_check_args and before anything is launched (for the one-shot
// form before a context is made); the message names the value and [0, KNN_METRIC_MAX].
inline bool knn_metric_ok(int32_t metric) { return metric >= KNN_METRIC_EUCLIDEAN && metric <= KNN_METRIC_MAX; }

// One workgroup is one wave; lane l owns queries_per_lane queries.  Instances 0 .. 3 keep the coordinates in registers for
// n_dims in [1, 8], [9, 16], [17, 32] (two queries per lane) and [33, 64] (one: two would need 256 VGPRs for the
// coordinates alone); instance 4 is the generic kernel of every rank above.
struct KnnPlan {
    int instance;
    int queries_per_lane;
    int queries_per_wg;
    int64_t query_blocks;
    int segments;          // the references [s * segment_refs, min((s + 1) * segment_refs, n_ref)) go to grid row s
    int64_t segment_refs;
    int lists_global;      // 0: candidate lists in LDS; 1: in global scratch
    int64_t lds_bytes;     // dynamic LDS of one workgroup
};

inline int knn_instance(int n_dims) {
    return n_dims <= 8 ? 0 : n_dims <= 16 ? 1 : n_dims <= 32 ? 2 : n_dims <= KNN_REG_MAX_DIMS ? 3 : KNN_GENERIC_INSTANCE;
}

// The arguments have passed knn_check_args; n_query >= 1.
inline KnnPlan knn_plan(int64_t n_query, int64_t n_ref, int n_dims, int n_neighbors) {
    KnnPlan P;
    P.instance = knn_instance(n_dims);
    P.queries_per_lane = P.instance <= 2 ? 2 : 1;
    P.queries_per_wg = 64 * P.queries_per_lane;
    P.query_blocks = (n_query + P.queries_per_wg - 1) / P.queries_per_wg;
    int64_t nseg = 1;
    if (P.query_blocks < KNN_TARGET_WAVES) {
        const int64_t want = (KNN_TARGET_WAVES + P.query_blocks - 1) / P.query_blocks;
        const int64_t shortest = KNN_MIN_SEGMENT_REFS > 4 * n_neighbors ? KNN_MIN_SEGMENT_REFS : 4 * n_neighbors;
        const int64_t by_length = n_ref / shortest;
        nseg = want < by_length ? want : by_length;
        if (nseg > KNN_MAX_SEGMENTS) nseg = KNN_MAX_SEGMENTS;
        if (nseg < 1) nseg = 1;
    }
    P.segment_refs = (n_ref + nseg - 1) / nseg;
    P.segments = (int)((n_ref + P.segment_refs - 1) / P.segment_refs);   // no segment is empty
    P.lists_global = n_neighbors > KNN_LDS_MAX_NEIGHBORS ? 1 : 0;
    P.lds_bytes = P.lists_global ? 0 : (int64_t)P.queries_per_wg * n_neighbors * 12;
    return P;
}
