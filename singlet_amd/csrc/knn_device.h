// What the scans of the embedding neighbour searches share: the exact scan (kernels_knn.hip) and the inverted-list scan
// (kernels_knn_ivf.hip) form a pair's sum, its key and a candidate's place in a list with the very same code, so that the two
// give the same bits.  Device code, and the few host entries of kernels_knn.hip that the inverted-list search calls.  Both
// units are compiled with -ffp-contract=off.
#pragma once
#include "sgl_internal.h"
#include "knn_host.h"

namespace {

// One (pair, dimension) of the scan.  Euclidean: the three instructions of the unit's head comment.  DOT: the product and the
// addition of the dot of two unit columns.
template <bool DOT>
__device__ __forceinline__ double knn_step(double s, double q, double r) {
    if constexpr (DOT) {
        return s + q * r;
    } else {
        const double t = q - r;
        return s + t * t;
    }
}

// What a pair is ranked by, once per pair.  Euclidean: the sum itself.  DOT: 1 - dot, and +0.0 below 2^-40 -- two bitwise
// equal unit columns with a direction give a dot within rounding of 1, and the snap puts them at exactly +0.0.
template <bool DOT>
__device__ __forceinline__ double knn_key(double s) {
    if constexpr (DOT) {
        const double key = 1.0 - s;
        return key < 0x1p-40 ? 0.0 : key;
    } else {
        return s;
    }
}

// The candidate enters the list sorted by (s, index) whose slot t is ld[t * stride], li[t * stride]: behind every entry
// whose s is not greater.  cnt = the slots filled; worst = the K-th s once the list is full.
__device__ __forceinline__ void knn_insert(double* __restrict__ ld, int32_t* __restrict__ li, int64_t stride, int K, int& cnt, double& worst,
                                           double s, int32_t r) {
    int t = cnt < K ? cnt : K - 1;   // the slot that opens: the end of a list still filling, the last of a full one
    while (t > 0) {
        const double p = ld[(int64_t)(t - 1) * stride];
        if (!(p > s)) break;
        ld[(int64_t)t * stride] = p;
        li[(int64_t)t * stride] = li[(int64_t)(t - 1) * stride];
        --t;
    }
    ld[(int64_t)t * stride] = s;
    li[(int64_t)t * stride] = r;
    if (cnt < K) ++cnt;
    if (cnt == K) worst = ld[(int64_t)(K - 1) * stride];
}

}  // namespace

// ---- host entries of kernels_knn.hip ----------------------------------------------------------------------------------
// sgl_knn's argument refusals and sgl_knn_metric's, with their messages under the caller's name
int sgl_knn_args(const char* who, int32_t k, int64_t n_ref, int64_t n_query, const int32_t* dims, int32_t n_dims, int32_t n_neighbors);
int sgl_knn_metric_arg(const char* who, int32_t metric);
// SGL_EINVAL naming the first non-finite value of the k x n operand X on the device; first_dev: one word of scratch
int sgl_knn_check_finite(sgl_ctx* c, const char* who, const char* name, const double* X, int32_t k, int64_t n, unsigned long long* first_dev);
// The operand the scans read, from the raw k x n columns X on the device: rows dims_dev (nullptr: the first nd), gathered
// (metric 0) or as unit columns (1, 2: *no_direction counts the columns without direction).  packed: nd x n, packed[j * nd + f];
// transposed: n x nd, transposed[f * n + j]; either may be nullptr.  Launches only.
int sgl_knn_operand(sgl_ctx* c, const double* X, int32_t k, int64_t n, const int32_t* dims_dev, int nd, int32_t metric, double* packed,
                    double* transposed, unsigned long long* no_direction);
// The scan of plan P over the packed references Rs and its merge: idx[j * K + t], dist[j * K + t] (either may be nullptr).
// Qs: packed, for the generic instance transposed.  cs / ci: P.segments x K x nq slots of scratch.  dot: the form of metrics 1, 2.
int sgl_knn_scan(hipStream_t s, const KnnPlan& P, bool dot, const double* Rs, const double* Qs, int nd, int64_t nq, int64_t n_ref, int K,
                 double* cs, int32_t* ci, int32_t* idx, double* dist);
