// Labels and values of the reference cells transferred to query cells along their neighbour lists (include/singlet_hip.h,
// "Neighbour index and transfer": sgl_op_knn_transfer, and the transfer stage of sgl_knn_index_map in kernels_knn_ivf.hip).
// gfx950 only, wave64, compiled with -ffp-contract=off: w * v and the addition after it are two roundings.
//
//   knn_transfer_wave    one workgroup is one wave and owns one query
//
// The wave stages the query's slots in LDS once: the cell, its label and the slot's distance, which the weight then replaces.
// The valid slots are a prefix of the list (the searches write the padding last; the operator refuses anything else), so their
// number is an integer count.  Every floating-point sum is owned by one lane from its first term to its last and runs over
// the slots in rank order from +0.0: lane l owns the classes l, l + 64, ... and the value rows l, l + 64, ...; W and Wv are
// formed by every lane for itself, in the same order, hence with the same bits.  A slot's label and weight are LDS broadcasts;
// for the values the 64 lanes read 64 consecutive doubles of column idx_i of V.  The arg-max is a wave reduction on
// (score, class) by comparisons alone.  No floating-point atomics; 64-bit offsets.
#include "sgl_internal.h"
#include "knn_transfer_host.h"
#include "knn_device.h"   // sgl_knn_check_finite

#include <limits>
#include <vector>

namespace {

__global__ __launch_bounds__(64) void knn_transfer_wave(const int32_t* __restrict__ idx, const double* __restrict__ dist, int K, int64_t nq,
                                                        const int32_t* __restrict__ labels, int n_classes, const double* __restrict__ V,
                                                        int n_values, int weighting, int32_t* __restrict__ pred, double* __restrict__ best,
                                                        double* __restrict__ scores, double* __restrict__ values) {
    __shared__ int32_t s_cell[KNN_MAX_NEIGHBORS];
    __shared__ int32_t s_label[KNN_MAX_NEIGHBORS];
    __shared__ double s_w[KNN_MAX_NEIGHBORS];
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x;
    if (j >= nq) return;
    const int32_t* ij = idx + j * K;
    const double* dj = dist + j * K;
    int mine = 0;
    for (int t = lane; t < K; t += 64) {
        const int32_t cell = ij[t];
        s_cell[t] = cell;
        s_w[t] = dj[t];
        s_label[t] = cell >= 0 && labels ? labels[cell] : -1;
        mine += cell >= 0 ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    const int nv = mine;   // the valid slots: 0 .. nv - 1
    __syncthreads();
    // the weights: Dudani's (d_last - d_i) / (d_last - d_first) when d_last is finite and above d_first, 1.0 otherwise
    const double d_first = nv > 0 ? s_w[0] : 0.0;
    const double d_last = nv > 0 ? s_w[nv - 1] : 0.0;
    const bool by_distance = weighting == 1 && nv > 0 && __builtin_isfinite(d_last) && d_last > d_first;
    const double span = d_last - d_first;
    __syncthreads();
    for (int t = lane; t < nv; t += 64) s_w[t] = by_distance ? (d_last - s_w[t]) / span : 1.0;
    __syncthreads();

    if (labels && (pred || best || scores)) {
        double W = 0.0;
        for (int t = 0; t < nv; ++t)
            if (s_label[t] >= 0) W = W + s_w[t];
        const bool voted = W > 0.0;
        double bs = 0.0;
        int32_t bc = INT32_MAX;   // no class yet
        for (int c0 = 0; c0 < n_classes; c0 += 64) {
            const int c = c0 + lane;
            if (c >= n_classes) continue;
            double s = 0.0;
            for (int t = 0; t < nv; ++t)
                if (s_label[t] == c) s = s + s_w[t];
            const double sc = voted ? s / W : 0.0;
            if (scores) scores[j * n_classes + c] = sc;
            if (bc == INT32_MAX || sc > bs) { bs = sc; bc = c; }   // the lane's classes ascend: an equal score keeps the lower
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o);
            const int32_t oc = __shfl_xor(bc, o);
            if (oc != INT32_MAX && (bc == INT32_MAX || os > bs || (os == bs && oc < bc))) { bs = os; bc = oc; }
        }
        if (lane == 0) {
            if (pred) pred[j] = voted ? bc : -1;
            if (best) best[j] = voted ? bs : 0.0;
        }
    }
    if (V && values) {
        double Wv = 0.0;
        for (int t = 0; t < nv; ++t) Wv = Wv + s_w[t];
        for (int f0 = 0; f0 < n_values; f0 += 64) {
            const int f = f0 + lane;
            if (f >= n_values) continue;
            double acc = 0.0;
            for (int t = 0; t < nv; ++t) acc = acc + s_w[t] * V[(int64_t)s_cell[t] * n_values + f];
            values[j * n_values + f] = nv > 0 ? acc / Wv : std::numeric_limits<double>::quiet_NaN();
        }
    }
}

}  // namespace

int sgl_knn_transfer_args(const char* who, int32_t weighting, int32_t n_neighbors, int64_t n_query, int64_t n_ref, bool has_labels,
                          int32_t n_classes, bool has_values, int32_t n_values) {
    switch (knn_transfer_check_args(weighting, n_neighbors, n_query, n_ref, has_labels, n_classes, has_values, n_values)) {
    case KNN_TRANSFER_ARGS_OK: return SGL_OK;
    case KNN_TRANSFER_ARGS_WEIGHTING: sgl_set_error("%s: weighting = %d is outside [0, %d]", who, weighting, KNN_TRANSFER_WEIGHTING_MAX); break;
    case KNN_TRANSFER_ARGS_NEIGHBORS: sgl_set_error("%s: n_neighbors = %d is outside [1, %d]", who, n_neighbors, KNN_MAX_NEIGHBORS); break;
    case KNN_TRANSFER_ARGS_NQUERY: sgl_set_error("%s: n_query = %lld is negative", who, (long long)n_query); break;
    case KNN_TRANSFER_ARGS_NREF: sgl_set_error("%s: n_ref = %lld is outside [1, 2^31)", who, (long long)n_ref); break;
    case KNN_TRANSFER_ARGS_CLASSES: sgl_set_error("%s: n_classes = %d is outside [1, %d]", who, n_classes, KNN_TRANSFER_MAX_CLASSES); break;
    case KNN_TRANSFER_ARGS_VALUES: sgl_set_error("%s: n_values = %d is outside [1, %d]", who, n_values, KNN_TRANSFER_MAX_VALUES); break;
    }
    return SGL_EINVAL;
}

int sgl_knn_transfer_labels_check(const char* who, const int32_t* labels, int64_t n_ref, int32_t n_classes) {
    const int64_t bad = knn_transfer_first_bad_label(labels, n_ref, n_classes);
    if (bad < 0) return SGL_OK;
    sgl_set_error("%s: labels[%lld] = %d is outside [-1, n_classes = %d)", who, (long long)bad, labels[bad], n_classes);
    return SGL_EINVAL;
}

int sgl_knn_transfer_dev(sgl_ctx* c, const int32_t* idx, const double* dist, int K, int64_t nq, const int32_t* labels, int n_classes,
                         const double* V, int n_values, int weighting, int32_t* pred, double* best, double* scores, double* values) {
    if (nq == 0) return SGL_OK;
    Phase ph(c, SGL_PH_SCALE);
    knn_transfer_wave<<<dim3((unsigned)nq), dim3(64), 0, c->stream>>>(idx, dist, K, nq, labels, n_classes, V, n_values, weighting, pred, best,
                                                                      scores, values);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

namespace {

struct TransferBuffers {
    DevBuf<int32_t> idx, labels, pred;
    DevBuf<double> dist, V, best, scores, values;
    DevBuf<unsigned long long> first;
};

int transfer_drain(sgl_ctx* c, int rc, const char* who) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("%s: HIP call failed: %s", who, hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

int transfer_body(sgl_ctx* c, const char* who, TransferBuffers& B, const int32_t* idx, const double* dist, int32_t K, int64_t nq, int64_t n_ref,
                  const int32_t* labels, int32_t n_classes, const double* V, int32_t n_values, int32_t weighting, int32_t* pred_out,
                  double* best_out, double* scores_out, double* values_out) {
    const size_t slots = (size_t)K * (size_t)nq;
    const bool want_labels = pred_out || best_out || scores_out;
    if (V && values_out) {
        SGLCHK(B.V.alloc((size_t)n_values * (size_t)n_ref));
        SGLCHK(B.first.alloc(1));
        HIPCHK(hipMemcpyAsync(B.V.p, V, sizeof(double) * (size_t)n_values * (size_t)n_ref, hipMemcpyHostToDevice, c->stream));
        SGLCHK(sgl_knn_check_finite(c, who, "V", B.V.p, n_values, n_ref, B.first.p));
    }
    SGLCHK(B.idx.alloc(slots));
    SGLCHK(B.dist.alloc(slots));
    HIPCHK(hipMemcpyAsync(B.idx.p, idx, sizeof(int32_t) * slots, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(B.dist.p, dist, sizeof(double) * slots, hipMemcpyHostToDevice, c->stream));
    if (labels && want_labels) {
        SGLCHK(B.labels.alloc((size_t)n_ref));
        HIPCHK(hipMemcpyAsync(B.labels.p, labels, sizeof(int32_t) * (size_t)n_ref, hipMemcpyHostToDevice, c->stream));
    }
    if (pred_out) SGLCHK(B.pred.alloc((size_t)nq));
    if (best_out) SGLCHK(B.best.alloc((size_t)nq));
    if (scores_out) SGLCHK(B.scores.alloc((size_t)n_classes * (size_t)nq));
    if (values_out) SGLCHK(B.values.alloc((size_t)n_values * (size_t)nq));
    SGLCHK(sgl_knn_transfer_dev(c, B.idx.p, B.dist.p, K, nq, B.labels.p, n_classes, B.V.p, n_values, weighting, B.pred.p, B.best.p, B.scores.p,
                                B.values.p));
    if (pred_out) HIPCHK(hipMemcpyAsync(pred_out, B.pred.p, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    if (best_out) HIPCHK(hipMemcpyAsync(best_out, B.best.p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    if (scores_out) HIPCHK(hipMemcpyAsync(scores_out, B.scores.p, sizeof(double) * (size_t)n_classes * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    if (values_out) HIPCHK(hipMemcpyAsync(values_out, B.values.p, sizeof(double) * (size_t)n_values * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SGL_OK;
}

}  // namespace

extern "C" int sgl_op_knn_transfer(sgl_ctx* c, const int32_t* idx, const double* dist, int32_t n_neighbors, int64_t n_query, int64_t n_ref,
                                   const int32_t* labels, int32_t n_classes, const double* V, int32_t n_values, int32_t weighting,
                                   int32_t* pred_out, double* best_out, double* scores_out, double* values_out) {
    const char* who = "sgl_op_knn_transfer";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    SGLCHK(sgl_knn_transfer_args(who, weighting, n_neighbors, n_query, n_ref, labels != nullptr, n_classes, V != nullptr, n_values));
    if ((pred_out || best_out || scores_out) && !labels) {
        sgl_set_error("%s: pred_out, best_out or scores_out is asked for, but labels is NULL", who);
        return SGL_EINVAL;
    }
    if (values_out && !V) { sgl_set_error("%s: values_out is asked for, but V is NULL", who); return SGL_EINVAL; }
    if (n_query > 0 && (!idx || !dist)) { sgl_set_error("%s: idx or dist is NULL", who); return SGL_EINVAL; }
    if (labels) SGLCHK(sgl_knn_transfer_labels_check(who, labels, n_ref, n_classes));
    int64_t query = -1;
    int32_t slot = -1, value = 0;
    switch (knn_transfer_check_slots(idx, n_neighbors, n_query, n_ref, &query, &slot, &value)) {
    case KNN_TRANSFER_SLOTS_OK: break;
    case KNN_TRANSFER_SLOTS_RANGE:
        sgl_set_error("%s: idx holds %d in column %lld, slot %d (0-based): outside [-1, n_ref = %lld)", who, value, (long long)query, slot,
                      (long long)n_ref);
        return SGL_EINVAL;
    case KNN_TRANSFER_SLOTS_ORDER:
        sgl_set_error("%s: idx holds the valid entry %d in column %lld, slot %d (0-based) behind a padding slot", who, value, (long long)query,
                      slot);
        return SGL_EINVAL;
    }
    if (n_query == 0) return SGL_OK;
    TransferBuffers B;
    const int rc = transfer_body(c, who, B, idx, dist, n_neighbors, n_query, n_ref, labels, n_classes, V, n_values, weighting, pred_out, best_out,
                                 scores_out, values_out);
    return transfer_drain(c, rc, who);
}
