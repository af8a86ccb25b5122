// Exact k-nearest neighbours of query columns among reference columns of a k x n embedding (include/singlet_hip.h, sgl_knn
// and sgl_knn_metric).  gfx950 only.  This unit is compiled with -ffp-contract=off: s = s + t * t is a product and an
// addition, two roundings.
//
//   knn_first_nonfinite   the first NaN / Inf of an operand in column-major order (the refusal names it)
//   knn_gather            the rows `dims` of an operand, packed n_dims x n -- or, for the generic scan's queries, n x n_dims
//   knn_unit              cosine / correlation: in place of the gather, the unit columns of an operand in the same two layouts
//   knn_scan_reg          n_dims <= 64: a lane owns one or two queries and keeps their coordinates in registers
//   knn_scan_generic      every rank above: a lane owns one query, eight references at a time keep their running sums
//   knn_finish            merges the segments' candidates by (s, index), takes the root (Euclidean only), writes the result
//
// The scan.  One workgroup is one wave; grid = (query blocks, reference segments).  The references of the segment stream in
// ascending index.  A reference coordinate is the same for all 64 lanes: its address depends on the loop counter and the
// block index alone, so it is read through the scalar cache into SGPRs and enters the three FP64 VALU instructions of a
// (pair, dimension) -- v_add (the subtraction), v_mul, v_add -- as their scalar operand.  Nothing else is issued per pair
// and dimension: the operand delivery costs the vector unit nothing, whatever the number of queries per lane.
//
// Selection.  Per query a list of K candidates sorted ascending by (s, index), and its K-th s in a register.  Inside a
// segment the indices ascend, so a candidate enters a full list only when s < the K-th s, strictly, and goes behind every
// entry with an equal s: no index is compared.  The list lives in LDS, slot-major ([slot][query of the workgroup]: the
// lanes of a wave hit 64 consecutive doubles), up to K = 32 -- 48 KiB for the 128 queries of a workgroup -- and above in
// the global candidate array the merge reads anyway.  Insertions are divergent and rare: K (1 + ln(n / K)) per query.
//
// Cosine and correlation (DOT = true).  The operands are unit columns (knn_unit) and the inner form is dot = dot + q_f * r_f:
// v_mul, v_add with the reference coordinate as the scalar operand, two FP64 VALU instructions per (pair, dimension) where the
// Euclidean form issues three.  The key 1 - dot, snapped to +0.0 below 2^-40, is formed once per pair (knn_key) and is what
// the lists, the segments and the merge rank exactly as they rank s; knn_finish takes no root of it.
//
// Merge.  Every segment leaves K candidates per query, (+Inf, INT32_MAX) where it had fewer than K references.  (s, index)
// is a total order and no real index is INT32_MAX, so the K least of their union are the K least of all references,
// however the references were cut.
#include "sgl_internal.h"
#include "knn_host.h"
#include "knn_device.h"   // knn_step, knn_key, knn_insert: shared with the inverted-list scan

#include <limits>

namespace {

constexpr int KNN_TILE = 8;   // references per tile of the generic scan

__global__ __launch_bounds__(256) void knn_first_nonfinite(const double* __restrict__ X, int64_t n, unsigned long long* first) {
    unsigned long long best = ~0ull;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(X[e]);
        if (((bits >> 52) & 0x7ffull) == 0x7ffull) { best = (unsigned long long)e; break; }   // e ascends: the thread's first
    }
    if (best != ~0ull) atomicMin(first, best);
}

// out[j * nd + f] = X[j * k + dims[f]] (transposed: out[f * n + j]); dims == nullptr: the first nd rows
__global__ __launch_bounds__(256) void knn_gather(const double* __restrict__ X, int k, int64_t n, const int32_t* __restrict__ dims, int nd,
                                                  int transposed, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * nd) return;
    const int64_t j = transposed ? e % n : e / nd;
    const int f = (int)(transposed ? e / n : e % nd);
    out[e] = X[j * k + (dims ? dims[f] : f)];
}

// Unit columns (include/singlet_hip.h, sgl_knn_metric, rule 1).  One workgroup is one wave and owns 64 columns; lane l walks
// column l sequentially -- the rule's shape -- three times: the mean (correlation only), the sum of squares, the division.
// Each walk goes in chunks of KNN_UNIT_ROWS rows that the wave stages through LDS: in global memory a lane group reads
// (writes) 32 consecutive doubles of one column, in LDS lane l reads row l of the tile, whose stride of 33 doubles spreads
// the 32 lanes of a group over all banks.  The second and third walk find the tile's columns in L2.
// out: nd x n packed (out[j * nd + f]); out_t: n x nd (out_t[f * n + j]); either may be nullptr.  no_direction counts the
// columns whose norm is 0 or +Inf: every coordinate of their unit column is a zero.
constexpr int KNN_UNIT_ROWS = 32;
constexpr int KNN_UNIT_STRIDE = KNN_UNIT_ROWS + 1;

__global__ __launch_bounds__(64) void knn_unit(const double* __restrict__ X, int k, int64_t n, const int32_t* __restrict__ dims, int nd, int centre,
                                               double* __restrict__ out, double* __restrict__ out_t, unsigned long long* no_direction) {
    __shared__ double tile[64 * KNN_UNIT_STRIDE];
    const int lane = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * 64;
    const int64_t j = j0 + lane;
    const bool mine = j < n;
    double* row = tile + lane * KNN_UNIT_STRIDE;
    // rows [f0, f0 + KNN_UNIT_ROWS) of the 64 columns into the tile; element e of the tile is (column e / 32, row e % 32)
    auto stage = [&](int f0) {
        __syncthreads();
        for (int e = lane; e < 64 * KNN_UNIT_ROWS; e += 64) {
            const int c = e / KNN_UNIT_ROWS, f = f0 + e % KNN_UNIT_ROWS;
            if (j0 + c < n && f < nd) tile[c * KNN_UNIT_STRIDE + e % KNN_UNIT_ROWS] = X[(j0 + c) * k + (dims ? dims[f] : f)];
        }
        __syncthreads();
    };
    double m = 0.0;
    if (centre) {
        for (int f0 = 0; f0 < nd; f0 += KNN_UNIT_ROWS) {
            stage(f0);
            const int len = nd - f0 < KNN_UNIT_ROWS ? nd - f0 : KNN_UNIT_ROWS;
            if (mine)
                for (int f = 0; f < len; ++f) m = m + row[f];
        }
        m = m / (double)nd;
    }
    double s2 = 0.0;
    for (int f0 = 0; f0 < nd; f0 += KNN_UNIT_ROWS) {
        stage(f0);
        const int len = nd - f0 < KNN_UNIT_ROWS ? nd - f0 : KNN_UNIT_ROWS;
        if (mine)
            for (int f = 0; f < len; ++f) {
                const double y = centre ? row[f] - m : row[f];
                s2 = s2 + y * y;
            }
    }
    const double nrm = __builtin_sqrt(s2);
    if (mine && (nrm == 0.0 || nrm == std::numeric_limits<double>::infinity())) atomicAdd(no_direction, 1ull);
    for (int f0 = 0; f0 < nd; f0 += KNN_UNIT_ROWS) {
        stage(f0);
        const int len = nd - f0 < KNN_UNIT_ROWS ? nd - f0 : KNN_UNIT_ROWS;
        if (mine)
            for (int f = 0; f < len; ++f) {
                const double y = centre ? row[f] - m : row[f];
                const double u = nrm != 0.0 ? y / nrm : 0.0;
                if (out_t) out_t[(int64_t)(f0 + f) * n + j] = u;
                row[f] = u;   // the lane's own row: nobody else reads it before the barrier
            }
        if (out) {
            __syncthreads();
            for (int e = lane; e < 64 * KNN_UNIT_ROWS; e += 64) {
                const int c = e / KNN_UNIT_ROWS, f = f0 + e % KNN_UNIT_ROWS;
                if (j0 + c < n && f < nd) out[(j0 + c) * nd + f] = tile[c * KNN_UNIT_STRIDE + e % KNN_UNIT_ROWS];
            }
        }
    }
}

// The lists of one lane's QPL queries: where they live, and what the scan leaves in cs / ci when it ends.
template <int QPL, bool LISTS_GLOBAL>
struct KnnLists {
    double* ld[QPL];
    int32_t* li[QPL];
    int64_t stride;
    int cnt[QPL];
    double worst[QPL];
    int64_t j[QPL];      // the query; -1: past the last one (the lane computes on a copy of the last query and keeps nothing)
    double* out_d[QPL];  // slot 0 of the query's candidates of this segment in cs / ci (slot t at t * nq)
    int32_t* out_i[QPL];

    __device__ __forceinline__ void init(double* lds, int64_t q0, int lane, int64_t nq, int K, int seg, double* cs, int32_t* ci) {
        stride = LISTS_GLOBAL ? nq : 64 * QPL;
#pragma unroll
        for (int u = 0; u < QPL; ++u) {
            const int64_t jj = q0 + u * 64 + lane;
            j[u] = jj < nq ? jj : -1;
            const int64_t jc = jj < nq ? jj : nq - 1;
            out_d[u] = cs + (int64_t)seg * K * nq + jc;
            out_i[u] = ci + (int64_t)seg * K * nq + jc;
            if (LISTS_GLOBAL) {
                ld[u] = out_d[u];
                li[u] = out_i[u];
            } else {
                ld[u] = lds + u * 64 + lane;
                li[u] = reinterpret_cast<int32_t*>(lds + (int64_t)64 * QPL * K) + u * 64 + lane;
            }
            cnt[u] = j[u] >= 0 ? 0 : K;   // a lane without a query takes nothing: its list is "full" and no s is below -1
            worst[u] = j[u] >= 0 ? std::numeric_limits<double>::infinity() : -1.0;
        }
    }
    __device__ __forceinline__ void offer(int u, int K, double s, int32_t r) {
        if (cnt[u] < K || s < worst[u]) knn_insert(ld[u], li[u], stride, K, cnt[u], worst[u], s, r);
    }
    __device__ __forceinline__ void flush(int K, int64_t nq) {
#pragma unroll
        for (int u = 0; u < QPL; ++u) {
            if (j[u] < 0) continue;
            if (!LISTS_GLOBAL)
                for (int t = 0; t < cnt[u]; ++t) {
                    out_d[u][(int64_t)t * nq] = ld[u][(int64_t)t * stride];
                    out_i[u][(int64_t)t * nq] = li[u][(int64_t)t * stride];
                }
            for (int t = cnt[u]; t < K; ++t) {
                out_d[u][(int64_t)t * nq] = std::numeric_limits<double>::infinity();
                out_i[u][(int64_t)t * nq] = INT32_MAX;
            }
        }
    }
};

// n_dims in [NDLO, NDHI].  The dimensions go in chunks of CH.  A chunk that ends at or below NDLO is unconditional; behind it
// one wave-uniform test per chunk: a whole chunk is CH contiguous doubles of the reference column (one wide scalar load),
// and the one partial chunk reads the column's last coordinate in place of those past it and replaces them by +0.0 -- the
// query's registers hold +0.0 there, t = +0.0 and s + t * t = s, bit for bit (s is never -0.0).  Chunks past n_dims are skipped.
// DOT: the padded product is +0.0 * +0.0 = +0.0, and dot + (+0.0) = dot for every dot that can occur: dot starts at +0.0 and
// a sum is -0.0 only when both terms are, so dot is never -0.0 either.
template <int NDLO, int NDHI, int CH, int QPL, bool LISTS_GLOBAL, bool DOT = false>
__global__ __launch_bounds__(64) void knn_scan_reg(const double* __restrict__ R, const double* __restrict__ Q, int nd, int64_t nq, int64_t n_ref,
                                                   int64_t segment_refs, int K, double* __restrict__ cs, int32_t* __restrict__ ci) {
    static_assert(NDHI % CH == 0, "whole chunks");
    extern __shared__ double knn_lds[];
    const int lane = threadIdx.x;
    const int seg = blockIdx.y;
    const int64_t lo = (int64_t)seg * segment_refs;
    const int64_t hi = lo + segment_refs < n_ref ? lo + segment_refs : n_ref;
    KnnLists<QPL, LISTS_GLOBAL> L;
    L.init(knn_lds, (int64_t)blockIdx.x * (64 * QPL), lane, nq, K, seg, cs, ci);
    double q[QPL][NDHI];
#pragma unroll
    for (int u = 0; u < QPL; ++u) {
        const double* qp = Q + (L.j[u] >= 0 ? L.j[u] : nq - 1) * nd;
#pragma unroll
        for (int f = 0; f < NDHI; ++f) q[u][f] = f < nd ? qp[f] : 0.0;
    }
    for (int64_t r = lo; r < hi; ++r) {
        const double* __restrict__ rp = R + r * nd;   // wave-uniform: scalar loads
        double s[QPL];
#pragma unroll
        for (int u = 0; u < QPL; ++u) s[u] = 0.0;
#pragma unroll
        for (int c = 0; c < NDHI; c += CH) {
            if (c + CH <= NDLO || c + CH <= nd) {
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    const double rf = rp[c + e];
#pragma unroll
                    for (int u = 0; u < QPL; ++u) s[u] = knn_step<DOT>(s[u], q[u][c + e], rf);
                }
            } else if (c < nd) {
                double rf[CH];
#pragma unroll
                for (int e = 0; e < CH; ++e) rf[e] = rp[c + e < nd ? c + e : nd - 1];
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    const double re = c + e < nd ? rf[e] : 0.0;
#pragma unroll
                    for (int u = 0; u < QPL; ++u) s[u] = knn_step<DOT>(s[u], q[u][c + e], re);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < QPL; ++u) L.offer(u, K, knn_key<DOT>(s[u]), (int32_t)r);
    }
    L.flush(K, nq);
}

// Qt is n_dims x nq transposed (Qt[f * nq + j]: the lanes of a wave read consecutive doubles).  The running sums of a tile
// of KNN_TILE references stay in registers over the whole loop over f, which goes four dimensions at a time (four contiguous
// doubles of each reference column: one scalar load) and ends with the partial chunk of knn_scan_reg.
template <bool LISTS_GLOBAL, bool DOT = false>
__global__ __launch_bounds__(64) void knn_scan_generic(const double* __restrict__ R, const double* __restrict__ Qt, int nd, int64_t nq, int64_t n_ref,
                                                       int64_t segment_refs, int K, double* __restrict__ cs, int32_t* __restrict__ ci) {
    constexpr int CH = 4;
    extern __shared__ double knn_lds[];
    const int lane = threadIdx.x;
    const int seg = blockIdx.y;
    const int64_t lo = (int64_t)seg * segment_refs;
    const int64_t hi = lo + segment_refs < n_ref ? lo + segment_refs : n_ref;
    KnnLists<1, LISTS_GLOBAL> L;
    L.init(knn_lds, (int64_t)blockIdx.x * 64, lane, nq, K, seg, cs, ci);
    const double* qp = Qt + (L.j[0] >= 0 ? L.j[0] : nq - 1);
    for (int64_t r0 = lo; r0 < hi; r0 += KNN_TILE) {
        const double* __restrict__ rp[KNN_TILE];
#pragma unroll
        for (int i = 0; i < KNN_TILE; ++i) rp[i] = R + (r0 + i < hi ? r0 + i : hi - 1) * nd;   // past the end: the last one again, not offered
        double s[KNN_TILE];
#pragma unroll
        for (int i = 0; i < KNN_TILE; ++i) s[i] = 0.0;
        int f = 0;
        for (; f + CH <= nd; f += CH) {
            double qf[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) qf[e] = qp[(int64_t)(f + e) * nq];
#pragma unroll
            for (int i = 0; i < KNN_TILE; ++i) {
#pragma unroll
                for (int e = 0; e < CH; ++e) s[i] = knn_step<DOT>(s[i], qf[e], rp[i][f + e]);
            }
        }
        if (f < nd) {
            double qf[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const double v = qp[(int64_t)(f + e < nd ? f + e : nd - 1) * nq];
                qf[e] = f + e < nd ? v : 0.0;
            }
#pragma unroll
            for (int i = 0; i < KNN_TILE; ++i) {
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    const double v = rp[i][f + e < nd ? f + e : nd - 1];
                    s[i] = knn_step<DOT>(s[i], qf[e], f + e < nd ? v : 0.0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < KNN_TILE; ++i)
            if (r0 + i < hi) L.offer(0, K, knn_key<DOT>(s[i]), (int32_t)(r0 + i));
    }
    L.flush(K, nq);
}

// One thread per query: K times the least head of the segments' sorted lists by (s, index).  ROOT: the distance is the root
// of the Euclidean sum; a cosine or correlation key goes out as it is.
template <bool ROOT>
__global__ __launch_bounds__(256) void knn_finish(const double* __restrict__ cs, const int32_t* __restrict__ ci, int nseg, int K, int64_t nq,
                                                  int32_t* __restrict__ idx_out, double* __restrict__ dist_out) {
    __shared__ uint16_t head[KNN_MAX_SEGMENTS][256];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    if (j >= nq) return;
    for (int g = 0; g < nseg; ++g) head[g][tid] = 0;
    for (int t = 0; t < K; ++t) {
        int best = -1;
        double bd = 0.0;
        int32_t bi = 0;
        for (int g = 0; g < nseg; ++g) {
            const int h = head[g][tid];
            if (h >= K) continue;
            const int64_t at = ((int64_t)g * K + h) * nq + j;
            const double d = cs[at];
            const int32_t i = ci[at];
            if (best < 0 || d < bd || (d == bd && i < bi)) { best = g; bd = d; bi = i; }
        }
        head[best][tid] = (uint16_t)(head[best][tid] + 1);   // nseg * K >= K slots: a head is always left
        if (idx_out) idx_out[j * K + t] = bi;
        if (dist_out) dist_out[j * K + t] = ROOT ? __builtin_sqrt(bd) : bd;
    }
}

template <int NDLO, int NDHI, int CH, int QPL, bool DOT>
int launch_reg(hipStream_t s, const KnnPlan& P, const double* R, const double* Q, int nd, int64_t nq, int64_t n_ref, int K, double* cs,
               int32_t* ci) {
    const dim3 grid((unsigned)P.query_blocks, (unsigned)P.segments);
    if (P.lists_global)
        knn_scan_reg<NDLO, NDHI, CH, QPL, true, DOT><<<grid, dim3(64), 0, s>>>(R, Q, nd, nq, n_ref, P.segment_refs, K, cs, ci);
    else
        knn_scan_reg<NDLO, NDHI, CH, QPL, false, DOT><<<grid, dim3(64), (size_t)P.lds_bytes, s>>>(R, Q, nd, nq, n_ref, P.segment_refs, K, cs, ci);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

// The scan of plan P and the merge.  DOT = false is sgl_knn's code, DOT = true the cosine / correlation form of every instance.
template <bool DOT>
int launch_scan(hipStream_t s, const KnnPlan& P, const double* Rs, const double* Qs, int nd, int64_t nq, int64_t n_ref, int K, double* cs,
                int32_t* ci, int32_t* idx, double* dist) {
    switch (P.instance) {
    case 0: SGLCHK((launch_reg<1, 8, 2, 2, DOT>(s, P, Rs, Qs, nd, nq, n_ref, K, cs, ci))); break;
    case 1: SGLCHK((launch_reg<9, 16, 4, 2, DOT>(s, P, Rs, Qs, nd, nq, n_ref, K, cs, ci))); break;
    case 2: SGLCHK((launch_reg<17, 32, 8, 2, DOT>(s, P, Rs, Qs, nd, nq, n_ref, K, cs, ci))); break;
    case 3: SGLCHK((launch_reg<33, 64, 8, 1, DOT>(s, P, Rs, Qs, nd, nq, n_ref, K, cs, ci))); break;
    default: {
        const dim3 grid((unsigned)P.query_blocks, (unsigned)P.segments);
        if (P.lists_global)
            knn_scan_generic<true, DOT><<<grid, dim3(64), 0, s>>>(Rs, Qs, nd, nq, n_ref, P.segment_refs, K, cs, ci);
        else
            knn_scan_generic<false, DOT><<<grid, dim3(64), (size_t)P.lds_bytes, s>>>(Rs, Qs, nd, nq, n_ref, P.segment_refs, K, cs, ci);
        HIPCHK(hipGetLastError());
    }
    }
    knn_finish<!DOT><<<dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s>>>(cs, ci, P.segments, K, nq, idx, dist);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

// every return path waits for the stream before the device buffers (and the caller's host arrays) go
int knn_drain(sgl_ctx* c, int rc, const char* who) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("%s: HIP call failed: %s", who, hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

// SGL_EINVAL naming the first non-finite value of the k x n operand X (on the device) in column-major order
int knn_check_finite(sgl_ctx* c, const char* who, const char* name, const double* X, int32_t k, int64_t n, unsigned long long* first_dev) {
    const int64_t total = (int64_t)k * n;
    if (total == 0) return SGL_OK;
    HIPCHK(hipMemsetAsync(first_dev, 0xff, sizeof(unsigned long long), c->stream));
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 4096);
    knn_first_nonfinite<<<dim3((unsigned)blocks), dim3(256), 0, c->stream>>>(X, total, first_dev);
    HIPCHK(hipGetLastError());
    unsigned long long first = 0;
    HIPCHK(hipMemcpyAsync(&first, first_dev, sizeof(first), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (first != ~0ull) {
        sgl_set_error("%s: %s holds a non-finite value in column %lld, row %lld (0-based; the first in column-major order)", who, name,
                      (long long)(first / (unsigned long long)k), (long long)(first % (unsigned long long)k));
        return SGL_EINVAL;
    }
    return SGL_OK;
}

struct KnnBuffers {
    DevBuf<double> R, Q, Rp, Qp, cs, dist;
    DevBuf<int32_t> dims, ci, idx;
    DevBuf<unsigned long long> first, no_direction;
};

// Rdev: the k x n_ref references on the device (the fit's H, or B.R).  Arguments checked by the caller.
int knn_body(sgl_ctx* c, const char* who, KnnBuffers& B, const double* Rdev, const char* Rname, int32_t k, int64_t n_ref, const double* Q,
             int64_t n_query, const int32_t* dims, int32_t n_dims, int32_t K, int32_t metric, int32_t* idx_out, double* dist_out) {
    const int nd = dims ? n_dims : k;
    const double* Qdev = Rdev;
    int64_t nq = n_ref;
    if (Q) {
        nq = n_query;
        SGLCHK(B.Q.alloc((size_t)k * (size_t)std::max<int64_t>(nq, 1)));
        if (nq > 0) HIPCHK(hipMemcpyAsync(B.Q.p, Q, sizeof(double) * (size_t)k * (size_t)nq, hipMemcpyHostToDevice, c->stream));
        Qdev = B.Q.p;
    }
    SGLCHK(B.first.alloc(1));
    SGLCHK(knn_check_finite(c, who, Rname, Rdev, k, n_ref, B.first.p));
    if (Q) SGLCHK(knn_check_finite(c, who, "Q", Qdev, k, nq, B.first.p));
    if (nq == 0) return SGL_OK;
    const KnnPlan P = knn_plan(nq, n_ref, nd, K);
    // the operands the scan reads: n_dims x n packed; the generic scan's queries n x n_dims
    const double* Rs = Rdev;
    const double* Qs = Qdev;
    const bool generic = P.instance == KNN_GENERIC_INSTANCE;
    if (dims) {
        SGLCHK(B.dims.alloc((size_t)nd));
        HIPCHK(hipMemcpyAsync(B.dims.p, dims, sizeof(int32_t) * (size_t)nd, hipMemcpyHostToDevice, c->stream));
    }
    if (metric != KNN_METRIC_EUCLIDEAN) {
        // the unit columns of both operands, in the call's own buffers (the resident H is only read), in the layouts of the gather
        const int centre = metric == KNN_METRIC_CORRELATION ? 1 : 0;
        const int32_t* dd = dims ? B.dims.p : nullptr;
        SGLCHK(B.no_direction.alloc(1));
        HIPCHK(hipMemsetAsync(B.no_direction.p, 0, sizeof(unsigned long long), c->stream));
        SGLCHK(B.Rp.alloc((size_t)nd * (size_t)n_ref));
        if (Q || generic) SGLCHK(B.Qp.alloc((size_t)nd * (size_t)nq));
        Phase ph(c, SGL_PH_GRAM);   // the pass alone, apart from the scan's "scale": the call books nothing else here
        knn_unit<<<dim3((unsigned)((n_ref + 63) / 64)), dim3(64), 0, c->stream>>>(Rdev, k, n_ref, dd, nd, centre, B.Rp.p,
                                                                                   !Q && generic ? B.Qp.p : nullptr, B.no_direction.p);
        HIPCHK(hipGetLastError());
        if (Q) {
            knn_unit<<<dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, c->stream>>>(Qdev, k, nq, dd, nd, centre, generic ? nullptr : B.Qp.p,
                                                                                generic ? B.Qp.p : nullptr, B.no_direction.p);
            HIPCHK(hipGetLastError());
        }
        Rs = B.Rp.p;
        Qs = Q || generic ? B.Qp.p : B.Rp.p;
    } else if (dims) {
        SGLCHK(B.Rp.alloc((size_t)nd * (size_t)n_ref));
        knn_gather<<<dim3((unsigned)(((int64_t)nd * n_ref + 255) / 256)), dim3(256), 0, c->stream>>>(Rdev, k, n_ref, B.dims.p, nd, 0, B.Rp.p);
        HIPCHK(hipGetLastError());
        Rs = B.Rp.p;
        if (!Q && !generic) Qs = Rs;
    }
    if (metric == KNN_METRIC_EUCLIDEAN && (generic || (dims && Qs != Rs))) {
        SGLCHK(B.Qp.alloc((size_t)nd * (size_t)nq));
        knn_gather<<<dim3((unsigned)(((int64_t)nd * nq + 255) / 256)), dim3(256), 0, c->stream>>>(Qdev, k, nq, dims ? B.dims.p : nullptr, nd,
                                                                                              generic ? 1 : 0, B.Qp.p);
        HIPCHK(hipGetLastError());
        Qs = B.Qp.p;
    }
    const size_t slots = (size_t)P.segments * (size_t)K * (size_t)nq;
    SGLCHK(B.cs.alloc(slots));
    SGLCHK(B.ci.alloc(slots));
    if (idx_out) SGLCHK(B.idx.alloc((size_t)K * (size_t)nq));
    if (dist_out) SGLCHK(B.dist.alloc((size_t)K * (size_t)nq));
    {
        Phase ph(c, SGL_PH_SCALE);   // where scripts/knn_rate.py reads the kernels' time
        if (metric == KNN_METRIC_EUCLIDEAN)
            SGLCHK(launch_scan<false>(c->stream, P, Rs, Qs, nd, nq, n_ref, K, B.cs.p, B.ci.p, B.idx.p, B.dist.p));
        else
            SGLCHK(launch_scan<true>(c->stream, P, Rs, Qs, nd, nq, n_ref, K, B.cs.p, B.ci.p, B.idx.p, B.dist.p));
    }
    unsigned long long no_direction = 0;
    if (metric != KNN_METRIC_EUCLIDEAN)
        HIPCHK(hipMemcpyAsync(&no_direction, B.no_direction.p, sizeof(no_direction), hipMemcpyDeviceToHost, c->stream));
    if (idx_out) HIPCHK(hipMemcpyAsync(idx_out, B.idx.p, sizeof(int32_t) * (size_t)K * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    if (dist_out) HIPCHK(hipMemcpyAsync(dist_out, B.dist.p, sizeof(double) * (size_t)K * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->knn_last[0] = P.instance;
    c->knn_last[1] = P.segments;
    c->knn_last[2] = P.queries_per_wg;
    c->knn_last[3] = P.lists_global;
    c->knn_last[4] = metric;
    c->knn_last[5] = (int64_t)no_direction;
    return SGL_OK;
}

int knn_args(const char* who, int32_t k, int64_t n_ref, int64_t n_query, const int32_t* dims, int32_t n_dims, int32_t n_neighbors) {
    int32_t pos = -1, value = 0;
    switch (knn_check_args(k, n_ref, n_query, dims, n_dims, n_neighbors, &pos, &value)) {
    case KNN_ARGS_OK: return SGL_OK;
    case KNN_ARGS_RANK: sgl_set_error("%s: k = %d is outside [1, %d]", who, k, KNN_MAX_RANK); break;
    case KNN_ARGS_NREF: sgl_set_error("%s: n_ref = %lld is outside [1, 2^31)", who, (long long)n_ref); break;
    case KNN_ARGS_NQUERY: sgl_set_error("%s: n_query = %lld is negative", who, (long long)n_query); break;
    case KNN_ARGS_NEIGHBORS:
        sgl_set_error("%s: n_neighbors = %d is outside [1, min(%d, n_ref = %lld)]", who, n_neighbors, KNN_MAX_NEIGHBORS, (long long)n_ref);
        break;
    case KNN_ARGS_NDIMS: sgl_set_error("%s: n_dims = %d is outside [1, k = %d]", who, n_dims, k); break;
    case KNN_ARGS_DIM_RANGE: sgl_set_error("%s: dims[%d] = %d is outside [0, k = %d)", who, pos, value, k); break;
    case KNN_ARGS_DIM_REPEAT: sgl_set_error("%s: dims[%d] = %d repeats an earlier entry", who, pos, value); break;
    }
    return SGL_EINVAL;
}

int knn_metric_arg(const char* who, int32_t metric) {
    if (knn_metric_ok(metric)) return SGL_OK;
    sgl_set_error("%s: metric = %d is outside [0, %d]", who, metric, KNN_METRIC_MAX);
    return SGL_EINVAL;
}

int knn_entry(sgl_ctx* c, const char* who, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims,
              int32_t n_dims, int32_t n_neighbors, int32_t metric, int32_t* idx_out, double* dist_out) {
    if (c->team || c->allreduce) {
        sgl_set_error("%s: the context is a shard of a team or has an all-reduce hook; the H of this shard's cells is not the embedding", who);
        return SGL_ESTATE;
    }
    if (!R && c->k == 0) { sgl_set_error("%s: R is NULL and no fit is initialised (call sgl_fit_init)", who); return SGL_ESTATE; }
    if (!R && (k != c->k || n_ref != c->A.ncol)) {
        sgl_set_error("%s: R is NULL, but k = %d, n_ref = %lld are not the fit's %d x %d", who, k, (long long)n_ref, c->k, c->A.ncol);
        return SGL_EINVAL;
    }
    SGLCHK(knn_args(who, k, n_ref, n_query, dims, n_dims, n_neighbors));
    SGLCHK(knn_metric_arg(who, metric));
    KnnBuffers B;
    int rc = SGL_OK;
    const double* Rdev = c->H;
    if (R) {
        rc = B.R.alloc((size_t)k * (size_t)n_ref);
        if (rc == SGL_OK && hipMemcpyAsync(B.R.p, R, sizeof(double) * (size_t)k * (size_t)n_ref, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            sgl_set_error("%s: the copy of R to the device failed", who);
            rc = SGL_EHIP;
        }
        Rdev = B.R.p;
    }
    if (rc == SGL_OK) rc = knn_body(c, who, B, Rdev, R ? "R" : "H", k, n_ref, Q, n_query, dims, n_dims, n_neighbors, metric, idx_out, dist_out);
    return knn_drain(c, rc, who);
}

}  // namespace

// ---- what the inverted-list search (kernels_knn_ivf.hip) calls: knn_device.h --------------------------------------------
int sgl_knn_args(const char* who, int32_t k, int64_t n_ref, int64_t n_query, const int32_t* dims, int32_t n_dims, int32_t n_neighbors) {
    return knn_args(who, k, n_ref, n_query, dims, n_dims, n_neighbors);
}
int sgl_knn_metric_arg(const char* who, int32_t metric) { return knn_metric_arg(who, metric); }
int sgl_knn_check_finite(sgl_ctx* c, const char* who, const char* name, const double* X, int32_t k, int64_t n, unsigned long long* first_dev) {
    return knn_check_finite(c, who, name, X, k, n, first_dev);
}
int sgl_knn_operand(sgl_ctx* c, const double* X, int32_t k, int64_t n, const int32_t* dims_dev, int nd, int32_t metric, double* packed,
                    double* transposed, unsigned long long* no_direction) {
    if (n == 0) return SGL_OK;
    if (metric != KNN_METRIC_EUCLIDEAN) {
        knn_unit<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream>>>(X, k, n, dims_dev, nd, metric == KNN_METRIC_CORRELATION ? 1 : 0,
                                                                              packed, transposed, no_direction);
        HIPCHK(hipGetLastError());
        return SGL_OK;
    }
    const dim3 grid((unsigned)(((int64_t)nd * n + 255) / 256));
    if (packed) {
        knn_gather<<<grid, dim3(256), 0, c->stream>>>(X, k, n, dims_dev, nd, 0, packed);
        HIPCHK(hipGetLastError());
    }
    if (transposed) {
        knn_gather<<<grid, dim3(256), 0, c->stream>>>(X, k, n, dims_dev, nd, 1, transposed);
        HIPCHK(hipGetLastError());
    }
    return SGL_OK;
}
int sgl_knn_scan(hipStream_t s, const KnnPlan& P, bool dot, const double* Rs, const double* Qs, int nd, int64_t nq, int64_t n_ref, int K,
                 double* cs, int32_t* ci, int32_t* idx, double* dist) {
    return dot ? launch_scan<true>(s, P, Rs, Qs, nd, nq, n_ref, K, cs, ci, idx, dist)
               : launch_scan<false>(s, P, Rs, Qs, nd, nq, n_ref, K, cs, ci, idx, dist);
}

extern "C" int sgl_knn(sgl_ctx* c, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims,
                       int32_t n_dims, int32_t n_neighbors, int32_t* idx_out, double* dist_out) {
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    return knn_entry(c, "sgl_knn", R, k, n_ref, Q, n_query, dims, n_dims, n_neighbors, KNN_METRIC_EUCLIDEAN, idx_out, dist_out);
}

extern "C" int sgl_c_knn(const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims, int32_t n_dims,
                         int32_t n_neighbors, int32_t* idx_out, double* dist_out) {
    if (!R) { sgl_set_error("sgl_c_knn: R is NULL"); return SGL_EINVAL; }
    SGLCHK(knn_args("sgl_c_knn", k, n_ref, n_query, dims, n_dims, n_neighbors));   // before a context is made
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    return knn_entry(hd.c, "sgl_c_knn", R, k, n_ref, Q, n_query, dims, n_dims, n_neighbors, KNN_METRIC_EUCLIDEAN, idx_out, dist_out);
}

extern "C" int sgl_knn_info(sgl_ctx* c, int64_t out[4]) {
    if (c == nullptr || out == nullptr) { sgl_set_error("sgl_knn_info: NULL context or output"); return SGL_EINVAL; }
    for (int q = 0; q < 4; ++q) out[q] = c->knn_last[q];
    return SGL_OK;
}

extern "C" int sgl_knn_metric(sgl_ctx* c, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims,
                              int32_t n_dims, int32_t n_neighbors, int32_t metric, int32_t* idx_out, double* dist_out) {
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    return knn_entry(c, "sgl_knn_metric", R, k, n_ref, Q, n_query, dims, n_dims, n_neighbors, metric, idx_out, dist_out);
}

extern "C" int sgl_c_knn_metric(const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims, int32_t n_dims,
                                int32_t n_neighbors, int32_t metric, int32_t* idx_out, double* dist_out) {
    if (!R) { sgl_set_error("sgl_c_knn_metric: R is NULL"); return SGL_EINVAL; }
    SGLCHK(knn_args("sgl_c_knn_metric", k, n_ref, n_query, dims, n_dims, n_neighbors));   // before a context is made
    SGLCHK(knn_metric_arg("sgl_c_knn_metric", metric));
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    return knn_entry(hd.c, "sgl_c_knn_metric", R, k, n_ref, Q, n_query, dims, n_dims, n_neighbors, metric, idx_out, dist_out);
}

extern "C" int sgl_knn_metric_info(sgl_ctx* c, int64_t out[6]) {
    if (c == nullptr || out == nullptr) { sgl_set_error("sgl_knn_metric_info: NULL context or output"); return SGL_EINVAL; }
    for (int q = 0; q < 6; ++q) out[q] = c->knn_last[q];
    return SGL_OK;
}
