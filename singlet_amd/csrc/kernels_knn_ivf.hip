// Approximate neighbours in a k x n embedding by an inverted-file search (include/singlet_hip.h, "Approximate embedding
// neighbours": sgl_knn_ivf, sgl_op_ivf_train, sgl_op_ivf_search).  gfx950 only, wave64, compiled with -ffp-contract=off.
//
// A coarse k-means over the operands of sgl_knn_metric cuts the references into lists; a query scans the n_probe lists whose
// centroids are nearest; inside them the sums, the keys and the ranking are those of kernels_knn.hip, through the same code
// (knn_device.h), so that n_probe == n_lists gives the exact search bit for bit.
//
//   operands             knn_gather / knn_unit of kernels_knn.hip (sgl_knn_operand)
//   assignment, probes   the exact scan and merge of kernels_knn.hip with the centroids as the references (sgl_knn_scan): one
//                        neighbour for a Lloyd step and for the final assignment, n_probe for the probes
//   centroid update      sgl_group_sums_dev (kernels_group.hip) as it is: the order sgl_group_means documents
//   ivf_take_columns     training picks and seeds: column t of the output is column floor(t n_from / n_take) of the input
//   ivf_reorder          the packed references in list order
//   knn_scan_lists_reg / knn_scan_lists_generic   the list scan below
//   knn_finish_lists     knn_finish's merge over the n_probe probe slots; the padding goes out as -1 / +Inf and is counted
//
// The list scan.  The host sorts the (query, probe slot) pairs of a batch stably by probed list and cuts every list's pairs into
// blocks of 64 x queries-per-lane (knn_ivf_host.h).  One workgroup is one wave and takes one block: its list, the list's
// bounds and the block's pair range depend on blockIdx alone and arrive through scalar loads.  A lane owns its pairs' queries:
// for n_dims <= 64 their coordinates sit in registers, in the instance families, chunks and padding of knn_scan_reg.  The
// list's members stream in stored order -- ascending cell index --; a member's coordinates and its cell index are wave-uniform
// and reach the FP64 instructions as scalar operands.  The candidate offered is the member's cell index, so knn_insert's
// "behind every entry whose s is not greater" keeps ties with the lower index.  The lists live in LDS up to 32 neighbours,
// above in the candidate array itself.  A pair writes the candidates of its probe slot: cs / ci are n_probe x K x queries of
// the batch, exactly the segments knn_finish merges.  No floating-point atomics; 64-bit offsets.
#include "sgl_internal.h"
#include "knn_ivf_host.h"
#include "knn_transfer_host.h"
#include "knn_device.h"
#include "umap_transform_dev.h"

#include <chrono>
#include <cmath>
#include <functional>
#include <limits>
#include <vector>

namespace {

constexpr int IVF_TILE = 8;   // members per tile of the generic scan (KNN_TILE of kernels_knn.hip)

// out[t * nd + f] = X[floor(t * n_from / n_take) * nd + f]
__global__ __launch_bounds__(256) void ivf_take_columns(const double* __restrict__ X, int nd, int64_t n_from, int64_t n_take,
                                                        double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_take * nd) return;
    const int64_t t = e / nd;
    const int f = (int)(e - t * nd);
    out[e] = X[(t * n_from / n_take) * nd + f];
}

// out[pos * nd + f] = X[cell[pos] * nd + f]
__global__ __launch_bounds__(256) void ivf_reorder(const double* __restrict__ X, int nd, const int32_t* __restrict__ cell, int64_t n,
                                                   double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * nd) return;
    const int64_t pos = e / nd;
    const int f = (int)(e - pos * nd);
    out[e] = X[(int64_t)cell[pos] * nd + f];
}

// What the host's task table and the bucketing hand to the scan (device pointers).
struct IvfTasks {
    const int32_t* pair_query;    // sorted pairs: the query (index inside the batch) ...
    const int32_t* pair_slot;     // ... and its probe slot
    const int32_t* block_list;    // block b scans this list ...
    const int64_t* block_begin;   // ... for the pairs block_begin[b] .. block_begin[b + 1]
    const int64_t* off;           // list g is the positions off[g] .. off[g + 1] of Rl and cell
    const int32_t* cell;          // position -> reference index
};

// The lists of one lane's QPL pairs: KnnLists of kernels_knn.hip with the pair's (query, probe slot) in place of
// (query, segment).  q[u]: the query whose coordinates the lane computes on (a lane without a pair: a copy of the block's last).
template <int QPL, bool LISTS_GLOBAL>
struct IvfLists {
    double* ld[QPL];
    int32_t* li[QPL];
    int64_t stride;
    int cnt[QPL];
    double worst[QPL];
    bool mine[QPL];
    int64_t q[QPL];
    double* out_d[QPL];
    int32_t* out_i[QPL];

    __device__ __forceinline__ void init(double* lds, const IvfTasks& T, int64_t pb, int64_t pe, int lane, int64_t nq, int K, double* cs,
                                         int32_t* ci) {
        stride = LISTS_GLOBAL ? nq : 64 * QPL;
#pragma unroll
        for (int u = 0; u < QPL; ++u) {
            const int64_t at = pb + u * 64 + lane;
            mine[u] = at < pe;
            const int64_t ac = mine[u] ? at : pe - 1;   // a block holds at least one pair
            q[u] = T.pair_query[ac];
            const int64_t base = (int64_t)T.pair_slot[ac] * K * nq + q[u];
            out_d[u] = cs + base;
            out_i[u] = ci + base;
            if (LISTS_GLOBAL) {
                ld[u] = out_d[u];
                li[u] = out_i[u];
            } else {
                ld[u] = lds + u * 64 + lane;
                li[u] = reinterpret_cast<int32_t*>(lds + (int64_t)64 * QPL * K) + u * 64 + lane;
            }
            cnt[u] = mine[u] ? 0 : K;   // a lane without a pair takes nothing: its list is "full" and no key is below -1
            worst[u] = mine[u] ? std::numeric_limits<double>::infinity() : -1.0;
        }
    }
    __device__ __forceinline__ void offer(int u, int K, double s, int32_t r) {
        if (cnt[u] < K || s < worst[u]) knn_insert(ld[u], li[u], stride, K, cnt[u], worst[u], s, r);
    }
    __device__ __forceinline__ void flush(int K, int64_t nq) {
#pragma unroll
        for (int u = 0; u < QPL; ++u) {
            if (!mine[u]) continue;
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

// n_dims in [NDLO, NDHI], chunks of CH: the loop body of knn_scan_reg, over the members of one list.
template <int NDLO, int NDHI, int CH, int QPL, bool LISTS_GLOBAL, bool DOT>
__global__ __launch_bounds__(64) void knn_scan_lists_reg(const double* __restrict__ Rl, const double* __restrict__ Q, int nd, int64_t nq,
                                                         IvfTasks T, int K, double* __restrict__ cs, int32_t* __restrict__ ci) {
    static_assert(NDHI % CH == 0, "whole chunks");
    extern __shared__ double ivf_lds[];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int32_t g = T.block_list[b];
    const int64_t lo = T.off[g], hi = T.off[g + 1];
    IvfLists<QPL, LISTS_GLOBAL> L;
    L.init(ivf_lds, T, T.block_begin[b], T.block_begin[b + 1], lane, nq, K, cs, ci);
    double q[QPL][NDHI];
#pragma unroll
    for (int u = 0; u < QPL; ++u) {
        const double* qp = Q + L.q[u] * nd;
#pragma unroll
        for (int f = 0; f < NDHI; ++f) q[u][f] = f < nd ? qp[f] : 0.0;
    }
    for (int64_t r = lo; r < hi; ++r) {
        const double* __restrict__ rp = Rl + r * nd;   // wave-uniform: scalar loads
        const int32_t id = T.cell[r];
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
        for (int u = 0; u < QPL; ++u) L.offer(u, K, knn_key<DOT>(s[u]), id);
    }
    L.flush(K, nq);
}

// Every rank above 64: a lane owns one pair and reads its query's packed column four dimensions at a time; the running sums
// of a tile of IVF_TILE members stay in registers over the loop over the dimensions (the body of knn_scan_generic).
template <bool LISTS_GLOBAL, bool DOT>
__global__ __launch_bounds__(64) void knn_scan_lists_generic(const double* __restrict__ Rl, const double* __restrict__ Q, int nd, int64_t nq,
                                                             IvfTasks T, int K, double* __restrict__ cs, int32_t* __restrict__ ci) {
    constexpr int CH = 4;
    extern __shared__ double ivf_lds[];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int32_t g = T.block_list[b];
    const int64_t lo = T.off[g], hi = T.off[g + 1];
    IvfLists<1, LISTS_GLOBAL> L;
    L.init(ivf_lds, T, T.block_begin[b], T.block_begin[b + 1], lane, nq, K, cs, ci);
    const double* qp = Q + L.q[0] * nd;
    for (int64_t r0 = lo; r0 < hi; r0 += IVF_TILE) {
        const double* __restrict__ rp[IVF_TILE];
#pragma unroll
        for (int i = 0; i < IVF_TILE; ++i) rp[i] = Rl + (r0 + i < hi ? r0 + i : hi - 1) * nd;   // past the end: the last one again, not offered
        double s[IVF_TILE];
#pragma unroll
        for (int i = 0; i < IVF_TILE; ++i) s[i] = 0.0;
        int f = 0;
        for (; f + CH <= nd; f += CH) {
            double qf[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) qf[e] = qp[f + e];
#pragma unroll
            for (int i = 0; i < IVF_TILE; ++i) {
#pragma unroll
                for (int e = 0; e < CH; ++e) s[i] = knn_step<DOT>(s[i], qf[e], rp[i][f + e]);
            }
        }
        if (f < nd) {
            double qf[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const double v = qp[f + e < nd ? f + e : nd - 1];
                qf[e] = f + e < nd ? v : 0.0;
            }
#pragma unroll
            for (int i = 0; i < IVF_TILE; ++i) {
#pragma unroll
                for (int e = 0; e < CH; ++e) {
                    const double v = rp[i][f + e < nd ? f + e : nd - 1];
                    s[i] = knn_step<DOT>(s[i], qf[e], f + e < nd ? v : 0.0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < IVF_TILE; ++i)
            if (r0 + i < hi) L.offer(0, K, knn_key<DOT>(s[i]), T.cell[r0 + i]);
    }
    L.flush(K, nq);
}

// knn_finish over the probe slots.  A slot's list ends in (+Inf, INT32_MAX) where its list held fewer than K members; no
// cell index is INT32_MAX, so a head with that index means every slot is exhausted: it goes out as -1 / +Inf, and the query
// counts as short, once.
template <bool ROOT>
__global__ __launch_bounds__(256) void knn_finish_lists(const double* __restrict__ cs, const int32_t* __restrict__ ci, int nseg, int K, int64_t nq,
                                                        int32_t* __restrict__ idx_out, double* __restrict__ dist_out,
                                                        unsigned long long* __restrict__ short_queries) {
    __shared__ uint16_t head[KNN_IVF_MAX_PROBES][256];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    if (j >= nq) return;
    for (int g = 0; g < nseg; ++g) head[g][tid] = 0;
    bool is_short = false;
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
        const bool pad = bi == INT32_MAX;
        is_short = is_short || pad;
        if (idx_out) idx_out[j * K + t] = pad ? -1 : bi;
        if (dist_out) dist_out[j * K + t] = pad ? std::numeric_limits<double>::infinity() : (ROOT ? __builtin_sqrt(bd) : bd);
    }
    if (is_short) atomicAdd(short_queries, 1ull);
}

template <int NDLO, int NDHI, int CH, int QPL, bool DOT>
int launch_lists_reg(hipStream_t s, int64_t blocks, bool lists_global, size_t lds, const double* Rl, const double* Q, int nd, int64_t nq,
                     const IvfTasks& T, int K, double* cs, int32_t* ci) {
    if (lists_global)
        knn_scan_lists_reg<NDLO, NDHI, CH, QPL, true, DOT><<<dim3((unsigned)blocks), dim3(64), 0, s>>>(Rl, Q, nd, nq, T, K, cs, ci);
    else
        knn_scan_lists_reg<NDLO, NDHI, CH, QPL, false, DOT><<<dim3((unsigned)blocks), dim3(64), lds, s>>>(Rl, Q, nd, nq, T, K, cs, ci);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

template <bool DOT>
int launch_lists(hipStream_t s, int instance, int64_t blocks, const double* Rl, const double* Q, int nd, int64_t nq, const IvfTasks& T, int K,
                 double* cs, int32_t* ci) {
    const bool lists_global = K > KNN_LDS_MAX_NEIGHBORS;
    const size_t lds = lists_global ? 0 : (size_t)knn_ivf_pairs_per_block(nd) * (size_t)K * 12;
    switch (instance) {
    case 0: return launch_lists_reg<1, 8, 2, 2, DOT>(s, blocks, lists_global, lds, Rl, Q, nd, nq, T, K, cs, ci);
    case 1: return launch_lists_reg<9, 16, 4, 2, DOT>(s, blocks, lists_global, lds, Rl, Q, nd, nq, T, K, cs, ci);
    case 2: return launch_lists_reg<17, 32, 8, 2, DOT>(s, blocks, lists_global, lds, Rl, Q, nd, nq, T, K, cs, ci);
    case 3: return launch_lists_reg<33, 64, 8, 1, DOT>(s, blocks, lists_global, lds, Rl, Q, nd, nq, T, K, cs, ci);
    default:
        if (lists_global)
            knn_scan_lists_generic<true, DOT><<<dim3((unsigned)blocks), dim3(64), 0, s>>>(Rl, Q, nd, nq, T, K, cs, ci);
        else
            knn_scan_lists_generic<false, DOT><<<dim3((unsigned)blocks), dim3(64), lds, s>>>(Rl, Q, nd, nq, T, K, cs, ci);
        HIPCHK(hipGetLastError());
    }
    return SGL_OK;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
enum { ST_OPERANDS = 0, ST_LLOYD, ST_ASSIGN, ST_BUCKET, ST_PROBES, ST_TASKS, ST_SCAN, ST_MERGE, ST_COUNT };

// A buffer that grows and never shrinks.  It is (re)allocated only while nothing of the call is in flight: every stage that
// asks for one ends in a stream synchronisation before the next asks again.
template <typename T>
struct Grow {
    DevBuf<T> b;
    size_t cap = 0;
    T* p() const { return b.p; }
    int need(size_t n) {
        if (n == 0) n = 1;
        if (b.p && n <= cap) return SGL_OK;
        cap = n;
        return b.alloc(n);
    }
};

struct IvfBuffers {
    DevBuf<double> R, Q, Rp, Qp, Rl, C, Tr;
    DevBuf<int32_t> dims, cell;
    DevBuf<int64_t> off;
    DevBuf<unsigned long long> first, no_direction, short_queries;
    Grow<double> Xt, cs, dist;       // the coarse scans' transposed queries, candidates, distances of a batch
    Grow<int32_t> ci, near, idx;     // candidates, the nearest centroids of a coarse scan, the result of a batch
    Grow<int32_t> pair_query, pair_slot, block_list;
    Grow<int64_t> block_begin;
    // what the operand stage leaves
    const double* Rs = nullptr;      // packed references, nd x n_ref
    const double* Qs = nullptr;      // packed queries, nd x nq
    int64_t nq = 0;
    int nd = 0;
};

// Stage times of the last search, when timing is on: GPU stages between two events on the stream, the host-built task table
// by the host clock.
struct StageClock {
    sgl_ctx* c;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool on = false;
    std::chrono::steady_clock::time_point h0;
    explicit StageClock(sgl_ctx* c_, bool enabled = true) : c(c_) {   // enabled false: the calls on a kept index, which time no stage
        on = enabled && c->timing && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
        if (!on) (void)hipGetLastError();
    }
    ~StageClock() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void begin() { if (on) (void)hipEventRecord(e0, c->stream); }
    void end(int stage) {
        if (!on) return;
        float ms = 0.f;
        if (hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
            c->knn_ivf_ms[stage] += (double)ms;
        else
            (void)hipGetLastError();
    }
    void host_begin() { if (on) h0 = std::chrono::steady_clock::now(); }
    void host_end(int stage) {
        if (on) c->knn_ivf_ms[stage] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    }
};

int ivf_drain(sgl_ctx* c, int rc, const char* who) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("%s: HIP call failed: %s", who, hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

int ivf_args(const char* who, int64_t n_ref, int32_t n_lists, int32_t n_probe, int32_t n_iter, int32_t metric) {
    switch (knn_ivf_check_args(n_ref, n_lists, n_probe, n_iter, metric)) {
    case KNN_IVF_ARGS_OK: return SGL_OK;
    case KNN_IVF_ARGS_LISTS:
        sgl_set_error("%s: n_lists = %d is outside [1, min(n_ref = %lld, %d)]", who, n_lists, (long long)n_ref, KNN_IVF_MAX_LISTS);
        break;
    case KNN_IVF_ARGS_PROBES:
        sgl_set_error("%s: n_probe = %d is outside [1, min(n_lists = %d, %d)]", who, n_probe, n_lists, KNN_IVF_MAX_PROBES);
        break;
    case KNN_IVF_ARGS_ITER: sgl_set_error("%s: n_iter = %d is outside [0, %d]", who, n_iter, KNN_IVF_MAX_ITER); break;
    case KNN_IVF_ARGS_METRIC: return sgl_knn_metric_arg(who, metric);
    }
    return SGL_EINVAL;
}

// sgl_knn's state refusals, in its order and words
int ivf_state(sgl_ctx* c, const char* who, const double* R, int32_t k, int64_t n_ref) {
    if (c->team || c->allreduce) {
        sgl_set_error("%s: the context is a shard of a team or has an all-reduce hook; the H of this shard's cells is not the embedding", who);
        return SGL_ESTATE;
    }
    if (!R && c->k == 0) { sgl_set_error("%s: R is NULL and no fit is initialised (call sgl_fit_init)", who); return SGL_ESTATE; }
    if (!R && (k != c->k || n_ref != c->A.ncol)) {
        sgl_set_error("%s: R is NULL, but k = %d, n_ref = %lld are not the fit's %d x %d", who, k, (long long)n_ref, c->k, c->A.ncol);
        return SGL_EINVAL;
    }
    return SGL_OK;
}

// The operands of sgl_knn_metric: uploads, the finiteness pass on the raw operands, the packed columns.  with_queries false:
// the references alone (the training operator).
int ivf_operands(sgl_ctx* c, const char* who, IvfBuffers& B, const double* R, int32_t k, int64_t n_ref, bool with_queries, const double* Q,
                 int64_t n_query, const int32_t* dims, int32_t n_dims, int32_t metric, unsigned long long* no_direction) {
    const double* Rdev = c->H;
    if (R) {
        SGLCHK(B.R.alloc((size_t)k * (size_t)n_ref));
        HIPCHK(hipMemcpyAsync(B.R.p, R, sizeof(double) * (size_t)k * (size_t)n_ref, hipMemcpyHostToDevice, c->stream));
        Rdev = B.R.p;
    }
    const bool own_queries = with_queries && Q;
    const double* Qdev = Rdev;
    B.nq = with_queries ? n_ref : 0;
    if (own_queries) {
        B.nq = n_query;
        SGLCHK(B.Q.alloc((size_t)k * (size_t)std::max<int64_t>(n_query, 1)));
        if (n_query > 0) HIPCHK(hipMemcpyAsync(B.Q.p, Q, sizeof(double) * (size_t)k * (size_t)n_query, hipMemcpyHostToDevice, c->stream));
        Qdev = B.Q.p;
    }
    SGLCHK(B.first.alloc(1));
    SGLCHK(sgl_knn_check_finite(c, who, R ? "R" : "H", Rdev, k, n_ref, B.first.p));
    if (own_queries) SGLCHK(sgl_knn_check_finite(c, who, "Q", Qdev, k, n_query, B.first.p));
    B.nd = dims ? n_dims : k;
    if (dims) {
        SGLCHK(B.dims.alloc((size_t)B.nd));
        HIPCHK(hipMemcpyAsync(B.dims.p, dims, sizeof(int32_t) * (size_t)B.nd, hipMemcpyHostToDevice, c->stream));
    }
    SGLCHK(B.no_direction.alloc(1));
    HIPCHK(hipMemsetAsync(B.no_direction.p, 0, sizeof(unsigned long long), c->stream));
    SGLCHK(B.Rp.alloc((size_t)B.nd * (size_t)n_ref));
    if (own_queries) SGLCHK(B.Qp.alloc((size_t)B.nd * (size_t)std::max<int64_t>(n_query, 1)));
    {
        Phase ph(c, SGL_PH_GRAM);   // as sgl_knn_metric books knn_unit
        SGLCHK(sgl_knn_operand(c, Rdev, k, n_ref, B.dims.p, B.nd, metric, B.Rp.p, nullptr, B.no_direction.p));
        if (own_queries) SGLCHK(sgl_knn_operand(c, Qdev, k, n_query, B.dims.p, B.nd, metric, B.Qp.p, nullptr, B.no_direction.p));
    }
    B.Rs = B.Rp.p;
    B.Qs = own_queries ? B.Qp.p : B.Rp.p;
    HIPCHK(hipMemcpyAsync(no_direction, B.no_direction.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SGL_OK;
}

// near[j * K + t] (device, B.near): the K centroids nearest to column j of the packed nd x n columns X, by (s, centroid index)
// -- sgl_knn's Euclidean scan and merge with the centroids as the references.  Launches only; nothing of an earlier stage
// may be in flight (the buffers may move).
int ivf_nearest(sgl_ctx* c, IvfBuffers& B, const double* C, int32_t n_lists, const double* X, int64_t n, int K) {
    const int nd = B.nd;
    const KnnPlan P = knn_plan(n, n_lists, nd, K);
    const double* Qs = X;
    if (P.instance == KNN_GENERIC_INSTANCE) {
        SGLCHK(B.Xt.need((size_t)nd * (size_t)n));
        SGLCHK(sgl_knn_operand(c, X, nd, n, nullptr, nd, KNN_METRIC_EUCLIDEAN, nullptr, B.Xt.p(), nullptr));
        Qs = B.Xt.p();
    }
    const size_t slots = (size_t)P.segments * (size_t)K * (size_t)n;
    SGLCHK(B.cs.need(slots));
    SGLCHK(B.ci.need(slots));
    SGLCHK(B.near.need((size_t)K * (size_t)n));
    return sgl_knn_scan(c->stream, P, false, C, Qs, nd, n, n_lists, K, B.cs.p(), B.ci.p(), B.near.p(), nullptr);
}

// Training on the packed references B.Rs: the centroids on the device (B.C) and on the host, and the list of every reference.
int ivf_train(sgl_ctx* c, IvfBuffers& B, StageClock& clk, int64_t n_ref, int32_t n_lists, int32_t n_iter, std::vector<double>& Chost,
              std::vector<int32_t>& assign, int64_t* T_out) {
    const int nd = B.nd;
    const int64_t T = knn_ivf_train_count(n_ref, n_lists);
    *T_out = T;
    const size_t csize = (size_t)nd * (size_t)n_lists;
    Chost.resize(csize);
    assign.resize((size_t)n_ref);
    SGLCHK(B.Tr.alloc((size_t)nd * (size_t)T));
    SGLCHK(B.C.alloc(csize));
    clk.begin();
    ivf_take_columns<<<dim3((unsigned)(((int64_t)nd * T + 255) / 256)), dim3(256), 0, c->stream>>>(B.Rs, nd, n_ref, T, B.Tr.p);
    HIPCHK(hipGetLastError());
    ivf_take_columns<<<dim3((unsigned)(((int64_t)nd * n_lists + 255) / 256)), dim3(256), 0, c->stream>>>(B.Tr.p, nd, T, n_lists, B.C.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(Chost.data(), B.C.p, sizeof(double) * csize, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<int32_t> tassign((size_t)T);
    std::vector<double> means(csize);
    std::vector<int64_t> counts((size_t)n_lists);
    for (int32_t it = 0; it < n_iter; ++it) {
        SGLCHK(ivf_nearest(c, B, B.C.p, n_lists, B.Tr.p, T, 1));
        HIPCHK(hipMemcpyAsync(tassign.data(), B.near.p(), sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        // the mean of every list's training cells in sgl_group_means' order (it synchronises); 0 cells: NaN, and the centroid stays
        SGLCHK(sgl_group_sums_dev(c, B.Tr.p, nd, T, tassign.data(), n_lists, true, means.data(), counts.data()));
        for (int32_t g = 0; g < n_lists; ++g)
            if (counts[(size_t)g] > 0)
                for (int f = 0; f < nd; ++f) Chost[(size_t)g * nd + f] = means[(size_t)g * nd + f];
        HIPCHK(hipMemcpyAsync(B.C.p, Chost.data(), sizeof(double) * csize, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    clk.end(ST_LLOYD);
    clk.begin();
    SGLCHK(ivf_nearest(c, B, B.C.p, n_lists, B.Rs, n_ref, 1));
    HIPCHK(hipMemcpyAsync(assign.data(), B.near.p(), sizeof(int32_t) * (size_t)n_ref, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    clk.end(ST_ASSIGN);
    return SGL_OK;
}

// What a search reads of the lists (device pointers): the one-shot calls point it at their own buffers, a kept index at its own.
struct IvfResident {
    const double* Rl;      // the packed references in list order
    const double* C;       // the centroids
    const int64_t* off;
    const int32_t* cell;
    int32_t n_lists;
};

// Called once per batch of queries with the batch's result still on the device: idx / dist are n_neighbors x nb (B.idx, B.dist).
// The stream has been synchronised when it returns.
typedef std::function<int(int64_t q0, int64_t nb, const int32_t* idx_dev, const double* dist_dev)> IvfAfterBatch;

// Bucketing under a checked assignment: list offsets and the table from position to cell on the host, the packed references
// in list order on the device (B.off, B.cell, B.Rl).  info: the lists' part of what sgl_knn_ivf_info reports.
int ivf_bucket(sgl_ctx* c, IvfBuffers& B, StageClock& clk, int64_t n_ref, int32_t n_lists, const int32_t* assign, int64_t info[8]) {
    const int nd = B.nd;
    clk.begin();
    std::vector<int64_t> off((size_t)n_lists + 1);
    std::vector<int32_t> cell((size_t)n_ref);
    knn_ivf_bucket(assign, n_ref, n_lists, off.data(), cell.data());
    SGLCHK(B.off.alloc(off.size()));
    SGLCHK(B.cell.alloc(cell.size()));
    SGLCHK(B.Rl.alloc((size_t)nd * (size_t)n_ref));
    HIPCHK(hipMemcpyAsync(B.off.p, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(B.cell.p, cell.data(), sizeof(int32_t) * cell.size(), hipMemcpyHostToDevice, c->stream));
    ivf_reorder<<<dim3((unsigned)(((int64_t)nd * n_ref + 255) / 256)), dim3(256), 0, c->stream>>>(B.Rs, nd, B.cell.p, n_ref, B.Rl.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    clk.end(ST_BUCKET);
    info[0] = n_lists;
    knn_ivf_list_stats(off.data(), n_lists, &info[3], &info[4], &info[5]);
    info[6] = 0;
    info[7] = knn_instance(nd);
    return SGL_OK;
}

// The queries B.Qs (packed, nd x B.nq) against the lists S: probes, task table, list scan and merge, in batches.  info[1], [6]
// and [7] are filled here.  after: see IvfAfterBatch (may be empty).
int ivf_query(sgl_ctx* c, IvfBuffers& B, StageClock& clk, const IvfResident& S, int32_t K, int32_t metric, int32_t n_probe, int64_t query_batch,
              int32_t* idx_out, double* dist_out, int64_t info[8], const IvfAfterBatch& after) {
    const int nd = B.nd;
    const int64_t nq = B.nq;
    const int32_t n_lists = S.n_lists;
    info[1] = n_probe;
    info[6] = 0;
    info[7] = knn_instance(nd);
    if (nq == 0) return SGL_OK;
    SGLCHK(B.short_queries.alloc(1));
    HIPCHK(hipMemsetAsync(B.short_queries.p, 0, sizeof(unsigned long long), c->stream));

    const int ppb = knn_ivf_pairs_per_block(nd);
    const int64_t batch = knn_ivf_batch(nq, n_probe, K, query_batch, KNN_IVF_SCRATCH_BYTES);
    std::vector<int32_t> probes, pair_query, pair_slot, block_list;
    std::vector<int64_t> first((size_t)n_lists + 1), cursor((size_t)n_lists), block_begin;
    for (int64_t q0 = 0; q0 < nq; q0 += batch) {
        const int64_t nb = std::min(batch, nq - q0);
        const int64_t n_pairs = nb * n_probe;
        const double* Xb = B.Qs + q0 * nd;
        clk.begin();
        SGLCHK(ivf_nearest(c, B, S.C, n_lists, Xb, nb, n_probe));
        probes.resize((size_t)n_pairs);
        HIPCHK(hipMemcpyAsync(probes.data(), B.near.p(), sizeof(int32_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        clk.end(ST_PROBES);
        clk.host_begin();
        const int64_t blocks = knn_ivf_task_count(probes.data(), nb, n_probe, n_lists, ppb, first.data());
        pair_query.resize((size_t)n_pairs);
        pair_slot.resize((size_t)n_pairs);
        block_list.resize((size_t)blocks);
        block_begin.resize((size_t)blocks + 1);
        knn_ivf_task_fill(probes.data(), nb, n_probe, n_lists, ppb, first.data(), cursor.data(), pair_query.data(), pair_slot.data(),
                          block_list.data(), block_begin.data());
        clk.host_end(ST_TASKS);
        const size_t slots = (size_t)n_pairs * (size_t)K;
        SGLCHK(B.pair_query.need((size_t)n_pairs));
        SGLCHK(B.pair_slot.need((size_t)n_pairs));
        SGLCHK(B.block_list.need((size_t)blocks));
        SGLCHK(B.block_begin.need((size_t)blocks + 1));
        SGLCHK(B.cs.need(slots));
        SGLCHK(B.ci.need(slots));
        SGLCHK(B.idx.need((size_t)K * (size_t)nb));
        SGLCHK(B.dist.need((size_t)K * (size_t)nb));
        HIPCHK(hipMemcpyAsync(B.pair_query.p(), pair_query.data(), sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(B.pair_slot.p(), pair_slot.data(), sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(B.block_list.p(), block_list.data(), sizeof(int32_t) * (size_t)blocks, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(B.block_begin.p(), block_begin.data(), sizeof(int64_t) * ((size_t)blocks + 1), hipMemcpyHostToDevice, c->stream));
        const IvfTasks T = {B.pair_query.p(), B.pair_slot.p(), B.block_list.p(), B.block_begin.p(), S.off, S.cell};
        const bool dot = metric != KNN_METRIC_EUCLIDEAN;
        {
            Phase ph(c, SGL_PH_SCALE);   // scan and merge, as under sgl_knn
            clk.begin();
            if (dot) SGLCHK(launch_lists<true>(c->stream, (int)info[7], blocks, S.Rl, Xb, nd, nb, T, K, B.cs.p(), B.ci.p()));
            else SGLCHK(launch_lists<false>(c->stream, (int)info[7], blocks, S.Rl, Xb, nd, nb, T, K, B.cs.p(), B.ci.p()));
            clk.end(ST_SCAN);
            clk.begin();
            const dim3 grid((unsigned)((nb + 255) / 256));
            if (dot)
                knn_finish_lists<false><<<grid, dim3(256), 0, c->stream>>>(B.cs.p(), B.ci.p(), n_probe, K, nb, B.idx.p(), B.dist.p(), B.short_queries.p);
            else
                knn_finish_lists<true><<<grid, dim3(256), 0, c->stream>>>(B.cs.p(), B.ci.p(), n_probe, K, nb, B.idx.p(), B.dist.p(), B.short_queries.p);
            HIPCHK(hipGetLastError());
            clk.end(ST_MERGE);
        }
        if (idx_out) HIPCHK(hipMemcpyAsync(idx_out + q0 * K, B.idx.p(), sizeof(int32_t) * (size_t)K * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        if (dist_out) HIPCHK(hipMemcpyAsync(dist_out + q0 * K, B.dist.p(), sizeof(double) * (size_t)K * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        if (after) SGLCHK(after(q0, nb, B.idx.p(), B.dist.p()));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    unsigned long long short_queries = 0;
    HIPCHK(hipMemcpyAsync(&short_queries, B.short_queries.p, sizeof(short_queries), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    info[6] = (int64_t)short_queries;
    return SGL_OK;
}

// The search under the centroids B.C (device) and a checked assignment.  info: what sgl_knn_ivf_info reports, filled here
// except the training cells.
int ivf_search(sgl_ctx* c, IvfBuffers& B, StageClock& clk, int64_t n_ref, int32_t K, int32_t metric, int32_t n_lists, const int32_t* assign,
               int32_t n_probe, int64_t query_batch, int32_t* idx_out, double* dist_out, int64_t info[8]) {
    SGLCHK(ivf_bucket(c, B, clk, n_ref, n_lists, assign, info));
    const IvfResident S = {B.Rl.p, B.C.p, B.off.p, B.cell.p, n_lists};
    return ivf_query(c, B, clk, S, K, metric, n_probe, query_batch, idx_out, dist_out, info, IvfAfterBatch());
}

void ivf_clock_reset(sgl_ctx* c) {
    for (int q = 0; q < ST_COUNT; ++q) c->knn_ivf_ms[q] = 0.0;
}

int knn_ivf_entry(sgl_ctx* c, const char* who, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims,
                  int32_t n_dims, int32_t K, int32_t metric, int32_t n_lists, int32_t n_probe, int32_t n_iter, int32_t* idx_out,
                  double* dist_out) {
    SGLCHK(ivf_state(c, who, R, k, n_ref));
    SGLCHK(sgl_knn_args(who, k, n_ref, n_query, dims, n_dims, K));
    SGLCHK(ivf_args(who, n_ref, n_lists, n_probe, n_iter, metric));
    IvfBuffers B;
    StageClock clk(c);
    ivf_clock_reset(c);
    std::vector<double> Chost;
    std::vector<int32_t> assign;
    int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long no_direction = 0;
    clk.begin();
    int rc = ivf_operands(c, who, B, R, k, n_ref, true, Q, n_query, dims, n_dims, metric, &no_direction);
    clk.end(ST_OPERANDS);
    if (rc == SGL_OK) rc = ivf_train(c, B, clk, n_ref, n_lists, n_iter, Chost, assign, &info[2]);
    if (rc == SGL_OK) rc = ivf_search(c, B, clk, n_ref, K, metric, n_lists, assign.data(), n_probe, 0, idx_out, dist_out, info);
    rc = ivf_drain(c, rc, who);
    if (rc == SGL_OK)
        for (int q = 0; q < 8; ++q) c->knn_ivf_last[q] = info[q];
    return rc;
}

}  // namespace

extern "C" int sgl_knn_ivf(sgl_ctx* c, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims,
                           int32_t n_dims, int32_t n_neighbors, int32_t metric, int32_t n_lists, int32_t n_probe, int32_t n_iter,
                           int32_t* idx_out, double* dist_out) {
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    return knn_ivf_entry(c, "sgl_knn_ivf", R, k, n_ref, Q, n_query, dims, n_dims, n_neighbors, metric, n_lists, n_probe, n_iter, idx_out, dist_out);
}

extern "C" int sgl_c_knn_ivf(const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims, int32_t n_dims,
                             int32_t n_neighbors, int32_t metric, int32_t n_lists, int32_t n_probe, int32_t n_iter, int32_t* idx_out,
                             double* dist_out) {
    if (!R) { sgl_set_error("sgl_c_knn_ivf: R is NULL"); return SGL_EINVAL; }
    SGLCHK(sgl_knn_args("sgl_c_knn_ivf", k, n_ref, n_query, dims, n_dims, n_neighbors));   // before a context is made
    SGLCHK(ivf_args("sgl_c_knn_ivf", n_ref, n_lists, n_probe, n_iter, metric));
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    return knn_ivf_entry(hd.c, "sgl_c_knn_ivf", R, k, n_ref, Q, n_query, dims, n_dims, n_neighbors, metric, n_lists, n_probe, n_iter, idx_out,
                         dist_out);
}

extern "C" int sgl_knn_ivf_info(sgl_ctx* c, int64_t out[8]) {
    if (c == nullptr || out == nullptr) { sgl_set_error("sgl_knn_ivf_info: NULL context or output"); return SGL_EINVAL; }
    for (int q = 0; q < 8; ++q) out[q] = c->knn_ivf_last[q];
    return SGL_OK;
}

extern "C" int sgl_knn_ivf_stage_ms(sgl_ctx* c, double out[8]) {
    if (c == nullptr || out == nullptr) { sgl_set_error("sgl_knn_ivf_stage_ms: NULL context or output"); return SGL_EINVAL; }
    for (int q = 0; q < ST_COUNT; ++q) out[q] = c->knn_ivf_ms[q];
    return SGL_OK;
}

extern "C" int sgl_op_ivf_train(sgl_ctx* c, const double* R, int32_t k, int64_t n_ref, const int32_t* dims, int32_t n_dims, int32_t metric,
                                int32_t n_lists, int32_t n_iter, double* centroids_out, int32_t* assign_out) {
    const char* who = "sgl_op_ivf_train";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    SGLCHK(ivf_state(c, who, R, k, n_ref));
    SGLCHK(sgl_knn_args(who, k, n_ref, 0, dims, n_dims, 1));
    SGLCHK(ivf_args(who, n_ref, n_lists, 1, n_iter, metric));
    if (!centroids_out || !assign_out) { sgl_set_error("%s: centroids_out or assign_out is NULL", who); return SGL_EINVAL; }
    IvfBuffers B;
    StageClock clk(c);
    ivf_clock_reset(c);
    std::vector<double> Chost;
    std::vector<int32_t> assign;
    int64_t T = 0;
    unsigned long long no_direction = 0;
    clk.begin();
    int rc = ivf_operands(c, who, B, R, k, n_ref, false, nullptr, 0, dims, n_dims, metric, &no_direction);
    clk.end(ST_OPERANDS);
    if (rc == SGL_OK) rc = ivf_train(c, B, clk, n_ref, n_lists, n_iter, Chost, assign, &T);
    rc = ivf_drain(c, rc, who);
    if (rc != SGL_OK) return rc;
    std::copy(Chost.begin(), Chost.end(), centroids_out);
    std::copy(assign.begin(), assign.end(), assign_out);
    return SGL_OK;
}

extern "C" int sgl_op_ivf_search(sgl_ctx* c, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims,
                                 int32_t n_dims, int32_t n_neighbors, int32_t metric, const double* centroids, int32_t n_lists,
                                 const int32_t* assign, int32_t n_probe, int64_t query_batch, int32_t* idx_out, double* dist_out) {
    const char* who = "sgl_op_ivf_search";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    SGLCHK(ivf_state(c, who, R, k, n_ref));
    SGLCHK(sgl_knn_args(who, k, n_ref, n_query, dims, n_dims, n_neighbors));
    SGLCHK(ivf_args(who, n_ref, n_lists, n_probe, 0, metric));
    if (!centroids || !assign) { sgl_set_error("%s: centroids or assign is NULL", who); return SGL_EINVAL; }
    if (query_batch < 0) { sgl_set_error("%s: query_batch = %lld is negative", who, (long long)query_batch); return SGL_EINVAL; }
    const int nd = dims ? n_dims : k;
    for (int64_t e = 0; e < (int64_t)nd * n_lists; ++e)
        if (!std::isfinite(centroids[e])) {
            sgl_set_error("%s: centroids holds a non-finite value in column %lld, row %lld (0-based)", who, (long long)(e / nd), (long long)(e % nd));
            return SGL_EINVAL;
        }
    const int64_t bad = knn_ivf_first_bad_assign(assign, n_ref, n_lists);
    if (bad >= 0) {
        sgl_set_error("%s: assign[%lld] = %d is outside [0, n_lists = %d)", who, (long long)bad, assign[bad], n_lists);
        return SGL_EINVAL;
    }
    IvfBuffers B;
    StageClock clk(c);
    ivf_clock_reset(c);
    int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long no_direction = 0;
    clk.begin();
    int rc = ivf_operands(c, who, B, R, k, n_ref, true, Q, n_query, dims, n_dims, metric, &no_direction);
    clk.end(ST_OPERANDS);
    if (rc == SGL_OK) rc = B.C.alloc((size_t)nd * (size_t)n_lists);
    if (rc == SGL_OK && hipMemcpyAsync(B.C.p, centroids, sizeof(double) * (size_t)nd * (size_t)n_lists, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        sgl_set_error("%s: the copy of the centroids to the device failed", who);
        rc = SGL_EHIP;
    }
    if (rc == SGL_OK) rc = ivf_search(c, B, clk, n_ref, n_neighbors, metric, n_lists, assign, n_probe, query_batch, idx_out, dist_out, info);
    rc = ivf_drain(c, rc, who);
    if (rc == SGL_OK)
        for (int q = 0; q < 8; ++q) c->knn_ivf_last[q] = info[q];
    return rc;
}

// ---- the neighbour index kept on the device (include/singlet_hip.h, "Neighbour index and transfer") ----------------------
// What ivf_search has after its bucketing stage, kept instead of dropped -- or, for the exact method, the packed references of
// sgl_knn_metric -- with the annotations sgl_knn_index_annotate puts onto it.  One per context (sgl_ctx::knn_index).
struct KnnIndex {
    int32_t method = 0, metric = 0, k = 0, nd = 0, n_lists = 0;
    int64_t n_ref = 0;
    DevBuf<double> Rx;        // the packed references: in list order (method 1), in stored order (method 0)
    DevBuf<double> C;         // method 1: the centroids, the table from position to cell, the list offsets
    DevBuf<int32_t> cell;
    DevBuf<int64_t> off;
    DevBuf<int32_t> dims;     // the build's dims (p == nullptr: all k rows)
    int64_t train_cells = 0, shortest = 0, longest = 0, empty = 0;
    DevBuf<int32_t> labels;   // int32[n_ref] in [-1, n_classes)
    DevBuf<double> V;         // n_values x n_ref
    int32_t n_classes = 0, n_values = 0;
    DevBuf<double> Y;         // the layout of the reference cells, ydim x n_ref (sgl_knn_index_set_layout)
    int32_t ydim = 0;
    int64_t searches = 0, last_queries = 0, last_short = 0, instance = 0;

    int64_t bytes() const {
        int64_t b = 8 * (int64_t)nd * n_ref;
        if (method == 1) b += 8 * (int64_t)nd * n_lists + 4 * n_ref + 8 * ((int64_t)n_lists + 1);
        if (dims.p) b += 4 * (int64_t)nd;
        if (labels.p) b += 4 * n_ref;
        if (V.p) b += 8 * (int64_t)n_values * n_ref;
        if (Y.p) b += 8 * (int64_t)ydim * n_ref;
        return b;
    }
};

void sgl_knn_index_free(sgl_ctx* c) {
    delete c->knn_index;
    c->knn_index = nullptr;
}

namespace {

template <typename T>
void take(DevBuf<T>& to, DevBuf<T>& from) { std::swap(to.p, from.p); }

int index_method_arg(const char* who, int32_t method) {
    if (method == 0 || method == 1) return SGL_OK;
    sgl_set_error("%s: method = %d is outside [0, 1]", who, method);
    return SGL_EINVAL;
}

KnnIndex* index_of(sgl_ctx* c, const char* who) {
    if (!c->knn_index) sgl_set_error("%s: the context holds no neighbour index (call sgl_knn_index_build)", who);
    return c->knn_index;
}

// The refusals of a search against the index ix, before anything is uploaded.
int index_search_args(const char* who, const KnnIndex* ix, const double* Q, int64_t n_query, int32_t K, int32_t n_probe, int64_t query_batch) {
    if (!Q) { sgl_set_error("%s: Q is NULL (a search of the references among themselves is sgl_knn's, sgl_knn_ivf's)", who); return SGL_EINVAL; }
    if (n_query < 0) { sgl_set_error("%s: n_query = %lld is negative", who, (long long)n_query); return SGL_EINVAL; }
    if (K < 1 || K > KNN_MAX_NEIGHBORS || (int64_t)K > ix->n_ref) {
        sgl_set_error("%s: n_neighbors = %d is outside [1, min(%d, n_ref = %lld)]", who, K, KNN_MAX_NEIGHBORS, (long long)ix->n_ref);
        return SGL_EINVAL;
    }
    if (ix->method == 1 && (n_probe < 1 || n_probe > knn_ivf_max_probes(ix->n_lists))) {
        sgl_set_error("%s: n_probe = %d is outside [1, min(n_lists = %d, %d)]", who, n_probe, ix->n_lists, KNN_IVF_MAX_PROBES);
        return SGL_EINVAL;
    }
    if (ix->method == 1 && query_batch < 0) { sgl_set_error("%s: query_batch = %lld is negative", who, (long long)query_batch); return SGL_EINVAL; }
    return SGL_OK;
}

// One search of the k x nq host columns Q against the index: the upload, the finiteness pass on the raw Q, the packed queries
// under the build's dims and metric, and the scan of the index's method.  exact_batch: queries per pass of method 0 (0: all).
int index_query(sgl_ctx* c, const char* who, KnnIndex* ix, IvfBuffers& B, const double* Q, int64_t nq, int32_t K, int32_t n_probe,
                int64_t query_batch, int64_t exact_batch, int32_t* idx_out, double* dist_out, const IvfAfterBatch& after, int64_t* short_out) {
    const int nd = ix->nd;
    const int32_t k = ix->k;
    StageClock clk(c, false);
    SGLCHK(B.Q.alloc((size_t)k * (size_t)nq));
    HIPCHK(hipMemcpyAsync(B.Q.p, Q, sizeof(double) * (size_t)k * (size_t)nq, hipMemcpyHostToDevice, c->stream));
    SGLCHK(B.first.alloc(1));
    SGLCHK(sgl_knn_check_finite(c, who, "Q", B.Q.p, k, nq, B.first.p));
    SGLCHK(B.no_direction.alloc(1));
    HIPCHK(hipMemsetAsync(B.no_direction.p, 0, sizeof(unsigned long long), c->stream));
    SGLCHK(B.Qp.alloc((size_t)nd * (size_t)nq));
    {
        Phase ph(c, SGL_PH_GRAM);   // as sgl_knn_metric books knn_unit
        SGLCHK(sgl_knn_operand(c, B.Q.p, k, nq, ix->dims.p, nd, ix->metric, B.Qp.p, nullptr, B.no_direction.p));
    }
    B.nd = nd;
    B.nq = nq;
    B.Qs = B.Qp.p;
    *short_out = 0;
    if (ix->method == 1) {
        int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const IvfResident S = {ix->Rx.p, ix->C.p, ix->off.p, ix->cell.p, ix->n_lists};
        SGLCHK(ivf_query(c, B, clk, S, K, ix->metric, n_probe, query_batch, idx_out, dist_out, info, after));
        *short_out = info[6];
        return SGL_OK;
    }
    // the exact scan of sgl_knn_metric over the kept references; the merge makes the result independent of the cut
    const int64_t batch = exact_batch > 0 && exact_batch < nq ? exact_batch : nq;
    const bool dot = ix->metric != KNN_METRIC_EUCLIDEAN;
    for (int64_t q0 = 0; q0 < nq; q0 += batch) {
        const int64_t nb = std::min(batch, nq - q0);
        const KnnPlan P = knn_plan(nb, ix->n_ref, nd, K);
        const double* Xb = B.Qs + q0 * nd;
        if (P.instance == KNN_GENERIC_INSTANCE) {
            SGLCHK(B.Xt.need((size_t)nd * (size_t)nb));
            SGLCHK(sgl_knn_operand(c, Xb, nd, nb, nullptr, nd, KNN_METRIC_EUCLIDEAN, nullptr, B.Xt.p(), nullptr));
            Xb = B.Xt.p();
        }
        const size_t slots = (size_t)P.segments * (size_t)K * (size_t)nb;
        SGLCHK(B.cs.need(slots));
        SGLCHK(B.ci.need(slots));
        SGLCHK(B.idx.need((size_t)K * (size_t)nb));
        SGLCHK(B.dist.need((size_t)K * (size_t)nb));
        {
            Phase ph(c, SGL_PH_SCALE);
            SGLCHK(sgl_knn_scan(c->stream, P, dot, ix->Rx.p, Xb, nd, nb, ix->n_ref, K, B.cs.p(), B.ci.p(), B.idx.p(), B.dist.p()));
        }
        if (idx_out) HIPCHK(hipMemcpyAsync(idx_out + q0 * K, B.idx.p(), sizeof(int32_t) * (size_t)K * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        if (dist_out) HIPCHK(hipMemcpyAsync(dist_out + q0 * K, B.dist.p(), sizeof(double) * (size_t)K * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
        if (after) SGLCHK(after(q0, nb, B.idx.p(), B.dist.p()));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return SGL_OK;
}

void index_served(KnnIndex* ix, int64_t nq, int64_t short_queries) {
    ++ix->searches;
    ix->last_queries = nq;
    ix->last_short = short_queries;
}

}  // namespace

extern "C" int sgl_knn_index_build(sgl_ctx* c, const double* R, int32_t k, int64_t n_ref, const int32_t* dims, int32_t n_dims, int32_t metric,
                                   int32_t method, int32_t n_lists, int32_t n_iter) {
    const char* who = "sgl_knn_index_build";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    SGLCHK(ivf_state(c, who, R, k, n_ref));
    SGLCHK(sgl_knn_args(who, k, n_ref, 0, dims, n_dims, 1));
    SGLCHK(index_method_arg(who, method));
    if (method == 1) SGLCHK(ivf_args(who, n_ref, n_lists, 1, n_iter, metric));
    else SGLCHK(sgl_knn_metric_arg(who, metric));
    IvfBuffers B;
    StageClock clk(c, false);
    std::vector<double> Chost;
    std::vector<int32_t> assign;
    int64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long no_direction = 0;
    int rc = ivf_operands(c, who, B, R, k, n_ref, false, nullptr, 0, dims, n_dims, metric, &no_direction);
    if (rc == SGL_OK && method == 1) rc = ivf_train(c, B, clk, n_ref, n_lists, n_iter, Chost, assign, &info[2]);
    if (rc == SGL_OK && method == 1) rc = ivf_bucket(c, B, clk, n_ref, n_lists, assign.data(), info);
    rc = ivf_drain(c, rc, who);
    if (rc != SGL_OK) return rc;
    KnnIndex* ix = new KnnIndex;
    ix->method = method;
    ix->metric = metric;
    ix->k = k;
    ix->nd = B.nd;
    ix->n_ref = n_ref;
    ix->instance = knn_instance(B.nd);
    take(ix->dims, B.dims);
    if (method == 1) {
        ix->n_lists = n_lists;
        ix->train_cells = info[2];
        ix->shortest = info[3];
        ix->longest = info[4];
        ix->empty = info[5];
        take(ix->Rx, B.Rl);
        take(ix->C, B.C);
        take(ix->cell, B.cell);
        take(ix->off, B.off);
    } else {
        take(ix->Rx, B.Rp);
    }
    sgl_knn_index_free(c);   // a second build replaces the first
    c->knn_index = ix;
    return SGL_OK;            // B releases everything else: the raw upload, and for method 1 Rp and the training buffers
}

extern "C" int sgl_knn_index_search(sgl_ctx* c, const double* Q, int64_t n_query, int32_t n_neighbors, int32_t n_probe, int64_t query_batch,
                                    int32_t* idx_out, double* dist_out) {
    const char* who = "sgl_knn_index_search";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    KnnIndex* ix = index_of(c, who);
    if (!ix) return SGL_ESTATE;
    SGLCHK(index_search_args(who, ix, Q, n_query, n_neighbors, n_probe, query_batch));
    int64_t short_queries = 0;
    if (n_query > 0) {
        IvfBuffers B;
        const int rc = ivf_drain(c, index_query(c, who, ix, B, Q, n_query, n_neighbors, n_probe, query_batch, 0, idx_out, dist_out, IvfAfterBatch(),
                                                &short_queries), who);
        if (rc != SGL_OK) return rc;
    }
    index_served(ix, n_query, short_queries);
    return SGL_OK;
}

extern "C" int sgl_knn_index_drop(sgl_ctx* c) {
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    sgl_knn_index_free(c);
    return SGL_OK;
}

extern "C" int sgl_knn_index_info(sgl_ctx* c, int64_t out[16]) {
    if (c == nullptr || out == nullptr) { sgl_set_error("sgl_knn_index_info: NULL context or output"); return SGL_EINVAL; }
    for (int q = 0; q < 16; ++q) out[q] = 0;
    const KnnIndex* ix = c->knn_index;
    if (!ix) return SGL_OK;
    const int64_t v[16] = {1, ix->method, ix->metric, ix->k, ix->nd, ix->n_ref, ix->n_lists, ix->train_cells, ix->shortest, ix->longest,
                           ix->empty, ix->bytes(), ix->searches, ix->last_queries, ix->last_short, ix->instance};
    for (int q = 0; q < 16; ++q) out[q] = v[q];
    return SGL_OK;
}

extern "C" int sgl_knn_index_annotate(sgl_ctx* c, const int32_t* labels, int32_t n_classes, const double* V, int32_t n_values) {
    const char* who = "sgl_knn_index_annotate";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    KnnIndex* ix = index_of(c, who);
    if (!ix) return SGL_ESTATE;
    SGLCHK(sgl_knn_transfer_args(who, 0, 1, 0, ix->n_ref, labels != nullptr, n_classes, V != nullptr, n_values));
    if (labels) SGLCHK(sgl_knn_transfer_labels_check(who, labels, ix->n_ref, n_classes));
    DevBuf<int32_t> lab;
    DevBuf<double> val;
    DevBuf<unsigned long long> first;
    int rc = SGL_OK;
    auto stage = [&]() -> int {
        if (V) {
            SGLCHK(val.alloc((size_t)n_values * (size_t)ix->n_ref));
            SGLCHK(first.alloc(1));
            HIPCHK(hipMemcpyAsync(val.p, V, sizeof(double) * (size_t)n_values * (size_t)ix->n_ref, hipMemcpyHostToDevice, c->stream));
            SGLCHK(sgl_knn_check_finite(c, who, "V", val.p, n_values, ix->n_ref, first.p));
        }
        if (labels) {
            SGLCHK(lab.alloc((size_t)ix->n_ref));
            HIPCHK(hipMemcpyAsync(lab.p, labels, sizeof(int32_t) * (size_t)ix->n_ref, hipMemcpyHostToDevice, c->stream));
        }
        return SGL_OK;
    };
    rc = ivf_drain(c, stage(), who);
    if (rc != SGL_OK) return rc;   // the index keeps what it had
    if (labels) { take(ix->labels, lab); ix->n_classes = n_classes; }
    if (V) { take(ix->V, val); ix->n_values = n_values; }
    return SGL_OK;   // lab / val release what they replaced
}

extern "C" int sgl_knn_index_map(sgl_ctx* c, const double* Q, int64_t n_query, int32_t n_neighbors, int32_t n_probe, int32_t weighting,
                                 int32_t* idx_out, double* dist_out, int32_t* pred_out, double* best_out, double* scores_out,
                                 double* values_out) {
    const char* who = "sgl_knn_index_map";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    KnnIndex* ix = index_of(c, who);
    if (!ix) return SGL_ESTATE;
    if (weighting < 0 || weighting > KNN_TRANSFER_WEIGHTING_MAX) {
        sgl_set_error("%s: weighting = %d is outside [0, %d]", who, weighting, KNN_TRANSFER_WEIGHTING_MAX);
        return SGL_EINVAL;
    }
    SGLCHK(index_search_args(who, ix, Q, n_query, n_neighbors, n_probe, 0));
    const bool want_labels = pred_out || best_out || scores_out;
    if (want_labels && !ix->labels.p) {
        sgl_set_error("%s: pred_out, best_out or scores_out is asked for, but the index holds no labels (call sgl_knn_index_annotate)", who);
        return SGL_ESTATE;
    }
    if (values_out && !ix->V.p) {
        sgl_set_error("%s: values_out is asked for, but the index holds no values (call sgl_knn_index_annotate)", who);
        return SGL_ESTATE;
    }
    int64_t short_queries = 0;
    if (n_query > 0) {
        const int32_t n_classes = ix->n_classes, n_values = ix->n_values;
        const int64_t per_query = knn_transfer_query_bytes(ix->method == 1 ? n_probe : KNN_MAX_SEGMENTS, n_neighbors, scores_out ? n_classes : 0,
                                                           values_out ? n_values : 0);
        const int64_t batch = knn_transfer_batch(n_query, per_query, KNN_TRANSFER_SCRATCH_BYTES);
        IvfBuffers B;
        DevBuf<int32_t> pred;
        DevBuf<double> best, scores, values;
        auto body = [&]() -> int {
            if (pred_out) SGLCHK(pred.alloc((size_t)batch));
            if (best_out) SGLCHK(best.alloc((size_t)batch));
            if (scores_out) SGLCHK(scores.alloc((size_t)n_classes * (size_t)batch));
            if (values_out) SGLCHK(values.alloc((size_t)n_values * (size_t)batch));
            // the transfer of a batch on the device: the neighbour lists do not travel to the host and back
            const IvfAfterBatch after = [&](int64_t q0, int64_t nb, const int32_t* idx_dev, const double* dist_dev) -> int {
                if (!want_labels && !values_out) return SGL_OK;
                SGLCHK(sgl_knn_transfer_dev(c, idx_dev, dist_dev, n_neighbors, nb, want_labels ? ix->labels.p : nullptr, n_classes,
                                            values_out ? ix->V.p : nullptr, n_values, weighting, pred.p, best.p, scores.p, values.p));
                if (pred_out) HIPCHK(hipMemcpyAsync(pred_out + q0, pred.p, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
                if (best_out) HIPCHK(hipMemcpyAsync(best_out + q0, best.p, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
                if (scores_out)
                    HIPCHK(hipMemcpyAsync(scores_out + q0 * n_classes, scores.p, sizeof(double) * (size_t)n_classes * (size_t)nb,
                                          hipMemcpyDeviceToHost, c->stream));
                if (values_out)
                    HIPCHK(hipMemcpyAsync(values_out + q0 * n_values, values.p, sizeof(double) * (size_t)n_values * (size_t)nb,
                                          hipMemcpyDeviceToHost, c->stream));
                return SGL_OK;
            };
            return index_query(c, who, ix, B, Q, n_query, n_neighbors, n_probe, batch, batch, idx_out, dist_out, after, &short_queries);
        };
        const int rc = ivf_drain(c, body(), who);
        if (rc != SGL_OK) return rc;
    }
    index_served(ix, n_query, short_queries);
    return SGL_OK;
}

// ---- the layout on the index, and query cells placed in it (include/singlet_hip.h, "Layout transform") -------------------
extern "C" int sgl_knn_index_set_layout(sgl_ctx* c, const double* Yref, int32_t dim) {
    const char* who = "sgl_knn_index_set_layout";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    KnnIndex* ix = index_of(c, who);
    if (!ix) return SGL_ESTATE;
    if (!Yref) { sgl_set_error("%s: Yref is NULL", who); return SGL_EINVAL; }
    if (dim < 1 || dim > 8) { sgl_set_error("%s: dim = %d is outside [1, 8]", who, dim); return SGL_EINVAL; }
    DevBuf<double> val;
    DevBuf<unsigned long long> first;
    auto stage = [&]() -> int {
        SGLCHK(val.alloc((size_t)dim * (size_t)ix->n_ref));
        SGLCHK(first.alloc(1));
        HIPCHK(hipMemcpyAsync(val.p, Yref, sizeof(double) * (size_t)dim * (size_t)ix->n_ref, hipMemcpyHostToDevice, c->stream));
        SGLCHK(sgl_knn_check_finite(c, who, "Yref", val.p, dim, ix->n_ref, first.p));
        return SGL_OK;
    };
    const int rc = ivf_drain(c, stage(), who);
    if (rc != SGL_OK) return rc;   // the index keeps what it had
    take(ix->Y, val);
    ix->ydim = dim;
    return SGL_OK;                 // val releases what it replaced
}

extern "C" int sgl_knn_index_project(sgl_ctx* c, const double* Q, int64_t n_query, int32_t n_neighbors, int32_t n_probe, int64_t query_batch,
                                     double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, int32_t* idx_out,
                                     double* dist_out, double* Y0_out, double* Y_out) {
    const char* who = "sgl_knn_index_project";
    if (c == nullptr) { sgl_set_error("null context"); return SGL_EINVAL; }
    HIPCHK(hipSetDevice(c->device));
    KnnIndex* ix = index_of(c, who);
    if (!ix) return SGL_ESTATE;
    if (!ix->Y.p) {
        sgl_set_error("%s: the index holds no layout (call sgl_knn_index_set_layout)", who);
        return SGL_ESTATE;
    }
    SGLCHK(index_search_args(who, ix, Q, n_query, n_neighbors, n_probe, query_batch));
    if (query_batch < 0) { sgl_set_error("%s: query_batch = %lld is negative", who, (long long)query_batch); return SGL_EINVAL; }
    const int32_t dim = ix->ydim;
    SGLCHK(sgl_umap_transform_args(who, n_query, n_neighbors, ix->n_ref, dim, a, b, n_epochs, alpha0, neg_rate));
    int64_t short_queries = 0, launches = 0;
    unsigned long long hstats[2] = {0, 0};
    if (n_query > 0) {
        // the batch: the caller's, or as many queries as the map's budget keeps (the lists, the memberships, two positions)
        const int64_t per_query = knn_transfer_query_bytes(ix->method == 1 ? n_probe : KNN_MAX_SEGMENTS, n_neighbors, n_neighbors, 2 * dim);
        const int64_t batch = query_batch > 0 ? std::min(query_batch, n_query) : knn_transfer_batch(n_query, per_query, KNN_TRANSFER_SCRATCH_BYTES);
        IvfBuffers B;
        DevBuf<double> W, Y0, Y;
        DevBuf<unsigned long long> stats;
        int64_t cap = 0;
        auto body = [&]() -> int {
            SGLCHK(stats.alloc(2));
            HIPCHK(hipMemsetAsync(stats.p, 0, 2 * sizeof(unsigned long long), c->stream));
            // memberships, start and transform of a batch on the device: the neighbour lists do not travel to the host and back
            const IvfAfterBatch after = [&](int64_t q0, int64_t nb, const int32_t* idx_dev, const double* dist_dev) -> int {
                if (nb > cap) {
                    SGLCHK(W.alloc((size_t)n_neighbors * (size_t)nb));
                    SGLCHK(Y0.alloc((size_t)dim * (size_t)nb));
                    SGLCHK(Y.alloc((size_t)dim * (size_t)nb));
                    cap = nb;
                }
                int64_t issued = 0;
                SGLCHK(sgl_umap_transform_dev(c->stream, idx_dev, dist_dev, n_neighbors, nb, ix->Y.p, dim, ix->n_ref, a, b, n_epochs, alpha0,
                                              neg_rate, seed, q0, W.p, Y0_out ? Y0.p : nullptr, Y.p, stats.p, &issued));
                launches += issued;
                if (Y0_out) HIPCHK(hipMemcpyAsync(Y0_out + q0 * dim, Y0.p, sizeof(double) * (size_t)dim * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
                if (Y_out) HIPCHK(hipMemcpyAsync(Y_out + q0 * dim, Y.p, sizeof(double) * (size_t)dim * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(hipStreamSynchronize(c->stream));   // the scratch is free for the next batch, a fault surfaces here
                return SGL_OK;
            };
            SGLCHK(index_query(c, who, ix, B, Q, n_query, n_neighbors, n_probe, batch, batch, idx_out, dist_out, after, &short_queries));
            HIPCHK(hipMemcpyAsync(hstats, stats.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            return SGL_OK;
        };
        const int rc = ivf_drain(c, body(), who);
        if (rc != SGL_OK) return rc;
    }
    sgl_umap_transform_note(dim, b, (int64_t)hstats[0], (int64_t)hstats[1], launches);
    index_served(ix, n_query, short_queries);
    return SGL_OK;
}
