// Layout transform on the GPU: sgl_c_fuzzy_query (the memberships of a query's neighbour list against the reference),
// sgl_c_umap_transform and sgl_op_umap_transform_epochs (query cells placed in the FIXED layout of the reference),
// sgl_umap_transform_info, and the device stage sgl_umap_transform_dev that sgl_knn_index_project runs per batch
// (include/singlet_hip.h, "Layout transform"; the rules restated in tests/umap_transform_restatement.py).  The reference
// positions are read-only, negative samples are reference points, only the query moves: a query's trajectory depends on that
// query and the reference alone.  So one wave runs ALL epochs of a launch for its query with the position in registers, and
// the result is one function of (query, reference) whatever the batching.  Every sum has one stated order, no floating-point
// atomic anywhere, no contraction.
//
// Memberships: one thread per query (the serial order of psum forbids a wave reduction).
// Transform: one wave per query.  The wave stages its slots (reference index, membership) in LDS once.  Per epoch it takes
// the slots in steps of 64; a ballot compacts the firing slots, and the (firing slot, term) pairs -- the attractive term and
// the negative samples -- are spread over the lanes; the clipped terms go through LDS to lane f < dim, which adds component
// f in the stated order and carries the sums from step to step; y' is published to the wave by a shuffle, so every lane
// holds the current y.  y is written to memory once, at the end of the launch.
#include "sgl_internal.h"
#include "umap_transform_host.h"
#include "umap_transform_dev.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

int64_t g_tinfo[4] = {-1, 0, 0, 0};   // sgl_umap_transform_info

unsigned grid_for(int64_t n, int per_block) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, 1 << 20)); }

int hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return SGL_OK;
    (void)hipGetLastError();
    sgl_set_error("%s failed: %s", what, hipGetErrorString(e));
    return SGL_EHIP;
}
#define UTCHK(expr, what) SGLCHK(hip_ok((expr), what))
#define UTLAUNCHED(name) UTCHK(hipGetLastError(), name)

template <typename T>
int upload(hipStream_t s, DevBuf<T>& d, const T* h, size_t n, const char* what) {
    SGLCHK(d.alloc(std::max<size_t>(n, 1)));
    if (n > 0) UTCHK(hipMemcpyAsync(d.p, h, sizeof(T) * n, hipMemcpyHostToDevice, s), what);
    return SGL_OK;
}
template <typename T>
int fetch(hipStream_t s, T* h, const T* d, size_t n, const char* what) {   // synchronous
    if (n > 0) UTCHK(hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, s), what);
    UTCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    return SGL_OK;
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// ----------------------------------------------------------------------------------------------------------- memberships ---
// One thread per query: rho, sigma and the memberships of its K slots (+0.0 in the padding).  stats (may be null): [0] the
// widest list, [1] the queries without a valid slot -- integer atomics.
__global__ __launch_bounds__(256) void fq_query_kernel(const int32_t* __restrict__ idx, const double* __restrict__ dist, int64_t nq, int K,
                                                       double target, double* __restrict__ W, double* __restrict__ rho_out,
                                                       double* __restrict__ sigma_out, unsigned long long* __restrict__ stats) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nq; j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t* li = idx + j * K;
        const double* ld = dist + j * K;
        double rho = 0.0, sum = 0.0;
        int own = 0;
        while (own < K && li[own] >= 0) {
            const double d = ld[own];
            sum = sum + d;
            if (rho == 0.0 && d > 0.0) rho = d;   // the lists ascend: the first distance above 0 is the smallest
            ++own;
        }
        if (stats) {
            atomicMax(&stats[0], (unsigned long long)own);
            if (own == 0) atomicAdd(&stats[1], 1ull);
        }
        double sigma = 0.0;
        if (own > 0) {
            const double mean = sum / (double)own;
            double lo = 0.0, hi = INFINITY, mid = 1.0;
            for (int step = 0; step < 64; ++step) {
                double ps = 0.0;
                for (int q = 0; q < own; ++q) {
                    const double t = ld[q] - rho;
                    ps = ps + (t > 0.0 ? exp(-t / mid) : 1.0);
                }
                if (ps > target) {
                    hi = mid;
                    mid = (lo + hi) / 2.0;
                } else {
                    lo = mid;
                    mid = hi == INFINITY ? 2.0 * mid : (lo + hi) / 2.0;
                }
            }
            sigma = fmax(mid, 1e-3 * mean);
        }
        if (rho_out) rho_out[j] = rho;
        if (sigma_out) sigma_out[j] = sigma;
        if (W)
            for (int q = 0; q < K; ++q) {
                double m = 0.0;
                if (q < own) {
                    const double t = ld[q] - rho;
                    m = t > 0.0 ? exp(-t / sigma) : 1.0;
                }
                W[j * K + q] = m;
            }
    }
}

// ------------------------------------------------------------------------------------------------------------- transform ---
struct UtArgs {
    const int32_t* idx;   // K x nq
    const double* W;      // K x nq
    const double* Yref;   // dim x n_ref (read-only)
    const double* Yin;    // dim x nq, or null: the launch begins at the start y0
    double* Y0;           // dim x nq, or null: where the start is written
    double* Y;            // dim x nq: each y written once, at the end of the launch (may alias Yin: a wave reads its own column only)
    int64_t nq, n_ref, query_offset;
    int32_t K, dim;
    int32_t terms;        // 1 + neg_rate
    int32_t n_epochs;
    int64_t t_first, t_last;
    double a, b, m2ab, tb, alpha0;
    uint64_t seed;
};

// One wave per query.  DIM = 2 or 3: compile-time; DIM = 0: the generic loop up to UMAP_MAX_DIM.  B1: b == 1.0, p = d2.
template <int DIM, bool B1>
__global__ __launch_bounds__(64) void ut_epochs_kernel(UtArgs A) {
    constexpr int D = DIM ? DIM : UMAP_MAX_DIM;
    __shared__ int32_t s_idx[UMAP_MAX_NEIGHBORS];
    __shared__ double s_w[UMAP_MAX_NEIGHBORS];
    __shared__ int32_t s_q[64];
    __shared__ double s_term[64 * D];
    const int dim = DIM ? DIM : A.dim;
    const int lane = threadIdx.x;
    const int T = A.terms;
    const int K = A.K;
    for (int64_t j = blockIdx.x; j < A.nq; j += gridDim.x) {
        __syncthreads();   // the previous query's slots are no longer read
        int mine = 0;      // the valid slots among this lane's
        for (int s = lane; s < K; s += 64) {
            const int32_t r = A.idx[j * K + s];
            s_idx[s] = r;
            s_w[s] = A.W[j * K + s];
            if (r >= 0) ++mine;
        }
        int nv = mine;     // the valid slots lead the list: their number is the sum over the lanes
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o);
        __syncthreads();
        if (nv == 0) {     // no valid slot: a quiet NaN, as the transfer's values
            if (lane < dim) {
                if (A.Y0) A.Y0[j * dim + lane] = quiet_nan();
                A.Y[j * dim + lane] = quiet_nan();
            }
            continue;
        }
        double ymine = 0.0;   // component `lane` of y (lanes below dim)
        if (A.Yin) {
            if (lane < dim) ymine = A.Yin[j * dim + lane];
        } else {
            if (lane < dim) {
                double num = 0.0, den = 0.0;
                for (int s = 0; s < nv; ++s) {
                    const double w = s_w[s];
                    num = num + w * A.Yref[(int64_t)s_idx[s] * dim + lane];
                    den = den + w;
                }
                ymine = num / den;
                if (A.Y0) A.Y0[j * dim + lane] = ymine;
            }
        }
        double yj[D];
#pragma unroll
        for (int f = 0; f < D; ++f) yj[f] = f < dim ? __shfl(ymine, f) : 0.0;
        const uint64_t ctr0 = 256ull * ((uint64_t)A.query_offset + (uint64_t)j);
        for (int64_t t = A.t_first; t <= A.t_last; ++t) {
            const double t1 = (double)t, t0 = (double)(t - 1);
            double g = 0.0, delta = 0.0;   // of component `lane` (lanes below dim)
            bool open = false;             // a slot's partial sum g is under way (uniform over the wave)
            for (int c0 = 0; c0 < nv; c0 += UMAP_CHUNK) {
                const int e = c0 + lane;
                bool fire = false;
                if (e < nv) {
                    const double r = s_w[e];
                    fire = floor(t1 * r) > floor(t0 * r);
                }
                const unsigned long long mask = __ballot(fire);
                const int nf = __popcll(mask);
                if (nf == 0) continue;
                if (fire) s_q[__popcll(mask & ((1ull << lane) - 1ull))] = e;
                __syncthreads();
                const int items = nf * T;
                for (int I0 = 0; I0 < items; I0 += 64) {
                    const int I = I0 + lane;
                    if (I < items) {
                        const int q = I / T, sidx = I - q * T;
                        const int s = s_q[q];
                        int64_t o;
                        if (sidx == 0) {
                            o = s_idx[s];
                        } else {
                            const uint64_t u = sgl_rand2(A.seed, ctr0 + (uint64_t)s, 256ull * (uint64_t)t + (uint64_t)(sidx - 1));
                            o = (int64_t)(((u >> 32) * (uint64_t)A.n_ref) >> 32);
                        }
                        double df[D], d2 = 0.0;
#pragma unroll
                        for (int f = 0; f < D; ++f) {
                            if (f < dim) {
                                df[f] = yj[f] - A.Yref[o * dim + f];
                                d2 = d2 + df[f] * df[f];
                            } else {
                                df[f] = 0.0;
                            }
                        }
                        double c = 0.0;
                        bool plain = false, four = false;   // plain: the term is +0.0; four: every component is +4.0
                        if (sidx == 0) {
                            if (d2 > 0.0) {
                                const double pw = B1 ? d2 : pow(d2, A.b);
                                c = (A.m2ab * (pw / d2)) / (A.a * pw + 1.0);
                            } else {
                                plain = true;
                            }
                        } else if (d2 == 0.0) {
                            four = true;
                        } else {
                            const double pw = B1 ? d2 : pow(d2, A.b);
                            c = A.tb / ((0.001 + d2) * (A.a * pw + 1.0));
                        }
#pragma unroll
                        for (int f = 0; f < D; ++f)
                            if (f < dim) s_term[lane * D + f] = plain ? 0.0 : four ? 4.0 : fmin(fmax(c * df[f], -4.0), 4.0);
                    }
                    __syncthreads();
                    if (lane < dim) {
                        const int cnt = items - I0 < 64 ? items - I0 : 64;
                        int sidx = I0 % T;
                        for (int u = 0; u < cnt; ++u) {
                            const double v = s_term[u * D + lane];
                            if (sidx == 0) {
                                if (open) delta = delta + g;
                                g = v;
                                open = true;
                            } else {
                                g = g + v;
                            }
                            if (++sidx == T) sidx = 0;
                        }
                    }
                    open = true;   // nf > 0: the first item of the first round opened a sum
                    __syncthreads();
                }
            }
            if (open) {   // uniform; a query without a firing slot keeps the bits of y
                if (lane < dim) {
                    delta = delta + g;
                    const double alpha = A.alpha0 * (1.0 - t0 / (double)A.n_epochs);
                    const double step = alpha * delta;
                    ymine = ymine + step;
                }
#pragma unroll
                for (int f = 0; f < D; ++f)
                    if (f < dim) yj[f] = __shfl(ymine, f);
            }
        }
        if (lane < dim) A.Y[j * dim + lane] = ymine;
    }
}

int ut_launch(hipStream_t s, const UtArgs& A, int instance) {
    const dim3 grid(grid_for(A.nq, 1)), block(64);
    switch (instance) {
        case 0: ut_epochs_kernel<2, false><<<grid, block, 0, s>>>(A); break;
        case 1: ut_epochs_kernel<2, true><<<grid, block, 0, s>>>(A); break;
        case 2: ut_epochs_kernel<3, false><<<grid, block, 0, s>>>(A); break;
        case 3: ut_epochs_kernel<3, true><<<grid, block, 0, s>>>(A); break;
        case 4: ut_epochs_kernel<0, false><<<grid, block, 0, s>>>(A); break;
        default: ut_epochs_kernel<0, true><<<grid, block, 0, s>>>(A); break;
    }
    UTLAUNCHED("ut_epochs_kernel");
    return SGL_OK;
}

// The launches of the epochs t_first .. t_last on device arrays; Yin == nullptr: from the start (written to Y0 when asked).
int ut_run(hipStream_t s, const int32_t* idx, const double* W, int32_t K, int64_t nq, const double* Yref, int32_t dim, int64_t n_ref,
           const double* Yin, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, int64_t query_offset,
           int64_t t_first, int64_t t_last, double* Y0, double* Y, int64_t* launches) {
    UtArgs A;
    A.idx = idx;
    A.W = W;
    A.Yref = Yref;
    A.Yin = Yin;
    A.Y0 = Y0;
    A.Y = Y;
    A.nq = nq;
    A.n_ref = n_ref;
    A.query_offset = query_offset;
    A.K = K;
    A.dim = dim;
    A.terms = 1 + neg_rate;
    A.n_epochs = n_epochs;
    A.a = a;
    A.b = b;
    A.m2ab = -2.0 * a * b;
    A.tb = 2.0 * b;
    A.alpha0 = alpha0;
    A.seed = seed;
    const int instance = umap_instance(dim, b);
    int rc = SGL_OK;
    *launches = ut_run_launches(t_first, t_last, [&](int64_t first, int64_t last) -> int {
        A.t_first = first;
        A.t_last = last;
        const int r = ut_launch(s, A, instance);
        A.Yin = Y;       // the next launch goes on from this one's result, in place
        A.Y0 = nullptr;
        return r;
    }, &rc, ut_epochs_per_launch(getenv("SGL_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH")));
    return rc;
}

int refuse(const char* who, UtDefect f, int64_t query, int32_t slot) {
    if (f == UT_YREF_NOT_FINITE) sgl_set_error("%s: %s (Yref, at position %lld)", who, ut_defect_text(f), (long long)query);
    else if (f == UT_YIN_NOT_FINITE) sgl_set_error("%s: %s (Yin, query %lld, component %d)", who, ut_defect_text(f), (long long)query, slot);
    else if (query >= 0) sgl_set_error("%s: invalid neighbour list of query %lld at slot %d: %s", who, (long long)query, slot, ut_defect_text(f));
    else sgl_set_error("%s: %s", who, ut_defect_text(f));
    return SGL_EINVAL;
}

void note_plan(const UtPlan& P) {
    g_tinfo[0] = P.instance;
    g_tinfo[1] = P.widest;
    g_tinfo[2] = P.empty;
    g_tinfo[3] = P.launches;
}

}  // namespace

// The device stage of one batch (sgl_knn_index_project): idx / dist / W / Y0 / Y on the device, W a scratch of K x nq, Y0 may
// be null; stats as fq_query_kernel takes them (may be null).  The lists come from a search: they are not validated again.
int sgl_umap_transform_dev(hipStream_t s, const int32_t* idx, const double* dist, int32_t K, int64_t nq, const double* Yref, int32_t dim,
                           int64_t n_ref, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed,
                           int64_t query_offset, double* W, double* Y0, double* Y, unsigned long long* stats, int64_t* launches) {
    fq_query_kernel<<<dim3(grid_for(nq, 256)), dim3(256), 0, s>>>(idx, dist, nq, K, log2((double)K), W, nullptr, nullptr, stats);
    UTLAUNCHED("fq_query_kernel");
    return ut_run(s, idx, W, K, nq, Yref, dim, n_ref, nullptr, a, b, n_epochs, alpha0, neg_rate, seed, query_offset, 1, n_epochs, Y0, Y, launches);
}

void sgl_umap_transform_note(int32_t dim, double b, int64_t widest, int64_t empty, int64_t launches) {
    UtPlan P;
    P.instance = umap_instance(dim, b);
    P.widest = widest;
    P.empty = empty;
    P.launches = launches;
    note_plan(P);
}

// The refusals of the layout arguments alone (sgl_knn_index_project: its lists come from the search).
int sgl_umap_transform_args(const char* who, int64_t n_query, int32_t K, int64_t n_ref, int32_t dim, double a, double b, int32_t n_epochs,
                            double alpha0, int32_t neg_rate) {
    const UtDefect f = ut_check_scalars(n_query, K, n_ref, true, dim, a, b, n_epochs, 1, n_epochs, alpha0, neg_rate, 0);
    return f == UT_OK ? SGL_OK : refuse(who, f, -1, -1);
}

extern "C" int sgl_c_fuzzy_query(const int32_t* idx, const double* dist, int64_t n_query, int32_t K, int64_t n_ref, double* W_out,
                                 double* rho_out, double* sigma_out) {
    static const char* who = "c_fuzzy_query";
    UtDefect f = ut_check_scalars(n_query, K, n_ref, false, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    if (f != UT_OK) return refuse(who, f, -1, -1);
    if (n_query == 0) return SGL_OK;
    if (!idx || !dist) return refuse(who, UT_ARGS_NULL, -1, -1);
    int64_t query = -1;
    int32_t slot = -1;
    f = ut_check_lists(idx, dist, nullptr, n_query, K, n_ref, &query, &slot);
    if (f != UT_OK) return refuse(who, f, query, slot);
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    hipStream_t s = hd.c->stream;
    const size_t nk = (size_t)n_query * (size_t)K;
    DevBuf<int32_t> didx;
    DevBuf<double> ddist, W, rho, sigma;
    SGLCHK(upload(s, didx, idx, nk, "upload of the indices"));
    SGLCHK(upload(s, ddist, dist, nk, "upload of the distances"));
    SGLCHK(W.alloc(nk)); SGLCHK(rho.alloc((size_t)n_query)); SGLCHK(sigma.alloc((size_t)n_query));
    fq_query_kernel<<<dim3(grid_for(n_query, 256)), dim3(256), 0, s>>>(didx.p, ddist.p, n_query, K, log2((double)K), W.p, rho.p, sigma.p, nullptr);
    UTLAUNCHED("fq_query_kernel");
    if (W_out) SGLCHK(fetch(s, W_out, W.p, nk, "download of W"));
    if (rho_out) SGLCHK(fetch(s, rho_out, rho.p, (size_t)n_query, "download of rho"));
    if (sigma_out) SGLCHK(fetch(s, sigma_out, sigma.p, (size_t)n_query, "download of sigma"));
    UTCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    return SGL_OK;
}

extern "C" int sgl_c_umap_transform(const int32_t* idx, const double* dist, int64_t n_query, int32_t K, const double* Yref, int32_t dim,
                                    int64_t n_ref, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed,
                                    int64_t query_offset, double* Y0_out, double* Y_out) {
    static const char* who = "c_umap_transform";
    UtDefect f = ut_check_scalars(n_query, K, n_ref, true, dim, a, b, n_epochs, 1, n_epochs, alpha0, neg_rate, query_offset);
    if (f != UT_OK) return refuse(who, f, -1, -1);
    if (n_query == 0) return SGL_OK;
    if (!idx || !dist || !Yref) return refuse(who, UT_ARGS_NULL, -1, -1);
    int64_t query = -1, pos = -1;
    int32_t slot = -1;
    f = ut_check_lists(idx, dist, nullptr, n_query, K, n_ref, &query, &slot);
    if (f != UT_OK) return refuse(who, f, query, slot);
    if (!ut_all_finite(Yref, n_ref * dim, &pos)) return refuse(who, UT_YREF_NOT_FINITE, pos, -1);
    UtPlan plan = ut_plan(idx, n_query, K, dim, b, 1, n_epochs);
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    hipStream_t s = hd.c->stream;
    const size_t nk = (size_t)n_query * (size_t)K, nd = (size_t)n_query * (size_t)dim;
    DevBuf<int32_t> didx;
    DevBuf<double> ddist, dY, W, Y0, Y;
    SGLCHK(upload(s, didx, idx, nk, "upload of the indices"));
    SGLCHK(upload(s, ddist, dist, nk, "upload of the distances"));
    SGLCHK(upload(s, dY, Yref, (size_t)n_ref * (size_t)dim, "upload of Yref"));
    SGLCHK(W.alloc(nk)); SGLCHK(Y0.alloc(nd)); SGLCHK(Y.alloc(nd));
    int64_t launches = 0;
    SGLCHK(sgl_umap_transform_dev(s, didx.p, ddist.p, K, n_query, dY.p, dim, n_ref, a, b, n_epochs, alpha0, neg_rate, seed, query_offset, W.p,
                                  Y0_out ? Y0.p : nullptr, Y.p, nullptr, &launches));
    UTCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    plan.launches = launches;
    note_plan(plan);
    if (Y0_out) SGLCHK(fetch(s, Y0_out, Y0.p, nd, "download of Y0"));
    if (Y_out) SGLCHK(fetch(s, Y_out, Y.p, nd, "download of Y"));
    return SGL_OK;
}

extern "C" int sgl_op_umap_transform_epochs(const int32_t* idx, const double* W, int64_t n_query, int32_t K, const double* Yref, int32_t dim,
                                            int64_t n_ref, const double* Yin, double a, double b, int32_t n_epochs, double alpha0,
                                            int32_t neg_rate, uint64_t seed, int64_t query_offset, int32_t t_first, int32_t t_last,
                                            double* Y_out) {
    static const char* who = "op_umap_transform_epochs";
    UtDefect f = ut_check_scalars(n_query, K, n_ref, true, dim, a, b, n_epochs, t_first, t_last, alpha0, neg_rate, query_offset);
    if (f != UT_OK) return refuse(who, f, -1, -1);
    if (n_query == 0) return SGL_OK;
    if (!idx || !W || !Yref || !Yin || !Y_out) return refuse(who, UT_ARGS_NULL, -1, -1);
    int64_t query = -1, pos = -1;
    int32_t slot = -1;
    f = ut_check_lists(idx, nullptr, W, n_query, K, n_ref, &query, &slot);
    if (f != UT_OK) return refuse(who, f, query, slot);
    if (!ut_all_finite(Yref, n_ref * dim, &pos)) return refuse(who, UT_YREF_NOT_FINITE, pos, -1);
    if (!ut_yin_finite(Yin, idx, n_query, K, dim, &query, &slot)) return refuse(who, UT_YIN_NOT_FINITE, query, slot);
    UtPlan plan = ut_plan(idx, n_query, K, dim, b, t_first, t_last);
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    hipStream_t s = hd.c->stream;
    const size_t nk = (size_t)n_query * (size_t)K, nd = (size_t)n_query * (size_t)dim;
    DevBuf<int32_t> didx;
    DevBuf<double> dW, dY, Y;
    SGLCHK(upload(s, didx, idx, nk, "upload of the indices"));
    SGLCHK(upload(s, dW, W, nk, "upload of W"));
    SGLCHK(upload(s, dY, Yref, (size_t)n_ref * (size_t)dim, "upload of Yref"));
    SGLCHK(upload(s, Y, Yin, nd, "upload of Yin"));
    int64_t launches = 0;
    SGLCHK(ut_run(s, didx.p, dW.p, K, n_query, dY.p, dim, n_ref, Y.p, a, b, n_epochs, alpha0, neg_rate, seed, query_offset, t_first, t_last,
                  nullptr, Y.p, &launches));
    UTCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    plan.launches = launches;
    note_plan(plan);
    return fetch(s, Y_out, Y.p, nd, "download of Y");
}

extern "C" int sgl_umap_transform_info(int64_t out[4]) {
    if (!out) { sgl_set_error("sgl_umap_transform_info: out is NULL"); return SGL_EINVAL; }
    for (int q = 0; q < 4; ++q) out[q] = g_tinfo[q];
    return SGL_OK;
}
