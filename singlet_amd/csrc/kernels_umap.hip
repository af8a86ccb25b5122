// Cell layout on the GPU: sgl_c_fuzzy_graph (the fuzzy neighbour graph of the k-NN lists), sgl_c_umap_layout and
// sgl_op_umap_epoch (the synchronous, owner-computes form of UMAP's optimiser), sgl_umap_info (include/singlet_hip.h,
// "Layout"; the rules restated in tests/umap_restatement.py).  The reference package has no layout code (it hands the embedding
// to Seurat / uwot), so the rules are this library's own, and every result is ONE function of its inputs: every sum has one
// stated order, negative samples come from the counter hash sgl_rand2, positions of the epoch's start are read-only, no
// floating-point atomic anywhere, no contraction.
//
// Fuzzy graph: one thread per cell computes rho, sigma (64 bisection steps) and the memberships of its own list; the incoming
// lists come from a counting transpose (integer histogram, scan, cursor fill); one wave per vertex sorts the keys
// (row << 32 | direction << 31 | position) of its own and incoming entries -- in LDS up to UMAP_MERGE_WIDTH keys, through a
// segmented radix sort in HBM above (a hub's in-degree is unbounded) -- and combines the two directions of a row.
//
// Layout: one launch per epoch, one wave per vertex.  The wave takes its column in steps of 64 stored entries; a ballot
// compacts the firing entries, and the (firing entry, term) pairs -- the attractive term and the negative samples -- are
// spread over the lanes, so that only firing entries pay for pow and the lanes are full at ~ 6 terms per entry.  The clipped
// terms go through LDS to lane f < dim, which adds component f in the stated order and carries the sums from step to step.
#include "sgl_internal.h"
#include "umap_host.h"
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int CAP = UMAP_MERGE_WIDTH;
constexpr int BLK = UMAP_SUM_BLOCK;
constexpr uint64_t NO_KEY = ~0ull;      // the cell's own slot and the padding: sorts after every key
constexpr uint64_t DIR_IN = 1ull << 31;

int64_t g_info[4] = {-1, 0, 0, 0};      // sgl_umap_info

unsigned grid_for(int64_t n, int per_block) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, 1 << 20)); }

int hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return SGL_OK;
    (void)hipGetLastError();
    sgl_set_error("%s failed: %s", what, hipGetErrorString(e));
    return SGL_EHIP;
}
#define UMCHK(expr, what) SGLCHK(hip_ok((expr), what))
#define UMLAUNCHED(name) UMCHK(hipGetLastError(), name)

template <typename T>
int upload(hipStream_t s, DevBuf<T>& d, const T* h, size_t n, const char* what) {
    SGLCHK(d.alloc(std::max<size_t>(n, 1)));
    if (n > 0) UMCHK(hipMemcpyAsync(d.p, h, sizeof(T) * n, hipMemcpyHostToDevice, s), what);
    return SGL_OK;
}
template <typename T>
int fetch(hipStream_t s, T* h, const T* d, size_t n, const char* what) {   // synchronous
    if (n > 0) UMCHK(hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, s), what);
    UMCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    return SGL_OK;
}
template <typename F>
int cub_run(F call, const char* what) {
    size_t bytes = 0;
    UMCHK(call(nullptr, bytes), what);
    DevBuf<char> tmp;
    SGLCHK(tmp.alloc(std::max<size_t>(bytes, 1)));
    UMCHK(call(tmp.p, bytes), what);
    return SGL_OK;
}

// ---------------------------------------------------------------------------------------------------------- fuzzy graph ---
// The blocked sum of v[0, len) by one wave (kernels_cluster.hip's rule: blocks of BLK consecutive terms, each sequential from
// +0.0, then the block sums sequential in ascending block order) -> out[0].
__global__ __launch_bounds__(64) void fz_total_kernel(const double* __restrict__ v, int64_t len, double* __restrict__ out) {
    const int lane = threadIdx.x;
    double total = 0.0;
    for (int64_t b0 = 0; b0 * BLK < len; b0 += 64) {
        const int64_t lo = (b0 + lane) * BLK, hi = lo + BLK < len ? lo + BLK : len;
        double s = 0.0;
        for (int64_t t = lo; t < hi; ++t) s = s + v[t];
        const int64_t left = (len - b0 * BLK + BLK - 1) / BLK;
        const int nb = left < 64 ? (int)left : 64;
        for (int q = 0; q < nb; ++q) total = total + __shfl(s, q);
    }
    if (lane == 0) out[0] = total;
}

// One thread per cell: rho, sigma, the memberships of its K slots (the cell's own slot gets +0.0 and is never read), and the
// in-degree histogram of the others.
__global__ __launch_bounds__(256) void fz_cell_kernel(const int32_t* __restrict__ idx, const double* __restrict__ dist, int64_t n, int K,
                                                      double target, const double* __restrict__ total, double* __restrict__ rho_out,
                                                      double* __restrict__ sigma_out, double* __restrict__ P,
                                                      int64_t* __restrict__ indeg) {
    const double gmean = total[0] / (double)(n * (int64_t)K);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int32_t* li = idx + j * K;
        const double* ld = dist + j * K;
        double rho = 0.0, sum = 0.0;
        int own = 0;
        for (int q = 0; q < K; ++q) {
            if (li[q] == (int32_t)j) continue;
            const double d = ld[q];
            sum = sum + d;
            ++own;
            if (rho == 0.0 && d > 0.0) rho = d;   // the lists ascend: the first distance above 0 is the smallest
        }
        const double mean = rho > 0.0 ? sum / (double)own : gmean;
        double lo = 0.0, hi = INFINITY, mid = 1.0;
        for (int step = 0; step < 64; ++step) {
            double ps = 0.0;
            for (int q = 0; q < K; ++q) {
                if (li[q] == (int32_t)j) continue;
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
        const double sigma = fmax(mid, 1e-3 * mean);
        rho_out[j] = rho;
        sigma_out[j] = sigma;
        for (int q = 0; q < K; ++q) {
            const int32_t r = li[q];
            double m = 0.0;
            if (r != (int32_t)j) {
                const double t = ld[q] - rho;
                m = t > 0.0 ? exp(-t / sigma) : 1.0;
                atomicAdd((unsigned long long*)&indeg[r], 1ull);
            }
            P[j * K + q] = m;
        }
    }
}

// The counting transpose: entry (cell j, slot q) with r = idx != j goes to the incoming list of r, in no particular order
// (the merge sorts it).
__global__ void fz_fill_in_kernel(const int32_t* __restrict__ idx, const double* __restrict__ P, int64_t n, int K,
                                  int64_t* __restrict__ cursor, int32_t* __restrict__ Tsrc, double* __restrict__ Tp) {
    const int64_t total = n * (int64_t)K;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t r = idx[e];
        const int64_t j = e / K;
        if (r == (int32_t)j) continue;
        const int64_t pos = (int64_t)atomicAdd((unsigned long long*)&cursor[r], 1ull);
        Tsrc[pos] = (int32_t)j;
        Tp[pos] = P[e];
    }
}

struct FzArgs {
    const int32_t* idx;
    const double* P;
    const int64_t* inoff;     // [n + 1] offsets of the incoming lists
    const int32_t* Tsrc;
    const double* Tp;
    int K;
};

__device__ __forceinline__ uint64_t fz_key(const FzArgs& a, int64_t j, int64_t q) {   // q in [0, K + indeg_j)
    if (q < a.K) {
        const int32_t r = a.idx[j * a.K + q];
        return r == (int32_t)j ? NO_KEY : (((uint64_t)(uint32_t)r << 32) | (uint64_t)q);
    }
    const int64_t t = q - a.K;
    return ((uint64_t)(uint32_t)a.Tsrc[a.inoff[j] + t] << 32) | DIR_IN | (uint64_t)t;
}

// keys[0, m) ascending: a row's own-list entry (if any) right before its incoming entry (if any).  One whole wave.  For every
// row: w = (p_out + p_in) - p_out * p_in with an absent direction +0.0; entries with w != 0 are counted (cnt[j], !FILL) or
// written in ascending row at off[j] (FILL).
template <bool FILL>
__device__ __forceinline__ void fz_emit(const uint64_t* keys, int64_t m, int64_t j, const FzArgs& a, int32_t* __restrict__ cnt,
                                        const int64_t* __restrict__ off, int32_t* __restrict__ oi, double* __restrict__ ox) {
    const int lane = threadIdx.x & 63;
    int64_t base = 0;
    for (int64_t q0 = 0; q0 < m; q0 += 64) {
        const int64_t q = q0 + lane;
        bool keep = false;
        uint32_t row = 0;
        double w = 0.0;
        if (q < m) {
            const uint64_t k0 = keys[q];
            row = (uint32_t)(k0 >> 32);
            if (q == 0 || (uint32_t)(keys[q - 1] >> 32) != row) {
                double po = 0.0, pi = 0.0;
                const int64_t pos = (int64_t)(k0 & (DIR_IN - 1));
                if (k0 & DIR_IN) {
                    pi = a.Tp[a.inoff[j] + pos];
                } else {
                    po = a.P[j * a.K + pos];
                    if (q + 1 < m) {
                        const uint64_t k1 = keys[q + 1];
                        if ((uint32_t)(k1 >> 32) == row) pi = a.Tp[a.inoff[j] + (int64_t)(k1 & (DIR_IN - 1))];
                    }
                }
                w = (po + pi) - po * pi;
                keep = w != 0.0;
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (FILL && keep) {
            const int64_t at = off[j] + base + __popcll(mask & ((1ull << lane) - 1ull));
            oi[at] = (int32_t)row;
            ox[at] = w;
        }
        base += __popcll(mask);
    }
    if (!FILL && lane == 0) cnt[j] = (int32_t)base;
}

// The LDS merge: one wave per vertex of up to CAP keys.
template <bool FILL>
__global__ __launch_bounds__(64) void fz_merge_fast_kernel(FzArgs a, const int32_t* __restrict__ work, int64_t nwork,
                                                           int32_t* __restrict__ cnt, const int64_t* __restrict__ off,
                                                           int32_t* __restrict__ oi, double* __restrict__ ox) {
    __shared__ uint64_t s[CAP];
    const int lane = threadIdx.x;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t j = work[w];
        const int len = a.K + (int)(a.inoff[j + 1] - a.inoff[j]);   // <= CAP
        int P = 64;
        while (P < len) P <<= 1;
        int self = 0;
        for (int q = lane; q < P; q += 64) {
            const uint64_t key = q < len ? fz_key(a, j, q) : NO_KEY;
            if (q < len && key == NO_KEY) self = 1;
            s[q] = key;
        }
        const int m = len - (__any(self) ? 1 : 0);
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)   // bitonic sort, as the neighbour graphs' LDS sort
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = lane; t < P; t += 64) {
                    const int u = t ^ stride;
                    if (u > t) {
                        const uint64_t x = s[t], y = s[u];
                        const bool up = (t & size) == 0;
                        if ((x > y) == up) { s[t] = y; s[u] = x; }
                    }
                }
                __syncthreads();
            }
        fz_emit<FILL>(s, m, j, a, cnt, off, oi, ox);
        __syncthreads();
    }
}

// The fallback, step 1: the keys of the vertices above CAP into HBM, vertex w at soff[w].
__global__ __launch_bounds__(256) void fz_slow_keys_kernel(FzArgs a, const int32_t* __restrict__ work, int64_t nwork,
                                                           const int64_t* __restrict__ soff, uint64_t* __restrict__ keys) {
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t j = work[w], len = soff[w + 1] - soff[w];
        for (int64_t q = threadIdx.x; q < len; q += blockDim.x) keys[soff[w] + q] = fz_key(a, j, q);
    }
}
// Step 2, after the segmented sort: one wave per vertex.
template <bool FILL>
__global__ __launch_bounds__(64) void fz_merge_slow_kernel(FzArgs a, const int32_t* __restrict__ work, int64_t nwork,
                                                           const int64_t* __restrict__ soff, const uint64_t* __restrict__ sorted,
                                                           int32_t* __restrict__ cnt, const int64_t* __restrict__ off,
                                                           int32_t* __restrict__ oi, double* __restrict__ ox) {
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t j = work[w], len = soff[w + 1] - soff[w];
        const uint64_t* keys = sorted + soff[w];
        const int64_t m = len - (keys[len - 1] == NO_KEY ? 1 : 0);   // len > CAP; at most one own slot
        fz_emit<FILL>(keys, m, j, a, cnt, off, oi, ox);
    }
}

// --------------------------------------------------------------------------------------------------------------- layout ---
struct UmArgs {
    const int64_t* p;
    const int32_t* i;
    const double* x;
    const double* Y;      // positions of the epoch's start (read-only)
    double* Yn;           // each y written once
    int64_t n;
    int32_t dim;
    int32_t terms;        // 1 + neg_rate
    double a, b, m2ab, tb, alpha, w_max;
    int64_t t;            // the epoch, 1-based
    uint64_t seed;
};

// One wave per vertex.  DIM = 2 or 3: compile-time; DIM = 0: the generic loop up to UMAP_MAX_DIM.  B1: b == 1.0, p = d2.
template <int DIM, bool B1>
__global__ __launch_bounds__(64) void um_epoch_kernel(UmArgs A) {
    constexpr int D = DIM ? DIM : UMAP_MAX_DIM;
    __shared__ int32_t s_q[64];
    __shared__ double s_term[64 * D];
    const int dim = DIM ? DIM : A.dim;
    const int lane = threadIdx.x;
    const int T = A.terms;
    const double t1 = (double)A.t, t0 = (double)(A.t - 1);
    for (int64_t j = blockIdx.x; j < A.n; j += gridDim.x) {
        const int64_t p0 = A.p[j], p1 = A.p[j + 1];
        double yj[D];
#pragma unroll
        for (int f = 0; f < D; ++f) yj[f] = f < dim ? A.Y[j * dim + f] : 0.0;
        double g = 0.0, delta = 0.0;   // of component `lane` (lanes below dim)
        bool open = false;             // an entry's partial sum g is under way
        for (int64_t c0 = p0; c0 < p1; c0 += UMAP_CHUNK) {
            const int64_t e = c0 + lane;
            bool fire = false;
            if (e < p1 && A.i[e] != (int32_t)j) {
                const double r = A.x[e] / A.w_max;
                fire = floor(t1 * r) > floor(t0 * r);
            }
            const unsigned long long mask = __ballot(fire);
            const int nf = __popcll(mask);
            if (nf == 0) continue;
            if (fire) s_q[__popcll(mask & ((1ull << lane) - 1ull))] = lane;
            __syncthreads();
            const int items = nf * T;
            for (int I0 = 0; I0 < items; I0 += 64) {
                const int I = I0 + lane;
                if (I < items) {
                    const int q = I / T, sidx = I - q * T;
                    const int64_t ee = c0 + s_q[q];
                    int64_t o;
                    if (sidx == 0) {
                        o = A.i[ee];
                    } else {
                        const uint64_t u = sgl_rand2(A.seed, (uint64_t)ee, 256ull * (uint64_t)A.t + (uint64_t)(sidx - 1));
                        o = (int64_t)(((u >> 32) * (uint64_t)A.n) >> 32);
                    }
                    double df[D], d2 = 0.0;
#pragma unroll
                    for (int f = 0; f < D; ++f) {
                        if (f < dim) {
                            df[f] = yj[f] - A.Y[o * dim + f];
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
                    } else if (o == j) {
                        plain = true;
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
                __syncthreads();
            }
        }
        if (lane < dim) {
            const double y = A.Y[j * dim + lane];
            if (open) {
                delta = delta + g;
                const double step = A.alpha * delta;
                A.Yn[j * dim + lane] = y + step;
            } else {
                A.Yn[j * dim + lane] = y;   // no firing entry: the bits of y
            }
        }
    }
}

int um_launch(hipStream_t s, const UmArgs& A, int instance) {
    const dim3 grid(grid_for(A.n, 1)), block(64);
    switch (instance) {
        case 0: um_epoch_kernel<2, false><<<grid, block, 0, s>>>(A); break;
        case 1: um_epoch_kernel<2, true><<<grid, block, 0, s>>>(A); break;
        case 2: um_epoch_kernel<3, false><<<grid, block, 0, s>>>(A); break;
        case 3: um_epoch_kernel<3, true><<<grid, block, 0, s>>>(A); break;
        case 4: um_epoch_kernel<0, false><<<grid, block, 0, s>>>(A); break;
        default: um_epoch_kernel<0, true><<<grid, block, 0, s>>>(A); break;
    }
    UMLAUNCHED("um_epoch_kernel");
    return SGL_OK;
}

struct Layout {   // the graph and the two position buffers on the device
    DevBuf<int64_t> p;
    DevBuf<int32_t> i;
    DevBuf<double> x, Y[2];
};

// The refusals (on the host: nothing is launched for a refused call); *w_max receives the exact maximum weight.
int um_check(const char* who, const double* Gx, const int32_t* Gi, const int32_t* Gp, int64_t n, const double* Y0, int32_t dim, double a,
             double b, int32_t n_epochs, double alpha0, int32_t neg_rate, int64_t t, bool is_op, double* w_max) {
    int64_t pos = -1, col = -1;
    const UmapDefect f = umap_check(Gx, Gi, Gp, n, Y0, dim, a, b, n_epochs, alpha0, neg_rate, t, is_op, &pos, &col);
    if (f != UMAP_OK) {
        if (col >= 0) sgl_set_error("%s: invalid graph at column %lld, row %lld: %s", who, (long long)col, (long long)Gi[pos], umap_defect_text(f));
        else if (pos >= 0) sgl_set_error("%s: %s (at position %lld)", who, umap_defect_text(f), (long long)pos);
        else sgl_set_error("%s: %s", who, umap_defect_text(f));
        return SGL_EINVAL;
    }
    *w_max = umap_w_max(Gx, Gp[n]);
    return SGL_OK;
}

int um_upload(hipStream_t s, const double* Gx, const int32_t* Gi, const int32_t* Gp, int64_t n, const double* Y0, int32_t dim, Layout& L) {
    const int64_t nnz = Gp[n];
    std::vector<int64_t> hp((size_t)n + 1);
    for (int64_t c = 0; c <= n; ++c) hp[(size_t)c] = Gp[c];
    SGLCHK(upload(s, L.p, hp.data(), hp.size(), "upload of G@p"));
    SGLCHK(upload(s, L.i, Gi, (size_t)nnz, "upload of G@i"));
    SGLCHK(upload(s, L.x, Gx, (size_t)nnz, "upload of G@x"));
    SGLCHK(upload(s, L.Y[0], Y0, (size_t)(n * dim), "upload of Y"));
    SGLCHK(L.Y[1].alloc((size_t)(n * dim)));
    UMCHK(hipStreamSynchronize(s), "hipStreamSynchronize");   // hp leaves scope
    return SGL_OK;
}

UmArgs um_args(const Layout& L, int64_t n, int32_t dim, double a, double b, int32_t neg_rate, uint64_t seed, double w_max) {
    UmArgs A;
    A.p = L.p.p;
    A.i = L.i.p;
    A.x = L.x.p;
    A.Y = nullptr;
    A.Yn = nullptr;
    A.n = n;
    A.dim = dim;
    A.terms = 1 + neg_rate;
    A.a = a;
    A.b = b;
    A.m2ab = -2.0 * a * b;
    A.tb = 2.0 * b;
    A.alpha = 0.0;
    A.w_max = w_max;
    A.t = 0;
    A.seed = seed;
    return A;
}

void um_note_plan(const UmapPlan& P) {
    g_info[0] = P.instance;
    g_info[1] = P.widest;
    g_info[2] = P.multi_chunk;
}

struct StreamHolder {
    hipStream_t s = nullptr;
    ~StreamHolder() { if (s) (void)hipStreamDestroy(s); }
};

}  // namespace

extern "C" int sgl_c_fuzzy_graph(const int32_t* idx, const double* dist, int64_t n, int32_t K, int32_t* p_out, int64_t* nnz_out,
                                 int32_t* i_out, double* x_out, int64_t cap, double* rho_out, double* sigma_out) {
    static const char* who = "c_fuzzy_graph";
    if (!p_out || !nnz_out) { sgl_set_error("%s: bad arguments (p_out and nnz_out are needed)", who); return SGL_EINVAL; }
    if ((i_out == nullptr) != (x_out == nullptr)) { sgl_set_error("%s: i_out and x_out go together", who); return SGL_EINVAL; }
    int64_t cell = -1;
    int32_t slot = -1;
    const FuzzyDefect f = fuzzy_check(idx, dist, n, K, &cell, &slot);
    if (f != FUZZY_OK) {
        if (cell >= 0) sgl_set_error("%s: invalid neighbour list of cell %lld at place %d: %s", who, (long long)cell, slot, fuzzy_defect_text(f));
        else sgl_set_error("%s: %s", who, fuzzy_defect_text(f));
        return SGL_EINVAL;
    }
    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    hipStream_t s = hd.c->stream;
    const size_t nk = (size_t)n * (size_t)K;
    DevBuf<int32_t> didx, Tsrc, cnt, dfast, dslow, oi;
    DevBuf<double> ddist, total, rho, sigma, P, Tp, ox;
    DevBuf<int64_t> indeg, inoff, cursor, dsoff, doff;
    DevBuf<uint64_t> skeys, skeys2;
    SGLCHK(upload(s, didx, idx, nk, "upload of the indices"));
    SGLCHK(upload(s, ddist, dist, nk, "upload of the distances"));
    SGLCHK(total.alloc(1)); SGLCHK(rho.alloc((size_t)n)); SGLCHK(sigma.alloc((size_t)n)); SGLCHK(P.alloc(nk));
    SGLCHK(indeg.alloc((size_t)n + 1)); SGLCHK(inoff.alloc((size_t)n + 1)); SGLCHK(cursor.alloc((size_t)n + 1));
    SGLCHK(Tsrc.alloc(nk)); SGLCHK(Tp.alloc(nk)); SGLCHK(cnt.alloc((size_t)n));
    UMCHK(hipMemsetAsync(indeg.p, 0, sizeof(int64_t) * ((size_t)n + 1), s), "hipMemsetAsync");
    fz_total_kernel<<<dim3(1), dim3(64), 0, s>>>(ddist.p, (int64_t)nk, total.p);
    UMLAUNCHED("fz_total_kernel");
    fz_cell_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(didx.p, ddist.p, n, K, log2((double)K), total.p, rho.p, sigma.p, P.p, indeg.p);
    UMLAUNCHED("fz_cell_kernel");
    SGLCHK(k_exclusive_scan(hd.c, indeg.p, inoff.p, n));
    SGLCHK(k_scan_total(s, indeg.p, inoff.p, n));
    UMCHK(hipMemcpyAsync(cursor.p, inoff.p, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyDeviceToDevice, s), "copy");
    fz_fill_in_kernel<<<dim3(grid_for((int64_t)nk, 256)), dim3(256), 0, s>>>(didx.p, P.p, n, K, cursor.p, Tsrc.p, Tp.p);
    UMLAUNCHED("fz_fill_in_kernel");
    std::vector<int64_t> hindeg((size_t)n);
    SGLCHK(fetch(s, hindeg.data(), indeg.p, (size_t)n, "download of the in-degrees"));
    std::vector<int32_t> fast, slow;
    std::vector<int64_t> soff;
    fuzzy_split(hindeg.data(), n, K, fast, slow, soff);
    const int64_t nfast = (int64_t)fast.size(), nslow = (int64_t)slow.size(), stot = soff.back();
    if (stot > (int64_t)INT32_MAX) {
        sgl_set_error("%s: the vertices beyond the LDS merge hold %lld keys, more than one segmented sort takes", who, (long long)stot);
        return SGL_EINVAL;
    }
    SGLCHK(upload(s, dfast, fast.data(), fast.size(), "upload"));
    SGLCHK(upload(s, dslow, slow.data(), slow.size(), "upload"));
    SGLCHK(upload(s, dsoff, soff.data(), soff.size(), "upload"));
    const FzArgs a{didx.p, P.p, inoff.p, Tsrc.p, Tp.p, K};
    // --- count pass
    if (nfast > 0) {
        fz_merge_fast_kernel<false><<<dim3(grid_for(nfast, 1)), dim3(64), 0, s>>>(a, dfast.p, nfast, cnt.p, nullptr, nullptr, nullptr);
        UMLAUNCHED("fz_merge_fast_kernel");
    }
    if (nslow > 0) {
        SGLCHK(skeys.alloc((size_t)stot));
        SGLCHK(skeys2.alloc((size_t)stot));
        fz_slow_keys_kernel<<<dim3(grid_for(nslow, 1)), dim3(256), 0, s>>>(a, dslow.p, nslow, dsoff.p, skeys.p);
        UMLAUNCHED("fz_slow_keys_kernel");
        SGLCHK(cub_run([&](void* tmp, size_t& bytes) {
            return hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, bytes, skeys.p, skeys2.p, (int)stot, (int)nslow, dsoff.p, dsoff.p + 1,
                                                              0, 64, s);
        }, "segmented sort of the hub keys"));
        fz_merge_slow_kernel<false><<<dim3(grid_for(nslow, 1)), dim3(64), 0, s>>>(a, dslow.p, nslow, dsoff.p, skeys2.p, cnt.p, nullptr,
                                                                                 nullptr, nullptr);
        UMLAUNCHED("fz_merge_slow_kernel");
    }
    std::vector<int32_t> hcnt((size_t)n);
    SGLCHK(fetch(s, hcnt.data(), cnt.p, (size_t)n, "download of the counts"));
    std::vector<int32_t> hp((size_t)n + 1);
    int64_t nnz = 0;
    if (!fuzzy_pointers(hcnt.data(), n, hp.data(), &nnz)) {
        sgl_set_error("%s: the graph would hold %lld entries, which a dgCMatrix (32-bit column pointers) cannot hold", who, (long long)nnz);
        return SGL_EINVAL;
    }
    if (i_out && cap < nnz) {
        sgl_set_error("%s: output capacity %lld < %lld entries", who, (long long)cap, (long long)nnz);
        return SGL_EINVAL;
    }
    g_info[3] = nslow;
    memcpy(p_out, hp.data(), sizeof(int32_t) * ((size_t)n + 1));
    *nnz_out = nnz;
    if (rho_out) SGLCHK(fetch(s, rho_out, rho.p, (size_t)n, "download of rho"));
    if (sigma_out) SGLCHK(fetch(s, sigma_out, sigma.p, (size_t)n, "download of sigma"));
    if (!i_out) return SGL_OK;
    // --- fill pass
    std::vector<int64_t> hoff(hp.begin(), hp.end());
    SGLCHK(upload(s, doff, hoff.data(), hoff.size(), "upload of p"));
    SGLCHK(oi.alloc((size_t)std::max<int64_t>(nnz, 1)));
    SGLCHK(ox.alloc((size_t)std::max<int64_t>(nnz, 1)));
    if (nfast > 0) {
        fz_merge_fast_kernel<true><<<dim3(grid_for(nfast, 1)), dim3(64), 0, s>>>(a, dfast.p, nfast, nullptr, doff.p, oi.p, ox.p);
        UMLAUNCHED("fz_merge_fast_kernel");
    }
    if (nslow > 0) {
        fz_merge_slow_kernel<true><<<dim3(grid_for(nslow, 1)), dim3(64), 0, s>>>(a, dslow.p, nslow, dsoff.p, skeys2.p, nullptr, doff.p,
                                                                                oi.p, ox.p);
        UMLAUNCHED("fz_merge_slow_kernel");
    }
    if (nnz > 0) {
        UMCHK(hipMemcpyAsync(i_out, oi.p, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, s), "download of i");
        UMCHK(hipMemcpyAsync(x_out, ox.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, s), "download of x");
    }
    UMCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    return SGL_OK;
}

extern "C" int sgl_c_umap_layout(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* Y0, int32_t dim,
                                 double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, double* Y) {
    static const char* who = "c_umap_layout";
    if (!Y) { sgl_set_error("%s: Y is NULL", who); return SGL_EINVAL; }
    StreamHolder sh;
    Layout L;
    double w_max = 0.0;
    SGLCHK(um_check(who, Gx, Gi, Gp, n, Y0, dim, a, b, n_epochs, alpha0, neg_rate, 0, false, &w_max));
    const UmapPlan plan = umap_plan(Gp, n, dim, b, n_epochs);
    if (!(w_max > 0.0)) {   // nothing attracts and nothing fires: the start
        um_note_plan(plan);
        memmove(Y, Y0, sizeof(double) * (size_t)n * (size_t)dim);
        return SGL_OK;
    }
    UMCHK(hipStreamCreate(&sh.s), "hipStreamCreate");
    SGLCHK(um_upload(sh.s, Gx, Gi, Gp, n, Y0, dim, L));
    um_note_plan(plan);
    UmArgs A = um_args(L, n, dim, a, b, neg_rate, seed, w_max);
    int rc = SGL_OK;
    const int last = umap_run_epochs(n_epochs, alpha0, [&](int64_t t, double alpha, int from, int to) -> int {
        A.Y = L.Y[from].p;
        A.Yn = L.Y[to].p;
        A.t = t;
        A.alpha = alpha;
        return um_launch(sh.s, A, plan.instance);
    }, &rc);
    SGLCHK(rc);
    return fetch(sh.s, Y, L.Y[last].p, (size_t)n * (size_t)dim, "download of Y");
}

extern "C" int sgl_op_umap_epoch(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* Yin, int32_t dim,
                                 double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, int32_t t,
                                 double* Y) {
    static const char* who = "op_umap_epoch";
    if (!Y) { sgl_set_error("%s: Y is NULL", who); return SGL_EINVAL; }
    StreamHolder sh;
    Layout L;
    double w_max = 0.0;
    SGLCHK(um_check(who, Gx, Gi, Gp, n, Yin, dim, a, b, n_epochs, alpha0, neg_rate, t, true, &w_max));
    const UmapPlan plan = umap_plan(Gp, n, dim, b, n_epochs);
    if (!(w_max > 0.0)) {
        um_note_plan(plan);
        memmove(Y, Yin, sizeof(double) * (size_t)n * (size_t)dim);
        return SGL_OK;
    }
    UMCHK(hipStreamCreate(&sh.s), "hipStreamCreate");
    SGLCHK(um_upload(sh.s, Gx, Gi, Gp, n, Yin, dim, L));
    um_note_plan(plan);
    UmArgs A = um_args(L, n, dim, a, b, neg_rate, seed, w_max);
    A.Y = L.Y[0].p;
    A.Yn = L.Y[1].p;
    A.t = t;
    A.alpha = umap_alpha(alpha0, t, n_epochs);
    SGLCHK(um_launch(sh.s, A, plan.instance));
    return fetch(sh.s, Y, L.Y[1].p, (size_t)n * (size_t)dim, "download of Y");
}

extern "C" int sgl_umap_info(int64_t out[4]) {
    if (!out) { sgl_set_error("sgl_umap_info: out is NULL"); return SGL_EINVAL; }
    for (int q = 0; q < 4; ++q) out[q] = g_info[q];
    return SGL_OK;
}
