// Louvain clustering of a neighbour graph on the GPU: sgl_c_louvain, sgl_op_louvain_sweep, sgl_louvain_info
// (include/singlet_hip.h, "Clustering"; the rules restated in tests/louvain_restatement.py).  The reference package has no
// clustering code (it hands the graph to Seurat), so the rules are this library's own and every sum has ONE order that
// depends on the graph and the labels alone: no floating-point atomic anywhere, no contraction, and no result that depends
// on the launch shape.
//
//   per-vertex sums (k_v, own_v, w_c of a sweep): sequential in ascending row, from +0.0;
//   sums over members, communities and the fine entries of a coarse entry: blocks of LOUVAIN_SUM_BLOCK consecutive terms,
//   each sequential from +0.0, then the block sums sequential from +0.0 (wave_blocked_sum: 64 blocks in flight per wave).
//
// The sweep is a gather of the label of every stored entry plus a group-by per vertex: keys (community << 32 | position in the
// column) are sorted -- by one wave in LDS up to LOUVAIN_FAST_DEGREE entries, by a segmented radix sort in HBM above -- so
// that a community's entries are a run in ascending row; lv_decide turns the runs into gains and picks the move.
#include "sgl_internal.h"
#include "cluster_host.h"
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

constexpr int CAP = LOUVAIN_FAST_DEGREE;
constexpr int BLK = LOUVAIN_SUM_BLOCK;
constexpr uint64_t NO_KEY = ~0ull;      // the diagonal entry and the padding: sorts after every key

int64_t g_info[4] = {CAP, 0, 0, 0};     // sgl_louvain_info

unsigned grid_for(int64_t n, int per_block) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, 1 << 20)); }

int hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return SGL_OK;
    (void)hipGetLastError();
    sgl_set_error("%s failed: %s", what, hipGetErrorString(e));
    return SGL_EHIP;
}
#define LVCHK(expr, what) SGLCHK(hip_ok((expr), what))
#define LVLAUNCHED(name) LVCHK(hipGetLastError(), name)

template <typename T>
int upload(hipStream_t s, DevBuf<T>& d, const T* h, size_t n, const char* what) {
    SGLCHK(d.alloc(std::max<size_t>(n, 1)));
    if (n > 0) LVCHK(hipMemcpyAsync(d.p, h, sizeof(T) * n, hipMemcpyHostToDevice, s), what);
    return SGL_OK;
}
template <typename T>
int fetch(hipStream_t s, T* h, const T* d, size_t n, const char* what) {   // synchronous
    if (n > 0) LVCHK(hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, s), what);
    LVCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    return SGL_OK;
}
template <typename F>
int cub_run(F call, const char* what) {
    size_t bytes = 0;
    LVCHK(call(nullptr, bytes), what);
    DevBuf<char> tmp;
    SGLCHK(tmp.alloc(std::max<size_t>(bytes, 1)));
    LVCHK(call(tmp.p, bytes), what);
    return SGL_OK;
}
struct StreamHolder {
    hipStream_t s = nullptr;
    ~StreamHolder() { if (s) (void)hipStreamDestroy(s); }
};
int bits_for(int64_t values) {   // bits that hold 0 .. values-1
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < values) ++b;
    return b;
}

// ------------------------------------------------------------------------------------------------------ device helpers ---
// The blocked sum of term(0) .. term(len-1) by one whole wave (all 64 lanes call it with the same len), to every lane.
// Lane l sums block b0 + l sequentially; the block sums are then added in ascending block order by every lane alike.
template <typename F>
__device__ __forceinline__ double wave_blocked_sum(F term, int64_t len) {
    const int lane = threadIdx.x & 63;
    double total = 0.0;
    for (int64_t b0 = 0; b0 * BLK < len; b0 += 64) {
        const int64_t lo = (b0 + lane) * BLK, hi = lo + BLK < len ? lo + BLK : len;
        double s = 0.0;
        int64_t t = lo;
        for (; t + 8 <= hi; t += 8) {   // eight loads in flight, the additions in order
            double a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = term(t + u);
#pragma unroll
            for (int u = 0; u < 8; ++u) s = s + a[u];
        }
        for (; t < hi; ++t) s = s + term(t);
        const int64_t left = (len - b0 * BLK + BLK - 1) / BLK;
        const int nb = left < 64 ? (int)left : 64;
        for (int q = 0; q < nb; ++q) total = total + __shfl(s, q);
    }
    return total;
}

// the first position of sorted[0, n) that is not below key
template <typename T>
__device__ __forceinline__ int64_t lower_bound_dev(const T* sorted, int64_t n, T key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void atomic_min_u64(unsigned long long* a, unsigned long long v) { atomicMin(a, v); }

// In-LDS bitonic sort of s[0, P) ascending, P a power of two >= 64; one 64-lane workgroup (as kernels_neighbors.hip).
__device__ __forceinline__ void bitonic_lds(uint64_t* s, int P) {
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < P; t += 64) {
                const int u = t ^ stride;
                if (u > t) {
                    const uint64_t x = s[t], y = s[u];
                    const bool up = (t & size) == 0;
                    if ((x > y) == up) { s[t] = y; s[u] = x; }
                }
            }
            __syncthreads();
        }
}

// ---------------------------------------------------------------------------------------------------------- validation ---
// One wave per column.  first = the lowest entry index with a defect (integer atomicMin).  Pass 0: row range, row order,
// non-finite and negative weights.  Pass 1 (on a graph that passed 0): A_rc exists with the bits of A_cr.
template <int PASS>
__global__ __launch_bounds__(256) void lv_validate_kernel(const int64_t* __restrict__ p, const int32_t* __restrict__ i,
                                                          const double* __restrict__ x, int64_t n, unsigned long long* first) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t c = wave; c < n; c += nwaves)
        for (int64_t e = p[c] + lane; e < p[c + 1]; e += 64) {
            const int64_t r = i[e];
            bool bad;
            if (PASS == 0) {
                const double v = x[e];
                bad = r < 0 || r >= n || (e > p[c] && i[e - 1] >= r) || !(v - v == 0.0) || v < 0.0;
            } else {
                bad = false;
                if (r != c) {
                    const int64_t lo = p[r], len = p[r + 1] - lo;
                    const int64_t at = lower_bound_dev(i + lo, len, (int32_t)c);
                    bad = at >= len || i[lo + at] != (int32_t)c ||
                          __double_as_longlong(x[lo + at]) != __double_as_longlong(x[e]);
                }
            }
            if (bad) atomic_min_u64(first, (unsigned long long)e);
        }
}

// --------------------------------------------------------------------------------------------------- degrees, modularity ---
__global__ void lv_iota_kernel(int32_t* a, int64_t n) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) a[v] = (int32_t)v;
}

// k_v: the sequential sum of column v.
__global__ void lv_degree_kernel(const int64_t* __restrict__ p, const double* __restrict__ x, int64_t n, double* __restrict__ k) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int64_t e = p[v]; e < p[v + 1]; ++e) s = s + x[e];
        k[v] = s;
    }
}

// own_v: the sequential sum of the entries of column v whose row lies in v's community (the diagonal is one of them).
__global__ void lv_own_kernel(const int64_t* __restrict__ p, const int32_t* __restrict__ i, const double* __restrict__ x,
                              const int32_t* __restrict__ L, int64_t n, double* __restrict__ own) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const int32_t o = L[v];
        double s = 0.0;
        for (int64_t e = p[v]; e < p[v + 1]; ++e)
            if (L[i[e]] == o) s = s + x[e];
        own[v] = s;
    }
}

// out[0] = the blocked sum of v[0, n): one wave.
__global__ __launch_bounds__(64) void lv_total_kernel(const double* __restrict__ v, int64_t n, double* __restrict__ out) {
    const double t = wave_blocked_sum([&](int64_t q) { return v[q]; }, n);
    if (threadIdx.x == 0) out[0] = t;
}

// The members of community c are mem[cstart[c], cend[c]) of the vertices sorted (stably) by label, in ascending vertex; both
// arrays are zero beforehand, so an id without members has none.
__global__ void lv_bounds_kernel(const int32_t* __restrict__ sl, int64_t n, int32_t* __restrict__ cstart, int32_t* __restrict__ cend) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = sl[q];
        if (q == 0 || sl[q - 1] != c) cstart[c] = (int32_t)q;
        if (q == n - 1 || sl[q + 1] != c) cend[c] = (int32_t)(q + 1);
    }
}

// One wave per community id c.  tot_c, in_c: blocked sums over its members; term_c = in_c / S - (gamma * (tot_c / S)) * (tot_c / S).
__global__ __launch_bounds__(256) void lv_community_kernel(const int32_t* __restrict__ cstart, const int32_t* __restrict__ cend,
                                                           const int32_t* __restrict__ mem, const double* __restrict__ k,
                                                           const double* __restrict__ own, int64_t n, const double* __restrict__ Sp,
                                                           double gamma, double* __restrict__ tot, int32_t* __restrict__ size,
                                                           double* __restrict__ term) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const double S = Sp[0];
    for (int64_t c = wave; c < n; c += nwaves) {
        const int64_t lo = cstart[c], len = cend[c] - lo;
        const double t = wave_blocked_sum([&](int64_t q) { return k[mem[lo + q]]; }, len);
        const double in = wave_blocked_sum([&](int64_t q) { return own[mem[lo + q]]; }, len);
        if (lane == 0) {
            const double b = t / S;
            tot[c] = t;
            size[c] = (int32_t)len;
            term[c] = in / S - (gamma * b) * b;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- sweep ---
struct SweepArgs {
    const int64_t* p;
    const int32_t* i;
    const double* x;
    const int32_t* L;        // labels of the sweep's start
    const double* k;
    const double* tot;       // of the sweep's start
    const int32_t* size;
    const double* S;
    double gamma;
    int32_t* Lnew;
    unsigned long long* moved;
};

// keys[0, m): the off-diagonal entries of vertex v as (community << 32 | position in the column), ascending: a community's
// entries are a run in ascending row.  NT threads of one workgroup.  For each run, w_c sequentially over the run, then
//     g(c) = w_c - ((gamma * k_v) * (c == o ? tot_c - k_v : tot_c)) / S
// and the best candidate by (g descending, id ascending) among the runs and the own community o (w_o = +0.0 without a run).
// The vertex moves when best != o, g(best) > g(o), and not (o and best both hold one vertex and best > o).
template <int NT>
__device__ __forceinline__ void lv_decide(const uint64_t* keys, int64_t m, int64_t v, int64_t p0, const SweepArgs& a, double* sg,
                                          int32_t* sc, double* s_go) {
    const int tid = threadIdx.x;
    const int32_t o = a.L[v];
    const double kv = a.k[v], S = a.S[0], gk = a.gamma * kv;
    if (tid == 0) *s_go = NAN;   // NaN: no run of the own community (g is never NaN on a finite graph)
    __syncthreads();
    double gb = 0.0;
    int32_t cb = -1;
    for (int64_t q = tid; q < m; q += NT) {
        const int32_t c = (int32_t)(keys[q] >> 32);
        if (q > 0 && (int32_t)(keys[q - 1] >> 32) == c) continue;
        double w = 0.0;
        for (int64_t t = q; t < m && (int32_t)(keys[t] >> 32) == c; ++t) w = w + a.x[p0 + (int64_t)(uint32_t)keys[t]];
        const double tc = c == o ? a.tot[c] - kv : a.tot[c];
        const double g = w - (gk * tc) / S;
        if (c == o) *s_go = g;
        if (cb < 0 || g > gb) { gb = g; cb = c; }   // a thread's runs come in ascending id: a tie stays with the lower
    }
    sg[tid] = gb;
    sc[tid] = cb;
    __syncthreads();
    if (tid == 0) {
        double go = *s_go;
        double best_g = 0.0;
        int32_t best = -1;
        for (int t = 0; t < NT; ++t) {
            const int32_t c = sc[t];
            if (c < 0) continue;
            if (best < 0 || sg[t] > best_g || (sg[t] == best_g && c < best)) { best_g = sg[t]; best = c; }
        }
        if (go != go) {   // the own community has no run
            go = 0.0 - (gk * (a.tot[o] - kv)) / S;
            if (best < 0 || go > best_g || (go == best_g && o < best)) { best_g = go; best = o; }
        }
        int32_t to = o;
        if (m > 0 && best != o && best_g > go && !(a.size[o] == 1 && a.size[best] == 1 && best > o)) to = best;
        a.Lnew[v] = to;
        if (to != o) atomicAdd(a.moved, 1ull);
    }
    __syncthreads();
}

// Fast path: one wave per vertex of up to CAP stored entries (the vertices without any included).
__global__ __launch_bounds__(64) void lv_sweep_fast_kernel(SweepArgs a, const int32_t* __restrict__ work, int64_t nwork) {
    __shared__ uint64_t s[CAP];
    __shared__ double sg[64];
    __shared__ int32_t sc[64];
    __shared__ double s_go;
    const int lane = threadIdx.x;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t v = work[w];
        const int64_t p0 = a.p[v];
        const int len = (int)(a.p[v + 1] - p0);   // <= CAP
        int P = 64;
        while (P < len) P <<= 1;
        int diag = 0;
        for (int q = lane; q < P; q += 64) {
            uint64_t key = NO_KEY;
            if (q < len) {
                const int32_t j = a.i[p0 + q];
                if (j == (int32_t)v) diag = 1;
                else key = ((uint64_t)(uint32_t)a.L[j] << 32) | (uint32_t)q;
            }
            s[q] = key;
        }
        const int m = len - (__any(diag) ? 1 : 0);
        __syncthreads();
        if (len > 1) bitonic_lds(s, P);   // (by len, not m: a diagonal entry ahead of the only neighbour has to move behind it)
        lv_decide<64>(s, m, v, p0, a, sg, sc, &s_go);
    }
}

// Slow path, step 1: the keys of the vertices above CAP into HBM, vertex w at soff[w].
__global__ __launch_bounds__(256) void lv_slow_keys_kernel(SweepArgs a, const int32_t* __restrict__ work, int64_t nwork,
                                                           const int64_t* __restrict__ soff, uint64_t* __restrict__ keys) {
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t v = work[w], p0 = a.p[v], len = a.p[v + 1] - p0;
        for (int64_t q = threadIdx.x; q < len; q += blockDim.x) {
            const int32_t j = a.i[p0 + q];
            keys[soff[w] + q] = j == (int32_t)v ? NO_KEY : (((uint64_t)(uint32_t)a.L[j] << 32) | (uint32_t)q);
        }
    }
}
// Step 2, after the segmented sort: one 256-thread workgroup per vertex.
__global__ __launch_bounds__(256) void lv_sweep_slow_kernel(SweepArgs a, const int32_t* __restrict__ work, int64_t nwork,
                                                            const int64_t* __restrict__ soff, const uint64_t* __restrict__ sorted) {
    __shared__ double sg[256];
    __shared__ int32_t sc[256];
    __shared__ double s_go;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t v = work[w], len = soff[w + 1] - soff[w];
        const uint64_t* keys = sorted + soff[w];
        const int64_t m = len - (keys[len - 1] == NO_KEY ? 1 : 0);   // len > CAP >= 1; at most one diagonal entry
        lv_decide<256>(keys, m, v, a.p[v], a, sg, sc, &s_go);
    }
}

// --------------------------------------------------------------------------------------------------------- aggregation ---
__global__ void lv_mark_kernel(const int32_t* __restrict__ L, int64_t n, int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) flag[L[v]] = 1;
}
// assign[u] = cmap[L[assign[u]]] for every vertex u of the input graph
__global__ void lv_assign_kernel(int32_t* __restrict__ assign, int64_t n0, const int32_t* __restrict__ L, const int32_t* __restrict__ cmap) {
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n0; u += (int64_t)gridDim.x * blockDim.x)
        assign[u] = cmap[L[assign[u]]];
}
// key of fine entry e = (u, v): (community of the column << 32 | community of the row), value e: a stable sort by key leaves
// every coarse entry's fine entries in column-major order.  One wave per column.
__global__ __launch_bounds__(256) void lv_edge_keys_kernel(const int64_t* __restrict__ p, const int32_t* __restrict__ i,
                                                           const int32_t* __restrict__ L, const int32_t* __restrict__ cmap, int64_t n,
                                                           uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t v = wave; v < n; v += nwaves) {
        const uint64_t d = (uint64_t)(uint32_t)cmap[L[v]] << 32;
        for (int64_t e = p[v] + lane; e < p[v + 1]; e += 64) {
            key[e] = d | (uint32_t)cmap[L[i[e]]];
            val[e] = (uint32_t)e;
        }
    }
}
__global__ void lv_heads_kernel(const uint64_t* __restrict__ skey, int64_t nnz, int32_t* __restrict__ head) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= nnz; e += (int64_t)gridDim.x * blockDim.x)
        head[e] = e < nnz && (e == 0 || skey[e] != skey[e - 1]) ? 1 : 0;
}
__global__ void lv_group_start_kernel(const uint64_t* __restrict__ skey, const int32_t* __restrict__ gidx, int64_t nnz, int64_t ng,
                                      int64_t* __restrict__ gstart, uint64_t* __restrict__ gkey) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x) {
        if (e == 0 || skey[e] != skey[e - 1]) {
            gstart[gidx[e]] = e;
            gkey[gidx[e]] = skey[e];
        }
        if (e == 0) gstart[ng] = nnz;
    }
}
// One wave per coarse entry: the blocked sum of its fine entries in sorted (column-major) order.
__global__ __launch_bounds__(256) void lv_group_sum_kernel(const int64_t* __restrict__ gstart, const uint64_t* __restrict__ gkey,
                                                           const uint32_t* __restrict__ sval, const double* __restrict__ x, int64_t ng,
                                                           int32_t* __restrict__ ci, double* __restrict__ cx) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t g = wave; g < ng; g += nwaves) {
        const int64_t lo = gstart[g], len = gstart[g + 1] - lo;
        const double t = wave_blocked_sum([&](int64_t q) { return x[sval[lo + q]]; }, len);
        if (lane == 0) {
            ci[g] = (int32_t)(uint32_t)gkey[g];
            cx[g] = t;
        }
    }
}
__global__ void lv_coarse_p_kernel(const uint64_t* __restrict__ gkey, int64_t ng, int64_t nc, int64_t* __restrict__ cp) {
    for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d <= nc; d += (int64_t)gridDim.x * blockDim.x)
        cp[d] = lower_bound_dev(gkey, ng, (uint64_t)d << 32);
}

// ----------------------------------------------------------------------------------------------------------- host side ---
struct Graph {   // a level's graph on the device (not owned)
    const int64_t* p = nullptr;
    const int32_t* i = nullptr;
    const double* x = nullptr;
    int64_t n = 0, nnz = 0;
};
struct OwnedGraph {
    DevBuf<int64_t> p;
    DevBuf<int32_t> i;
    DevBuf<double> x;
    int64_t n = 0, nnz = 0;
    Graph view() const { Graph g; g.p = p.p; g.i = i.p; g.x = x.p; g.n = n; g.nnz = nnz; return g; }
    void take(OwnedGraph& o) { std::swap(p.p, o.p.p); std::swap(i.p, o.i.p); std::swap(x.p, o.x.p); n = o.n; nnz = o.nnz; }
};

// Buffers of the level-0 size, reused by every level and resolution.
struct Work {
    DevBuf<double> k, own, tot, tot2, term, S, Q;
    DevBuf<int32_t> size, size2, sl, mem, cstart, cend, iota, La, Lb, flag, cmap, assign, dfast, dslow;
    DevBuf<int64_t> dsoff;
    DevBuf<uint64_t> skeys, skeys2;
    DevBuf<unsigned long long> moved;
    std::vector<int32_t> fast, slow;
    std::vector<int64_t> soff;
    int alloc(int64_t n) {
        const size_t m = (size_t)std::max<int64_t>(n, 1);
        SGLCHK(k.alloc(m)); SGLCHK(own.alloc(m)); SGLCHK(tot.alloc(m)); SGLCHK(tot2.alloc(m)); SGLCHK(term.alloc(m));
        SGLCHK(S.alloc(1)); SGLCHK(Q.alloc(1)); SGLCHK(size.alloc(m)); SGLCHK(size2.alloc(m)); SGLCHK(sl.alloc(m));
        SGLCHK(mem.alloc(m)); SGLCHK(cstart.alloc(m)); SGLCHK(cend.alloc(m)); SGLCHK(iota.alloc(m)); SGLCHK(La.alloc(m)); SGLCHK(Lb.alloc(m)); SGLCHK(flag.alloc(m + 1));
        SGLCHK(cmap.alloc(m + 1)); SGLCHK(assign.alloc(m)); SGLCHK(moved.alloc(1));
        return SGL_OK;
    }
};

// k and S of a level's graph; *S_host receives S.
int lv_degrees(hipStream_t s, const Graph& G, Work& W, double* S_host) {
    lv_degree_kernel<<<dim3(grid_for(G.n, 256)), dim3(256), 0, s>>>(G.p, G.x, G.n, W.k.p);
    LVLAUNCHED("lv_degree_kernel");
    lv_total_kernel<<<dim3(1), dim3(64), 0, s>>>(W.k.p, G.n, W.S.p);
    LVLAUNCHED("lv_total_kernel");
    return fetch(s, S_host, W.S.p, 1, "download of S");
}

// Q of labels L on G (k and S of the level in W) -> *Q_host; tot and size of L into the given buffers.
int lv_modularity(hipStream_t s, const Graph& G, const int32_t* L, double gamma, Work& W, double* tot, int32_t* size, double* Q_host) {
    const int64_t n = G.n;
    lv_own_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(G.p, G.i, G.x, L, n, W.own.p);
    LVLAUNCHED("lv_own_kernel");
    const int bits = bits_for(n);
    SGLCHK(cub_run([&](void* tmp, size_t& bytes) {   // LSD radix sort is stable: a community's members stay in ascending vertex
        return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, L, W.sl.p, W.iota.p, W.mem.p, (int)n, 0, bits, s);
    }, "sort of the vertices by label"));
    LVCHK(hipMemsetAsync(W.cstart.p, 0, sizeof(int32_t) * (size_t)n, s), "hipMemsetAsync");
    LVCHK(hipMemsetAsync(W.cend.p, 0, sizeof(int32_t) * (size_t)n, s), "hipMemsetAsync");
    lv_bounds_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(W.sl.p, n, W.cstart.p, W.cend.p);
    LVLAUNCHED("lv_bounds_kernel");
    lv_community_kernel<<<dim3(grid_for(n, 4)), dim3(256), 0, s>>>(W.cstart.p, W.cend.p, W.mem.p, W.k.p, W.own.p, n, W.S.p, gamma, tot, size, W.term.p);
    LVLAUNCHED("lv_community_kernel");
    lv_total_kernel<<<dim3(1), dim3(64), 0, s>>>(W.term.p, n, W.Q.p);
    LVLAUNCHED("lv_total_kernel");
    return fetch(s, Q_host, W.Q.p, 1, "download of Q");
}

// The two work lists of a level from its column pointers on the host.
template <typename P_>
int lv_split(hipStream_t s, const P_* hp, int64_t n, Work& W) {
    louvain_split(hp, n, W.fast, W.slow, W.soff);
    SGLCHK(upload(s, W.dfast, W.fast.data(), W.fast.size(), "upload"));
    SGLCHK(upload(s, W.dslow, W.slow.data(), W.slow.size(), "upload"));
    SGLCHK(upload(s, W.dsoff, W.soff.data(), W.soff.size(), "upload"));
    const size_t stot = (size_t)W.soff.back();
    if (stot > 0) {
        SGLCHK(W.skeys.alloc(stot));
        SGLCHK(W.skeys2.alloc(stot));
    }
    return SGL_OK;
}

// One synchronous sweep: L -> Lnew with the tot / size of L; *moved_host receives the number of moved vertices.
int lv_sweep(hipStream_t s, const Graph& G, const int32_t* L, int32_t* Lnew, const double* tot, const int32_t* size, double gamma,
             Work& W, int64_t* moved_host) {
    SweepArgs a{G.p, G.i, G.x, L, W.k.p, tot, size, W.S.p, gamma, Lnew, W.moved.p};
    LVCHK(hipMemsetAsync(W.moved.p, 0, sizeof(unsigned long long), s), "hipMemsetAsync");
    const int64_t nfast = (int64_t)W.fast.size(), nslow = (int64_t)W.slow.size();
    if (nfast > 0) {
        lv_sweep_fast_kernel<<<dim3(grid_for(nfast, 1)), dim3(64), 0, s>>>(a, W.dfast.p, nfast);
        LVLAUNCHED("lv_sweep_fast_kernel");
    }
    if (nslow > 0) {
        const int64_t stot = W.soff.back();
        lv_slow_keys_kernel<<<dim3(grid_for(nslow, 1)), dim3(256), 0, s>>>(a, W.dslow.p, nslow, W.dsoff.p, W.skeys.p);
        LVLAUNCHED("lv_slow_keys_kernel");
        SGLCHK(cub_run([&](void* tmp, size_t& bytes) {
            return hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, bytes, W.skeys.p, W.skeys2.p, (int)stot, (int)nslow, W.dsoff.p,
                                                              W.dsoff.p + 1, 0, 64, s);
        }, "segmented sort of the hub keys"));
        lv_sweep_slow_kernel<<<dim3(grid_for(nslow, 1)), dim3(256), 0, s>>>(a, W.dslow.p, nslow, W.dsoff.p, W.skeys2.p);
        LVLAUNCHED("lv_sweep_slow_kernel");
    }
    unsigned long long mv = 0;
    SGLCHK(fetch(s, &mv, W.moved.p, 1, "download of the move count"));
    *moved_host = (int64_t)mv;
    return SGL_OK;
}

// Renumbers the surviving ids of L in ascending order (cmap), applies the level to assign[0, n0), and, with build, makes
// the coarse graph of L.  *nc_out = the number of communities.
int lv_aggregate(hipStream_t s, const Graph& G, const int32_t* L, Work& W, int64_t n0, bool build, OwnedGraph& out, int64_t* nc_out,
                 std::vector<int64_t>& cp_host) {
    const int64_t n = G.n, nnz = G.nnz;
    LVCHK(hipMemsetAsync(W.flag.p, 0, sizeof(int32_t) * (size_t)(n + 1), s), "hipMemsetAsync");
    lv_mark_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(L, n, W.flag.p);
    LVLAUNCHED("lv_mark_kernel");
    SGLCHK(cub_run([&](void* tmp, size_t& bytes) {
        return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, W.flag.p, W.cmap.p, (int)(n + 1), s);
    }, "scan of the surviving ids"));
    int32_t nc32 = 0;
    SGLCHK(fetch(s, &nc32, W.cmap.p + n, 1, "download of the community count"));
    const int64_t nc = nc32;
    *nc_out = nc;
    lv_assign_kernel<<<dim3(grid_for(n0, 256)), dim3(256), 0, s>>>(W.assign.p, n0, L, W.cmap.p);
    LVLAUNCHED("lv_assign_kernel");
    if (!build) return SGL_OK;

    DevBuf<uint64_t> key, skey, gkey;
    DevBuf<uint32_t> val, sval;
    DevBuf<int32_t> head, gidx;
    DevBuf<int64_t> gstart;
    const size_t m = (size_t)std::max<int64_t>(nnz, 1);
    SGLCHK(key.alloc(m)); SGLCHK(skey.alloc(m)); SGLCHK(val.alloc(m)); SGLCHK(sval.alloc(m));
    SGLCHK(head.alloc(m + 1)); SGLCHK(gidx.alloc(m + 1));
    lv_edge_keys_kernel<<<dim3(grid_for(n, 4)), dim3(256), 0, s>>>(G.p, G.i, L, W.cmap.p, n, key.p, val.p);
    LVLAUNCHED("lv_edge_keys_kernel");
    const int bits = 32 + bits_for(nc);
    SGLCHK(cub_run([&](void* tmp, size_t& bytes) {   // stable: equal keys keep the order of e, which is column-major
        return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, key.p, skey.p, val.p, sval.p, (int)nnz, 0, bits, s);
    }, "sort of the entries by community pair"));
    lv_heads_kernel<<<dim3(grid_for(nnz + 1, 256)), dim3(256), 0, s>>>(skey.p, nnz, head.p);
    LVLAUNCHED("lv_heads_kernel");
    SGLCHK(cub_run([&](void* tmp, size_t& bytes) {
        return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, head.p, gidx.p, (int)(nnz + 1), s);
    }, "scan of the coarse entries"));
    int32_t ng32 = 0;
    SGLCHK(fetch(s, &ng32, gidx.p + nnz, 1, "download of the coarse entry count"));
    const int64_t ng = ng32;
    SGLCHK(gstart.alloc((size_t)ng + 1));
    SGLCHK(gkey.alloc((size_t)std::max<int64_t>(ng, 1)));
    SGLCHK(out.p.alloc((size_t)nc + 1));
    SGLCHK(out.i.alloc((size_t)std::max<int64_t>(ng, 1)));
    SGLCHK(out.x.alloc((size_t)std::max<int64_t>(ng, 1)));
    lv_group_start_kernel<<<dim3(grid_for(nnz, 256)), dim3(256), 0, s>>>(skey.p, gidx.p, nnz, ng, gstart.p, gkey.p);
    LVLAUNCHED("lv_group_start_kernel");
    lv_group_sum_kernel<<<dim3(grid_for(ng, 4)), dim3(256), 0, s>>>(gstart.p, gkey.p, sval.p, G.x, ng, out.i.p, out.x.p);
    LVLAUNCHED("lv_group_sum_kernel");
    lv_coarse_p_kernel<<<dim3(grid_for(nc + 1, 256)), dim3(256), 0, s>>>(gkey.p, ng, nc, out.p.p);
    LVLAUNCHED("lv_coarse_p_kernel");
    out.n = nc;
    out.nnz = ng;
    cp_host.resize((size_t)nc + 1);
    return fetch(s, cp_host.data(), out.p.p, (size_t)nc + 1, "download of the coarse column pointers");
}

const char* defect_text(LouvainDefect d) {
    switch (d) {
        case LOUVAIN_ROW_RANGE: return "row index outside [0, n)";
        case LOUVAIN_ROW_ORDER: return "row indices not strictly ascending within the column";
        case LOUVAIN_NOT_FINITE: return "weight is not finite";
        case LOUVAIN_NEGATIVE: return "weight is negative";
        case LOUVAIN_ASYMMETRIC: return "the graph is not symmetric (A_ij and A_ji must both be stored, with the same bits)";
        default: return "defect";
    }
}

// Arguments, upload, the device validation.  symmetric: also the symmetry pass (sgl_c_louvain; the stage operator takes
// coarse graphs, which need not be symmetric).  On SGL_OK with n > 0 the graph is on the device and W holds k and S.
int lv_open(const char* who, hipStream_t s, const double* x, const int32_t* i, const int32_t* p, int64_t n, bool symmetric,
            OwnedGraph& G0, Work& W, double* S_host) {
    std::vector<int64_t> hp((size_t)n + 1);
    for (int64_t c = 0; c <= n; ++c) hp[(size_t)c] = p[c];
    const int64_t nnz = hp[(size_t)n];
    SGLCHK(upload(s, G0.p, hp.data(), hp.size(), "upload of G@p"));
    SGLCHK(upload(s, G0.i, i, (size_t)nnz, "upload of G@i"));
    SGLCHK(upload(s, G0.x, x, (size_t)nnz, "upload of G@x"));
    G0.n = n;
    G0.nnz = nnz;
    SGLCHK(W.alloc(n));
    for (int pass = 0; pass < (symmetric ? 2 : 1); ++pass) {
        LVCHK(hipMemsetAsync(W.moved.p, 0xff, sizeof(unsigned long long), s), "hipMemsetAsync");
        if (pass == 0) lv_validate_kernel<0><<<dim3(grid_for(n, 4)), dim3(256), 0, s>>>(G0.p.p, G0.i.p, G0.x.p, n, W.moved.p);
        else lv_validate_kernel<1><<<dim3(grid_for(n, 4)), dim3(256), 0, s>>>(G0.p.p, G0.i.p, G0.x.p, n, W.moved.p);
        LVLAUNCHED("lv_validate_kernel");
        unsigned long long first = 0;
        SGLCHK(fetch(s, &first, W.moved.p, 1, "download of the validation result"));
        if (first != ~0ull) {
            const int64_t e = (int64_t)first, c = louvain_column_of(p, n, e);
            const LouvainDefect d = louvain_entry_defect(p, i, x, n, c, e, pass == 1);
            sgl_set_error("%s: invalid graph at column %lld, row %lld: %s", who, (long long)c, (long long)i[e], defect_text(d));
            return SGL_EINVAL;
        }
    }
    lv_iota_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(W.iota.p, n);
    LVLAUNCHED("lv_iota_kernel");
    SGLCHK(lv_degrees(s, G0.view(), W, S_host));
    if (!(*S_host > 0.0) || !(*S_host < INFINITY)) {
        sgl_set_error(*S_host > 0.0 ? "%s: the sum of the weights overflows" : "%s: the graph has no weight (S = 0): nothing to cluster", who);
        return SGL_EINVAL;
    }
    return SGL_OK;
}

int lv_refuse_args(const char* who, LouvainArgError err, int64_t pos) {
    switch (err) {
        case LOUVAIN_ARGS_OK: return SGL_OK;
        case LOUVAIN_ARGS_N: sgl_set_error("%s: n is negative", who); break;
        case LOUVAIN_ARGS_NULL: sgl_set_error("%s: bad arguments (a NULL array of the graph)", who); break;
        case LOUVAIN_ARGS_P0: sgl_set_error("%s: invalid column pointer array (p[0] is not 0)", who); break;
        case LOUVAIN_ARGS_P_DECREASES: sgl_set_error("%s: invalid column pointer array: p decreases at column %lld", who, (long long)pos); break;
        case LOUVAIN_ARGS_NRES: sgl_set_error("%s: at least one resolution is needed", who); break;
        case LOUVAIN_ARGS_RESOLUTION: sgl_set_error("%s: resolution %lld must be finite and > 0", who, (long long)pos); break;
        case LOUVAIN_ARGS_TOL: sgl_set_error("%s: tol must be >= 0", who); break;
        case LOUVAIN_ARGS_SWEEPS: sgl_set_error("%s: max_sweeps must lie in [1, %d]", who, LOUVAIN_MAX_SWEEPS); break;
        case LOUVAIN_ARGS_LEVELS: sgl_set_error("%s: max_levels must lie in [1, %d]", who, LOUVAIN_MAX_LEVELS); break;
    }
    return SGL_EINVAL;
}

// All levels for one resolution on the validated level-0 graph.
int lv_run(hipStream_t s, const OwnedGraph& G0, const int32_t* p0_host, Work& W, double gamma, double tol, int32_t max_sweeps,
           int32_t max_levels, int32_t* labels, int32_t* n_clusters, int32_t* n_levels, double* q_levels, int32_t* sweeps_levels) {
    const int64_t n0 = G0.n;
    OwnedGraph C;          // the current coarse graph (levels >= 1)
    Graph G = G0.view();
    std::vector<int64_t> cp_host;
    LVCHK(hipMemcpyAsync(W.assign.p, W.iota.p, sizeof(int32_t) * (size_t)n0, hipMemcpyDeviceToDevice, s), "copy");
    int32_t levels = 0;
    for (int32_t level = 0; level < max_levels; ++level) {
        double S = 0.0, Q = 0.0;
        SGLCHK(lv_degrees(s, G, W, &S));
        if (level == 0) SGLCHK(lv_split(s, p0_host, G.n, W)); else SGLCHK(lv_split(s, cp_host.data(), G.n, W));
        (level == 0 ? g_info[1] : g_info[2]) += (int64_t)W.slow.size();
        int32_t *L = W.La.p, *Lnew = W.Lb.p;
        double *tot = W.tot.p, *tot2 = W.tot2.p;
        int32_t *size = W.size.p, *size2 = W.size2.p;
        LVCHK(hipMemcpyAsync(L, W.iota.p, sizeof(int32_t) * (size_t)G.n, hipMemcpyDeviceToDevice, s), "copy");
        SGLCHK(lv_modularity(s, G, L, gamma, W, tot, size, &Q));
        LouvainPhase ph = louvain_phase_begin(Q, tol, max_sweeps);
        while (louvain_phase_wants_sweep(ph)) {
            int64_t moved = 0;
            double Q2 = 0.0;
            SGLCHK(lv_sweep(s, G, L, Lnew, tot, size, gamma, W, &moved));
            if (moved > 0) SGLCHK(lv_modularity(s, G, Lnew, gamma, W, tot2, size2, &Q2));
            if (louvain_phase_after_sweep(ph, moved, Q2) != LOUVAIN_DISCARD_END) {
                std::swap(L, Lnew);
                std::swap(tot, tot2);
                std::swap(size, size2);
            }
        }
        if (q_levels) q_levels[level] = ph.q;
        if (sweeps_levels) sweeps_levels[level] = ph.kept;
        levels = level + 1;
        if (ph.kept == 0) break;
        OwnedGraph N;
        int64_t nc = 0;
        const bool build = level + 1 < max_levels;
        SGLCHK(lv_aggregate(s, G, L, W, n0, build, N, &nc, cp_host));
        if (build) {
            g_info[3] = 1;
            C.take(N);   // N leaves with the previous coarse graph
            G = C.view();
        }
    }
    if (n_levels) *n_levels = levels;
    std::vector<int32_t> assign((size_t)n0);
    SGLCHK(fetch(s, assign.data(), W.assign.p, (size_t)n0, "download of the clusters"));
    const int64_t ncl = louvain_renumber_by_size(assign.data(), n0, assign.data());
    if (n_clusters) *n_clusters = (int32_t)ncl;
    if (labels) memcpy(labels, assign.data(), sizeof(int32_t) * (size_t)n0);
    return SGL_OK;
}

}  // namespace

extern "C" int sgl_c_louvain(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* resolutions,
                             int32_t n_res, double tol, int32_t max_sweeps, int32_t max_levels, int32_t* labels, int32_t* n_clusters,
                             int32_t* n_levels, double* q_levels, int32_t* sweeps_levels) {
    static const char* who = "c_louvain";
    int64_t pos = -1;
    SGLCHK(lv_refuse_args(who, louvain_check_args(n, Gp, Gi, Gx, n_res, resolutions, tol, max_sweeps, max_levels, &pos), pos));
    for (int32_t r = 0; r < n_res; ++r) {
        if (n_clusters) n_clusters[r] = 0;
        if (n_levels) n_levels[r] = 0;
        for (int q = 0; q < LOUVAIN_MAX_LEVELS; ++q) {
            if (q_levels) q_levels[(size_t)r * LOUVAIN_MAX_LEVELS + q] = 0.0;
            if (sweeps_levels) sweeps_levels[(size_t)r * LOUVAIN_MAX_LEVELS + q] = 0;
        }
    }
    if (n == 0) return SGL_OK;
    StreamHolder sh;
    LVCHK(hipStreamCreate(&sh.s), "hipStreamCreate");
    OwnedGraph G0;
    Work W;
    double S = 0.0;
    SGLCHK(lv_open(who, sh.s, Gx, Gi, Gp, n, true, G0, W, &S));
    g_info[1] = g_info[2] = g_info[3] = 0;
    for (int32_t r = 0; r < n_res; ++r)
        SGLCHK(lv_run(sh.s, G0, Gp, W, resolutions[r], tol, max_sweeps, max_levels, labels ? labels + (size_t)r * (size_t)n : nullptr,
                      n_clusters ? n_clusters + r : nullptr, n_levels ? n_levels + r : nullptr,
                      q_levels ? q_levels + (size_t)r * LOUVAIN_MAX_LEVELS : nullptr,
                      sweeps_levels ? sweeps_levels + (size_t)r * LOUVAIN_MAX_LEVELS : nullptr));
    return SGL_OK;
}

extern "C" int sgl_op_louvain_sweep(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const int32_t* labels_in,
                                    double resolution, int32_t* labels_out, double* q_in, double* q_out, int64_t* moved_out) {
    static const char* who = "op_louvain_sweep";
    int64_t pos = -1;
    SGLCHK(lv_refuse_args(who, louvain_check_args(n, Gp, Gi, Gx, 1, &resolution, 0.0, 1, 1, &pos), pos));
    if (q_in) *q_in = 0.0;
    if (q_out) *q_out = 0.0;
    if (moved_out) *moved_out = 0;
    if (n == 0) return SGL_OK;
    if (!labels_in) { sgl_set_error("%s: labels_in is NULL", who); return SGL_EINVAL; }
    for (int64_t v = 0; v < n; ++v)
        if (labels_in[v] < 0 || labels_in[v] >= n) {
            sgl_set_error("%s: label %d of vertex %lld lies outside [0, n)", who, labels_in[v], (long long)v);
            return SGL_EINVAL;
        }
    StreamHolder sh;
    LVCHK(hipStreamCreate(&sh.s), "hipStreamCreate");
    hipStream_t s = sh.s;
    OwnedGraph G0;
    Work W;
    double S = 0.0, Q0 = 0.0, Q1 = 0.0;
    SGLCHK(lv_open(who, s, Gx, Gi, Gp, n, false, G0, W, &S));
    const Graph G = G0.view();
    SGLCHK(lv_split(s, Gp, n, W));
    g_info[1] = (int64_t)W.slow.size();
    g_info[2] = g_info[3] = 0;
    LVCHK(hipMemcpyAsync(W.La.p, labels_in, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s), "upload of the labels");
    SGLCHK(lv_modularity(s, G, W.La.p, resolution, W, W.tot.p, W.size.p, &Q0));
    int64_t moved = 0;
    SGLCHK(lv_sweep(s, G, W.La.p, W.Lb.p, W.tot.p, W.size.p, resolution, W, &moved));
    SGLCHK(lv_modularity(s, G, W.Lb.p, resolution, W, W.tot2.p, W.size2.p, &Q1));
    if (labels_out) SGLCHK(fetch(s, labels_out, W.Lb.p, (size_t)n, "download of the labels"));
    if (q_in) *q_in = Q0;
    if (q_out) *q_out = Q1;
    if (moved_out) *moved_out = moved;
    return SGL_OK;
}

extern "C" int sgl_louvain_info(int64_t out[4]) {
    if (!out) { sgl_set_error("sgl_louvain_info: out is NULL"); return SGL_EINVAL; }
    for (int q = 0; q < 4; ++q) out[q] = g_info[q];
    return SGL_OK;
}
