// Spatial neighbour graphs of FindLocalNeighbors (R/FindLocalNeighbors.R:95-98): c_LKNN (src/singlet.cpp:1491-1603) and
// c_SNN (:1606-1665) on the GPU.  The reference checks every pair of points (c_LKNN, O(n^2) radius tests) and every pair of
// columns (c_SNN, O(n^2) serial list merges); here a spatial cell list bounds the LKNN candidates to the 3 x 3 buckets around
// a point, and SNN counts the columns that share a row of G through G's row-major pattern.
//
// LKNN arithmetic is FP32 as in the reference (Eigen::MatrixXf, float radius / max_dist), summed in dimension order, with NO
// contraction: the reference is built for x86-64 without FMA, so every distance, the radius test and the zero test are
// bit-identical to it (kl: the log is within an ulp of glibc's, so a few ulps).  tests/test_kernel_codegen_neighbors.py checks the
// emitted gfx950 code of the lknn kernels for fused multiply-adds.
//
// Where the reference is undefined, this build's rules (include/singlet_hip.h, sgl_c_lknn): candidates are ranked by
// (distance, index) -- ties at the k-th place go to the lower index, NaN distances (0/0 of all-zero embedding columns) rank
// after every number -- and a point that keeps more neighbours than the reference's n_max_edges slots per point is refused.
#include "sgl_internal.h"
#include <hipcub/hipcub.hpp>
#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------------ shared plumbing ---
namespace {

unsigned grid_for(int64_t n, int per_block) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, 65535)); }

int hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return SGL_OK;
    (void)hipGetLastError();
    sgl_set_error("%s failed: %s", what, hipGetErrorString(e));
    return SGL_EHIP;
}
#define NBCHK(expr, what) SGLCHK(hip_ok((expr), what))

// n host elements into a fresh device buffer, and n device elements back (n = 0: nothing is copied).
template <typename T>
int upload(hipStream_t s, DevBuf<T>& d, const T* h, size_t n, const char* what) {
    SGLCHK(d.alloc(n));
    if (n > 0) NBCHK(hipMemcpyAsync(d.p, h, sizeof(T) * n, hipMemcpyHostToDevice, s), what);
    return SGL_OK;
}
template <typename T>
int download(hipStream_t s, T* h, const T* d, size_t n, const char* what) {
    if (n > 0) NBCHK(hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, s), what);
    return SGL_OK;
}

// A hipcub call in its two steps: call(nullptr, bytes) asks for the size of the temporary storage, call(tmp, bytes) runs.
template <typename F>
int cub_run(F call, const char* what) {
    size_t bytes = 0;
    NBCHK(call(nullptr, bytes), what);
    DevBuf<char> tmp;
    SGLCHK(tmp.alloc(bytes));
    NBCHK(call(tmp.p, bytes), what);
    return SGL_OK;
}

// Work lists of LKNN (sorted positions) and SNN (columns): the items of length 1 .. cap sort in LDS, one 64-lane workgroup
// each (fast); the longer ones go through HBM (slow); those of length 0 have no work.  Both lists on the host and the device.
struct WorkLists {
    std::vector<int32_t> fast, slow;
    DevBuf<int32_t> dfast, dslow;
};
int split_work(hipStream_t s, const std::vector<int64_t>& len, int64_t cap, WorkLists& w) {
    for (size_t e = 0; e < len.size(); ++e)
        if (len[e] > 0) (len[e] <= cap ? w.fast : w.slow).push_back((int32_t)e);
    SGLCHK(upload(s, w.dfast, w.fast.data(), w.fast.size(), "upload"));
    return upload(s, w.dslow, w.slow.data(), w.slow.size(), "upload");
}

// In-LDS bitonic sort of s[0, P) ascending, P a power of two; one 64-lane workgroup.
template <typename K>
__device__ __forceinline__ void bitonic_lds(K* s, int P) {
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < P; t += 64) {
                const int u = t ^ stride;
                if (u > t) {
                    const K x = s[t], y = s[u];
                    const bool up = (t & size) == 0;
                    if ((x > y) == up) { s[t] = y; s[u] = x; }
                }
            }
            __syncthreads();
        }
}

// The sum of v over the workgroup, to every thread; *acc is an LDS word of the caller, free again on return.
__device__ __forceinline__ int block_sum(int* acc, int v) {
    if (threadIdx.x == 0) *acc = 0;
    __syncthreads();
    atomicAdd(acc, v);
    __syncthreads();
    const int sum = *acc;
    __syncthreads();
    return sum;
}

// ---- the spatial cell list of LKNN (float coordinates, reach = radius) and spatial_graph (double, reach = max_dist).
// Points are keyed by their bucket by * W + bx of a W x H grid of square buckets, b = floor((c - cmin) / side) in double, and
// sorted by key (stable: a bucket's members stay in ascending index order).  Every pair of points that passes the operator's
// distance test lies in adjacent buckets, so the candidates of a point are the 3 x 3 buckets around it: three runs of sorted
// positions, one per bucket row.
//
// Why the prefilter is conservative.  Let the test be d = fl(sqrt(fl(fl(dx*dx) + fl(dy*dy)))) <= r (spatial_graph: < r) with
// dx = fl(x1 - x2), in a format of p significand bits whose smallest normal number is 2^e, without contraction.  If
// |dx| < 2^(e/2), then |x1 - x2| < 2^(e/2 + 1) (a difference that rounds below 2^(e/2) is below it too, or subnormal and exact).
// Otherwise dx*dx >= 2^e is normal, so fl(dx*dx) >= dx^2 (1 - 2^-p); adding a non-negative fl(dy*dy) and taking the rounded
// root are monotone, each losing at most a factor (1 - 2^-p), so |dx| <= d (1 + 2^(2-p)) and |x1 - x2| <= |dx| (1 + 2^(1-p)) <=
// r (1 + 2^(3-p)).  Either way |x1 - x2| <= R = max(r, 2^(e/2 + 1)) (1 + 2^(3-p)), and the same holds for y.  Buckets have side
// s >= max(r, 2^(e/2 + 1)) (1 + 2^-10), so |x1 - x2| / s < 1 - 2^-11.  The bucket coordinate u = fl(fl(x - xmin) / s) in double is
// off by at most 2^-52 u <= 2^-21, since s is also raised so that u <= 2^30; so |u1 - u2| < 1 and floor(u1), floor(u2) differ by
// at most one.  The test itself is then evaluated exactly as the reference does, underflow of dx*dx included.
//   float  (LKNN):          p = 24, e = -126:  factor 1 + 2^-21, reach floor 2^-62  (radius 0: buckets of side ~2^-62, exact
//                           coordinates up to the underflow of dx*dx that the reference's test also lets through)
//   double (spatial_graph): p = 53, e = -1022: factor 1 + 2^-50, reach floor 2^-510; here the quotient (x - xmin) / s can be
//                           subnormal, which adds 2^-1074 to u's error: still <= 2^-21
// Both factors sit inside the side's 1 + 2^-10.
struct CellGrid {
    double xmin, ymin, side;
    int64_t W, H;
};

// The grid over the extent [xmin, xmax] x [ymin, ymax] for a reach and its floor; an extent that overflows double is one
// bucket (every pair is a candidate).
CellGrid cell_grid(double xmin, double xmax, double ymin, double ymax, double reach, double reach_floor) {
    CellGrid g{xmin, ymin, INFINITY, 1, 1};
    const double ext = std::max(xmax - xmin, ymax - ymin);
    if (ext < INFINITY) {
        g.side = std::max(std::max(reach, reach_floor) * (1.0 + ldexp(1.0, -10)), ext * ldexp(1.0, -30));
        g.W = (int64_t)floor((xmax - xmin) / g.side) + 2;
        g.H = (int64_t)floor((ymax - ymin) / g.side) + 2;
    }
    return g;
}

template <typename T>
__global__ void cell_keys_kernel(const T* __restrict__ cx, const T* __restrict__ cy, int64_t n, CellGrid g, uint64_t* __restrict__ keys,
                                 uint32_t* __restrict__ iota) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t bx = 0, by = 0;
        if (g.W > 1) {   // cell_grid's W, H hold every point: the clamps never bind
            bx = std::min<int64_t>((int64_t)floor(((double)cx[e] - g.xmin) / g.side), g.W - 1);
            by = std::min<int64_t>((int64_t)floor(((double)cy[e] - g.ymin) / g.side), g.H - 1);
        }
        keys[e] = (uint64_t)(by * g.W + bx);
        iota[e] = (uint32_t)e;
    }
}

// The boundary table: bnd[12 pos + 4 q + r] = the sorted position where bucket bx - 1 + r of row by - 1 + q starts (r = 0 .. 3,
// q = 0 .. 2; a row outside the grid: 0), for the bucket (bx, by) of sorted position pos.  So [bnd[4 q + r], bnd[4 q + r + 1]) is
// one of the nine buckets and [bnd[4 q], bnd[4 q + 3]) the run of row q.  ncand, unless null: the three runs' total.
__global__ void cell_bounds_kernel(const uint64_t* __restrict__ skeys, int64_t n, int64_t W, int64_t H, int32_t* __restrict__ bnd,
                                   int64_t* __restrict__ ncand) {
    for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < n; pos += (int64_t)gridDim.x * blockDim.x) {
        const int64_t key = (int64_t)skeys[pos], by = key / W, bx = key % W;
        int64_t tot = 0;
        for (int q = 0; q < 3; ++q) {
            const int64_t yy = by - 1 + q;
            int64_t b[4] = {0, 0, 0, 0};
            for (int r = 0; r < 4; ++r) {
                if (yy >= 0 && yy < H) {   // the first sorted position whose key is not below the bucket's
                    const uint64_t v = (uint64_t)(yy * W + std::min<int64_t>(std::max<int64_t>(bx - 1 + r, 0), W));
                    int64_t lo = 0, hi = n;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (skeys[mid] < v) lo = mid + 1;
                        else hi = mid;
                    }
                    b[r] = lo;
                }
                bnd[pos * 12 + q * 4 + r] = (int32_t)b[r];
            }
            tot += b[3] - b[0];
        }
        if (ncand) ncand[pos] = tot;
    }
}

struct CellList {
    DevBuf<uint32_t> sidx;   // point at each sorted position
    DevBuf<int32_t> bnd;     // the boundary table, 12 per sorted position
};

// The cell list of n > 0 device-resident points on grid g; ncand (device, n entries) may be null.
template <typename T>
int cell_list_build(hipStream_t s, const T* cx, const T* cy, int64_t n, const CellGrid& g, CellList& cl, int64_t* ncand) {
    DevBuf<uint64_t> keys, skeys;
    DevBuf<uint32_t> iota;
    SGLCHK(keys.alloc((size_t)n));
    SGLCHK(skeys.alloc((size_t)n));
    SGLCHK(iota.alloc((size_t)n));
    SGLCHK(cl.sidx.alloc((size_t)n));
    SGLCHK(cl.bnd.alloc((size_t)n * 12));
    cell_keys_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(cx, cy, n, g, keys.p, iota.p);
    NBCHK(hipGetLastError(), "cell_keys_kernel");
    int end_bit = 1;
    while (end_bit < 64 && ((uint64_t)1 << end_bit) <= (uint64_t)(g.W * g.H)) ++end_bit;
    SGLCHK(cub_run([&](void* tmp, size_t& bytes) {   // LSD radix sort is stable
        return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys.p, skeys.p, iota.p, cl.sidx.p, (int)n, 0, end_bit, s);
    }, "radix sort"));
    cell_bounds_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(skeys.p, n, g.W, g.H, cl.bnd.p, ncand);
    NBCHK(hipGetLastError(), "cell_bounds_kernel");
    return SGL_OK;
}

// ---- the two-call CSC tail of the three entries (api._two_call makes the two calls).
// Host counts per column -> p_out and *nnz_out; a graph of more than 2^31 - 1 entries is refused with too_many (one %lld).
template <typename C>
int csc_pointers(const std::vector<C>& cnt, const char* too_many, int32_t* p_out, int64_t* nnz_out) {
    int64_t nnz = 0;
    for (const C c : cnt) nnz += c;
    if (nnz > INT32_MAX) { sgl_set_error(too_many, (long long)nnz); return SGL_EINVAL; }
    p_out[0] = 0;
    for (size_t c = 0; c < cnt.size(); ++c) p_out[c + 1] = p_out[c] + (int32_t)cnt[c];
    *nnz_out = nnz;
    return SGL_OK;
}
// After csc_pointers: the count-only call (no i_out) ends here, and a capacity below nnz is refused with too_small (two
// %lld) -- p_out and *nnz_out stay filled, the caller sizes its arrays by them.  Else fill(off, oi, ox) enqueues the
// operator's kernels that write rows and values at the column offsets off (device, of type OFF), and both come back.
template <typename OFF, typename F>
int csc_fill(hipStream_t s, int64_t n, const int32_t* p_out, int64_t nnz, int64_t cap, const char* too_small, int32_t* i_out, double* x_out,
             F fill) {
    if (!i_out) return SGL_OK;
    if (cap < nnz) { sgl_set_error(too_small, (long long)cap, (long long)nnz); return SGL_EINVAL; }
    const std::vector<OFF> off(p_out, p_out + n + 1);
    DevBuf<OFF> doff;
    DevBuf<int32_t> oi;
    DevBuf<double> ox;
    SGLCHK(upload(s, doff, off.data(), off.size(), "upload of p"));
    SGLCHK(oi.alloc((size_t)nnz));
    SGLCHK(ox.alloc((size_t)nnz));
    SGLCHK(fill(doff.p, oi.p, ox.p));
    SGLCHK(download(s, i_out, oi.p, (size_t)nnz, "download of i"));
    SGLCHK(download(s, x_out, ox.p, (size_t)nnz, "download of x"));
    NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    return SGL_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- LKNN ---
namespace {

enum { NB_EUCLIDEAN = 0, NB_JACCARD, NB_COSINE, NB_MANHATTAN, NB_HAMMING, NB_KL };

constexpr int LKNN_CAP = 512;    // candidates a point sorts in LDS (one 64-lane workgroup, 4 KB); above: segmented sort in HBM
constexpr uint64_t NO_KEY = ~0ull;

// Order-preserving 32-bit key of a distance: -0 is +0 (they tie and are both dropped), every NaN is one value above +inf.
// key_dist returns that NaN as x86's default NaN (0xffc00000, sign set), the one the reference's 0/0 gives.
__device__ __forceinline__ uint32_t dist_key(float d) {
    uint32_t u = __float_as_uint(d);
    if (d != d) u = 0x7fc00000u;
    else if (d == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_dist(uint32_t k) {
    if (k == (0x7fc00000u | 0x80000000u)) return __uint_as_float(0xffc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Correctly rounded float root and quotient through double (53 >= 2 * 24 + 2 bits: the double rounding is innocuous), so that
// the distance kernels hold no f32 fused multiply-add at all -- not even the ones of the f32 division / root expansions --
// and the codegen test can tell a contraction from them.  logf likewise goes through the double log.  The empty asm keeps
// the compiler from folding the widened operation back to f32 (which it may: the results are the same).
__device__ __forceinline__ double widen(float x) {
    double d = (double)x;
    asm volatile("" : "+v"(d));
    return d;
}
__device__ __forceinline__ float sqrt_rn(float x) { return (float)__builtin_sqrt(widen(x)); }
__device__ __forceinline__ float div_rn(float a, float b) { return (float)(widen(a) / widen(b)); }
__device__ __forceinline__ float log_f(float x) { return (float)log(widen(x)); }

// The six distance functions of src/singlet.cpp:1426-1478, in float, in dimension order (p = the point, q = the candidate).
template <int MET>
__device__ __forceinline__ float nb_distance(const float* __restrict__ p, const float* __restrict__ q, int D, int similarity) {
    if (MET == NB_JACCARD || MET == NB_COSINE) {
        float pq = 0.0f, pp = 0.0f, qq = 0.0f;
        for (int d = 0; d < D; ++d) {
            const float a = p[d], b = q[d];
            pq += a * b;
            pp += a * a;
            qq += b * b;
        }
        float r = (MET == NB_JACCARD) ? 1.0f - div_rn(pq, pp + qq - pq) : 1.0f - div_rn(pq, sqrt_rn(pp) * sqrt_rn(qq));
        if (!similarity) r = 1.0f - r;
        return r;
    } else if (MET == NB_MANHATTAN) {
        float s = 0.0f;
        for (int d = 0; d < D; ++d) s += __builtin_fabsf(p[d] - q[d]);
        return sqrt_rn(s);   // sic: the reference takes the root of the L1 sum
    } else if (MET == NB_HAMMING) {
        float s = 0.0f;
        for (int d = 0; d < D; ++d)
            if (p[d] != q[d]) s += 1.0f;
        return s;
    } else if (MET == NB_KL) {
        float pdivq = 0.0f, psum = 0.0f;
        for (int d = 0; d < D; ++d) {
            if (q[d] != 0.0f) pdivq += div_rn(p[d], q[d]);
            psum += p[d];
        }
        return psum * log_f(pdivq);
    } else {
        float s = 0.0f;
        for (int d = 0; d < D; ++d) {
            const float t = p[d] - q[d];
            s += t * t;
        }
        return sqrt_rn(s);
    }
}

struct LknnArgs {
    const float* m;          // D x n, column-major
    int D;
    const float* cx;
    const float* cy;
    float radius, max_dist;
    int similarity;
    const uint32_t* sidx;    // point at each sorted position
    const int32_t* bnd;      // the cell list's boundary table: run q of a position's candidates is [bnd[4 q], bnd[4 q + 3])
    int64_t k;
};

// The candidate c (0 <= c < C) of the point at sorted position pos -> its sort key (distance key << 32 | index), or NO_KEY when
// it is the point itself, outside the radius (the reference's exact test, :1520-1523) or pruned by max_dist (:1541).
template <int MET>
__device__ __forceinline__ uint64_t lknn_candidate(const LknnArgs& a, int64_t pos, uint32_t pt, int c) {
    const int32_t* r = a.bnd + pos * 12;
    int32_t sp;
    const int32_t l0 = r[3] - r[0], l1 = r[7] - r[4];
    if (c < l0) sp = r[0] + c;
    else if (c < l0 + l1) sp = r[4] + (c - l0);
    else sp = r[8] + (c - l0 - l1);
    const uint32_t j = a.sidx[sp];
    if (j == pt) return NO_KEY;
    const float dx = a.cx[pt] - a.cx[j], dy = a.cy[pt] - a.cy[j];
    const float d = sqrt_rn(dx * dx + dy * dy);
    if (!(d <= a.radius)) return NO_KEY;
    const float d12 = nb_distance<MET>(a.m + (size_t)pt * a.D, a.m + (size_t)j * a.D, a.D, a.similarity);
    if (a.max_dist != 0.0f && d12 > a.max_dist) return NO_KEY;
    return ((uint64_t)dist_key(d12) << 32) | j;
}

// The kk kept neighbours of a point, as sorted index-major keys (index << 32 | distance key), to its staging slots
// [o, o + kk), zeros included; the calling thread handles every stride-th one and returns how many of its are non-zero.
__device__ __forceinline__ int lknn_write_kept(const uint64_t* keys, int kk, int stride, int64_t o, int32_t* __restrict__ ti,
                                               float* __restrict__ tx) {
    int nz = 0;
    for (int c = threadIdx.x; c < kk; c += stride) {
        const uint64_t v = keys[c];
        const float d = key_dist((uint32_t)v);
        ti[o + c] = (int32_t)(v >> 32);
        tx[o + c] = d;
        nz += d != 0.0f;
    }
    return nz;
}

// Points whose 3 x 3 buckets hold at most LKNN_CAP candidates, one 64-lane workgroup each, in spatial (sorted) order so that
// neighbouring workgroups gather the same embedding columns.  Keeps the k smallest (distance, index), re-sorts them by index,
// and writes them (zeros included) to the point's slots [toff[pt], toff[pt] + kept) of the staging list.
template <int MET>
__global__ __launch_bounds__(64) void lknn_fast_kernel(LknnArgs a, const int32_t* __restrict__ work, int64_t nwork,
                                                       const int64_t* __restrict__ toff, int32_t* __restrict__ ti,
                                                       float* __restrict__ tx, int32_t* __restrict__ kept,
                                                       int32_t* __restrict__ nzc) {
    __shared__ uint64_t s[LKNN_CAP];
    __shared__ int acc;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t pos = work[w];
        const uint32_t pt = a.sidx[pos];
        const int32_t* r = a.bnd + pos * 12;
        const int C = (r[3] - r[0]) + (r[7] - r[4]) + (r[11] - r[8]);
        int P = 64;
        while (P < C) P <<= 1;
        int mine = 0;
        for (int c = threadIdx.x; c < P; c += 64) {
            const uint64_t key = c < C ? lknn_candidate<MET>(a, pos, pt, c) : NO_KEY;
            mine += key != NO_KEY;
            s[c] = key;
        }
        const int kk = (int)std::min<int64_t>(a.k, (int64_t)block_sum(&acc, mine));
        bitonic_lds(s, P);
        for (int c = threadIdx.x; c < P; c += 64) {   // the kept ones, index-major
            const uint64_t v = s[c];
            s[c] = c < kk ? (((v & 0xffffffffull) << 32) | (v >> 32)) : NO_KEY;
        }
        __syncthreads();
        bitonic_lds(s, P);
        const int nz = block_sum(&acc, lknn_write_kept(s, kk, 64, toff[pt], ti, tx));
        if (threadIdx.x == 0) { kept[pt] = kk; nzc[pt] = nz; }
    }
}

// Points with more than LKNN_CAP candidates, one workgroup each: every candidate's key goes to the point's segment
// [soff[w], soff[w + 1]) of an HBM list, sorted afterwards by a segmented radix sort.
template <int MET>
__global__ __launch_bounds__(256) void lknn_slow_keys_kernel(LknnArgs a, const int32_t* __restrict__ work, int64_t nwork,
                                                            const int32_t* __restrict__ soff, uint64_t* __restrict__ keys,
                                                            int32_t* __restrict__ npass) {
    __shared__ int acc;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t pos = work[w];
        const uint32_t pt = __builtin_amdgcn_readfirstlane(a.sidx[pos]);   // (one point per workgroup)
        const int C = soff[w + 1] - soff[w];
        int mine = 0;
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            const uint64_t key = lknn_candidate<MET>(a, pos, pt, c);
            mine += key != NO_KEY;
            keys[soff[w] + c] = key;
        }
        const int n = block_sum(&acc, mine);
        if (threadIdx.x == 0) npass[w] = n;
    }
}

// After the (distance, index) sort: the kept prefix of each segment becomes index-major keys, whose segments [soff, kend) are
// sorted next.
__global__ void lknn_slow_trim_kernel(const uint64_t* __restrict__ sorted, uint64_t* __restrict__ keys2, const int32_t* __restrict__ soff,
                                      const int32_t* __restrict__ npass, int64_t nwork, int64_t k, int32_t* __restrict__ kend) {
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int kk = (int)std::min<int64_t>(k, (int64_t)npass[w]);
        for (int c = threadIdx.x; c < kk; c += blockDim.x) {
            const uint64_t v = sorted[soff[w] + c];
            keys2[soff[w] + c] = ((v & 0xffffffffull) << 32) | (v >> 32);
        }
        if (threadIdx.x == 0) kend[w] = soff[w] + kk;
    }
}

__global__ void lknn_slow_write_kernel(const uint64_t* __restrict__ sorted2, const int32_t* __restrict__ soff,
                                       const int32_t* __restrict__ kend, const int32_t* __restrict__ work, int64_t nwork,
                                       const uint32_t* __restrict__ sidx, const int64_t* __restrict__ toff,
                                       int32_t* __restrict__ ti, float* __restrict__ tx, int32_t* __restrict__ kept,
                                       int32_t* __restrict__ nzc) {
    __shared__ int acc;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const uint32_t pt = __builtin_amdgcn_readfirstlane(sidx[work[w]]);
        const int kk = kend[w] - soff[w];
        const int nz = block_sum(&acc, lknn_write_kept(sorted2 + soff[w], kk, blockDim.x, toff[pt], ti, tx));
        if (threadIdx.x == 0) { kept[pt] = kk; nzc[pt] = nz; }
    }
}

// m (m_rows x m_cols, column-major doubles) -> D x n floats, column-major, rounded to nearest once; flag = 1 on NaN / Inf.
__global__ void lknn_to_float_kernel(const double* __restrict__ m, int64_t m_rows, int transpose, int64_t D, int64_t n,
                                     float* __restrict__ out, int* __restrict__ flag) {
    int bad = 0;
    const int64_t tot = D * n;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = e % D, pt = e / D;
        const double v = transpose ? m[pt + d * m_rows] : m[e];
        if (!(__builtin_fabs(v) < __builtin_inf())) bad = 1;
        out[e] = (float)v;
    }
    if (bad) atomicOr(flag, 1);
}

// Drop the zeros (:1572-1588) and widen to double: point pt's staged entries -> its output column at off[pt].
__global__ void lknn_compact_kernel(const int64_t* __restrict__ toff, const int32_t* __restrict__ kept, const int64_t* __restrict__ off,
                                    const int32_t* __restrict__ ti, const float* __restrict__ tx, int64_t n,
                                    int32_t* __restrict__ oi, double* __restrict__ ox) {
    for (int64_t pt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pt < n; pt += (int64_t)gridDim.x * blockDim.x) {
        int64_t o = off[pt];
        const int64_t t0 = toff[pt], t1 = t0 + kept[pt];
        for (int64_t t = t0; t < t1; ++t)
            if (tx[t] != 0.0f) { oi[o] = ti[t]; ox[o] = (double)tx[t]; ++o; }
    }
}

template <int MET>
int lknn_launch_fast(hipStream_t s, const LknnArgs& a, const int32_t* work, int64_t nwork, const int64_t* toff, int32_t* ti, float* tx,
                     int32_t* kept, int32_t* nzc) {
    if (nwork > 0) lknn_fast_kernel<MET><<<dim3(grid_for(nwork, 1)), dim3(64), 0, s>>>(a, work, nwork, toff, ti, tx, kept, nzc);
    return hip_ok(hipGetLastError(), "lknn_fast_kernel");
}
template <int MET>
int lknn_launch_slow_keys(hipStream_t s, const LknnArgs& a, const int32_t* work, int64_t nwork, const int32_t* soff, uint64_t* keys,
                          int32_t* npass) {
    lknn_slow_keys_kernel<MET><<<dim3(grid_for(nwork, 1)), dim3(256), 0, s>>>(a, work, nwork, soff, keys, npass);
    return hip_ok(hipGetLastError(), "lknn_slow_keys_kernel");
}

#define NB_DISPATCH(met, fn, ...)                                   \
    ((met) == NB_JACCARD     ? fn<NB_JACCARD>(__VA_ARGS__)          \
     : (met) == NB_COSINE    ? fn<NB_COSINE>(__VA_ARGS__)           \
     : (met) == NB_MANHATTAN ? fn<NB_MANHATTAN>(__VA_ARGS__)        \
     : (met) == NB_HAMMING   ? fn<NB_HAMMING>(__VA_ARGS__)          \
     : (met) == NB_KL        ? fn<NB_KL>(__VA_ARGS__)               \
                             : fn<NB_EUCLIDEAN>(__VA_ARGS__))

}  // namespace

extern "C" int sgl_c_lknn(const double* m, int32_t m_rows, int32_t m_cols, const double* coord_x, const double* coord_y,
                          int32_t n_coords, int64_t k, double radius_d, const char* metric, int similarity, double max_dist_d,
                          int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap) {
    // --- arguments, in the reference's order (:1492-1494)
    if (!p_out || !nnz_out || (!m && (int64_t)m_rows * m_cols > 0) || (n_coords > 0 && (!coord_x || !coord_y)) || !metric ||
        m_rows < 0 || m_cols < 0 || n_coords < 0) {
        sgl_set_error("sgl_c_lknn: bad arguments");
        return SGL_EINVAL;
    }
    if ((i_out == nullptr) != (x_out == nullptr)) { sgl_set_error("sgl_c_lknn: i_out and x_out go together"); return SGL_EINVAL; }
    const int64_t n = n_coords;
    const bool transpose = m_cols != m_rows && m_rows == n;
    const int64_t D = transpose ? m_cols : m_rows, mcols = transpose ? m_rows : m_cols;
    if (mcols != n) { sgl_set_error("number of columns in 'm' must be equal to number of coordinates"); return SGL_EINVAL; }
    if (k < 0) { sgl_set_error("sgl_c_lknn: k = %lld is negative", (long long)k); return SGL_EINVAL; }
    const float radius = (float)radius_d, max_dist = (float)max_dist_d;
    if (!(radius >= 0.0f) || !(radius < INFINITY)) {
        sgl_set_error("c_LKNN: radius %g must be finite and non-negative", radius_d);
        return SGL_EINVAL;
    }
    if (max_dist != max_dist) { sgl_set_error("c_LKNN: max_dist is NaN"); return SGL_EINVAL; }
    std::vector<float> cx((size_t)n), cy((size_t)n);
    double xmin = 0, xmax = 0, ymin = 0, ymax = 0;
    for (int64_t e = 0; e < n; ++e) {
        cx[e] = (float)coord_x[e];
        cy[e] = (float)coord_y[e];
        if (!(fabsf(cx[e]) < INFINITY) || !(fabsf(cy[e]) < INFINITY)) {
            sgl_set_error("c_LKNN: coordinate %lld is not finite (as float)", (long long)e);
            return SGL_EINVAL;
        }
        if (e == 0 || cx[e] < xmin) xmin = cx[e];
        if (e == 0 || cx[e] > xmax) xmax = cx[e];
        if (e == 0 || cy[e] < ymin) ymin = cy[e];
        if (e == 0 || cy[e] > ymax) ymax = cy[e];
    }
    int met = NB_EUCLIDEAN;   // an unknown name is euclidean (:1539-1540)
    if (!strcmp(metric, "jaccard")) met = NB_JACCARD;
    else if (!strcmp(metric, "cosine")) met = NB_COSINE;
    else if (!strcmp(metric, "manhattan")) met = NB_MANHATTAN;
    else if (!strcmp(metric, "hamming")) met = NB_HAMMING;
    else if (!strcmp(metric, "kl")) met = NB_KL;
    // slots per point of the reference (:1496): ceil(pow(radius * 2 + 1, 2)) - 1, the base in float, the power in double
    const float base = radius * 2.0f + 1.0f;
    const double n_max_edges = ceil((double)base * (double)base) - 1.0;

    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    hipStream_t s = hd.c->stream;
    if (n == 0) {
        p_out[0] = 0;
        *nnz_out = 0;
        return SGL_OK;
    }

    // --- embedding as float, D x n
    DevBuf<double> dm;
    DevBuf<float> mf, dcx, dcy;
    DevBuf<int> flag;
    SGLCHK(mf.alloc((size_t)(D * n)));
    SGLCHK(flag.alloc(1));
    NBCHK(hipMemsetAsync(flag.p, 0, sizeof(int), s), "hipMemsetAsync");
    SGLCHK(upload(s, dm, m, (size_t)(D * n), "upload of m"));
    if (D > 0) {
        lknn_to_float_kernel<<<dim3(grid_for(D * n, 256)), dim3(256), 0, s>>>(dm.p, m_rows, transpose ? 1 : 0, D, n, mf.p, flag.p);
        NBCHK(hipGetLastError(), "lknn_to_float_kernel");
    }
    SGLCHK(upload(s, dcx, cx.data(), (size_t)n, "upload of coord_x"));
    SGLCHK(upload(s, dcy, cy.data(), (size_t)n, "upload of coord_y"));
    int hflag = 0;
    SGLCHK(download(s, &hflag, flag.p, 1, "download of the flag"));
    NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (hflag) { sgl_set_error("c_LKNN: 'm' holds a NaN or infinite value (or one that overflows float)"); return SGL_EINVAL; }
    { DevBuf<double> tmp; std::swap(tmp.p, dm.p); }   // the double copy is done with

    // --- spatial cell list, the candidates of every sorted position
    CellList cl;
    DevBuf<int64_t> dC;
    SGLCHK(dC.alloc((size_t)n));
    SGLCHK(cell_list_build(s, dcx.p, dcy.p, n, cell_grid(xmin, xmax, ymin, ymax, radius, ldexp(1.0, -62)), cl, dC.p));
    std::vector<int64_t> C((size_t)n);
    std::vector<uint32_t> hsidx((size_t)n);
    SGLCHK(download(s, C.data(), dC.p, (size_t)n, "download of the candidate counts"));
    SGLCHK(download(s, hsidx.data(), cl.sidx.p, (size_t)n, "download of the order"));
    NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");

    // --- staging slots: min(k, candidates) per point, in point order; work lists in sorted (spatial) order
    std::vector<int64_t> toff((size_t)n + 1);
    toff[0] = 0;
    {
        std::vector<int64_t> room((size_t)n);
        for (int64_t pos = 0; pos < n; ++pos) room[hsidx[pos]] = std::min<int64_t>(k, C[pos]);
        for (int64_t pt = 0; pt < n; ++pt) toff[pt + 1] = toff[pt] + room[pt];
    }
    const int64_t staged = toff[n];
    WorkLists wl;   // (every position has a candidate: the point itself)
    DevBuf<int64_t> dtoff;
    DevBuf<int32_t> ti, kept, nzc;
    DevBuf<float> tx;
    SGLCHK(split_work(s, C, LKNN_CAP, wl));
    SGLCHK(upload(s, dtoff, toff.data(), toff.size(), "upload"));
    SGLCHK(ti.alloc((size_t)staged));
    SGLCHK(tx.alloc((size_t)staged));
    SGLCHK(kept.alloc((size_t)n));
    SGLCHK(nzc.alloc((size_t)n));
    const std::vector<int32_t>& slow = wl.slow;
    LknnArgs a{mf.p, (int)D, dcx.p, dcy.p, radius, max_dist, similarity ? 1 : 0, cl.sidx.p, cl.bnd.p, k};
    SGLCHK(NB_DISPATCH(met, lknn_launch_fast, s, a, wl.dfast.p, (int64_t)wl.fast.size(), dtoff.p, ti.p, tx.p, kept.p, nzc.p));

    // --- points with more than LKNN_CAP candidates: segmented sorts in HBM, in batches of at most 2^27 candidates
    const int64_t BATCH = (int64_t)1 << 27;
    for (size_t b0 = 0; b0 < slow.size();) {
        size_t b1 = b0;
        int64_t tot = 0;
        while (b1 < slow.size() && (b1 == b0 || tot + C[slow[b1]] <= BATCH)) tot += C[slow[b1++]];
        if (tot >= INT32_MAX) { sgl_set_error("c_LKNN: one point has %lld candidates in its 3 x 3 buckets (limit 2^31)", (long long)tot); return SGL_EINVAL; }
        const int64_t nw = (int64_t)(b1 - b0);
        const int32_t* dwork = wl.dslow.p + b0;
        std::vector<int32_t> hsoff((size_t)nw + 1);
        hsoff[0] = 0;
        for (int64_t w = 0; w < nw; ++w) hsoff[w + 1] = hsoff[w] + (int32_t)C[slow[b0 + w]];
        DevBuf<int32_t> dsoff, dnpass, dkend;
        DevBuf<uint64_t> k1, k2;
        SGLCHK(upload(s, dsoff, hsoff.data(), hsoff.size(), "upload"));
        SGLCHK(dnpass.alloc((size_t)nw));
        SGLCHK(dkend.alloc((size_t)nw));
        SGLCHK(k1.alloc((size_t)tot));
        SGLCHK(k2.alloc((size_t)tot));
        SGLCHK(NB_DISPATCH(met, lknn_launch_slow_keys, s, a, dwork, nw, dsoff.p, k1.p, dnpass.p));
        const auto sort_segments = [&](int32_t* ends) {   // k1's segments [soff[w], ends[w]) -> k2
            return cub_run([&](void* tmp, size_t& bytes) {
                return hipcub::DeviceSegmentedRadixSort::SortKeys(tmp, bytes, k1.p, k2.p, (int)tot, (int)nw, dsoff.p, ends, 0, 64, s);
            }, "segmented sort");
        };
        SGLCHK(sort_segments(dsoff.p + 1));
        lknn_slow_trim_kernel<<<dim3(grid_for(nw, 1)), dim3(256), 0, s>>>(k2.p, k1.p, dsoff.p, dnpass.p, nw, k, dkend.p);
        NBCHK(hipGetLastError(), "lknn_slow_trim_kernel");
        SGLCHK(sort_segments(dkend.p));
        lknn_slow_write_kernel<<<dim3(grid_for(nw, 1)), dim3(256), 0, s>>>(k2.p, dsoff.p, dkend.p, dwork, nw, cl.sidx.p, dtoff.p, ti.p, tx.p,
                                                                            kept.p, nzc.p);
        NBCHK(hipGetLastError(), "lknn_slow_write_kernel");
        NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");   // the batch's buffers go back to the pool
        b0 = b1;
    }

    // --- counts, slot overflow, column pointers
    std::vector<int32_t> hkept((size_t)n), hnz((size_t)n);
    SGLCHK(download(s, hkept.data(), kept.p, (size_t)n, "download"));
    SGLCHK(download(s, hnz.data(), nzc.p, (size_t)n, "download"));
    NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    for (int64_t pt = 0; pt < n; ++pt)
        if ((double)hkept[pt] > n_max_edges) {
            sgl_set_error("c_LKNN: point %lld keeps %d neighbours, more than the %.0f slots per point the reference allocates "
                          "(ceil((2 * radius + 1)^2) - 1): the reference would write into the next point's slots",
                          (long long)pt, hkept[pt], n_max_edges);
            return SGL_EINVAL;
        }
    SGLCHK(csc_pointers(hnz, "c_LKNN: %lld edges do not fit a dgCMatrix", p_out, nnz_out));
    return csc_fill<int64_t>(s, n, p_out, *nnz_out, cap, "sgl_c_lknn: output capacity %lld < %lld edges", i_out, x_out,
                             [&](const int64_t* off, int32_t* oi, double* ox) {
        lknn_compact_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(dtoff.p, kept.p, off, ti.p, tx.p, n, oi, ox);
        NBCHK(hipGetLastError(), "lknn_compact_kernel");
        return SGL_OK;
    });
}

// ----------------------------------------------------------------------------------------------------------------- SNN ---
namespace {

constexpr int SNN_CAP = 2048;    // gathered column indices a column sorts in LDS (8 KB); above: dense counters in HBM

__global__ void snn_row_hist_kernel(const int32_t* __restrict__ Gi, int64_t nnz, int64_t* __restrict__ rcnt) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x)
        atomicAdd((unsigned long long*)&rcnt[Gi[e]], 1ull);
}

// Row-major pattern: the columns of each row (in no particular order: every use sorts or counts them).
__global__ void snn_row_fill_kernel(const int32_t* __restrict__ Gi, const int64_t* __restrict__ Gp, int64_t ncol,
                                    int64_t* __restrict__ cursor, int32_t* __restrict__ Rj) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t c = wave; c < ncol; c += nwaves)
        for (int64_t e = Gp[c] + lane; e < Gp[c + 1]; e += 64)
            Rj[atomicAdd((unsigned long long*)&cursor[Gi[e]], 1ull)] = (int32_t)c;
}

// T[i] = the gathered list length of column i: the sum of its rows' lengths.
__global__ void snn_gather_len_kernel(const int32_t* __restrict__ Gi, const int64_t* __restrict__ Gp, const int64_t* __restrict__ Rp,
                                      int64_t ncol, int64_t* __restrict__ T) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncol; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = 0;
        for (int64_t e = Gp[c]; e < Gp[c + 1]; ++e) t += Rp[Gi[e] + 1] - Rp[Gi[e]];
        T[c] = t;
    }
}

// Entry (i, j) of the SNN (:1612-1652): the diagonal always, else the Jaccard index of the two columns' row sets, in FP64,
// kept when strictly above min_similarity.
__device__ __forceinline__ bool snn_keep(int64_t i, int64_t j, int64_t inter, const int64_t* Gp, double min_sim, double* sim) {
    if (j == i) { *sim = 1.0; return true; }
    const int64_t ni = Gp[i + 1] - Gp[i], nj = Gp[j + 1] - Gp[j];
    *sim = (double)inter / (double)(ni + nj - inter);
    return *sim > min_sim;
}

// Columns whose gathered list fits LDS, one 64-lane workgroup each: sort the list; a run of j of length L means |rows(i) and
// rows(j)| = L.  FILL = false: count the entries; FILL = true: write them at off[i], ascending j.
template <bool FILL>
__global__ __launch_bounds__(64) void snn_fast_kernel(const int32_t* __restrict__ Gi, const int64_t* __restrict__ Gp,
                                                      const int64_t* __restrict__ Rp, const int32_t* __restrict__ Rj,
                                                      const int32_t* __restrict__ work, int64_t nwork, const int64_t* __restrict__ T,
                                                      double min_sim, int64_t* __restrict__ cnt, const int64_t* __restrict__ off,
                                                      int32_t* __restrict__ oi, double* __restrict__ ox) {
    __shared__ uint32_t s[SNN_CAP + 1];
    const int lane = threadIdx.x;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t i = work[w];
        const int Tn = (int)T[i];
        int P = 64;
        while (P < Tn) P <<= 1;
        int at = 0;
        for (int64_t e = Gp[i]; e < Gp[i + 1]; ++e) {
            const int64_t r0 = Rp[Gi[e]], len = Rp[Gi[e] + 1] - r0;
            for (int q = lane; q < len; q += 64) s[at + q] = (uint32_t)Rj[r0 + q];
            at += (int)len;
        }
        for (int q = Tn + lane; q < P; q += 64) s[q] = 0xffffffffu;
        if (lane == 0) s[P] = 0xffffffffu;
        __syncthreads();
        bitonic_lds(s, P);
        int64_t base = FILL ? off[i] : 0;
        for (int q0 = 0; q0 < Tn; q0 += 64) {
            const int q = q0 + lane;
            bool emit = false;
            double sim = 0.0;
            uint32_t j = 0;
            if (q < Tn && (q == 0 || s[q - 1] != s[q])) {
                j = s[q];
                int L = 1;
                while (s[q + L] == j) ++L;   // s[P] is a sentinel; j < ncol
                emit = snn_keep(i, j, L, Gp, min_sim, &sim);
            }
            const uint64_t bal = __ballot(emit);
            if (FILL && emit) {
                const int64_t o = base + __popcll(bal & ((1ull << lane) - 1ull));
                oi[o] = (int32_t)j;
                ox[o] = sim;
            }
            base += __popcll(bal);
        }
        if (!FILL && lane == 0) cnt[i] = base;
        __syncthreads();
    }
}

// Columns whose gathered list does not fit LDS (hub rows): one workgroup per column at a time, with a dense counter row of
// ncol entries per resident workgroup (slot) in HBM.  Counting: atomicAdd per gathered j; then each j is claimed once by
// atomicExch(.., 0) (which also leaves the counters zero for the next column).  FILL writes the column's entries, unordered,
// to [soff[w], ...) of a staging list that a segmented sort puts in order.
template <bool FILL>
__global__ __launch_bounds__(256) void snn_slow_kernel(const int32_t* __restrict__ Gi, const int64_t* __restrict__ Gp,
                                                       const int64_t* __restrict__ Rp, const int32_t* __restrict__ Rj,
                                                       const int32_t* __restrict__ work, int64_t nwork, int64_t ncol,
                                                       uint32_t* __restrict__ counters, double min_sim, int64_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ soff, int32_t* __restrict__ si,
                                                       double* __restrict__ sx) {
    __shared__ unsigned long long total;
    uint32_t* my = counters + (size_t)blockIdx.x * (size_t)ncol;
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t i = work[w];
        if (threadIdx.x == 0) total = 0;
        for (int64_t e = Gp[i]; e < Gp[i + 1]; ++e)
            for (int64_t q = Rp[Gi[e]] + threadIdx.x; q < Rp[Gi[e] + 1]; q += blockDim.x) atomicAdd(&my[Rj[q]], 1u);
        __syncthreads();
        unsigned long long mine = 0;
        for (int64_t e = Gp[i]; e < Gp[i + 1]; ++e)
            for (int64_t q = Rp[Gi[e]] + threadIdx.x; q < Rp[Gi[e] + 1]; q += blockDim.x) {
                const int32_t j = Rj[q];
                const uint32_t L = atomicExch(&my[j], 0u);
                double sim;
                if (L && snn_keep(i, j, L, Gp, min_sim, &sim)) {
                    if (FILL) {
                        const unsigned long long o = atomicAdd(&total, 1ull);
                        si[soff[w] + (int64_t)o] = j;
                        sx[soff[w] + (int64_t)o] = sim;
                    } else {
                        ++mine;
                    }
                }
            }
        if (!FILL) atomicAdd(&total, mine);
        __syncthreads();
        if (!FILL && threadIdx.x == 0) cnt[i] = (int64_t)total;
        __syncthreads();
    }
}

__global__ void snn_scatter_kernel(const int32_t* __restrict__ si, const double* __restrict__ sx, const int64_t* __restrict__ soff,
                                   const int32_t* __restrict__ work, int64_t nwork, const int64_t* __restrict__ off,
                                   int32_t* __restrict__ oi, double* __restrict__ ox) {
    for (int64_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int64_t o = off[work[w]];
        for (int64_t q = soff[w] + threadIdx.x; q < soff[w + 1]; q += blockDim.x) {
            oi[o + q - soff[w]] = si[q];
            ox[o + q - soff[w]] = sx[q];
        }
    }
}

}  // namespace

extern "C" int sgl_c_snn(const int32_t* Gi, const int32_t* Gp, int32_t G_nrow, int32_t G_ncol, double min_similarity,
                         int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap) {
    if (!Gp || !p_out || !nnz_out || G_nrow < 0 || G_ncol < 0) { sgl_set_error("sgl_c_snn: bad arguments"); return SGL_EINVAL; }
    if ((i_out == nullptr) != (x_out == nullptr)) { sgl_set_error("sgl_c_snn: i_out and x_out go together"); return SGL_EINVAL; }
    const int64_t n = G_ncol;
    if (Gp[0] != 0) { sgl_set_error("c_SNN: invalid column pointer array (p[0] = %d)", Gp[0]); return SGL_EINVAL; }
    std::vector<int64_t> hp((size_t)n + 1);
    for (int64_t c = 0; c <= n; ++c) {
        if (c > 0 && Gp[c] < Gp[c - 1]) { sgl_set_error("c_SNN: invalid column pointer array: p decreases at column %lld", (long long)(c - 1)); return SGL_EINVAL; }
        hp[c] = Gp[c];
    }
    const int64_t gnnz = hp[n];
    if (gnnz > 0 && !Gi) { sgl_set_error("sgl_c_snn: bad arguments"); return SGL_EINVAL; }

    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    hipStream_t s = hd.c->stream;
    DevBuf<int32_t> dGi, Rj;
    DevBuf<int64_t> dGp, Rp, rcnt, T, cnt;
    DevBuf<int> flag;
    SGLCHK(upload(s, dGi, Gi, (size_t)gnnz, "upload of G@i"));
    SGLCHK(upload(s, dGp, hp.data(), hp.size(), "upload of G@p"));
    SGLCHK(flag.alloc(1));
    NBCHK(hipMemsetAsync(flag.p, 0, sizeof(int), s), "hipMemsetAsync");
    SGLCHK(k_validate_csc(s, dGi.p, dGp.p, n, G_nrow, flag.p));
    int hflag = 0;
    SGLCHK(download(s, &hflag, flag.p, 1, "download of the flag"));
    NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (hflag) {
        sgl_set_error("c_SNN: G is not a valid dgCMatrix: %s%s", (hflag & 1) ? "row index outside [0, nrow) " : "",
                      (hflag & 2) ? "row indices not strictly ascending within a column" : "");
        return SGL_EINVAL;
    }

    // --- row-major pattern, gathered list lengths
    const int64_t nr = G_nrow;
    SGLCHK(rcnt.alloc((size_t)nr + 1));
    SGLCHK(Rp.alloc((size_t)nr + 1));
    SGLCHK(Rj.alloc((size_t)gnnz));
    SGLCHK(T.alloc((size_t)n));
    SGLCHK(cnt.alloc((size_t)n));
    NBCHK(hipMemsetAsync(rcnt.p, 0, sizeof(int64_t) * ((size_t)nr + 1), s), "hipMemsetAsync");
    if (gnnz > 0) {
        snn_row_hist_kernel<<<dim3(grid_for(gnnz, 256)), dim3(256), 0, s>>>(dGi.p, gnnz, rcnt.p);
        NBCHK(hipGetLastError(), "snn_row_hist_kernel");
    }
    SGLCHK(k_exclusive_scan(hd.c, rcnt.p, Rp.p, nr));
    SGLCHK(k_scan_total(s, rcnt.p, Rp.p, nr));
    NBCHK(hipMemcpyAsync(rcnt.p, Rp.p, sizeof(int64_t) * (size_t)nr, hipMemcpyDeviceToDevice, s), "copy");
    if (n > 0) {
        snn_row_fill_kernel<<<dim3(grid_for(n, 4)), dim3(256), 0, s>>>(dGi.p, dGp.p, n, rcnt.p, Rj.p);
        NBCHK(hipGetLastError(), "snn_row_fill_kernel");
        snn_gather_len_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(dGi.p, dGp.p, Rp.p, n, T.p);
        NBCHK(hipGetLastError(), "snn_gather_len_kernel");
    }
    std::vector<int64_t> hT((size_t)n), hcnt((size_t)n, 0);
    SGLCHK(download(s, hT.data(), T.p, (size_t)n, "download"));
    NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    WorkLists wl;   // (an empty column has no entries, :1611)
    SGLCHK(split_work(s, hT, SNN_CAP, wl));
    const int64_t nfast = (int64_t)wl.fast.size(), nslow = (int64_t)wl.slow.size();
    NBCHK(hipMemsetAsync(cnt.p, 0, sizeof(int64_t) * (size_t)std::max<int64_t>(n, 1), s), "hipMemsetAsync");
    DevBuf<uint32_t> counters;
    int64_t nslots = 0;
    if (nslow > 0) {   // one counter row of ncol per resident workgroup, at most 256 MB of them
        nslots = std::max<int64_t>(1, std::min<int64_t>({nslow, 1024, ((int64_t)1 << 26) / std::max<int64_t>(n, 1)}));
        SGLCHK(counters.alloc((size_t)(nslots * n)));
        NBCHK(hipMemsetAsync(counters.p, 0, sizeof(uint32_t) * (size_t)(nslots * n), s), "hipMemsetAsync");
    }

    // --- count pass
    if (nfast > 0) {
        snn_fast_kernel<false><<<dim3(grid_for(nfast, 1)), dim3(64), 0, s>>>(
            dGi.p, dGp.p, Rp.p, Rj.p, wl.dfast.p, nfast, T.p, min_similarity, cnt.p, nullptr, nullptr, nullptr);
        NBCHK(hipGetLastError(), "snn_fast_kernel");
    }
    if (nslow > 0) {
        snn_slow_kernel<false><<<dim3((unsigned)nslots), dim3(256), 0, s>>>(dGi.p, dGp.p, Rp.p, Rj.p, wl.dslow.p, nslow, n, counters.p,
                                                                          min_similarity, cnt.p, nullptr, nullptr, nullptr);
        NBCHK(hipGetLastError(), "snn_slow_kernel");
    }
    SGLCHK(download(s, hcnt.data(), cnt.p, (size_t)n, "download"));
    NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    SGLCHK(csc_pointers(hcnt, "c_SNN: the graph would hold %lld entries, which a dgCMatrix (32-bit column pointers) cannot hold; "
                              "raise min_similarity", p_out, nnz_out));

    // --- fill pass
    return csc_fill<int64_t>(s, n, p_out, *nnz_out, cap, "sgl_c_snn: output capacity %lld < %lld entries", i_out, x_out,
                             [&](const int64_t* off, int32_t* oi, double* ox) -> int {
        if (nfast > 0) {
            snn_fast_kernel<true><<<dim3(grid_for(nfast, 1)), dim3(64), 0, s>>>(
                dGi.p, dGp.p, Rp.p, Rj.p, wl.dfast.p, nfast, T.p, min_similarity, nullptr, off, oi, ox);
            NBCHK(hipGetLastError(), "snn_fast_kernel");
        }
        if (nslow == 0) return SGL_OK;
        std::vector<int64_t> hsoff((size_t)nslow + 1);
        hsoff[0] = 0;
        for (int64_t w = 0; w < nslow; ++w) hsoff[w + 1] = hsoff[w] + hcnt[wl.slow[w]];
        const int64_t stot = hsoff[nslow];
        DevBuf<int64_t> dsoff;
        DevBuf<int32_t> si, si2;
        DevBuf<double> sx, sx2;
        SGLCHK(upload(s, dsoff, hsoff.data(), hsoff.size(), "upload"));
        SGLCHK(si.alloc((size_t)stot));
        SGLCHK(si2.alloc((size_t)stot));
        SGLCHK(sx.alloc((size_t)stot));
        SGLCHK(sx2.alloc((size_t)stot));
        snn_slow_kernel<true><<<dim3((unsigned)nslots), dim3(256), 0, s>>>(dGi.p, dGp.p, Rp.p, Rj.p, wl.dslow.p, nslow, n, counters.p,
                                                                         min_similarity, nullptr, dsoff.p, si.p, sx.p);
        NBCHK(hipGetLastError(), "snn_slow_kernel");
        SGLCHK(cub_run([&](void* tmp, size_t& bytes) {
            return hipcub::DeviceSegmentedRadixSort::SortPairs(tmp, bytes, si.p, si2.p, sx.p, sx2.p, (int)stot, (int)nslow, dsoff.p, dsoff.p + 1,
                                                               0, 32, s);
        }, "segmented sort"));
        snn_scatter_kernel<<<dim3(grid_for(nslow, 1)), dim3(256), 0, s>>>(si2.p, sx2.p, dsoff.p, wl.dslow.p, nslow, off, oi, ox);
        NBCHK(hipGetLastError(), "snn_scatter_kernel");
        NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
        return SGL_OK;
    });
}

// ------------------------------------------------------------------------------------------------------- spatial_graph ---
// spatial_graph (src/singlet.cpp:1365-1414): for every point i, the points j = 0, 1, ... in INDEX order with
// d = sqrt((c1[i]-c1[j])^2 + (c2[i]-c2[j])^2) < max_dist (double, no contraction), up to max_k of them, weighted
// (max_dist - d) * (1 / max_dist) and divided by the column's sum.  The selection is by index, not by distance, and the
// reference stops scanning at the max_k-th accepted point.  Here a cell list bounds the candidates to the 3 x 3 buckets of
// a point; each bucket's members stay in ascending index order (stable sort), and one 64-lane workgroup per point visits the
// nine lists as a merge in ascending index, in batches: T = the smallest "64th remaining index" over the nine lists, and a
// batch is every remaining candidate <= T (at most 64 per list, at least 64 in all unless the lists run out).  The accepted
// ones of a batch are ranked by index across the lists (binary searches in LDS) and taken in that order until max_k.  The
// early stop keeps the all-in-range case (max_dist above the data's extent) at O(n max_k), as the reference's loop is.
// Count pass (per point: kept entries, and the column sum, sequential in ascending row order), a host scan, fill pass.
namespace {

constexpr int SG_LISTS = 9;

struct SgArgs {
    const double* sx;        // coordinates at each sorted position
    const double* sy;
    const uint32_t* sidx;    // point at each sorted position
    const int32_t* bnd;      // 12 per sorted position: for rows by-1 .. by+1, the sorted positions where buckets bx-1 .. bx+2 start
    int64_t n;
    double max_dist, scale;  // scale = 1 / max_dist, rounded once on the host (the reference's scale_factor)
    int64_t K;               // min(max_k, n) >= 1
};

// Coordinates in sorted order.
__global__ void sg_gather_kernel(const uint32_t* __restrict__ sidx, const double* __restrict__ c1, const double* __restrict__ c2, int64_t n,
                                 double* __restrict__ sx, double* __restrict__ sy) {
    for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < n; pos += (int64_t)gridDim.x * blockDim.x) {
        sx[pos] = c1[sidx[pos]];
        sy[pos] = c2[sidx[pos]];
    }
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    for (int m = 32; m > 0; m >>= 1) v = std::min(v, (uint32_t)__shfl_xor((int)v, m));
    return v;
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const uint64_t u = __double_as_longlong(v);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, l), hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), l);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// One 64-lane workgroup per point, in sorted (spatial) order.  FILL = false: cnt[pt] = the kept entries, colsum[pt] = their
// weights summed in ascending row order.  FILL = true: rows and weights / colsum[pt] at off[pt], ascending rows.
template <bool FILL>
__global__ __launch_bounds__(64) void sg_merge_kernel(SgArgs a, int32_t* __restrict__ cnt, double* __restrict__ colsum,
                                                      const int32_t* __restrict__ off, int32_t* __restrict__ oi, double* __restrict__ ox) {
    __shared__ uint32_t aj[SG_LISTS * 64];   // accepted indices of the batch, list b's at [64 b, 64 b + acnt[b]), ascending
    __shared__ double aw[SG_LISTS * 64];     // their weights
    __shared__ uint16_t order[SG_LISTS * 64];   // slot of aj / aw at each rank (ascending index) of the batch
    __shared__ int acnt[SG_LISTS];
    const int lane = threadIdx.x;
    for (int64_t pos = blockIdx.x; pos < a.n; pos += gridDim.x) {
        const uint32_t pt = a.sidx[pos];
        const double px = a.sx[pos], py = a.sy[pos];
        int cur = 0, end = 0;   // lane b < 9: the remaining run [cur, end) of list b
        if (lane < SG_LISTS) {
            const int32_t* bb = a.bnd + pos * 12 + (lane / 3) * 4 + lane % 3;
            cur = bb[0];
            end = bb[1];
        }
        int64_t acc = 0;
        double sum = FILL ? colsum[pt] : 0.0;
        const int64_t base = FILL ? off[pt] : 0;
        while (acc < a.K) {
            if (__ballot(cur < end) == 0) break;   // every list exhausted
            const uint32_t T = wave_min_u32((lane < SG_LISTS && end - cur >= 64) ? a.sidx[cur + 63] : 0xffffffffu);
            int took = 0;   // lane b < 9: the candidates of list b this batch consumes
            for (int b = 0; b < SG_LISTS; ++b) {
                const int cb = __shfl(cur, b), eb = __shfl(end, b);
                int na = 0;
                if (cb < eb) {
                    const int e = cb + lane;
                    bool in = false, ok = false;
                    uint32_t j = 0;
                    double w = 0.0;
                    if (e < eb) {
                        j = a.sidx[e];
                        in = j <= T;   // a prefix of the list's remaining run
                        if (in) {
                            const double dx = px - a.sx[e], dy = py - a.sy[e];
                            const double d = __builtin_sqrt(dx * dx + dy * dy);
                            ok = d < a.max_dist;
                            w = (a.max_dist - d) * a.scale;
                        }
                    }
                    const uint64_t bok = __ballot(ok);
                    if (ok) {
                        const int slot = b * 64 + __popcll(bok & ((1ull << lane) - 1ull));
                        aj[slot] = j;
                        aw[slot] = w;
                    }
                    na = __popcll(bok);
                    const int nin = __popcll(__ballot(in));
                    if (lane == b) took = nin;
                }
                if (lane == 0) acnt[b] = na;
            }
            __syncthreads();
            int A = 0;
            for (int b = 0; b < SG_LISTS; ++b) A += acnt[b];
            if (A > 0) {
                // rank of each accepted candidate among the batch's: its place in its own list plus, in every other list, the
                // number of accepted indices below it (the indices are distinct: a point lies in one bucket)
                for (int e = lane; e < SG_LISTS * 64; e += 64) {
                    const int b = e >> 6, q = e & 63;
                    if (q < acnt[b]) {
                        const uint32_t j = aj[e];
                        int r = q;
                        for (int o = 0; o < SG_LISTS; ++o) {
                            if (o == b) continue;
                            int lo = 0, hi = acnt[o];
                            while (lo < hi) {
                                const int mid = (lo + hi) >> 1;
                                if (aj[o * 64 + mid] < j) lo = mid + 1;
                                else hi = mid;
                            }
                            r += lo;
                        }
                        order[r] = (uint16_t)e;
                    }
                }
                __syncthreads();
                const int take = (int)std::min<int64_t>(A, a.K - acc);
                for (int r0 = 0; r0 < take; r0 += 64) {
                    const int r = r0 + lane;
                    if (FILL) {
                        if (r < take) {
                            const int e = order[r];
                            oi[base + acc + r] = (int32_t)aj[e];
                            ox[base + acc + r] = aw[e] / sum;
                        }
                    } else {   // the column sum, one weight after the other in ascending row order
                        const double v = r < take ? aw[order[r]] : 0.0;
                        const int m = std::min(64, take - r0);
                        for (int l = 0; l < m; ++l) sum += readlane_f64(v, l);
                    }
                }
                acc += take;
            }
            __syncthreads();   // the batch's LDS is read by every lane before the next batch writes it
            cur += took;
        }
        if (!FILL && lane == 0) {
            cnt[pt] = (int32_t)acc;
            colsum[pt] = sum;
        }
    }
}

}  // namespace

extern "C" int sgl_spatial_graph(const double* c1, const double* c2, int32_t n, double max_dist, int64_t max_k,
                                 int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap) {
    if (!p_out || !nnz_out || n < 0 || (n > 0 && (!c1 || !c2))) { sgl_set_error("sgl_spatial_graph: bad arguments"); return SGL_EINVAL; }
    if ((i_out == nullptr) != (x_out == nullptr)) { sgl_set_error("sgl_spatial_graph: i_out and x_out go together"); return SGL_EINVAL; }
    if (max_k < 0) { sgl_set_error("spatial_graph: max_k = %lld is negative", (long long)max_k); return SGL_EINVAL; }
    if (!(max_dist > 0.0) || !(max_dist < INFINITY)) {
        sgl_set_error("spatial_graph: max_dist = %g must be finite and > 0", max_dist);
        return SGL_EINVAL;
    }
    const double scale = 1.0 / max_dist;   // the reference's scale_factor
    if (!(scale < INFINITY)) { sgl_set_error("spatial_graph: 1 / max_dist (max_dist = %g) is not finite", max_dist); return SGL_EINVAL; }
    double xmin = 0, xmax = 0, ymin = 0, ymax = 0;
    for (int64_t e = 0; e < n; ++e) {
        const double x = c1[e], y = c2[e];
        if (!(fabs(x) < INFINITY) || !(fabs(y) < INFINITY)) {
            sgl_set_error("spatial_graph: coordinate %lld is not finite", (long long)e);
            return SGL_EINVAL;
        }
        if (e == 0 || x < xmin) xmin = x;
        if (e == 0 || x > xmax) xmax = x;
        if (e == 0 || y < ymin) ymin = y;
        if (e == 0 || y > ymax) ymax = y;
    }
    const int64_t K = std::min<int64_t>(max_k, n);   // max_k > n acts as n: the scan of n points ends there

    CtxHolder hd;
    SGLCHK(sgl_create(current_device_or_zero(), &hd.c));
    hipStream_t s = hd.c->stream;
    if (K == 0) {   // n = 0 or max_k = 0: the empty n x n graph
        for (int64_t c = 0; c <= n; ++c) p_out[c] = 0;
        *nnz_out = 0;
        return SGL_OK;
    }

    // --- spatial cell list, coordinates in sorted order
    DevBuf<double> d1, d2, sx, sy, colsum;
    DevBuf<int32_t> cnt;
    CellList cl;
    SGLCHK(upload(s, d1, c1, (size_t)n, "upload of c1"));
    SGLCHK(upload(s, d2, c2, (size_t)n, "upload of c2"));
    SGLCHK(cell_list_build(s, d1.p, d2.p, n, cell_grid(xmin, xmax, ymin, ymax, max_dist, ldexp(1.0, -510)), cl, nullptr));
    SGLCHK(sx.alloc((size_t)n));
    SGLCHK(sy.alloc((size_t)n));
    sg_gather_kernel<<<dim3(grid_for(n, 256)), dim3(256), 0, s>>>(cl.sidx.p, d1.p, d2.p, n, sx.p, sy.p);
    NBCHK(hipGetLastError(), "sg_gather_kernel");

    // --- count pass, scan, 2^31 check
    SGLCHK(cnt.alloc((size_t)n));
    SGLCHK(colsum.alloc((size_t)n));
    const SgArgs a{sx.p, sy.p, cl.sidx.p, cl.bnd.p, n, max_dist, scale, K};
    sg_merge_kernel<false><<<dim3(grid_for(n, 1)), dim3(64), 0, s>>>(a, cnt.p, colsum.p, nullptr, nullptr, nullptr);
    NBCHK(hipGetLastError(), "sg_merge_kernel (count)");
    std::vector<int32_t> hcnt((size_t)n);
    SGLCHK(download(s, hcnt.data(), cnt.p, (size_t)n, "download of the counts"));
    NBCHK(hipStreamSynchronize(s), "hipStreamSynchronize");
    SGLCHK(csc_pointers(hcnt, "spatial_graph: the graph would hold %lld entries, which a dgCMatrix (32-bit column pointers) cannot hold; "
                              "lower max_dist or max_k", p_out, nnz_out));

    // --- fill pass
    return csc_fill<int32_t>(s, n, p_out, *nnz_out, cap, "sgl_spatial_graph: output capacity %lld < %lld entries", i_out, x_out,
                             [&](const int32_t* off, int32_t* oi, double* ox) -> int {
        sg_merge_kernel<true><<<dim3(grid_for(n, 1)), dim3(64), 0, s>>>(a, nullptr, colsum.p, off, oi, ox);
        NBCHK(hipGetLastError(), "sg_merge_kernel (fill)");
        return SGL_OK;
    });
}
