// Graph convolution of graph-convolutional NMF (c_gcnmf, src/singlet.cpp:1668-1710):
//     Y(:, j) = sum over the entries (r, v) of column j of G, in stored order, of v * X(:, r)
// X, Y: k x n column-major (k doubles per cell), G: n x n CSC with 64-bit offsets.  The H-update convolves the
// right-hand sides (Bc = B G, l.1684-1690), the W-update the scaled factor (Hc = H G, whose right-hand sides over t(A)
// are those of l.1703-1706).
//
// The cost is the gather: k * 8 bytes of X per entry against 12 bytes of G, with few entries per column (6 - 30 on
// spatial and kNN graphs).  Mapping: LPC lanes per output column, each lane holding VEC consecutive factor rows (16-byte
// loads when k is even), NP passes of 64 lanes when one column needs more than 64 lanes; 64 / LPC columns per wave at
// small k.  Every lane of a column's group reads the column's (row, value) pairs itself (one address per group: the
// loads coalesce) and keeps four gathers in flight.  Each column is summed sequentially in its stored order, FMA onto a
// zero start, so the result is deterministic and a unit self-loop reproduces X exactly.
//
// Hubs: a column with more than SGL_GRAPH_HUB entries is skipped by the main pass; its entries are cut into segments of
// SGL_GRAPH_SEG, one lane group each (same loop, into a partial slab), and a last kernel adds the partials of every hub
// in segment order.  One long column thus costs its length / SGL_GRAPH_SEG groups of the second pass instead of
// serialising a wave of the first.
//
// Team ranks (multi.hip, sgl_multi_set_graph): a rank holds the columns of its own cells, and the rows it reads from other
// ranks' cells arrive in a halo slab.  Its row indices are rewritten on the host: below n_src a column of X, from n_src
// on a column of the slab (n_src + s * E + e = entry e of rank s's export list).  graph_pack_kernel copies a rank's
// exported columns into its block of the slab; the HALO instances of graph_conv_kernel choose the source per entry and
// are otherwise the same loop (same lanes per column, four gathers in flight, sequential FMA from zero, hub segments).
#include "sgl_internal.h"

template <int VEC>
struct GVec;
template <>
struct GVec<1> {
    double a;
    __device__ __forceinline__ static GVec load(const double* p) { return GVec{*p}; }
    __device__ __forceinline__ void fma_into(double v, const GVec& x) { a = fma(v, x.a, a); }
    __device__ __forceinline__ void store(double* p) const { *p = a; }
};
template <>
struct GVec<2> {
    double a, b;
    __device__ __forceinline__ static GVec load(const double* p) {
        const double2 t = *reinterpret_cast<const double2*>(p);
        return GVec{t.x, t.y};
    }
    __device__ __forceinline__ void fma_into(double v, const GVec& x) { a = fma(v, x.a, a); b = fma(v, x.b, b); }
    __device__ __forceinline__ void store(double* p) const { *reinterpret_cast<double2*>(p) = make_double2(a, b); }
};

// SEGS = false: item = output column j (hubs skipped), written to Y(:, j).
// SEGS = true:  item = segment s of a hub column, its partial written to part + s * k.
// HALO = true: a row index r >= n_src names column r - n_src of `halo` instead of a column of X.
template <int VEC, int LPC, int NP, bool SEGS, bool HALO>
__global__ __launch_bounds__(256) void graph_conv_kernel(const double* __restrict__ X, double* __restrict__ Y,
                                                         const int64_t* __restrict__ Gp, const int32_t* __restrict__ Gi,
                                                         const double* __restrict__ Gx, int64_t nitems, int k,
                                                         const int32_t* __restrict__ seg_col,
                                                         const int64_t* __restrict__ seg_q0,
                                                         const double* __restrict__ halo, int32_t n_src) {
    // column r of the source: of X, or (HALO) of the slab past n_src
    auto src = [&](int32_t r) -> const double* {
        if (HALO && r >= n_src) return halo + (int64_t)(r - n_src) * k;
        return X + (int64_t)r * k;
    };
    const int gl = threadIdx.x & (LPC - 1);
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LPC;
    const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) / LPC;
    const int ne = k / VEC;   // vector elements per column
    for (int64_t item = group; item < nitems; item += ngroups) {
        int64_t lo, hi;
        double* out;
        if (SEGS) {
            const int64_t col = seg_col[item];
            lo = seg_q0[item];
            hi = min(lo + (int64_t)SGL_GRAPH_SEG, Gp[col + 1]);
            out = Y + item * k;
        } else {
            lo = Gp[item];
            hi = Gp[item + 1];
            if (hi - lo > SGL_GRAPH_HUB) continue;   // a hub: the segment pass sums it
            out = Y + item * k;
        }
        GVec<VEC> acc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] = GVec<VEC>{};
        int64_t q = lo;
        for (; q + 4 <= hi; q += 4) {
            const int32_t r0 = Gi[q], r1 = Gi[q + 1], r2 = Gi[q + 2], r3 = Gi[q + 3];
            const double v0 = Gx[q], v1 = Gx[q + 1], v2 = Gx[q + 2], v3 = Gx[q + 3];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int e = gl + LPC * p;
                if (e < ne) {
                    const GVec<VEC> x0 = GVec<VEC>::load(src(r0) + e * VEC);
                    const GVec<VEC> x1 = GVec<VEC>::load(src(r1) + e * VEC);
                    const GVec<VEC> x2 = GVec<VEC>::load(src(r2) + e * VEC);
                    const GVec<VEC> x3 = GVec<VEC>::load(src(r3) + e * VEC);
                    acc[p].fma_into(v0, x0);
                    acc[p].fma_into(v1, x1);
                    acc[p].fma_into(v2, x2);
                    acc[p].fma_into(v3, x3);
                }
            }
        }
        for (; q < hi; ++q) {
            const int32_t r0 = Gi[q];
            const double v0 = Gx[q];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int e = gl + LPC * p;
                if (e < ne) acc[p].fma_into(v0, GVec<VEC>::load(src(r0) + e * VEC));
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int e = gl + LPC * p;
            if (e < ne) acc[p].store(out + e * VEC);
        }
    }
}

// Y(:, hub_col[h]) = sum of the partials of the hub's segments, in segment order (one thread per hub and factor row)
__global__ __launch_bounds__(256) void graph_hub_combine_kernel(const double* __restrict__ part, double* __restrict__ Y,
                                                                const int32_t* __restrict__ hub_col,
                                                                const int32_t* __restrict__ hub_seg0, int32_t nhub, int k) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)nhub * k) return;
    const int32_t h = (int32_t)(t / k);
    const int f = (int)(t - (int64_t)h * k);
    double s = 0.0;
    for (int32_t g = hub_seg0[h]; g < hub_seg0[h + 1]; ++g) s += part[(int64_t)g * k + f];
    Y[(int64_t)hub_col[h] * k + f] = s;
}

template <int VEC, int LPC, int NP, bool SEGS, bool HALO>
static int launch_conv(hipStream_t s, const DevGraph& g, const double* X, double* Y, int k, int64_t nitems) {
    if (nitems <= 0) return SGL_OK;
    const int64_t per_block = 256 / LPC;
    int64_t blocks = (nitems + per_block - 1) / per_block;
    if (blocks > (int64_t)1 << 20) blocks = (int64_t)1 << 20;   // grid-stride beyond (a million workgroups: 4096 per CU)
    graph_conv_kernel<VEC, LPC, NP, SEGS, HALO><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(X, Y, g.p, g.i, g.x, nitems, k, g.seg_col,
                                                                                            g.seg_q0, g.halo, g.n_src);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

// One ladder for both VEC.  Two of its rungs no rank reaches: <1, 2, 1> (an odd k with ne <= 2 is k = 1) and <2, 64, 16>
// (an even k <= SGL_MAX_K = 1024 has ne <= 512); they stay so that the ladder reads the same for both and a larger
// SGL_MAX_K needs no new rung.  The 20 reachable ones are run one by one by tests/test_gpu_graph_conv.py.
template <int VEC, bool SEGS, bool HALO>
static int dispatch_lpc(hipStream_t s, const DevGraph& g, const double* X, double* Y, int k, int64_t nitems) {
    const int ne = k / VEC;
    if (ne <= 1) return launch_conv<VEC, 1, 1, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 2) return launch_conv<VEC, 2, 1, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 4) return launch_conv<VEC, 4, 1, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 8) return launch_conv<VEC, 8, 1, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 16) return launch_conv<VEC, 16, 1, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 32) return launch_conv<VEC, 32, 1, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 64) return launch_conv<VEC, 64, 1, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 128) return launch_conv<VEC, 64, 2, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 256) return launch_conv<VEC, 64, 4, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 512) return launch_conv<VEC, 64, 8, SEGS, HALO>(s, g, X, Y, k, nitems);
    if (ne <= 1024) return launch_conv<VEC, 64, 16, SEGS, HALO>(s, g, X, Y, k, nitems);
    sgl_set_error("graph convolution: k=%d too large", k);
    return SGL_EINVAL;
}

template <bool SEGS, bool HALO>
static int dispatch(hipStream_t s, const DevGraph& g, const double* X, double* Y, int k, int64_t nitems) {
    // 16-byte loads need every column start 16-byte aligned: k even (the buffers themselves are 256-byte aligned)
    return (k % 2 == 0) ? dispatch_lpc<2, SEGS, HALO>(s, g, X, Y, k, nitems) : dispatch_lpc<1, SEGS, HALO>(s, g, X, Y, k, nitems);
}

int k_graph_conv(hipStream_t s, DevGraph& g, const double* X, double* Y, int k) {
    if (g.n <= 0) return SGL_OK;
    if (k <= 0 || k > SGL_MAX_K) { sgl_set_error("graph convolution: k=%d out of range", k); return SGL_EINVAL; }
    // a team rank whose team exchanges a halo (E > 0) reads [X | slab]; every other graph keeps the plain instances
    const bool halo = g.E > 0;
    if (halo && !g.halo) { sgl_set_error("graph convolution: the halo slab is missing"); return SGL_ESTATE; }
    SGLCHK((halo ? dispatch<false, true>(s, g, X, Y, k, g.n) : dispatch<false, false>(s, g, X, Y, k, g.n)));
    if (g.nhub > 0) {
        SGLCHK((halo ? dispatch<true, true>(s, g, X, g.part, k, g.nseg) : dispatch<true, false>(s, g, X, g.part, k, g.nseg)));
        const int64_t threads = (int64_t)g.nhub * k;
        graph_hub_combine_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(g.part, Y, g.hub_col, g.hub_seg0,
                                                                                               g.nhub, k);
        HIPCHK(hipGetLastError());
    }
    return SGL_OK;
}

// slab block of this rank: column e = X(:, exp[e]).  One group of `lpc` lanes (a power of two, the convolution's lanes per
// column) per exported column, each lane VEC consecutive factor rows per pass.
template <int VEC>
__global__ __launch_bounds__(256) void graph_pack_kernel(const double* __restrict__ X, double* __restrict__ block,
                                                         const int32_t* __restrict__ exp, int64_t n_exp, int k, int lpc) {
    const int gl = threadIdx.x & (lpc - 1);
    const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / lpc;
    const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) / lpc;
    const int ne = k / VEC;
    for (int64_t item = group; item < n_exp; item += ngroups) {
        const double* from = X + (int64_t)exp[item] * k;
        double* to = block + item * k;
        for (int e = gl; e < ne; e += lpc) GVec<VEC>::load(from + e * VEC).store(to + e * VEC);
    }
}

// rank `rank` of a team packs the columns of X its peers read (g.exp) into block `rank` of its halo slab
int k_graph_pack(hipStream_t s, DevGraph& g, const double* X, int k, int rank) {
    if (g.E <= 0 || g.n_exp <= 0) return SGL_OK;
    if (k <= 0 || k > SGL_MAX_K) { sgl_set_error("graph pack: k=%d out of range", k); return SGL_EINVAL; }
    if (!g.halo || !g.exp || g.n_exp > g.E || rank < 0) { sgl_set_error("graph pack: no halo slab or export list"); return SGL_ESTATE; }
    const int vec = (k % 2 == 0) ? 2 : 1;
    const int ne = k / vec;
    int lpc = 1;
    while (lpc < ne && lpc < 64) lpc *= 2;
    const int64_t per_block = 256 / lpc;
    int64_t blocks = (g.n_exp + per_block - 1) / per_block;
    if (blocks > (int64_t)1 << 20) blocks = (int64_t)1 << 20;
    double* block = g.halo + (size_t)rank * g.E * k;   // (k even: rank * E * k is even, the 16-byte stores stay aligned)
    if (vec == 2) graph_pack_kernel<2><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(X, block, g.exp, g.n_exp, k, lpc);
    else graph_pack_kernel<1><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(X, block, g.exp, g.n_exp, k, lpc);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}
