// Co-occurrence of classes by distance (include/singlet_hip.h, "Co-occurrence by distance"): for every pair of classes and every
// distance interval the number of ordered pairs of points whose squared distance lies in the interval.  Everything the device
// computes is an integer, so the table is one function of the inputs whatever the grid, the bin path, the flush bound or the
// order of the atomics.  This file holds
//   1. co_extent_kernel: the bounding box (partials per workgroup, finished on the host); co_keys_kernel / hipcub's stable radix
//      sort / co_gather_kernel: the points by bucket key, x, y and label gathered into sorted order; co_ranges_kernel: per centre
//      tile of 256 sorted positions the candidate positions [p0, A1) and [B0, B1) (see below).  One bucket: no sort, the points
//      as they came, every later position a candidate.
//   2. co_tally_kernel: an n-body loop.  A lane holds one centre in registers, candidate tiles of 256 are staged in LDS and read
//      by every lane at the same address (a broadcast).  An unordered pair is counted ONCE, by the lower sorted position: the
//      exact d2 test and pos_j > pos_i decide, the candidate ranges only have to be supersets.  A lane takes the staged slots eight
//      at a time: eight reads, eight d2, then the eight interval searches side by side.  It adds 1 to bin
//      [t][min(a, b)][max(a, b)] -- LDS path: uint32 bins in LDS, flushed with 64-bit global atomics at the end and whenever the
//      pairs evaluated since the last flush could pass the bound; global path: 64-bit global atomics.
//   3. co_epilogue_kernel: the ordered table, the off-diagonal mirrored and the diagonal doubled.
//
// The candidates of a centre tile.  For a centre at sorted position pos in bucket (bx, by), the partners at later positions lie in
// its own bucket row up to the end of bucket bx + 1 -- the positions (pos, e1(pos)) -- and in buckets bx - 1 .. bx + 1 of row
// by + 1 -- the positions [s2(pos), e2(pos)); e1, s2 and e2 never descend along the sorted order and e1(pos) > pos, s2(pos) > pos.
// So over a tile [p0, p1) the first kind is exactly [p0, e1(p1 - 1)) and the second kind lies in [s2(p0), e2(p1 - 1)); the tile
// walks A = [p0, e1(p1 - 1)) and B = [max(s2(p0), e1(p1 - 1)), e2(p1 - 1)), two disjoint runs that hold both.
#include "sgl_internal.h"
#include "cooccur_host.h"

#include <hipcub/hipcub.hpp>

#define CO_THREADS COOCCUR_TILE
#define CO_BATCH 8   // staged candidates a lane reads ahead of testing them; divides COOCCUR_TILE

typedef unsigned long long co_u64;

// ---- 1. extent, keys, gather, ranges ----------------------------------------------------------------------------------------------------
// part[4 b ..]: xmin, xmax, ymin, ymax over the points workgroup b walked (finite coordinates: no NaN to order)
__global__ __launch_bounds__(CO_THREADS) void co_extent_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t n,
                                                              double* __restrict__ part) {
    __shared__ double red[4][CO_THREADS / SGL_WAVE];
    double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int64_t e = (int64_t)blockIdx.x * CO_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * CO_THREADS) {
        const double a = x[e], b = y[e];
        v[0] = a < v[0] ? a : v[0];
        v[1] = a > v[1] ? a : v[1];
        v[2] = b < v[2] ? b : v[2];
        v[3] = b > v[3] ? b : v[3];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int m = SGL_WAVE / 2; m >= 1; m >>= 1) {
            const double o = __shfl_xor(v[q], m);
            v[q] = (q & 1) ? (o > v[q] ? o : v[q]) : (o < v[q] ? o : v[q]);
        }
    if (threadIdx.x % SGL_WAVE == 0)
        for (int q = 0; q < 4; ++q) red[q][threadIdx.x / SGL_WAVE] = v[q];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        double r = red[q][0];
        for (int w = 1; w < CO_THREADS / SGL_WAVE; ++w) r = (q & 1) ? (red[q][w] > r ? red[q][w] : r) : (red[q][w] < r ? red[q][w] : r);
        part[4 * blockIdx.x + q] = r;
    }
}

__global__ __launch_bounds__(CO_THREADS) void co_keys_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t n, CooccurGrid g,
                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ iota) {
    const int64_t e = (int64_t)blockIdx.x * CO_THREADS + threadIdx.x;
    if (e >= n) return;
    // cooccur_grid's W, H hold every point: the clamps never bind
    const int64_t bx = std::min<int64_t>((int64_t)floor((x[e] - g.xmin) / g.side), g.W - 1);
    const int64_t by = std::min<int64_t>((int64_t)floor((y[e] - g.ymin) / g.side), g.H - 1);
    keys[e] = (uint64_t)(by * g.W + bx);
    iota[e] = (uint32_t)e;
}

__global__ __launch_bounds__(CO_THREADS) void co_gather_kernel(const uint32_t* __restrict__ sidx, const double* __restrict__ x,
                                                              const double* __restrict__ y, const int32_t* __restrict__ lab, int64_t n,
                                                              double* __restrict__ sx, double* __restrict__ sy, int32_t* __restrict__ slab) {
    const int64_t p = (int64_t)blockIdx.x * CO_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint32_t e = sidx[p];
    sx[p] = x[e];
    sy[p] = y[e];
    slab[p] = lab[e];
}

// the first sorted position whose key is not below v
__device__ __forceinline__ int64_t co_lower_bound(const uint64_t* __restrict__ skeys, int64_t n, uint64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skeys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// rng[3 tile ..] = A1, B0, B1 of the header comment
__global__ __launch_bounds__(CO_THREADS) void co_ranges_kernel(const uint64_t* __restrict__ skeys, int64_t n, int64_t W, int64_t H, int64_t tiles,
                                                              int64_t* __restrict__ rng) {
    const int64_t tile = (int64_t)blockIdx.x * CO_THREADS + threadIdx.x;
    if (tile >= tiles) return;
    const int64_t p0 = tile * COOCCUR_TILE, p1 = std::min<int64_t>(p0 + COOCCUR_TILE, n);
    const int64_t kf = (int64_t)skeys[p0], kl = (int64_t)skeys[p1 - 1];
    const int64_t byf = kf / W, bxf = kf % W, byl = kl / W, bxl = kl % W;
    const int64_t e1 = co_lower_bound(skeys, n, (uint64_t)(byl * W + std::min<int64_t>(bxl + 2, W)));
    const int64_t s2 = byf + 1 < H ? co_lower_bound(skeys, n, (uint64_t)((byf + 1) * W + std::max<int64_t>(bxf - 1, 0))) : n;
    const int64_t e2 = byl + 1 < H ? co_lower_bound(skeys, n, (uint64_t)((byl + 1) * W + std::min<int64_t>(bxl + 2, W))) : n;
    const int64_t b0 = std::max(s2, e1);
    rng[3 * tile] = e1;
    rng[3 * tile + 1] = b0;
    rng[3 * tile + 2] = std::max(e2, b0);
}

// ---- 2. the tally ---------------------------------------------------------------------------------------------------------------------
// grid (workgroups over the centre tiles, split).  LDS, from its 16-byte aligned base: x[256] | y[256] | thr2[66] doubles,
// label[256] int32, then at COOCCUR_STAGE_BYTES the T x K x K uint32 bins (LDS path).  sym: T x K x K, bin [t][lo][hi]; stat: [0]
// flushes, [1] candidate pairs evaluated.  rng == nullptr: one bucket.  Labels are in [0, K) (checked on the host), so every bin
// index is below T K K; every staged index is below n.
template <bool LDS>
__global__ __launch_bounds__(CO_THREADS) void co_tally_kernel(const double* __restrict__ sx, const double* __restrict__ sy, const int32_t* __restrict__ slab,
                                                             const int64_t* __restrict__ rng, int64_t n, int K, int T, const double* __restrict__ thr2,
                                                             int64_t tiles, int64_t tiles_per_wg, int64_t flush_bound, co_u64* __restrict__ sym,
                                                             co_u64* __restrict__ stat) {
    extern __shared__ __align__(16) unsigned char co_lds[];
    double* cx = reinterpret_cast<double*>(co_lds);
    double* cy = cx + COOCCUR_TILE;
    double* th = cy + COOCCUR_TILE;
    int32_t* cl = reinterpret_cast<int32_t*>(th + COOCCUR_MAX_T + 2);
    uint32_t* bins = reinterpret_cast<uint32_t*>(co_lds + COOCCUR_STAGE_BYTES);
    const int KK = K * K, nbins = T * KK;
    const int split = (int)gridDim.y;
    for (int i = threadIdx.x; i <= T; i += CO_THREADS) th[i] = thr2[i];
    if (LDS)
        for (int i = threadIdx.x; i < nbins; i += CO_THREADS) bins[i] = 0u;
    __syncthreads();
    const double lo2 = th[0], hi2 = th[T];
    int steps = 0;   // halvings of an interval search: the least with 2^steps >= T
    while ((1 << steps) < T) ++steps;
    int64_t since = 0, flushes = 0, pairs = 0;   // the same in every thread
    const int64_t t0 = (int64_t)blockIdx.x * tiles_per_wg, t1 = std::min(t0 + tiles_per_wg, tiles);
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t p0 = tile * COOCCUR_TILE, p1 = std::min<int64_t>(p0 + COOCCUR_TILE, n);
        const int64_t pos = p0 + threadIdx.x;
        const bool active = pos < p1;
        const double mx = active ? sx[pos] : 0.0, my = active ? sy[pos] : 0.0;
        const int ma = active ? slab[pos] : 0;
        const int64_t A1 = rng ? rng[3 * tile] : n, B0 = rng ? rng[3 * tile + 1] : n, B1 = rng ? rng[3 * tile + 2] : n;
        const int64_t nA = (A1 - p0 + COOCCUR_TILE - 1) / COOCCUR_TILE, nB = (B1 - B0 + COOCCUR_TILE - 1) / COOCCUR_TILE;
        for (int64_t c = blockIdx.y; c < nA + nB; c += split) {
            const int64_t q0 = c < nA ? p0 + c * COOCCUR_TILE : B0 + (c - nA) * COOCCUR_TILE;
            const int64_t q1 = std::min<int64_t>(q0 + COOCCUR_TILE, c < nA ? A1 : B1);
            const int len = (int)(q1 - q0);
            const int64_t add = (p1 - p0) * len;
            __syncthreads();   // the stage before is done with the staging and with its atomics
            if (LDS && cooccur_must_flush(since, add, flush_bound)) {
                for (int i = threadIdx.x; i < nbins; i += CO_THREADS) {   // (a thread re-zeroes only what it read: the barrier below suffices)
                    const uint32_t v = bins[i];
                    if (v) {
                        atomicAdd(&sym[i], (co_u64)v);
                        bins[i] = 0u;
                    }
                }
                since = 0;
                ++flushes;
            }
            since += add;
            pairs += add;
            if ((int)threadIdx.x < len) {
                cx[threadIdx.x] = sx[q0 + threadIdx.x];
                cy[threadIdx.x] = sy[q0 + threadIdx.x];
                cl[threadIdx.x] = slab[q0 + threadIdx.x];
            }
            __syncthreads();
            if (active) {
                // staged slots from jmin on lie at later sorted positions (jmin > 0 only where the tile meets itself)
                const int jmin = (int)std::max<int64_t>(std::min<int64_t>(pos + 1 - q0, len), 0);
                // CO_BATCH slots are read into registers before any of them is tested, so the LDS reads of a batch are in flight
                // together instead of one at a time behind the bins' atomics; a slot past len holds an older tile or nothing: the
                // j < len test leaves it out
                for (int j0 = 0; j0 < len; j0 += CO_BATCH) {
                    double bx[CO_BATCH], by[CO_BATCH];
#pragma unroll
                    for (int u = 0; u < CO_BATCH; ++u) {
                        bx[u] = cx[j0 + u];
                        by[u] = cy[j0 + u];
                    }
                    double d2[CO_BATCH];
                    bool in[CO_BATCH];
                    bool any = false;
#pragma unroll
                    for (int u = 0; u < CO_BATCH; ++u) {
                        const int j = j0 + u;
                        const double dx = mx - bx[u], dy = my - by[u];
                        d2[u] = dx * dx + dy * dy;
                        in[u] = !(d2[u] > hi2 || d2[u] <= lo2 || j < jmin || j >= len);
                        any |= in[u];
                    }
                    if (!any) continue;
                    // the batch's interval searches side by side, `steps` halvings each (2^steps >= T), so their LDS reads overlap
                    // instead of queueing behind one another; th[lo] < d2 <= th[hi] holds for a pair that is in, and a pair that is
                    // not only ever reads th[0 .. T]
                    int lo[CO_BATCH], hi[CO_BATCH], lb[CO_BATCH];
#pragma unroll
                    for (int u = 0; u < CO_BATCH; ++u) {
                        lo[u] = 0;
                        hi[u] = T;
                        lb[u] = cl[j0 + u];
                    }
                    for (int s = 0; s < steps; ++s) {
#pragma unroll
                        for (int u = 0; u < CO_BATCH; ++u) {
                            const int mid = (lo[u] + hi[u]) >> 1;   // hi - lo == 1: mid == lo, th[lo] < d2, nothing moves
                            const bool up = th[mid] < d2[u];
                            lo[u] = up ? mid : lo[u];
                            hi[u] = up ? hi[u] : mid;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < CO_BATCH; ++u) {
                        if (!in[u]) continue;
                        const int b = lb[u];
                        const int bin = lo[u] * KK + (ma < b ? ma * K + b : b * K + ma);
                        if (LDS) atomicAdd(&bins[bin], 1u);
                        else atomicAdd(&sym[bin], 1ull);
                    }
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        if (since > 0) {
            for (int i = threadIdx.x; i < nbins; i += CO_THREADS) {
                const uint32_t v = bins[i];
                if (v) atomicAdd(&sym[i], (co_u64)v);
            }
            ++flushes;
        }
    }
    if (threadIdx.x == 0) {
        if (flushes) atomicAdd(&stat[0], (co_u64)flushes);
        if (pairs) atomicAdd(&stat[1], (co_u64)pairs);
    }
}

// ---- 3. the ordered table -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CO_THREADS) void co_epilogue_kernel(const co_u64* __restrict__ sym, int K, int64_t total, int64_t* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * CO_THREADS + threadIdx.x;
    if (q >= total) return;
    const int64_t KK = (int64_t)K * K, t = q / KK, a = q % K, b = (q / K) % K;
    const co_u64 v = sym[t * KK + std::min(a, b) * K + std::max(a, b)];
    out[q] = (int64_t)(a == b ? 2 * v : v);
}

// =================================================================================================================================
namespace {
inline unsigned co_blocks(int64_t n) { return (unsigned)((n + CO_THREADS - 1) / CO_THREADS); }

// stage timer of sgl_c_cooccur's stage_ms: events around a stage when the caller asked for the times
struct CoTimer {
    hipStream_t s;
    double* ms;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CoTimer(hipStream_t s_, double* ms_) : s(s_), ms(ms_) {
        if (ms && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) { (void)hipGetLastError(); ms = nullptr; }
    }
    ~CoTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    void begin() { if (ms) (void)hipEventRecord(e0, s); }
    void end(int stage) {
        if (!ms) return;
        float t = 0.f;
        if (hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) ms[stage] += t;
        else (void)hipGetLastError();
    }
};

template <bool LDS>
int co_tally_launch(sgl_ctx* c, const CooccurPlan& P, const double* sx, const double* sy, const int32_t* slab, const int64_t* rng, int64_t n, int K, int T,
                    const double* thr2, co_u64* sym, co_u64* stat) {
    if (LDS) SGLCHK((sgl_allow_dynamic_lds<&co_tally_kernel<true>>((int)COOCCUR_LDS_BYTES)));
    co_tally_kernel<LDS><<<dim3((unsigned)P.wgs, (unsigned)P.split), dim3(CO_THREADS), (size_t)P.lds_bytes, c->stream>>>(
        sx, sy, slab, rng, n, K, T, thr2, P.tiles, P.tiles_per_wg, P.flush_pairs, sym, stat);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}
}   // namespace

int sgl_cooccur_args_check(const char* who, const double* c1, const double* c2, int64_t n, const int32_t* lab, int64_t K, const double* r, int64_t T,
                           int64_t grid_mode, int64_t bin_path, int64_t flush_pairs, double* thr2) {
    int64_t at = -1, val = 0;
    CooccurArgError e = cooccur_check_call(c1, c2, n, lab, K, r, T, thr2, &at, &val);
    if (e == COOCCUR_ARGS_OK) e = cooccur_check_knobs(grid_mode, bin_path, flush_pairs, &at, &val);
    static const char* knob[3] = {"grid_mode", "bin_path", "flush_pairs"};
    switch (e) {
    case COOCCUR_ARGS_OK: return SGL_OK;
    case COOCCUR_ARGS_NULL: sgl_set_error("%s: NULL c1, c2, lab or r", who); break;
    case COOCCUR_ARGS_N: sgl_set_error("%s: n = %lld: at least one point", who, (long long)n); break;
    case COOCCUR_ARGS_COORD: sgl_set_error("%s: c%lld[%lld] = %g is not finite", who, (long long)val, (long long)at, val == 1 ? c1[at] : c2[at]); break;
    case COOCCUR_ARGS_K: sgl_set_error("%s: K = %lld is outside [1, %d]", who, (long long)K, COOCCUR_MAX_K); break;
    case COOCCUR_ARGS_LABEL: sgl_set_error("%s: lab[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)K); break;
    case COOCCUR_ARGS_T: sgl_set_error("%s: T = %lld intervals is outside [1, %d]", who, (long long)T, COOCCUR_MAX_T); break;
    case COOCCUR_ARGS_R: sgl_set_error("%s: r[%lld] = %g is negative or not finite", who, (long long)at, r[at]); break;
    case COOCCUR_ARGS_THR2:
        sgl_set_error("%s: the square of r[%lld] = %g is not finite or not above the square of r[%lld]: the thresholds ascend strictly", who,
                      (long long)at, r[at], (long long)(at > 0 ? at - 1 : 0));
        break;
    case COOCCUR_ARGS_KNOB:
        if (at == 2) sgl_set_error("%s: flush_pairs = %lld is negative or above 2^32 - 1", who, (long long)val);
        else sgl_set_error("%s: %s = %lld is none of 0, 1, 2", who, knob[at], (long long)val);
        break;
    }
    return SGL_EINVAL;
}

static int co_run(sgl_ctx* c, const double* c1, const double* c2, int64_t n, const int32_t* lab, int K, const double* r, const double* thr2, int T,
                  int grid_mode, int bin_path, int64_t flush_pairs, int64_t* counts, double* stage_ms) {
    hipStream_t s = c->stream;
    if (stage_ms) std::fill(stage_ms, stage_ms + 3, 0.0);
    CoTimer tm(s, stage_ms);
    const int64_t nbins = (int64_t)T * K * K;
    DevBuf<double> dx, dy, sx, sy, dthr, dpart;
    DevBuf<int32_t> dlab, slab;
    DevBuf<uint64_t> keys, skeys;
    DevBuf<uint32_t> iota, sidx;
    DevBuf<int64_t> rng, dout;
    DevBuf<co_u64> sym;   // the bins, then the two counters
    DevBuf<char> tmp;
    SGLCHK(dx.alloc((size_t)n));
    SGLCHK(dy.alloc((size_t)n));
    SGLCHK(dlab.alloc((size_t)n));
    SGLCHK(dthr.alloc((size_t)T + 1));
    SGLCHK(sym.alloc((size_t)nbins + 2));
    SGLCHK(dout.alloc((size_t)nbins));
    HIPCHK(hipMemcpyAsync(dx.p, c1, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dy.p, c2, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dlab.p, lab, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dthr.p, thr2, sizeof(double) * ((size_t)T + 1), hipMemcpyHostToDevice, s));
    // stage 0: extent, sort, gather, ranges
    tm.begin();
    const unsigned eb = std::min<unsigned>(co_blocks(n), COOCCUR_EXTENT_BLOCKS);
    SGLCHK(dpart.alloc(4 * (size_t)eb));
    double hp[4 * COOCCUR_EXTENT_BLOCKS];
    {
        Phase ph(c, SGL_PH_SCALE);
        co_extent_kernel<<<dim3(eb), dim3(CO_THREADS), 0, s>>>(dx.p, dy.p, n, dpart.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(hp, dpart.p, sizeof(double) * 4 * eb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double ext[4] = {hp[0], hp[1], hp[2], hp[3]};
    for (unsigned b = 1; b < eb; ++b) {
        ext[0] = std::min(ext[0], hp[4 * b]);
        ext[1] = std::max(ext[1], hp[4 * b + 1]);
        ext[2] = std::min(ext[2], hp[4 * b + 2]);
        ext[3] = std::max(ext[3], hp[4 * b + 3]);
    }
    const CooccurGrid g = cooccur_grid(ext[0], ext[1], ext[2], ext[3], r[T], grid_mode);
    CooccurPlan P;
    cooccur_plan(n, K, T, g.mode, bin_path, flush_pairs, &P);
    const double *px = dx.p, *py = dy.p;
    const int32_t* pl = dlab.p;
    if (g.mode == 2) {
        SGLCHK(keys.alloc((size_t)n));
        SGLCHK(skeys.alloc((size_t)n));
        SGLCHK(iota.alloc((size_t)n));
        SGLCHK(sidx.alloc((size_t)n));
        SGLCHK(sx.alloc((size_t)n));
        SGLCHK(sy.alloc((size_t)n));
        SGLCHK(slab.alloc((size_t)n));
        SGLCHK(rng.alloc(3 * (size_t)P.tiles));
        Phase ph(c, SGL_PH_SCALE);
        co_keys_kernel<<<dim3(co_blocks(n)), dim3(CO_THREADS), 0, s>>>(dx.p, dy.p, n, g, keys.p, iota.p);
        HIPCHK(hipGetLastError());
        int end_bit = 1;
        while (end_bit < 64 && ((uint64_t)1 << end_bit) <= (uint64_t)(g.W * g.H)) ++end_bit;
        size_t bytes = 0;   // LSD radix sort is stable: a bucket's members stay in ascending index order
        HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, keys.p, skeys.p, iota.p, sidx.p, (int)n, 0, end_bit, s));
        SGLCHK(tmp.alloc(bytes));
        HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, keys.p, skeys.p, iota.p, sidx.p, (int)n, 0, end_bit, s));
        co_gather_kernel<<<dim3(co_blocks(n)), dim3(CO_THREADS), 0, s>>>(sidx.p, dx.p, dy.p, dlab.p, n, sx.p, sy.p, slab.p);
        HIPCHK(hipGetLastError());
        co_ranges_kernel<<<dim3(co_blocks(P.tiles)), dim3(CO_THREADS), 0, s>>>(skeys.p, n, g.W, g.H, P.tiles, rng.p);
        HIPCHK(hipGetLastError());
        px = sx.p;
        py = sy.p;
        pl = slab.p;
    }
    tm.end(0);
    // stage 1: the tally
    tm.begin();
    HIPCHK(hipMemsetAsync(sym.p, 0, sizeof(co_u64) * ((size_t)nbins + 2), s));
    {
        Phase ph(c, SGL_PH_SCALE);
        if (P.path == 1) SGLCHK(co_tally_launch<true>(c, P, px, py, pl, rng.p, n, K, T, dthr.p, sym.p, sym.p + nbins));
        else SGLCHK(co_tally_launch<false>(c, P, px, py, pl, rng.p, n, K, T, dthr.p, sym.p, sym.p + nbins));
    }
    tm.end(1);
    // stage 2: the ordered table and its way home
    tm.begin();
    {
        Phase ph(c, SGL_PH_SCALE);
        co_epilogue_kernel<<<dim3(co_blocks(nbins)), dim3(CO_THREADS), 0, s>>>(sym.p, K, nbins, dout.p);
        HIPCHK(hipGetLastError());
    }
    std::vector<int64_t> h((size_t)nbins);
    co_u64 hstat[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h.data(), dout.p, sizeof(int64_t) * (size_t)nbins, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hstat, sym.p + nbins, sizeof(hstat), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    tm.end(2);
    std::copy(h.begin(), h.end(), counts);
    const int64_t v[8] = {g.mode, g.W, g.H, P.path, P.lds_bytes, P.wgs * P.split, (int64_t)hstat[0], (int64_t)hstat[1]};
    std::copy(v, v + 8, c->cooccur_last);
    return SGL_OK;
}

int sgl_cooccur_core(sgl_ctx* c, const double* c1, const double* c2, int64_t n, const int32_t* lab, int K, const double* r, const double* thr2, int T,
                     int grid_mode, int bin_path, int64_t flush_pairs, int64_t* counts, double* stage_ms) {
    const int rc = co_run(c, c1, c2, n, lab, K, r, thr2, T, grid_mode, bin_path, flush_pairs, counts, stage_ms);
    // every return path waits for the stream before the buffers (and the host arrays) go
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("cooccur: HIP call failed: %s", hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}
