// Kernels of sgl_upload_typed (include/singlet_hip.h): the arrays of a SciPy / AnnData / torch CSR or CSC, as the caller
// holds them, become the resident image -- double values, int32 indices ascending within a major slice, int64 offsets.
//
//   convert   one grid-stride kernel per (source type -> slot).  Every source element is read once: the widening, the
//             finite / inexact / integral tests of a value, the 64-bit range test of an index and the monotonicity test
//             of a device-space offset array ride on that one read.  Two elements per thread and load where both
//             pointers are aligned for it.  What a thread found goes out through one atomicOr.
//   mark      a wave per major slice, as validate_csc_kernel walks them: is any index below its predecessor?  Marked
//             slices of at most SGL_INGEST_LDS_CAP entries form the short list, the longer ones the long list (two scans).
//   LDS sort  one workgroup per short slice: (index << 32 | local position) as ONE 64-bit key per entry, padded to a
//             power of two with INT32_MAX indices, bitonic sort, then the values are gathered by position through
//             registers and both arrays written back in place.  8 LDS bytes per entry (the pair form would take 12).
//   long path the long slices are gathered into a compact buffer, sorted by hipcub's segmented radix sort in batches of
//             fewer than 2^31 entries (ingest_batch_edges, ingest_host.h), and scattered back.
//
// No atomics on floating-point data; a slice's result depends on its own entries only, never on the launch.  Streaming
// index work, HBM-bound: a canonical matrix pays the convert pass and one validator pass and nothing else.
#include "sgl_internal.h"
#include "ingest_host.h"
#include <hipcub/hipcub.hpp>
#include <type_traits>

namespace {

constexpr int INGEST_THREADS = 256;
constexpr int INGEST_GRID_CAP = 8192;                              // as all_finite_kernel: 8192 x 256 elements per pass
constexpr int INGEST_PER_THREAD = SGL_INGEST_LDS_CAP / INGEST_THREADS;   // values a thread carries through the write-back
static_assert(SGL_INGEST_LDS_CAP % INGEST_THREADS == 0 && (SGL_INGEST_LDS_CAP & (SGL_INGEST_LDS_CAP - 1)) == 0, "capacity: a power of two");
static_assert(2 * SGL_INGEST_LDS_CAP * 8 <= 160 * 1024, "two workgroups of the LDS sort must fit a CU's 160 KiB");

template <typename T>
struct alignas(2 * sizeof(T)) Pair {
    T a, b;
};

// ---- values -> double.  flag |= FINITE on NaN / Inf, INEXACT on an int64 beyond +-2^53, FRACTION on a value with a fraction
template <typename S>
__device__ __forceinline__ double widen_value(S v, int& bad) {
    const double d = (double)v;
    if constexpr (sizeof(S) == 8 && !std::is_floating_point<S>::value) {
        if (v > ((int64_t)1 << 53) || v < -((int64_t)1 << 53)) bad |= SGL_INGEST_INEXACT;
    }
    if constexpr (std::is_floating_point<S>::value) {
        if (!(__builtin_fabs(d) < __builtin_inf())) bad |= SGL_INGEST_FINITE;
        else if (__builtin_trunc(d) != d) bad |= SGL_INGEST_FRACTION;
    }
    return d;
}

// ---- int64 index -> int32, range-tested as a 64-bit number; an index out of range is never stored as its low 32 bits:
// a negative one becomes -1 and one at or above the extent INT32_MAX (>= extent), which the validator calls out of range
// too and which compare with their in-range neighbours as the 64-bit numbers did
struct NarrowIndex {
    int64_t extent;
    __device__ __forceinline__ int32_t operator()(int64_t v, int& bad) const {
        if (v < 0) { bad |= SGL_INGEST_RANGE; return -1; }
        if (v >= extent) { bad |= SGL_INGEST_RANGE; return INT32_MAX; }
        return (int32_t)v;
    }
};
template <typename S>
struct WidenValue {
    __device__ __forceinline__ double operator()(S v, int& bad) const { return widen_value<S>(v, bad); }
};

// dst[e] = op(src[e]) for e in [0, n).  VEC = 2: thread t of a pass takes elements 2t and 2t + 1 by one load and one
// store (both pointers aligned to a pair); the grid is capped so that a pass covers 8192 x 256 ELEMENTS either way.
// src may be dst (the F64 values of a HOST call are tested where they landed).
template <typename S, typename D, int VEC, typename Op>
__global__ __launch_bounds__(INGEST_THREADS) void convert_kernel(const S* src, D* dst, int64_t n, Op op, int* __restrict__ flag) {
    int bad = 0;
    const int64_t nv = (n + VEC - 1) / VEC;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
        if (VEC == 2 && 2 * v + 1 < n) {
            const Pair<S> in = reinterpret_cast<const Pair<S>*>(src)[v];
            Pair<D> out;
            out.a = op(in.a, bad);
            out.b = op(in.b, bad);
            reinterpret_cast<Pair<D>*>(dst)[v] = out;
        } else {
            const int64_t e = VEC * v;   // VEC = 1, or the odd last element
            dst[e] = op(src[e], bad);
        }
    }
    if (bad) atomicOr(flag, bad);
}

template <typename S, typename D, typename Op>
int launch_convert(hipStream_t s, const S* src, D* dst, int64_t n, Op op, int* flag) {
    if (n <= 0) return SGL_OK;
    const bool wide = ((uintptr_t)src % (2 * sizeof(S))) == 0 && ((uintptr_t)dst % (2 * sizeof(D))) == 0;
    const int vec = wide ? 2 : 1;
    const int64_t nv = (n + vec - 1) / vec;
    const unsigned grid = (unsigned)std::min<int64_t>((nv + INGEST_THREADS - 1) / INGEST_THREADS, INGEST_GRID_CAP / vec);
    if (wide) convert_kernel<S, D, 2, Op><<<dim3(grid), dim3(INGEST_THREADS), 0, s>>>(src, dst, n, op, flag);
    else convert_kernel<S, D, 1, Op><<<dim3(grid), dim3(INGEST_THREADS), 0, s>>>(src, dst, n, op, flag);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

// ---- offsets -> int64.  check: ptr[0] == 0 and ptr[q] <= ptr[q + 1] (the neighbour is read a second time, from cache)
template <typename S>
__global__ __launch_bounds__(INGEST_THREADS) void offsets_kernel(const S* __restrict__ src, int64_t n1, int64_t* __restrict__ dst, int check,
                                                                 int* __restrict__ flag) {
    int bad = 0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n1; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = (int64_t)src[q];
        dst[q] = v;
        if (check && (q == 0 ? v != 0 : (int64_t)src[q - 1] > v)) bad = SGL_INGEST_OFFSETS;
    }
    if (bad) atomicOr(flag, bad);
}

// ---- mark: fs[c] = 1 when slice c is out of order and fits the LDS sort, fl[c] = 1 when it is out of order and does not.
// Equal neighbours are not "out of order": no sort separates a duplicate, the second validator pass refuses it.
__global__ __launch_bounds__(256) void mark_kernel(const int32_t* __restrict__ idx, const int64_t* __restrict__ p, int64_t n_major,
                                                   int64_t* __restrict__ fs, int64_t* __restrict__ fl) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t c = wave; c < n_major; c += nwaves) {
        const int64_t lo = p[c], hi = p[c + 1];
        int bad = 0;
        for (int64_t e = lo + 1 + lane; e < hi; e += 64)
            if (idx[e - 1] > idx[e]) bad = 1;
        bad = __any(bad);
        if (lane == 0) {
            const bool fits = hi - lo <= SGL_INGEST_LDS_CAP;
            fs[c] = bad && fits ? 1 : 0;
            fl[c] = bad && !fits ? 1 : 0;
        }
    }
}

// the lists from the scans of the marks: slice c is entry ps[c] of the short list or entry pl[c] of the long one
__global__ void lists_kernel(const int64_t* __restrict__ p, int64_t n_major, const int64_t* __restrict__ fs, const int64_t* __restrict__ fl,
                             const int64_t* __restrict__ ps, const int64_t* __restrict__ pl, int32_t* __restrict__ short_list,
                             int32_t* __restrict__ long_list, int64_t* __restrict__ long_len) {
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_major; c += (int64_t)gridDim.x * blockDim.x) {
        if (fs[c]) short_list[ps[c]] = (int32_t)c;
        if (fl[c]) {
            long_list[pl[c]] = (int32_t)c;
            long_len[pl[c]] = p[c + 1] - p[c];
        }
    }
}

// ---- LDS sort: workgroup w sorts slice list[w] (2 <= length <= SGL_INGEST_LDS_CAP) in place.  The slice is padded to
// its own power of two Q; pads carry INT32_MAX and a position past the slice, so they end behind every real entry (a
// real index is below n_minor <= INT32_MAX).
__global__ __launch_bounds__(INGEST_THREADS) void lds_sort_kernel(int32_t* __restrict__ idx, double* __restrict__ x, const int64_t* __restrict__ p,
                                                                   const int32_t* __restrict__ list) {
    __shared__ unsigned long long keys[SGL_INGEST_LDS_CAP];
    const int64_t lo = p[list[blockIdx.x]];
    const int len = (int)(p[list[blockIdx.x] + 1] - lo);
    int Q = 2;
    while (Q < len) Q <<= 1;
    for (int t = threadIdx.x; t < Q; t += INGEST_THREADS)
        keys[t] = ((unsigned long long)(uint32_t)(t < len ? idx[lo + t] : INT32_MAX) << 32) | (uint32_t)t;
    __syncthreads();
    for (int size = 2; size <= Q; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < Q; t += INGEST_THREADS) {
                const int u = t ^ stride;
                if (u > t) {
                    const unsigned long long a = keys[t], b = keys[u];
                    if ((a > b) == ((t & size) == 0)) { keys[t] = b; keys[u] = a; }
                }
            }
            __syncthreads();
        }
    // every value is read into a register before the barrier, every slot written after it: in place without a copy
    double v[INGEST_PER_THREAD];
#pragma unroll
    for (int j = 0; j < INGEST_PER_THREAD; ++j) {
        const int t = threadIdx.x + j * INGEST_THREADS;
        v[j] = t < len ? x[lo + (uint32_t)keys[t]] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < INGEST_PER_THREAD; ++j) {
        const int t = threadIdx.x + j * INGEST_THREADS;
        if (t < len) {
            x[lo + t] = v[j];
            idx[lo + t] = (int32_t)(keys[t] >> 32);
        }
    }
}

// ---- long path: segment g of a batch is slice list[g]; off[g] its first entry in the compact buffers
template <bool BACK>
__global__ __launch_bounds__(256) void long_move_kernel(int32_t* __restrict__ idx, double* __restrict__ x, const int64_t* __restrict__ p,
                                                        const int32_t* __restrict__ list, const int64_t* __restrict__ off, int64_t nseg,
                                                        int32_t* __restrict__ ki, double* __restrict__ kx) {
    for (int64_t g = blockIdx.x; g < nseg; g += gridDim.x) {
        const int64_t lo = p[list[g]], o = off[g], len = off[g + 1] - o;
        for (int64_t e = threadIdx.x; e < len; e += blockDim.x) {
            if (BACK) { idx[lo + e] = ki[o + e]; x[lo + e] = kx[o + e]; }
            else { ki[o + e] = idx[lo + e]; kx[o + e] = x[lo + e]; }
        }
    }
}

unsigned wave_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, 4096)); }

}  // namespace

extern "C" int sgl_ingest_batch_edges(const int64_t* len, int64_t n, int64_t max_entries, int64_t* cut, int64_t* n_runs) {
    if (!len || !cut || !n_runs || n < 0 || max_entries < 1) { sgl_set_error("sgl_ingest_batch_edges: bad arguments"); return SGL_EINVAL; }
    for (int64_t s = 0; s < n; ++s)
        if (len[s] < 0) { sgl_set_error("sgl_ingest_batch_edges: negative length at %lld", (long long)s); return SGL_EINVAL; }
    *n_runs = ingest_batch_edges(len, n, max_entries, cut);
    return SGL_OK;
}

int k_ingest_values(hipStream_t s, const void* src, int x_type, double* dst, int64_t n, int* flag) {
    switch (x_type) {
    case SGL_T_F64: return launch_convert(s, static_cast<const double*>(src), dst, n, WidenValue<double>(), flag);
    case SGL_T_F32: return launch_convert(s, static_cast<const float*>(src), dst, n, WidenValue<float>(), flag);
    case SGL_T_I32: return launch_convert(s, static_cast<const int32_t*>(src), dst, n, WidenValue<int32_t>(), flag);
    default: return launch_convert(s, static_cast<const int64_t*>(src), dst, n, WidenValue<int64_t>(), flag);
    }
}

int k_ingest_narrow_index(hipStream_t s, const int64_t* src, int32_t* dst, int64_t n, int64_t extent, int* flag) {
    return launch_convert(s, src, dst, n, NarrowIndex{extent}, flag);
}

int k_ingest_offsets(hipStream_t s, const void* src, int ptr_type, int64_t n1, int64_t* dst, int check, int* flag) {
    const unsigned grid = (unsigned)std::min<int64_t>((n1 + INGEST_THREADS - 1) / INGEST_THREADS, INGEST_GRID_CAP);
    if (ptr_type == SGL_T_I32) offsets_kernel<<<dim3(grid), dim3(INGEST_THREADS), 0, s>>>(static_cast<const int32_t*>(src), n1, dst, check, flag);
    else offsets_kernel<<<dim3(grid), dim3(INGEST_THREADS), 0, s>>>(static_cast<const int64_t*>(src), n1, dst, check, flag);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}

// Sorts the (index, value) pairs of every out-of-order major slice of M by index, in place; M.i holds indices in
// [0, M.nrow) (the validator found no range defect).  *n_short / *n_long: slices sorted by either path.  Synchronises.
int k_ingest_sort_slices(sgl_ctx* c, DevCSC& M, int64_t* n_short, int64_t* n_long) {
    hipStream_t s = c->stream;
    const int64_t n = M.ncol;
    *n_short = *n_long = 0;
    DevBuf<int64_t> fs, fl, ps, pl, long_len;
    DevBuf<int32_t> short_list, long_list;
    SGLCHK(fs.alloc((size_t)n));
    SGLCHK(fl.alloc((size_t)n));
    SGLCHK(ps.alloc((size_t)n + 1));
    SGLCHK(pl.alloc((size_t)n + 1));
    mark_kernel<<<dim3(wave_blocks(n)), dim3(256), 0, s>>>(M.i, M.p, n, fs.p, fl.p);
    HIPCHK(hipGetLastError());
    SGLCHK(k_exclusive_scan(c, fs.p, ps.p, n));
    SGLCHK(k_scan_total(s, fs.p, ps.p, n));
    SGLCHK(k_exclusive_scan(c, fl.p, pl.p, n));
    SGLCHK(k_scan_total(s, fl.p, pl.p, n));
    int64_t ns = 0, nl = 0;
    HIPCHK(hipMemcpyAsync(&ns, ps.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&nl, pl.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ns + nl == 0) return SGL_OK;
    SGLCHK(short_list.alloc((size_t)ns));
    SGLCHK(long_list.alloc((size_t)nl));
    SGLCHK(long_len.alloc((size_t)nl));
    lists_kernel<<<dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, s>>>(M.p, n, fs.p, fl.p, ps.p, pl.p, short_list.p,
                                                                                               long_list.p, long_len.p);
    HIPCHK(hipGetLastError());
    if (ns > 0) {   // one workgroup per listed slice; at most 2^31 - 1 of them (n <= INT32_MAX), which a grid's x extent holds
        lds_sort_kernel<<<dim3((unsigned)ns), dim3(INGEST_THREADS), 0, s>>>(M.i, M.x, M.p, short_list.p);
        HIPCHK(hipGetLastError());
    }
    if (nl > 0) {
        std::vector<int64_t> len((size_t)nl), cut((size_t)nl + 1), off;
        HIPCHK(hipMemcpyAsync(len.data(), long_len.p, sizeof(int64_t) * (size_t)nl, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const int64_t runs = ingest_batch_edges(len.data(), nl, (int64_t)INT32_MAX, cut.data());
        int64_t max_entries = 0, max_seg = 0;
        for (int64_t b = 0; b < runs; ++b) {
            int64_t sum = 0;
            for (int64_t g = cut[(size_t)b]; g < cut[(size_t)b + 1]; ++g) sum += len[(size_t)g];
            max_entries = std::max(max_entries, sum);
            max_seg = std::max(max_seg, cut[(size_t)b + 1] - cut[(size_t)b]);
        }
        if (max_entries > INT32_MAX) { sgl_set_error("ingest: a major slice holds %lld entries", (long long)max_entries); return SGL_EINVAL; }
        DevBuf<int32_t> ki, ki2;
        DevBuf<double> kx, kx2;
        DevBuf<int64_t> doff;
        DevBuf<char> tmp;
        SGLCHK(ki.alloc((size_t)max_entries));
        SGLCHK(ki2.alloc((size_t)max_entries));
        SGLCHK(kx.alloc((size_t)max_entries));
        SGLCHK(kx2.alloc((size_t)max_entries));
        SGLCHK(doff.alloc((size_t)max_seg + 1));
        int end_bit = 1;
        while (((int64_t)1 << end_bit) < (int64_t)M.nrow && end_bit < 31) ++end_bit;
        size_t tmp_cap = 0;
        for (int64_t b = 0; b < runs; ++b) {
            const int64_t g0 = cut[(size_t)b], nseg = cut[(size_t)b + 1] - g0;
            off.assign((size_t)nseg + 1, 0);
            for (int64_t g = 0; g < nseg; ++g) off[(size_t)g + 1] = off[(size_t)g] + len[(size_t)(g0 + g)];
            const int64_t tot = off[(size_t)nseg];
            HIPCHK(hipMemcpyAsync(doff.p, off.data(), sizeof(int64_t) * ((size_t)nseg + 1), hipMemcpyHostToDevice, s));
            const unsigned grid = (unsigned)std::min<int64_t>(nseg, 65535);
            long_move_kernel<false><<<dim3(grid), dim3(256), 0, s>>>(M.i, M.x, M.p, long_list.p + g0, doff.p, nseg, ki.p, kx.p);
            HIPCHK(hipGetLastError());
            size_t bytes = 0;
            HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, bytes, ki.p, ki2.p, kx.p, kx2.p, (int)tot, (int)nseg, doff.p, doff.p + 1, 0,
                                                               end_bit, s));
            if (bytes > tmp_cap) {
                HIPCHK(hipStreamSynchronize(s));
                SGLCHK(tmp.alloc(bytes));
                tmp_cap = bytes;
            }
            HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(tmp.p, bytes, ki.p, ki2.p, kx.p, kx2.p, (int)tot, (int)nseg, doff.p, doff.p + 1, 0,
                                                               end_bit, s));
            long_move_kernel<true><<<dim3(grid), dim3(256), 0, s>>>(M.i, M.x, M.p, long_list.p + g0, doff.p, nseg, ki2.p, kx2.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));   // `off` is rewritten for the next batch
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    *n_short = ns;
    *n_long = nl;
    return SGL_OK;
}
