// Simulated doublets: S[:, s] = A[:, parent_a[s]] + A[:, parent_b[s]], the sum of two sparse columns of a resident CSC as
// a new CSC (include/singlet_hip.h, "Simulated doublets"; the host rules in doublet_host.h).  Three passes: the length of
// every merged column, the 64-bit exclusive scan of the lengths, the fill.
//
// One wave per simulated column, no sort and no atomics on the data.  Both parents are ascending, so the place of an
// entry in the merged column follows from counts alone: entry j of parent a, at row r, has j entries of a below it and
// lb_b = lower_bound(b, r) entries of b below it, of which the rows stored in BOTH parents must be counted once -- those
// are the shared rows among a[0 .. j), counted in order by a ballot and mbcnt within a chunk of 64 entries and by a
// wave-uniform carry from chunk to chunk.  The a-side writes all its entries (x_a + x_b, one IEEE addition, at a shared
// row), the b-side the unshared ones by the same formula over its own order.  Every slot of the column is written by
// exactly one lane, with plain vector stores.
//
// The searches run over the row indices of both parents.  A pair whose la + lb indices fit the cap (4 bytes each, 16 KiB
// at the default of 4096: ten waves' worth in the 160 KiB of a CU) is staged in LDS by its wave and searched there: a
// search reads one dword per lane per step at unrelated addresses, which is what the 64 banks are for, and a step that
// lands lanes l and l + 32 on one bank costs nothing (they are served in different halves).  A longer pair (a dense upload
// has columns of nrow entries) is searched where it lies, through the caches.  The path is a wave-uniform branch inside
// one kernel, so both produce the same bits by construction of the slot formula; sgl_doublets_info says which ran.
//
// HBM-bound index work: both parents read once (12 bytes an entry) plus the merged column written once (12 bytes an
// entry); the length pass reads the indices once more.
#include "sgl_internal.h"
#include "doublet_host.h"

namespace {

constexpr int DOUBLET_THREADS = 64;          // one wave per workgroup: a wave owns its LDS image, a barrier is the wave's own
constexpr int64_t DOUBLET_MAX_GRID = 4096;   // workgroups of a launch (16 a CU: more than the LDS lets reside); more columns go round the grid-stride loop

__device__ __forceinline__ int lane_rank(unsigned long long m) {   // set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

struct PairOf {
    int64_t a0, b0;
    int32_t la, lb;
};
__device__ __forceinline__ PairOf pair_of(const int64_t* __restrict__ p, const int32_t* __restrict__ pa, const int32_t* __restrict__ pb,
                                          int64_t s) {
    const int32_t ca = pa[s], cb = pb[s];
    PairOf r;
    r.a0 = p[ca];
    r.b0 = p[cb];
    r.la = (int32_t)(p[ca + 1] - r.a0);   // (a column holds at most nrow <= INT32_MAX entries)
    r.lb = (int32_t)(p[cb + 1] - r.b0);
    return r;
}

// Pass 1: len[s] = la + lb - shared(s).  The shorter parent's rows are looked up in the longer one, in global memory
// (the indices of a column stay in cache for the few steps of a search).  tally: [0] pairs on the LDS path, [1] on the
// long path, [2] shared rows over all pairs -- integer atomics, one per wave, whose order cannot change a bit.
__global__ __launch_bounds__(DOUBLET_THREADS) void doublet_len_kernel(const int32_t* __restrict__ idx, const int64_t* __restrict__ p,
                                                                      const int32_t* __restrict__ pa, const int32_t* __restrict__ pb,
                                                                      int64_t n, int64_t cap, int64_t* __restrict__ len,
                                                                      unsigned long long* __restrict__ tally) {
    const int lane = threadIdx.x;
    unsigned long long n_lds = 0, n_long = 0, n_shared = 0;
    for (int64_t s = blockIdx.x; s < n; s += gridDim.x) {
        const PairOf q = pair_of(p, pa, pb, s);
        const bool a_short = q.la <= q.lb;
        const int32_t* __restrict__ few = idx + (a_short ? q.a0 : q.b0);
        const int32_t* __restrict__ many = idx + (a_short ? q.b0 : q.a0);
        const int32_t nf = a_short ? q.la : q.lb, nm = a_short ? q.lb : q.la;
        int64_t shared = 0;
        for (int32_t base = 0; base < nf; base += 64) {
            const int32_t j = base + lane;
            bool hit = false;
            if (j < nf) {
                const int32_t row = few[j];
                const int32_t lo = doublet_lower_bound(many, nm, row);
                hit = lo < nm && many[lo] == row;
            }
            shared += __popcll(__ballot(hit));
            if (nf - base <= 64) break;   // (base + 64 would overflow at nf near INT32_MAX)
        }
        if (lane == 0) len[s] = (int64_t)q.la + (int64_t)q.lb - shared;
        if (doublet_pair_in_lds(q.la, q.lb, cap)) ++n_lds; else ++n_long;
        n_shared += (unsigned long long)shared;
    }
    if (lane == 0) {
        if (n_lds) atomicAdd(&tally[0], n_lds);
        if (n_long) atomicAdd(&tally[1], n_long);
        if (n_shared) atomicAdd(&tally[2], n_shared);
    }
}

// One side of one pair: the wave's lanes take the `ln` entries of `mine` (rows in sm[0 .. ln), values at xm) in chunks of
// 64 and look each row up in `other` (so[0 .. lo), values at xo_).  write_shared: the a-side, which writes the sum at a
// shared row; the b-side skips a shared row.  sm / so point into LDS or into global memory: the caller's branch decides,
// and the two instantiations differ in nothing else.  bad: the lowest simulated column with a non-finite sum.
template <bool WRITE_SHARED>
__device__ __forceinline__ void merge_side(const int32_t* sm, int32_t ln, const double* __restrict__ xm, const int32_t* so, int32_t lo,
                                           const double* __restrict__ xo_, int64_t o0, int64_t s, int lane, int32_t* __restrict__ io,
                                           double* __restrict__ xo, unsigned long long* __restrict__ bad) {
    int64_t shared = 0;   // shared rows among mine[0 .. base): wave-uniform
    for (int32_t base = 0; base < ln; base += 64) {
        const int32_t j = base + lane;
        const bool active = j < ln;
        int32_t row = 0, below = 0;
        bool hit = false;
        if (active) {
            row = sm[j];
            below = doublet_lower_bound(so, lo, row);
            hit = below < lo && so[below] == row;
        }
        const unsigned long long m = __ballot(hit);
        if (active && (WRITE_SHARED || !hit)) {
            const int64_t o = o0 + doublet_slot(j, below, shared + lane_rank(m));
            double v = xm[j];
            if (WRITE_SHARED && hit) {
                v = v + xo_[below];
                if (!isfinite(v)) atomicMin(bad, (unsigned long long)s);
            }
            io[o] = row;
            xo[o] = v;
        }
        shared += __popcll(m);
        if (ln - base <= 64) break;
    }
}

// Pass 3: the fill.  pn = the scanned lengths (n + 1 offsets).  Dynamic LDS: cap row indices.
__global__ __launch_bounds__(DOUBLET_THREADS) void doublet_fill_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                       const int64_t* __restrict__ p, const int32_t* __restrict__ pa,
                                                                       const int32_t* __restrict__ pb, const int64_t* __restrict__ pn,
                                                                       int64_t n, int64_t cap, int32_t* __restrict__ io,
                                                                       double* __restrict__ xo, unsigned long long* __restrict__ bad) {
    extern __shared__ int32_t rows_lds[];
    const int lane = threadIdx.x;
    for (int64_t s = blockIdx.x; s < n; s += gridDim.x) {
        const PairOf q = pair_of(p, pa, pb, s);
        const int64_t o0 = pn[s];
        const int32_t* ga = idx + q.a0;
        const int32_t* gb = idx + q.b0;
        if (doublet_pair_in_lds(q.la, q.lb, cap)) {   // wave-uniform: la + lb <= cap entries fit the image
            for (int32_t j = lane; j < q.la; j += 64) rows_lds[j] = ga[j];
            for (int32_t j = lane; j < q.lb; j += 64) rows_lds[q.la + j] = gb[j];
            __syncthreads();
            merge_side<true>(rows_lds, q.la, x + q.a0, rows_lds + q.la, q.lb, x + q.b0, o0, s, lane, io, xo, bad);
            merge_side<false>(rows_lds + q.la, q.lb, x + q.b0, rows_lds, q.la, x + q.a0, o0, s, lane, io, xo, bad);
            __syncthreads();   // the next pair's image overwrites this one
        } else {
            merge_side<true>(ga, q.la, x + q.a0, gb, q.lb, x + q.b0, o0, s, lane, io, xo, bad);
            merge_side<false>(gb, q.lb, x + q.b0, ga, q.la, x + q.a0, o0, s, lane, io, xo, bad);
        }
    }
}

}  // namespace

// S = the pair sums of A's columns (parent lists on the HOST, checked by the caller), built on c's stream with c's pool.  S
// comes in empty and leaves with its own p (and, unless count_only, i / x): a failure leaves what was allocated in S for
// the caller to free.  info[0 .. 4): pairs on the LDS path, on the long path, stored entries of S, shared rows.  *bad_col:
// the lowest simulated column whose sum is not finite, or -1 (always -1 when count_only).  Synchronises the stream.
int sgl_pair_columns_core(sgl_ctx* c, const DevCSC& A, const int32_t* parent_a, const int32_t* parent_b, int64_t n, int64_t lds_cap,
                          bool count_only, DevCSC& S, int64_t info[4], int64_t* bad_col) {
    hipStream_t s = c->stream;
    const int64_t cap = doublet_lds_cap(lds_cap);
    *bad_col = -1;
    S.nrow = A.nrow;
    S.ncol = (int32_t)n;
    DevBuf<int32_t> pa, pb;
    DevBuf<int64_t> len;
    DevBuf<unsigned long long> tally;   // [0 .. 3): the length pass's counts; [3]: the lowest column with a non-finite sum
    SGLCHK(pa.alloc((size_t)n));
    SGLCHK(pb.alloc((size_t)n));
    SGLCHK(len.alloc((size_t)n));
    SGLCHK(tally.alloc(4));
    SGLCHK(dev_alloc(&S.p, (size_t)n + 1));
    const unsigned long long tally0[4] = {0, 0, 0, ~0ull};
    unsigned long long got[4] = {0, 0, 0, ~0ull};
    int64_t nnz = 0;
    HIPCHK(hipMemcpyAsync(pa.p, parent_a, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(pb.p, parent_b, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(tally.p, tally0, sizeof(tally0), hipMemcpyHostToDevice, s));
    const unsigned grid = (unsigned)std::min<int64_t>(n, DOUBLET_MAX_GRID);
    {
        Phase ph(c, SGL_PH_SCALE);
        doublet_len_kernel<<<dim3(grid), dim3(DOUBLET_THREADS), 0, s>>>(A.i, A.p, pa.p, pb.p, n, cap, len.p, tally.p);
        HIPCHK(hipGetLastError());
        SGLCHK(k_exclusive_scan(c, len.p, S.p, n));
        SGLCHK(k_scan_total(s, len.p, S.p, n));
    }
    HIPCHK(hipMemcpyAsync(&nnz, S.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(got, tally.p, sizeof(got), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   // (also: the host images of the lists and of tally0 have been read)
    S.nnz = nnz;
    info[0] = (int64_t)got[0];
    info[1] = (int64_t)got[1];
    info[2] = nnz;
    info[3] = (int64_t)got[2];
    if (count_only) return SGL_OK;
    SGLCHK(dev_alloc(&S.x, (size_t)nnz));
    SGLCHK(dev_alloc(&S.i, (size_t)nnz));
    if (nnz == 0) return SGL_OK;
    const int lds_bytes = (int)(cap * (int64_t)sizeof(int32_t));   // at most 16 KiB: below the 48 KiB every kernel may take
    {
        Phase ph(c, SGL_PH_SCALE);
        doublet_fill_kernel<<<dim3(grid), dim3(DOUBLET_THREADS), lds_bytes, s>>>(A.x, A.i, A.p, pa.p, pb.p, S.p, n, cap, S.i, S.x,
                                                                                 tally.p + 3);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(got + 3, tally.p + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (got[3] != ~0ull) *bad_col = (int64_t)got[3];
    return SGL_OK;
}
