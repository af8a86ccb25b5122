// Column gather of a CSC: D = S[:, sel], the primitive of sgl_subset (include/singlet_hip.h).  Column j of D is column
// sel[j] of S as it stands -- its entries in their stored (ascending-row) order, bit for bit -- so any order of sel and
// any number of duplicates come for free.  A row subset of A is this gather on t(A); the other orientation is rebuilt by
// the device transpose (kernels_transpose.hip), whose stable sort gives the ascending rows.
//
// Three steps: len[j] = S.p[sel[j] + 1] - S.p[sel[j]], the exclusive scan of len into D.p, and the copy of (i, x).  The
// copy is balanced by OUTPUT ENTRIES, not by columns: a gene of t(A) holds up to ncol entries, a cell of a 2 000-gene
// matrix about a hundred, and a wave per column would serialise on the one and idle on the other.  HBM-bound index work:
// every kept entry is read once and written once (12 bytes each way), plus the searches in D.p, which stay in cache.
#include "sgl_internal.h"

namespace {

constexpr int SGL_SUBSET_TILE = 4096;   // consecutive output entries one workgroup copies
constexpr int SUBSET_THREADS = 256;

__global__ void subset_len_kernel(const int64_t* __restrict__ p, const int32_t* __restrict__ sel, int64_t n,
                                  int64_t* __restrict__ len) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) len[j] = p[sel[j] + 1] - p[sel[j]];
}

// the last column of [lo, hi] that starts at or before entry e (pn[lo] <= e): upper bound - 1, so runs of empty columns
// (equal offsets) are stepped over to the one column that holds e
__device__ __forceinline__ int64_t column_of(const int64_t* __restrict__ pn, int64_t lo, int64_t hi, int64_t e) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (pn[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Tile t = output entries [t TILE, min((t + 1) TILE, nnz)).  Two uniform searches in pn (n + 1 offsets, pn[0] = 0,
// pn[n] = nnz) give the tile's first and last column; thread tid copies entries t0 + tid + 256 j (consecutive lanes,
// consecutive entries: the stores of x and i are coalesced, the loads too within a source column) and finds each entry's
// column by a search narrowed to the tile's range -- no step at all inside a column that spans the tile.
__global__ __launch_bounds__(SUBSET_THREADS) void subset_copy_kernel(const double* __restrict__ x, const int32_t* __restrict__ idx,
                                                                     const int64_t* __restrict__ p, const int32_t* __restrict__ sel,
                                                                     const int64_t* __restrict__ pn, int64_t n, int64_t nnz,
                                                                     int64_t ntiles, double* __restrict__ xo, int32_t* __restrict__ io) {
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * SGL_SUBSET_TILE, t1 = std::min<int64_t>(t0 + SGL_SUBSET_TILE, nnz);
        const int64_t c_lo = column_of(pn, 0, n - 1, t0);
        const int64_t c_hi = column_of(pn, c_lo, n - 1, t1 - 1);
        for (int64_t e = t0 + threadIdx.x; e < t1; e += SUBSET_THREADS) {
            const int64_t j = column_of(pn, c_lo, c_hi, e);
            const int64_t q = p[sel[j]] + (e - pn[j]);
            xo[e] = x[q];
            io[e] = idx[q];
        }
    }
}

}  // namespace

// D = S[:, sel[0 .. n)]: sel on the device, every value in [0, S.ncol) (the caller has checked it), n >= 1.  D comes in
// empty and leaves with its own p / i / x (a failure leaves what was allocated in D for the caller to free).  Enqueues on
// the context's stream and synchronises once, for the new entry count.
int k_subset_gather(sgl_ctx* c, const DevCSC& S, const int32_t* sel, int64_t n, DevCSC& D) {
    hipStream_t s = c->stream;
    D.nrow = S.nrow;
    D.ncol = (int32_t)n;
    SGLCHK(dev_alloc(&D.p, (size_t)n + 1));
    DevBuf<int64_t> len;
    SGLCHK(len.alloc((size_t)n));
    subset_len_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(S.p, sel, n, len.p);
    HIPCHK(hipGetLastError());
    SGLCHK(k_exclusive_scan(c, len.p, D.p, n));
    SGLCHK(k_scan_total(s, len.p, D.p, n));
    int64_t nnz = 0;
    HIPCHK(hipMemcpyAsync(&nnz, D.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    D.nnz = nnz;
    SGLCHK(dev_alloc(&D.x, (size_t)nnz));
    SGLCHK(dev_alloc(&D.i, (size_t)nnz));
    if (nnz == 0) return SGL_OK;
    const int64_t ntiles = (nnz + SGL_SUBSET_TILE - 1) / SGL_SUBSET_TILE;
    const unsigned grid = (unsigned)std::min<int64_t>(ntiles, 1 << 20);
    subset_copy_kernel<<<dim3(grid), dim3(SUBSET_THREADS), 0, s>>>(S.x, S.i, S.p, sel, D.p, n, nnz, ntiles, D.x, D.i);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}
