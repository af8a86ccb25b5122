// Signature scores (include/singlet_hip.h, "Signature scores"): the rank-based UCell score of every gene set in every cell of
// the resident matrix A (one column per cell, 64-bit offsets), from ONE descending ordering of the cell's stored non-zero
// values.  This file holds
//   1. sig_count_kernel: one wave per cell: its stored positive and negative entries P and N, which decide its path.
//   2. sig_lds_kernel<CAP, MODE>: one workgroup per short cell: the (key, payload) pairs of its stored non-zero entries are
//      gathered into LDS, sorted there (bitonic) and walked.  Two instances, CAP = 1024 and 4096 entries.
//   3. sig_fill_kernel / hipcub's segmented radix sort / sig_walk_kernel<MODE>: the long cells in batches through scratch.
//   The walk (sig_run_rank) gives a position BOTH ends of its tie run at once, by two binary searches over the sorted keys:
//   the cap is not linear in a + b + 1, so the two ends cannot be added in separate passes as the markers' walk adds them.
//   MODE 0 (sgl_op_cell_ranks) writes the doubled capped midrank of every stored entry; the payload is the entry's place in
//   its cell.  MODE 1 (the scores) adds it to the LDS accumulators (64-bit sum, 32-bit hits) of every set that holds the
//   entry's gene, found through the gene -> sets table; the payload is the gene, and a gene in no set costs one lookup and no
//   search.  The sets are taken in passes of at most SIGNATURE_PASS_SETS inside the kernel: the sorted cell stays where it is.
// All integers up to the score, which is one conversion, one division and one subtraction per (set, cell): no tiling, batch,
// pass size or order of the atomics can change a bit.  There is no floating-point atomic; the unit is compiled with
// -ffp-contract=off.  tests/signature_restatement.py restates all of it in numpy.
#include "sgl_internal.h"
#include "signature_host.h"

#include <hipcub/hipcub.hpp>
#include <climits>

#define SIG_THREADS 256
#define SIG_WAVES (SIG_THREADS / SGL_WAVE)
static_assert((SIGNATURE_LDS_SMALL & (SIGNATURE_LDS_SMALL - 1)) == 0 && (SIGNATURE_LDS_CAP & (SIGNATURE_LDS_CAP - 1)) == 0, "capacities: powers of two");
static_assert(SIGNATURE_LDS_SMALL >= SIG_THREADS && SIGNATURE_LDS_SMALL < SIGNATURE_LDS_CAP, "two instances, the small one a round of the workgroup");
static_assert(SIGNATURE_LDS_CAP * 12 + SIGNATURE_PASS_SETS * 12 + 1024 <= 64 * 1024, "the large instance stays below 64 KiB: no launch attribute");

typedef unsigned long long sg_u64;

// Descending image of a finite non-zero double: the positives first (top bit clear), the larger value the smaller key; then
// the negatives (top bit set).  ~0 is the image of no finite value: it pads the bitonic sort.
__device__ __forceinline__ sg_u64 sig_key(double x) {
    const sg_u64 u = (sg_u64)__double_as_longlong(x);
    return (u >> 63) ? u : (~u & 0x7fffffffffffffffull);
}

struct SigArgs {
    const double* x;          // the resident matrix A
    const int32_t* idx;
    const int64_t* p;
    const int32_t* cnt;       // 2 per cell: P, N
    sg_u64 m, R;
    // MODE 1
    const int64_t* gene_ptr;  // the gene -> sets table
    const int32_t* gene_sets;
    const int32_t* set_size;
    int32_t n_sets, pass;
    sg_u64* rank2;            // n_sets x ncol, set fastest
    double* score;
    // MODE 0
    sg_u64* entry;            // one per stored entry
    sg_u64* zero2;            // one per cell
};

// ---- 1. stored positive and negative entries per cell -------------------------------------------------------------------------
__global__ __launch_bounds__(SIG_THREADS) void sig_count_kernel(const double* __restrict__ x, const int64_t* __restrict__ p, int64_t n,
                                                               int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & (SGL_WAVE - 1);
    const int64_t c = (int64_t)blockIdx.x * SIG_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (c >= n) return;
    const int64_t lo = p[c], hi = p[c + 1];
    uint32_t np = 0, nn = 0;
    for (int64_t q = lo + lane; q < hi; q += SGL_WAVE) {
        const double v = x[q];
        np += v > 0.0 ? 1u : 0u;
        nn += v < 0.0 ? 1u : 0u;
    }
#pragma unroll
    for (int off = SGL_WAVE / 2; off > 0; off >>= 1) {
        np += __shfl_xor(np, off, SGL_WAVE);
        nn += __shfl_xor(nn, off, SGL_WAVE);
    }
    if (lane == 0) { cnt[2 * c] = (int32_t)np; cnt[2 * c + 1] = (int32_t)nn; }
}

// ---- the walk over a cell's sorted (key, payload) pairs ----------------------------------------------------------------------
// The doubled capped midrank of position j of the L sorted keys: its run [a, b) by two binary searches; the negatives sit
// behind the zero block of Z values.
template <typename KeyPtr>
__device__ __forceinline__ sg_u64 sig_run_rank(KeyPtr key, int L, int j, sg_u64 Z, sg_u64 R) {
    const sg_u64 k = key[j];
    int lo = 0, hi = j;               // a = the first position whose key is not below k
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < k) lo = mid + 1; else hi = mid;
    }
    const int a = lo;
    lo = j + 1;                       // b = the first position whose key is above k
    hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] <= k) lo = mid + 1; else hi = mid;
    }
    const sg_u64 shift = (k >> 63) ? Z : 0;
    return signature_cap_rank((sg_u64)a + (sg_u64)lo + 1 + 2 * shift, R);
}

// MODE 0: every stored entry of cell c gets its value (the stored zeros the zero block's), the cell its zero block's (0: none)
template <typename KeyPtr, typename PayPtr>
__device__ __forceinline__ void sig_emit_ranks(const SigArgs& A, int64_t c, KeyPtr key, PayPtr pay, int L) {
    const int64_t lo = A.p[c], hi = A.p[c + 1];
    const sg_u64 P = (sg_u64)A.cnt[2 * c], Z = A.m - P - (sg_u64)A.cnt[2 * c + 1];
    const sg_u64 z2 = signature_zero_rank(P, Z, A.R);
    for (int j = threadIdx.x; j < L; j += SIG_THREADS) A.entry[lo + pay[j]] = sig_run_rank(key, L, j, Z, A.R);
    for (int64_t q = lo + threadIdx.x; q < hi; q += SIG_THREADS)
        if (A.x[q] == 0.0) A.entry[q] = z2;
    if (threadIdx.x == 0) A.zero2[c] = Z > 0 ? z2 : 0;
}

// MODE 1: rank2 and score of every set in cell c, the sets in passes of A.pass; acc / hits hold A.pass values each (LDS).
// Every thread of the workgroup calls it; it begins and ends with a barrier.
template <typename KeyPtr, typename PayPtr>
__device__ __forceinline__ void sig_emit_scores(const SigArgs& A, int64_t c, KeyPtr key, PayPtr pay, int L, sg_u64* acc, uint32_t* hits) {
    const sg_u64 P = (sg_u64)A.cnt[2 * c], Z = A.m - P - (sg_u64)A.cnt[2 * c + 1];
    const sg_u64 z2 = signature_zero_rank(P, Z, A.R);
    for (int32_t s0 = 0; s0 < A.n_sets; s0 += A.pass) {
        const int32_t s1 = min(s0 + A.pass, A.n_sets);
        __syncthreads();
        for (int s = threadIdx.x; s < s1 - s0; s += SIG_THREADS) { acc[s] = 0; hits[s] = 0; }
        __syncthreads();
        for (int j = threadIdx.x; j < L; j += SIG_THREADS) {
            const int32_t g = pay[j];
            const int64_t q0 = A.gene_ptr[g], q1 = A.gene_ptr[g + 1];
            if (q0 == q1) continue;   // a gene in no set: one lookup
            sg_u64 r2 = 0;
            bool have = false;
            for (int64_t q = q0; q < q1; ++q) {
                const int32_t s = A.gene_sets[q];
                if (s < s0 || s >= s1) continue;
                if (!have) { r2 = sig_run_rank(key, L, j, Z, A.R); have = true; }
                atomicAdd(&acc[s - s0], r2);
                atomicAdd(&hits[s - s0], 1u);
            }
        }
        __syncthreads();
        for (int s = s0 + threadIdx.x; s < s1; s += SIG_THREADS) {
            const sg_u64 ns = (sg_u64)A.set_size[s];
            const sg_u64 r = acc[s - s0] + (ns - (sg_u64)hits[s - s0]) * z2;   // the members in the zero block
            const size_t at = (size_t)s + (size_t)A.n_sets * (size_t)c;
            A.rank2[at] = r;
            A.score[at] = signature_score(r, ns, A.R);
        }
    }
    __syncthreads();
}

// ---- 2. short cells: sort in LDS -----------------------------------------------------------------------------------------------
template <int CAP, int MODE>
__global__ __launch_bounds__(SIG_THREADS) void sig_lds_kernel(SigArgs A, const int32_t* __restrict__ list) {
    __shared__ sg_u64 key[CAP];
    __shared__ int32_t pay[CAP];
    __shared__ sg_u64 acc[MODE ? SIGNATURE_PASS_SETS : 1];
    __shared__ uint32_t hits[MODE ? SIGNATURE_PASS_SETS : 1];
    __shared__ uint32_t fill;
    const int tid = threadIdx.x;
    const int64_t c = list[blockIdx.x];
    if (tid == 0) fill = 0;
    __syncthreads();
    const int64_t lo = A.p[c], hi = A.p[c + 1];
    for (int64_t q = lo + tid; q < hi; q += SIG_THREADS) {   // (the order of the gathered pairs is free: they are sorted next)
        const double xv = A.x[q];
        if (xv != 0.0) {
            const uint32_t at = atomicAdd(&fill, 1u);
            if (at < (uint32_t)CAP) { key[at] = sig_key(xv); pay[at] = MODE ? A.idx[q] : (int32_t)(q - lo); }   // (the host sent only cells that fit)
        }
    }
    __syncthreads();
    const int L = (int)min(fill, (uint32_t)CAP);
    int n2 = 2;
    while (n2 < L) n2 <<= 1;
    for (int i = L + tid; i < n2; i += SIG_THREADS) { key[i] = ~0ull; pay[i] = 0; }   // above the key of every finite value
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += SIG_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const sg_u64 a = key[i], b = key[o];
                    if ((a > b) == ((i & k) == 0)) {
                        key[i] = b; key[o] = a;
                        const int32_t t = pay[i]; pay[i] = pay[o]; pay[o] = t;
                    }
                }
            }
            __syncthreads();
        }
    if (MODE) sig_emit_scores(A, c, key, pay, L, acc, hits);
    else sig_emit_ranks(A, c, key, pay, L);
}

// ---- 3. long cells: scratch, segmented sort, walk ----------------------------------------------------------------------------------
// one workgroup per cell of the batch: its stored non-zero entries as (key, payload) at off[b] ..
template <int MODE>
__global__ __launch_bounds__(SIG_THREADS) void sig_fill_kernel(SigArgs A, const int32_t* __restrict__ list, const int64_t* __restrict__ off,
                                                              sg_u64* __restrict__ key, int32_t* __restrict__ pay) {
    __shared__ uint32_t fill;
    const int b = blockIdx.x;
    const int64_t c = list[b];
    const int64_t o = off[b], cap = off[b + 1] - o;
    if (threadIdx.x == 0) fill = 0;
    __syncthreads();
    const int64_t lo = A.p[c], hi = A.p[c + 1];
    for (int64_t q = lo + threadIdx.x; q < hi; q += SIG_THREADS) {
        const double xv = A.x[q];
        if (xv != 0.0) {
            const int64_t at = (int64_t)atomicAdd(&fill, 1u);
            if (at < cap) { key[o + at] = sig_key(xv); pay[o + at] = MODE ? A.idx[q] : (int32_t)(q - lo); }   // (cap = the count of the same entries)
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(SIG_THREADS) void sig_walk_kernel(SigArgs A, const int32_t* __restrict__ list, const int64_t* __restrict__ off,
                                                              const sg_u64* __restrict__ key, const int32_t* __restrict__ pay) {
    __shared__ sg_u64 acc[MODE ? SIGNATURE_PASS_SETS : 1];
    __shared__ uint32_t hits[MODE ? SIGNATURE_PASS_SETS : 1];
    const int b = blockIdx.x;
    const int64_t o = off[b];
    const int L = (int)(off[b + 1] - o);
    if (MODE) sig_emit_scores(A, (int64_t)list[b], key + o, pay + o, L, acc, hits);
    else sig_emit_ranks(A, (int64_t)list[b], key + o, pay + o, L);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
namespace {
template <int MODE>
int sig_paths(sgl_ctx* c, SigArgs A, int64_t lds_cap, int64_t max_batch_entries) {
    const DevCSC& M = c->A;
    const int64_t n = M.ncol;
    hipStream_t s = c->stream;
    const size_t n1 = (size_t)std::max<int64_t>(n, 1);
    DevBuf<int32_t> dcnt, dlist;
    SGLCHK(dcnt.alloc(2 * n1));
    SGLCHK(dlist.alloc(3 * n1));
    std::vector<int32_t> cnt(2 * n1, 0);
    if (n > 0) {
        Phase ph(c, SGL_PH_SCALE);
        sig_count_kernel<<<dim3((unsigned)((n + SIG_WAVES - 1) / SIG_WAVES)), dim3(SIG_THREADS), 0, s>>>(M.x, M.p, n, dcnt.p);
        HIPCHK(hipGetLastError());
    }
    if (n > 0) HIPCHK(hipMemcpyAsync(cnt.data(), dcnt.p, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    A.cnt = dcnt.p;
    std::vector<int64_t> len(n1), long_len(n1), cut(n1 + 1);
    for (int64_t j = 0; j < n; ++j) len[(size_t)j] = (int64_t)cnt[2 * (size_t)j] + (int64_t)cnt[2 * (size_t)j + 1];
    std::vector<int32_t> lists(3 * n1);
    int32_t *small_list = lists.data(), *large_list = lists.data() + n1, *long_list = lists.data() + 2 * n1;
    int64_t ns = 0, ng = 0, nl = 0;
    const int64_t cap = signature_lds_cap(lds_cap);
    signature_split_paths(len.data(), n, cap, small_list, &ns, large_list, &ng, long_list, long_len.data(), &nl);
    const int64_t runs = nl > 0 ? signature_batches(long_len.data(), nl, max_batch_entries, cut.data()) : 0;
    c->signature_last[0] = ns;
    c->signature_last[1] = ng;
    c->signature_last[2] = nl;
    c->signature_last[3] = runs;
    c->signature_last[4] = MODE ? (A.n_sets + A.pass - 1) / A.pass : 0;
    c->signature_last[5] = cap;
    c->signature_last[6] = signature_batch_cap(max_batch_entries);
    c->signature_last[7] = MODE ? A.pass : 0;
    HIPCHK(hipMemcpyAsync(dlist.p, lists.data(), sizeof(int32_t) * lists.size(), hipMemcpyHostToDevice, s));
    {
        Phase ph(c, SGL_PH_SCALE);
        if (ns > 0) {
            sig_lds_kernel<SIGNATURE_LDS_SMALL, MODE><<<dim3((unsigned)ns), dim3(SIG_THREADS), 0, s>>>(A, dlist.p);
            HIPCHK(hipGetLastError());
        }
        if (ng > 0) {
            sig_lds_kernel<SIGNATURE_LDS_CAP, MODE><<<dim3((unsigned)ng), dim3(SIG_THREADS), 0, s>>>(A, dlist.p + n1);
            HIPCHK(hipGetLastError());
        }
    }
    if (nl > 0) {
        int64_t max_entries = 0, max_cells = 0;
        for (int64_t b = 0; b < runs; ++b) {
            int64_t sum = 0;
            for (int64_t g = cut[(size_t)b]; g < cut[(size_t)b + 1]; ++g) sum += long_len[(size_t)g];
            max_entries = std::max(max_entries, sum);
            max_cells = std::max(max_cells, cut[(size_t)b + 1] - cut[(size_t)b]);
        }
        if (max_entries > INT32_MAX) { sgl_set_error("signature scores: a batch holds %lld entries", (long long)max_entries); return SGL_EINVAL; }
        DevBuf<sg_u64> k1, k2;
        DevBuf<int32_t> p1, p2;
        DevBuf<int64_t> doff;
        DevBuf<char> tmp;
        SGLCHK(k1.alloc((size_t)max_entries));
        SGLCHK(k2.alloc((size_t)max_entries));
        SGLCHK(p1.alloc((size_t)max_entries));
        SGLCHK(p2.alloc((size_t)max_entries));
        SGLCHK(doff.alloc((size_t)max_cells + 1));
        std::vector<int64_t> off;
        size_t tmp_cap = 0;
        const int32_t* dlong = dlist.p + 2 * n1;
        Phase ph(c, SGL_PH_SCALE);
        for (int64_t b = 0; b < runs; ++b) {
            const int64_t g0 = cut[(size_t)b], nc = cut[(size_t)b + 1] - g0;
            off.assign((size_t)nc + 1, 0);
            for (int64_t g = 0; g < nc; ++g) off[(size_t)g + 1] = off[(size_t)g] + long_len[(size_t)(g0 + g)];
            const int64_t tot = off[(size_t)nc];
            HIPCHK(hipMemcpyAsync(doff.p, off.data(), sizeof(int64_t) * ((size_t)nc + 1), hipMemcpyHostToDevice, s));
            sig_fill_kernel<MODE><<<dim3((unsigned)nc), dim3(SIG_THREADS), 0, s>>>(A, dlong + g0, doff.p, k1.p, p1.p);
            HIPCHK(hipGetLastError());
            size_t bytes = 0;
            HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, bytes, k1.p, k2.p, p1.p, p2.p, (int)tot, (int)nc, doff.p, doff.p + 1, 0, 64, s));
            if (bytes > tmp_cap) {
                HIPCHK(hipStreamSynchronize(s));
                SGLCHK(tmp.alloc(bytes));
                tmp_cap = bytes;
            }
            HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(tmp.p, bytes, k1.p, k2.p, p1.p, p2.p, (int)tot, (int)nc, doff.p, doff.p + 1, 0, 64, s));
            sig_walk_kernel<MODE><<<dim3((unsigned)nc), dim3(SIG_THREADS), 0, s>>>(A, dlong + g0, doff.p, k2.p, p2.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(s));   // `off` is rewritten for the next batch
        }
    }
    HIPCHK(hipStreamSynchronize(s));   // the lists and the counts go
    return SGL_OK;
}

SigArgs sig_base_args(sgl_ctx* c, int64_t max_rank) {
    SigArgs A = {};
    A.x = c->A.x;
    A.idx = c->A.i;
    A.p = c->A.p;
    A.m = (sg_u64)c->A.nrow;
    A.R = (sg_u64)max_rank;
    return A;
}

int sig_scores_on(sgl_ctx* c, const int64_t* set_ptr, const int32_t* set_genes, int32_t n_sets, int64_t max_rank, int64_t lds_cap,
                  int64_t max_batch_entries, int64_t pass_sets, uint64_t* rank2_out, double* score_out) {
    const int64_t m = c->A.nrow, n = c->A.ncol;
    hipStream_t s = c->stream;
    std::vector<int64_t> gene_ptr((size_t)m + 1);
    std::vector<int32_t> gene_sets((size_t)std::max<int64_t>(set_ptr[n_sets], 1)), set_size((size_t)n_sets);
    signature_gene_table(set_ptr, set_genes, n_sets, m, gene_ptr.data(), gene_sets.data());
    for (int32_t j = 0; j < n_sets; ++j) set_size[(size_t)j] = (int32_t)(set_ptr[j + 1] - set_ptr[j]);
    DevBuf<int64_t> dptr;
    DevBuf<int32_t> dsets, dsize;
    DevBuf<sg_u64> drank;
    DevBuf<double> dscore;
    const size_t cells = (size_t)n_sets * (size_t)std::max<int64_t>(n, 1);
    SGLCHK(dptr.alloc(gene_ptr.size()));
    SGLCHK(dsets.alloc(gene_sets.size()));
    SGLCHK(dsize.alloc(set_size.size()));
    SGLCHK(drank.alloc(cells));
    SGLCHK(dscore.alloc(cells));
    HIPCHK(hipMemcpyAsync(dptr.p, gene_ptr.data(), sizeof(int64_t) * gene_ptr.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dsets.p, gene_sets.data(), sizeof(int32_t) * gene_sets.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dsize.p, set_size.data(), sizeof(int32_t) * set_size.size(), hipMemcpyHostToDevice, s));
    SigArgs A = sig_base_args(c, max_rank);
    A.gene_ptr = dptr.p;
    A.gene_sets = dsets.p;
    A.set_size = dsize.p;
    A.n_sets = n_sets;
    A.pass = (int32_t)signature_pass_size(pass_sets);
    A.rank2 = drank.p;
    A.score = dscore.p;
    SGLCHK(sig_paths<1>(c, A, lds_cap, max_batch_entries));
    if (n > 0) {
        const size_t out = (size_t)n_sets * (size_t)n;
        if (rank2_out) HIPCHK(hipMemcpyAsync(rank2_out, drank.p, sizeof(uint64_t) * out, hipMemcpyDeviceToHost, s));
        if (score_out) HIPCHK(hipMemcpyAsync(score_out, dscore.p, sizeof(double) * out, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    return SGL_OK;
}

int sig_ranks_on(sgl_ctx* c, int64_t max_rank, int64_t lds_cap, int64_t max_batch_entries, uint64_t* entry_out, uint64_t* zero2_out) {
    const int64_t n = c->A.ncol, nnz = c->A.nnz;
    hipStream_t s = c->stream;
    DevBuf<sg_u64> dentry, dzero;
    SGLCHK(dentry.alloc((size_t)std::max<int64_t>(nnz, 1)));
    SGLCHK(dzero.alloc((size_t)std::max<int64_t>(n, 1)));
    SigArgs A = sig_base_args(c, max_rank);
    A.entry = dentry.p;
    A.zero2 = dzero.p;
    SGLCHK(sig_paths<0>(c, A, lds_cap, max_batch_entries));
    if (entry_out && nnz > 0) HIPCHK(hipMemcpyAsync(entry_out, dentry.p, sizeof(uint64_t) * (size_t)nnz, hipMemcpyDeviceToHost, s));
    if (zero2_out && n > 0) HIPCHK(hipMemcpyAsync(zero2_out, dzero.p, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return SGL_OK;
}

// every return path waits for the stream before the temporaries (and the caller's host arrays) go
int sig_finish(sgl_ctx* c, int rc) {
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("signature scores: HIP call failed: %s", hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}
}   // namespace

int sgl_signature_args_check(const char* who, const int64_t* set_ptr, const int32_t* set_genes, int64_t n_sets, int64_t m, int64_t max_rank,
                             int64_t lds_cap, int64_t max_batch_entries, int64_t pass_sets) {
    static const char* const knob[3] = {"lds_cap", "max_batch_entries", "pass_sets"};
    std::vector<int32_t> stamp((size_t)std::max<int64_t>(m, 1));
    int64_t at = -1, val = 0;
    switch (signature_check_args(set_ptr, set_genes, n_sets, m, max_rank, lds_cap, max_batch_entries, pass_sets, stamp.data(), &at, &val)) {
    case SIGNATURE_ARGS_OK: return SGL_OK;
    case SIGNATURE_ARGS_NULL: sgl_set_error("%s: NULL set_ptr or set_genes", who); break;
    case SIGNATURE_ARGS_SETS: sgl_set_error("%s: n_sets = %lld: at least one set is needed", who, (long long)val); break;
    case SIGNATURE_ARGS_RANK: sgl_set_error("%s: max_rank = %lld is outside [1, %lld] (the genes of the matrix)", who, (long long)val, (long long)m); break;
    case SIGNATURE_ARGS_KNOB: sgl_set_error("%s: %s = %lld is negative", who, knob[at], (long long)val); break;
    case SIGNATURE_ARGS_PTR: sgl_set_error("%s: set_ptr[%lld] = %lld: the offsets start at 0 and ascend", who, (long long)at, (long long)val); break;
    case SIGNATURE_ARGS_EMPTY: sgl_set_error("%s: set %lld is empty", who, (long long)at); break;
    case SIGNATURE_ARGS_SIZE: sgl_set_error("%s: set %lld holds %lld genes, more than max_rank = %lld", who, (long long)at, (long long)val, (long long)max_rank); break;
    case SIGNATURE_ARGS_GENE: sgl_set_error("%s: set_genes[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)m); break;
    case SIGNATURE_ARGS_TWICE: sgl_set_error("%s: set_genes[%lld] = %lld occurs twice in its set", who, (long long)at, (long long)val); break;
    }
    return SGL_EINVAL;
}

int sgl_signature_scores_core(sgl_ctx* c, const int64_t* set_ptr, const int32_t* set_genes, int32_t n_sets, int64_t max_rank, int64_t lds_cap,
                              int64_t max_batch_entries, int64_t pass_sets, uint64_t* rank2_out, double* score_out) {
    return sig_finish(c, sig_scores_on(c, set_ptr, set_genes, n_sets, max_rank, lds_cap, max_batch_entries, pass_sets, rank2_out, score_out));
}

int sgl_cell_ranks_core(sgl_ctx* c, int64_t max_rank, int64_t lds_cap, int64_t max_batch_entries, uint64_t* entry_out, uint64_t* zero2_out) {
    return sig_finish(c, sig_ranks_on(c, max_rank, lds_cap, max_batch_entries, entry_out, zero2_out));
}
