// Neighbourhood enrichment of clusters on a cell graph (include/singlet_hip.h, "Neighbourhood enrichment"): the count of stored
// graph entries between every pair of classes, observed and under nperm label permutations drawn from the counter hash.
// Everything the device computes is an integer, so every result is one function of the inputs whatever the path, the
// permutations per group, the batch or the order of the atomics.  This file holds
//   1. nh_keys_kernel / hipcub's radix sort / nh_gather_kernel: per permutation the cells by (key, cell) -- the sort is stable
//      and the cells enter in ascending order -- and lab_r = lab[order_r], written PERMUTATION-INTERLEAVED: the labels of one
//      cell under the PG permutations of a group are PG adjacent bytes, so one load of PG bytes at a neighbour's index serves
//      the whole group.  Up to the plan's switch the permutations of a chunk are the segments of one segmented sort (one
//      workgroup per segment); above it every permutation is one device-wide sort.
//   2. nh_colid_kernel: the column of every stored entry, by a search in Gp, once per call.
//   3. nh_tally_kernel: the work is cut by STORED ENTRIES (a workgroup takes a whole number of 4096-entry segments, whatever
//      columns they belong to: a hub column is nobody's walk).  LDS path: the PG x K x K uint32 tiles of the group live in LDS,
//      an entry adds 1 to one bin of every tile with an LDS atomic, the non-zero bins of the valid permutations are flushed to
//      the batch's int64 counts with global atomics.  A tile's bin counts entries of ONE workgroup, at most nnz < 2^31: it
//      cannot overflow.  Global path (K above 181, or forced): the atomics go straight to the counts.
//   4. nh_reduce_kernel: one thread per pair walks the batch's permutations and adds S1, S2, n_ge, n_le in int64.
// The observed tally is the same gather (identity order) and the same tally with one permutation per group.
#include "sgl_internal.h"
#include "nhood_host.h"

#include <hipcub/hipcub.hpp>
#include <stdlib.h>

#define NH_THREADS 256          // the element-wise kernels
#define NH_TALLY_THREADS 512    // the tally: eight waves share the tiles of a workgroup

typedef unsigned long long nh_u64;

// ---- 1. permutations ------------------------------------------------------------------------------------------------------------
// permutations [r0, r0 + total / n): key(r, c) and c, permutation-major
__global__ __launch_bounds__(NH_THREADS) void nh_keys_kernel(uint64_t seed, int64_t r0, int64_t n, int64_t total, nh_u64* __restrict__ key,
                                                            int32_t* __restrict__ cell) {
    const int64_t t = (int64_t)blockIdx.x * NH_THREADS + threadIdx.x;
    if (t >= total) return;
    const int64_t c = t % n;
    key[t] = sgl_rand2(seed, (uint64_t)(r0 + t / n), (uint64_t)c);
    cell[t] = (int32_t)c;
}
// offsets of n1 - 1 segments of n items
__global__ __launch_bounds__(NH_THREADS) void nh_offsets_kernel(int64_t n, int64_t n1, int64_t* __restrict__ off) {
    const int64_t t = (int64_t)blockIdx.x * NH_THREADS + threadIdx.x;
    if (t < n1) off[t] = t * n;
}

// The interleaved labels of np label vectors (local index l): out[((l / PG) n + c) PG + l % PG] = lab[l lab_stride + idx],
// idx = order[l n + c], or c itself without an order.  A slot past np holds label 0.  One thread per (group, cell) writes the
// PG bytes of its cell in one store.
template <int PG>
__global__ __launch_bounds__(NH_THREADS) void nh_gather_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ lab, int64_t lab_stride,
                                                              int64_t n, int64_t np, int64_t total, uint8_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * NH_THREADS + threadIdx.x;
    if (t >= total) return;
    const int64_t g = t / n, c = t % n;
    uint8_t b[PG];
#pragma unroll
    for (int q = 0; q < PG; ++q) {
        const int64_t l = g * PG + q;
        int32_t v = 0;
        if (l < np) {
            const int64_t idx = order ? (int64_t)order[l * n + c] : c;
            v = lab[l * lab_stride + idx];
        }
        b[q] = (uint8_t)v;
    }
    __builtin_memcpy(__builtin_assume_aligned(out + t * PG, PG), b, PG);
}

// ---- 2. the column of every stored entry ----------------------------------------------------------------------------------------
// col[e] = the j with Gp[j] <= e < Gp[j + 1]: the largest j in [0, n) with Gp[j] <= e (empty columns are stepped over)
__global__ __launch_bounds__(NH_THREADS) void nh_colid_kernel(const int32_t* __restrict__ Gp, int64_t n, int64_t nnz, int32_t* __restrict__ col) {
    const int64_t e = (int64_t)blockIdx.x * NH_THREADS + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)Gp[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    col[e] = (int32_t)lo;
}

// ---- 3. the tally ---------------------------------------------------------------------------------------------------------------
// grid (groups, workgroups over the entries).  lab8: the interleaved labels of the groups, every byte < K.  counts: np x K x K,
// zero or holding earlier sums on entry.  Gi[e] and col[e] are in [0, n) (checked on the host / by construction).
template <int PG, bool LDS>
__global__ __launch_bounds__(NH_TALLY_THREADS) void nh_tally_kernel(const int32_t* __restrict__ Gi, const int32_t* __restrict__ col, int64_t nnz,
                                                                   int64_t wg_entries, const uint8_t* __restrict__ lab8, int64_t n, int K, int drop,
                                                                   int64_t np, nh_u64* __restrict__ counts) {
    extern __shared__ uint32_t nh_tile[];
    const int KK = K * K;
    const int64_t g = blockIdx.x;
    const int valid = (int)(np - g * PG < PG ? np - g * PG : PG);
    if (LDS) {
        for (int i = threadIdx.x; i < PG * KK; i += NH_TALLY_THREADS) nh_tile[i] = 0u;
        __syncthreads();
    }
    const uint8_t* __restrict__ L = lab8 + (size_t)g * (size_t)n * PG;
    nh_u64* __restrict__ out = counts + (size_t)g * PG * (size_t)KK;
    const int64_t e0 = (int64_t)blockIdx.y * wg_entries, e1 = e0 + wg_entries < nnz ? e0 + wg_entries : nnz;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += NH_TALLY_THREADS) {
        const int64_t r = Gi[e], j = col[e];
        if (drop && r == j) continue;
        uint8_t a[PG], b[PG];
        __builtin_memcpy(a, __builtin_assume_aligned(L + j * PG, PG), PG);   // the centre cell's classes
        __builtin_memcpy(b, __builtin_assume_aligned(L + r * PG, PG), PG);   // the neighbour's
#pragma unroll
        for (int q = 0; q < PG; ++q) {
            const int bin = q * KK + (int)a[q] + K * (int)b[q];
            if (LDS) atomicAdd(&nh_tile[bin], 1u);
            else if (q < valid) atomicAdd(&out[bin], 1ull);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < valid * KK; i += NH_TALLY_THREADS) {
            const uint32_t v = nh_tile[i];
            if (v) atomicAdd(&out[i], (nh_u64)v);
        }
    }
}

// ---- 4. the reduction -------------------------------------------------------------------------------------------------------------
// cb: nb x KK counts of a batch; the four tallies are carried from batch to batch
__global__ __launch_bounds__(NH_THREADS) void nh_reduce_kernel(const int64_t* __restrict__ cb, int64_t KK, int64_t nb, const int64_t* __restrict__ C,
                                                              int64_t* __restrict__ S1, int64_t* __restrict__ S2, int64_t* __restrict__ n_ge,
                                                              int64_t* __restrict__ n_le) {
    const int64_t q = (int64_t)blockIdx.x * NH_THREADS + threadIdx.x;
    if (q >= KK) return;
    const int64_t obs = C[q];
    int64_t s1 = S1[q], s2 = S2[q], ge = n_ge[q], le = n_le[q];
    for (int64_t r = 0; r < nb; ++r) {
        const int64_t v = cb[r * KK + q];
        s1 += v;
        s2 += v * v;
        ge += v >= obs;
        le += v <= obs;
    }
    S1[q] = s1;
    S2[q] = s2;
    n_ge[q] = ge;
    n_le[q] = le;
}

// =================================================================================================================================
namespace {
inline unsigned nh_blocks(int64_t n) { return (unsigned)((n + NH_THREADS - 1) / NH_THREADS); }

// stage timer of sgl_c_nhood_enrichment's stage_ms: events around a stage when the caller asked for the times
struct NhTimer {
    hipStream_t s;
    double* ms;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    NhTimer(hipStream_t s_, double* ms_) : s(s_), ms(ms_) {
        if (ms && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) { (void)hipGetLastError(); ms = nullptr; }
    }
    ~NhTimer() {
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

// the knob of the tests and the benchmarks: cells above which every permutation is one device-wide sort (read per call)
int64_t nh_sort_switch() {
    const char* e = getenv("SGL_NHOOD_SORT_SWITCH");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (int64_t)v : 0;
}

struct NhGraph {
    DevBuf<int32_t> Gi, Gp, col;
    int64_t nnz = 0;
    int upload(sgl_ctx* c, const int32_t* hGi, const int32_t* hGp, int64_t n) {
        hipStream_t s = c->stream;
        nnz = hGp[n];
        SGLCHK(Gi.alloc((size_t)nnz));
        SGLCHK(Gp.alloc((size_t)n + 1));
        SGLCHK(col.alloc((size_t)nnz));
        HIPCHK(hipMemcpyAsync(Gp.p, hGp, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, s));
        if (nnz > 0) {
            HIPCHK(hipMemcpyAsync(Gi.p, hGi, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, s));
            Phase ph(c, SGL_PH_SCALE);
            nh_colid_kernel<<<dim3(nh_blocks(nnz)), dim3(NH_THREADS), 0, s>>>(Gp.p, n, nnz, col.p);
            HIPCHK(hipGetLastError());
        }
        return SGL_OK;
    }
};

template <int PG>
int nh_gather_pg(hipStream_t s, const int32_t* order, const int32_t* lab, int64_t lab_stride, int64_t n, int64_t np, uint8_t* out) {
    const int64_t total = (np + PG - 1) / PG * n;
    nh_gather_kernel<PG><<<dim3(nh_blocks(total)), dim3(NH_THREADS), 0, s>>>(order, lab, lab_stride, n, np, total, out);
    HIPCHK(hipGetLastError());
    return SGL_OK;
}
// out: the groups of these np label vectors, (np rounded up to pg) * n bytes
int nh_gather(hipStream_t s, int pg, const int32_t* order, const int32_t* lab, int64_t lab_stride, int64_t n, int64_t np, uint8_t* out) {
    switch (pg) {
    case 1: return nh_gather_pg<1>(s, order, lab, lab_stride, n, np, out);
    case 2: return nh_gather_pg<2>(s, order, lab, lab_stride, n, np, out);
    case 4: return nh_gather_pg<4>(s, order, lab, lab_stride, n, np, out);
    case 8: return nh_gather_pg<8>(s, order, lab, lab_stride, n, np, out);
    default: return nh_gather_pg<16>(s, order, lab, lab_stride, n, np, out);
    }
}

struct NhPermuter {
    DevBuf<nh_u64> k1, k2;
    DevBuf<int32_t> v1, v2;
    DevBuf<int64_t> off;
    DevBuf<char> tmp;
    size_t tmp_cap = 0;
    int64_t perms = 0;
    int sort = 0;
    int alloc(int64_t n, const NhoodPlan& P) {
        perms = P.sort_perms;
        sort = P.sort;
        const size_t items = (size_t)perms * (size_t)n;
        SGLCHK(k1.alloc(items));
        SGLCHK(k2.alloc(items));
        SGLCHK(v1.alloc(items));
        SGLCHK(v2.alloc(items));
        return off.alloc((size_t)perms + 1);
    }
    int reserve(hipStream_t s, size_t bytes) {
        if (bytes > tmp_cap) {
            HIPCHK(hipStreamSynchronize(s));
            SGLCHK(tmp.alloc(bytes));
            tmp_cap = bytes;
        }
        return SGL_OK;
    }
};

// the interleaved labels of the permutations [r0, r0 + nb) in groups of pg; lab on the device
int nh_permute(sgl_ctx* c, NhPermuter& Q, const int32_t* lab, int64_t n, uint64_t seed, int64_t r0, int64_t nb, int pg, uint8_t* out8) {
    hipStream_t s = c->stream;
    Phase ph(c, SGL_PH_SCALE);
    for (int64_t q0 = 0; q0 < nb; q0 += Q.perms) {
        const int64_t nq = std::min(Q.perms, nb - q0), total = nq * n;
        nh_keys_kernel<<<dim3(nh_blocks(total)), dim3(NH_THREADS), 0, s>>>(seed, r0 + q0, n, total, Q.k1.p, Q.v1.p);
        HIPCHK(hipGetLastError());
        size_t bytes = 0;
        if (Q.sort == 0) {
            nh_offsets_kernel<<<dim3(nh_blocks(nq + 1)), dim3(NH_THREADS), 0, s>>>(n, nq + 1, Q.off.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, bytes, Q.k1.p, Q.k2.p, Q.v1.p, Q.v2.p, (int)total, (int)nq, Q.off.p, Q.off.p + 1,
                                                               0, 64, s));
            SGLCHK(Q.reserve(s, bytes));
            HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(Q.tmp.p, bytes, Q.k1.p, Q.k2.p, Q.v1.p, Q.v2.p, (int)total, (int)nq, Q.off.p, Q.off.p + 1,
                                                               0, 64, s));
        } else {
            HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, Q.k1.p, Q.k2.p, Q.v1.p, Q.v2.p, (int)n, 0, 64, s));
            SGLCHK(Q.reserve(s, bytes));
            for (int64_t q = 0; q < nq; ++q)
                HIPCHK(hipcub::DeviceRadixSort::SortPairs(Q.tmp.p, bytes, Q.k1.p + q * n, Q.k2.p + q * n, Q.v1.p + q * n, Q.v2.p + q * n, (int)n, 0, 64, s));
        }
        SGLCHK(nh_gather(s, pg, Q.v2.p, lab, 0, n, nq, out8 + (size_t)(q0 / pg) * (size_t)n * (size_t)pg));   // (q0 is a multiple of 16)
    }
    return SGL_OK;
}

template <int PG, bool LDS>
int nh_tally_pg(sgl_ctx* c, const NhGraph& G, const NhoodPlan& P, const uint8_t* lab8, int64_t n, int K, int drop, int64_t np, int64_t* counts) {
    const size_t lds = LDS ? (size_t)PG * (size_t)K * (size_t)K * sizeof(uint32_t) : 0;
    if (LDS) SGLCHK((sgl_allow_dynamic_lds<&nh_tally_kernel<PG, LDS>>((int)NHOOD_LDS_TILE_BYTES)));
    const dim3 grid((unsigned)((np + PG - 1) / PG), (unsigned)P.wgs);
    nh_tally_kernel<PG, LDS><<<grid, dim3(NH_TALLY_THREADS), lds, c->stream>>>(G.Gi.p, G.col.p, G.nnz, P.wg_entries, lab8, n, K, drop, np,
                                                                              reinterpret_cast<nh_u64*>(counts));
    HIPCHK(hipGetLastError());
    return SGL_OK;
}
// counts (np x K x K, cleared by the caller) += the tally of the np interleaved label vectors in groups of pg
int nh_tally(sgl_ctx* c, const NhGraph& G, const NhoodPlan& P, int pg, const uint8_t* lab8, int64_t n, int K, int drop, int64_t np, int64_t* counts) {
    if (G.nnz == 0 || np == 0) return SGL_OK;
    Phase ph(c, SGL_PH_SCALE);
#define NH_CASE(PG_)                                                                                    \
    case PG_:                                                                                           \
        return P.path == 1 ? nh_tally_pg<PG_, true>(c, G, P, lab8, n, K, drop, np, counts)              \
                           : nh_tally_pg<PG_, false>(c, G, P, lab8, n, K, drop, np, counts)
    switch (pg) {
        NH_CASE(1);
        NH_CASE(2);
        NH_CASE(4);
        NH_CASE(8);
    default:
        NH_CASE(16);
    }
#undef NH_CASE
}

void nh_record(sgl_ctx* c, const NhoodPlan& P, int64_t batches, int64_t batch) {
    const int64_t v[6] = {P.path, P.pg, batches, batch, P.lds_bytes, P.sort};
    std::copy(v, v + 6, c->nhood_last);
}
}   // namespace

static int nh_refuse(const char* who, NhoodArgError e, int64_t n, int64_t K, int64_t nperm, int64_t at, int64_t val) {
    switch (e) {
    case NHOOD_ARGS_OK: return SGL_OK;
    case NHOOD_ARGS_NULL: sgl_set_error("%s: NULL Gi, Gp, lab or labs", who); break;
    case NHOOD_ARGS_N: sgl_set_error("%s: n = %lld: at least one cell", who, (long long)n); break;
    case NHOOD_ARGS_PTR: sgl_set_error("%s: Gp[%lld] = %lld: Gp starts at 0 and never descends", who, (long long)at, (long long)val); break;
    case NHOOD_ARGS_ROW: sgl_set_error("%s: Gi[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)n); break;
    case NHOOD_ARGS_K: sgl_set_error("%s: K = %lld is outside [1, %d]", who, (long long)K, NHOOD_MAX_K); break;
    case NHOOD_ARGS_LABEL: sgl_set_error("%s: lab[%lld] = %lld is outside [0, %lld)", who, (long long)at, (long long)val, (long long)K); break;
    case NHOOD_ARGS_NPERM: sgl_set_error("%s: nperm = %lld is outside [1, %lld]", who, (long long)val, (long long)NHOOD_MAX_NPERM); break;
    case NHOOD_ARGS_OVERFLOW:
        sgl_set_error("%s: nperm = %lld: nperm * nnz^2 reaches 2^63 and the sum of squared counts would not fit int64; the largest nperm that fits is %lld",
                      who, (long long)nperm, (long long)val);
        break;
    case NHOOD_ARGS_BATCH: sgl_set_error("%s: batch = %lld is negative", who, (long long)val); break;
    case NHOOD_ARGS_PATH: sgl_set_error("%s: path = %lld is none of 0 (automatic), 1 (LDS), 2 (global)", who, (long long)val); break;
    case NHOOD_ARGS_PG:
        sgl_set_error("%s: perms_per_group = %lld is no power of two in [1, %lld] (what this path holds at K = %lld)", who, (long long)val, (long long)at,
                      (long long)K);
        break;
    case NHOOD_ARGS_RANGE: sgl_set_error("%s: permutations [%lld, %lld + %lld): not 0 <= r0, 1 <= nb, r0 + nb <= %lld", who, (long long)at, (long long)at, (long long)val, (long long)NHOOD_MAX_NPERM); break;
    case NHOOD_ARGS_NB: sgl_set_error("%s: nb = %lld: at least one label vector", who, (long long)val); break;
    }
    return SGL_EINVAL;
}

int sgl_nhood_args_check(const char* who, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* lab, int64_t K, int64_t nperm, int64_t batch) {
    int64_t at = -1, val = 0;
    const NhoodArgError e = nhood_check_call(Gi, Gp, n, lab, K, nperm, batch, &at, &val);
    return nh_refuse(who, e, n, K, nperm, at, val);
}

int sgl_nhood_permute_args_check(const char* who, int64_t n, const int32_t* lab, int64_t r0, int64_t nb) {
    int64_t at = -1, val = 0;
    NhoodArgError e = !lab ? NHOOD_ARGS_NULL : (n < 1 ? NHOOD_ARGS_N : NHOOD_ARGS_OK);
    if (e == NHOOD_ARGS_OK) e = nhood_check_labels(lab, n, 1, NHOOD_MAX_K, &at, &val);
    if (e == NHOOD_ARGS_OK && (e = nhood_check_range(r0, nb)) != NHOOD_ARGS_OK) { at = r0; val = nb; }
    return nh_refuse(who, e, n, NHOOD_MAX_K, 1, at, val);
}

int sgl_nhood_tally_args_check(const char* who, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* labs, int64_t nb, int64_t K, int path,
                               int64_t pg) {
    int64_t at = -1, val = 0;
    NhoodArgError e = (!Gi || !Gp || !labs) ? NHOOD_ARGS_NULL : nhood_check_graph(Gi, Gp, n, &at, &val);
    if (e == NHOOD_ARGS_OK && nb < 1) { e = NHOOD_ARGS_NB; val = nb; }
    if (e == NHOOD_ARGS_OK) e = nhood_check_labels(labs, n, nb, K, &at, &val);
    if (e == NHOOD_ARGS_OK) {
        NhoodPlan P;
        e = nhood_plan(n, Gp[n], K, nb, 0, path, pg, 0, &P, &at, &val);
    }
    return nh_refuse(who, e, n, K, 1, at, val);
}

static int nh_finish(sgl_ctx* c, int rc) {   // every return path waits for the stream before the buffers (and the host arrays) go
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == SGL_OK && e != hipSuccess) { (void)hipGetLastError(); sgl_set_error("nhood: HIP call failed: %s", hipGetErrorString(e)); return SGL_EHIP; }
    return rc;
}

static int nh_permute_on(sgl_ctx* c, int64_t n, const int32_t* lab, uint64_t seed, int64_t r0, int64_t nb, int32_t* lab_out) {
    hipStream_t s = c->stream;
    NhoodPlan P;
    int64_t at, val;
    (void)nhood_plan(n, 0, NHOOD_MAX_K, nb, 0, 2, NHOOD_MAX_PG, nh_sort_switch(), &P, &at, &val);
    const int pg = NHOOD_MAX_PG;
    DevBuf<int32_t> dlab;
    DevBuf<uint8_t> d8;
    NhPermuter Q;
    SGLCHK(dlab.alloc((size_t)n));
    SGLCHK(Q.alloc(n, P));
    const int64_t chunk = P.sort_perms;   // a multiple of 16: the permutations downloaded at a time
    SGLCHK(d8.alloc((size_t)chunk * (size_t)n));
    HIPCHK(hipMemcpyAsync(dlab.p, lab, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    std::vector<uint8_t> h8((size_t)chunk * (size_t)n);
    int64_t batches = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += chunk, ++batches) {
        const int64_t nq = std::min(chunk, nb - b0);
        SGLCHK(nh_permute(c, Q, dlab.p, n, seed, r0 + b0, nq, pg, d8.p));
        const size_t bytes = (size_t)((nq + pg - 1) / pg) * (size_t)n * (size_t)pg;
        HIPCHK(hipMemcpyAsync(h8.data(), d8.p, bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (lab_out)
            for (int64_t l = 0; l < nq; ++l) {
                const uint8_t* src = h8.data() + (size_t)(l / pg) * (size_t)n * (size_t)pg + (size_t)(l % pg);
                int32_t* dst = lab_out + (size_t)(b0 + l) * (size_t)n;
                for (int64_t cell = 0; cell < n; ++cell) dst[cell] = src[(size_t)cell * (size_t)pg];
            }
    }
    P.path = 0;
    nh_record(c, P, batches, chunk);
    return SGL_OK;
}
int sgl_nhood_permute_core(sgl_ctx* c, int64_t n, const int32_t* lab, uint64_t seed, int64_t r0, int64_t nb, int32_t* lab_out) {
    return nh_finish(c, nh_permute_on(c, n, lab, seed, r0, nb, lab_out));
}

static int nh_tally_on(sgl_ctx* c, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* labs, int64_t nb, int K, int drop, int path,
                       int64_t pg, int64_t* counts_out) {
    hipStream_t s = c->stream;
    NhoodPlan P;
    int64_t at, val;
    if (nhood_plan(n, Gp[n], K, nb, 0, path, pg, 0, &P, &at, &val) != NHOOD_ARGS_OK) { sgl_set_error("nhood: the plan refused knobs the check accepted"); return SGL_EINVAL; }
    const int64_t KK = (int64_t)K * K;
    // the label vectors in chunks of a whole number of groups within the batch budget
    int64_t chunk = std::max<int64_t>(NHOOD_BATCH_BYTES / (5 * n + 8 * KK), 1);
    chunk = std::max<int64_t>(chunk - chunk % NHOOD_MAX_PG, NHOOD_MAX_PG);
    chunk = std::min(chunk, (nb + NHOOD_MAX_PG - 1) / NHOOD_MAX_PG * NHOOD_MAX_PG);
    NhGraph G;
    DevBuf<int32_t> dlabs;
    DevBuf<uint8_t> d8;
    DevBuf<int64_t> dcounts;
    SGLCHK(G.upload(c, Gi, Gp, n));
    SGLCHK(dlabs.alloc((size_t)chunk * (size_t)n));
    SGLCHK(d8.alloc((size_t)chunk * (size_t)n));
    SGLCHK(dcounts.alloc((size_t)chunk * (size_t)KK));
    int64_t batches = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += chunk, ++batches) {
        const int64_t nq = std::min(chunk, nb - b0);
        HIPCHK(hipMemcpyAsync(dlabs.p, labs + (size_t)b0 * (size_t)n, sizeof(int32_t) * (size_t)nq * (size_t)n, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(dcounts.p, 0, sizeof(int64_t) * (size_t)nq * (size_t)KK, s));
        {
            Phase ph(c, SGL_PH_SCALE);
            SGLCHK(nh_gather(s, P.pg, nullptr, dlabs.p, n, n, nq, d8.p));
        }
        SGLCHK(nh_tally(c, G, P, P.pg, d8.p, n, K, drop, nq, dcounts.p));
        if (counts_out) HIPCHK(hipMemcpyAsync(counts_out + (size_t)b0 * (size_t)KK, dcounts.p, sizeof(int64_t) * (size_t)nq * (size_t)KK, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    nh_record(c, P, batches, chunk);
    return SGL_OK;
}
int sgl_nhood_tally_core(sgl_ctx* c, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* labs, int64_t nb, int K, int drop, int path,
                         int64_t pg, int64_t* counts_out) {
    return nh_finish(c, nh_tally_on(c, Gi, Gp, n, labs, nb, K, drop, path, pg, counts_out));
}

static int nh_all_on(sgl_ctx* c, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* lab, int K, int drop, int64_t nperm, uint64_t seed,
                     int64_t batch, int64_t* counts, int64_t* S1, int64_t* S2, int64_t* n_ge, int64_t* n_le, int64_t* null_out, double* stage_ms) {
    hipStream_t s = c->stream;
    NhoodPlan P;
    int64_t at, val;
    if (nhood_plan(n, Gp[n], K, nperm, batch, 0, 0, nh_sort_switch(), &P, &at, &val) != NHOOD_ARGS_OK) { sgl_set_error("nhood: the plan refused a batch the check accepted"); return SGL_EINVAL; }
    const int64_t KK = (int64_t)K * K, B = P.batch;
    const int64_t groups = (B + P.pg - 1) / P.pg;
    if (stage_ms) std::fill(stage_ms, stage_ms + 3, 0.0);
    NhTimer T(s, stage_ms);
    NhGraph G;
    DevBuf<int32_t> dlab;
    DevBuf<uint8_t> d8;
    DevBuf<int64_t> dcb, dacc;   // the batch's counts; C | S1 | S2 | n_ge | n_le
    NhPermuter Q;
    SGLCHK(G.upload(c, Gi, Gp, n));
    SGLCHK(dlab.alloc((size_t)n));
    SGLCHK(d8.alloc((size_t)groups * (size_t)P.pg * (size_t)n));
    SGLCHK(dcb.alloc((size_t)B * (size_t)KK));
    SGLCHK(dacc.alloc(5 * (size_t)KK));
    SGLCHK(Q.alloc(n, P));
    HIPCHK(hipMemcpyAsync(dlab.p, lab, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dacc.p, 0, sizeof(int64_t) * 5 * (size_t)KK, s));
    // the observed counts: the identity, one label vector per group
    T.begin();
    {
        Phase ph(c, SGL_PH_SCALE);
        SGLCHK(nh_gather(s, 1, nullptr, dlab.p, 0, n, 1, d8.p));
    }
    T.end(0);
    T.begin();
    SGLCHK(nh_tally(c, G, P, 1, d8.p, n, K, drop, 1, dacc.p));
    T.end(1);
    int64_t batches = 0;
    for (int64_t b0 = 0; b0 < nperm; b0 += B, ++batches) {
        const int64_t nb = std::min(B, nperm - b0);
        T.begin();
        SGLCHK(nh_permute(c, Q, dlab.p, n, seed, b0, nb, P.pg, d8.p));
        T.end(0);
        T.begin();
        HIPCHK(hipMemsetAsync(dcb.p, 0, sizeof(int64_t) * (size_t)nb * (size_t)KK, s));
        SGLCHK(nh_tally(c, G, P, P.pg, d8.p, n, K, drop, nb, dcb.p));
        T.end(1);
        T.begin();
        {
            Phase ph(c, SGL_PH_SCALE);
            nh_reduce_kernel<<<dim3(nh_blocks(KK)), dim3(NH_THREADS), 0, s>>>(dcb.p, KK, nb, dacc.p, dacc.p + KK, dacc.p + 2 * KK, dacc.p + 3 * KK,
                                                                            dacc.p + 4 * KK);
            HIPCHK(hipGetLastError());
        }
        T.end(2);
        if (null_out) HIPCHK(hipMemcpyAsync(null_out + (size_t)b0 * (size_t)KK, dcb.p, sizeof(int64_t) * (size_t)nb * (size_t)KK, hipMemcpyDeviceToHost, s));
    }
    std::vector<int64_t> h(5 * (size_t)KK);
    HIPCHK(hipMemcpyAsync(h.data(), dacc.p, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int64_t* outs[5] = {counts, S1, S2, n_ge, n_le};
    for (int q = 0; q < 5; ++q)
        if (outs[q]) std::copy(h.begin() + q * KK, h.begin() + (q + 1) * KK, outs[q]);
    nh_record(c, P, batches, B);
    return SGL_OK;
}
int sgl_nhood_all(sgl_ctx* c, const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* lab, int K, int drop, int64_t nperm, uint64_t seed,
                  int64_t batch, int64_t* counts, int64_t* S1, int64_t* S2, int64_t* n_ge, int64_t* n_le, int64_t* null_out, double* stage_ms) {
    return nh_finish(c, nh_all_on(c, Gi, Gp, n, lab, K, drop, nperm, seed, batch, counts, S1, S2, n_ge, n_le, null_out, stage_ms));
}

// ---- the label tables for the other permutation tests (kernels_ligrec.hip) --------------------------------------------------------------
// The same keys, sorts and gather, always in groups of NHOOD_MAX_PG: vector l of the table is byte l % 16 of cell c in group l / 16,
// out8[((l / 16) n + c) 16 + l % 16].  Nothing of the neighbourhood calls above goes through these.
struct sgl_nhood_labeller {
    NhPermuter Q;
};
int sgl_nhood_labeller_create(sgl_ctx* c, int64_t n, int64_t batch, sgl_nhood_labeller** out) {
    (void)c;
    NhoodPlan P;
    int64_t at, val;
    (void)nhood_plan(n, 0, NHOOD_MAX_K, batch, 0, 2, NHOOD_MAX_PG, nh_sort_switch(), &P, &at, &val);
    sgl_nhood_labeller* h = new sgl_nhood_labeller;
    const int rc = h->Q.alloc(n, P);
    if (rc != SGL_OK) { delete h; return rc; }
    *out = h;
    return SGL_OK;
}
void sgl_nhood_labeller_free(sgl_nhood_labeller* h) { delete h; }
int sgl_nhood_labels_permuted(sgl_ctx* c, sgl_nhood_labeller* h, const int32_t* dlab, int64_t n, uint64_t seed, int64_t r0, int64_t nb, uint8_t* out8) {
    return nh_permute(c, h->Q, dlab, n, seed, r0, nb, NHOOD_MAX_PG, out8);
}
int sgl_nhood_labels_given(sgl_ctx* c, const int32_t* dlabs, int64_t lab_stride, int64_t n, int64_t np, uint8_t* out8) {
    Phase ph(c, SGL_PH_SCALE);
    return nh_gather(c->stream, NHOOD_MAX_PG, nullptr, dlabs, lab_stride, n, np, out8);
}
