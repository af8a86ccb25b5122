// Host logic of the neighbourhood enrichment calls (include/singlet_hip.h, "Neighbourhood enrichment") that makes no HIP call:
// the argument rules and the naming of the offender, the plan (path, permutations per group, LDS bytes, batch, sort) as a pure
// function of the sizes and the knobs, and the statistics from the integer tallies in exact 128-bit arithmetic.  Plain C++ over
// plain pointers, so tests/nhood_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include "gsea_host.h"   // gsea_bh: Benjamini-Hochberg under the one rule of the library

#define NHOOD_MAX_K 256                            // a label is one byte of the interleaved label table
#define NHOOD_MAX_NPERM ((int64_t)1 << 20)
#define NHOOD_MAX_PG 16                            // permutations per group: the labels of a cell in one 16-byte load
#define NHOOD_LDS_TILE_BYTES ((int64_t)128 << 10)  // the PG x K x K uint32 tiles of a workgroup: 128 KiB of the CU's 160 KiB
#define NHOOD_SEG 4096                             // stored entries per segment; a workgroup takes whole segments
#define NHOOD_MAX_WG 512                           // workgroups over the entries of one group (above, a workgroup takes more segments)
#define NHOOD_BATCH_BYTES ((int64_t)256 << 20)     // default budget of a batch: per permutation n label bytes + K x K x 8 count bytes
#define NHOOD_SORT_SWITCH ((int64_t)32768)         // cells up to which the permutations are sorted as segments of ONE segmented sort
#define NHOOD_SORT_ITEMS ((int64_t)1 << 24)        // keys in flight of one sort chunk (whole permutations, a multiple of 16, at least 16)

enum NhoodArgError {
    NHOOD_ARGS_OK = 0,
    NHOOD_ARGS_NULL,       // Gi, Gp or lab == NULL
    NHOOD_ARGS_N,          // n < 1
    NHOOD_ARGS_PTR,        // Gp[0] != 0 (*at = 0) or Gp[*at] < Gp[*at - 1]
    NHOOD_ARGS_ROW,        // Gi[*at] = *val is outside [0, n)
    NHOOD_ARGS_K,          // K outside [1, 256]
    NHOOD_ARGS_LABEL,      // lab[*at] = *val is outside [0, K)
    NHOOD_ARGS_NPERM,      // nperm outside [1, 2^20]
    NHOOD_ARGS_OVERFLOW,   // nperm * nnz^2 >= 2^63; *val = the largest nperm that fits
    NHOOD_ARGS_BATCH,      // a negative batch
    NHOOD_ARGS_PATH,       // path outside {0, 1, 2}
    NHOOD_ARGS_PG,         // perms_per_group = *val is no power of two in [1, 16], or above what the LDS path holds at this K (*at)
    NHOOD_ARGS_RANGE,      // not 0 <= r0, 1 <= nb, r0 + nb <= 2^20
    NHOOD_ARGS_NB,         // nb < 1
};

// the graph's structure: Gp starts at 0 and never descends, every row in [0, n); rows may repeat and need not be sorted
inline NhoodArgError nhood_check_graph(const int32_t* Gi, const int32_t* Gp, int64_t n, int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (!Gi || !Gp) return NHOOD_ARGS_NULL;
    if (n < 1) return NHOOD_ARGS_N;
    if (Gp[0] != 0) { *at = 0; *val = Gp[0]; return NHOOD_ARGS_PTR; }
    for (int64_t j = 1; j <= n; ++j)
        if (Gp[j] < Gp[j - 1]) { *at = j; *val = Gp[j]; return NHOOD_ARGS_PTR; }
    for (int64_t e = 0; e < Gp[n]; ++e)
        if (Gi[e] < 0 || Gi[e] >= n) { *at = e; *val = Gi[e]; return NHOOD_ARGS_ROW; }
    return NHOOD_ARGS_OK;
}

// count label vectors of n labels each, all in [0, K); *at is the offset into lab
inline NhoodArgError nhood_check_labels(const int32_t* lab, int64_t n, int64_t count, int64_t K, int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (!lab) return NHOOD_ARGS_NULL;
    if (K < 1 || K > NHOOD_MAX_K) return NHOOD_ARGS_K;
    for (int64_t q = 0; q < n * count; ++q)
        if (lab[q] < 0 || lab[q] >= K) { *at = q; *val = lab[q]; return NHOOD_ARGS_LABEL; }
    return NHOOD_ARGS_OK;
}

// the largest nperm with nperm * nnz^2 < 2^63: S2 = sum_r C_r^2 <= nperm * nnz^2 then fits int64 (nnz = 0: no limit)
inline int64_t nhood_max_nperm(int64_t nnz) {
    if (nnz <= 0) return INT64_MAX;
    const unsigned __int128 sq = (unsigned __int128)nnz * (unsigned __int128)nnz;
    const unsigned __int128 q = ((((unsigned __int128)1) << 63) - 1) / sq;
    return q > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)q;
}

inline NhoodArgError nhood_check_nperm(int64_t nperm, int64_t nnz, int64_t batch, int64_t* val) {
    if (nperm < 1 || nperm > NHOOD_MAX_NPERM) { *val = nperm; return NHOOD_ARGS_NPERM; }
    if (nperm > nhood_max_nperm(nnz)) { *val = nhood_max_nperm(nnz); return NHOOD_ARGS_OVERFLOW; }
    if (batch < 0) { *val = batch; return NHOOD_ARGS_BATCH; }
    return NHOOD_ARGS_OK;
}

// every refusal of the whole call, in the stated order
inline NhoodArgError nhood_check_call(const int32_t* Gi, const int32_t* Gp, int64_t n, const int32_t* lab, int64_t K, int64_t nperm, int64_t batch,
                                      int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (!Gi || !Gp || !lab) return NHOOD_ARGS_NULL;
    NhoodArgError e = nhood_check_graph(Gi, Gp, n, at, val);
    if (e == NHOOD_ARGS_OK) e = nhood_check_labels(lab, n, 1, K, at, val);
    if (e == NHOOD_ARGS_OK) e = nhood_check_nperm(nperm, Gp[n], batch, val);
    return e;
}

// the permutations [r0, r0 + nb) of the stage operator
inline NhoodArgError nhood_check_range(int64_t r0, int64_t nb) {
    return (r0 >= 0 && nb >= 1 && nb <= NHOOD_MAX_NPERM && r0 <= NHOOD_MAX_NPERM - nb) ? NHOOD_ARGS_OK : NHOOD_ARGS_RANGE;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------
// the most permutations per group whose K x K uint32 tiles fit the LDS budget: 16 up to K = 45, 8 up to 64, 4 up to 90, 2 up to
// 128, 1 up to 181; 0 above (no tile fits: the global path)
inline int nhood_pg_max(int64_t K) {
    for (int pg = NHOOD_MAX_PG; pg >= 1; pg >>= 1)
        if ((int64_t)pg * K * K * 4 <= NHOOD_LDS_TILE_BYTES) return pg;
    return 0;
}

struct NhoodPlan {
    int path;             // 1 the LDS path, 2 the global path
    int pg;               // permutations per group
    int64_t lds_bytes;    // dynamic LDS of a workgroup of the tally (0 on the global path)
    int64_t batch;        // permutations per batch
    int sort;             // 0 one segmented sort over the permutations of a chunk, 1 one device-wide sort per permutation
    int64_t sort_perms;   // permutations per sort chunk: a multiple of 16
    int64_t wg_entries;   // stored entries per workgroup of the tally: a whole number of segments
    int64_t wgs;          // workgroups over the entries of one group
};

// path 0 automatic / 1 the LDS path (K above 181 still takes the global path) / 2 the global path; pg 0: the plan's value;
// batch 0: by the budget; sort_switch 0: NHOOD_SORT_SWITCH.  NHOOD_ARGS_PATH / _PG / _BATCH on a knob that is not admissible.
inline NhoodArgError nhood_plan(int64_t n, int64_t nnz, int64_t K, int64_t nperm, int64_t batch, int path, int64_t pg, int64_t sort_switch,
                                NhoodPlan* P, int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (path < 0 || path > 2) { *val = path; return NHOOD_ARGS_PATH; }
    if (batch < 0) { *val = batch; return NHOOD_ARGS_BATCH; }
    const int pg_max = nhood_pg_max(K);
    P->path = (path == 2 || pg_max == 0) ? 2 : 1;
    const int64_t cap = P->path == 1 ? pg_max : NHOOD_MAX_PG;
    if (pg < 0 || pg > cap || (pg & (pg - 1)) != 0) { *at = cap; *val = pg; return NHOOD_ARGS_PG; }
    P->pg = pg > 0 ? (int)pg : (int)cap;
    P->lds_bytes = P->path == 1 ? (int64_t)P->pg * K * K * 4 : 0;
    int64_t b = batch;
    if (b == 0) {
        b = NHOOD_BATCH_BYTES / (n + 8 * K * K);
        b -= b % NHOOD_MAX_PG;
        if (b < NHOOD_MAX_PG) b = NHOOD_MAX_PG;
    }
    P->batch = b < nperm ? b : nperm;
    P->sort = n > (sort_switch > 0 ? sort_switch : NHOOD_SORT_SWITCH) ? 1 : 0;
    int64_t q = NHOOD_SORT_ITEMS / n;
    q -= q % NHOOD_MAX_PG;
    if (q < NHOOD_MAX_PG) q = NHOOD_MAX_PG;
    const int64_t bcap = (P->batch + NHOOD_MAX_PG - 1) / NHOOD_MAX_PG * NHOOD_MAX_PG;
    P->sort_perms = q < bcap ? q : bcap;
    int64_t per = (nnz + NHOOD_MAX_WG - 1) / NHOOD_MAX_WG;
    per = (per + NHOOD_SEG - 1) / NHOOD_SEG * NHOOD_SEG;
    P->wg_entries = per > NHOOD_SEG ? per : NHOOD_SEG;
    P->wgs = (nnz + P->wg_entries - 1) / P->wg_entries;
    return NHOOD_ARGS_OK;
}

// ---- the statistics ---------------------------------------------------------------------------------------------------------------
// D = nperm * S2 - S1^2, exact: S1 < 2^51 and S2 < 2^63 by the refusals, so both products fit 128 bits
inline __int128 nhood_D(int64_t nperm, int64_t S1, int64_t S2) {
    return (__int128)nperm * (__int128)S2 - (__int128)S1 * (__int128)S1;
}

// z, mean, sd, p and Benjamini-Hochberg of the K x K pairs; any output may be NULL.  An integer becomes a double by ONE
// conversion, round to nearest even (the compiler's __int128 -> double conversion).
inline void nhood_stats(int64_t K, int64_t nperm, const int64_t* counts, const int64_t* S1, const int64_t* S2, const int64_t* n_ge,
                        const int64_t* n_le, double* z, double* mean, double* sd, double* p_enr, double* p_dep, double* padj_enr,
                        double* padj_dep) {
    const int64_t KK = K * K;
    std::vector<double> pe((size_t)KK), pd((size_t)KK);
    for (int64_t q = 0; q < KK; ++q) {
        const __int128 D = nhood_D(nperm, S1[q], S2[q]);
        const double root = sqrt((double)D);
        if (mean) mean[q] = (double)S1[q] / (double)nperm;
        if (sd) sd[q] = root / (double)nperm;
        if (z) z[q] = D == 0 ? NAN : (double)((__int128)nperm * (__int128)counts[q] - (__int128)S1[q]) / root;
        pe[(size_t)q] = (double)(1 + n_ge[q]) / (double)(1 + nperm);
        pd[(size_t)q] = (double)(1 + n_le[q]) / (double)(1 + nperm);
    }
    if (p_enr) std::copy(pe.begin(), pe.end(), p_enr);
    if (p_dep) std::copy(pd.begin(), pd.end(), p_dep);
    if (padj_enr) gsea_bh(pe.data(), KK, padj_enr);
    if (padj_dep) gsea_bh(pd.data(), KK, padj_dep);
}
