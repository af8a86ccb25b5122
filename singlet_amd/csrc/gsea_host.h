// Host logic of sgl_c_gsea (include/singlet_hip.h, "Gene set enrichment") that makes no HIP call: the argument rules and the
// naming of the offender, the table of distinct set sizes, the batch plan of the permutations, and the derived statistics
// (p, NES, the same-side tally, Benjamini-Hochberg) from the integer tallies and running sums of the device.  Plain C++ over
// plain pointers, so tests/gsea_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#ifdef __HIPCC__
#define GSEA_HD __host__ __device__
#else
#define GSEA_HD
#endif

#define GSEA_MAX_K 1024
#define GSEA_LDS_CAP 4096                       // genes of a set that one wave sorts and scores in LDS
#define GSEA_MAX_NPERM ((int32_t)1 << 20)
#define GSEA_BLOCK 64                           // hits per block of the prefix sums: part of the stated summation order
#define GSEA_NULL_BYTES ((int64_t)256 << 20)    // default budget of one batch of null scores: k x sizes x batch x 8 bytes
#define GSEA_SORT_ITEMS ((int64_t)1 << 24)      // keys of one segmented sort of the null sample (whole permutations)

enum GseaArgError {
    GSEA_ARGS_OK = 0,
    GSEA_ARGS_NULL,        // w, set_ptr or set_genes == NULL
    GSEA_ARGS_K,           // k outside [1, 1024]
    GSEA_ARGS_GENES,       // m < 2
    GSEA_ARGS_SETS,        // n_sets < 1
    GSEA_ARGS_SCORE,       // score_type outside {0, 1, 2}
    GSEA_ARGS_NPERM,       // nperm outside [1, 2^20]
    GSEA_ARGS_BATCH,       // a negative forced batch size
    GSEA_ARGS_W,           // w[*at] is not finite
    GSEA_ARGS_PTR,         // set_ptr[0] != 0 (*at = 0) or set_ptr[*at] < set_ptr[*at - 1]
    GSEA_ARGS_EMPTY,       // set *at is empty
    GSEA_ARGS_WHOLE,       // set *at holds *val >= m genes
    GSEA_ARGS_CAP,         // set *at holds *val > GSEA_LDS_CAP genes
    GSEA_ARGS_GENE,        // set_genes[*at] = *val is outside [0, m)
    GSEA_ARGS_TWICE,       // set_genes[*at] = *val occurs twice in its set
    GSEA_ARGS_SIZES,       // (stage operator) sizes[*at] = *val is not in [1, min(m - 1, cap)] or not above sizes[*at - 1]
    GSEA_ARGS_RANGE,       // (stage operator) not 0 <= r0 < r1 <= 2^20
};

// The scalar refusals, in this order; nothing is read through the pointers.
inline GseaArgError gsea_check_scalars(int64_t m, int64_t k, int score_type, int64_t nperm, int64_t batch) {
    if (k < 1 || k > GSEA_MAX_K) return GSEA_ARGS_K;
    if (m < 2) return GSEA_ARGS_GENES;
    if (score_type < 0 || score_type > 2) return GSEA_ARGS_SCORE;
    if (nperm < 1 || nperm > GSEA_MAX_NPERM) return GSEA_ARGS_NPERM;
    if (batch < 0) return GSEA_ARGS_BATCH;
    return GSEA_ARGS_OK;
}

// the first entry of w (m x k, column-major) that is not finite: GSEA_ARGS_W with *at its offset
inline GseaArgError gsea_check_w(const double* w, int64_t m, int64_t k, int64_t* at) {
    for (int64_t q = 0; q < m * k; ++q)
        if (!(w[q] - w[q] == 0.0)) { *at = q; return GSEA_ARGS_W; }
    return GSEA_ARGS_OK;
}

// The refusals of the gene sets, the whole list read before anything is launched: first set_ptr over all sets (ascending,
// no empty set, no set of m genes or more, none above the cap), then the genes set by set (range, then twice).  `stamp`
// is scratch of m values.
inline GseaArgError gsea_check_sets(const int64_t* set_ptr, const int32_t* set_genes, int64_t n_sets, int64_t m, int32_t* stamp,
                                    int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (set_ptr[0] != 0) { *at = 0; *val = set_ptr[0]; return GSEA_ARGS_PTR; }
    for (int64_t j = 0; j < n_sets; ++j) {
        const int64_t s = set_ptr[j + 1] - set_ptr[j];
        *at = j;
        *val = s;
        if (s < 0) { *at = j + 1; *val = set_ptr[j + 1]; return GSEA_ARGS_PTR; }
        if (s == 0) return GSEA_ARGS_EMPTY;
        if (s >= m) return GSEA_ARGS_WHOLE;
        if (s > GSEA_LDS_CAP) return GSEA_ARGS_CAP;
    }
    for (int64_t g = 0; g < m; ++g) stamp[g] = -1;
    for (int64_t j = 0; j < n_sets; ++j)
        for (int64_t q = set_ptr[j]; q < set_ptr[j + 1]; ++q) {
            const int32_t g = set_genes[q];
            *at = q;
            *val = g;
            if (g < 0 || g >= m) return GSEA_ARGS_GENE;
            if (stamp[g] == (int32_t)j) return GSEA_ARGS_TWICE;
            stamp[g] = (int32_t)j;
        }
    *at = -1;
    *val = 0;
    return GSEA_ARGS_OK;
}

// the sizes of the null stage operator: strictly ascending, each in [1, min(m - 1, cap)]
inline GseaArgError gsea_check_sizes(const int32_t* sizes, int64_t n_sizes, int64_t m, int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (!sizes) return GSEA_ARGS_NULL;
    if (n_sizes < 1) return GSEA_ARGS_SETS;
    for (int64_t i = 0; i < n_sizes; ++i) {
        const int64_t s = sizes[i];
        if (s < 1 || s >= m || s > GSEA_LDS_CAP || (i > 0 && s <= sizes[i - 1])) { *at = i; *val = s; return GSEA_ARGS_SIZES; }
    }
    return GSEA_ARGS_OK;
}

// The table of distinct set sizes, ascending: sizes (room for n_sets) and size_idx[j] = the place of set j's size in it;
// set_size[j] (may be NULL) receives the sizes themselves.  Returns the number of distinct sizes.
inline int64_t gsea_size_table(const int64_t* set_ptr, int64_t n_sets, int32_t* sizes, int32_t* size_idx, int32_t* set_size) {
    std::vector<int32_t> all((size_t)n_sets);
    for (int64_t j = 0; j < n_sets; ++j) all[(size_t)j] = (int32_t)(set_ptr[j + 1] - set_ptr[j]);
    if (set_size) std::copy(all.begin(), all.end(), set_size);
    std::vector<int32_t> u(all);
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    std::copy(u.begin(), u.end(), sizes);
    for (int64_t j = 0; j < n_sets; ++j)
        size_idx[j] = (int32_t)(std::lower_bound(u.begin(), u.end(), all[(size_t)j]) - u.begin());
    return (int64_t)u.size();
}

// Permutations per batch: the forced size when one is given (> 0), else what the budget of k x n_sizes x batch x 8 bytes
// allows; at least 1, at most nperm.  The results of the library do not depend on it.
inline int64_t gsea_batch_size(int64_t k, int64_t n_sizes, int64_t nperm, int64_t forced, int64_t budget_bytes) {
    int64_t b = forced > 0 ? forced : (budget_bytes > 0 ? budget_bytes : GSEA_NULL_BYTES) / (k * n_sizes * 8);
    if (b < 1) b = 1;
    if (b > nperm) b = nperm;
    return b;
}
// whole permutations per segmented sort of the null sample: at most GSEA_SORT_ITEMS keys, at least one permutation
inline int64_t gsea_sort_perms(int64_t m, int64_t batch) {
    int64_t b = GSEA_SORT_ITEMS / m;
    if (b < 1) b = 1;
    return b < batch ? b : batch;
}

// std: the score that is larger in magnitude, +0.0 when the two are equal in magnitude
GSEA_HD inline double gsea_std_score(double es_pos, double es_neg) {
    const double a = fabs(es_neg);
    return es_pos > a ? es_pos : (es_pos < a ? es_neg : 0.0);
}

// The derived statistics of set j in factor f (P x k column-major, set fastest) from the observed score, the tallies of
// the set (n_ge, n_le) and those of its size in the factor (n_sizes x k, size fastest: the nulls >= 0 and <= 0, and their
// sums added in ascending r).  Any output may be NULL.
inline void gsea_derive(int64_t P, int64_t k, int score_type, int64_t nperm, const int32_t* size_idx, int64_t n_sizes, const double* es,
                        const int64_t* n_ge, const int64_t* n_le, const int64_t* cnt_pos, const int64_t* cnt_neg, const double* sum_pos,
                        const double* sum_neg, double* nes, double* pval, int64_t* n_side) {
    for (int64_t f = 0; f < k; ++f)
        for (int64_t j = 0; j < P; ++j) {
            const size_t at = (size_t)j + (size_t)P * (size_t)f, sz = (size_t)size_idx[j] + (size_t)n_sizes * (size_t)f;
            const double e = es[at];
            const bool upper = score_type == 0 || (score_type == 2 && e >= 0.0);   // the side of the null this score is held to
            const int64_t side = upper ? cnt_pos[sz] : cnt_neg[sz];
            const int64_t hits = upper ? n_ge[at] : n_le[at];
            const int64_t denom = score_type == 2 ? side : nperm;
            if (pval) pval[at] = (double)(1 + hits) / (double)(1 + denom);
            if (n_side) n_side[at] = side;
            if (nes) {
                double v = NAN;
                if (side > 0) {
                    const double mean = (upper ? sum_pos[sz] : sum_neg[sz]) / (double)side;
                    if (mean != 0.0) v = e / fabs(mean);
                }
                nes[at] = v;
            }
        }
}

// Benjamini-Hochberg over the n values of p that are not NaN (a NaN stays NaN): the values in ascending order (ties by
// index), rank i = 1 .. n_valid; padj of rank i = min(1, min over i' >= i of ((double)n_valid / (double)i') * p_(i')).
inline void gsea_bh(const double* p, int64_t n, double* padj) {
    std::vector<int64_t> o;
    o.reserve((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        if (p[j] == p[j]) o.push_back(j);
        else padj[j] = NAN;
    }
    std::sort(o.begin(), o.end(), [p](int64_t a, int64_t b) { return p[a] < p[b] || (p[a] == p[b] && a < b); });
    const double nv = (double)o.size();
    double run = INFINITY;
    for (int64_t i = (int64_t)o.size(); i >= 1; --i) {
        const double v = (nv / (double)i) * p[o[(size_t)i - 1]];
        if (v < run) run = v;
        padj[o[(size_t)i - 1]] = run < 1.0 ? run : 1.0;
    }
}
