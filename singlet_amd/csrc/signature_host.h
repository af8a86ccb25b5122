// Host logic of sgl_signature_scores (include/singlet_hip.h, "Signature scores") that makes no HIP call: the argument rules and
// the naming of the first defect, the gene -> sets table, the split of the cells into the LDS instances and the long path, the
// batches of the long path, the set passes, and the two formulas (the cap of a doubled midrank, the score of a rank sum) that
// the device evaluates with the same text.  Plain C++ over plain pointers, so tests/signature_host_main.cpp compiles it alone
// under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <stdint.h>

#include "ingest_host.h"

#ifdef __HIPCC__
#define SIG_HD __host__ __device__
#else
#define SIG_HD
#endif

#define SIGNATURE_LDS_SMALL 1024                     // stored non-zero entries of a cell that the small LDS instance sorts
#define SIGNATURE_LDS_CAP 4096                       // ... that the large LDS instance sorts: the default (and largest) lds_cap
#define SIGNATURE_PASS_SETS 1024                     // sets whose accumulators one pass holds in LDS: the default (and largest) pass
#define SIGNATURE_BATCH_ENTRIES ((int64_t)1 << 27)   // default entries per batch of the long path: 24 bytes of scratch each, 3 GiB

enum SignatureArgError {
    SIGNATURE_ARGS_OK = 0,
    SIGNATURE_ARGS_NULL,     // set_ptr or set_genes == NULL
    SIGNATURE_ARGS_SETS,     // n_sets < 1
    SIGNATURE_ARGS_RANK,     // max_rank outside [1, m]
    SIGNATURE_ARGS_KNOB,     // a negative knob: *at = 0 lds_cap, 1 max_batch_entries, 2 pass_sets; *val its value
    SIGNATURE_ARGS_PTR,      // set_ptr[0] != 0 (*at = 0) or set_ptr[*at] < set_ptr[*at - 1]
    SIGNATURE_ARGS_EMPTY,    // set *at is empty
    SIGNATURE_ARGS_SIZE,     // set *at holds *val > max_rank genes
    SIGNATURE_ARGS_GENE,     // set_genes[*at] = *val is outside [0, m)
    SIGNATURE_ARGS_TWICE,    // set_genes[*at] = *val occurs twice in its set
};

// The refusals that need no device, in this order: the scalars (n_sets, max_rank, the knobs), then set_ptr over all sets
// (ascending, no empty set, none above max_rank), then the genes set by set (range, then twice).  The whole list is read
// before anything is launched.  `stamp` is scratch of m values (unused when a scalar is refused; may be NULL when m < 1).
inline SignatureArgError signature_check_args(const int64_t* set_ptr, const int32_t* set_genes, int64_t n_sets, int64_t m, int64_t max_rank,
                                              int64_t lds_cap, int64_t max_batch_entries, int64_t pass_sets, int32_t* stamp, int64_t* at,
                                              int64_t* val) {
    *at = -1;
    *val = 0;
    if (!set_ptr || !set_genes) return SIGNATURE_ARGS_NULL;
    if (n_sets < 1) { *val = n_sets; return SIGNATURE_ARGS_SETS; }
    if (max_rank < 1 || max_rank > m) { *val = max_rank; return SIGNATURE_ARGS_RANK; }
    if (lds_cap < 0) { *at = 0; *val = lds_cap; return SIGNATURE_ARGS_KNOB; }
    if (max_batch_entries < 0) { *at = 1; *val = max_batch_entries; return SIGNATURE_ARGS_KNOB; }
    if (pass_sets < 0) { *at = 2; *val = pass_sets; return SIGNATURE_ARGS_KNOB; }
    if (set_ptr[0] != 0) { *at = 0; *val = set_ptr[0]; return SIGNATURE_ARGS_PTR; }
    for (int64_t j = 0; j < n_sets; ++j) {
        const int64_t s = set_ptr[j + 1] - set_ptr[j];
        *at = j;
        *val = s;
        if (s < 0) { *at = j + 1; *val = set_ptr[j + 1]; return SIGNATURE_ARGS_PTR; }
        if (s == 0) return SIGNATURE_ARGS_EMPTY;
        if (s > max_rank) return SIGNATURE_ARGS_SIZE;
    }
    for (int64_t g = 0; g < m; ++g) stamp[g] = -1;
    for (int64_t j = 0; j < n_sets; ++j)
        for (int64_t q = set_ptr[j]; q < set_ptr[j + 1]; ++q) {
            const int32_t g = set_genes[q];
            *at = q;
            *val = g;
            if (g < 0 || g >= m) return SIGNATURE_ARGS_GENE;
            if (stamp[g] == (int32_t)j) return SIGNATURE_ARGS_TWICE;
            stamp[g] = (int32_t)j;
        }
    *at = -1;
    *val = 0;
    return SIGNATURE_ARGS_OK;
}

// The gene -> sets table, the transpose of the sets: gene_sets[gene_ptr[g] .. gene_ptr[g + 1]) = the sets that hold gene g,
// ascending.  gene_ptr has m + 1 values, gene_sets set_ptr[n_sets].  Sets checked before.
inline void signature_gene_table(const int64_t* set_ptr, const int32_t* set_genes, int64_t n_sets, int64_t m, int64_t* gene_ptr,
                                 int32_t* gene_sets) {
    for (int64_t g = 0; g <= m; ++g) gene_ptr[g] = 0;
    for (int64_t q = 0; q < set_ptr[n_sets]; ++q) ++gene_ptr[(int64_t)set_genes[q] + 1];
    for (int64_t g = 0; g < m; ++g) gene_ptr[g + 1] += gene_ptr[g];
    for (int64_t j = 0; j < n_sets; ++j)        // ascending j: every gene's list comes out ascending; gene_ptr[g] runs ahead ...
        for (int64_t q = set_ptr[j]; q < set_ptr[j + 1]; ++q) gene_sets[gene_ptr[set_genes[q]]++] = (int32_t)j;
    for (int64_t g = m; g > 0; --g) gene_ptr[g] = gene_ptr[g - 1];   // ... to the start of the next gene: shifted back here
    gene_ptr[0] = 0;
}

// the caps in force: a knob of 0 is the default, a larger one is cut to it
inline int64_t signature_lds_cap(int64_t lds_cap) { return lds_cap > 0 && lds_cap < SIGNATURE_LDS_CAP ? lds_cap : SIGNATURE_LDS_CAP; }
inline int64_t signature_pass_size(int64_t pass_sets) { return pass_sets > 0 && pass_sets < SIGNATURE_PASS_SETS ? pass_sets : SIGNATURE_PASS_SETS; }
inline int64_t signature_passes(int64_t n_sets, int64_t pass_sets) {
    const int64_t ps = signature_pass_size(pass_sets);
    return (n_sets + ps - 1) / ps;
}

// The paths: cell c with len[c] stored non-zero entries is sorted by the small LDS instance when len[c] <= min(cap,
// SIGNATURE_LDS_SMALL), by the large one when len[c] <= cap, else it is long.  cap = signature_lds_cap(knob).  The three
// lists (room for n each) receive the cells in ascending order, long_len the counts of the long ones.
inline void signature_split_paths(const int64_t* len, int64_t n, int64_t cap, int32_t* small_list, int64_t* n_small, int32_t* large_list,
                                  int64_t* n_large, int32_t* long_list, int64_t* long_len, int64_t* n_long) {
    const int64_t small = cap < SIGNATURE_LDS_SMALL ? cap : SIGNATURE_LDS_SMALL;
    int64_t a = 0, b = 0, l = 0;
    for (int64_t c = 0; c < n; ++c) {
        if (len[c] <= small) small_list[a++] = (int32_t)c;
        else if (len[c] <= cap) large_list[b++] = (int32_t)c;
        else { long_list[l] = (int32_t)c; long_len[l] = len[c]; ++l; }
    }
    *n_small = a;
    *n_large = b;
    *n_long = l;
}

// the batch cap in force, and the batches of the long path: whole cells in list order, greedily, each batch at most the cap
// and never more than INT32_MAX entries, which the segmented sort counts in; a cell above the cap is a batch of its own (it
// holds at most m <= INT32_MAX entries).  cut has room for n + 1 values; returns the number of batches.
inline int64_t signature_batch_cap(int64_t max_batch_entries) {
    const int64_t cap = max_batch_entries > 0 ? max_batch_entries : SIGNATURE_BATCH_ENTRIES;
    return cap > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : cap;
}
inline int64_t signature_batches(const int64_t* len, int64_t n, int64_t max_batch_entries, int64_t* cut) {
    return ingest_batch_edges(len, n, signature_batch_cap(max_batch_entries), cut);
}

// the cap of a doubled midrank: ranks above max_rank become max_rank + 1
SIG_HD inline uint64_t signature_cap_rank(uint64_t r2, uint64_t R) { return r2 <= 2 * R ? r2 : 2 * R + 2; }
// the doubled capped midrank of the zero block [P, P + Z)
SIG_HD inline uint64_t signature_zero_rank(uint64_t P, uint64_t Z, uint64_t R) { return signature_cap_rank(2 * P + Z + 1, R); }
// the score of a set of n_s genes whose doubled capped midranks sum to rank2: one division and one subtraction
SIG_HD inline double signature_score(uint64_t rank2, uint64_t n_s, uint64_t R) {
    return 1.0 - (double)(rank2 - n_s * (n_s + 1)) / (2.0 * (double)n_s * (double)R);
}
