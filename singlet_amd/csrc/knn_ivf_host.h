// Host logic of the inverted-list neighbour search (include/singlet_hip.h, "Approximate embedding neighbours") that makes no
// HIP call: the argument rules, the training picks and seeds, the check of a caller's assignment, the list offsets with the
// table from list position to cell, the task table of the list scan and the batch plan.  Plain C++ over plain pointers, so
// tests/knn_ivf_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <stdint.h>

#include "knn_host.h"

#define KNN_IVF_MAX_LISTS 65536
#define KNN_IVF_MAX_PROBES KNN_MAX_SEGMENTS   // the width of the merge pass
#define KNN_IVF_MAX_ITER 1000
#define KNN_IVF_TRAIN_PER_LIST 64             // training cells per list: T = min(n_ref, 64 n_lists)
#define KNN_IVF_SCRATCH_BYTES (1ll << 30)     // the candidate scratch of one batch of queries stays below this
// What Context.knn(method="ivf", n_probe=None) asks for (clamped to n_lists): the smallest power of two whose mean recall@20 is
// at least 0.99 on both data sets of profiles/knn_ivf_rate.json (scripts/knn_ivf_rate.py) at the default n_lists =
// ceil(sqrt(cells)).  pbmc3k, rank 15, 52 lists: 0.9674 at 4 probes, 0.9973 at 8.  The clustered synthetic: 0.9363 at 4 and
// 0.9949 at 8 in its worst case, "self50-1000000" (1000 lists); 0.9765 and 0.9996 in "self50-200000" (448 lists).
#define KNN_IVF_DEFAULT_PROBES 8

enum KnnIvfArgError {
    KNN_IVF_ARGS_OK = 0,
    KNN_IVF_ARGS_LISTS,    // n_lists outside [1, min(n_ref, 65536)]
    KNN_IVF_ARGS_PROBES,   // n_probe outside [1, min(n_lists, 64)]
    KNN_IVF_ARGS_ITER,     // n_iter outside [0, 1000]
    KNN_IVF_ARGS_METRIC,   // metric outside [0, 2]
};

inline int64_t knn_ivf_max_lists(int64_t n_ref) { return n_ref < KNN_IVF_MAX_LISTS ? n_ref : KNN_IVF_MAX_LISTS; }
inline int32_t knn_ivf_max_probes(int32_t n_lists) { return n_lists < KNN_IVF_MAX_PROBES ? n_lists : KNN_IVF_MAX_PROBES; }

// The refusals the inverted-list entries add, in this order, after knn_check_args has passed (n_ref >= 1).
inline KnnIvfArgError knn_ivf_check_args(int64_t n_ref, int32_t n_lists, int32_t n_probe, int32_t n_iter, int32_t metric) {
    if (n_lists < 1 || (int64_t)n_lists > knn_ivf_max_lists(n_ref)) return KNN_IVF_ARGS_LISTS;
    if (n_probe < 1 || n_probe > knn_ivf_max_probes(n_lists)) return KNN_IVF_ARGS_PROBES;
    if (n_iter < 0 || n_iter > KNN_IVF_MAX_ITER) return KNN_IVF_ARGS_ITER;
    if (!knn_metric_ok(metric)) return KNN_IVF_ARGS_METRIC;
    return KNN_IVF_ARGS_OK;
}

// Training cells: T of them; training cell t is reference floor(t n_ref / T); centroid g starts as training cell
// floor(g T / n_lists).  t < 2^22 and n_ref < 2^31: the products stay below 2^53.
inline int64_t knn_ivf_train_count(int64_t n_ref, int32_t n_lists) {
    const int64_t cap = (int64_t)KNN_IVF_TRAIN_PER_LIST * n_lists;
    return n_ref < cap ? n_ref : cap;
}
inline int64_t knn_ivf_pick(int64_t t, int64_t n_from, int64_t n_take) { return t * n_from / n_take; }

// The first entry of assign outside [0, n_lists): its position, or -1.
inline int64_t knn_ivf_first_bad_assign(const int32_t* assign, int64_t n_ref, int32_t n_lists) {
    for (int64_t r = 0; r < n_ref; ++r)
        if (assign[r] < 0 || assign[r] >= n_lists) return r;
    return -1;
}

// Lists: off[g] .. off[g + 1] are the positions of list g (off: n_lists + 1), cell[pos] the reference at a position; a list
// holds its members in ascending cell index (a stable counting sort).  assign has passed knn_ivf_first_bad_assign.
inline void knn_ivf_bucket(const int32_t* assign, int64_t n_ref, int32_t n_lists, int64_t* off, int32_t* cell) {
    for (int32_t g = 0; g <= n_lists; ++g) off[g] = 0;
    for (int64_t r = 0; r < n_ref; ++r) ++off[assign[r] + 1];
    for (int32_t g = 0; g < n_lists; ++g) off[g + 1] += off[g];
    // off[g] serves as list g's cursor and ends as off[g + 1]; one shift puts the offsets back
    for (int64_t r = 0; r < n_ref; ++r) cell[off[assign[r]]++] = (int32_t)r;
    for (int32_t g = n_lists; g > 0; --g) off[g] = off[g - 1];
    off[0] = 0;
}

inline void knn_ivf_list_stats(const int64_t* off, int32_t n_lists, int64_t* shortest, int64_t* longest, int64_t* empty) {
    *shortest = off[1] - off[0];
    *longest = *shortest;
    *empty = 0;
    for (int32_t g = 0; g < n_lists; ++g) {
        const int64_t len = off[g + 1] - off[g];
        if (len < *shortest) *shortest = len;
        if (len > *longest) *longest = len;
        if (len == 0) ++*empty;
    }
}

// The list scan: one wave per block of (query, probe slot) pairs that share a list; a lane owns queries_per_lane pairs, with
// knn_plan's rule (two up to n_dims = 32, one above).
inline int knn_ivf_pairs_per_block(int n_dims) { return 64 * (knn_instance(n_dims) <= 2 ? 2 : 1); }

// Task table, first pass.  probes: n_query x n_probe, probes[j * n_probe + p] the list of query j's probe slot p.  Writes
// first[g] .. first[g + 1], the places of list g's pairs in the sorted pair array (first: n_lists + 1), and returns the number
// of blocks: every list's pairs are cut into blocks of at most pairs_per_block, so no block crosses a list edge.
inline int64_t knn_ivf_task_count(const int32_t* probes, int64_t n_query, int32_t n_probe, int32_t n_lists, int pairs_per_block,
                                  int64_t* first) {
    for (int32_t g = 0; g <= n_lists; ++g) first[g] = 0;
    const int64_t n_pairs = n_query * n_probe;
    for (int64_t e = 0; e < n_pairs; ++e) ++first[probes[e] + 1];
    int64_t blocks = 0;
    for (int32_t g = 0; g < n_lists; ++g) {
        blocks += (first[g + 1] + pairs_per_block - 1) / pairs_per_block;
        first[g + 1] += first[g];
    }
    return blocks;
}

// Second pass.  The pairs sorted stably by list -- in (query, probe slot) order inside a list --: pair_query / pair_slot
// (n_query n_probe each); block b is the pairs block_begin[b] .. block_begin[b + 1] of list block_list[b] (block_begin: blocks
// + 1, block_list: blocks).  cursor: n_lists words of scratch.  A list nobody probes has no block; a probed list without members has blocks
// like any other, and their pairs receive padding only.
inline void knn_ivf_task_fill(const int32_t* probes, int64_t n_query, int32_t n_probe, int32_t n_lists, int pairs_per_block,
                              const int64_t* first, int64_t* cursor, int32_t* pair_query, int32_t* pair_slot, int32_t* block_list,
                              int64_t* block_begin) {
    for (int32_t g = 0; g < n_lists; ++g) cursor[g] = first[g];
    for (int64_t j = 0; j < n_query; ++j)
        for (int32_t p = 0; p < n_probe; ++p) {
            const int64_t at = cursor[probes[j * n_probe + p]]++;
            pair_query[at] = (int32_t)j;
            pair_slot[at] = p;
        }
    int64_t b = 0;
    for (int32_t g = 0; g < n_lists; ++g)
        for (int64_t at = first[g]; at < first[g + 1]; at += pairs_per_block) {
            block_list[b] = g;
            block_begin[b++] = at;
        }
    block_begin[b] = n_query * n_probe;
}

// Queries per pass: a forced query_batch as it is (at most n_query); 0: as many as keep the n_probe x n_neighbors x 12 bytes
// of candidates per query below `budget`, at least one.  n_query >= 1.
inline int64_t knn_ivf_batch(int64_t n_query, int32_t n_probe, int32_t n_neighbors, int64_t query_batch, int64_t budget) {
    int64_t b = query_batch;
    if (b <= 0) {
        b = budget / ((int64_t)n_probe * n_neighbors * 12);
        if (b < 1) b = 1;
    }
    return b < n_query ? b : n_query;
}
