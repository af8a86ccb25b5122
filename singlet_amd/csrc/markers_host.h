// Host logic of sgl_markers (include/singlet_hip.h, "Marker genes") that makes no HIP call: the argument rules and the naming
// of a defective label, the cluster sizes, the split of the genes into the two rank paths, the batches of the long path and
// the derived statistics of every (gene, cluster) from the integer results of the device.  Plain C++ over plain pointers, so
// tests/markers_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ingest_host.h"

#define MARKERS_MAX_GROUPS 1024
#define MARKERS_MAX_CELLS ((int64_t)1 << 21)   // N^3 - N < 2^63: the tie term of a gene fits 64 bits
#define MARKERS_SEG 8192                       // entries per segment of the group sums: part of the stated summation order
#define MARKERS_LDS_CAP 2048                   // included non-zero entries of a gene that one workgroup sorts in LDS
#define MARKERS_WALK 1024                      // positions per chunk of the long path's walks
#define MARKERS_BATCH_ENTRIES ((int64_t)1 << 27)   // default entries per batch of the long path: 24 bytes of scratch each, 3 GiB

enum MarkersArgError {
    MARKERS_ARGS_OK = 0,
    MARKERS_ARGS_NULL,         // labels == NULL
    MARKERS_ARGS_GROUPS,       // n_groups outside [1, 1024]
    MARKERS_ARGS_TRANSFORM,    // transform outside {0, 1}
    MARKERS_ARGS_PSEUDOCOUNT,  // pseudocount negative or not finite
    MARKERS_ARGS_CELLS,        // ncol outside [0, 2^21]
    MARKERS_ARGS_LABEL,        // labels[*pos] = *val is outside [-1, n_groups)
};

// The refusals that need no device, in this order; the whole list is read before anything is launched.
inline MarkersArgError markers_check_args(const int32_t* labels, int64_t ncol, int32_t n_groups, int transform, double pseudocount,
                                          int64_t* pos, int32_t* val) {
    *pos = -1;
    *val = 0;
    if (!labels) return MARKERS_ARGS_NULL;
    if (n_groups < 1 || n_groups > MARKERS_MAX_GROUPS) return MARKERS_ARGS_GROUPS;
    if (transform != 0 && transform != 1) return MARKERS_ARGS_TRANSFORM;
    if (!(pseudocount >= 0.0) || !(pseudocount < INFINITY)) return MARKERS_ARGS_PSEUDOCOUNT;
    if (ncol < 0 || ncol > MARKERS_MAX_CELLS) return MARKERS_ARGS_CELLS;
    for (int64_t j = 0; j < ncol; ++j)
        if (labels[j] < -1 || labels[j] >= n_groups) { *pos = j; *val = labels[j]; return MARKERS_ARGS_LABEL; }
    return MARKERS_ARGS_OK;
}

// group_n[c] = the cells labelled c (n_groups values); returns N, the cells labelled 0 or above.  Labels checked before.
inline int64_t markers_group_counts(const int32_t* labels, int64_t ncol, int32_t n_groups, int64_t* group_n) {
    int64_t N = 0;
    for (int32_t c = 0; c < n_groups; ++c) group_n[c] = 0;
    for (int64_t j = 0; j < ncol; ++j)
        if (labels[j] >= 0) { ++group_n[labels[j]]; ++N; }
    return N;
}

// The two rank paths: gene g with count[g] included non-zero entries sorts in LDS when count[g] <= cap, else it is long.
// short_list / long_list (room for m each) receive the genes in ascending order, long_len the counts of the long ones.
inline void markers_split_paths(const int64_t* count, int32_t m, int64_t cap, int32_t* short_list, int64_t* n_short,
                                int32_t* long_list, int64_t* long_len, int64_t* n_long) {
    int64_t ns = 0, nl = 0;
    for (int32_t g = 0; g < m; ++g) {
        if (count[g] <= cap) short_list[ns++] = g;
        else { long_list[nl] = g; long_len[nl] = count[g]; ++nl; }
    }
    *n_short = ns;
    *n_long = nl;
}

// Batches of the long path: whole genes in list order, each batch at most `max_batch_entries` entries (<= 0: the default)
// and never more than INT32_MAX, which the segmented sort counts in; a gene above the cap is a batch of its own (it holds at
// most 2^21 entries).  cut has room for n + 1 values; returns the number of batches.
inline int64_t markers_batches(const int64_t* len, int64_t n, int64_t max_batch_entries, int64_t* cut) {
    int64_t cap = max_batch_entries > 0 ? max_batch_entries : MARKERS_BATCH_ENTRIES;
    if (cap > (int64_t)INT32_MAX) cap = (int64_t)INT32_MAX;
    return ingest_batch_edges(len, n, cap, cut);
}

// The derived statistics of gene g and cluster c, g < m, c < G, from the m x G column-major (gene fastest) integer results
// and group sums; any output may be NULL.  The rules are those of include/singlet_hip.h, operation by operation.
inline void markers_derive(int32_t m, int32_t G, const int64_t* group_n, const int64_t* pos, const double* sum, const int64_t* rank2,
                           const uint64_t* tie, double pseudocount, double* pct_in, double* pct_out, double* log2fc, double* z,
                           double* p) {
    int64_t N = 0;
    for (int32_t c = 0; c < G; ++c) N += group_n[c];
    const double dN = (double)N;
    for (int32_t g = 0; g < m; ++g) {
        int64_t pos_all = 0;
        if (pos)
            for (int32_t c = 0; c < G; ++c) pos_all += pos[(size_t)g + (size_t)m * c];
        for (int32_t c = 0; c < G; ++c) {
            const size_t at = (size_t)g + (size_t)m * c;
            const int64_t n1 = group_n[c], n2 = N - n1;
            const double d1 = (double)n1, d2 = (double)n2;
            if (pos) {
                if (pct_in) pct_in[at] = (double)pos[at] / d1;
                if (pct_out) pct_out[at] = (double)(pos_all - pos[at]) / d2;
            }
            if (sum && log2fc) {
                double s_out = 0.0;
                for (int32_t o = 0; o < G; ++o)
                    if (o != c) s_out += sum[(size_t)g + (size_t)m * o];
                const double mean_in = sum[at] / d1, mean_out = s_out / d2;
                log2fc[at] = log2(mean_in + pseudocount) - log2(mean_out + pseudocount);
            }
            if (rank2 && tie && (z || p)) {
                const int64_t U2 = rank2[at] - n1 * (n1 + 1);
                const int64_t D = U2 - n1 * n2;
                const double var = (d1 * d2 / 12.0) * ((dN + 1.0) - (double)tie[g] / (dN * (dN - 1.0)));
                double zv = NAN, pv = NAN;
                if (n1 != 0 && n2 != 0 && var > 0.0) {
                    const double absD = (double)(D < 0 ? -D : D);
                    double a = absD / 2.0 - 0.5;
                    if (a < 0.0) a = 0.0;
                    const double zz = a / sqrt(var);
                    zv = D < 0 ? -zz : zz;
                    pv = erfc(zz * M_SQRT1_2);
                }
                if (z) z[at] = zv;
                if (p) p[at] = pv;
            }
        }
    }
}
