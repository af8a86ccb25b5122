// Host logic of sgl_c_louvain (include/singlet_hip.h, "Clustering") that makes no HIP call: the argument rules, the check of
// the column pointers, the naming of a defective entry, the guard and the sweep bookkeeping of a level's moving phase, the
// split of a level's vertices into the two sweep paths, and the final renumbering of the clusters by size.  Plain C++ over
// plain pointers, so tests/cluster_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define LOUVAIN_MAX_LEVELS 32
#define LOUVAIN_MAX_SWEEPS 1024
#define LOUVAIN_FAST_DEGREE 512   // stored entries of a column that one wave sorts in LDS (4 KiB of keys: LDS does not cap the 32 waves of a CU)
#define LOUVAIN_SUM_BLOCK 1024    // the sums over members, communities and coarse entries run sequentially inside blocks of this many terms

enum LouvainArgError {
    LOUVAIN_ARGS_OK = 0,
    LOUVAIN_ARGS_N,            // n < 0
    LOUVAIN_ARGS_NULL,         // p == NULL, or entries without i / x
    LOUVAIN_ARGS_P0,           // p[0] != 0
    LOUVAIN_ARGS_P_DECREASES,  // p[*pos + 1] < p[*pos]
    LOUVAIN_ARGS_NRES,         // n_res < 1 or resolutions == NULL
    LOUVAIN_ARGS_RESOLUTION,   // resolutions[*pos] not finite or <= 0
    LOUVAIN_ARGS_TOL,          // tol < 0 or NaN
    LOUVAIN_ARGS_SWEEPS,       // max_sweeps outside [1, 1024]
    LOUVAIN_ARGS_LEVELS,       // max_levels outside [1, 32]
};

// The refusals that need no device, in this order; *pos names the offending column or resolution.
inline LouvainArgError louvain_check_args(int64_t n, const int32_t* p, const int32_t* i, const double* x, int32_t n_res,
                                          const double* resolutions, double tol, int32_t max_sweeps, int32_t max_levels, int64_t* pos) {
    *pos = -1;
    if (n < 0) return LOUVAIN_ARGS_N;
    if (n_res < 1 || !resolutions) return LOUVAIN_ARGS_NRES;
    for (int32_t r = 0; r < n_res; ++r)
        if (!(resolutions[r] > 0.0) || !(resolutions[r] < INFINITY)) { *pos = r; return LOUVAIN_ARGS_RESOLUTION; }
    if (!(tol >= 0.0)) return LOUVAIN_ARGS_TOL;
    if (max_sweeps < 1 || max_sweeps > LOUVAIN_MAX_SWEEPS) return LOUVAIN_ARGS_SWEEPS;
    if (max_levels < 1 || max_levels > LOUVAIN_MAX_LEVELS) return LOUVAIN_ARGS_LEVELS;
    if (n == 0) return LOUVAIN_ARGS_OK;   // nothing is read
    if (!p) return LOUVAIN_ARGS_NULL;
    if (p[0] != 0) return LOUVAIN_ARGS_P0;
    for (int64_t c = 0; c < n; ++c)
        if (p[c + 1] < p[c]) { *pos = c; return LOUVAIN_ARGS_P_DECREASES; }
    if (p[n] > 0 && (!i || !x)) return LOUVAIN_ARGS_NULL;
    return LOUVAIN_ARGS_OK;
}

// The column that holds entry e: the last c with p[c] <= e (empty columns before it are skipped).  0 <= e < p[n].
inline int64_t louvain_column_of(const int32_t* p, int64_t n, int64_t e) {
    int64_t lo = 0, hi = n;   // invariant: p[lo] <= e < p[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)p[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

enum LouvainDefect {
    LOUVAIN_ENTRY_OK = 0,
    LOUVAIN_ROW_RANGE,
    LOUVAIN_ROW_ORDER,      // not above the row before it in its column
    LOUVAIN_NOT_FINITE,
    LOUVAIN_NEGATIVE,
    LOUVAIN_ASYMMETRIC,     // A_rc missing, or its bits differ
};

// What is wrong with the entry e of column c (the device pass found e; this names the defect for the message), in the
// order of the enum.  with_symmetry: look A_cr up in column r by bisection (the columns are sorted when this is asked).
inline LouvainDefect louvain_entry_defect(const int32_t* p, const int32_t* i, const double* x, int64_t n, int64_t c, int64_t e,
                                          bool with_symmetry) {
    const int64_t r = i[e];
    if (r < 0 || r >= n) return LOUVAIN_ROW_RANGE;
    if (e > p[c] && i[e - 1] >= r) return LOUVAIN_ROW_ORDER;
    if (!(x[e] - x[e] == 0.0)) return LOUVAIN_NOT_FINITE;
    if (x[e] < 0.0) return LOUVAIN_NEGATIVE;
    if (!with_symmetry || r == c) return LOUVAIN_ENTRY_OK;
    int64_t lo = p[r], hi = p[r + 1];
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (i[mid] < c) lo = mid + 1; else hi = mid;
    }
    if (lo >= p[r + 1] || i[lo] != c) return LOUVAIN_ASYMMETRIC;
    return memcmp(&x[lo], &x[e], sizeof(double)) == 0 ? LOUVAIN_ENTRY_OK : LOUVAIN_ASYMMETRIC;
}

// ---- the moving phase of one level.  The guard: after a sweep Q' is computed from the new labels; Q' <= Q (or a sweep
// that moved nothing, whose Q' is Q): the sweep is discarded and the phase ends; Q' - Q <= tol: kept, and the phase ends;
// otherwise kept, and the phase goes on up to max_sweeps sweeps.
enum LouvainVerdict { LOUVAIN_DISCARD_END = 0, LOUVAIN_KEEP_END, LOUVAIN_KEEP_GO };

struct LouvainPhase {
    double q, tol;
    int32_t tried, kept, max_sweeps;
    bool over;
};

inline LouvainPhase louvain_phase_begin(double q_start, double tol, int32_t max_sweeps) {
    LouvainPhase P;
    P.q = q_start;
    P.tol = tol;
    P.tried = 0;
    P.kept = 0;
    P.max_sweeps = max_sweeps;
    P.over = false;
    return P;
}
inline bool louvain_phase_wants_sweep(const LouvainPhase& P) { return !P.over && P.tried < P.max_sweeps; }
// A sweep that moved nothing needs no Q' (q_new is not read).
inline LouvainVerdict louvain_phase_after_sweep(LouvainPhase& P, int64_t moved, double q_new) {
    ++P.tried;
    if (moved <= 0 || !(q_new > P.q)) { P.over = true; return LOUVAIN_DISCARD_END; }
    const double gain = q_new - P.q;
    P.q = q_new;
    ++P.kept;
    if (gain <= P.tol) { P.over = true; return LOUVAIN_KEEP_END; }
    return LOUVAIN_KEEP_GO;
}

// ---- the two sweep paths of a level: columns of up to LOUVAIN_FAST_DEGREE stored entries (the empty ones too) go to the
// wave-per-vertex kernel, the longer ones to the segmented global sort; soff = the offsets of the slow columns' keys.
template <typename P_>
inline void louvain_split(const P_* p, int64_t n, std::vector<int32_t>& fast, std::vector<int32_t>& slow, std::vector<int64_t>& soff) {
    fast.clear();
    slow.clear();
    soff.assign(1, 0);
    for (int64_t v = 0; v < n; ++v) {
        const int64_t len = (int64_t)p[v + 1] - (int64_t)p[v];
        if (len <= LOUVAIN_FAST_DEGREE) {
            fast.push_back((int32_t)v);
        } else {
            slow.push_back((int32_t)v);
            soff.push_back(soff.back() + len);
        }
    }
}

// ---- the output labels: clusters numbered by descending size, ties by smallest member; 0 is the largest.  assign[v] in
// [0, n) is the cluster id the levels gave vertex v; labels may alias assign.  Returns the number of clusters.
inline int64_t louvain_renumber_by_size(const int32_t* assign, int64_t n, int32_t* labels) {
    std::vector<int64_t> count((size_t)n, 0), first((size_t)n, -1);
    for (int64_t v = 0; v < n; ++v) {
        const int32_t c = assign[v];
        if (count[(size_t)c]++ == 0) first[(size_t)c] = v;
    }
    std::vector<int32_t> ids;
    for (int64_t c = 0; c < n; ++c)
        if (count[(size_t)c] > 0) ids.push_back((int32_t)c);
    std::sort(ids.begin(), ids.end(), [&](int32_t a, int32_t b) {
        if (count[(size_t)a] != count[(size_t)b]) return count[(size_t)a] > count[(size_t)b];
        return first[(size_t)a] < first[(size_t)b];
    });
    std::vector<int32_t> rank((size_t)n, -1);
    for (size_t q = 0; q < ids.size(); ++q) rank[(size_t)ids[q]] = (int32_t)q;
    for (int64_t v = 0; v < n; ++v) labels[v] = rank[(size_t)assign[v]];
    return (int64_t)ids.size();
}
