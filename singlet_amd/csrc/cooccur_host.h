// Host logic of the co-occurrence calls (include/singlet_hip.h, "Co-occurrence by distance") that makes no HIP call: the argument
// rules and the naming of the offender, the squared thresholds, the bucket grid and the bin plan as pure functions of the sizes
// and the knobs, the flush bound's arithmetic, and both statistics from the integer table.  Plain C++ over plain pointers, so
// tests/cooccur_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it on the CPU.  The one function the
// device shares (cooccur_must_flush) is marked for both sides when hipcc compiles this header.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define COOCCUR_HD __host__ __device__
#else
#define COOCCUR_HD
#endif

#define COOCCUR_MAX_K 256                           // a label is one byte's worth, as in the neighbourhood enrichment
#define COOCCUR_MAX_T 64                            // intervals: at most 65 thresholds
#define COOCCUR_TILE 256                            // sorted positions per centre tile and per staged candidate tile
#define COOCCUR_LDS_BYTES ((int64_t)128 << 10)      // bins + staging of a workgroup: 128 KiB of the CU's 160 KiB (kernels_nhood.hip's budget)
#define COOCCUR_STAGE_BYTES ((int64_t)6144)         // x, y, label of a candidate tile, the squared thresholds: the front of the workgroup's LDS
#define COOCCUR_MAX_WG 1024                         // workgroups over the centre tiles (above, a workgroup takes more tiles)
#define COOCCUR_WG_TARGET 2048                      // all-pairs regime: workgroups wanted; the candidate tiles of a centre tile are dealt to `split` workgroups
#define COOCCUR_MAX_SPLIT 64
#define COOCCUR_EXTENT_BLOCKS 64                    // workgroups of the extent reduction (a stride loop walks the rest)
#define COOCCUR_FLUSH_PAIRS (((int64_t)1 << 32) - 1)   // pairs a workgroup may evaluate between two flushes: what a uint32 bin holds
#define COOCCUR_REACH_FLOOR 0x1p-510                // below it dx * dx may underflow: the buckets are never smaller (see cooccur_grid)
#define COOCCUR_PI 0x1.921fb54442d18p+1

enum CooccurArgError {
    COOCCUR_ARGS_OK = 0,
    COOCCUR_ARGS_NULL,     // c1, c2, lab or r == NULL
    COOCCUR_ARGS_N,        // n < 1
    COOCCUR_ARGS_COORD,    // c1 (*val == 1) or c2 (*val == 2) at *at is not finite
    COOCCUR_ARGS_K,        // K outside [1, 256]
    COOCCUR_ARGS_LABEL,    // lab[*at] = *val is outside [0, K)
    COOCCUR_ARGS_T,        // T outside [1, 64]
    COOCCUR_ARGS_R,        // r[0] < 0 (*at == 0) or r[*at] is not finite
    COOCCUR_ARGS_THR2,     // fl(r[*at]^2) is not finite, or not above fl(r[*at - 1]^2)
    COOCCUR_ARGS_KNOB,     // knob *at (0 grid_mode, 1 bin_path, 2 flush_pairs) = *val is negative or out of range
};

// every refusal of a call, in the stated order; thr2 (T + 1 doubles, may be NULL) receives fl(r[t] * r[t]) on success
inline CooccurArgError cooccur_check_call(const double* c1, const double* c2, int64_t n, const int32_t* lab, int64_t K, const double* r, int64_t T,
                                          double* thr2, int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (!c1 || !c2 || !lab || !r) return COOCCUR_ARGS_NULL;
    if (n < 1) return COOCCUR_ARGS_N;
    for (int64_t e = 0; e < n; ++e) {
        if (!isfinite(c1[e])) { *at = e; *val = 1; return COOCCUR_ARGS_COORD; }
        if (!isfinite(c2[e])) { *at = e; *val = 2; return COOCCUR_ARGS_COORD; }
    }
    if (K < 1 || K > COOCCUR_MAX_K) return COOCCUR_ARGS_K;
    for (int64_t e = 0; e < n; ++e)
        if (lab[e] < 0 || lab[e] >= K) { *at = e; *val = lab[e]; return COOCCUR_ARGS_LABEL; }
    if (T < 1 || T > COOCCUR_MAX_T) return COOCCUR_ARGS_T;
    if (!(r[0] >= 0.0)) { *at = 0; return COOCCUR_ARGS_R; }   // (a NaN is refused here too)
    for (int64_t t = 0; t <= T; ++t)
        if (!isfinite(r[t])) { *at = t; return COOCCUR_ARGS_R; }
    double prev = 0.0;
    for (int64_t t = 0; t <= T; ++t) {
        const volatile double sq = r[t] * r[t];   // one rounding, never fused with the comparison's subtraction
        if (!isfinite(sq) || (t > 0 && !(sq > prev))) { *at = t; return COOCCUR_ARGS_THR2; }
        if (thr2) thr2[t] = sq;
        prev = sq;
    }
    return COOCCUR_ARGS_OK;
}

inline CooccurArgError cooccur_check_knobs(int64_t grid_mode, int64_t bin_path, int64_t flush_pairs, int64_t* at, int64_t* val) {
    if (grid_mode < 0 || grid_mode > 2) { *at = 0; *val = grid_mode; return COOCCUR_ARGS_KNOB; }
    if (bin_path < 0 || bin_path > 2) { *at = 1; *val = bin_path; return COOCCUR_ARGS_KNOB; }
    if (flush_pairs < 0 || flush_pairs > COOCCUR_FLUSH_PAIRS) { *at = 2; *val = flush_pairs; return COOCCUR_ARGS_KNOB; }
    return COOCCUR_ARGS_OK;
}

// ---- the bucket grid ----------------------------------------------------------------------------------------------------------------
// Points are keyed by their bucket by * W + bx of a W x H grid of square buckets, b = floor((c - cmin) / side) in double, and
// sorted by key with a stable sort.  Every pair that passes the test lies in adjacent buckets.
//
// Why, for the squared test d2 = fl(fl(dx*dx) + fl(dy*dy)) <= thr2[T] = fl(R*R), dx = fl(x1 - x2), in double (p = 53, smallest
// normal 2^-1022), uncontracted.  If |dx| < 2^-511 then |x1 - x2| < 2^-510 (a difference that rounds below 2^-511 is below it too,
// or subnormal and exact).  Otherwise dx*dx >= 2^-1022 is normal and fl(dx*dx) >= dx^2 (1 - 2^-53); adding the non-negative
// fl(dy*dy) is monotone, so fl(dx*dx) <= d2 <= fl(R*R), which is then normal too and at most R^2 (1 + 2^-53).  Hence dx^2 <=
// R^2 (1 + 2^-51), |dx| <= R (1 + 2^-51) and |x1 - x2| <= |dx| (1 + 2^-52) <= R (1 + 2^-50).  Either way |x1 - x2| <=
// max(R, 2^-510) (1 + 2^-50), and the same holds for y.  Buckets have side s >= max(R, 2^-510) (1 + 2^-10), so |x1 - x2| / s <
// 1 - 2^-11.  The bucket coordinate u = fl(fl(x - xmin) / s) is off by at most 2^-52 u + 2^-1074 <= 2^-21, since s is also raised
// so that u <= 2^30; so |u1 - u2| < 1 and floor(u1), floor(u2) differ by at most one.  No root is taken anywhere.
struct CooccurGrid {
    double xmin, ymin, side;
    int64_t W, H;
    int mode;   // 1 one bucket (all pairs), 2 the bucket grid
};

// grid_mode 0: the plan (one bucket when the grid would be at most 3 x 3 buckets), 1: one bucket, 2: the grid whatever its
// size.  An extent that overflows double is one bucket in every mode.
inline CooccurGrid cooccur_grid(double xmin, double xmax, double ymin, double ymax, double reach, int grid_mode) {
    CooccurGrid g{xmin, ymin, INFINITY, 1, 1, 1};
    const double ex = xmax - xmin, ey = ymax - ymin, ext = ex > ey ? ex : ey;
    if (grid_mode == 1 || !(ext < INFINITY)) return g;
    const double base = (reach > COOCCUR_REACH_FLOOR ? reach : COOCCUR_REACH_FLOOR) * (1.0 + 0x1p-10), cap = ext * 0x1p-30;
    const double side = base > cap ? base : cap;
    const int64_t W = (int64_t)floor(ex / side) + 2, H = (int64_t)floor(ey / side) + 2;
    if (grid_mode == 0 && W <= 3 && H <= 3) return g;
    g.side = side;
    g.W = W;
    g.H = H;
    g.mode = 2;
    return g;
}

// ---- the bin plan ---------------------------------------------------------------------------------------------------------------------
struct CooccurPlan {
    int path;              // 1 the LDS path, 2 the global path
    int64_t lds_bytes;     // dynamic LDS of a workgroup: the staging, plus the T x K x K uint32 bins on the LDS path
    int64_t tiles;         // centre tiles of 256 sorted positions
    int64_t tiles_per_wg;  // a workgroup's contiguous range of centre tiles
    int64_t wgs;           // workgroups over the centre tiles
    int64_t split;         // workgroups that share a range of centre tiles, each taking every split-th candidate tile
    int64_t flush_pairs;   // the bound in force
};

inline bool cooccur_lds_fits(int64_t K, int64_t T) { return T * K * K * 4 + COOCCUR_STAGE_BYTES <= COOCCUR_LDS_BYTES; }

// bin_path 0 the plan / 1 the LDS path (bins that do not fit still go global) / 2 the global path; flush_pairs 0: the plan's
// bound, 2^32 - 1.  grid_run: what cooccur_grid chose; only the all-pairs regime splits the candidates.
inline void cooccur_plan(int64_t n, int64_t K, int64_t T, int grid_run, int bin_path, int64_t flush_pairs, CooccurPlan* P) {
    P->path = (bin_path == 2 || !cooccur_lds_fits(K, T)) ? 2 : 1;
    P->lds_bytes = COOCCUR_STAGE_BYTES + (P->path == 1 ? T * K * K * 4 : 0);
    P->tiles = (n + COOCCUR_TILE - 1) / COOCCUR_TILE;
    P->tiles_per_wg = (P->tiles + COOCCUR_MAX_WG - 1) / COOCCUR_MAX_WG;
    P->wgs = (P->tiles + P->tiles_per_wg - 1) / P->tiles_per_wg;
    int64_t s = 1;
    if (grid_run == 1) {
        s = (COOCCUR_WG_TARGET + P->wgs - 1) / P->wgs;
        if (s > COOCCUR_MAX_SPLIT) s = COOCCUR_MAX_SPLIT;
        if (s > P->tiles) s = P->tiles;
    }
    P->split = s;
    P->flush_pairs = flush_pairs > 0 ? flush_pairs : COOCCUR_FLUSH_PAIRS;
}

// The flush rule.  A bin is a uint32 and one evaluated pair adds at most 1 to one bin, so the bins hold what a workgroup tallies
// as long as the pairs evaluated since its last flush stay at or below bound <= 2^32 - 1.  Before a stage of `add` pairs (at most
// 256 x 256) the workgroup flushes when since + add would pass the bound -- written without the sum, which need not fit.  With
// since == 0 there is nothing to flush: a bound below one stage flushes before every stage, and one stage alone never overflows.
COOCCUR_HD inline bool cooccur_must_flush(int64_t since, int64_t add, int64_t bound) {
    return since > 0 && (add > bound || since > bound - add);
}

// ---- the statistics ---------------------------------------------------------------------------------------------------------------------
// A table that can be a tally: no negative count, symmetric in (a, b), an even diagonal, a total that fits int64.  *at: the offender.
inline bool cooccur_table_ok(int64_t K, int64_t T, const int64_t* counts, int64_t* at) {
    const int64_t KK = K * K;
    unsigned __int128 total = 0;
    for (int64_t t = 0; t < T; ++t)
        for (int64_t b = 0; b < K; ++b)
            for (int64_t a = 0; a < K; ++a) {
                const int64_t q = a + K * b + KK * t, v = counts[q];
                if (v < 0 || v != counts[b + K * a + KK * t] || (a == b && (v & 1))) { *at = q; return false; }
                total += (unsigned __int128)v;
                if (total > (unsigned __int128)INT64_MAX) { *at = q; return false; }
            }
    *at = -1;
    return true;
}

// ratio[a + K b + K^2 t] = ((double)N / (double)row[a]) / ((double)row[b] / (double)tot) per interval, or of the running sums
// with `cumulative`; NaN when row[a] == 0 or row[b] == 0.  scratch: K^2 + K int64 of the caller.
inline void cooccur_stats(int64_t K, int64_t T, const int64_t* counts, bool cumulative, double* ratio, int64_t* scratch) {
    const int64_t KK = K * K;
    int64_t* cur = scratch;
    int64_t* row = scratch + KK;
    for (int64_t q = 0; q < KK; ++q) cur[q] = 0;
    for (int64_t t = 0; t < T; ++t) {
        for (int64_t q = 0; q < KK; ++q) cur[q] = (cumulative ? cur[q] : 0) + counts[q + KK * t];
        int64_t tot = 0;
        for (int64_t a = 0; a < K; ++a) row[a] = 0;
        for (int64_t b = 0; b < K; ++b)
            for (int64_t a = 0; a < K; ++a) {
                row[a] += cur[a + K * b];
                tot += cur[a + K * b];
            }
        for (int64_t b = 0; b < K; ++b)
            for (int64_t a = 0; a < K; ++a) {
                double v = NAN;
                if (row[a] != 0 && row[b] != 0) {
                    const double cond = (double)cur[a + K * b] / (double)row[a];
                    const double marg = (double)row[b] / (double)tot;
                    v = cond / marg;
                }
                ratio[a + K * b + KK * t] = v;
            }
    }
}

// Ripley's K and L from the cumulative diagonal: Kfun[a + K t] = (area * (double)Ncum[a, a, t]) / (double)(n_a (n_a - 1)),
// L = sqrt(Kfun / pi); NaN for n_a < 2.  Either output may be NULL.
inline void cooccur_ripley(int64_t K, int64_t T, const int64_t* counts, const int64_t* group_n, double area, double* K_out, double* L_out) {
    const int64_t KK = K * K;
    for (int64_t a = 0; a < K; ++a) {
        int64_t cum = 0;
        for (int64_t t = 0; t < T; ++t) {
            cum += counts[a + K * a + KK * t];
            double kf = NAN;
            if (group_n[a] >= 2) {
                const double num = area * (double)cum;
                kf = num / (double)(group_n[a] * (group_n[a] - 1));
            }
            if (K_out) K_out[a + K * t] = kf;
            if (L_out) L_out[a + K * t] = sqrt(kf / COOCCUR_PI);
        }
    }
}

// what sgl_ripley_stats refuses beyond cooccur_table_ok: 0 fine, 1 area, 2 group_n[*at] negative or above 2^31, 3 the diagonal of
// class *at counts more ordered pairs than n_a (n_a - 1)
inline int cooccur_ripley_check(int64_t K, int64_t T, const int64_t* counts, const int64_t* group_n, double area, int64_t* at) {
    *at = -1;
    if (!(area > 0.0) || !isfinite(area)) return 1;
    for (int64_t a = 0; a < K; ++a) {
        if (group_n[a] < 0 || group_n[a] > ((int64_t)1 << 31)) { *at = a; return 2; }
        unsigned __int128 cum = 0;
        for (int64_t t = 0; t < T; ++t) cum += (unsigned __int128)counts[a + K * a + K * K * t];
        const unsigned __int128 cap = group_n[a] >= 1 ? (unsigned __int128)group_n[a] * (unsigned __int128)(group_n[a] - 1) : 0;
        if (cum > cap) { *at = a; return 3; }
    }
    return 0;
}
