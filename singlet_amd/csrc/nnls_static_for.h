// compile-time loops and device helpers shared by the NNLS kernels
#pragma once
#include "sgl_internal.h"
#include <utility>
#include <type_traits>

// compile-time loop: guarantees that b[] / x[] are only ever indexed by constants
// (so they live in VGPRs) regardless of the optimiser's unroll thresholds.
template <typename F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// host side: f(std::integral_constant<int, I>{}) for the run-time index i clamped into [LO, HI] -- the instance of a launcher that
// serves a rank, one per index of the range and no other.  Callers that have no instance for an index outside check it first.
template <int LO, int HI, typename F>
int sgl_rank_dispatch(int i, F&& f) {
    if constexpr (LO < HI) {
        if (i > LO) return sgl_rank_dispatch<LO + 1, HI>(i, f);
    }
    return f(std::integral_constant<int, LO>{});
}


// x / y, correctly rounded, for finite operands in the normal range (no over- / underflow on the way): the
// instruction sequence hipcc emits for an FP64 division (v_rcp_f64, two Newton steps, quotient, remainder,
// correction) WITHOUT its v_div_scale / v_div_fixup frame, which only acts on denormal or extreme-exponent
// operands and on inf / nan / zero divisors.  In the NNLS the divisors are x + 1e-15 >= 1e-15 and Gram
// diagonals >= 1e-15, the dividends finite steps: bit-identical to `x / y` there, 8 instructions instead of 11
// and no special-case control flow (hipcc had wrapped the division of the tol term in exec-mask branches).
__device__ __forceinline__ double sgl_div_normal(double x, double y) {
    double r = __builtin_amdgcn_rcp(y);
    double e = __builtin_fma(-y, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-y, r, 1.0);
    r = __builtin_fma(r, e, r);
    const double q = x * r;
    const double rem = __builtin_fma(-y, q, x);
    return __builtin_fma(rem, r, q);
}

// One coordinate step of nnls (src/singlet.cpp:233-247) without the row update, branch-free.  In: diff0 = b_i / a_ii
// (before the penalties), x_i >= 0, running tol, go (false: the column has stopped -- its step is forced to zero, which
// leaves x, b and tol as they are).  Out: x_i, tol updated; returns nd = -delta, the factor of the row update
// b += a[:, i] * nd.
//   clamp (-diff > x_i): x_i -> 0, delta = -x_i, tol = 1 unless x_i was 0 (then nothing changes);
//   otherwise            x_i += diff, delta = diff, tol += |diff / (x_i + 1e-15)|  (diff == 0 adds exact zeros).
// Both branches are ONE expression: nd = min(-diff, x_i) is x_i exactly when the reference clamps and -diff otherwise,
// x_i - nd is 0 / x_i + diff, and |nd / (x_i - nd + 1e-15)| is the tol term of the second branch and an exact 0 in the
// "clamped at zero already" case -- which leaves a single select, the tol = 1 of a coordinate that was clamped from a
// positive value.  22 VALU instructions per step where the select-per-quantity form needed 38 (5 selects of 2 v_cndmask,
// the negation); same values bit for bit (the sign of a zero step differs, which no later operation can see).
// The two halves of the step, for the kernels that test whether the coordinate moves at all before paying for the rest
// (four columns per wave: a coordinate at rest in all four skips sgl_nnls_apply and the row update -- with nd = 0,
// sgl_nnls_apply leaves x_i and tol as they are, bit for bit: x_i - 0, tol + |0 / (x_i + 1e-15)|, no reset).
__device__ __forceinline__ double sgl_nnls_nd(double diff0, double xi, bool go, double L1, double L2, double& diff) {
    diff = diff0 - L1;                             // exact no-op when L1 == 0
    diff = __builtin_fma(L2, xi, diff);            // exact no-op when L2 == 0 (x >= 0)
    diff *= go ? 1.0 : 0.0;                        // one multiply instead of two v_cndmask (finite operands)
    double nd;
    asm("v_min_f64 %0, -%1, %2" : "=v"(nd) : "v"(diff), "v"(xi));
    return nd;
}
__device__ __forceinline__ void sgl_nnls_apply(double diff, double nd, double& xi, double& tol) {
    const double xn = xi - nd;
    const double tadd = __builtin_fabs(sgl_div_normal(nd, xn + 1e-15));
    const bool reset = (-diff > xi) & (xi != 0.0);
    tol = reset ? 1.0 : tol + tadd;
    xi = xn;
}
// The same first half for the solves against PER-COLUMN Grams (predict_mask, src/singlet.cpp:458-463), where a diagonal entry
// a_ii - asub_ii can be exactly zero -- a factor whose row of the other factor matrix is all zero, or lies entirely inside
// the column's drawn rows -- and the reference's `b(i) / a(i, i)` is +-inf or NaN (l.233): non-finite steps must come out as
// the reference's do.  With nd = clamp ? x_i : -diff (instead of v_min_f64, which returns the OTHER operand for a NaN):
//   diff NaN   l.237 false, l.243 true: x_i += NaN, b -= a.col(i) * NaN, tol NaN     = nd NaN:  x_i - nd, b += a.col(i) * nd, tol + |nd / ..|
//   diff +inf  the same branch: x_i = inf, b -= a.col(i) * inf, tol += |inf / inf|   = nd -inf: the same expressions
//   diff -inf  l.237 true: the clamp of a finite step (x_i -> 0, tol = 1; nothing if x_i == 0)     = nd x_i
// and a stopped column is gated by a select (0 * inf would be NaN).  Finite steps: the same bits as sgl_nnls_nd.
__device__ __forceinline__ double sgl_nnls_nd_strict(double diff0, double xi, bool go, double L1, double L2, double& diff) {
    diff = diff0 - L1;
    diff = __builtin_fma(L2, xi, diff);
    diff = go ? diff : 0.0;
    return (-diff > xi) ? xi : -diff;
}
// b_i / g_ii, correctly rounded, from the correctly rounded reciprocal r_ii = RN(1 / g_ii) (Markstein): q = RN(b r),
// rem = b - q g_ii exactly (FMA), RN(q + rem r).  Three instructions where an IEEE division takes eleven; exact for a normal
// r_ii and finite operands (a shared Gram: its diagonal is the same for all columns and sweeps).
__device__ __forceinline__ double sgl_nnls_markstein(double bi, double gii, double rii) {
    const double q0 = bi * rii;
    return __builtin_fma(__builtin_fma(-q0, gii, bi), rii, q0);
}
// b_i / g_ii for a per-column Gram: sgl_nnls_markstein wherever r_ii is a normal number; elsewhere (g_ii zero, denormal, huge,
// non-finite) the IEEE division the reference performs.  `any_irregular` is wave-uniform and false for all but degenerate
// columns: one scalar branch per coordinate.
__device__ __forceinline__ double sgl_nnls_quotient(double bi, double gii, double rii, bool any_irregular) {
    double diff0 = sgl_nnls_markstein(bi, gii, rii);
    if (any_irregular) {
        const double q = bi / gii;
        diff0 = __builtin_isnormal(rii) ? diff0 : q;
    }
    return diff0;
}

__device__ __forceinline__ double sgl_nnls_step(double diff0, double& xi, double& tol, bool go, double L1, double L2) {
    double diff;
    const double nd = sgl_nnls_nd(diff0, xi, go, L1, L2, diff);
    sgl_nnls_apply(diff, nd, xi, tol);
    return nd;
}

// ---- bookkeeping of the solves -------------------------------------------------------------------------------------------------
// Sweep counts (sweep_counter, optional): [0] the sweeps of the columns, each booked once, when the column stops; [2] the sweeps
// the waves executed (a wave runs until its slowest column stops).  s: this lane's share of [0], ran: the wave's share of [2] (the
// same in every lane).  REDUCE = false: s is the same in every lane too (one wave per column), lane 0 books it alone.
template <bool REDUCE = true, typename T>
__device__ __forceinline__ void sgl_nnls_book_sweeps(unsigned long long* __restrict__ sweep_counter, T s, T ran) {
    if (sweep_counter == nullptr) return;
    if constexpr (REDUCE) {
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && (s != 0 || ran != 0)) {
        atomicAdd(sweep_counter, (unsigned long long)s);
        atomicAdd(sweep_counter + 2, (unsigned long long)ran);
    }
}

// the packing key of the next solve (kernels_nnls.hip, "packing by sweep count"): the sweeps a column needed, written when it stops
__device__ __forceinline__ void sgl_nnls_packing_key(uint8_t* prev_it, int64_t col, int it) {
    if (prev_it != nullptr) prev_it[col] = (uint8_t)it;
}

// Re-packing passes (NnlsPass, sgl_internal.h; the lane solves of a shared Gram: nnls_lane.h, nnls_half.h and their generated
// forms).  Lanes of a wave run in lock-step, so a wave is busy until its slowest column stops: at config 3 the columns need 31
// sweeps on average but a wave runs 46.  The solve is therefore done in PASSES: a pass takes its columns from the list the
// previous one wrote (all ncols of them, or the list of a packing order, in the first); a wave leaves the pass as soon as fewer
// than SGL_NNLS_REPACK_NUM / _DEN of the lanes it started with are still iterating (unless the pass runs to the end), and the
// unfinished columns save their state -- b in place in B, x, the sweep count and the running tol -- and append themselves to the
// list of the next pass, where they resume densely packed.  A column's own sequence of sweeps is unchanged (same order, same
// arithmetic, same stop test after every sweep), so results are bit-identical to a single pass whatever the packing; only the
// order in which columns land in the list varies from run to run.  A column that stops writes its packing key.
#ifndef SGL_NNLS_REPACK_NUM
#define SGL_NNLS_REPACK_NUM 3
#define SGL_NNLS_REPACK_DEN 8
#endif

// the number of columns in pass ps
__device__ __forceinline__ int64_t sgl_nnls_pass_size(const NnlsPass& ps, int64_t ncols) { return ps.list ? (int64_t)*ps.count : ncols; }

// the column at position pos of a pass of n_in columns
struct SglNnlsPassCol {
    int64_t col;    // (0 past the end of the pass)
    bool valid;     // in the pass, and resumed or not empty: empty columns are skipped and keep their stale values (src/singlet.cpp:340)
    bool resume;    // a later pass: the column's state was saved by the previous one
    bool to_end;    // the pass runs its columns to the end: the last pass, or one over a list too short to fill the GPU
};
__device__ __forceinline__ SglNnlsPassCol sgl_nnls_pass_entry(const NnlsPass& ps, int64_t n_in, int64_t pos, const int64_t* __restrict__ col_nnz) {
    SglNnlsPassCol pc;
    const bool in_range = pos < n_in;
    pc.col = in_range ? (ps.list ? (int64_t)ps.list[pos] : pos) : 0;
    pc.resume = ps.list != nullptr && !ps.fresh;
    pc.valid = in_range && (pc.resume || col_nnz == nullptr || col_nnz[pc.col] != 0);
    pc.to_end = (ps.next_list == nullptr) || n_in <= (int64_t)ps.final_below;
    return pc;
}
// the running tol and sweep count the column starts the pass with
__device__ __forceinline__ void sgl_nnls_pass_state(const NnlsPass& ps, const SglNnlsPassCol& pc, double& tol, int& it) {
    tol = 1.0;
    it = 0;
    if (pc.valid && pc.resume) {
        tol = ps.tol_state[pc.col];
        it = (int)ps.it_state[pc.col];
    }
}
// The end of the pass for a column (after the kernel has stored x): an unfinished column -- possible only when !to_end -- saves
// its state (save_b(): the lane's share of b, in place in B; tol and the sweep count) and is appended to the next pass's list
// (wave-aggregated: one atomic per wave), a stopped one writes its packing key and books its sweeps, the wave books the `ran`
// sweeps it executed.  LANES: the lanes that hold the columns (all 64, or the lower 32 where two lanes share a column);
// `speaks`: this lane speaks for its column (the lower lane of a pair).
template <unsigned long long LANES, typename SaveB>
__device__ __forceinline__ void sgl_nnls_pass_exit(const NnlsPass& ps, const SglNnlsPassCol& pc, bool unfinished, bool speaks, double tol, int it,
                                                   int ran, unsigned long long* __restrict__ sweep_counter, SaveB&& save_b) {
    if (unfinished) {
        save_b();
        if (speaks) {
            ps.tol_state[pc.col] = tol;
            ps.it_state[pc.col] = (uint8_t)it;
        }
    }
    if (pc.valid && !unfinished && speaks) sgl_nnls_packing_key(ps.prev_it, pc.col, it);
    const unsigned long long um = __ballot(unfinished) & LANES;
    if (um != 0ull) {
        const int lane = threadIdx.x & 63;
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(ps.next_count, (unsigned)__popcll(um));
        base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
        if (unfinished && speaks) ps.next_list[base + (unsigned)__popcll(um & ((1ull << lane) - 1ull))] = (int32_t)pc.col;
    }
    sgl_nnls_book_sweeps(sweep_counter, (pc.valid && !unfinished && speaks) ? it : 0, ran);
}
// The bounded-tol solve (kernels_nnls_asm_bounded.hip): a lane whose stop test the bounded tol could not decide is TAINTED.  The
// kernel has stored nothing of it -- B, X, tol_state and it_state hold the state the column entered the pass with -- and
// sgl_nnls_pass_exit has seen it as a lane without a column (no packing key, no sweeps booked).  It is appended to the redo list
// (wave-aggregated, like next_list), which the exact kernel runs over after the last pass, resuming every column; a column of
// a first pass has no saved state yet and gets the one every column starts with.
__device__ __forceinline__ void sgl_nnls_pass_redo(const NnlsPass& ps, const SglNnlsPassCol& pc, bool tainted) {
    const unsigned long long tm = __ballot(tainted);
    if (tm == 0ull) return;
    const int lane = threadIdx.x & 63;
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(ps.redo_count, (unsigned)__popcll(tm));
    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    if (tainted) {
        ps.redo_list[base + (unsigned)__popcll(tm & ((1ull << lane) - 1ull))] = (int32_t)pc.col;
        if (!pc.resume && ps.tol_state != nullptr) {
            ps.tol_state[pc.col] = 1.0;
            ps.it_state[pc.col] = 0;
        }
    }
}
