// nnls_lane_kernel<KP>: nnls (src/singlet.cpp:229-250) with ONE LANE PER COLUMN (see kernels_nnls.hip
// for the two mappings), in re-packing passes (nnls_static_for.h).  Included by kernels_nnls_lane{1,2}.hip,
// which instantiate disjoint sets of KP so that the (long) compiles run in parallel.
#pragma once
#include "sgl_internal.h"
#ifndef SGL_NNLS_GRAM_LDS
#define SGL_NNLS_GRAM_LDS 1
#endif

#include "nnls_static_for.h"

// GV = false: the Gram reaches the FMAs as scalar operands (s_load; row stride KP).
// GV = true : row i of the Gram is fetched with ceil(KP / 16) coalesced vector loads, every 16-lane row of
//   the wave holding the same 16 entries (row stride GS = KP rounded up to 16), and entry j reaches FMA j as a
//   DPP row broadcast (v_fmac_f64_dpp ... row_newbcast:j%16).  Vector loads return in order and cost no
//   SGPRs: a whole row no longer has to fit the ~100 free SGPRs (the cliff above k = 50) and hipcc can
//   keep the next rows in flight.
template <int J>
__device__ __forceinline__ void nnls_dpp_fmac(double& acc, double g, double nd) {
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(g), "v"(nd), "n"(J));
}
template <int J>
__device__ __forceinline__ double nnls_dpp_bcast(double g) {
    int lo = __double2loint(g), hi = __double2hiint(g), rl, rh;
    asm("v_mov_b32_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(rl) : "v"(lo), "n"(J));
    asm("v_mov_b32_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(rh) : "v"(hi), "n"(J));
    return __hiloint2double(rh, rl);
}

// k <= 64: b and x of a column both live in VGPRs (ranks above run two lanes per column, nnls_half.h).
template <int KP, bool GV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void nnls_lane_kernel(const double* __restrict__ Gpad, double* __restrict__ B,
                                                        double* __restrict__ X, const int64_t* __restrict__ col_nnz,
                                                        int k, int64_t ncols, double L1, double L2,
                                                        unsigned long long* __restrict__ sweep_counter, NnlsPass ps) {
    const int64_t n_in = sgl_nnls_pass_size(ps, ncols);
    if ((int64_t)blockIdx.x * blockDim.x >= n_in) return;
    // GV: the padded Gram (rows 0 .. KP: the Gram and the reciprocals of its diagonal, (KP + 1) x GS doubles, 33 KB
    // at KP = 64) is staged ONCE per workgroup in LDS and the sweeps read their rows from there: immediate offsets off one
    // per-lane base (no per-coordinate address arithmetic), LDS latency instead of the vector cache's.
    constexpr bool GLDS = GV && SGL_NNLS_GRAM_LDS;
    constexpr int GS_ = ((KP + 15) / 16) * 16;
    __shared__ double Gl[GLDS ? (KP + 1) * GS_ : 1];
    __shared__ __attribute__((aligned(16))) double Dl[GLDS ? 2 * KP : 2];   // (G_jj, 1 / G_jj) pairs: one uniform 16-byte read per coordinate
    if (GLDS) {
        for (int e = threadIdx.x; e < (KP + 1) * GS_; e += blockDim.x) Gl[e] = Gpad[e];
        for (int j = threadIdx.x; j < KP; j += blockDim.x) {
            Dl[2 * j] = Gpad[j * GS_ + j];
            Dl[2 * j + 1] = Gpad[KP * GS_ + j];
        }
        __syncthreads();
    }
    const SglNnlsPassCol pc = sgl_nnls_pass_entry(ps, n_in, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, col_nnz);
    const int64_t col = pc.col;
    const bool valid = pc.valid, to_end = pc.to_end;
    // An instance serves KP - 1 <= k <= KP: for the coordinates below KLOW the run-time test
    // `i < k` is always true.  hipcc implemented it as a lane mask kept in (spilled) SGPRs -- ~10 instructions per
    // coordinate -- but simply dropping it makes the whole sweep ONE basic block, and then the register allocator
    // spills (368 B of scratch per lane at KP = 50 against 20, nnls_h 7.1 -> 10.7 ms at config 3).  So those
    // coordinates keep a branch, on an opaque always-true scalar: s_cmp + s_cbranch, no mask (nnls_h 6.6 -> 5.8 ms).
    constexpr int KLOW = KP - 1;
    int one = 1;
    double b[KP], x[KP];
    double* bp = B + col * k;
    double* xp = X + col * k;
    static_for<KP>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        b[j] = (valid && j < k) ? bp[j] : 0.0;
        x[j] = (valid && j < k) ? xp[j] : 0.0;
    });
    const double kd = (double)k;
    double tol;
    int it;
    sgl_nnls_pass_state(ps, pc, tol, it);
    int gofs = 0, ran = 0;
    const int n_act0 = __popcll(__ballot(valid && it < 100 && (tol / kd) > 1e-8));
    while (true) {
        const bool go = valid && it < 100 && (tol / kd) > 1e-8;
        const int n_act = __popcll(__ballot(go));
        if (n_act == 0) break;
        if (!to_end && n_act * SGL_NNLS_REPACK_DEN < n_act0 * SGL_NNLS_REPACK_NUM) break;  // re-pack the stragglers
        ++ran;
        if (go) tol = 0.0;
        // launder a (wave-uniform, always zero) offset once per sweep: the k*k scalar loads of the
        // Gram must be re-issued every sweep instead of being hoisted out of the loop and spilled.
        // The pointer itself keeps its provenance (global, read-only) so the loads stay s_load.
        asm volatile("" : "+s"(gofs));
        const double* __restrict__ Gs = Gpad + gofs;
        constexpr int NG = (KP + 15) / 16, GS = NG * 16;
        const double* __restrict__ Gvg = Gpad + gofs + (threadIdx.x & 15);
        const int gl0 = gofs + (int)(threadIdx.x & 15);
        // entry X of this lane's column of the padded Gram (LDS keeps its address space: no generic pointer)
        auto Gv = [&](int X) -> double { if constexpr (GLDS) return Gl[gl0 + X]; else return Gvg[X]; };
        // GV: explicit one-row-ahead software pipeline of the Gram rows (g2[parity]), fenced with
        // scheduling barriers: left alone, hipcc hoists the loads of dozens of rows of this straight-line
        // code and spills.
        // row KP of the padded Gram holds the correctly rounded reciprocals 1 / G_jj (k_pad_gram): the step
        // b_i / G_ii then costs a multiply and two FMAs instead of an 11-instruction IEEE division (below)
        double rrow[(GV && !GLDS) ? NG : 1];
        if (GV && !GLDS) {
#pragma unroll
            for (int m = 0; m < NG; ++m) rrow[m] = Gv(KP * GS + 16 * m);
        }
        // GLDS: the diagonal pair of the coming coordinate, read (uniform address: a broadcast) one coordinate ahead
        double dnext0 = 0.0, dnext1 = 1.0;
        if (GLDS) { dnext0 = Dl[gofs]; dnext1 = Dl[gofs + 1]; }
        double g2[2][NG];
        if (GV) {
#pragma unroll
            for (int m = 0; m < NG; ++m) g2[0][m] = Gv(16 * m);
        }
        static_for<KP>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            bool run_i = i < k;
            if (i < KLOW) { asm volatile("" : "+s"(one)); run_i = one != 0; }   // opaque, always true: keeps one basic block per coordinate
            if (run_i) {
                const double xi = x[i];
                double grow[NG];
                double gii, rii;
                if (GV) {
                    if (i + 1 < KLOW || i + 1 < k) {
#pragma unroll
                        for (int m = 0; m < NG; ++m) g2[(i + 1) & 1][m] = Gv((i + 1) * GS + 16 * m);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int m = 0; m < NG; ++m) grow[m] = g2[i & 1][m];
                    if (GLDS) {
                        gii = dnext0; rii = dnext1;
                        if (i + 1 < KP) { dnext0 = Dl[gofs + 2 * (i + 1)]; dnext1 = Dl[gofs + 2 * (i + 1) + 1]; }
                    } else {
                        gii = nnls_dpp_bcast<(i & 15)>(grow[i >> 4]);
                        rii = nnls_dpp_bcast<(i & 15)>(rrow[GLDS ? 0 : (i >> 4)]);
                    }
                } else {
                    gii = Gs[i + KP * i];
                    rii = Gs[KP * KP + i];
                }
                const double diff0 = sgl_nnls_markstein(b[i], gii, rii);
                // l.235-247 through sgl_nnls_step (branch-free; a stopped column takes a zero step)
                double xv = xi;
                const double nd = sgl_nnls_step(diff0, xv, tol, go, L1, L2);
                x[i] = xv;
                static_for<KP>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    if (GV) nnls_dpp_fmac<(j & 15)>(b[j], grow[j >> 4], nd);
                    else b[j] = fma(Gs[j + KP * i], nd, b[j]);
                });
                if (GV) __builtin_amdgcn_sched_barrier(0);
            }
        });
        it += go ? 1 : 0;
    }
    const bool unfinished = valid && it < 100 && (tol / kd) > 1e-8;  // only possible when !to_end
    if (valid) {
        static_for<KP>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (j < k) xp[j] = x[j];
        });
    }
    sgl_nnls_pass_exit<~0ull>(ps, pc, unfinished, true, tol, it, ran, sweep_counter, [&] {
        static_for<KP>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (j < k) bp[j] = b[j];
        });
    });
}

// the instances for the even KP in [KLO, KHI].  GV is fixed per translation unit: scalar operands up to KP = 40 (3-10 % faster
// there), vector loads + DPP broadcast from KP = 42 (11 % faster at k = 50, 2.3x at k = 56 .. 64, where a row no longer fits the
// free SGPRs).  nnls_gram_stride() in kernels_nnls.hip must agree.
template <int KLO, int KHI, bool GV>
static int nnls_lane_launch(hipStream_t s, const double* Gpad, int KP, double* B, double* X, const int64_t* col_nnz, int k, int64_t ncols,
                            double L1, double L2, unsigned long long* sweep_counter, const NnlsPass& ps, dim3 g, dim3 b) {
    if (KP % 2 != 0 || KP < KLO || KP > KHI) { sgl_set_error("k_nnls_lane: unsupported KP=%d", KP); return SGL_EINVAL; }
    return sgl_rank_dispatch<KLO / 2, KHI / 2>(KP / 2, [&](auto h) {
        nnls_lane_kernel<2 * decltype(h)::value, GV><<<g, b, 0, s>>>(Gpad, B, X, col_nnz, k, ncols, L1, L2, sweep_counter, ps);
        return SGL_OK;
    });
}
