// The generated lane-per-column NNLS (kernels_nnls_asm.hip) with a BOUNDED tol: gen_nnls_lane.py's Sweep(KP, bounded=True).
//
// tol enters one comparison per sweep -- tol / k > 1e-8 -- and nothing else: x, b and the sweep counts never see it.  The exact
// kernel pays 8 FP64 instructions per coordinate for the correctly rounded quotient nd / (x_i + 1e-15) behind it.  Here the
// quotient is v_rcp_f64 and ONE Newton step (4 instructions), the running sum S is within a relative delta of the exact tol
// ("The bounded tol": delta >= 2 (eps_r^2 + (KP + 4) 2^-52)), and the stop test -- the same correctly rounded one -- is
// run on S (1 - delta) and on S (1 + delta).  It is monotone in tol, so where both ends agree that IS the exact kernel's
// decision.  Where they do not, the lane is tainted: it stops, nothing of it is stored, it is listed, and k_nnls_lane runs the
// exact kernel over the list afterwards (sgl_nnls_pass_redo).  Results are the exact kernel's bit for bit, sweep for sweep.
// For L2 = 0 and L1 >= 0 only (the L2 term is not issued; the gate and L1 are one FMA), ranks with x in the vector registers.
#include "sgl_internal.h"
#include "nnls_static_for.h"
#include "nnls_lane_gen.inc"

#define SGL_DEFINE_NNLS_ASMB_KERNEL(KP)                                                                                             \
    __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NNLS_ASM_WAVES_##KP, NNLS_ASM_WAVES_##KP))) void nnls_lane_asmb_kernel_##KP(           \
        const double* __restrict__ Gpad, int gs_in, double* __restrict__ B, double* __restrict__ X,                                \
        const int64_t* __restrict__ col_nnz, int k, int64_t ncols, double L1, double dlt,                                          \
        unsigned long long* __restrict__ sweep_counter, NnlsPass ps) {                                                             \
        constexpr int NG = (KP + 15) / 16, NGP = NNLS_ASM_NGP_##KP, ROW = 16 * NGP;                                                \
        const int64_t n_in = sgl_nnls_pass_size(ps, ncols);                                                                         \
        /* (the order of a packed single pass: kernels_nnls_asm.hip) */                                                            \
        unsigned bx = blockIdx.x;                                                                                                   \
        if (ps.fresh == 2 && gridDim.x > 256u && gridDim.x <= 512u) {                                                               \
            const unsigned alone = 512u - gridDim.x;                                                                                \
            bx = bx >= 256u ? gridDim.x - 1u - (bx - 256u) : (bx < 256u - alone ? alone + bx : bx - (256u - alone));               \
        }                                                                                                                           \
        if ((int64_t)bx * blockDim.x >= n_in) return;                                                                               \
        extern __shared__ __attribute__((aligned(16))) double nnls_asmb_lds[];                                                      \
        double* const Gl = nnls_asmb_lds;             /* Gl[i][l][m] = G[i, l + 16 m] */                                            \
        double* const Dl = nnls_asmb_lds + KP * ROW;  /* (G_ii, 1 / G_ii) */                                                        \
        for (int e = threadIdx.x; e < KP * ROW; e += blockDim.x) {                                                                  \
            const int i = e / ROW, r = e - i * ROW, l = r / NGP, m = r - l * NGP, j = l + 16 * m;                                   \
            Gl[e] = (m < NG && j < KP) ? Gpad[j + gs_in * i] : 0.0;                                                                 \
        }                                                                                                                           \
        for (int j = threadIdx.x; j < KP; j += blockDim.x) {                                                                        \
            Dl[2 * j] = Gpad[j * gs_in + j];                                                                                        \
            Dl[2 * j + 1] = Gpad[KP * gs_in + j];                                                                                   \
        }                                                                                                                           \
        __syncthreads();                                                                                                            \
        const SglNnlsPassCol pc = sgl_nnls_pass_entry(ps, n_in, (int64_t)bx * blockDim.x + threadIdx.x, col_nnz);                   \
        double* const bp = B + pc.col * k;                                                                                          \
        double* const xp = X + pc.col * k;                                                                                          \
        typedef __attribute__((address_space(3))) char lds_char;                                                                    \
        const unsigned gl = (unsigned)(uintptr_t)(lds_char*)Gl + (unsigned)(threadIdx.x & 15) * (NGP * 8);                          \
        const unsigned dl = (unsigned)(uintptr_t)(lds_char*)Dl;                                                                     \
        const double kd = (double)k;                                                                                                \
        double tol;                                                                                                                 \
        int it;                                                                                                                     \
        sgl_nnls_pass_state(ps, pc, tol, it);                                                                                       \
        int ran = 0, tlo = __double2loint(tol), thi = __double2hiint(tol);                                                          \
        unsigned long long um = 0ull, tn = 0ull;                                                                                    \
        const unsigned long long vm = __ballot(pc.valid);                                                                           \
        const double eps = 1e-15, thr = 1e-8;                                                                                       \
        const unsigned one_hi = 0x3ff00000u;                                                                                        \
        const int toend_s = __builtin_amdgcn_readfirstlane(pc.to_end ? 1 : 0), klast_s = __builtin_amdgcn_readfirstlane(k == KP ? 1 : 0); \
        asm volatile(NNLS_ASMB_BODY_##KP                                                                                            \
                     : [it] "+v"(it), [lo] "+v"(tlo), [hi] "+v"(thi), [ran] "+s"(ran), [um] "=&s"(um), [tn] "+s"(tn)                \
                     : [bp] "v"(bp), [xp] "v"(xp), [gl] "v"(gl), [dl] "v"(dl), [one_hi] "v"(one_hi), [valid] "s"(vm),               \
                       [l1] "s"(L1), [dlt] "s"(dlt), [eps] "s"(eps), [kd] "s"(kd), [thr] "s"(thr), [toend] "s"(toend_s),           \
                       [klast] "s"(klast_s)                                                                                         \
                     : NNLS_ASM_VCLOB_##KP, "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51",     \
                       "vcc", "scc", "memory");                                                                                     \
        tol = __hiloint2double(thi, tlo);                                                                                           \
        const bool unfinished = ((um >> (threadIdx.x & 63)) & 1ull) != 0ull; /* only possible when !to_end */                       \
        const bool tainted = ((tn >> (threadIdx.x & 63)) & 1ull) != 0ull;                                                           \
        SglNnlsPassCol pq = pc;   /* a tainted lane leaves the pass like a lane without a column */                                 \
        pq.valid = pc.valid && !tainted;                                                                                            \
        sgl_nnls_pass_exit<~0ull>(ps, pq, unfinished, true, tol, it, ran, sweep_counter, [] {});                                    \
        sgl_nnls_pass_redo(ps, pc, tainted);                                                                                        \
    }

SGL_NNLS_ASMB_INSTANCES(SGL_DEFINE_NNLS_ASMB_KERNEL)

bool nnls_lane_asm_has(int KP, double L1, int64_t ncols);

// whether the bounded variant serves this solve: wherever the exact generated sweep does, with L2 = 0, at the ranks it has
bool nnls_lane_asm_bounded_has(int KP, double L1, double L2, int64_t ncols) {
    if (L2 != 0.0 || getenv("SGL_NNLS_EXACT_TOL") || !nnls_lane_asm_has(KP, L1, ncols)) return false;
#define SGL_NNLS_ASMB_HAS(K_) if (KP == K_) return true;
    SGL_NNLS_ASMB_INSTANCES(SGL_NNLS_ASMB_HAS)
#undef SGL_NNLS_ASMB_HAS
    return false;
}

// delta, the relative band of the bounded tol around the exact one: 2 (eps_r^2 + (KP + 4) 2^-52) with eps_r = 2^-13, the relative
// error of v_rcp_f64 the exact quotient relies on too ("The bounded tol").  SGL_NNLS_TOL_BAND widens it (tests: more
// columns, or all of them, take the redo path); it never narrows it.
double nnls_lane_asm_bounded_band(int KP) {
    const double d0 = 2.0 * (0x1p-26 + (double)(KP + 4) * 0x1p-52);
    const char* e = getenv("SGL_NNLS_TOL_BAND");
    const double d = e ? atof(e) : 0.0;
    return d > d0 ? d : d0;
}

int k_nnls_lane_launch_asm_bounded(hipStream_t s, const double* Gpad, int KP, double* B, double* X, const int64_t* col_nnz, int k,
                                   int64_t ncols, double L1, double dlt, unsigned long long* sweep_counter, const NnlsPass& ps, dim3 g, dim3 b) {
    const int gs_in = nnls_gram_stride(KP);
#define SGL_NNLS_ASMB_CASE(K_)                                                                                                      \
    if (KP == K_) {                                                                                                                 \
        const size_t lds = sizeof(double) * ((size_t)K_ * 16 * NNLS_ASM_NGP_##K_ + 2 * K_);                                         \
        nnls_lane_asmb_kernel_##K_<<<g, b, lds, s>>>(Gpad, gs_in, B, X, col_nnz, k, ncols, L1, dlt, sweep_counter, ps);             \
        HIPCHK(hipGetLastError());                                                                                                  \
        return SGL_OK;                                                                                                              \
    }
    SGL_NNLS_ASMB_INSTANCES(SGL_NNLS_ASMB_CASE)
#undef SGL_NNLS_ASMB_CASE
    sgl_set_error("k_nnls_lane_asm_bounded: no instance for KP=%d", KP);
    return SGL_EINVAL;
}
