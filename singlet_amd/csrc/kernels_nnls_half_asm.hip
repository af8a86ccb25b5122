// nnls (src/singlet.cpp:229-250) for 64 < k <= 128, TWO lanes per column, with the whole solve as generated, hand-scheduled
// assembly (gen_nnls_half.py -> nnls_half_gen.inc; round 5).  Same interface, passes / packing protocol (nnls_static_for.h) and results as
// nnls_half_kernel<KH> (nnls_half.h): lane c and lane 32 + c of a wave share column c of the wave's 32, the lower half-wave holds
// coordinates 0 .. KH - 1 of b and x, the upper half KH .. 2 KH - 1.  What differs is inside the sweep (header of gen_nnls_half.py):
// one half computes a coordinate's step, only nd crosses the halves, and the step's chain is interleaved with the row-update FMAs
// of its neighbours.  As in kernels_nnls_asm.hip the solve is ONE asm statement whose clobbers b, x and its working set are.
#include "sgl_internal.h"
#include "nnls_static_for.h"
#include "nnls_half_gen.inc"

#define SGL_DEFINE_NNLS_HALF_ASM_KERNEL(KP)                                                                                         \
    __global__ __launch_bounds__(NNLS_HALF_ASM_THREADS_##KP) __attribute__((amdgpu_waves_per_eu(NNLS_HALF_ASM_WAVES_##KP, NNLS_HALF_ASM_WAVES_##KP)))      \
    void nnls_half_asm_kernel_##KP(const double* __restrict__ Gpad, int gs_in, double* __restrict__ B, double* __restrict__ X,       \
                                   const int64_t* __restrict__ col_nnz, int k, int64_t ncols, double L1, double L2,                 \
                                   unsigned long long* __restrict__ sweep_counter, NnlsPass ps) {                                   \
        constexpr int KH = KP / 2, NGH = NNLS_HALF_ASM_NGH_##KP, NGHP = NNLS_HALF_ASM_NGHP_##KP, ROW = 32 * NGHP;                   \
        const int64_t n_in = sgl_nnls_pass_size(ps, ncols);                                                                         \
        const int cpb = (int)(blockDim.x >> 1); /* columns per workgroup */                                                         \
        if ((int64_t)blockIdx.x * cpb >= n_in) return;                                                                              \
        extern __shared__ __attribute__((aligned(16))) double nnls_half_asm_lds[];                                                  \
        double* const Dl = nnls_half_asm_lds;            /* (G_ii, 1 / G_ii) */                                                     \
        double* const Gl = nnls_half_asm_lds + 2 * KP;   /* Gl[i][h][l][m] = G[i, h KH + l + 16 m] */                               \
        for (int e = threadIdx.x; e < KP * ROW; e += blockDim.x) {                                                                  \
            const int i = e / ROW, r = e - i * ROW, hl = r / NGHP, m = r - hl * NGHP, h = hl >> 4, jl = (hl & 15) + 16 * m;          \
            Gl[e] = (m < NGH && jl < KH) ? Gpad[h * KH + jl + gs_in * i] : 0.0;                                                     \
        }                                                                                                                           \
        for (int j = threadIdx.x; j < KP; j += blockDim.x) {                                                                        \
            Dl[2 * j] = Gpad[j * gs_in + j];                                                                                        \
            Dl[2 * j + 1] = Gpad[KP * gs_in + j];   /* row KP of the padded Gram: the correctly rounded reciprocals */              \
        }                                                                                                                           \
        __syncthreads();                                                                                                            \
        const int lane = threadIdx.x & 63, half = lane >> 5;                                                                        \
        const int64_t gid = (int64_t)blockIdx.x * cpb + (threadIdx.x >> 6) * 32 + (lane & 31);   /* position in this pass */        \
        const SglNnlsPassCol pc = sgl_nnls_pass_entry(ps, n_in, gid, col_nnz);                                                      \
        double* const bp = B + pc.col * k + half * KH;                                                                              \
        double* const xp = X + pc.col * k + half * KH;                                                                              \
        const unsigned kh = (unsigned)(half ? k - KH : KH);   /* coordinates this lane holds */                                     \
        typedef __attribute__((address_space(3))) char lds_char;                                                                    \
        const unsigned gl = (unsigned)(uintptr_t)(lds_char*)Gl + (unsigned)(half * 16 + (lane & 15)) * (NGHP * 8);                  \
        const unsigned dl = (unsigned)(uintptr_t)(lds_char*)Dl;                                                                     \
        const double kd = (double)k;                                                                                                \
        double tol;                                                                                                                 \
        int it;                                                                                                                     \
        sgl_nnls_pass_state(ps, pc, tol, it);                                                                                       \
        int ran = 0, tlo = __double2loint(tol), thi = __double2hiint(tol);                                                          \
        unsigned long long um = 0ull;                                                                                               \
        const unsigned long long vm = __ballot(pc.valid);                                                                           \
        const double eps = 1e-15, thr = 1e-8;                                                                                       \
        const unsigned one_hi = 0x3ff00000u;                                                                                        \
        const int toend_s = __builtin_amdgcn_readfirstlane(pc.to_end ? 1 : 0);                                                      \
        asm volatile(NNLS_HALF_ASM_BODY_##KP                                                                                        \
                     : [it] "+v"(it), [lo] "+v"(tlo), [hi] "+v"(thi), [ran] "+s"(ran), [um] "=s"(um)                                \
                     : [bp] "v"(bp), [xp] "v"(xp), [gl] "v"(gl), [dl] "v"(dl), [one_hi] "v"(one_hi), [kh] "v"(kh), [valid] "s"(vm), \
                       [l1] "s"(L1), [l2] "s"(L2), [eps] "s"(eps), [kd] "s"(kd), [thr] "s"(thr), [toend] "s"(toend_s)               \
                     : NNLS_HALF_ASM_VCLOB_##KP, "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50",       \
                       "s51", "vcc", "scc", "memory");                                                                              \
        tol = __hiloint2double(thi, tlo);                                                                                           \
        const bool unfinished = ((um >> lane) & 1ull) != 0ull; /* only possible when !to_end; both lanes of a column agree */       \
        sgl_nnls_pass_exit<0xffffffffull>(ps, pc, unfinished, half == 0, tol, it, ran, sweep_counter, [] {});                       \
    }

SGL_NNLS_HALF_ASM_INSTANCES(SGL_DEFINE_NNLS_HALF_ASM_KERNEL)

// whether the generated two-lane solve serves padded rank KP.  Instances are multiples of 4 -- k = 100 runs unpadded, where the
// compiled kernels' multiples of 8 make it 104 -- and need L1 >= 0 (a padded coordinate is an exact no-op only then).
bool nnls_half_asm_has(int KP, double L1) {
    if (!(L1 >= 0.0) || getenv("SGL_NNLS_NO_ASM")) return false;
#define SGL_NNLS_HALF_ASM_HAS(K_) if (KP == K_) return true;
    SGL_NNLS_HALF_ASM_INSTANCES(SGL_NNLS_HALF_ASM_HAS)
#undef SGL_NNLS_HALF_ASM_HAS
    return false;
}

int k_nnls_half_launch_asm(hipStream_t s, const double* Gpad, int KP, double* B, double* X, const int64_t* col_nnz, int k,
                           int64_t ncols, double L1, double L2, unsigned long long* sweep_counter, const NnlsPass& ps) {
    const int gs_in = nnls_gram_stride(KP);
#define SGL_NNLS_HALF_ASM_CASE(K_)                                                                                                  \
    if (KP == K_) {                                                                                                                 \
        const size_t lds = sizeof(double) * ((size_t)K_ * 32 * NNLS_HALF_ASM_NGHP_##K_ + 2 * K_);                                   \
        /* the staged Gram leaves room for ONE workgroup per CU from KP = 80 on: 512 threads there (two waves per SIMD) when     */ \
        /* there are columns enough, 256 below                                                                                   */ \
        const int cpb = (2 * lds > 160 * 1024 && ncols >= 256 * 256 && NNLS_HALF_ASM_WAVES_##K_ > 1) ? 256 : 128;                   \
        const dim3 g((unsigned)((ncols + cpb - 1) / cpb)), b(2 * cpb);                                                              \
        SGLCHK(sgl_allow_dynamic_lds<&nnls_half_asm_kernel_##K_>((int)lds));                                                        \
        nnls_half_asm_kernel_##K_<<<g, b, lds, s>>>(Gpad, gs_in, B, X, col_nnz, k, ncols, L1, L2, sweep_counter, ps);               \
        HIPCHK(hipGetLastError());                                                                                                  \
        return SGL_OK;                                                                                                              \
    }
    SGL_NNLS_HALF_ASM_INSTANCES(SGL_NNLS_HALF_ASM_CASE)
#undef SGL_NNLS_HALF_ASM_CASE
    sgl_set_error("k_nnls_half_asm: no instance for KP=%d", KP);
    return SGL_EINVAL;
}
