// Host logic of the spatial autocorrelation calls (include/singlet_hip.h, "Spatial autocorrelation") that makes no HIP call: the
// rules of the arguments and the naming of the first offender, the graph moments S0 / S1 / S2 / t, and the assembly of Moran's
// I, its expectation, its standard deviation under either variance, z, p and Benjamini-Hochberg from the per-row moments.
// Plain C++ over plain pointers, so tests/moran_host_main.cpp compiles it alone under -fsanitize=address,undefined and runs it
// on the CPU.  Every sum is sequential, in double, and no product is contracted into the addition after it.
#pragma once
#include <math.h>
#include <cmath>
#include <stdint.h>

#include <vector>

#include "gsea_host.h"   // gsea_bh: Benjamini-Hochberg over the values that are not NaN

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF   // (a host compiler without the pragma targets no fused multiply-add unless asked to)
#endif

#define MORAN_SEG 8192       // entries per segment: part of the stated summation order
#define MORAN_LDS_CAP 5120   // entries of one gene staged in LDS by the search path: the default (and largest) lds_cap
#define MORAN_MAX_K 1024
#define MORAN_MIN_N 4

enum MoranArgError {
    MORAN_ARGS_OK = 0,
    MORAN_ARGS_NULL,      // a NULL graph array
    MORAN_ARGS_N,         // n < 4 or n > INT32_MAX; *val = n
    MORAN_ARGS_NGENES,    // n_genes < 0, or a list without an address; *val = n_genes
    MORAN_ARGS_RANGE,     // genes[*at] = *val outside [0, m)
    MORAN_ARGS_REPEAT,    // genes[*at] = *val was listed before
    MORAN_ARGS_PATH,      // path outside {0, 1, 2}; *val = path
    MORAN_ARGS_CAP,       // lds_cap < 0 or table_batch < 0; *val = the knob
};

// The refusals of the gene list and the knobs, in this order; the whole list is read before anything is uploaded.
// genes == NULL: all m genes (n_genes is then ignored).
inline MoranArgError moran_check_genes(const int32_t* genes, int64_t n_genes, int64_t m, int64_t path, int64_t lds_cap, int64_t table_batch,
                                       int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (path < 0 || path > 2) { *val = path; return MORAN_ARGS_PATH; }
    if (lds_cap < 0) { *val = lds_cap; return MORAN_ARGS_CAP; }
    if (table_batch < 0) { *val = table_batch; return MORAN_ARGS_CAP; }
    if (!genes) return MORAN_ARGS_OK;
    if (n_genes < 0 || n_genes > (int64_t)INT32_MAX) { *val = n_genes; return MORAN_ARGS_NGENES; }
    std::vector<bool> seen((size_t)(m > 0 ? m : 0), false);
    for (int64_t q = 0; q < n_genes; ++q) {
        const int64_t g = genes[q];
        if (g < 0 || g >= m) { *at = q; *val = g; return MORAN_ARGS_RANGE; }
        if (seen[(size_t)g]) { *at = q; *val = g; return MORAN_ARGS_REPEAT; }
        seen[(size_t)g] = true;
    }
    return MORAN_ARGS_OK;
}

// the LDS cap in force: 0 and anything above the largest are the default
inline int64_t moran_lds_cap(int64_t lds_cap) { return lds_cap <= 0 || lds_cap > MORAN_LDS_CAP ? MORAN_LDS_CAP : lds_cap; }
// the path of a gene of c stored entries: 1 search, 2 table.  A forced search path still sends a gene that LDS cannot hold
// to the table.
inline int moran_gene_path(int64_t c, int path, int64_t lds_cap) {
    if (path == 2) return 2;
    if (path == 1) return c <= MORAN_LDS_CAP ? 1 : 2;
    return c <= moran_lds_cap(lds_cap) ? 1 : 2;
}

// The graph moments of a checked n x n dgCMatrix (finite weights, ascending rows).  t: n values, may be NULL.
//  S0 = sum of w in stored order (one chain over all columns, ascending);
//  colsum_j = sequential in stored order; rowsum_i through a counting transpose = sequential over ascending column index;
//  t_i = rowsum_i + colsum_i;  S2 = sum of t_i * t_i, ascending i;
//  S1 = 0.5 * sum over the union pattern of (w_ij + w_ji)^2, walked by merging column j of G with column j of t(G), j
//  ascending, rows ascending, an absent partner counting as +0.0.
// Returns 0, or 1 when S0 == 0 or a moment is not finite (the caller refuses the graph).
inline int moran_graph_moments(const double* Gx, const int32_t* Gi, const int32_t* Gp, int64_t n, double* S0_out, double* S1_out,
                               double* S2_out, double* t_out) {
    const int64_t nnz = Gp[n];
    // counting transpose: row i of G as (column, weight) pairs, columns ascending
    std::vector<int64_t> tp((size_t)n + 1, 0);
    for (int64_t q = 0; q < nnz; ++q) ++tp[(size_t)Gi[q] + 1];
    for (int64_t i = 0; i < n; ++i) tp[(size_t)i + 1] += tp[(size_t)i];
    std::vector<int32_t> ti((size_t)(nnz > 0 ? nnz : 1));
    std::vector<double> tx((size_t)(nnz > 0 ? nnz : 1));
    {
        std::vector<int64_t> at(tp.begin(), tp.end() - 1);
        for (int64_t j = 0; j < n; ++j)
            for (int64_t q = Gp[j]; q < Gp[j + 1]; ++q) {
                const int64_t d = at[(size_t)Gi[q]]++;
                ti[(size_t)d] = (int32_t)j;
                tx[(size_t)d] = Gx[q];
            }
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    std::vector<double> t((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        double cs = 0.0, rs = 0.0;
        for (int64_t q = Gp[j]; q < Gp[j + 1]; ++q) { S0 += Gx[q]; cs += Gx[q]; }
        for (int64_t q = tp[(size_t)j]; q < tp[(size_t)j + 1]; ++q) rs += tx[(size_t)q];
        t[(size_t)j] = rs + cs;
    }
    for (int64_t i = 0; i < n; ++i) S2 += t[(size_t)i] * t[(size_t)i];
    for (int64_t j = 0; j < n; ++j) {
        int64_t a = Gp[j], b = tp[(size_t)j];
        const int64_t a1 = Gp[j + 1], b1 = tp[(size_t)j + 1];
        while (a < a1 || b < b1) {
            // w_rj from column j of G, w_jr from column j of t(G); the lower row index goes first
            double wa = 0.0, wb = 0.0;
            if (b >= b1 || (a < a1 && Gi[a] < ti[(size_t)b])) wa = Gx[a++];
            else if (a >= a1 || ti[(size_t)b] < Gi[a]) wb = tx[(size_t)b++];
            else { wa = Gx[a++]; wb = tx[(size_t)b++]; }
            const double s = wa + wb;
            S1 += s * s;
        }
    }
    S1 = 0.5 * S1;
    *S0_out = S0;
    *S1_out = S1;
    *S2_out = S2;
    if (t_out)
        for (int64_t i = 0; i < n; ++i) t_out[i] = t[(size_t)i];
    bool finite = std::isfinite(S0) && std::isfinite(S1) && std::isfinite(S2);
    for (int64_t i = 0; i < n && finite; ++i) finite = std::isfinite(t[(size_t)i]);
    return (S0 == 0.0 || !finite) ? 1 : 0;
}

// The assembly.  moments: 6 x rows column-major (mean, M2, M4, T, P, c_g); variance 0 randomisation, 1 normality;
// alternative 0 two.sided, 1 greater, 2 less.  Any output may be NULL.  Arguments checked by the caller (n >= 4, S0 != 0).
//   C = (P - m * T) + (m * m) * S0;  I = ((double)n / S0) * (C / M2);  EI = -1 / (double)(n - 1);
//   normality:      V = ((nn * nn) * S1 - nn * S2 + 3 * (S0 * S0)) / (((nn * nn) - 1) * (S0 * S0)) - EI * EI
//   randomisation:  b2 = (nn * M4) / (M2 * M2),
//                   V = (nn * (((nn * nn) - 3 * nn + 3) * S1 - nn * S2 + 3 * (S0 * S0))
//                        - b2 * ((nn * (nn - 1)) * S1 - (2 * nn) * S2 + 6 * (S0 * S0))) / (((nn - 1) * (nn - 2) * (nn - 3)) * (S0 * S0)) - EI * EI
//   sd = sqrt(V);  z = (I - EI) / sd;  p = erfc(|z| / sqrt(2)) two.sided, 0.5 erfc(-z / sqrt(2)) less, 0.5 erfc(z / sqrt(2)) greater.
// M2 == 0 (a constant row): I, z and p are NaN.  p_adj: Benjamini-Hochberg over the rows whose p is not NaN.
inline void moran_stats(int64_t n, double S0, double S1, double S2, int64_t rows, const double* moments, int variance, int alternative,
                        double* I_out, double* EI_out, double* sd_out, double* z_out, double* p_out, double* padj_out) {
    const double nn = (double)n;
    const double EI = -1.0 / (double)(n - 1);
    const double s02 = S0 * S0;
    std::vector<double> pv((size_t)(rows > 0 ? rows : 1), NAN);
    for (int64_t r = 0; r < rows; ++r) {
        const double* mo = moments + 6 * r;
        const double m = mo[0], M2 = mo[1], M4 = mo[2], T = mo[3], P = mo[4];
        const double C = (P - m * T) + (m * m) * S0;
        double I = (nn / S0) * (C / M2);
        double V;
        if (variance == 1) {
            V = ((nn * nn) * S1 - nn * S2 + 3.0 * s02) / (((nn * nn) - 1.0) * s02) - EI * EI;
        } else {
            const double b2 = (nn * M4) / (M2 * M2);
            const double a = nn * (((nn * nn) - 3.0 * nn + 3.0) * S1 - nn * S2 + 3.0 * s02);
            const double b = b2 * ((nn * (nn - 1.0)) * S1 - (2.0 * nn) * S2 + 6.0 * s02);
            V = (a - b) / (((nn - 1.0) * (nn - 2.0) * (nn - 3.0)) * s02) - EI * EI;
        }
        const double sd = sqrt(V);
        double z = (I - EI) / sd, p;
        if (M2 == 0.0) { I = NAN; z = NAN; }
        if (z != z) p = NAN;
        else if (alternative == 1) p = 0.5 * erfc(z / M_SQRT2);
        else if (alternative == 2) p = 0.5 * erfc(-z / M_SQRT2);
        else p = erfc(fabs(z) / M_SQRT2);
        if (I_out) I_out[r] = I;
        if (EI_out) EI_out[r] = EI;
        if (sd_out) sd_out[r] = sd;
        if (z_out) z_out[r] = z;
        if (p_out) p_out[r] = p;
        pv[(size_t)r] = p;
    }
    if (padj_out && rows > 0) gsea_bh(pv.data(), rows, padj_out);
}
