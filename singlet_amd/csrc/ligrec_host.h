// Host logic of the ligand-receptor calls (include/singlet_hip.h, "Ligand-receptor interactions") that makes no HIP call: the
// argument rules in their stated order and the naming of the offender, the plan (path, vectors per wave, waves per workgroup, LDS
// bytes, batch) as a pure function of the sizes and the knobs, the cut of the genes' entries into segments, and the statistics
// (expressed mask, p, Benjamini-Hochberg).  Plain C++ over plain pointers, so tests/ligrec_host_main.cpp compiles it alone under
// -fsanitize=address,undefined and runs it on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "gsea_host.h"   // gsea_bh: Benjamini-Hochberg under the one rule of the library

#define LIGREC_MAX_K 256                            // a label is one byte of the interleaved label table
#define LIGREC_MAX_NPERM ((int64_t)1 << 20)
#define LIGREC_SEG ((int64_t)8192)                  // stored entries of a gene per segment: the unit of one wave's sequential walk
#define LIGREC_MAX_VPW 64                           // label vectors per wave: one per lane
#define LIGREC_WAVE_LDS_BYTES ((int64_t)32 << 10)   // the K x vpw double bins of one wave
#define LIGREC_WG_LDS_BYTES ((int64_t)64 << 10)     // the bins of a workgroup's waves: two workgroups share a CU's 160 KiB
#define LIGREC_MAX_WAVES 8                          // waves per workgroup
#define LIGREC_GRID_WAVES ((int64_t)4096)           // waves of the sums kernel at most: each walks (segment, vector group) items in turn
#define LIGREC_BATCH_BYTES ((int64_t)256 << 20)     // default budget of a batch: per vector n label bytes + (segments + 2 G) K doubles

enum LigrecArgError {
    LIGREC_ARGS_OK = 0,
    LIGREC_ARGS_NULL,        // lab, genes, lig or rec == NULL
    LIGREC_ARGS_K,           // K outside [1, 256]
    LIGREC_ARGS_G,           // G < 1 or G > m
    LIGREC_ARGS_P,           // P < 1
    LIGREC_ARGS_NPERM,       // nperm outside [1, 2^20]
    LIGREC_ARGS_LABEL,       // lab[*at] = *val is outside [0, K)
    LIGREC_ARGS_GENE,        // genes[*at] = *val is outside [0, m)
    LIGREC_ARGS_GENE_TWICE,  // genes[*at] = *val was listed before
    LIGREC_ARGS_LIG,         // lig[*at] = *val is outside [0, G)
    LIGREC_ARGS_REC,         // rec[*at] = *val is outside [0, G)
    LIGREC_ARGS_THRESHOLD,   // threshold outside [0, 1] or NaN
    LIGREC_ARGS_BATCH,       // a negative batch
    LIGREC_ARGS_N,           // n != ncol (*val = n)
    LIGREC_ARGS_PATH,        // path outside {0, 1, 2}
    LIGREC_ARGS_VPW,         // vectors_per_wave = *val is no power of two in [1, *at]
    LIGREC_ARGS_NB,          // nb < 1
};

// count label vectors of n labels each, all in [0, K); *at is the offset into lab
inline LigrecArgError ligrec_check_labels(const int32_t* lab, int64_t n, int64_t count, int64_t K, int64_t* at, int64_t* val) {
    for (int64_t q = 0; q < n * count; ++q)
        if (lab[q] < 0 || lab[q] >= K) { *at = q; *val = lab[q]; return LIGREC_ARGS_LABEL; }
    return LIGREC_ARGS_OK;
}

// distinct gene indices in [0, m)
inline LigrecArgError ligrec_check_genes(const int32_t* genes, int64_t G, int64_t m, int64_t* at, int64_t* val) {
    std::vector<uint8_t> seen((size_t)(m > 0 ? m : 0), 0);
    for (int64_t q = 0; q < G; ++q) {
        const int64_t g = genes[q];
        if (g < 0 || g >= m) { *at = q; *val = g; return LIGREC_ARGS_GENE; }
        if (seen[(size_t)g]) { *at = q; *val = g; return LIGREC_ARGS_GENE_TWICE; }
        seen[(size_t)g] = 1;
    }
    return LIGREC_ARGS_OK;
}

inline LigrecArgError ligrec_check_pairs(const int32_t* lig, const int32_t* rec, int64_t P, int64_t G, int64_t* at, int64_t* val) {
    for (int64_t q = 0; q < P; ++q) {
        if (lig[q] < 0 || lig[q] >= G) { *at = q; *val = lig[q]; return LIGREC_ARGS_LIG; }
        if (rec[q] < 0 || rec[q] >= G) { *at = q; *val = rec[q]; return LIGREC_ARGS_REC; }
    }
    return LIGREC_ARGS_OK;
}

inline bool ligrec_threshold_ok(double t) { return t >= 0.0 && t <= 1.0; }   // (a NaN compares false)

// every refusal of the whole call, in the stated order.  m, ncol: the matrix's genes and cells; n: the labels given.
inline LigrecArgError ligrec_check_call(const int32_t* lab, int64_t n, int64_t K, const int32_t* genes, int64_t G, int64_t m, const int32_t* lig,
                                        const int32_t* rec, int64_t P, int64_t nperm, double threshold, int64_t batch, int64_t ncol, int64_t* at,
                                        int64_t* val) {
    *at = -1;
    *val = 0;
    if (!lab || !genes || !lig || !rec) return LIGREC_ARGS_NULL;
    if (K < 1 || K > LIGREC_MAX_K) { *val = K; return LIGREC_ARGS_K; }
    if (G < 1 || G > m) { *val = G; return LIGREC_ARGS_G; }
    if (P < 1) { *val = P; return LIGREC_ARGS_P; }
    if (nperm < 1 || nperm > LIGREC_MAX_NPERM) { *val = nperm; return LIGREC_ARGS_NPERM; }
    LigrecArgError e = ligrec_check_labels(lab, n > 0 ? n : 0, 1, K, at, val);
    if (e == LIGREC_ARGS_OK) e = ligrec_check_genes(genes, G, m, at, val);
    if (e == LIGREC_ARGS_OK) e = ligrec_check_pairs(lig, rec, P, G, at, val);
    if (e != LIGREC_ARGS_OK) return e;
    if (!ligrec_threshold_ok(threshold)) return LIGREC_ARGS_THRESHOLD;
    if (batch < 0) { *val = batch; return LIGREC_ARGS_BATCH; }
    if (n != ncol) { *val = n; return LIGREC_ARGS_N; }
    return LIGREC_ARGS_OK;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------
// the most label vectors per wave whose K x vpw double bins fit a wave's LDS share: 64 up to K = 64, 32 up to 128, 16 up to 256
inline int ligrec_vpw_max(int64_t K) {
    for (int v = LIGREC_MAX_VPW; v >= 1; v >>= 1)
        if ((int64_t)v * K * 8 <= LIGREC_WAVE_LDS_BYTES) return v;
    return 0;
}

struct LigrecPlan {
    int path;            // 1 the LDS path, 2 the global path (bins in global scratch)
    int vpw;             // label vectors per wave
    int waves;           // waves per workgroup
    int64_t lds_bytes;   // dynamic LDS of a workgroup of the sums kernel (0 on the global path)
    int64_t batch;       // label vectors per batch
};

// path 0 automatic (the LDS path at every legal K) / 1 the LDS path / 2 the global path; vpw 0: the plan's value, otherwise a
// power of two up to ligrec_vpw_max(K); batch 0: by the budget, a multiple of 64, at least 64.  segs: the segments of the
// listed genes.  LIGREC_ARGS_PATH / _VPW / _BATCH on a knob that is not admissible.
inline LigrecArgError ligrec_plan(int64_t n, int64_t K, int64_t G, int64_t segs, int64_t nvec, int64_t batch, int path, int64_t vpw, LigrecPlan* P,
                                  int64_t* at, int64_t* val) {
    *at = -1;
    *val = 0;
    if (path < 0 || path > 2) { *val = path; return LIGREC_ARGS_PATH; }
    if (batch < 0) { *val = batch; return LIGREC_ARGS_BATCH; }
    const int cap = ligrec_vpw_max(K);
    if (vpw < 0 || vpw > cap || (vpw & (vpw - 1)) != 0) { *at = cap; *val = vpw; return LIGREC_ARGS_VPW; }
    P->path = path == 2 ? 2 : 1;
    P->vpw = vpw > 0 ? (int)vpw : cap;
    const int64_t wave_bytes = (int64_t)P->vpw * K * 8;
    int64_t w = LIGREC_WG_LDS_BYTES / wave_bytes;
    P->waves = (int)(w < 1 ? 1 : (w > LIGREC_MAX_WAVES ? LIGREC_MAX_WAVES : w));
    P->lds_bytes = P->path == 1 ? wave_bytes * P->waves : 0;
    int64_t b = batch;
    if (b == 0) {
        b = LIGREC_BATCH_BYTES / (n + (segs + 2 * G) * K * 8);
        b -= b % LIGREC_MAX_VPW;
        if (b < LIGREC_MAX_VPW) b = LIGREC_MAX_VPW;
    }
    P->batch = b < nvec ? b : nvec;
    return LIGREC_ARGS_OK;
}

// ---- the segments ---------------------------------------------------------------------------------------------------------------
// range[2 g], range[2 g + 1]: the first and one past the last stored entry of listed gene g.  The genes' entries are cut, counted
// from the gene's first entry, into segments of LIGREC_SEG; a gene without entries has none.  seg_first: G + 1 offsets into
// seg_begin / seg_end (the entry ranges of the segments, gene by gene in ascending order).
inline int64_t ligrec_count_segments(const int64_t* range, int64_t G) {
    int64_t s = 0;
    for (int64_t g = 0; g < G; ++g) s += (range[2 * g + 1] - range[2 * g] + LIGREC_SEG - 1) / LIGREC_SEG;
    return s;
}
inline void ligrec_segments(const int64_t* range, int64_t G, std::vector<int64_t>& seg_first, std::vector<int64_t>& seg_begin,
                            std::vector<int64_t>& seg_end) {
    seg_first.assign((size_t)G + 1, 0);
    seg_begin.clear();
    seg_end.clear();
    for (int64_t g = 0; g < G; ++g) {
        for (int64_t e = range[2 * g]; e < range[2 * g + 1]; e += LIGREC_SEG) {
            seg_begin.push_back(e);
            seg_end.push_back(e + LIGREC_SEG < range[2 * g + 1] ? e + LIGREC_SEG : range[2 * g + 1]);
        }
        seg_first[(size_t)g + 1] = (int64_t)seg_begin.size();
    }
}

// ---- the statistics ---------------------------------------------------------------------------------------------------------------
// group_n K; nz G x K (class fastest); n_ge P x K x K at q + P (a + K b).  expressed (G x K bytes), p and padj (P x K x K) may be
// NULL.  per_interaction 0: Benjamini-Hochberg over all P K^2 values that are not NaN; otherwise over the K^2 of every q alone.
inline void ligrec_stats(int64_t K, int64_t G, int64_t P, int64_t nperm, const int64_t* group_n, const int64_t* nz, const int32_t* lig,
                         const int32_t* rec, const int64_t* n_ge, double threshold, int per_interaction, uint8_t* expressed, double* p, double* padj) {
    std::vector<uint8_t> ex((size_t)(G * K));
    for (int64_t g = 0; g < G; ++g)
        for (int64_t c = 0; c < K; ++c)
            ex[(size_t)(g * K + c)] = group_n[c] > 0 && (double)nz[g * K + c] / (double)group_n[c] >= threshold ? 1 : 0;
    if (expressed) std::copy(ex.begin(), ex.end(), expressed);
    if (!p && !padj) return;
    const int64_t KK = K * K, total = P * KK;
    std::vector<double> pv((size_t)total);
    for (int64_t b = 0; b < K; ++b)
        for (int64_t a = 0; a < K; ++a)
            for (int64_t q = 0; q < P; ++q) {
                const int64_t at = q + P * (a + K * b);
                const bool on = ex[(size_t)(lig[q] * K + a)] && ex[(size_t)(rec[q] * K + b)];
                pv[(size_t)at] = on ? (double)(1 + n_ge[at]) / (double)(1 + nperm) : NAN;
            }
    if (p) std::copy(pv.begin(), pv.end(), p);
    if (!padj) return;
    if (!per_interaction) { gsea_bh(pv.data(), total, padj); return; }
    std::vector<double> one((size_t)KK), adj((size_t)KK);
    for (int64_t q = 0; q < P; ++q) {
        for (int64_t t = 0; t < KK; ++t) one[(size_t)t] = pv[(size_t)(q + P * t)];
        gsea_bh(one.data(), KK, adj.data());
        for (int64_t t = 0; t < KK; ++t) padj[q + P * t] = adj[(size_t)t];
    }
}
