/*
 * singlet_hip.h -- C ABI of libsinglet_hip.so, the MI355X (gfx950) engine for
 * singlet's alternating-least-squares hot path.
 *
 * This is the drop-in boundary.  The reference's R wrappers c_nmf / c_ard_nmf /
 * c_project_model (R/RcppExports.R:24-30, 78-80) reach C++ through the Rcpp
 * glue _singlet_c_nmf / _singlet_c_ard_nmf / _singlet_c_project_model
 * (src/RcppExports.cpp:98-116, 284-304, 444-447).  A maintainer replaces the
 * bodies of those three glue functions by calls to section 1 below (stub in
 * INTEGRATION.md); everything R-side stays unchanged.
 *
 * Conventions
 *  - plain C types only; no exceptions cross the ABI.  Every function returns
 *    0 on success or a negative SGL_E* code; sgl_last_error() gives the text
 *    (the R shim turns it into Rf_error, as END_RCPP does for exceptions,
 *    src/RcppExports.cpp:115).
 *  - sparse matrices are dgCMatrix slots (inst/include/singlet.h:36-44):
 *    x double[nnz], i int32[nnz] (row index, ascending within a column),
 *    p int32[ncol+1], Dim = (nrow, ncol).
 *  - dense matrices are column-major doubles exactly as R / Eigen hold them:
 *    w is k x nrow(A), h is k x ncol(A).
 *  - input pointers are never written through nor retained after return;
 *    outputs go to caller-allocated buffers.
 *  - all arithmetic on the path is FP64 on the GPU; there is no CPU fallback:
 *    without a usable gfx950 device every entry point fails with SGL_ENODEV.
 *    The two neighbour-graph entries are the exception, as in the reference:
 *    sgl_c_lknn is FP32 (its distances are floats, returned as doubles),
 *    sgl_c_snn is integer counting with one FP64 quotient per entry, and
 *    sgl_spatial_graph is FP64 as the reference.
 *  - ranks: every entry point takes 1 <= k <= 1024 (SGL_EINVAL above, before anything is uploaded; the
 *    reference's nnls / predict_mask have no limit, src/singlet.cpp:229-250, 436-466).  The tuned kernels cover
 *    k <= 128 (LDS-tiled accumulate, MFMA Grams and Gram downdates, lane NNLS); the plain fit runs ranks 129 - 256 on the
 *    same entry streams, with the Gram on the matrix cores and four lanes per column in the solve (round 6: an iteration
 *    at k = 130 costs 1.3 x one at k = 128); above 256, and for the masked Gram downdate above 128, generic kernels run
 *    (wave-per-column NNLS, VALU Grams in several launches): correct, several times slower.
 *  - device memory: blocks of 64 MB and more that a call frees are kept for the next call (sgl_pool_info,
 *    sgl_cache_release; SGL_POOL=0 switches it off).
 *  - several GPUs: section 2b; the one-shot sgl_c_nmf / sgl_c_ard_nmf honour SINGLET_NGPU.
 */
#ifndef SINGLET_HIP_H
#define SINGLET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGL_API __attribute__((visibility("default")))

#define SGL_OK 0
#define SGL_EINVAL (-1)   /* bad argument */
#define SGL_ENODEV (-2)   /* no HIP device / wrong architecture */
#define SGL_EHIP (-3)     /* a HIP runtime call failed */
#define SGL_ENOMEM (-4)   /* device or host allocation failed */
#define SGL_EINTR (-5)    /* the poll callback asked to stop (Rcpp::checkUserInterrupt) */
#define SGL_ESTATE (-6)   /* call out of order on a context */
#define SGL_ECOMM (-7)    /* the all-reduce callback failed, or RCCL is missing / returned an error */

SGL_API const char* sgl_last_error(void);
/* ABI version of this header; bumped on any signature change. */
SGL_API int sgl_abi_version(void);   /* 2: native multi-GPU section, sgl_nmf_iterate, chunk-list / dense ARD entry points */
/* Number of usable gfx950 devices (0 if none); never fails. */
SGL_API int sgl_device_count(void);

/* Callbacks, all invoked on the calling thread only (as Rprintf and
 * Rcpp::checkUserInterrupt are in the reference, src/singlet.cpp:643-663). */
typedef struct sgl_callbacks {
    void* user;
    /* per-iteration trace line: iter is 1-based as printed by the reference
     * (src/singlet.cpp:661-662, 1115-1127); overfit is NaN where the reference
     * prints "-" or has no such column. */
    void (*log)(void* user, int iter, double tol, double overfit);
    /* return non-zero to abort; polled at the two points where the reference
     * calls Rcpp::checkUserInterrupt() (src/singlet.cpp:652, 663). */
    int (*poll)(void* user);
} sgl_callbacks;

/* ------------------------------------------------------------------------
 * 1. One-shot entry points: exactly what the Rcpp glue binds.
 * ---------------------------------------------------------------------- */

/* c_nmf (src/singlet.cpp:669-672 -> c_nmf_base :638-666).
 * Replaces _singlet_c_nmf (src/RcppExports.cpp:98-116).
 * A is nrow x ncol (genes x cells); At is its transpose (ncol x nrow) as
 * R/run_nmf.R:40 builds it; Atx/Ati/Atp may all be NULL, then the transpose is
 * built on the device.  `threads` and `verbose` are accepted for signature
 * parity (threads is meaningless on the GPU; verbose output goes through
 * cb->log).  w_init: k x nrow.  Outputs: w_out k x nrow, d_out k, h_out k x ncol;
 * *n_iter = iterations run; tol_trace (optional, maxit doubles) = tol per
 * iteration. */
SGL_API int sgl_c_nmf(const double* Ax, const int32_t* Ai, const int32_t* Ap,
              const double* Atx, const int32_t* Ati, const int32_t* Atp,
              int32_t nrow, int32_t ncol,
              double tol, uint16_t maxit, int verbose,
              double L1_w, double L1_h, double L2_w, double L2_h, uint16_t threads,
              const double* w_init, int32_t k,
              double* w_out, double* d_out, double* h_out,
              int32_t* n_iter, double* tol_trace, const sgl_callbacks* cb);

/* Opt-in resident matrix between one-shot calls: with SINGLET_HIP_CACHE=1 in the environment sgl_c_nmf and
 * sgl_c_ard_nmf keep the context of their last call and skip upload / validation / transpose when the next call
 * passes the same host slots (same pointers, shape, non-zero count and a sampled fingerprint of x, i, p) -- the
 * unchanged R drivers' rank sweep (R/ard_nmf.R:95-160, R/cross_validate_nmf.R:69-97) then runs on a resident A.
 * The pointers are compared, never dereferenced later.  Unset (default): every call uploads.
 * sgl_cache_release frees the kept context (and its device memory); call it before unloading the library. */
SGL_API int sgl_cache_release(void);

/* c_ard_nmf (src/singlet.cpp:1155-1159 -> c_ard_nmf_base :1090-1152).
 * Replaces _singlet_c_ard_nmf (src/RcppExports.cpp:284-304).
 * Trace arrays (test_mse, iter, tol, score_overfit) must hold maxit + 1
 * entries; *n_trace receives their used length (the reference returns them as
 * R vectors, src/singlet.cpp:1144-1151).  Ranks as in the header's preamble (k <= 1024). */
SGL_API int sgl_c_ard_nmf(const double* Ax, const int32_t* Ai, const int32_t* Ap,
                  const double* Atx, const int32_t* Ati, const int32_t* Atp,
                  int32_t nrow, int32_t ncol,
                  double tol, uint16_t maxit, int verbose,
                  double L1, double L2, uint16_t threads,
                  const double* w_init, int32_t k,
                  uint64_t seed, uint64_t inv_density, double overfit_threshold, uint16_t trace_test_mse,
                  double* w_out, double* d_out, double* h_out,
                  double* test_mse, int32_t* iter, double* tol_out, double* score_overfit, int32_t* n_trace,
                  const sgl_callbacks* cb);

/* c_nmf_dense (src/singlet.cpp:1052-1054; dense predict :370-381), the branch
 * R/run_nmf.R:57 takes for a dense matrix.  Replaces _singlet_c_nmf_dense
 * (11 args; At is not needed).  A: nrow x ncol column-major doubles.  Unlike the
 * sparse path, all-zero columns are solved too (the dense predict has no
 * empty-column skip). */
SGL_API int sgl_c_nmf_dense(const double* A, int32_t nrow, int32_t ncol,
                    double tol, uint16_t maxit, int verbose,
                    double L1_w, double L1_h, double L2_w, double L2_h, uint16_t threads,
                    const double* w_init, int32_t k,
                    double* w_out, double* d_out, double* h_out,
                    int32_t* n_iter, double* tol_trace, const sgl_callbacks* cb);

/* c_ard_nmf_dense (src/singlet.cpp:1357-1361; dense predict_mask :506-533, mse_test :608-632), the branch
 * R/ard_nmf.R:109 and R/cross_validate_nmf.R:82 take for a dense matrix.  Replaces _singlet_c_ard_nmf_dense
 * (13 args; At is not needed).  Every column is solved, as in sgl_c_nmf_dense. */
SGL_API int sgl_c_ard_nmf_dense(const double* A, int32_t nrow, int32_t ncol,
                        double tol, uint16_t maxit, int verbose,
                        double L1, double L2, uint16_t threads,
                        const double* w_init, int32_t k,
                        uint64_t seed, uint64_t inv_density, double overfit_threshold, uint16_t trace_test_mse,
                        double* w_out, double* d_out, double* h_out,
                        double* test_mse, int32_t* iter, double* tol_out, double* score_overfit, int32_t* n_trace,
                        const sgl_callbacks* cb);

/* c_nmf_sparse_list (src/singlet.cpp:715-743) and c_ard_nmf_sparse_list (:1162-1234): A as a LIST of column
 * chunks (each nrow x chunk_ncol[q], dgCMatrix slots), as R/ard_nmf.R:114,181 passes it; the reference walks
 * the chunks with a running column offset (:384-402, :485, :590).  Replace _singlet_c_nmf_sparse_list (9 args)
 * and _singlet_c_ard_nmf_sparse_list (13 args).  The chunks are joined on the device into one resident matrix
 * (64-bit column pointers: the total may exceed one dgCMatrix's 2^31 - 1 non-zeros).  At_: the list of column
 * chunks of t(A) (each ncol_total x t_chunk_ncol[q]); n_t_chunks = 0 builds the transpose on the device. */
SGL_API int sgl_c_nmf_sparse_list(int32_t n_chunks, const double* const* Ax, const int32_t* const* Ai, const int32_t* const* Ap,
                          const int32_t* chunk_ncol,
                          int32_t n_t_chunks, const double* const* Atx, const int32_t* const* Ati, const int32_t* const* Atp,
                          const int32_t* t_chunk_ncol,
                          int32_t nrow,
                          double tol, uint16_t maxit, int verbose, double L1, double L2, uint16_t threads,
                          const double* w_init, int32_t k,
                          double* w_out, double* d_out, double* h_out,
                          int32_t* n_iter, double* tol_trace, const sgl_callbacks* cb);
SGL_API int sgl_c_ard_nmf_sparse_list(int32_t n_chunks, const double* const* Ax, const int32_t* const* Ai, const int32_t* const* Ap,
                              const int32_t* chunk_ncol,
                              int32_t n_t_chunks, const double* const* Atx, const int32_t* const* Ati, const int32_t* const* Atp,
                              const int32_t* t_chunk_ncol,
                              int32_t nrow,
                              double tol, uint16_t maxit, int verbose, double L1, double L2, uint16_t threads,
                              const double* w_init, int32_t k,
                              uint64_t seed, uint64_t inv_density, double overfit_threshold, uint16_t trace_test_mse,
                              double* w_out, double* d_out, double* h_out,
                              double* test_mse, int32_t* iter, double* tol_out, double* score_overfit, int32_t* n_trace,
                              const sgl_callbacks* cb);

/* c_linked_nmf (src/singlet.cpp:1059-1086; predict_link :416-433), the linked
 * NMF behind R/RunLNMF.R:60.  Replaces _singlet_c_linked_nmf (11 args).  link_h
 * (link_h_rows x link_h_cols, column-major) multiplies the first link_h_rows
 * entries of every cell's right-hand side before its NNLS solve; it is applied
 * iff link_h_cols == ncol (l.1064).  link_w likewise for genes, iff
 * link_w_cols == nrow (l.1065).  Either may be NULL. */
SGL_API int sgl_c_linked_nmf(const double* Ax, const int32_t* Ai, const int32_t* Ap,
                     const double* Atx, const int32_t* Ati, const int32_t* Atp,
                     int32_t nrow, int32_t ncol,
                     double tol, uint16_t maxit, int verbose,
                     double L1, double L2, uint16_t threads,
                     const double* w_init, int32_t k,
                     const double* link_h, int32_t link_h_rows, int32_t link_h_cols,
                     const double* link_w, int32_t link_w_rows, int32_t link_w_cols,
                     double* w_out, double* d_out, double* h_out,
                     int32_t* n_iter, double* tol_trace, const sgl_callbacks* cb);

/* c_gcnmf (src/singlet.cpp:1668-1730; glue src/RcppExports.cpp:399-417), the
 * graph-convolutional NMF behind R/RunGCNMF.R:77.  Replaces _singlet_c_gcnmf
 * (10 args).  G (G_nrow x G_ncol, a dgCMatrix) is the n x n cell graph, n = ncol;
 * it may be asymmetric.  Each iteration: the H side convolves the right-hand
 * sides over G (Bc = B G, l.1684-1688) and solves EVERY cell, empty ones
 * included; the W side forms its right-hand sides from H G (l.1703-1706) with
 * the Gram of the plain scaled H and solves EVERY gene.  At may be NULL (the
 * device transposes).  w_init is w_rows x w_cols column-major, transposed iff
 * w_rows == nrow && w_rows != w_cols (l.1713); k = the factor dimension after
 * that.  Outputs: w_out nrow x k column-major (the reference returns
 * w.transpose()), d_out k, h_out k x ncol, n_iter / tol_trace as sgl_c_nmf.
 * An invalid G (shape, unsorted or out-of-range rows, non-finite values) is
 * SGL_EINVAL. */
SGL_API int sgl_c_gcnmf(const double* Ax, const int32_t* Ai, const int32_t* Ap,
                        const double* Atx, const int32_t* Ati, const int32_t* Atp,
                        int32_t nrow, int32_t ncol,
                        const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t G_nrow, int32_t G_ncol,
                        double tol, uint16_t maxit, int verbose,
                        double L1, double L2, uint16_t threads,
                        const double* w_init, int32_t w_rows, int32_t w_cols, int32_t k,
                        double* w_out, double* d_out, double* h_out,
                        int32_t* n_iter, double* tol_trace, const sgl_callbacks* cb);

/* c_LKNN (src/singlet.cpp:1491-1603; glue _singlet_c_LKNN, 10 args), the local
 * k-nearest-neighbour graph of R/FindLocalNeighbors.R:95.  m is m_rows x m_cols
 * column-major, transposed iff m_cols != m_rows && m_rows == n_coords (l.1492);
 * n = n_coords points.  FP32 throughout: m, the coordinates, radius and
 * max_dist are rounded to float once.  For each point, the other points with
 * sqrt(dx*dx + dy*dy) <= radius (float, l.1520-1523) get a distance in the
 * embedding ("jaccard", "cosine", "manhattan", "hamming", "kl", anything else
 * euclidean; l.1426-1478, in dimension order, no FMA, quirks kept); those with
 * max_dist != 0 && d > max_dist are dropped; of more than k, the k smallest
 * are kept.  Ranking is by (distance, index): ties at the cut go to the lower
 * index and NaN distances rank after every number (this build's rule; the
 * reference's std::sort leaves both unspecified).  Zero distances (+-0) are
 * dropped AFTER the selection (l.1572-1588).  Output: the n x n dgCMatrix,
 * column j = the neighbours of point j, rows ascending, x = the distances.
 * Refused (SGL_EINVAL, with a message): the reference's two stop()s, k < 0,
 * non-finite m or coordinates, a negative or non-finite radius, and a point
 * that keeps more than ceil((2 radius + 1)^2) - 1 neighbours (the slots per
 * point the reference allocates, l.1496: it would overwrite the next point's).
 * Two-call contract: with i_out / x_out NULL, fills p_out (n + 1) and *nnz_out;
 * with buffers of cap >= nnz, fills them too; cap < nnz is SGL_EINVAL.  The
 * result is deterministic, bit for bit. */
SGL_API int sgl_c_lknn(const double* m, int32_t m_rows, int32_t m_cols,
                       const double* coord_x, const double* coord_y, int32_t n_coords,
                       int64_t k, double radius, const char* metric, int similarity, double max_dist,
                       int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap);

/* c_SNN (src/singlet.cpp:1606-1665; glue _singlet_c_SNN, 3 args), the shared
 * nearest-neighbour graph of R/FindLocalNeighbors.R:98.  Only G's pattern is
 * read (G_nrow x G_ncol, any shape).  Output: the G_ncol x G_ncol dgCMatrix
 * whose column i, for nnz_i > 0, holds (i, i) = 1 and every j != i whose row
 * sets meet with sim = inter / (nnz_i + nnz_j - inter) > min_similarity (FP64,
 * strict); empty columns stay empty; rows ascend.  Unsorted or out-of-range
 * rows of G are SGL_EINVAL, and so is an output of 2^31 entries or more
 * (refused after the count pass, before anything is allocated for it).  Same
 * two-call contract as sgl_c_lknn; deterministic. */
SGL_API int sgl_c_snn(const int32_t* Gi, const int32_t* Gp, int32_t G_nrow, int32_t G_ncol,
                      double min_similarity,
                      int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap);

/* spatial_graph (src/singlet.cpp:1365-1414; glue _singlet_spatial_graph, 5
 * args), the distance-weighted cell graph that GCNMF convolves with.  n points
 * (c1[e], c2[e]), FP64.  For each point i the points j = 0, 1, ... are scanned
 * in INDEX order and j is kept when d = sqrt((c1[i]-c1[j])^2 + (c2[i]-c2[j])^2)
 * < max_dist (double, strict, no contraction), until max_k are kept: the
 * selection is by index, not by distance, and i itself (d = 0) is kept when it
 * falls among the first max_k.  Weight (max_dist - d) * scale, scale =
 * 1 / max_dist rounded once (the reference's product and reciprocal); each
 * column divided by its sum.  Output: the n x n dgCMatrix, column i = the
 * points kept by i, rows ascending.  This build's rules where the reference is
 * undefined or unsound:
 *  - refused (SGL_EINVAL, with a message): a non-finite coordinate (the
 *    reference writes max_k NaN entries of row 0), max_dist not finite and > 0
 *    or 1 / max_dist not finite (NaN columns), max_k < 0, and an output of 2^31
 *    entries or more (refused after the count pass, before anything is
 *    allocated for it).  c1 and c2 of different lengths (the reference reads
 *    past c2) are refused by the Python and R layers, which see both lengths.
 *    With these refused every column holds at least its own point and a sum
 *    > 0, and no weight is 0, so every kept point is an entry.
 *  - max_k = 0 and n = 0 give the empty n x n graph (p all 0); max_k > n acts
 *    as n, and nothing of max_k x n is ever allocated.
 *  - the column sum is sequential, in ascending row order (the reference's
 *    Eigen sum() is a vectorised reduction whose order depends on the Eigen
 *    version, the SIMD width and the column's alignment).
 *  - bit-exact: the pattern (p, i) and the weights before the division; the
 *    normalised x with the sequential sum above, and within max_k ulps
 *    (relative) of any other summation order.  Deterministic, bit for bit.
 * Same two-call contract as sgl_c_lknn.  One device: the current one. */
SGL_API int sgl_spatial_graph(const double* c1, const double* c2, int32_t n, double max_dist, int64_t max_k,
                              int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap);

/* c_project_model (src/singlet.cpp:405-413).
 * Replaces _singlet_c_project_model (src/RcppExports.cpp:444-447 region).
 * w is w_rows x w_cols column-major; if w_rows == nrow it is transposed first
 * (l.406).  k = the factor dimension after that.  h_out: k x ncol, d_out: k. */
SGL_API int sgl_c_project_model(const double* Ax, const int32_t* Ai, const int32_t* Ap,
                        int32_t nrow, int32_t ncol,
                        const double* w, int32_t w_rows, int32_t w_cols,
                        double L1, double L2, uint16_t threads,
                        double* h_out, double* d_out);

/* Rcpp_predict (src/singlet.cpp:350-367): the projection without the two
 * scale() calls.  Replaces _singlet_Rcpp_predict (src/RcppExports.cpp, 5 args,
 * registered at :462).  w is transposed iff w_rows == nrow && w_cols != nrow
 * (l.351 -- not the same rule as c_project_model's).  h_out: k x ncol. */
SGL_API int sgl_rcpp_predict(const double* Ax, const int32_t* Ai, const int32_t* Ap,
                             int32_t nrow, int32_t ncol,
                             const double* w, int32_t w_rows, int32_t w_cols,
                             double L1, double L2, uint16_t threads, double* h_out);

/* ------------------------------------------------------------------------
 * 2. Context API: the same path with the matrix kept resident in HBM, for
 *    rank sweeps (R/ard_nmf.R:95-160 calls c_ard_nmf many times on one A),
 *    for cell-sharded multi-GPU runs and for the benchmark.  One context =
 *    one device = one shard of cells.
 * ---------------------------------------------------------------------- */
typedef struct sgl_ctx sgl_ctx;

SGL_API int sgl_create(int device, sgl_ctx** out);
SGL_API int sgl_destroy(sgl_ctx* ctx);
/* Launch all work of this context on `hip_stream` (a hipStream_t; NULL = the
 * context's own stream).  Lets a host that owns a stream (torch's current
 * stream) order collectives against the kernels without host syncs.
 * Handle 0 / NULL = the private stream: the null stream (torch's default
 * stream) cannot be chosen, and the private stream is created non-blocking,
 * so it is not ordered against the null stream either.  A hook on the private
 * stream must have finished its writes when it returns (sgl_allreduce_fn). */
SGL_API int sgl_set_stream(sgl_ctx* ctx, void* hip_stream);

/* Upload a shard: columns [cell_offset, cell_offset + ncol) of a genes x
 * ncells_total matrix.  At describes the same shard transposed (ncol x nrow,
 * row indices local to the shard); pass NULLs to have it built on the device.
 * Replaces the Rcpp::SparseMatrix views (inst/include/singlet.h:108-127).
 * A refused or failed upload (any of the sgl_upload_* entries) leaves NO matrix
 * resident, the previous one included: sgl_dims reports 0 / 0 / 0. */
SGL_API int sgl_upload_csc(sgl_ctx* ctx, const double* Ax, const int32_t* Ai, const int32_t* Ap,
                   const double* Atx, const int32_t* Ati, const int32_t* Atp,
                   int32_t nrow, int32_t ncol, int64_t cell_offset, int64_t ncells_total);

/* The same from a list of column chunks (sgl_c_nmf_sparse_list above): the chunks become ONE resident shard. */
SGL_API int sgl_upload_csc_list(sgl_ctx* ctx, int32_t n_chunks, const double* const* Ax, const int32_t* const* Ai,
                        const int32_t* const* Ap, const int32_t* chunk_ncol,
                        int32_t n_t_chunks, const double* const* Atx, const int32_t* const* Ati, const int32_t* const* Atp,
                        const int32_t* t_chunk_ncol,
                        int32_t nrow, int64_t cell_offset, int64_t ncells_total);

/* The arrays of a SciPy / AnnData / torch CSR or CSC as the caller holds them: n_major + 1 offsets, and per stored entry
 * an index below n_minor and a value.  On success the context holds exactly what sgl_upload_csc(ctx, x64, i32, p32,
 * NULL...) leaves for the same matrix converted, sorted and (major_is_genes = 1) transposed on the host, bit for bit:
 *  - major_is_genes = 0: a major slice is a cell; the arrays are the CSC of A (= the CSR of t(A)) and fill A, t(A) is
 *    its device transpose.  major_is_genes = 1: a major slice is a gene; the arrays are the CSC of t(A) (= the CSR of A)
 *    and fill t(A), A is its device transpose.  A is n_minor x n_major or n_major x n_minor accordingly.
 *  - values: F32 and I32 widen exactly; an I64 beyond +-2^53 is refused ("inexact"); NaN / Inf is refused like at every
 *    door; explicit zeros stay stored.
 *  - indices: an I64 index is range-checked as a 64-bit number before it is narrowed (2^32 + 3 is out of range, never
 *    row 3).
 *  - offsets: ptr[0] == 0, non-decreasing; ptr[n_major] is the entry count (above 2^31 - 1 is legal with I64 offsets).
 *    HOST space: checked on the host.  DEVICE space: checked by a kernel, the count read back; the host never
 *    dereferences a device pointer.
 *  - order: without SGL_UP_SORT a slice whose indices are not strictly ascending is refused.  With it the (index, value)
 *    pairs of every slice that is out of order -- and of no other -- are sorted by index on the device; two equal
 *    indices in one slice are refused either way (duplicate entries are not summed).
 *  - space: HOST arrays are pageable host memory, copied once each.  DEVICE arrays must be device memory of the
 *    context's device (hipPointerGetAttributes, asked for all three before any copy; SGL_EINVAL otherwise); they are
 *    read on the context's stream and not retained, and the caller guarantees that their producer has finished.
 *  - n_major / n_minor outside [1, 2^31 - 1], an unknown type code, space, flag bit or major_is_genes: SGL_EINVAL before
 *    anything is allocated.  Every refusal or failure leaves NO matrix resident.
 *  - report (NULL or 8 values, written on success): [0] entries, [1] slices sorted in LDS, [2] slices sorted by the long
 *    path, [3] 1 if every stored value equals its truncation, [4] bytes read from the caller's arrays, [5] the LDS
 *    sort's capacity in entries, [6], [7] 0. */
#define SGL_T_F64 0
#define SGL_T_F32 1
#define SGL_T_I32 2
#define SGL_T_I64 3
#define SGL_SPACE_HOST 0
#define SGL_SPACE_DEVICE 1
#define SGL_UP_SORT 1u        /* indices of a major slice may come in any order: sorted on the device */
SGL_API int sgl_upload_typed(sgl_ctx* ctx, const void* x, int x_type, const void* idx, int idx_type,
                     const void* ptr, int ptr_type, int64_t n_major, int64_t n_minor, int major_is_genes,
                     int space, uint32_t flags, int64_t cell_offset, int64_t ncells_total, int64_t* report);

/* Host only (no device): the batches of sgl_upload_typed's long sort path.  The n slices of len[s] >= 0 entries are cut,
 * in order, into runs [cut[b], cut[b + 1]) of whole slices whose entries sum to at most max_entries >= 1 (a longer
 * slice is a run of its own); cut has room for n + 1 values, *n_runs receives the number of runs. */
SGL_API int sgl_ingest_batch_edges(const int64_t* len, int64_t n, int64_t max_entries, int64_t* cut, int64_t* n_runs);

/* A dense matrix (nrow x ncol, column-major doubles, as R / Eigen hold it; what c_nmf_dense and c_ard_nmf_dense take,
 * src/singlet.cpp:1052-1054, 1357-1361): resident as its CSC image (zeros dropped, both orientations, built on the
 * device) and -- when more than half of its entries are non-zero -- as the dense copy itself, on which the plain fit then
 * forms the right-hand sides of predict (`w * A.col(i)`, src/singlet.cpp:377) as FP64 GEMMs (rocBLAS, bound at run time).
 * A fit on it solves every column like the reference's dense predict (no empty-column skip) when the caller asks for it
 * (sgl_c_nmf_dense does). */
SGL_API int sgl_upload_dense(sgl_ctx* ctx, const double* A, int32_t nrow, int32_t ncol);

/* Generate the synthetic benchmark shard on the device:
 * entry (gene g, cell c) non-zero iff rand_S(c,g) % inv_density == 0, value
 * levels16[(rand_{S+1}(c,g) >> 11) % 16].  Both orientations are produced. */
SGL_API int sgl_synth_csc(sgl_ctx* ctx, uint64_t S, uint64_t inv_density, const double* levels16,
                  int32_t ngenes, int64_t cell_offset, int32_t ncells_local, int64_t ncells_total);
/* The same with SKEWED rows and columns (a benchmark matrix nearer to count data than the i.i.d. one; the
 * reference's own fixture pbmc3k has 3 ... 2700 non-zeros per gene): entry (g, c) is non-zero iff
 * u(c, g) < cell_w16[level(c)] * gene_w16[level(g)] / inv_density, u = (rand_S(c, g) >> 11) * 2^-53, the levels
 * 4-bit hashes of the cell / gene index alone.  Both tables NULL = sgl_synth_csc. */
SGL_API int sgl_synth_csc_skewed(sgl_ctx* ctx, uint64_t S, uint64_t inv_density, const double* levels16,
                  int32_t ngenes, int64_t cell_offset, int32_t ncells_local, int64_t ncells_total,
                  const double* cell_w16, const double* gene_w16);

/* Shape / size queries. */
SGL_API int sgl_dims(const sgl_ctx* ctx, int32_t* nrow, int32_t* ncol, int64_t* nnz);
/* Download the resident shard as dgCMatrix slots (tests of sgl_synth_csc and
 * of the device transpose).  which = 0: A, 1: At.  Buffers sized from sgl_dims. */
SGL_API int sgl_download_csc(sgl_ctx* ctx, int which, double* x, int32_t* i, int64_t* p);

/* Input staging on the resident shard, applied to A and its transpose in place
 * (call before sgl_fit_init; a running fit is dropped).
 * sgl_log_normalize: Seurat::LogNormalize as PreprocessData.dgCMatrix applies
 *   it (R/PreprocessData.R:34-39): x <- log1p(x / colSums(A)[cell] * scale_factor).
 * sgl_weight_by_split: weight_by_split (src/singlet.cpp:119-144): split_by[c] in
 *   [0, n_groups) is the group of local cell c; cells of group g != 0 are divided
 *   by (sum of group g) / (sum of group 0).  Group sums are global over shards
 *   (all-reduce hook). */
SGL_API int sgl_log_normalize(sgl_ctx* ctx, double scale_factor);
SGL_API int sgl_weight_by_split(sgl_ctx* ctx, const int32_t* split_by, int32_t n_groups);
/* The one-shot form the Rcpp glue binds (`_singlet_weight_by_split`, src/RcppExports.cpp:17-27, 445; called from
 * R/RunNMF.R:86-93): dgCMatrix slots in, the re-weighted values out.  x_out (nnz doubles) may be the x slot itself:
 * the reference rewrites the values of A in place (src/singlet.cpp:136-141). */
SGL_API int sgl_c_weight_by_split(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol,
                                  const int32_t* split_by, int32_t n_groups, double* x_out);

/* Row-wise rasterisation: rowwise_compress_sparse / rowwise_compress_dense (src/singlet.cpp:146-180; glue
 * _singlet_rowwise_compress_sparse / _dense, 3 args, src/RcppExports.cpp:446-447), which RasterizeRowwise
 * (R/rasterize_rowwise.R) calls for a dgCMatrix / anything else.  This build's rules:
 *  - out is floor(nrow / n) x ncol, column-major doubles.  Entry (b, j) = (sum over r in [b n, b n + n) of A[r, j]) / n:
 *    the sum in ascending r starting from +0.0, without contraction, then one true division by (double)n (a product
 *    with 1 / n gives other bits).  Bit-exact with the reference wherever it is defined (nrow % n == 0, n >= 1), and the
 *    sparse and dense forms of one matrix give the same bits: skipped zeros are additions of +0.0, which change no sum
 *    that starts at +0.0 (it is never -0.0).
 *  - the last nrow mod n rows are left out (their entries have no effect): the shape both references allocate and the
 *    row names the R wrapper assigns.  The reference is undefined there: the sparse form adds those entries to res(0,
 *    col + 1) -- the next column's first bin, racing with its thread, or past the result for the last column -- and the
 *    dense form reads past the column and writes the same alias.
 *  - n < 1 is refused (SGL_EINVAL, with a message; the reference divides by zero, and a negative n from R becomes a huge
 *    size_t): the R and Python layers refuse NA and truncate a fractional n toward zero as Rcpp's as<size_t> does.
 *    n > nrow gives the 0 x ncol result (nothing written).
 *  - values are not checked for finiteness (unlike the fit uploads): NaN / Inf propagate through the IEEE sums as in
 *    the reference.  The structure of the sparse form is validated (row indices in [0, nrow), strictly ascending
 *    within a column, p non-decreasing from 0): an invalid dgCMatrix is SGL_EINVAL with a message.
 *  - 64-bit indexing throughout: the result and a dense input may exceed 2^31 elements.  threads is the caller's to ignore.
 * One-shot entries: their own context on the current device, out sized floor(nrow / n) * ncol; neither uses nor touches
 * the SINGLET_HIP_CACHE context.  The dense form copies the matrix to the device as it is (no CSC image). */
SGL_API int sgl_c_rowwise_compress_sparse(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol,
                                          int64_t n, double* out);
SGL_API int sgl_c_rowwise_compress_dense(const double* A, int32_t nrow, int32_t ncol, int64_t n, double* out);
/* The resident form: the context's matrix (its CSC image A, from any upload, synth or staging step) is replaced by its
 * rasterisation, resident exactly as if sgl_upload_dense had received it (CSC image and transpose built on the device,
 * the dense copy kept when more than half of it is non-zero).  A running fit is dropped.  Refused, with the matrix kept:
 * SGL_ESTATE on a team member or with an all-reduce hook set (the gene-side images would differ across shards) or with
 * no matrix resident; SGL_EINVAL for n < 1 or n > nrow (a resident matrix cannot be empty).  A non-finite result (a
 * sum that overflows) is refused like sgl_upload_dense refuses one, and then no matrix stays resident. */
SGL_API int sgl_rasterize_rowwise(sgl_ctx* ctx, int64_t n);

/* Subset of the resident matrix by features and cells: R's A[features, ] of RunNMF.Seurat (R/RunNMF.R:72-81, after the
 * normalisation, before weight_by_split) and the gene alignment of ProjectData.Seurat (R/ProjectData.R:68-69), without
 * the matrix leaving the device.  The resident A (nrow x ncol) is replaced by A' with A'[r', c'] = A[rows[r'], cols[c']]:
 *  - indices are 0-based, in any order, duplicates allowed (R's A[c(3, 1, 3), ]).  rows == NULL keeps all rows (n_rows is
 *    ignored), cols == NULL all columns (n_cols is ignored); both NULL is a no-op that still drops a running fit.
 *  - data movement only: the stored values move bit for bit, explicit zeros stay stored, nothing is validated for
 *    finiteness again.  Both orientations end up exactly as sgl_upload_csc(..., At = NULL) leaves the host-side subset:
 *    row indices strictly ascending within every column of A' and of t(A'), 64-bit offsets.  (A column gather of one
 *    orientation -- cols on A, rows on t(A) -- and the device transpose for the other: one transpose for one list, two
 *    for both.  The old images are freed before the transpose allocates.)
 *  - afterwards: a running fit is dropped, and with it the entry streams, mask lists, graph, links and tiling segments,
 *    as when the matrix changes by any other door; the per-column counts are those of A'; cell_offset = 0 and
 *    ncells_total = the new ncol.  A dense copy kept by sgl_upload_dense is released (as sgl_log_normalize releases it);
 *    the matrix still counts as dense input, so sgl_set_graph stays refused.  A result without a stored entry is
 *    resident like the empty-but-shaped matrix sgl_upload_csc accepts.
 *  - refused with the matrix and a running fit untouched: SGL_ESTATE with no matrix resident, on a team member or with
 *    an all-reduce hook set (the gene-side images would differ across shards), or on a context that holds a shard
 *    (cell_offset != 0 or ncells_total != ncol); SGL_EINVAL for a non-NULL list with n == 0 (a resident matrix cannot be
 *    empty) or n > INT32_MAX, and for an index outside [0, nrow) / [0, ncol) -- the message names the list, the
 *    position and the value of the first offender.  Both lists are checked completely before anything is freed.
 *  - after that only an allocation or a HIP call can fail, and then no matrix stays resident (sgl_dims: 0 / 0 / 0), as
 *    after a failed upload. */
SGL_API int sgl_subset(sgl_ctx* ctx, const int32_t* rows, int64_t n_rows, const int32_t* cols, int64_t n_cols);

/* Simulated doublets: the first step of every doublet detector of the Scrublet kind (Wolock, Lopez & Klein 2019; also
 * DoubletFinder, scDblFinder) -- artificial doublets as the sums of the raw counts of pairs of cells -- made on the device
 * from the resident counts, so that no matrix of two or three times the original's size is merged on the host and
 * uploaded.  The reference's package has no such function; the rules below are this library's own, in full;
 * tests/doublet_restatement.py restates them in numpy.  The simulation needs COUNTS, and sgl_log_normalize rewrites the
 * matrix in place, so the call reads one context and writes another.
 *
 * sgl_simulate_doublets: the resident matrix of dst becomes S, nrow x n_sim, S[:, s] = A[:, parent_a[s]] + A[:, parent_b[s]],
 * A the resident CSC image of src, which is only read.
 *  - stored rows: the stored rows of column s are the union of the two parents' stored rows, ascending.  A row stored in
 *    one parent carries that value's bits; a row stored in both carries x_a + x_b, ONE IEEE addition (commutative: the order
 *    of the parents changes nothing).  An explicit zero stays stored; a sum that cancels stays stored as the zero it rounds
 *    to.  parent_a[s] == parent_b[s] is allowed and gives 2 x.  Parents may repeat and come in any order.
 *  - the image: dst ends up exactly as sgl_upload_csc(dst, S, At = NULL) would leave it -- both orientations, the
 *    transposed one through the device transpose, 64-bit offsets, cell_offset = 0, ncells_total = n_sim.  A fit of dst and
 *    everything that hangs on its matrix (entry streams, mask lists, graph, links, a dense copy) is dropped, as by any
 *    other door.  src keeps its matrix, its fit and its bits.
 *  - a non-finite sum (an overflow: the parents' values are finite) is refused as sgl_rasterize_rowwise refuses one:
 *    SGL_EINVAL, dst is left without a matrix, and the message names the lowest simulated column that holds one.
 *  - device and streams: both contexts must be on one device.  The kernels run on dst's stream.  First dst's stream waits
 *    for an event recorded on src's stream (what src still has queued -- a sgl_log_normalize, a sgl_synth_csc -- ends
 *    before its matrix is read); at the end src's stream waits for an event recorded on dst's stream, so a
 *    sgl_log_normalize of src issued right after cannot overtake the read.  The call returns with dst's stream
 *    synchronised (it needs the entry count of S on the host), on the private stream and on a caller's.
 *  - refused with BOTH contexts untouched: SGL_ESTATE for src == dst, src without a matrix, either context a member of a
 *    team or with an all-reduce hook, either context holding a shard (cell_offset != 0 or ncells_total != ncol);
 *    SGL_EINVAL for contexts on different devices, n_sim < 1 or > INT32_MAX, a NULL list, a parent outside [0, ncol) --
 *    the message names the list, the position and the value of the first offender (position by position, parent_a before
 *    parent_b).  The lists are checked completely before anything is freed.
 *  - after that only an allocation or a HIP call can fail, and then dst holds no matrix (sgl_dims: 0 / 0 / 0), as after a
 *    failed upload.
 *  - paths: one wave per simulated column, no sort, no atomics on the data, vector stores only.  Entry j of a parent
 *    goes to slot j + (entries of the other parent below its row) - (rows among them stored in both); the a-side writes
 *    the sum at a shared row, the b-side skips it.  A pair whose la + lb row indices fit 4096 is staged in LDS and
 *    searched there (the LDS path), a longer one (a dense upload has columns of nrow entries) is searched in global
 *    memory (the long path).  Both give the same bits.
 *  - there is NO team form and NO R shim entry. */
SGL_API int sgl_simulate_doublets(sgl_ctx* src, sgl_ctx* dst, const int32_t* parent_a, const int32_t* parent_b, int64_t n_sim);
/* What the last sgl_simulate_doublets INTO this context, or the last sgl_op_pair_columns on it, ran: out[0] the pairs merged
 * on the LDS path, out[1] on the long path, out[2] the stored entries of S, out[3] the rows stored in both parents, summed
 * over the pairs (out[2] + out[3] = the parents' entries together). */
SGL_API int sgl_doublets_info(sgl_ctx* ctx, int64_t out[4]);

/* Spatial autocorrelation: Moran's I of the genes of the resident matrix and of the rows of an embedding over a sparse
 * n x n cell graph G (weights w_ij = G[i, j]), the question Seurat asks with FindSpatiallyVariableFeatures(selection.method =
 * "moransi") and squidpy with spatial_autocorr.  The rules below are this library's own statement of the published
 * definitions (Cliff & Ord 1981; the randomisation variance as ape::Moran.I writes it); tests/moran_restatement.py restates
 * them in numpy.  NO parity run against ape, Seurat or squidpy is claimed.  The statistic needs the stored entries only:
 *     sum_ij w_ij (x_i - m)(x_j - m) = P - m sum_i x_i t_i + m^2 S0,
 *     P = sum over the stored j of x_j * (sum over the stored rows r of column j of G that the gene stores of w_rj x_r),
 *     t_i = rowsum_i + colsum_i,
 * so a gene costs its stored entries times the graph degree, never n^2.
 *
 * Graph: Gx / Gi / Gp, an n x n dgCMatrix, n = the cells, checked as sgl_set_graph checks its graph (finite weights, rows
 * strictly ascending within a column).  It may be asymmetric, may carry a diagonal and negative weights, and is used as
 * given (the Python front-end strips the diagonal by default).  It is uploaded per call, with 64-bit offsets.
 *
 * Graph moments (sgl_moran_graph_moments; host code, O(nnz(G)), once per call; all sums sequential, in double, no product
 * contracted into an addition):
 *  - S0 = the sum of w in stored order, one chain over the columns ascending;
 *  - colsum_j sequential in stored order; rowsum_i through a counting transpose, i.e. sequential over ascending column
 *    index; t_i = rowsum_i + colsum_i; S2 = the sum of t_i * t_i over ascending i;
 *  - S1 = 0.5 * the sum over the union pattern of (w_ij + w_ji)^2, walked by merging column j of G with column j of t(G),
 *    j ascending, rows ascending, an absent partner counting as +0.0 (an off-diagonal pair is met twice, once in each
 *    column, a diagonal entry once as (2 w_jj)^2);
 *  - S0 == 0 or a moment that is not finite: SGL_EINVAL.
 *
 * Per-gene moments, on the device over t(A), with sgl_op_gene_mean's conventions (c_g stored entries, an explicit zero is a
 * stored entry, double, no contraction, no floating-point atomics, no trip count that follows the launch):
 *  - mean_g = sgl_op_gene_mean's value (its kernel runs);
 *  - M2_g = Q2 + (double)(n - c_g) * (m * m), Q2 = sum d * d, d = x - m;
 *  - M4_g = Q4 + (double)(n - c_g) * ((m * m) * (m * m)), Q4 = sum (d * d) * (d * d);
 *  - T_g = sum x * t[cell];
 *  - Q2, Q4, T in the summation order of sgl_variable_features: segments of 8192 stored entries, lane l of 64 adds the
 *    segment's entries l, l + 64, ... from +0.0, the butterfly (lane ^ 32, 16, 8, 4, 2, 1), the segment sums ascending from
 *    +0.0.  One pass produces all three.
 *
 * Cross term P_g: for the entry at stored position e (cell j, value x_j), q_e = the sum from +0.0, over column j of G in
 * stored order, of w * x_r for the rows r that are stored entries of gene g (an absent r contributes nothing), and
 * p_e = x_j * q_e.  P_g = the sum of the p_e in the block order of sgl_gene_group_moments' E[g]: segments of 8192, blocks of
 * 64, a lane past the end holds +0.0, ONE butterfly per block, block sums ascending from +0.0 within a segment, segment sums
 * ascending from +0.0.  P_g is a function of (the gene's entries, G) alone: the path, the batching, the grid and the genes
 * processed before it change no bit.
 *  - search path (a gene of at most lds_cap entries; default and largest 5120: 12 bytes per entry + the block sums, 62 080
 *    bytes, so that two workgroups share the 160 KB of a CU): one workgroup per gene, the gene's ascending cells and its
 *    values staged in LDS, every lane owns an entry, walks its cell's column of G and finds each neighbour by binary search;
 *  - table path (a longer gene): a batch of B genes scatters its values into a B x n table in global memory, one wave per
 *    segment reads the neighbours straight from the table, the table is cleared by walking the entries again.  B is a quarter
 *    of the free memory / 8 n bytes, at most 4096, at most the genes on this path.  The table is a PLAIN VALUE table on a
 *    +0.0 background: an absent neighbour adds w * +0.0 = +-0.0 to q_e, and q_e, a sum that starts at +0.0, is never -0.0,
 *    so adding +-0.0 changes no bit; the values are finite (every upload refuses others), so no NaN arises from it.
 *  - hub columns of G are walked sequentially by their lane: the stated order demands it.
 *
 * Assembly (sgl_moran_stats; host code), nn = (double)n:
 *  - C = (P - m * T) + (m * m) * S0;  I = (nn / S0) * (C / M2);  EI = -1 / (double)(n - 1);
 *  - variance 1 "normality": V = ((nn * nn) * S1 - nn * S2 + 3 * (S0 * S0)) / (((nn * nn) - 1) * (S0 * S0)) - EI * EI;
 *  - variance 0 "randomisation" (ape's): b2 = (nn * M4) / (M2 * M2),
 *    V = (nn * (((nn * nn) - 3 * nn + 3) * S1 - nn * S2 + 3 * (S0 * S0)) - b2 * ((nn * (nn - 1)) * S1 - (2 * nn) * S2 + 6 * (S0 * S0)))
 *        / (((nn - 1) * (nn - 2) * (nn - 3)) * (S0 * S0)) - EI * EI;
 *  - sd = sqrt(V); z = (I - EI) / sd; p by alternative 0 "two.sided": erfc(|z| / sqrt 2), 1 "greater": 0.5 erfc(z / sqrt 2),
 *    2 "less": 0.5 erfc(-z / sqrt 2);
 *  - a constant row (M2 == 0) gives NaN for I, z and p: reported, not refused; p_adj is Benjamini-Hochberg over the rows
 *    whose p is not NaN (the host code of the annotation); n < 4 is refused.
 *  - cancellation: C is the difference of terms of the size of m^2 S0; for a dense, nearly constant gene its relative
 *    error grows as m^2 / var(x) ("Spatial autocorrelation").
 *
 * sgl_moran: over the resident matrix; genes NULL for all genes, or n_genes distinct 0-based gene indices; moments_out
 * 6 x n_genes column-major: mean, M2, M4, T, P, (double)c_g, in list order.  The call only reads: the matrix and a fit in
 * progress are untouched.  Time counts in the "scale" phase; all work goes to the context's stream (sgl_set_stream), which
 * is synchronised before the call returns.  After sgl_upload_dense it works over the CSC image.  64-bit entry indexing.
 *  - SGL_EINVAL, the whole list checked before anything is uploaded: a NULL or bad graph, n != ncol, n < 4, a gene index out
 *    of range or repeated (the message names the position and the value), S0 == 0.
 *  - SGL_ESTATE: no matrix resident, a team member, an all-reduce hook, a shard.
 * sgl_c_moran: the one-shot form, A and G from the host, in a context of its own.
 *
 * Embedding form (sgl_moran_embedding): F is k x n column-major on the host, or NULL for the embedding held by
 * sgl_annotate_hold or else the H of the fit (sgl_group_moments' conventions; 1 <= k <= 1024).  Dense, so the centred form
 * directly: m_f = the sum of F[f, :] in sgl_group_means' order over all cells (chunks of 256 ascending cells, slot s of
 * S = 256 / min(64, k rounded up to a power of two) adds the positions s, s + S, ..., the binary tree over the slots, the
 * chunk sums ascending from +0.0) / (double)n; z_j = F[f, j] - m_f; y_j = the sequential stored-order sum from +0.0 over
 * column j of G of w * z_r; C = sum z_j * y_j, M2 = sum z_j * z_j, M4 = sum (z_j * z_j) * (z_j * z_j), each in that same
 * order over all cells.  moments_out is 6 x k in sgl_moran_stats' layout with the rows ALREADY centred: +0.0, M2, M4, +0.0,
 * C, (double)n (the assembly then gives C back unchanged); mean_out (k values) holds m_f.  Either may be NULL.
 * The fit is only read: continued afterwards it gives the bits it would have given without the call.
 * There is NO team form and NO R shim entry; permutation p-values, Geary's C and local Moran are not provided. */
SGL_API int sgl_moran(sgl_ctx* ctx, const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const int32_t* genes, int64_t n_genes,
                      double* moments_out);
SGL_API int sgl_c_moran(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol, const double* Gx, const int32_t* Gi,
                        const int32_t* Gp, int32_t n, const int32_t* genes, int64_t n_genes, double* moments_out);
SGL_API int sgl_moran_embedding(sgl_ctx* ctx, const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* F, int32_t k,
                                double* moments_out, double* mean_out);
SGL_API int sgl_c_moran_embedding(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* F, int32_t k,
                                  double* moments_out, double* mean_out);
/* Host only, no device: the graph moments (t: n values, may be NULL) and the assembly (any output may be NULL). */
SGL_API int sgl_moran_graph_moments(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, double* S0, double* S1, double* S2,
                                    double* t);
SGL_API int sgl_moran_stats(int64_t n, double S0, double S1, double S2, int64_t rows, const double* moments, int variance, int alternative,
                            double* I, double* EI, double* sd, double* z, double* p, double* p_adj);
/* The cross term alone (P_out: n_genes values in list order); the refusals of sgl_moran apply, but a graph without weight is
 * accepted.  path 0 automatic, 1 forces the search path (a gene above 5120 entries still takes the table), 2 forces the table
 * path; lds_cap 0 the default, otherwise a smaller capacity in entries; table_batch 0 the default B, otherwise B itself.
 * The result does not depend on any of them. */
SGL_API int sgl_op_moran_cross(sgl_ctx* ctx, const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const int32_t* genes,
                               int64_t n_genes, int32_t path, int64_t lds_cap, int64_t table_batch, double* P_out);
/* What the last sgl_moran / sgl_op_moran_cross on this context ran: out[0] the genes on the search path, out[1] on the table
 * path, out[2] the table batches, out[3] the table batch B, out[4] the table's bytes, out[5] the LDS cap in force. */
SGL_API int sgl_moran_info(sgl_ctx* ctx, int64_t out[6]);

/* Neighbourhood enrichment: which classes of cells (clusters) sit next to which on a cell graph, more or less often than under
 * a random relabelling -- the permutation test squidpy calls gr.nhood_enrichment / gr.interaction_matrix and Giotto
 * cellProximityEnrichment.  The rules below are this library's own statement of the published scheme;
 * tests/nhood_restatement.py restates them in numpy.  NO parity with squidpy's seeded numpy shuffles (or with Giotto) is claimed:
 * the permutations are this library's.  Everything the device computes is an integer, so every result is one function of the
 * inputs, bit for bit the restatement, whatever the path, the permutations per group or the batch.
 *
 * Inputs:
 *  - graph: G is an n x n CSC graph, Gi / Gp int32.  There is no Gx argument: the values are not read.  Every STORED entry
 *    counts once, whatever its value, and a repeated row counts again.  Rows need not be sorted.
 *  - labels: lab[n], int32 in [0, K); K is the caller's, 1 <= K <= 256.  A class without cells is allowed: its rows and columns
 *    of every table are 0 and its z is NaN.
 *  - drop_diagonal (non-zero: on; the Python layer's default) skips the entries with row == column.
 *  - seed uint64; nperm in [1, 2^20].
 *
 * Observed counts: C[a + K * b] = the number of counted entries (row i, column j) with lab[j] == a and lab[i] == b: a is the
 * centre cell's class, b the neighbour's.  int64.
 *
 * Null: key(r, c) = rand(seed, r, c), the library's counter hash, exactly as in the null of the gene set enrichment; order_r =
 * the cells ascending by (key, c); lab_r[c] = lab[order_r[c]].  Every permutation keeps the class sizes exactly.  C_r is the
 * same tally under lab_r, r in [0, nperm).
 *
 * Tallies, integers per pair: S1 = sum_r C_r; S2 = sum_r C_r^2; n_ge = #{r: C_r >= C}; n_le = #{r: C_r <= C}.
 *
 * Statistics (sgl_nhood_stats; host code, nhood_host.h):
 *  - D = nperm * S2 - S1^2 in exact 128-bit integer arithmetic;
 *  - mean = (double)S1 / (double)nperm;  sd = sqrt((double)D) / (double)nperm (squidpy's std, ddof 0);
 *  - z = (double)(nperm * C - S1) / sqrt((double)D), NaN when D == 0;
 *  - p_enriched = (double)(1 + n_ge) / (double)(1 + nperm);  p_depleted = (double)(1 + n_le) / (double)(1 + nperm);
 *  - Benjamini-Hochberg over the K^2 pairs for each of the two p (the rule and the code of the gene set enrichment; a NaN is
 *    left out);
 *  - an integer becomes a double by one conversion that rounds to nearest even.
 *
 * Refusals, SGL_EINVAL before anything is uploaded or launched, the message naming the offender, in this order: NULL Gi, Gp or
 * lab; n < 1; Gp not starting at 0 or descending; a row outside [0, n); K outside [1, 256]; a label outside [0, K) (position and
 * value); nperm out of range; nperm * nnz^2 >= 2^63 with nnz = Gp[n] (S2 would not fit int64; the message states the largest
 * nperm that does); a negative batch.
 *
 * The plan (nhood_host.h, a pure function of the sizes and the knobs):
 *  - permutations: stable radix sorts of the keys with the cells entering in ascending order.  Up to 32 768 cells the
 *    permutations of a chunk are the segments of ONE segmented sort (one workgroup per segment); above, every permutation is one
 *    device-wide sort.  The environment variable SGL_NHOOD_SORT_SWITCH (read per call) moves the switch; the result does not
 *    depend on it.  lab_r is written permutation-interleaved: the labels of a cell under the PG permutations of a group are PG
 *    adjacent bytes, so one load at a neighbour's index serves the group.
 *  - tally: the work is cut by stored entries, in segments of 4096 entries whatever their columns (a workgroup takes a whole
 *    number of segments, at most 512 workgroups per group); an entry's column is found once per call by a search in Gp.
 *    LDS path: the PG x K x K uint32 tiles of a group in at most 128 KiB of LDS -- PG = 16 up to K = 45, 8 up to 64, 4 up to
 *    90, 2 up to 128, 1 up to 181 -- added to with LDS atomics and flushed (non-zero bins) with global atomics.  A tile's bin
 *    counts entries of one workgroup, at most nnz < 2^31: a uint32 cannot overflow.  Global path (K >= 182, or forced): global
 *    atomics straight to the int64 counts, PG = 16.
 *  - batch: permutations per batch; 0: what 256 MiB hold at n + 8 K^2 bytes per permutation, a multiple of 16, at least 16.
 *  - integer sums have one value in any order: there are no ordering rules.
 *
 * sgl_nhood_enrichment: on the context's device, stream and pool only; no resident matrix is needed and nothing of the context
 * changes but what sgl_nhood_info reports (a fit in progress continues with its bits).  All work goes to the context's stream
 * (sgl_set_stream), which is synchronised before the call returns.  Any output may be NULL: counts, S1, S2, n_ge, n_le K x K
 * int64; null_out nperm x K x K int64 (C_r at null_out[r K^2 + a + K b]), filled only when given.  The result does not
 * depend on batch.  SGL_ESTATE: a team member, an all-reduce hook, a resident shard.
 * sgl_c_nhood_enrichment: one-shot, in a context of its own; additionally the statistics (K x K doubles each, any may be NULL),
 * info (sgl_nhood_info's six values, may be NULL) and stage_ms[3] by events (keys + sort + gather; tallies; reduction; may be NULL).
 * sgl_nhood_stats: host only, no device; tallies that cannot be those of nperm permutations are refused.
 * sgl_op_nhood_permute: lab_r of the permutations [r0, r0 + nb) as nb x n int32 (0 <= r0, 1 <= nb, r0 + nb <= 2^20; labels in
 * [0, 256)), read back from the interleaved table the tally reads.
 * sgl_op_nhood_tally: the tally of nb given label vectors (labs nb x n int32, each validated) as nb x K x K int64.  path 0
 * automatic, 1 the LDS path (K >= 182 still takes the global path), 2 the global path; perms_per_group 0 the plan's value,
 * otherwise a power of two up to what the path holds at this K (else SGL_EINVAL).  The result depends on neither.
 * sgl_nhood_info: out[0] the tally's path (1 LDS, 2 global, 0 none ran), out[1] the permutations per group, out[2] the batches,
 * out[3] the permutations per batch, out[4] the LDS bytes per workgroup, out[5] the sort (0 segmented, 1 device-wide) of the
 * last of these calls on the context.
 * There is NO team form and NO R shim entry; weighted edge counts, unlabelled cells and an analytic null are not provided. */
SGL_API int sgl_nhood_enrichment(sgl_ctx* ctx, const int32_t* Gi, const int32_t* Gp, int32_t n, const int32_t* lab, int32_t K, int drop_diagonal,
                                 int32_t nperm, uint64_t seed, int32_t batch, int64_t* counts, int64_t* S1, int64_t* S2, int64_t* n_ge,
                                 int64_t* n_le, int64_t* null_out);
SGL_API int sgl_c_nhood_enrichment(const int32_t* Gi, const int32_t* Gp, int32_t n, const int32_t* lab, int32_t K, int drop_diagonal, int32_t nperm,
                                   uint64_t seed, int32_t batch, int64_t* counts, int64_t* S1, int64_t* S2, int64_t* n_ge, int64_t* n_le,
                                   int64_t* null_out, double* z, double* mean, double* sd, double* p_enr, double* p_dep, double* padj_enr,
                                   double* padj_dep, int64_t* info, double* stage_ms);
SGL_API int sgl_nhood_stats(int32_t K, int32_t nperm, const int64_t* counts, const int64_t* S1, const int64_t* S2, const int64_t* n_ge,
                            const int64_t* n_le, double* z, double* mean, double* sd, double* p_enr, double* p_dep, double* padj_enr,
                            double* padj_dep);
SGL_API int sgl_op_nhood_permute(sgl_ctx* ctx, int32_t n, const int32_t* lab, uint64_t seed, int32_t r0, int32_t nb, int32_t* lab_out);
SGL_API int sgl_op_nhood_tally(sgl_ctx* ctx, const int32_t* Gi, const int32_t* Gp, int32_t n, const int32_t* labs, int32_t nb, int32_t K,
                               int drop_diagonal, int32_t path, int32_t perms_per_group, int64_t* counts_out);
SGL_API int sgl_nhood_info(sgl_ctx* ctx, int64_t out[6]);

/* Ligand-receptor interactions: which ligand-receptor pairs are expressed between which pairs of clusters more strongly than
 * under a random relabelling of the cells -- the permutation test of CellPhoneDB (Efremova et al. 2020) and of squidpy's
 * gr.ligrec.  The rules below are this library's own statement of the published scheme; tests/ligrec_restatement.py restates
 * them in numpy.  NO parity with squidpy's or CellPhoneDB's seeded shuffles is claimed: the relabellings are this library's.
 * Every sum is formed in ONE stated order, so every result is one function of the inputs, bit for bit the restatement,
 * whatever the path, the batch or the label vectors per wave.
 *
 * Inputs:
 *  - the resident matrix, m genes x n cells, its values as they are (normally after sgl_log_normalize);
 *  - lab[n], int32 in [0, K), 1 <= K <= 256; a class without cells is allowed;
 *  - genes[G]: distinct gene indices in [0, m), the interacting genes;
 *  - lig[P], rec[P]: indices INTO genes.  lig[q] == rec[q] and repeated pairs are allowed;
 *  - nperm in [1, 2^20], seed uint64, threshold in [0, 1].
 *
 * Label vectors: vector -1 is lab itself.  Vector r in [0, nperm) is exactly the lab_r sgl_op_nhood_permute returns for
 * (lab, seed, r): the same seed gives the same relabellings in both tests.  The class sizes n_c are those of lab in every vector.
 *
 * Sums, sum_r[g, c], one order for the observed vector and the null:
 *  - gene g's stored entries in stored order, counted from the gene's first entry, are cut into segments of 8192;
 *  - within a segment the partial of class c is the sequential sum from +0.0, in stored order, of the values whose cell has
 *    label c under vector r;
 *  - the segment partials are added in ascending segment order from +0.0;
 *  - no floating-point atomics, no contraction: the sums are a function of (gene, label vector) alone;
 *  - nz[g, c] = the count of stored x != 0 of gene g in class c under lab (observed only, int64);
 *  - mean_r[g, c] = sum_r[g, c] / (double)n_c, one division; NaN with n_c == 0.
 *
 * Score: s_r[q, a, b] = 0.5 * (mean_r[lig[q], a] + mean_r[rec[q], b]) when both means are > 0, else +0.0 (a NaN mean compares
 * false: +0.0).  s is the score under lab.
 * Tallies: n_ge[q, a, b] = #{r in [0, nperm): s_r >= s}, int64.
 * Layouts: group_n[c]; nz, sum, mean at g K + c (class fastest); score and n_ge at q + P (a + K b); null_out (the s_r) at
 * r P K^2 + q + P (a + K b).
 *
 * Statistics (sgl_ligrec_stats; host code, ligrec_host.h):
 *  - expressed[g, c] = (double)nz[g, c] / (double)n_c >= threshold, false when n_c == 0 (one byte each, at g K + c);
 *  - p = (double)(1 + n_ge) / (double)(1 + nperm) where expressed[lig, a] and expressed[rec, b] both hold, NaN elsewhere.
 *    squidpy divides by nperm WITHOUT the + 1: its p can be 0, this one is at least 1 / (nperm + 1);
 *  - Benjamini-Hochberg with the rule and the code of the gene set enrichment, a NaN left out: per_interaction 0 over all
 *    P K^2 values, otherwise over the K^2 values of every pair q alone.
 *
 * Refusals, SGL_EINVAL before anything is uploaded or launched, every output untouched, the message naming the offender, in this
 * order: NULL lab, genes, lig or rec; K outside [1, 256]; G outside [1, m]; P < 1; nperm out of range; a label outside [0, K)
 * (position and value); a gene outside [0, m), or listed twice; a lig / rec index outside [0, G); a threshold outside [0, 1] or
 * NaN; a negative batch; n != the cells of the matrix.  SGL_ESTATE exactly where sgl_markers gives it: no matrix, a team
 * member, an all-reduce hook, a resident shard -- for a call on a context, before the arguments are looked at.  The context
 * stays usable after every refusal.
 *
 * The plan (ligrec_host.h, a pure function of the sizes and the knobs):
 *  - labels: the interleaved tables of the neighbourhood enrichment (groups of 16 label vectors, 16 adjacent bytes per cell);
 *  - sums: one wave owns (one segment, a group of label vectors), lane l owns vector l; the wave walks the segment in stored
 *    order and each lane adds the value to its own bin [class][lane].  LDS path: the K x vpw double bins of a wave in at most
 *    32 KiB -- vpw = 64 vectors per wave up to K = 64, 32 up to 128, 16 up to 256 -- and as many waves per workgroup (at most 8)
 *    as 64 KiB hold.  Global path (forced only): the same bins in global scratch, the same bits.  A second kernel adds the
 *    segment partials and divides;
 *  - batch: label vectors per batch; 0: what 256 MiB hold at n + (segments + 2 G) K x 8 bytes per vector, a multiple of 64, at
 *    least 64.
 *
 * sgl_ligrec: reads only the resident matrix (a fit in progress continues with its bits).  All work goes to the context's stream
 * (sgl_set_stream), which is synchronised before the call returns.  Any output may be NULL; null_out (nperm x P x K x K doubles)
 * is filled only when given.  The result does not depend on batch.
 * sgl_c_ligrec: one-shot from a dgCMatrix in a context of its own; additionally the statistics, info (sgl_ligrec_info's eight
 * values, may be NULL) and stage_ms[3] by events (labels; sums; tally; may be NULL).
 * sgl_ligrec_stats: host only, no device; tallies that cannot be those of nperm permutations are refused.
 * sgl_op_ligrec_sums: the sums of nb given label vectors (labs nb x n int32, each validated) as nb x G x K doubles at
 * (r G + g) K + c.  path 0 automatic, 1 the LDS path, 2 the global path; vectors_per_wave 0 the plan's value, otherwise a power
 * of two up to what a wave holds at this K (else SGL_EINVAL).  The result depends on neither.
 * sgl_op_ligrec_tally: score and n_ge (and the s_r) from mean tables alone: mean_obs G x K, means nb x G x K; no matrix is read.
 * sgl_ligrec_info: out[0] the sums' path (1 LDS, 2 global, 0 none ran), out[1] the label vectors per wave, out[2] the batches,
 * out[3] the vectors per batch, out[4] the LDS bytes per workgroup, out[5] the waves per workgroup, out[6] / out[7] the listed
 * genes on the LDS / on the global path, of the last sgl_ligrec / sgl_c_ligrec / sgl_op_ligrec_sums on the context.
 * NOT provided: multi-subunit complexes (CellPhoneDB's min over the subunits), unlabelled cells, a team form, an R shim entry, an
 * interaction database -- the caller brings the pairs. */
SGL_API int sgl_ligrec(sgl_ctx* ctx, const int32_t* lab, int32_t n, int32_t K, const int32_t* genes, int32_t G, const int32_t* lig, const int32_t* rec,
                       int32_t P, int32_t nperm, uint64_t seed, int32_t batch, int64_t* group_n, int64_t* nz, double* sum, double* mean,
                       double* score, int64_t* n_ge, double* null_out);
SGL_API int sgl_c_ligrec(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol, const int32_t* lab, int32_t K,
                         const int32_t* genes, int32_t G, const int32_t* lig, const int32_t* rec, int32_t P, int32_t nperm, uint64_t seed,
                         int32_t batch, double threshold, int per_interaction, int64_t* group_n, int64_t* nz, double* sum, double* mean,
                         double* score, int64_t* n_ge, double* null_out, uint8_t* expressed, double* p, double* padj, int64_t* info,
                         double* stage_ms);
SGL_API int sgl_ligrec_stats(int32_t K, int32_t G, int32_t P, int32_t nperm, const int64_t* group_n, const int64_t* nz, const int32_t* lig,
                             const int32_t* rec, const int64_t* n_ge, double threshold, int per_interaction, uint8_t* expressed, double* p,
                             double* padj);
SGL_API int sgl_op_ligrec_sums(sgl_ctx* ctx, const int32_t* labs, int32_t n, int32_t nb, int32_t K, const int32_t* genes, int32_t G, int32_t path,
                               int32_t vectors_per_wave, double* sum_out);
SGL_API int sgl_op_ligrec_tally(sgl_ctx* ctx, const double* mean_obs, const double* means, int32_t nb, int32_t K, int32_t G, const int32_t* lig,
                                const int32_t* rec, int32_t P, double* score_out, int64_t* n_ge_out, double* null_out);
SGL_API int sgl_ligrec_info(sgl_ctx* ctx, int64_t out[8]);

/* Co-occurrence by distance: how the presence of class b changes with the distance from a point of class a -- the score of
 * squidpy's gr.co_occurrence (Tosti et al. 2021) and, in its cumulative same-class form, Ripley's K / L (gr.ripley).  Where the
 * neighbourhood enrichment asks about adjacency on a graph, this asks about EVERY pair of points up to a radius.  The rules below
 * are this library's own statement of the published score; tests/cooccur_restatement.py restates them in numpy.  NO parity with
 * squidpy is claimed and no run against it is made: squidpy works in float32 and picks its thresholds from the data's pairwise
 * distances.  Everything the device computes is an integer, so the table is one function of the inputs, bit for bit the
 * restatement, whatever the grid, the bin path, the tiling or the flush bound.
 *
 * Inputs:
 *  - n points (c1[e], c2[e]) in FP64: two dimensions, as sgl_spatial_graph;
 *  - labels lab[e], int32 in [0, K), 1 <= K <= 256; a class without points is allowed;
 *  - thresholds r[0] < r[1] < ... < r[T], T intervals, 1 <= T <= 64.
 *
 * Distance: dx = fl(c1[i] - c1[j]), dy likewise, d2 = fl(fl(dx * dx) + fl(dy * dy)), uncontracted (the unit is compiled with
 * -ffp-contract=off): sgl_spatial_graph's sum without the root.  It is bitwise symmetric in (i, j).
 *
 * Binning: thr2[t] = fl(r[t] * r[t]), computed once on the host.  Pair (i, j), i != j, lies in interval t iff thr2[t] < d2 <=
 * thr2[t + 1] -- squidpy's (dist > lo) & (dist <= hi) on squares.  NO root is taken: this can differ from comparing sqrt(d2) with
 * r only where one rounding decides (d2 within a rounding of r[t]^2).  With r[0] = 0 coincident points (d2 == 0) are in no interval.
 *
 * Tallies, int64: N[a + K b + K^2 t] = the number of ORDERED pairs (i, j), i != j, with lab[i] == a, lab[j] == b, in interval
 * t.  N is symmetric in (a, b) and its diagonal is even (every unordered pair is two ordered ones); sgl_cooccur_stats and
 * sgl_ripley_stats refuse a table that is not.
 *
 * Statistics (host code, cooccur_host.h, pure functions):
 *  - per interval, or cumulatively: cumulative != 0 first replaces N[t] by sum_{s <= t} N[s] in exact integers;
 *  - tot = sum_{a, b} N[a, b, t];  row[a] = sum_b N[a, b, t];
 *  - ratio[a, b, t] = ((double)N / (double)row[a]) / ((double)row[b] / (double)tot), the divisions in this order: P(b | within
 *    the interval of an a) over P(b among all pairs of the interval), squidpy's probs_con; NaN when row[a] == 0 or row[b] == 0;
 *  - an integer becomes a double by one conversion that rounds to nearest even;
 *  - Ripley, from the cumulative diagonal Ncum[a, a, t] = sum_{s <= t} N[a, a, s]: Kfun[a, t] = (area * (double)Ncum[a, a, t]) /
 *    (double)(n_a (n_a - 1)), the product n_a (n_a - 1) in exact integers; L = sqrt(Kfun / pi), pi = 0x1.921fb54442d18p+1.  area is
 *    the caller's (the Python layer defaults it to the bounding box).  NaN for n_a < 2.  K_out / L_out hold [a + K t].  Out of
 *    scope: edge correction, simulation envelopes, the F and G functions.
 *
 * Refusals, SGL_EINVAL before anything is uploaded or launched, every output untouched, the message naming the offender, in this
 * order: NULL c1, c2, lab or r; n < 1; a coordinate that is not finite (position and value); K outside [1, 256]; a label outside
 * [0, K) (position and value); T outside [1, 64]; r[0] < 0 or a threshold that is not finite; thr2 not strictly ascending or not
 * finite (the index); a negative knob (or one outside its range).  SGL_ESTATE: a team member, an all-reduce hook, a resident
 * shard, as sgl_nhood_enrichment.  The context stays usable after every refusal.
 *
 * The plan (cooccur_host.h, pure functions of the extent, the sizes and the knobs):
 *  - bucket sort: the extent is computed on the device; square buckets of side max(r[T], 2^-510) (1 + 2^-10) (raised to the extent
 *    2^-30), key by * W + bx with b = floor((c - cmin) / side), a stable radix sort, x, y and the label gathered into sorted
 *    order.  Every pair that passes the test lies in adjacent buckets (the argument is written above cooccur_grid).  When the grid
 *    would be at most 3 x 3 buckets, or the extent overflows, the plan takes ONE bucket: all pairs, nothing sorted;
 *  - tally: sorted positions are cut into centre tiles of 256, a lane holds one centre, candidate tiles of 256 are staged in LDS.
 *    An unordered pair is counted exactly once, by the lower sorted position: a centre's candidates are the positions after its
 *    own in its bucket row up to the end of bucket bx + 1, and buckets bx - 1 .. bx + 1 of row by + 1; a tile walks a superset of
 *    its centres' candidates, the exact d2 test and pos_j > pos_i decide.  It adds 1 to bin [t][min(a, b)][max(a, b)]; an epilogue
 *    mirrors the off-diagonal and doubles the diagonal.  At most 1024 workgroups take contiguous ranges of centre tiles; in the
 *    all-pairs regime up to 64 workgroups share a range, each taking every split-th candidate tile;
 *  - bins: LDS path while T K^2 uint32 bins + 6144 bytes of staging fit 128 KiB -- LDS atomics, flushed (non-zero bins) with
 *    64-bit global atomics at the end and EARLIER whenever the pairs evaluated since the last flush would pass 2^32 - 1, what a
 *    uint32 bin holds; global path (the bins do not fit, or forced): 64-bit global atomics.  Integer sums have one value in any
 *    order: there are no ordering rules, only the once-per-unordered-pair rule.  No floating-point atomics anywhere.
 *
 * sgl_cooccur: on the context's device, stream and pool only; no resident matrix is needed and nothing of the context changes but
 * what sgl_cooccur_info reports (a fit in progress continues with its bits).  All work goes to the context's stream
 * (sgl_set_stream), which is synchronised before the call returns.  counts: T x K x K int64.
 * sgl_c_cooccur: one-shot, in a context of its own; additionally ratio (the per-interval statistic, T x K x K doubles), info
 * (sgl_cooccur_info's eight values) and stage_ms[3] by events (sort + gather; tally; epilogue + download); counts and each of
 * these may be NULL.
 * sgl_cooccur_stats, sgl_ripley_stats: host only, no device; either of K_out and L_out may be NULL.  Both refuse (SGL_EINVAL, the
 * message naming the offender, outputs untouched) K outside [1, 256], T outside [1, 64], NULL counts, and a table that is no
 * tally (a negative count, N[a, b] != N[b, a], an odd diagonal, a total above 2^63 - 1).  sgl_ripley_stats also refuses, in this
 * order: NULL group_n; an area that is not a positive finite number; a group_n[a] that is negative or above 2^31; a class whose
 * cumulative diagonal counts more ordered pairs than n_a (n_a - 1), which no n_a points can form.
 * sgl_op_cooccur_tally: the tally with its knobs.  grid_mode 0 the plan, 1 one bucket (all pairs), 2 the bucket grid whatever its
 * size; bin_path 0 the plan, 1 the LDS path (bins that do not fit still go global), 2 the global path; flush_pairs 0 the plan's
 * bound, otherwise a smaller one (a bound below one stage of 256 x 256 pairs flushes before every stage).  The result depends on
 * none of the three.
 * sgl_cooccur_info: out[0] the grid mode run (1 one bucket, 2 the bucket grid, 0 none ran), out[1] W, out[2] H, out[3] the bin path
 * (1 LDS, 2 global), out[4] the LDS bytes per workgroup, out[5] the workgroups, out[6] the flushes of all workgroups (the one at a
 * workgroup's end included), out[7] the candidate pairs evaluated, of the last co-occurrence call on the context.
 * NOT provided: a permutation null, 3-D coordinates, a team form, an R shim entry. */
SGL_API int sgl_cooccur(sgl_ctx* ctx, const double* c1, const double* c2, int32_t n, const int32_t* lab, int32_t K, const double* r, int32_t T,
                        int64_t* counts);
SGL_API int sgl_c_cooccur(const double* c1, const double* c2, int32_t n, const int32_t* lab, int32_t K, const double* r, int32_t T, int64_t* counts,
                          double* ratio, int64_t* info, double* stage_ms);
SGL_API int sgl_cooccur_stats(int32_t K, int32_t T, const int64_t* counts, int cumulative, double* ratio_out);
SGL_API int sgl_ripley_stats(int32_t K, int32_t T, const int64_t* counts, const int64_t* group_n, double area, double* K_out, double* L_out);
SGL_API int sgl_op_cooccur_tally(sgl_ctx* ctx, const double* c1, const double* c2, int32_t n, const int32_t* lab, int32_t K, const double* r, int32_t T,
                                 int32_t grid_mode, int32_t bin_path, int64_t flush_pairs, int64_t* counts);
SGL_API int sgl_cooccur_info(sgl_ctx* ctx, int64_t out[8]);

/* Start a fit at rank k.  w_init: k x nrow host array, or NULL to fill W on
 * the device with the synthetic init ((rand_{S+2}(f,g) >> 11) + 0.5) * 2^-53.
 * h = 0, d = 1 as in src/singlet.cpp:639-641.
 * May be called again and again on one resident matrix (R's ard_nmf / cross_validate_nmf refit one matrix tens
 * of times, R/ard_nmf.R:95-160): the re-blocked entry streams of the matrix (2 x ~15 bytes per non-zero at
 * k <= 128, + 8 per non-zero once a masked fit has run) are kept between fits -- a fit at an unchanged rank reuses
 * them as they are, another rank rebuilds them in the same allocations -- and are released when the matrix changes
 * (upload, synth, log-normalize, weight_by_split, rasterize, subset) or the context is destroyed. */
SGL_API int sgl_fit_init(sgl_ctx* ctx, int32_t k, const double* w_init, uint64_t synth_seed);

/* Link matrices of c_linked_nmf for the current fit (after sgl_fit_init; the
 * rules of sgl_c_linked_nmf; link_h columns are the cells of this shard). */
SGL_API int sgl_set_links(sgl_ctx* ctx, const double* link_h, int32_t link_h_rows, int32_t link_h_cols,
                          const double* link_w, int32_t link_w_rows, int32_t link_w_cols);

/* The grouped form of the link matrices, for links whose column is a function of the cell's (gene's) group alone, as
 * RunLNMF.Seurat builds them (R/RunLNMF.R:146-154).  Behaves exactly as if sgl_set_links had received
 *   link_h[j, c] = table_h[j, group_h[c]]   (table_h rows_h x groups_h column-major, group_h one id per LOCAL cell) and
 *   link_w[j, g] = table_w[j, group_w[g]]   (table_w rows_w x groups_w, group_w one id per gene),
 * without the expanded matrices ever existing: the device holds rows * groups doubles plus 4 bytes per cell / gene.
 *  - every entry of the right-hand sides gets the same single multiplication as in the dense form (never a select:
 *    b * 0.0 keeps the sign of b), so a fit gives the same bits either way.  A table of up to 32 KiB (rows * groups * 8)
 *    is staged in LDS by every workgroup, a larger one is read through the cache; the group id is loaded once per cell.
 *  - a NULL table (or rows < 1) switches that side off.  A side that is on needs its group list (SGL_EINVAL without).
 *  - lifetime as sgl_set_links: after sgl_fit_init, dropped by the next one.  sgl_set_links and sgl_set_links_grouped
 *    each replace everything the other (or an earlier call of itself) set, on both sides.
 *  - refused like sgl_set_links: with a cell graph set, and when a table has more rows than the rank (SGL_EINVAL; the
 *    links set before are gone then, as after sgl_set_links' refusal).
 *  - groups < 1 on a side that is on is SGL_EINVAL; a group id outside [0, groups) is SGL_EINVAL with a message naming
 *    the list, the position and the value of the first offender.  Both lists are checked completely before anything is
 *    freed or launched: after such a refusal the links set before are still in force.
 *  - table values are not checked for finiteness (sgl_set_links does not check its matrices either). */
SGL_API int sgl_set_links_grouped(sgl_ctx* ctx, const double* table_h, int32_t rows_h, int32_t groups_h, const int32_t* group_h,
                                  const double* table_w, int32_t rows_w, int32_t groups_w, const int32_t* group_w);

/* Group means of a k x n factor matrix: means[f, g] = mean of F[f, c] over the cells c with group[c] == g -- the k x G table
 * that RunLNMF.Seurat (R/RunLNMF.R:136-143) and MetadataSummary (R/MetadataSummary.R:18-26) form with k G calls of
 * mean(h[which(...)]).
 *  - F: a host k x n array (column-major, one column per cell), or NULL for the H of the current fit, which stays where it
 *    is; with NULL, k and n must be the fit's rank and the resident matrix's cell count (SGL_EINVAL otherwise).
 *  - means: k x n_groups column-major; counts: int64_t[n_groups] cells per group.  means[f, g] = sum / (double)counts[g], one
 *    true division; an empty group gives NaN, the 0.0 / 0.0 of R's mean(numeric(0)).
 *  - the summation order is a function of (n, group, n_groups) alone -- no floating-point atomics, nothing depends on the
 *    launch size or the occupancy -- so two calls give the same bits, and the resident, the host-F and the one-shot form
 *    agree bit for bit.  The order: the cells of a group, in ascending cell index, are cut into chunks of 256; inside a
 *    chunk, slot s of S = 256 / min(64, k rounded up to a power of two) takes the cells s, s + S, ... in turn and the S slot
 *    sums are added by a binary tree; the chunk sums are added in chunk order.  |error| <= n_g 2^-53 mean_g |x| to first order.
 *  - refused: SGL_ESTATE on a team member, with an all-reduce hook set (the shard's means are not the matrix's; a team
 *    uses sgl_multi_group_means), or with F == NULL and no fit; SGL_EINVAL for n_groups < 1, k outside [1, 1024], n < 0 and
 *    for a group id outside [0, n_groups), the message naming the list, the position and the value of the first offender
 *    (the whole list is checked before anything is launched).  The context stays usable after every refusal.
 *  - values are not checked for finiteness: NaN / Inf propagate through the IEEE sums. */
SGL_API int sgl_group_means(sgl_ctx* ctx, const double* F, int32_t k, int64_t n, const int32_t* group, int32_t n_groups,
                            double* means, int64_t* counts);
/* The one-shot form: its own context on the current device (like sgl_c_rowwise_compress_*); F must not be NULL. */
SGL_API int sgl_c_group_means(const double* F, int32_t k, int64_t n, const int32_t* group, int32_t n_groups,
                              double* means, int64_t* counts);

/* Model error of the current factors against the resident matrix: per cell j and per gene i the sum of the squared
 * residuals of the plain reconstruction w^T diag(d) h over ALL entries of the column (row), zeros included,
 *   cell_loss[j] = sum_i (A_ij - sum_f w_fi d_f h_fj)^2 = ||a_j||^2 - 2 h_j . b_j + h_j^T Gw h_j,   b_j = W^ a_j,  Gw = W^ W^^T,
 * with W^ = diag(d) w, from the sparse structure alone (nnz k + (m + n) k^2 multiply-adds, never m n k); the gene side is
 * the same over t(A) with H^ = diag(d) h.  b and Gw come from the fit's own accumulate and Gram kernels.
 *  - cell_loss: ncol doubles; gene_loss: nrow doubles.  Either may be NULL and that side's pass is skipped; with both NULL
 *    the cell side still runs, for sse.  sse = the sum of the cell losses; mse = sse / ((double)nrow * (double)ncol), one
 *    true division.  sse and mse may be NULL.
 *  - what is evaluated is w^T diag(d) h alone: link matrices (either form) and a cell graph set on the fit are ignored.
 *  - sign: a loss that cancellation leaves at or below zero is returned as +0.0 (the true value is >= 0); NaN and Inf
 *    propagate.  sse is formed from the clamped cell losses.  |error| of a loss <= (max column nnz + m + k^2 + 4) 2^-53
 *    (||a_j||^2 + 2 |h_j| . |b_j| + |h_j|^T |Gw| |h_j|) to first order: relative to the TERMS, not to the loss, so a
 *    near-exact fit keeps few digits of a small loss.
 *  - the result is a function of (matrix, k, factors) alone -- no floating-point atomics, nothing depends on the launch
 *    size or the occupancy -- so two calls give the same bits, and the resident and the one-shot form agree bit for bit.
 *    The orders: ||a_j||^2: lane l of 64 adds the squares of the entries l, l + 64, ... of the column in stored order, the
 *    lane sums are added by a butterfly (lane ^ 32, 16, ... 1).  t_f = sum_g Gw[f, g] h_g with g ascending; lane l adds
 *    h_f b_f and h_f t_f over f = l, l + 64, ...; the same butterfly; loss = (||a_j||^2 - 2 dot) + quad.  sse: the cells in
 *    matrix order are cut into chunks of 1024; thread t of 256 adds the cells t, t + 256, t + 512, t + 768 of its chunk in
 *    that order, the 256 sums are added by a binary tree (t += t + stride, stride = 128 ... 1), and the chunk sums are added
 *    in chunk order starting from +0.0.
 *  - the call uses the fit's scratch (right-hand sides, Gram, workspace) and changes nothing a later step reads: a fit
 *    continued after it gives the bits it would have given without it.  The kernels' time counts in the existing rhs_h,
 *    rhs_w and gram phases or in none.
 *  - refused: SGL_ESTATE without a resident matrix or without a fit; SGL_ESTATE on a team member or with an all-reduce
 *    hook set (the shard's losses are not the matrix's; a one-process team uses sgl_multi_evaluate).  After
 *    sgl_upload_dense the call WORKS: it runs over the CSC image that upload keeps next to the dense matrix (the sparse
 *    accumulate, whatever kernel the fit's own right-hand sides use).  The context stays usable after every refusal. */
SGL_API int sgl_evaluate(sgl_ctx* ctx, double* sse, double* mse, double* cell_loss, double* gene_loss);
/* The one-shot form: its own context on the current device (like sgl_c_group_means); A as a dgCMatrix (t(A) is built on
 * the device), w k x nrow, d k, h k x ncol as sgl_set_factors takes them.  SGL_EINVAL for k outside [1, 1024] and for a
 * NULL factor, before anything is uploaded; an invalid matrix is refused as by sgl_upload_csc. */
SGL_API int sgl_c_evaluate(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol,
                           const double* w, const double* d, const double* h, int32_t k,
                           double* sse, double* mse, double* cell_loss, double* gene_loss);

/* Variable features of the resident COUNTS: the selection Seurat stores in var.features by default,
 * FindVariableFeatures(selection.method = "vst"), which RunNMF.Seurat reads as features = "var.features"
 * (R/RunNMF.R:73-74) -- per-gene mean and variance of the counts, a smooth trend of log10(variance) on log10(mean), the
 * variance of the clipped standardised counts, and the top nfeatures genes by it.  Neither Seurat nor R was at hand:
 * the rules below are this library's own, stated in full; tests/variable_features_restatement.py restates them.
 *
 * The three gene passes run over the gene-side image t(A) (one column per gene, 64-bit offsets).  n = ncol; c_g = the
 * stored entries of gene g, explicit zeros included.  All sums are in double, without contraction (a product and the
 * addition that follows are two roundings) and without floating-point atomics; no loop's trip count follows the launch.
 *  - mean:   S_g = sum of the stored x;  mean_g = S_g / (double)n, one true division;  count_g = c_g.
 *  - variance, given mu (Seurat's SparseRowVar2):  d = x - mu_g, t = d * d for every stored x;  Q_g = sum of the t;
 *    Z_g = (double)(n - c_g) * (mu_g * mu_g);  var_g = (Q_g + Z_g) / (double)(n - 1).
 *  - standardised variance, given mu, sd and vmax (Seurat's SparseRowVarStd):  sd_g == 0 gives +0.0.  Otherwise
 *    z = (x - mu_g) / sd_g (a true division), z = z > vmax ? vmax : z, t = z * z;  Q_g = sum of the t;
 *    z0 = (0.0 - mu_g) / sd_g, NOT clipped (as in Seurat);  Z_g = (double)(n - c_g) * (z0 * z0);  the result is
 *    (Q_g + Z_g) / (double)(n - 1).
 *  - THE SUMMATION ORDER of S_g and of either Q_g is a function of c_g alone: the gene's entries, in stored order, are cut
 *    into segments of 8192 (the last one shorter); inside a segment lane l of 64 adds the terms of the segment's entries
 *    l, l + 64, ... in that order, starting from +0.0, and the 64 lane sums are added by a butterfly (v += v[lane ^ 32],
 *    then 16, 8, 4, 2, 1); the segment sums are added in ascending segment order starting from +0.0 (a gene without a
 *    stored entry gives +0.0).  One wave works on one segment, so a gene stored in every cell is not walked by one wave
 *    alone.  Two calls, the resident and the one-shot form give the same bits.  To first order, for terms that are not
 *    negative, |error| <= (c_g + 2) 2^-53 of the mean and (3 c_g + 8) 2^-53 of either variance.
 *  - the trend (sgl_op_loess_direct): x and y of length m, sorted ascending by (x, original index), and a window length
 *    q, 1 <= q <= m.  For every point i on its own:
 *      window   the q consecutive sorted positions s .. s + q - 1 containing i (max(0, i - q + 1) <= s <= min(i, m - q))
 *               whose farthest member is nearest: f(s) = max(x_i - x_s, x_{s + q - 1} - x_i) is least, ties to the lowest s;
 *               hmax = that f(s).
 *      weights  u = x_j - x_i, r = |u| / hmax, r3 = (r * r) * r, c = 1 - r3, w = (c * c) * c; every w is 1 when hmax == 0.
 *      degree   D = the distinct x among the window's members of POSITIVE weight (hmax == 0 or |u| < hmax; the members at
 *               the distance hmax itself weigh nothing and cannot carry a coefficient): degree 2 for D >= 3, 1 for
 *               D == 2, 0 for D == 1.
 *      moments  S0 .. S4 = sum of w, wu = w * u, wu2 = wu * u, wu3 = wu2 * u, wu4 = wu3 * u;  T0, T1, T2 = sum of w * y,
 *               wu * y, wu2 * y: lane l of 64 adds the members s + l, s + l + 64, ... in that order, then the butterfly above.
 *      fit      weighted least squares in u; the fitted value is the intercept: degree 0: T0 / S0;  degree 1:
 *               (S2 T0 - S1 T1) / (S0 S2 - S1 S1);  degree 2, by Cramer's rule with A = S2 S4 - S3 S3:
 *               (T0 A - S1 (T1 S4 - S3 T2) + S2 (T1 S3 - S2 T2)) / (S0 A - S1 (S1 S4 - S3 S2) + S2 (S1 S3 - S2 S2)).
 *    This is an exact local fit at EVERY point.  It is NOT R's default loess(surface = "interpolate"), which fits at the
 *    vertices of a k-d tree and blends them; that code was not at hand and nothing here is pinned to it.  The difference
 *    is in the trend alone: a caller with R's (or any other) loess at hand passes its expected variances (below) and
 *    gets exact parity with it for everything else.
 *
 * sgl_variable_features: mean and variance (mu = mean) as above; m' = the genes with variance > 0.  expected_var, when
 * not NULL, holds nrow doubles and IS the expected variance.  Otherwise the expected variance of the m' genes is
 * 10^fitted, from the trend of y = log10(variance) on x = log10(mean) over them with q = max(min(m', 3), floor(span m')),
 * and 0 for the constant genes.  sd = sqrt(expected); vmax <= 0 (or NaN) means sqrt((double)n).  The genes are ranked by
 * standardised variance, descending, ties to the lower gene index (a NaN ranks last).  features receives the first
 * min(nfeatures, nrow) gene indices (0-based) in rank order -- the order A[var.features, ] puts the rows in -- and *n_out
 * how many were written.  info, when not NULL, is 4 x nrow column-major: mean, variance, expected, standardised of gene g
 * at info[4 g .. 4 g + 3].  Host code in the library (nrow doubles): log10, the sort, pow, sqrt and the ranking; device:
 * the three passes over the stored values and the trend.
 *  - refused with SGL_EINVAL, nothing changed: nfeatures < 1; span outside (0, 1]; ncol < 2; a NULL features or n_out; a
 *    negative or non-finite expected_var; a gene of positive variance whose mean is not positive (the message names it).
 *  - refused with SGL_ESTATE: with no matrix resident, on a team member, with an all-reduce hook set, and on a context
 *    that holds a shard (cell_offset != 0 or ncells_total != ncol): a shard's moments are not the matrix's, and
 *    sgl_subset, which follows, is refused there too.  The context stays usable after every refusal.
 *  - after sgl_upload_dense the call WORKS, over the CSC image that upload keeps.
 *  - the call only reads: the matrix and a fit in progress stay untouched -- entry streams, mask lists and the packed
 *    solves' sweep counts included; a fit continued after it gives the bits it would have given without it.  The kernels'
 *    time counts in the "scale" phase when timing is on.
 *  - 64-bit indexing throughout; values are not checked again (an upload refuses non-finite ones). */
SGL_API int sgl_variable_features(sgl_ctx* ctx, int32_t nfeatures, double span, double vmax, const double* expected_var,
                                  int32_t* features, int32_t* n_out, double* info);
/* The one-shot form: its own context on the current device, A as a dgCMatrix (t(A) is built on the device); the argument
 * refusals come before anything is uploaded.  Neither uses nor touches the SINGLET_HIP_CACHE context. */
SGL_API int sgl_c_variable_features(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol,
                                    int32_t nfeatures, double span, double vmax, const double* expected_var,
                                    int32_t* features, int32_t* n_out, double* info);

/* Marker genes: which genes mark each cluster -- Seurat's FindAllMarkers / FindMarkers with the default Wilcoxon rank-sum
 * test, one-vs-rest, for every gene and every cluster from ONE ordering of the gene's values over the resident matrix.  The
 * reference's package has no such function (it hands the object to Seurat); the rules below are this library's own, stated
 * in full; tests/markers_restatement.py restates them in numpy and scipy.stats.mannwhitneyu is the independent yardstick.
 *
 * Inputs.  The resident matrix, m genes x n cells, values as they are (normally after sgl_log_normalize).  labels[n], int32
 * in [-1, G): a cell labelled -1 is left out of everything; every other cell is included.  N = the included cells, n_c = the
 * size of cluster c (group_n).  FindMarkers(ident.1, ident.2) is the case labels in {0, 1, -1}.  1 <= G <= 1024;
 * ncol <= 2^21, so that the tie term fits 64 bits (N^3 - N < 2^63).
 *
 * Entry classes, per gene g, over the gene's stored entries in included cells: x == 0.0 (either sign) is a zero and joins
 * the gene's implicit zeros; pos[g, c] = the stored x > 0 in cluster c; nz[g, c] = the stored x != 0 in cluster c.
 *
 * Ranks.  The N values of the gene are ordered: the negatives ascending, the zero block of N - sum_c nz[g, c] values, the
 * positives ascending.  A tie run is a maximal set of equal doubles; the zero block is one run.  A run at the 0-based
 * positions [a, b) gives each member the DOUBLED midrank a + b + 1.  rank2[g, c] (int64) = the sum of the doubled midranks
 * of the members in cluster c (the zero block has n_c - nz[g, c] members of c); tie[g] (uint64) = the sum over the runs of
 * t^3 - t, t = b - a.  sum_c rank2[g, c] = N (N + 1).  All integers: any correct kernel gives the same bits, whatever its
 * tiling, and the batching of the long path cannot change one.
 *
 * Group sums.  sum[g, c] = the sum of f(x) over the gene's stored entries in cluster c; transform 0: f = identity, 1:
 * f = expm1 (Seurat's mean function of log-normalised data), evaluated on the device.  THE SUMMATION ORDER is a function
 * of the gene's entries and the labels alone: the entries in stored order -- those of excluded cells included, as members of
 * no cluster -- are cut into segments of 8192; a segment into blocks of 64 consecutive entries; the block partial of cluster
 * c is the butterfly sum (v += v[lane ^ 32], then 16, 8, 4, 2, 1) of 64 lane values, +0.0 for a lane that holds no member of
 * c or lies past the end; the block partials are added in ascending block order from +0.0 within a segment, the segment
 * partials in ascending segment order from +0.0.  A block without a member of c may be skipped: the bits do not change.
 * No floating-point atomics, no contraction, no loop whose trip count follows the launch size.
 *
 * Derived statistics, on the host inside the library, once per (g, c), with n1 = n_c and n2 = N - n_c:
 *   pct_in = pos / n1;  pct_out = (sum over c' != c of pos) / n2;  mean_in = sum / n1;  S_out = the sum[g, c'] of c' != c
 *   added in ascending c' from +0.0;  mean_out = S_out / n2;  log2fc = log2(mean_in + pseudocount) - log2(mean_out +
 *   pseudocount);  U2 = rank2 - n1 (n1 + 1) and D = U2 - n1 n2 in int64;
 *   var = ((double)n1 * (double)n2 / 12.0) * (((double)N + 1.0) - (double)tie / ((double)N * ((double)N - 1.0))).
 *   With n1 or n2 zero, or !(var > 0): the ratios of the empty side are NaN (0 / 0), z and p are NaN.  Otherwise
 *   a = |D| / 2.0 - 0.5, raised to 0 when negative (the continuity correction); zz = a / sqrt(var); z = D < 0 ? -zz : zz;
 *   p = erfc(zz * M_SQRT1_2), two-sided: R's wilcox.test(exact = FALSE, correct = TRUE), scipy's asymptotic method.
 *
 * sgl_markers: the per-(g, c) arrays are m x G column-major, gene fastest (a cluster's column is contiguous); group_n has G
 * values, tie m.  ANY output pointer may be NULL.
 *  - refused with SGL_EINVAL, nothing launched: NULL labels; n_groups outside [1, 1024]; a transform outside {0, 1}; a
 *    pseudocount that is negative or not finite; ncol > 2^21; a label outside [-1, G) -- the whole list is checked first,
 *    the message names position and value.
 *  - refused with SGL_ESTATE: with no matrix resident, on a team member, with an all-reduce hook set, and on a context that
 *    holds a shard.  The context stays usable after every refusal.
 *  - after sgl_upload_dense the call WORKS, over the CSC image that upload keeps.
 *  - the call only reads: the matrix, a running fit, entry streams and mask lists stay untouched; a fit continued after it
 *    gives the bits it would have given without it.  The kernels' time counts in the "scale" phase when timing is on.
 *  - two rank paths: a gene with at most CAP = 2048 included non-zero entries is sorted in LDS by one workgroup; a longer
 *    one goes through scratch and a segmented radix sort, in batches of whole genes in ascending order (each below 2^31
 *    entries and the scratch budget, 24 bytes per entry; a gene above the budget is a batch of its own), and is then walked
 *    in chunks of 1024 positions with the run start and end carried across chunk edges.  64-bit indexing throughout.
 *  - there is NO team form and NO R shim entry: a team's shards hold different cells, and a gene's ranks need them all. */
SGL_API int sgl_markers(sgl_ctx* ctx, const int32_t* labels, int32_t n_groups, int transform, double pseudocount, int64_t* group_n,
                        int64_t* pos, double* sum, int64_t* rank2, uint64_t* tie, double* pct_in, double* pct_out, double* log2fc,
                        double* z, double* p);
/* The one-shot form: its own context on the current device, A as a dgCMatrix (t(A) is built on the device); the argument
 * refusals come before anything is uploaded.  Neither uses nor touches the SINGLET_HIP_CACHE context. */
SGL_API int sgl_c_markers(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol, const int32_t* labels,
                          int32_t n_groups, int transform, double pseudocount, int64_t* group_n, int64_t* pos, double* sum,
                          int64_t* rank2, uint64_t* tie, double* pct_in, double* pct_out, double* log2fc, double* z, double* p);
/* What the last rank pass on this context ran: out[0] the genes sorted in LDS, out[1] the genes on the long path, out[2]
 * the batches of the long path, out[3] the LDS cap (included non-zero entries). */
SGL_API int sgl_markers_info(sgl_ctx* ctx, int64_t out[4]);

/* Signature scores: how strongly every cell expresses every gene signature -- the rank-based UCell score (Andreatta &
 * Carmona 2021, "UCell: robust and scalable single-cell gene signature scoring"): the Mann-Whitney U of the signature's genes
 * within ONE descending ordering of the cell's values.  The reference's package has no such function; the rules below are this
 * library's own statement of UCell's published definition, in full; tests/signature_restatement.py restates them in numpy
 * and scipy.stats.rankdata is the independent yardstick.  NO parity run against the R package is claimed.
 *
 * Inputs.  The resident matrix A, m genes x n cells, values as they are (non-finite values are refused at upload).  The
 * score depends only on the order of the values within a cell: raw counts, the log-normalised matrix and a
 * sgl_weight_by_split matrix give the same scores.  max_rank R, 1 <= R <= m.  n_sets >= 1 gene sets as set_ptr (int64,
 * n_sets + 1 offsets from 0, ascending) and set_genes (int32, 0-based gene indices in [0, m)), the layout sgl_c_gsea takes.
 * No gene twice within a set; the size n_s of a set satisfies 1 <= n_s <= R; a gene may be in any number of sets.
 *
 * Order within cell c.  Descending by value: the P stored entries x > 0, then ONE zero block of Z = m - P - N genes, then
 * the N stored entries x < 0.  The zero block holds the implicit zeros and the stored zeros of either sign.  A tie run is a
 * maximal set of equal doubles; a run at the 0-based positions [a, b) gives each member the DOUBLED midrank r2 = a + b + 1.
 * The zero block is never materialised: it is the run a = P, b = P + Z, and the positions of the negatives are shifted by Z.
 *
 * Cap.  r2' = r2 when r2 <= 2 R, else 2 R + 2: UCell's "ranks above maxRank become maxRank + 1".  A midrank of exactly R is
 * kept, a midrank of R + 0.5 is capped.
 *
 * Per (set s, cell c).  rank2[s, c] (uint64) = the sum of r2' over the genes of the set.
 *   score[s, c] = 1.0 - (double)(rank2 - n_s (n_s + 1)) / (2.0 * n_s * R)
 * which is 1 - U / (n_s R) with U = rank sum - n_s (n_s + 1) / 2: one conversion (exact), one division and one subtraction,
 * both correctly rounded; the score lies in [(n_s - 1) / (2 R), 1].  rank2 is all integers: any correct kernel gives the same
 * bits, whatever its paths, batches or passes, and the score is the same expression in numpy, bit for bit.  No floating-point
 * atomics; integer atomics in any order cannot change a bit; no contraction.
 *
 * sgl_signature_scores: both outputs hold n_sets x ncol values, column-major with the SET fastest: out[s + n_sets * c] (a
 * cell's scores are contiguous; read as a C array it is ncol x n_sets).  EITHER output may be NULL.
 *  - refused with SGL_EINVAL, nothing launched, with a message that names the FIRST defect in this order: no matrix
 *    resident; a context that is a rank of a team; NULL set_ptr or set_genes; n_sets < 1; max_rank outside [1, m]; a
 *    negative knob (the operator forms below); then set_ptr over all sets -- an offset that does not start at 0 or
 *    descends, an empty set, a set with n_s > max_rank; then the genes set by set -- a gene outside [0, m), a gene twice in
 *    one set.  The context stays usable after every refusal.
 *  - works after sgl_upload_dense (over the CSC image that upload keeps) and after the typed / native upload.
 *  - the call only reads the context: the matrix, a running fit, entry streams and mask lists stay untouched; a fit
 *    continued after it gives the bits it would have given without it.  Its kernels count in the "scale" phase.
 *  - paths: a count pass gives every cell its P and N, L = P + N.  A cell with L <= 1024 is gathered into LDS as (key, gene)
 *    pairs -- the key the order-preserving 64-bit image of the double, descending -- sorted there by one workgroup and
 *    walked once; one with L <= CAP = 4096 goes to the second instance of the same kernel; a longer one (a dense upload
 *    makes L = m) goes through scratch and a segmented radix sort, in batches of whole cells in ascending order (each below
 *    2^31 entries and the scratch budget of 2^27 entries, 24 bytes each; a cell above the budget is a batch of its own).
 *    The walk finds both ends of a position's run at once, by binary search over the sorted keys, only for a gene that is
 *    in a set: the gene -> sets table (the transpose of the sets, built per call) is looked up first.
 *  - sets beyond the 1024 whose accumulators one pass holds in LDS are scored in further passes over the sorted cell.
 *  - there is NO team form and NO R shim entry. */
SGL_API int sgl_signature_scores(sgl_ctx* ctx, const int64_t* set_ptr, const int32_t* set_genes, int32_t n_sets, int32_t max_rank,
                                 uint64_t* rank2_out, double* score_out);
/* The one-shot form: its own context on the current device, A as a dgCMatrix; the argument refusals come before anything is
 * uploaded.  Neither uses nor touches the SINGLET_HIP_CACHE context. */
SGL_API int sgl_c_signature_scores(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol,
                                   const int64_t* set_ptr, const int32_t* set_genes, int32_t n_sets, int32_t max_rank,
                                   uint64_t* rank2_out, double* score_out);
/* What the last signature call (scores or sgl_op_cell_ranks) on this context ran: out[0] the cells sorted by the 1024-entry
 * LDS instance, out[1] by the 4096-entry one, out[2] the cells on the long path, out[3] the batches of the long path,
 * out[4] the set passes (0 for sgl_op_cell_ranks), and the caps in force: out[5] the LDS cap (stored non-zero entries),
 * out[6] the entries of a batch, out[7] the sets of a pass (0 for sgl_op_cell_ranks). */
SGL_API int sgl_signature_info(sgl_ctx* ctx, int64_t out[8]);

/* Factor annotation: which factors of a fit represent which levels of a metadata column (cell types, batches, donors) --
 * the reference's AnnotateNMF (R/AnnotateNMF.R:29-41, R/getDesigns.R, R/getModelMatrix.R, R/getModelFit.R,
 * R/getModelResults.R): for a factor-typed column the means model ~ 0 + column over the cells whose value is not NA, fitted
 * to every row of the embedding (or to every gene of the resident matrix, R/getModelFit.R:27), with the moderated t and the
 * log-odds of Smyth (2004, "Linear models and empirical Bayes methods for assessing differential expression in microarray
 * experiments").  The rules below are this library's own, stated in full; NO parity with limma is claimed (nothing here was
 * compared with it).  tests/annotate_restatement.py restates them in numpy and scipy.  OUT OF SCOPE: limma's robust = TRUE
 * (fitFDistRobustly) and trend = TRUE, arbitrary design matrices (designs =, ova = FALSE), a team form and an R shim entry.
 *
 * Labels.  labels[n], int32 in [-1, G), 1 <= G <= 1024: a cell labelled -1 is NA and left out of everything.  N = the
 * included cells, group_n[g] = the size of group g.  For a means model the fit needs three families of moments only.
 *
 * Embedding moments (sgl_group_moments).  F is k x n column-major on the host, or NULL for the H of the current fit, read in
 * place and untouched (k and n must then be the fit's); 1 <= k <= 1024.
 *  - sum[f, g], k x G column-major: the sum of F[f, c] over the cells of group g in EXACTLY sgl_group_means' summation order
 *    (the included cells of the group in ascending index, chunks of 256, slots, the binary tree, the chunk sums in chunk
 *    order; the same kernels run).  An empty group has sum = +0.0.
 *  - mean[f, g] = sum[f, g] / (double)group_n[g], one true division.
 *  - rss[f], k values: the sum over the included cells j of d * d, d = F[f, j] - mean[f, labels[j]]: one subtraction and one
 *    multiplication per cell, not contracted.  Order: inside a chunk as the group sums (slot s of S takes the positions
 *    s, s + S, ..., then the tree); then the chunk sums of ALL groups are added in ascending chunk order from +0.0 -- group
 *    0's chunks, then group 1's, and so on.  An empty group contributes nothing.
 *  - to first order, with u = 2^-53: |sum error| <= n_g u sum_g |x| (and far below it: chunks and trees shorten the chains to
 *    n_g / 256 + 256 / S + log2 S additions); |rss error| <= (N + 3) u rss + 2 sqrt(rss) sqrt(sum_j e_j^2), where e_j, the
 *    error of the mean the cell is compared with, is at most (n_g + 1) u mean_g |x|.
 *
 * Gene moments (sgl_gene_group_moments), over t(A) of the resident matrix, m genes:
 *  - nz[g, c] and sum[g, c], m x G column-major: exactly sgl_op_marker_sums with transform 0 (its code runs); a stored
 *    x == 0.0 of either sign joins the gene's implicit zeros, as it does there.  mean[g, c] = sum / (double)group_n[c].
 *  - rss[g] = E[g] + Z[g].  E[g]: the sum over the gene's stored non-zero entries in included cells of d * d,
 *    d = x - mean[g, c], in the segment / block order of the marker sums for a single accumulator: the entries in stored order
 *    are cut into segments of 8192, a segment into blocks of 64; a lane holds +0.0 for an excluded cell, a stored zero or a
 *    place past the end; ONE butterfly (v += v[lane ^ 32], 16, 8, 4, 2, 1) per block; the block sums are added in ascending
 *    order from +0.0 within a segment, the segment sums in ascending order from +0.0.  Skipping a block of zeros changes no bit.
 *    Z[g] = the sum over the non-empty groups c ascending, from +0.0, of (double)(group_n[c] - nz[g, c]) * (mean * mean): formed
 *    on the HOST inside the library.
 *  - 64-bit entry indexing; no 2^21-cell limit (nothing is cubed).  After sgl_upload_dense the call works, over the CSC image.
 *  - |E error| <= (8192 / 64 + 7 + segments + 2) u E + the mean term above; Z adds G + 2 roundings.
 *
 * Refusals and contract (both sides, and the whole calls below).  SGL_EINVAL, the whole list checked before anything is
 * launched: NULL labels; n_groups outside [1, 1024]; k outside [1, 1024]; a label outside [-1, G), the message naming
 * position and value; n outside [0, 2^31); F == NULL with k, n not the fit's.  SGL_ESTATE: on a team member, with an
 * all-reduce hook, on a context that holds a shard (gene side; embedding side with F == NULL), F == NULL without a fit, the
 * gene side without a resident matrix.  The context stays usable after every refusal.  Every call only reads: a fit continued
 * afterwards gives the bits it would have given without the call.  The kernels' time counts in the "scale" phase.  Any
 * output pointer may be NULL. */
SGL_API int sgl_group_moments(sgl_ctx* ctx, const double* F, int32_t k, int64_t n, const int32_t* labels, int32_t n_groups,
                              int64_t* group_n, double* sum, double* rss);
/* The one-shot form: its own context on the current device; F must not be NULL. */
SGL_API int sgl_c_group_moments(const double* F, int32_t k, int64_t n, const int32_t* labels, int32_t n_groups,
                                int64_t* group_n, double* sum, double* rss);
/* Keeps a copy of a host embedding F (k x n column-major) on the device for the annotation calls: while one is held,
 * F == NULL in sgl_group_moments and sgl_annotate reads IT (k and n must be its; it goes before the H of a fit), so the labels of
 * many metadata columns go against one upload.  F == NULL here drops it; a new call replaces it; sgl_destroy frees it.  The
 * fit and the matrix are not touched.  SGL_EINVAL for k outside [1, 1024] or n outside [1, 2^31) (nothing is held then). */
SGL_API int sgl_annotate_hold(sgl_ctx* ctx, const double* F, int32_t k, int64_t n);
SGL_API int sgl_gene_group_moments(sgl_ctx* ctx, const int32_t* labels, int32_t n_groups, int64_t* group_n, int64_t* nz,
                                   double* sum, double* rss);

/* The fit and the moderated statistics from the moments; host code (singlet_amd/csrc/annotate_host.h), needs no context and no
 * device.  sum is rows x G column-major (row fastest), rss has `rows` values.  Outputs, any may be NULL: coef, t, p_raw, p_adj,
 * lods rows x G; amean, sigma, s2_post `rows`; stdev_unscaled, var_prior G; scalars[4] = df_residual, s2_prior, df_prior, df_total.
 *
 * Fit.  G' = the non-empty groups; df = N - G', the same for every row.  grand[r] = the sum[r, g] added over g ascending from
 * +0.0; amean = grand / N; coef[r, g] = mean[r, g] - (center ? amean[r] : 0), one subtraction; stdev_unscaled[g] =
 * 1 / sqrt((double)group_n[g]); s2[r] = rss[r] / df; sigma = sqrt(s2).  With scale: tss[r] = rss[r] + the n_g (mean - amean)^2
 * added over the non-empty g ascending; sd = sqrt(tss / (N - 1)); coef /= sd; s2 /= sd * sd.  An empty group gives NaN in every
 * per-(r, g) output (and in its stdev_unscaled and var_prior) and is not counted by Benjamini-Hochberg.  df <= 0: NaN everywhere.
 *
 * Prior (Smyth 2004, section 6.2).  The usable rows have a finite s2 >= 0.  x = max(s2, 1e-5 median(s2)), a median of 0
 * replaced by 1; e = log x - digamma(df / 2) + log(df / 2); evar = the sample variance of e - trigamma(df / 2).  evar > 0:
 * df_prior = 2 trigamma^-1(evar), s2_prior = exp(mean e + digamma(df_prior / 2) - log(df_prior / 2)); otherwise df_prior = +Inf
 * and s2_prior = exp(mean e).  Fewer than two usable rows: df_prior = 0, s2_prior = NaN, no shrinkage.  s2_post = (df s2 +
 * df_prior s2_prior) / (df + df_prior), s2_prior when df_prior is infinite, s2 when it is 0 (NaN for a row that is not usable).
 * df_total = min(df + df_prior, usable rows * df).
 *
 * Moderated t and p.  t = coef / (stdev_unscaled * sqrt(s2_post)).  p_raw by tail: 0 (pos) P(T > t), 1 (neg) P(T < t), 2 (std)
 * 2 P(T > |t|), T Student's t with df_total degrees of freedom (real-valued; +Inf: the normal distribution).
 *
 * Log-odds (the B statistic with `proportion`, and coefficient standard deviation limits 0.1 and 4).  Per group g, over
 * the rows whose t is a number (rows' below is their count): the ntarget = ceil(proportion / 2 * rows') rows of largest |t|,
 * ties by row index, ranked i = 1 .. ntarget; pp = max(ntarget / rows', proportion); p0 = 2 P(T > |t|); ptarget_i =
 * ((i - 0.5) / rows' - (1 - pp) p0) / pp; where ptarget > p0, v0 = stdev_unscaled^2 ((|t| / q)^2 - 1) with q the upper
 * ptarget / 2 quantile of T, otherwise v0 = 0; v0 is clamped to [0.01, 16]; var_prior[g] = the mean of the ntarget values.
 * r = (stdev_unscaled^2 + var_prior) / stdev_unscaled^2; kernel = t^2 (1 - 1 / r) / 2 when df_prior > 1e6, else
 * (1 + df_total) / 2 * log((t^2 + df_total) / (t^2 / r + df_total)); lods = log(proportion / (1 - proportion)) - log(r) / 2 + kernel.
 *
 * p_adj: Benjamini-Hochberg over all values of p_raw that are not NaN, jointly over the table (before any filter).
 * The special functions are defined mathematically, not by an algorithm; tests/test_annotate_restatement.py holds them
 * against scipy, p_raw RELATIVELY down to 1e-300.  SGL_EINVAL: rows < 0, n_groups outside [1, 1024], a NULL input, a negative
 * group_n, proportion outside (0, 1), tail outside {0, 1, 2}. */
SGL_API int sgl_annotate_stats(int64_t rows, int32_t n_groups, const int64_t* group_n, const double* sum, const double* rss,
                               int center, int scale, double proportion, int tail, double* coef, double* stdev_unscaled,
                               double* amean, double* sigma, double* s2_post, double* scalars, double* var_prior, double* t,
                               double* p_raw, double* p_adj, double* lods);
/* The whole call: sgl_group_moments, then sgl_annotate_stats over the k rows.  F == NULL: the resident H. */
SGL_API int sgl_annotate(sgl_ctx* ctx, const double* F, int32_t k, int64_t n, const int32_t* labels, int32_t n_groups, int center,
                         int scale, double proportion, int tail, int64_t* group_n, double* sum, double* rss, double* coef,
                         double* stdev_unscaled, double* amean, double* sigma, double* s2_post, double* scalars,
                         double* var_prior, double* t, double* p_raw, double* p_adj, double* lods);
/* The one-shot form for a host F: its own context on the current device; the refusals come before a context is made. */
SGL_API int sgl_c_annotate(const double* F, int32_t k, int64_t n, const int32_t* labels, int32_t n_groups, int center, int scale,
                           double proportion, int tail, int64_t* group_n, double* sum, double* rss, double* coef,
                           double* stdev_unscaled, double* amean, double* sigma, double* s2_post, double* scalars,
                           double* var_prior, double* t, double* p_raw, double* p_adj, double* lods);
/* The same over the genes of the resident matrix: sgl_gene_group_moments, then sgl_annotate_stats over the m rows. */
SGL_API int sgl_annotate_genes(sgl_ctx* ctx, const int32_t* labels, int32_t n_groups, int center, int scale, double proportion,
                               int tail, int64_t* group_n, int64_t* nz, double* sum, double* rss, double* coef,
                               double* stdev_unscaled, double* amean, double* sigma, double* s2_post, double* scalars,
                               double* var_prior, double* t, double* p_raw, double* p_adj, double* lods);

/* Embedding neighbours: the EXACT n_neighbors nearest reference columns of every query column of a k x n embedding, by
 * brute force in FP64 -- the k-NN step of Seurat's FindNeighbors on the `nmf` reduction (its Jaccard step is sgl_c_snn), and
 * of label transfer after a projection.  The reference's package has no such function (it hands the embedding to Seurat);
 * the rules below are this library's own, stated in full; tests/embedding_knn_restatement.py restates them in numpy.
 *
 * R is k x n_ref and Q is k x n_query, column-major on the host (one column per cell).  R == NULL: the H of the current
 * fit, read where it lies on the device (k and n_ref must then be the fit's rank and cell count: SGL_EINVAL otherwise), in
 * the fit's stored factor order.  Q == NULL: the queries are the references themselves (n_query is not used beyond its sign).
 *  - distance: for query column q and reference column r, over the selected dimensions f in the listed order,
 *        s = +0.0;  for f:  t = q_f - r_f;  s = s + t * t
 *    in double, sequentially, without contraction (the product and the addition are two roundings).  s is a function of
 *    the two columns alone: it does not depend on tiling, on the launch or on which form of the call computed it.
 *  - ranking: by (s, reference index) ascending; ties go to the lower index.  The ranking is on the squared sum, not on its
 *    root (sqrt can merge two different sums).  With finite inputs no s is NaN; a sum that overflows to +Inf ties with every
 *    other +Inf and ranks by index.  This is a total order, so the result is the same however the references are cut into
 *    segments and merged.
 *  - output: idx_out int32, dist_out double, both n_neighbors x n_query column-major: column j holds the n_neighbors best
 *    references of query j in rank order, and __builtin_sqrt(s) of each (the IEEE root, as sgl_spatial_graph).  Either may
 *    be NULL.
 *  - self: with Q == NULL nothing is special-cased.  A cell is its own candidate at s = +0.0; it is in its result (first,
 *    unless identical columns of lower index tie with it) EXCEPT when n_neighbors or more identical columns precede it in
 *    index order: those fill the list at s = +0.0 before it.
 *  - dims: int32[n_dims], 0-based rows of R and Q, each in [0, k), no duplicates; NULL: all k rows in stored order (n_dims is
 *    not read).  One gather kernel writes the packed operands.
 *  - refused with SGL_EINVAL and a message, before anything is launched for the search: n_neighbors < 1, > 256 or > n_ref;
 *    k outside [1, 1024]; n_ref < 1 or >= 2^31; n_query < 0; n_dims outside [1, k], a dims entry out of range or repeated
 *    (named by position and value); a non-finite value in R, Q or the resident H: a device pass finds it, and the message
 *    names the array, the column and the row of the first one in column-major order.
 *  - refused with SGL_ESTATE: on a team member or with an all-reduce hook set (the shard's H is not the embedding; refused
 *    whatever R is); R == NULL without a fit.  The context stays usable after every refusal.
 *  - the call only reads the context; its temporaries are its own (the operands it uploads or gathers, and
 *    segments x n_neighbors x n_query candidates of 12 bytes).  A plain, a masked or a grouped-link fit continued after a
 *    call in mid-fit gives the bits it would have given without it.  The kernels' time counts in the "scale" phase when
 *    timing is on.
 *  - kernels (singlet_amd/csrc/kernels_knn.hip): a lane owns its queries; the references stream in ascending index and
 *    their coordinates reach the FP64 vector instructions as scalar operands.  n_dims <= 64 keeps the queries' coordinates
 *    in registers (instances 0 .. 3: n_dims up to 8, 16, 32 with two queries per lane, up to 64 with one); instance 4 serves
 *    every rank above.  The candidate lists live in LDS up to n_neighbors = 32, above in global scratch.  With fewer than
 *    1024 workgroups of queries the references are cut into up to 64 segments of at least max(1024, 4 n_neighbors)
 *    references, and a merge pass ranks the segments' candidates by (s, index).  64-bit offsets; no floating-point atomics. */
SGL_API int sgl_knn(sgl_ctx* ctx, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query,
                    const int32_t* dims, int32_t n_dims, int32_t n_neighbors, int32_t* idx_out, double* dist_out);
/* The one-shot form: its own context on the current device; R must not be NULL (SGL_EINVAL).  The argument refusals come
 * before a context is made. */
SGL_API int sgl_c_knn(const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query,
                      const int32_t* dims, int32_t n_dims, int32_t n_neighbors, int32_t* idx_out, double* dist_out);
/* What the last sgl_knn on this context ran (read-only, in the spirit of sgl_layout_get; all 0 before the first search):
 * out[0] the kernel instance (0 .. 4 above), [1] the reference segments, [2] the queries per workgroup, [3] 0 when the
 * candidate lists lay in LDS, 1 in global scratch.  A refused call leaves it as it was. */
SGL_API int sgl_knn_info(sgl_ctx* ctx, int64_t out[4]);

/* The same search under a metric: 0 Euclidean -- sgl_knn's own code, bit for bit --, 1 cosine, 2 correlation (Seurat's
 * RunUMAP defaults to metric = "cosine", and FindNeighbors offers it as annoy.metric: a column of H scales with the cell's
 * total signal, and Euclidean neighbours group cells by magnitude as much as by programme).  Everything not stated here is
 * as in sgl_knn: R / Q / dims, the refusals, the finiteness pass on the RAW operands with the same messages, the team and
 * hook refusal, the segments and their merge, and that the call only reads the context.  tests/knn_metric_restatement.py
 * restates the rules in numpy.  All arithmetic is FP64, every product and every addition its own rounding, everything
 * sequential in the listed order of the selected dimensions.
 *
 *  1. unit columns -- per column x of R and of Q, after dims has been applied, over the nd selected rows:
 *       correlation:  m = +0.0;  for f: m = m + x_f;  m = m / (double)nd;  y_f = x_f - m          cosine:  y = x
 *       s2 = +0.0;  for f: s2 = s2 + y_f * y_f;   nrm = sqrt(s2) (the IEEE root)
 *       u_f = y_f / nrm (an IEEE division, not a reciprocal multiply) when nrm != 0;   u_f = +0.0 for every f when nrm == 0
 *     Nothing else is special-cased.  An s2 that overflows gives nrm = +Inf and u_f = +-0; an s2 that underflows to 0 gives
 *     the zero column.  Such a column -- nrm == 0 or nrm == +Inf -- "has no direction"; it is not refused (cells with an
 *     all-zero h exist, and a constant column has no correlation), it is counted (sgl_knn_metric_info).  (Correlation only:
 *     a column whose plain sum overflows has m = +-Inf and a NaN unit column; its keys are NaN and its rank is not defined.
 *     That takes values above about 1.8e308 / nd.)
 *  2. key of a pair:  dot = +0.0;  for f: dot = dot + uq_f * ur_f;   key = 1.0 - dot;   key < 2^-40  ->  key = +0.0.
 *     The snap: for two bitwise-equal unit columns with a direction, |1 - dot| is the rounding of the rule itself, at most
 *     about (2 nd + 4) 2^-53 <= 2^-42 at nd = 1024 (measured on the CPU over nd = 1 .. 1024: 22 ulp of 1 for cosine, 182 for
 *     correlation, against the 4096 of the limit).  So a cell is at exactly +0.0 from itself, from its exact duplicates and
 *     from its copies scaled by a power of two; such pairs rank by index, as under sgl_knn, and the fuzzy graph's rho (the
 *     smallest distance > 0) skips them.  The guarantee covers bitwise-equal unit columns only: a pair that is parallel up
 *     to rounding gets what the rule gives (a correlation pair x, 3.7 x can land above the limit through the cancellation
 *     in the mean).  key is never negative and at most 2 + eps; a column without direction has key 1.0 to every column,
 *     itself included.
 *  3. ranking by (key, reference index) ascending, a total order; dist_out receives the key itself, not a root (uwot and
 *     umap-learn report 1 - cos the same way).  With Q == NULL nothing is special-cased by index.
 *
 *  - metric outside [0, 2]: SGL_EINVAL, "<entry>: metric = 7 is outside [0, 2]", after the argument refusals of sgl_knn and
 *    before anything is launched (sgl_c_knn_metric: before a context is made).
 *  - the unit columns are the call's own buffers (2 x 8 x nd x n bytes moved per operand); the resident H is never written.
 *  - kernels: knn_unit writes the packed unit operands in place of the gather, one sequential lane per column, the tile
 *    staged through LDS so that global memory is read and written in runs of 32 doubles; it counts the columns without
 *    direction with an integer atomic.  The scan kernels of sgl_knn have a second inner form: per (pair, dimension) v_mul_f64
 *    and v_add_f64 with the reference coordinate as the scalar operand -- two FP64 vector instructions where the Euclidean
 *    form issues three --, the key once per pair; candidates, lists, segments and merge are shared, and the merge takes no
 *    root.  A fused multiply-add form is deliberately not built: the rule is uncontracted arithmetic.  With timing on, the
 *    scan and merge count in the "scale" phase as under sgl_knn, and knn_unit alone in the "gram" phase. */
SGL_API int sgl_knn_metric(sgl_ctx* ctx, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query,
                           const int32_t* dims, int32_t n_dims, int32_t n_neighbors, int32_t metric, int32_t* idx_out,
                           double* dist_out);
SGL_API int sgl_c_knn_metric(const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query,
                             const int32_t* dims, int32_t n_dims, int32_t n_neighbors, int32_t metric, int32_t* idx_out,
                             double* dist_out);
/* out[0 .. 3] as sgl_knn_info; [4] the metric of the last search on this context (a plain sgl_knn: 0); [5] the number of
 * columns without direction among its operands -- the columns of R, plus those of Q when Q was given; 0 for Euclidean.  A
 * refused call leaves it as it was. */
SGL_API int sgl_knn_metric_info(sgl_ctx* ctx, int64_t out[6]);

/* Approximate embedding neighbours: an inverted-file search.  A coarse k-means over the embedding cuts the references into
 * n_lists lists, and every query scans only the n_probe lists whose centroids are nearest to it; inside those lists the sums,
 * the keys and the ranking are exactly sgl_knn's / sgl_knn_metric's.  (Seurat's FindNeighbors and RunUMAP default to annoy, an
 * approximate index; the exact scan is quadratic in the cells.)  The exact search stays the default everywhere.  Every sum
 * below has one stated order, so the result is one function of the inputs; tests/knn_ivf_restatement.py restates the rules in
 * numpy.  The rules are this library's own.
 *
 *  - operands: exactly those of sgl_knn_metric.  R, Q and dims are gathered to packed columns; the finiteness pass runs on the
 *    RAW operands with sgl_knn's messages; for metric 1 and 2 the operands are the unit columns of sgl_knn_metric, rule 1.
 *    R == NULL: the resident H (k, n_ref must be the fit's); Q == NULL: the queries are the references themselves.
 *  - the coarse quantiser always works on these operands with the EUCLIDEAN sum of sgl_knn, s = +0.0; s = s + t * t with
 *    t = x_f - c_f, sequential over the dimensions, uncontracted -- for every metric.  Only the final ranking uses the
 *    metric's key.  "Nearest centroid" is the least (s, centroid index): sgl_knn's ranking with the centroids as references.
 *  - training set: T = min(n_ref, 64 n_lists) training cells; training cell t is reference floor(t n_ref / T) in 64-bit
 *    integers (every cell trains when n_ref <= 64 n_lists).  No seed, no hash.
 *  - seeds: centroid g starts as training cell floor(g T / n_lists).
 *  - Lloyd step, n_iter times (0 allowed): every training cell goes to its nearest centroid; every centroid becomes the mean
 *    of its cells in the summation order sgl_group_means documents (group = list, over the training positions in ascending
 *    order, rank = n_dims): the sum, then one division by the count.  A centroid that received no cell keeps its value.
 *    Empty lists are legal: two equal seeds leave the one of higher index empty for as long as the two centroids stay equal
 *    (always with n_iter = 0; through every step when the cells of the lower one are all copies of it and their mean is exact).
 *  - lists: after training every reference -- all n_ref, not only the training cells -- goes to its nearest centroid.  A list
 *    holds its members in ascending cell index.
 *  - probes: a query probes the n_probe centroids nearest to it.
 *  - result: among the members of the probed lists, the n_neighbors best by the metric's own (key, cell index) rule --
 *    sgl_knn's sum for metric 0, sgl_knn_metric's 1 - dot with its snap to +0.0 for 1 and 2.  Layout, and the root for
 *    metric 0, as in sgl_knn.  A query whose probed lists hold fewer than n_neighbors cells gets idx = -1, dist = +Inf in the
 *    remaining slots; such queries are counted (sgl_knn_ivf_info).
 *  - consequences: the result does not depend on tiling, on batching or on which form of the call computed it; with
 *    n_probe == n_lists it equals sgl_knn / sgl_knn_metric bit for bit (a list streams in ascending cell index, a candidate
 *    goes behind every entry whose key is not greater, and the merge of the probe slots ranks by (key, cell index)).
 *  - refused with SGL_EINVAL and a message naming the value and its range, after sgl_knn's own argument refusals and before
 *    anything is launched (the one-shot form: before a context is made), in this order: n_lists outside
 *    [1, min(n_ref, 65536)]; n_probe outside [1, min(n_lists, 64)] (64 is the width of the merge pass); n_iter outside
 *    [0, 1000]; metric outside [0, 2].  SGL_ESTATE exactly where sgl_knn gives it.  The context stays usable after every
 *    refusal.  The call only reads the context: a fit continued after a search in mid-fit gives the bits it would have given.
 *  - kernels (singlet_amd/csrc/kernels_knn_ivf.hip; host rules in knn_ivf_host.h): operands, assignment passes and probe
 *    selection are the kernels of sgl_knn with the centroids as references; the centroid update is sgl_group_means' kernel
 *    pair; the list offsets, the table from list position to cell and the task table -- the (query, probe slot) pairs sorted
 *    stably by probed list, cut into blocks of 64 x queries-per-lane pairs that never cross a list edge -- are built on the
 *    host, one kernel copies the packed references into list order; knn_scan_lists gives one wave a block of pairs that share
 *    a list: a lane owns its pairs' queries (registers up to n_dims = 64, the instance families of sgl_knn), the list's
 *    members stream in stored order with their coordinates and cell index as scalar operands, candidate lists in LDS up to 32
 *    neighbours and in global scratch above; a sibling of knn_finish merges the n_probe slots and writes the padding as
 *    -1 / +Inf.  The candidates are n_probe x n_neighbors x queries x 12 bytes: the queries go in batches that keep them
 *    below 1 GiB, and batching cannot change a bit.  No floating-point atomics; 64-bit offsets.  With timing on the list
 *    scan, its merge and the centroid updates (as sgl_group_means books them) count in the "scale" phase, knn_unit in "gram". */
SGL_API int sgl_knn_ivf(sgl_ctx* ctx, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query,
                        const int32_t* dims, int32_t n_dims, int32_t n_neighbors, int32_t metric, int32_t n_lists,
                        int32_t n_probe, int32_t n_iter, int32_t* idx_out, double* dist_out);
/* The one-shot form: its own context on the current device; R must not be NULL (SGL_EINVAL). */
SGL_API int sgl_c_knn_ivf(const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query, const int32_t* dims,
                          int32_t n_dims, int32_t n_neighbors, int32_t metric, int32_t n_lists, int32_t n_probe,
                          int32_t n_iter, int32_t* idx_out, double* dist_out);
/* What the last inverted-list search on this context ran (sgl_knn_ivf or sgl_op_ivf_search; all 0 before the first; a
 * refused call leaves it as it was): out[0] n_lists, [1] n_probe, [2] the training cells T (0 after sgl_op_ivf_search, which
 * trains nothing), [3] the shortest and [4] the longest list, [5] the empty lists, [6] the queries that came back short,
 * [7] the kernel instance of the list scan (0 .. 4 as sgl_knn_info). */
SGL_API int sgl_knn_ivf_info(sgl_ctx* ctx, int64_t out[8]);
/* With timing on (sgl_set_timing), the milliseconds the stages of the last inverted-list call took: out[0] operands, [1]
 * Lloyd steps, [2] final assignment, [3] bucketing, [4] probes, [5] task table, [6] list scan, [7] merge.  [5] is host work
 * and read from the host clock; the others lie between two events on the stream and include the copies of their stage. */
SGL_API int sgl_knn_ivf_stage_ms(sgl_ctx* ctx, double out[8]);
/* The training alone: centroids_out n_dims x n_lists column-major, assign_out int32[n_ref] the list of every reference.
 * Refusals as sgl_knn_ivf (there is no n_probe, no n_neighbors and no Q). */
SGL_API int sgl_op_ivf_train(sgl_ctx* ctx, const double* R, int32_t k, int64_t n_ref, const int32_t* dims, int32_t n_dims,
                             int32_t metric, int32_t n_lists, int32_t n_iter, double* centroids_out, int32_t* assign_out);
/* The search under the caller's centroids (n_dims x n_lists, finite) and assignment.  Any assignment with entries in
 * [0, n_lists) is valid, including ones no training produces; the first offender is refused with position and value
 * (SGL_EINVAL), after the argument refusals above.  query_batch = 0: the automatic batches; positive: that many queries per
 * pass; negative: SGL_EINVAL. */
SGL_API int sgl_op_ivf_search(sgl_ctx* ctx, const double* R, int32_t k, int64_t n_ref, const double* Q, int64_t n_query,
                              const int32_t* dims, int32_t n_dims, int32_t n_neighbors, int32_t metric,
                              const double* centroids, int32_t n_lists, const int32_t* assign, int32_t n_probe,
                              int64_t query_batch, int32_t* idx_out, double* dist_out);

/* Neighbour index and transfer: the references of a search kept on the device between calls, and the step that consumes a
 * search of new cells against them -- labels and values of the reference cells transferred to the query cells (projection of
 * new cells onto a trained w, then "what are they": the counterpart of ProjectData followed by Seurat's TransferData /
 * MapQuery).  The one-shot searches upload, pack, train and bucket the references in every call; the index pays that once.
 * One index per context; no team form, no R shim entry.
 *
 * The index is what sgl_knn_ivf has after its bucketing stage, kept instead of dropped:
 *  - method 1 (inverted lists) keeps the packed references in list order, the table from list position to cell, the list
 *    offsets, the centroids, the dims, the metric and n_dims; method 0 (exact) keeps the packed (unit) references of
 *    sgl_knn_metric.  Everything else the build allocates -- the raw upload, for method 1 the packed references in stored
 *    order and the training buffers -- is released before it returns.
 *  - build: R, k, n_ref, dims, n_dims and metric are exactly sgl_knn_metric's, with its refusals and messages; R == NULL takes
 *    the resident H.  The index is a SNAPSHOT: it holds its own packed copy; a fit continued afterwards, a new upload or a
 *    subset neither changes it nor is changed by it.  method outside [0, 1]: SGL_EINVAL.  n_lists and n_iter follow
 *    sgl_knn_ivf's rules and refusals; method 0 does not read them.  A second build replaces the first (a refused one leaves
 *    it); the annotations of the replaced index go with it.  sgl_destroy frees the slot.  Team members and contexts with an
 *    all-reduce hook are refused as by sgl_knn (SGL_ESTATE).
 *  - search: Q is k x n_query with the build's k, and the build's dims are applied to it.  Q == NULL: SGL_EINVAL (a search of the
 *    references among themselves stays with the one-shot calls).  The finiteness pass runs on the raw Q with sgl_knn's message.
 *    n_neighbors in [1, min(256, n_ref)]; for method 1 n_probe in [1, min(n_lists, 64)], free to differ from search to search,
 *    and query_batch as in sgl_op_ivf_search; method 0 reads neither.  n_query == 0: SGL_OK, nothing is written.  Without an
 *    index: SGL_ESTATE.  The scan and merge count in the "scale" phase and knn_unit in "gram"; sgl_knn_info,
 *    sgl_knn_metric_info, sgl_knn_ivf_info and sgl_knn_ivf_stage_ms stay as they were.
 *  - the contract: for method 1 the result is bit for bit that of sgl_knn_ivf with the same R, Q, dims, metric, n_lists,
 *    n_probe, n_iter and n_neighbors; for method 0 bit for bit that of sgl_knn / sgl_knn_metric -- for any number of searches
 *    in any order against one index, whatever the batching.
 *  - info: out[0] 1 when an index is present (all 0 otherwise), [1] method, [2] metric, [3] k, [4] n_dims, [5] n_ref, [6] n_lists,
 *    [7] training cells, [8] shortest and [9] longest list, [10] empty lists ([6] .. [10]: 0 for method 0), [11] bytes resident
 *    (the kept arrays above plus the annotations), [12] searches served since the build (sgl_knn_index_search and
 *    sgl_knn_index_map calls that returned SGL_OK, those with n_query == 0 included), [13] the queries and [14] the short
 *    queries of the last of them, [15] the kernel instance of its scan (0 .. 4 as sgl_knn_info).  A refused call leaves the
 *    report as it was. */
SGL_API int sgl_knn_index_build(sgl_ctx* ctx, const double* R, int32_t k, int64_t n_ref, const int32_t* dims, int32_t n_dims,
                                int32_t metric, int32_t method, int32_t n_lists, int32_t n_iter);
SGL_API int sgl_knn_index_search(sgl_ctx* ctx, const double* Q, int64_t n_query, int32_t n_neighbors, int32_t n_probe,
                                 int64_t query_batch, int32_t* idx_out, double* dist_out);
/* Releases the index and its annotations; SGL_OK also when there is none. */
SGL_API int sgl_knn_index_drop(sgl_ctx* ctx);
SGL_API int sgl_knn_index_info(sgl_ctx* ctx, int64_t out[16]);

/* The transfer.  The rules are this library's own; tests/knn_transfer_restatement.py restates them in numpy and the device
 * holds them bit for bit.  Everything is FP64; every product, quotient and sum is its own rounding (the unit is compiled with
 * -ffp-contract=off); every sum is sequential over the slots in rank order, from +0.0.
 *
 * For one query, the slots i = 0 .. n_neighbors - 1 of its neighbour list (idx_i, d_i) are valid where idx_i >= 0; the
 * padding (-1 / +Inf) follows the valid slots.
 *  - weights.  weighting 0: w_i = 1.0.  weighting 1, the distance-weighted vote of Dudani (1976): with d_first and d_last the
 *    distances of the first and of the last valid slot, w_i = (d_last - d_i) / (d_last - d_first) when d_last is finite and
 *    d_last > d_first; otherwise every w_i = 1.0.  The nearest neighbour weighs 1 and the farthest 0; a single neighbour, or
 *    neighbours all at one distance, vote equally.
 *  - labels.  s_c = the sum of w_i over the valid slots whose reference has label c; W = the sum over the valid slots whose
 *    reference has any label (>= 0).  With W > 0: scores[c] = s_c / W, pred = the class of the largest score, ties to the
 *    lowest class, best = that score.  Otherwise -- no valid slot, none labelled, only zero-weight slots labelled --: every
 *    score +0.0, pred = -1, best = +0.0.  scores_out is n_classes x n_query column-major, pred_out int32[n_query],
 *    best_out double[n_query].
 *  - values.  Wv = the sum of w_i over all valid slots; values[f] = (the sum over the valid slots of w_i * V[f, idx_i]) / Wv;
 *    with no valid slot a quiet NaN.  values_out is n_values x n_query column-major.
 *
 * sgl_knn_index_annotate puts onto the index labels (int32[n_ref], every entry in [-1, n_classes), -1: the cell has no label;
 * n_classes in [1, 65536]) and / or V (n_values x n_ref column-major, finite; n_values in [1, 1024]: layout coordinates, any
 * per-cell covariate).  Either may be NULL and is then left as it is.  The arrays stay resident with the index.
 * sgl_knn_index_map is one search, in batches, with the transfer of every batch run on the device: the neighbour lists do not
 * travel to the host and back.  Q, n_neighbors and n_probe as sgl_knn_index_search.  Any output may be NULL; asking for
 * pred / best / scores without labels on the index, or for values without V, is SGL_ESTATE.  It equals sgl_knn_index_search
 * followed by sgl_op_knn_transfer bit for bit.
 * sgl_op_knn_transfer is the stage operator on the caller's idx / dist (n_neighbors x n_query column-major, as the searches
 * write them; n_neighbors in [1, 256]) and the caller's annotations (an output asked for without its annotation: SGL_EINVAL).
 *  - refused with SGL_EINVAL and a message naming the value and its range, before anything is launched: weighting outside
 *    [0, 1]; n_classes or n_values out of range; a label out of range (position and value); a non-finite V (column and row of
 *    the first one in column-major order); for the operator an idx entry outside [-1, n_ref), or a valid slot behind a padding
 *    slot (column, slot and value).  After every refusal the index and the context stay usable and no output has been written.
 *  - kernel (singlet_amd/csrc/kernels_knn_transfer.hip; host rules in knn_transfer_host.h): one wave per query; the wave
 *    stages the query's slots (cell, label, weight) in LDS once; lanes own the classes lane, lane + 64, ... and walk the slots
 *    in rank order, so every sum is owned by one lane from start to end; the arg-max is a wave reduction on (score, class) by
 *    comparisons alone; for the values lanes own the rows and read 64 consecutive doubles of column idx_i at a time.  No
 *    floating-point atomics; 64-bit offsets; the time counts in the "scale" phase. */
SGL_API int sgl_knn_index_annotate(sgl_ctx* ctx, const int32_t* labels, int32_t n_classes, const double* V, int32_t n_values);
SGL_API int sgl_knn_index_map(sgl_ctx* ctx, const double* Q, int64_t n_query, int32_t n_neighbors, int32_t n_probe,
                              int32_t weighting, int32_t* idx_out, double* dist_out, int32_t* pred_out, double* best_out,
                              double* scores_out, double* values_out);
SGL_API int sgl_op_knn_transfer(sgl_ctx* ctx, const int32_t* idx, const double* dist, int32_t n_neighbors, int64_t n_query,
                                int64_t n_ref, const int32_t* labels, int32_t n_classes, const double* V, int32_t n_values,
                                int32_t weighting, int32_t* pred_out, double* best_out, double* scores_out, double* values_out);

/* Clustering: a deterministic multi-level Louvain modularity optimiser on a neighbour graph -- the step after
 * find_neighbors (Seurat's FindClusters on the SNN graph).  The reference's package has no clustering code (it hands the
 * graph to Seurat, whose optimiser visits the vertices in a seeded random order), so the rules below are this library's own,
 * stated in full; tests/louvain_restatement.py restates them in numpy and the device holds them bit for bit.  No parity of
 * labels with Seurat is claimed.  One-shot on the current device; no team form, no R shim entry.
 *
 * Input: G is an n x n dgCMatrix (Gx, Gi, Gp): rows ascending within a column, weights finite and >= 0, pattern and values
 * symmetric (A_ij and A_ji both stored, with the same bits; the output of sgl_c_snn qualifies: its Jaccard index is one
 * division of commutative integer sums).  A diagonal entry is a self-loop, counted once.
 *  - refused with SGL_EINVAL and a message, before anything is uploaded: n < 0; n_res < 1 or a NULL resolutions; a resolution
 *    that is not finite or not > 0 (named by position); tol < 0 or NaN; max_sweeps outside [1, 1024]; max_levels outside
 *    [1, 32]; Gp[0] != 0 or a decreasing Gp (the column is named); a NULL array of a graph with entries.
 *  - refused with SGL_EINVAL by a device pass, with a message that names the column and the row of the first defective entry
 *    in column-major order: a row outside [0, n), a row not above the one before it in its column, a weight that is not
 *    finite, a negative weight.  A graph without such an entry goes through a second pass that names the first entry in
 *    column-major order whose mirror A_ji is missing or differs in its bits.  Then S (below) is computed: S = 0 (an all-zero
 *    graph, one without entries included) and an S that overflows are refused.  The library stays usable after every refusal.
 *  - n = 0: an empty result and no levels, nothing is read.
 *  - the graph is uploaded and validated once for all n_res resolutions; the outputs of resolution r lie at labels + r n,
 *    n_clusters + r, n_levels + r, q_levels + 32 r, sweeps_levels + 32 r.  Any output may be NULL.
 *
 * Quantities of one level (its graph A with n vertices, labels comm[], gamma = the resolution), every sum in ONE order that
 * depends on the graph and the labels alone -- never on the launch shape, never on a floating-point atomic -- every product
 * and addition its own rounding (the unit is compiled with -ffp-contract=off):
 *  - "sequential": from +0.0, the terms one after the other.  "blocked": the terms in their stated order are cut into blocks
 *    of 1024 consecutive terms; every block is summed sequentially, and the block sums are summed sequentially in ascending
 *    block order (so a million-term sum is not one serial chain, and up to 1024 terms it IS the sequential sum).
 *  - k_v = the sequential sum of column v in ascending row, the diagonal included.  S = the blocked sum of k_v, v ascending.
 *    Every level computes k and S from its own graph.
 *  - own_v = the sequential sum, in ascending row, of the entries A_jv of column v with comm[j] == comm[v] (the diagonal
 *    is one of them).  tot_c = the blocked sum of k_v, in_c = the blocked sum of own_v, over the members v of c ascending.
 *  - term_c = in_c / S - (gamma * (tot_c / S)) * (tot_c / S), evaluated in that order (+0.0 for an id without members), and
 *    Q = the blocked sum of term_c over the ids c = 0 .. n-1 ascending.
 *
 * One synchronous sweep: every vertex reads the labels, tot and the community sizes of the sweep's start.  For vertex v
 * with own community o = comm[v] the candidates are o and every community among its off-diagonal neighbours; for each,
 *     w_c  = the sequential sum of A_jv over j != v with comm[j] == c, in ascending j (w_o = +0.0 without such a j),
 *     g(c) = w_c - ((gamma * k_v) * (c == o ? tot_c - k_v : tot_c)) / S,       evaluated in that order.
 * best = the candidate of maximal g, ties to the lowest id.  v moves to best only if best != o and g(best) > g(o) strictly,
 * and -- the swap rule -- not when o and best both hold a single vertex and best > o (of two singletons that prefer each
 * other only the higher-numbered moves; without the rule they would swap for ever).  A vertex with no off-diagonal
 * neighbour never moves.
 *
 * One level: the labels start as comm[v] = v, Q is computed, then sweeps follow under the guard.  After a sweep Q' is
 * computed from the new labels: Q' <= Q (a sweep that moved nothing included): the sweep is discarded and the level's moving
 * phase ends; Q' - Q <= tol: the sweep is kept and the phase ends; otherwise it is kept and the phase continues, up to
 * max_sweeps sweeps.  So Q never decreases and the number of sweeps is bounded whatever the data.  (Synchronous moves can
 * lower Q where many gains tie, as on unweighted lattices: the guard then ends the phase early -- DESIGN.md "Clustering".)
 *
 * Aggregation: the ids that survive a level are renumbered in ascending order; the next level's graph has one vertex per
 * community and A'_cd = the blocked sum of A_uv over u in c, v in d in column-major order of the fine entries (v ascending,
 * then u); self-loops carry the intra-community weight.  A coarse graph need not be bitwise symmetric: nothing reads a row.
 * The optimiser stops after a level that kept no sweep, or after max_levels levels.
 *
 * Output per resolution: labels int32[n], clusters numbered by descending size, ties by smallest member, 0 the largest;
 * n_clusters; n_levels = the levels run (the last one that kept no sweep included); q_levels[32]: Q at the end of each
 * level's moving phase; sweeps_levels[32]: the sweeps KEPT at each level; entries past n_levels are 0.
 *
 * Kernels (singlet_amd/csrc/kernels_cluster.hip; the host logic without HIP in cluster_host.h): the sweep sorts the keys
 * (community << 32 | position in the column) of a vertex so that a community's entries become one run in ascending row --
 * one wave per vertex in LDS for columns of up to 512 stored entries (the fast path), a segmented radix sort in HBM and one
 * 256-thread workgroup per vertex above (the slow path; coarse levels produce such hubs).  tot, in, Q and the member lists
 * come from a stable radix sort of the vertices by label; the coarse graph from a stable radix sort of the entries by
 * (column community, row community).  64-bit offsets; integer atomics only (the move count, the first defect). */
SGL_API int sgl_c_louvain(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* resolutions,
                          int32_t n_res, double tol, int32_t max_sweeps, int32_t max_levels, int32_t* labels,
                          int32_t* n_clusters, int32_t* n_levels, double* q_levels, int32_t* sweeps_levels);
/* Stage operator: ONE sweep on G from labels_in (each in [0, n); any partition, not only a level's start) at one
 * resolution -> labels_out, Q of labels_in, Q of labels_out, the number of moved vertices.  It makes no guard decision.  G
 * goes through the first validation pass and the S rule only: a coarse graph, which need not be symmetric, is a valid
 * input.  Outputs may be NULL. */
SGL_API int sgl_op_louvain_sweep(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const int32_t* labels_in,
                                 double resolution, int32_t* labels_out, double* q_in, double* q_out, int64_t* moved_out);
/* What the last sgl_c_louvain or sgl_op_louvain_sweep of this process ran: out[0] the widest column (stored entries) of the
 * fast path in this build; [1] the vertices that took the slow path at level 0, [2] at later levels (each summed over the
 * call's resolutions); [3] the coarse-graph build path: 0 none was built, 1 the global radix sort.  A call refused before
 * its first sweep leaves [1] .. [3] as they were. */
SGL_API int sgl_louvain_info(int64_t out[4]);

/* Layout: the 2-D (or up to 8-D) picture of the cells -- the last step of the vignette's pipe, RunUMAP(reduction = "nmf"):
 * the fuzzy neighbour graph of the k-NN lists, then a force-directed layout of it.  The reference's package has no layout
 * code (it hands the embedding to Seurat / uwot), and the published optimiser is racy (hogwild SGD) and sequential per edge,
 * so the rules below are this library's own: a SYNCHRONOUS, OWNER-COMPUTES form of it, stated in full;
 * tests/umap_restatement.py restates them in numpy.  Every result is one function of its inputs.  No parity of coordinates
 * with uwot or umap-learn is claimed (DESIGN.md "Layout").  One-shot on the current device; no team form, no R shim entry.
 * All arithmetic is FP64, every product and addition its own rounding (the unit is compiled with -ffp-contract=off).
 *
 * 1. sgl_c_fuzzy_graph.  Input: what sgl_knn returns for n cells: idx int32 and dist double (the roots; or the keys of sgl_knn_metric), both K x n
 * column-major (the list of cell j at idx + j K, ranked ascending).  The cell itself is usually first in its list, but not
 * when K identical columns precede it.  Output: an n x n dgCMatrix, rows ascending within a column, no diagonal, pattern and
 * values bitwise symmetric (what sgl_c_louvain demands), in the two calls of sgl_c_snn: i_out == NULL counts (p_out and
 * *nnz_out are filled), the second call gets i_out / x_out of at least cap >= *nnz_out entries.  rho_out / sigma_out
 * (double[n], may be NULL) receive rho and sigma.
 *  - own list of cell j: its K candidates without the one whose index is j, if present, in list order.
 *  - rho_j = the smallest distance > 0 of the own list, 0 when there is none.
 *  - sigma_j: bisection on psum(s) = the sum over the own list, in list order from +0.0, of
 *    (d - rho_j > 0 ? exp(-(d - rho_j) / s) : 1.0), against log2(K).  lo = 0, hi = +Inf, mid = 1; a step: psum(mid) > log2(K)
 *    sets hi = mid and mid = (lo + hi) / 2; otherwise lo = mid, and mid = 2 mid while hi is infinite, else (lo + hi) / 2.
 *    EXACTLY 64 steps, no early exit (the bracket is then below an ulp, so an ulp of exp cannot send two implementations
 *    down different branches for long).  Then sigma_j = max(mid, 1e-3 * mean), mean = (the sum of the own list's distances in
 *    list order from +0.0) / (their number) when rho_j > 0, else the mean of all n K input distances: their blocked sum in
 *    memory order (blocks of 1024 consecutive terms, as in Clustering) / (n K).
 *  - membership p_ji = 1.0 when d_ji - rho_j <= 0, else exp(-(d_ji - rho_j) / sigma_j).
 *  - w_ij = (p_ij + p_ji) - p_ij * p_ji with an absent direction read as +0.0: the sum and the product commute, so the
 *    result is bitwise symmetric.  Entries equal to 0 are dropped.
 *  - refused with SGL_EINVAL and a message, on the host, before anything is launched and with every output untouched: K
 *    outside [2, 256]; n outside [1, 2^31); and, named by cell and place, the first of: an index outside [0, n), an index
 *    repeated in its list, a distance that is not finite, a negative distance, a distance below the one before it.  A graph of
 *    2^31 entries or more is refused after the count, outputs untouched.
 *  - kernels (singlet_amd/csrc/kernels_umap.hip; the host logic without HIP in umap_host.h): one thread per cell computes
 *    rho, sigma and the memberships; the incoming lists come from a counting transpose (integer histogram, scan, cursor
 *    fill); one wave per vertex sorts the keys of its own and incoming entries in LDS, up to 512 keys per vertex (the LDS
 *    merge); a vertex with more (a hub: the in-degree is unbounded) takes the fallback, a segmented radix sort in HBM.
 *    Integer atomics only.
 *
 * 2. sgl_c_umap_layout.  Input: a graph G as above -- validated on the host: rows in [0, n) and ascending within a column,
 * weights finite and >= 0; symmetry is NOT required; a diagonal entry is skipped (it never fires) -- Y0 (dim x n
 * column-major, finite, dim in [1, 8]); a, b finite and > 0; n_epochs in [1, 2^20]; alpha0 finite and > 0; neg_rate in
 * [0, 255]; seed.  n in [1, 2^31).  Anything else is SGL_EINVAL with a message, before anything is launched.  Output: Y
 * (dim x n).  The positions live in two buffers that swap per epoch: an epoch reads the positions of its start only.
 *  - firing: r_e = w_e / w_max, one division, w_max the exact maximum stored weight.  Entry e fires in epoch t (1-based) iff
 *    floor(t * r_e) > floor((t - 1) * r_e): stateless, and an edge below w_max / n_epochs never fires.  w_max == 0: Y = Y0.
 *  - head and tail: column j is the head, the stored row i the tail; only the head moves (a symmetric graph stores the other
 *    direction too).
 *  - a term of head j against a point o: d_f = y_j,f - y_o,f; d2 = the sum of d_f * d_f over f ascending from +0.0;
 *    p = d2 when b == 1.0 exactly, else pow(d2, b).  Attractive (o = the tail): c = (m2ab * (p / d2)) / (a * p + 1.0) with
 *    m2ab = -2.0 * a * b, when d2 > 0; else the term is +0.0.  Repulsive (o = a negative sample m):
 *    c = tb / ((0.001 + d2) * (a * p + 1.0)) with tb = 2.0 * b.  Component f of the term is fmin(fmax(c * d_f, -4.0), 4.0).
 *    A repulsive term with d2 == 0 and m != j has all components +4.0; a sample with m == j contributes +0.0.
 *  - negative samples of a firing entry: for s = 0 .. neg_rate - 1, u = rand(seed, e, 256 t + s) -- the hash of the mask,
 *    e the entry's position in Gx -- and m = ((u >> 32) * (uint64) n) >> 32: integers only.
 *  - orders: g_e = attractive + neg_0 + ... + neg_last, sequentially; delta_j = the sequential sum of g_e over the firing
 *    entries of column j in stored order, from +0.0; y_j' = y_j + alpha_t * delta_j, a product then an addition, with
 *    alpha_t = alpha0 * (1.0 - (t - 1) / n_epochs).  A vertex without a firing entry keeps the bits of y_j.
 *  - kernel: one launch per epoch, one wave per vertex; the column is taken in steps of 64 stored entries, a ballot compacts
 *    the firing entries and the (entry, term) pairs are spread over the lanes, so only firing entries pay for pow; lane
 *    f < dim adds component f in the stated order and carries the sums from step to step (no slow path for wide columns).
 *    Instances: 2 * (0: dim 2, 1: dim 3, 2: the generic loop up to 8) + (1 when b == 1.0).  Each y is written once; no
 *    floating-point atomics.
 *  - what holds: with b == 1.0 no transcendental is left and the device equals the restatement bit for bit; otherwise the
 *    two differ by the ulps of pow. */
SGL_API int sgl_c_fuzzy_graph(const int32_t* idx, const double* dist, int64_t n, int32_t K, int32_t* p_out, int64_t* nnz_out,
                              int32_t* i_out, double* x_out, int64_t cap, double* rho_out, double* sigma_out);
SGL_API int sgl_c_umap_layout(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* Y0, int32_t dim,
                              double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, double* Y);
/* Stage operator: ONE epoch t in [1, n_epochs] from the positions Yin -> Y, with the layout's validation and rules. */
SGL_API int sgl_op_umap_epoch(const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t n, const double* Yin, int32_t dim,
                              double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed, int32_t t,
                              double* Y);
/* What the last calls of this process ran: out[0] the layout's kernel instance (-1 before the first layout), [1] the widest
 * column (stored entries) and [2] the vertices that needed more than one step of 64 entries in the last sgl_c_umap_layout
 * or sgl_op_umap_epoch; [3] the vertices of the last sgl_c_fuzzy_graph that took the LDS merge's fallback.  A refused call
 * leaves them as they were. */
SGL_API int sgl_umap_info(int64_t out[4]);

/* Layout transform: query cells placed in the FIXED layout of a reference -- the picture of Seurat's MapQuery / ProjectUMAP,
 * umap-learn's transform, uwot's umap_transform.  The reference positions do not move, negative samples are reference points,
 * only the query moves: a query's trajectory depends on that query and the reference alone, never on another query.  So the
 * result is ONE function of (query, reference), bit for bit, whatever the batching, and all epochs of a query run inside one
 * kernel launch with the position in registers.  The rules are this library's own, stated in full below and restated in numpy
 * in tests/umap_transform_restatement.py; no parity of coordinates with uwot or umap-learn is claimed (DESIGN.md "Layout
 * transform").  FP64 throughout, every product, quotient and sum its own rounding (the unit is compiled with
 * -ffp-contract=off); no floating-point atomics.
 *
 * Input of one query q: its neighbour list against the reference, (idx_s, d_s) for s = 0 .. K-1, as the searches write it:
 * idx int32 and dist double, both K x n_query column-major (the list of query q at idx + q K), ascending, padding -1 / +Inf
 * behind the valid slots (a slot is padding iff its index is -1; its distance is not read).  K in [1, 256].  The own list is
 * the valid slots, ALL of them: a query is not a reference, so nothing is removed.
 *  - memberships: rho and sigma follow sgl_c_fuzzy_graph's rules on the own list, word for word -- rho = the smallest
 *    distance > 0, else 0; the bisection of EXACTLY 64 steps against log2(K); psum sequential in list order from +0.0 -- with
 *    one difference: sigma = max(mid, 1e-3 * mean) with mean ALWAYS the own list's mean (the sum of its distances in list order
 *    from +0.0 / their number).  There is no global mean: it would make one query depend on the others.  (When rho == 0 every
 *    distance is 0, every membership is 1.0 and sigma is never read.)  w_s = 1.0 when d_s - rho <= 0, else
 *    exp(-(d_s - rho) / sigma); a padding slot gets +0.0.  There is no symmetrisation: the graph is bipartite.  Consequence:
 *    every non-empty list holds a membership of exactly 1.0 (its first slot: d_0 <= rho).
 *  - start: y0_f = (sum_s w_s * Yref[f, idx_s]) / (sum_s w_s), both sums sequential in slot order over the valid slots from
 *    +0.0.
 *  - firing: r_s = w_s (the list's maximum is exactly 1.0, so sgl_c_umap_layout's division by w_max is the identity and is
 *    not performed).  Slot s fires in epoch t (1-based) iff floor(t * w_s) > floor((t - 1) * w_s).
 *  - terms: the layout's attractive and repulsive terms, clip and constants unchanged; the head is the query's position, the
 *    other point a reference position: Yref[:, idx_s] for the attractive term, Yref[:, m] for a negative sample.  There is
 *    no m == j exclusion: a sample is a reference and never the query.  A repulsive term with d2 == 0 has every component
 *    +4.0; b == 1.0 exactly skips pow.
 *  - negative samples of firing slot s: for i = 0 .. neg_rate - 1, u = rand(seed, 256 * (query_offset + q) + s, 256 * t + i)
 *    -- the hash of the mask -- and m = ((u >> 32) * (uint64) n_ref) >> 32.  query_offset is the global index of the call's
 *    first query (the same device as the global cell index in the mask hash of the sharded fit): with it, a batch cut out of
 *    a larger call reproduces that call's rows.
 *  - orders and update: the layout's.  g_s = attractive + the samples in order; delta = the g_s of the firing slots in slot
 *    order from +0.0; y' = y + alpha_t * delta, alpha_t = alpha0 * (1.0 - (t - 1) / n_epochs).  A query without a firing slot
 *    in an epoch keeps the bits of y.
 *  - a query with no valid slot: rho = sigma = +0.0, y0 and y are a quiet NaN (the transfer's rule for values); it is counted
 *    in sgl_umap_transform_info.  The stage operator does not read (or check) its column of Yin.
 *  - refused on the host, before anything is launched, with a message naming value and range and every output untouched
 *    (SGL_EINVAL): K outside [1, 256]; dim outside [1, 8]; n_epochs outside [1, 2^20]; neg_rate outside [0, 255]; alpha0, a
 *    or b not finite or not > 0; n_ref outside [1, 2^31); n_query < 0; not 1 <= t_first <= t_last <= n_epochs; query_offset
 *    < 0 or query_offset + n_query above 2^55; and, named by query and slot, the first of: an index outside [-1, n_ref), a
 *    valid slot behind a padding slot, an index repeated in its list, a distance of a valid slot that is not finite, negative
 *    or below the one before it; a non-finite Yref or Yin; a W of a valid slot outside [0, 1].  n_query == 0 returns SGL_OK
 *    and writes nothing.
 *  - kernels (singlet_amd/csrc/kernels_umap_transform.hip; the host logic without HIP in umap_transform_host.h).  Memberships:
 *    one thread per query (the serial order of psum forbids a wave reduction).  Transform: one wave per query; the wave
 *    stages its slots (reference index, membership) in LDS once and keeps y in registers, every lane holding the current y;
 *    per epoch a ballot compacts the firing slots in steps of 64, the (slot, term) pairs are spread over the lanes, the
 *    clipped terms go through LDS to lane f < dim, which adds them in the stated order, and y' is published to the wave; y
 *    is written to memory once, at the end of the launch.  The host cuts the epochs of a call into launches of at most 128
 *    epochs (the profiling switch SGL_UMAP_TRANSFORM_EPOCHS_PER_LAUNCH in the environment asks for fewer, 1 .. 128); the
 *    result does not depend on the cut.  Instances as the layout's: 2 * (0: dim 2, 1: dim 3, 2: the generic
 *    loop up to 8) + (1 when b == 1.0).
 *  - what holds: rho is bit for bit the restatement's; sigma and W differ from it by the ulps of the device's exp; from
 *    given W the epochs with b == 1.0 equal the restatement bit for bit, otherwise to the ulps of pow.
 *
 * sgl_c_fuzzy_query: the lists -> W (K x n_query), rho, sigma (double[n_query]); any output may be NULL.
 * sgl_c_umap_transform: the lists and Yref (dim x n_ref column-major, finite) -> Y0_out (the start) and Y_out (after n_epochs
 * epochs), each dim x n_query; either may be NULL.
 * sgl_op_umap_transform_epochs, the stage operator: the epochs t_first .. t_last from the caller's W (K x n_query) and Yin
 * (dim x n_query) -> Y_out.  Epochs 1 .. s followed by s + 1 .. n from its result equal 1 .. n.
 * sgl_knn_index_set_layout puts Yref (dim x n_ref of the index, finite) onto the neighbour index of the context, resident
 * with it: replaced by a second call, dropped with the index and by a rebuild, counted in sgl_knn_index_info's resident
 * bytes.  SGL_ESTATE without an index.
 * sgl_knn_index_project is one search in batches (Q, n_neighbors, n_probe, query_batch as sgl_knn_index_search), with
 * memberships, start and transform run on the device for every batch: the lists do not travel to the host and back.  It
 * equals sgl_knn_index_search followed by sgl_c_umap_transform (query_offset 0) bit for bit, for both index methods and any
 * query_batch.  Outputs idx, dist (K x n_query), Y0, Y (dim x n_query); any may be NULL.  SGL_ESTATE without an index or
 * without a layout.
 * sgl_umap_transform_info: what the last sgl_c_umap_transform, sgl_op_umap_transform_epochs or sgl_knn_index_project of this
 * process ran: out[0] the transform kernel's instance (-1 before the first), [1] the widest list (valid slots), [2] the
 * queries without a valid slot, [3] the launches of the transform kernel.  A refused call leaves them as they were. */
SGL_API int sgl_c_fuzzy_query(const int32_t* idx, const double* dist, int64_t n_query, int32_t K, int64_t n_ref, double* W_out,
                              double* rho_out, double* sigma_out);
SGL_API int sgl_c_umap_transform(const int32_t* idx, const double* dist, int64_t n_query, int32_t K, const double* Yref, int32_t dim,
                                 int64_t n_ref, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate, uint64_t seed,
                                 int64_t query_offset, double* Y0_out, double* Y_out);
SGL_API int sgl_op_umap_transform_epochs(const int32_t* idx, const double* W, int64_t n_query, int32_t K, const double* Yref, int32_t dim,
                                         int64_t n_ref, const double* Yin, double a, double b, int32_t n_epochs, double alpha0,
                                         int32_t neg_rate, uint64_t seed, int64_t query_offset, int32_t t_first, int32_t t_last,
                                         double* Y_out);
SGL_API int sgl_knn_index_set_layout(sgl_ctx* ctx, const double* Yref, int32_t dim);
SGL_API int sgl_knn_index_project(sgl_ctx* ctx, const double* Q, int64_t n_query, int32_t n_neighbors, int32_t n_probe,
                                  int64_t query_batch, double a, double b, int32_t n_epochs, double alpha0, int32_t neg_rate,
                                  uint64_t seed, int32_t* idx_out, double* dist_out, double* Y0_out, double* Y_out);
SGL_API int sgl_umap_transform_info(int64_t out[4]);

/* Gene set enrichment: which gene sets are enriched at the top of each factor's loadings -- the reference's RunGSEA
 * (R/RunGSEA.R), one pre-ranked enrichment test per factor and gene set.  The enrichment score is the weighted
 * Kolmogorov-Smirnov statistic of GSEA in the form fgsea's calcGseaStat computes it (exponent 1); the p-values come from a
 * permutation null of random gene sets of the same size (the scheme of fgseaSimple), drawn from the library's counter hash.
 * The rules below are stated in full; tests/gsea_restatement.py restates them in numpy, the textbook walk over all genes and
 * a calibration on random sets are the independent yardsticks.  NO parity with fgseaMultilevel's seeded sampler is
 * claimed, and p-values below 1 / (nperm + 1) are not resolved.  The result is one function of (w, sets, score type, nperm,
 * seed): tiling, batching and device do not change one bit.
 *
 * Inputs.  w: m genes x k factors, column-major doubles, finite, any sign.  The P gene sets as set_ptr[P + 1] (int64,
 * set_ptr[0] = 0) and set_genes[] (int32, 0-based): set j holds set_genes[set_ptr[j] .. set_ptr[j + 1]).  score_type: 0 pos
 * (RunGSEA's default), 1 neg, 2 std.  nperm >= 1.  seed (uint64).
 *
 * Ranking of factor f.  The genes are ordered by w[g, f] descending; ties (the zeros an L1 fit leaves; -0.0 counts as 0.0)
 * go by gene index ascending.  pos_f[g] = the 0-based position of gene g.  This tie rule replaces RunGSEA's add.noise.
 *
 * Score of a set S of s genes in factor f.  The hits are taken in position order, p_0 < ... < p_{s-1}, with the weights
 * a_i = |w| of the gene at p_i.  THE PREFIX SUMS cum_i follow one order: the hits are cut into blocks of 64 consecutive
 * hits; within a block the Kogge-Stone ladder: for d = 1, 2, 4, 8, 16, 32 every lane l >= d adds the previous step's value
 * of lane l - d, all lanes at once (a lane past the last hit holds +0.0), giving L_l; the block carry C starts at +0.0;
 * cum of lane l = C + L_l; then C = C + L_63 (the block's last prefix).  NR = cum_{s-1}.
 *   top_i = cum_i / NR - (double)(p_i - i) / (double)(m - s);   bottom_i = top_i - a_i / NR;
 * IEEE divisions, no contraction.  When NR == 0 (every hit has weight zero) fgsea's rule holds: cum_i / NR becomes
 * (double)(i + 1) / (double)s and a_i / NR becomes 1.0 / (double)s.  ES_pos = max top (>= 0), ES_neg = min bottom (<= 0);
 * std gives the one larger in magnitude, and +0.0 when they are equal in magnitude.
 *
 * Null.  key(r, g) = rand(seed, r, g), the reference's hash (src/singlet.cpp:30-64), r in [0, nperm).  The null set of size
 * s of permutation r = the s genes smallest by (key, g): the sets of one permutation are nested and the same for every
 * factor.  null[f, s, r] = the score (of the call's score type) of that set in factor f, for every distinct size s among
 * the tested sets.
 *
 * Tallies (integers) and statistics (on the host inside the library, gsea_host.h).  For every (set j, factor f), over the
 * nulls of its size: n_ge = #{null >= ES}, n_le = #{null <= ES}; per (size, factor): #{null >= 0}, #{null <= 0} and the
 * sums of the nulls >= 0 and of the nulls <= 0, each added in ascending r, sequentially, from +0.0 -- the running sum is
 * carried across the batches.  The side of a score: the nulls >= 0 for pos, the nulls <= 0 for neg, for std those >= 0
 * when ES >= 0 and those <= 0 otherwise; n_side = their number.
 *   p:  pos (1 + n_ge) / (1 + nperm);  neg (1 + n_le) / (1 + nperm);  std (1 + n_ge or n_le of the side) / (1 + n_side).
 *   NES = ES / |sum of the side / n_side|, NaN when the side is empty or its mean is 0.
 *   padj: Benjamini-Hochberg per factor over its P sets: the p in ascending order, rank i = 1 .. n;
 *         padj of rank i = min(1, min over i' >= i of ((double)n / (double)i') * p of rank i'); a NaN p is left out.
 *
 * sgl_c_gsea: one-shot, its own context on the current device; neither uses nor touches the SINGLET_HIP_CACHE context.
 * Outputs, P x k column-major (set fastest), ANY pointer may be NULL: es, nes, pval, padj, n_ge, n_le, n_side; set_size[P];
 * info[5] as sgl_gsea_info lays it out; stage_ms[5] = the device time of the five stages (rankings, observed scores, null
 * sample, null scores, tallies) by events, which costs a wait per stage and batch.  batch: permutations per batch, 0 = by
 * the memory budget of k x sizes x batch x 8 bytes (256 MiB); the results do not depend on it.
 *  - refused with SGL_EINVAL before anything is uploaded or launched, the message names the offender: a NULL w, set_ptr or
 *    set_genes; k outside [1, 1024]; m < 2; n_sets < 1; a score type outside {0, 1, 2}; nperm outside [1, 2^20]; a
 *    negative batch; a non-finite w; set_ptr not starting at 0 or not ascending; an empty set; a set of size >= m; a set
 *    above the LDS cap of 4096 genes (RunGSEA's max.size is 500); a gene outside [0, m); a gene twice in one set.
 *  - the kernels: a segmented radix sort per factor for the rankings; ONE WAVE per (set, factor) sorts the set's positions
 *    in LDS and scores them; a segmented radix sort of the m keys of every permutation, of which the s_max smallest are
 *    kept; ONE WAVE per (permutation, factor) sorts the s_max sampled positions once and, for every distinct size,
 *    compacts the members by a ballot and scores them; integer tallies per (set, factor) and (size, factor).
 *  - there is NO team form and NO R shim entry; fgseaMultilevel, leading-edge genes and exponents other than 1 are not
 *    offered. */
SGL_API int sgl_c_gsea(const double* w, int32_t m, int32_t k, const int64_t* set_ptr, const int32_t* set_genes, int32_t n_sets,
                       int score_type, int32_t nperm, uint64_t seed, int32_t batch, double* es, double* nes, double* pval,
                       double* padj, int64_t* n_ge, int64_t* n_le, int64_t* n_side, int32_t* set_size, int64_t* info,
                       double* stage_ms);
/* What the last enrichment call on this context ran: out[0] the sets, out[1] the distinct sizes, out[2] s_max, out[3] the
 * batches of permutations, out[4] the permutations per batch (sgl_op_gsea_es: sets and s_max; sgl_op_gsea_null: the rest). */
SGL_API int sgl_gsea_info(sgl_ctx* ctx, int64_t out[5]);

/* Cell graph of c_gcnmf for the current fit (after sgl_fit_init, which drops
 * it again; all-NULL slots clear it).  G is an n x n dgCMatrix, n = the cells of
 * the resident matrix; an invalid G is SGL_EINVAL with a message.  While it is
 * set, sgl_step_h convolves its right-hand sides over G and solves every cell,
 * and sgl_step_w accumulates over t(A) against H G and solves every gene (the
 * rules of sgl_c_gcnmf); the convolution's time counts in the rhs_h / rhs_w
 * phases.  Edges cross shards: the ranks of a one-process team take the graph
 * of the whole matrix through sgl_multi_set_graph (section 2b) and exchange a
 * halo; on a rank's own context, with an all-reduce hook, after a dense upload
 * and next to link matrices a graph is refused (SGL_EINVAL), and the masked
 * steps / sgl_ard_run refuse while one is set. */
SGL_API int sgl_set_graph(sgl_ctx* ctx, const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t G_nrow,
                          int32_t G_ncol);

/* Collective hook for cell-sharded runs.  Called with a device pointer to
 * `count` doubles that must be summed in place over all shards.  Ordering:
 * after sgl_set_stream(ctx, S) the buffer is produced and consumed by kernels
 * on S, so the hook enqueues its collective on S (or a stream ordered against
 * S) and returns without a host sync.  Without sgl_set_stream the context runs
 * on a private stream: the library then synchronises it before the call, and
 * the hook must have completed its writes when it returns.  NULL = one shard. */
typedef int (*sgl_allreduce_fn)(void* user, void* dev_ptr, int64_t count);
SGL_API int sgl_set_allreduce(sgl_ctx* ctx, sgl_allreduce_fn fn, void* user);
/* The hook may be installed or cleared at any time, before or after sgl_fit_init: what depends on it
 * (the per-gene non-zero counts over all shards, which decide the W columns predict() skips,
 * src/singlet.cpp:340) is rebuilt through the new hook at the next W-update. */

/* Step-level operators (what c_nmf_base's loop body is made of).  A sharded
 * host runs them in this order per iteration; sgl_nmf_run does the same
 * internally.
 *   sgl_step_h      predict(A, w, h, L1_h, L2_h)    src/singlet.cpp:650
 *   sgl_step_scale_h  scale(h, d)  (all-reduces k row sums if sharded)  :651
 *   sgl_step_w      predict(At, h, w, L1_w, L2_w)   :654  (all-reduces the
 *                   k x nrow right-hand sides and the k x k Gram if sharded)
 *   sgl_step_scale_w  scale(w, d); tol = cor(w, w_prev)  :655-659
 * sgl_step_begin snapshots w_it = w (:648). */
SGL_API int sgl_step_begin(sgl_ctx* ctx);
SGL_API int sgl_step_h(sgl_ctx* ctx, double L1, double L2);
SGL_API int sgl_step_scale_h(sgl_ctx* ctx);
SGL_API int sgl_step_w(sgl_ctx* ctx, double L1, double L2);
SGL_API int sgl_step_scale_w(sgl_ctx* ctx, double* tol_out);
/* The masked half-iterations c_ard_nmf_base's loop body is made of (src/singlet.cpp:1104, :1106):
 *   sgl_step_h_masked   predict_mask(A, seed, inv_density, w, h, L1, L2, threads, false)    :436-466
 *   sgl_step_w_masked   predict_mask(At, seed, inv_density, h, w, L1, L2, threads, true)
 * on the resident fit of a single shard (the sharded masked loop is sgl_ard_run / sgl_multi_ard_run); the hash sees
 * the shard's global cell index (cell_offset), as in the reference's chunked form (:485).  sgl_ard_run runs
 * sgl_step_begin, sgl_step_h_masked, sgl_step_scale_h, sgl_step_w_masked, sgl_step_scale_w per iteration. */
SGL_API int sgl_step_h_masked(sgl_ctx* ctx, double L1, double L2, uint64_t seed, uint64_t inv_density);
SGL_API int sgl_step_w_masked(sgl_ctx* ctx, double L1, double L2, uint64_t seed, uint64_t inv_density);

/* Whole loops on the resident shard. */
SGL_API int sgl_nmf_run(sgl_ctx* ctx, double tol, int32_t maxit,
                double L1_w, double L1_h, double L2_w, double L2_h,
                int32_t* n_iter, double* tol_trace, const sgl_callbacks* cb);
SGL_API int sgl_ard_run(sgl_ctx* ctx, double tol, int32_t maxit, double L1, double L2,
                uint64_t seed, uint64_t inv_density, double overfit_threshold, int32_t trace_test_mse,
                double* test_mse, int32_t* iter, double* tol_out, double* score_overfit, int32_t* n_trace,
                int32_t* n_iter, const sgl_callbacks* cb);
/* One H-update against a fixed, already scaled W (the body of c_project_model). */
SGL_API int sgl_project_run(sgl_ctx* ctx, double L1, double L2);

/* Results of the current fit: w k x nrow, d k, h k x ncol_local (any may be NULL). */
SGL_API int sgl_get_factors(sgl_ctx* ctx, double* w, double* d, double* h);
/* Overwrite the current factors (warm start / tests).  Any may be NULL. */
SGL_API int sgl_set_factors(sgl_ctx* ctx, const double* w, const double* d, const double* h);

/* One ALS iteration (src/singlet.cpp:648-659) on a context, whatever its exchange: none (one shard),
 * the all-reduce hook (the five steps above) or a native team (section 2b).  *tol = cor(w, w_prev). */
SGL_API int sgl_nmf_iterate(sgl_ctx* ctx, double L1_w, double L1_h, double L2_w, double L2_h, double* tol);

/* ------------------------------------------------------------------------
 * 2b. Native multi-GPU: cells sharded over the GPUs of one node, the exchange done by the library
 *     itself over RCCL / xGMI (no hook, no launcher, nothing for the R side to do).  Per iteration:
 *     ONE grouped collective -- reduce-scatter of the k x genes right-hand sides of the W-update by
 *     gene blocks + all-reduce of [k x k Gram of h | k row sums of h], all taken from the UNSCALED h
 *     (they commute with scale(h, d), src/singlet.cpp:651) -- then every rank solves its block of
 *     genes and the blocks of w are all-gathered.  W, d and tol come out identical on all ranks.
 *     Results equal the one-GPU fit to rounding (the scaling is applied after the sums).
 *     Limits: c_nmf, c_linked_nmf, c_ard_nmf and (one-process team only) c_gcnmf; no dense front-end; k as for one GPU.
 *     RCCL is loaded at run time (librccl.so.1; SGL_RCCL_PATH overrides); SGL_ECOMM if absent.
 * ---------------------------------------------------------------------- */
/* (a) ONE process drives all devices -- the form an R session uses.  sgl_c_nmf itself takes this
 *     path (and sgl_c_ard_nmf its masked counterpart) when the environment variable SINGLET_NGPU
 *     is set to a number > 1.
 *     devices: ndev device ids (NULL: 0 .. ndev-1), all distinct -> RCCL (ncclCommInitAll); all
 *     equal -> the ranks share one device and exchange through a HIP kernel (test configuration). */
typedef struct sgl_multi sgl_multi;
SGL_API int sgl_multi_create(int ndev, const int* devices, sgl_multi** out);
SGL_API int sgl_multi_destroy(sgl_multi* m);
SGL_API int sgl_multi_size(const sgl_multi* m);
/* rank's context, owned by m (for timing / layout queries; do not destroy). */
SGL_API int sgl_multi_ctx(sgl_multi* m, int rank, sgl_ctx** out);
/* Whole matrix in, cells split into contiguous blocks of (nearly) equal non-zero count; the transposed
 * shards are built on the devices. */
SGL_API int sgl_multi_upload_csc(sgl_multi* m, const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol);
SGL_API int sgl_multi_synth_csc(sgl_multi* m, uint64_t S, uint64_t inv_density, const double* levels16, int32_t ngenes,
                                int64_t ncells_total);
SGL_API int sgl_multi_fit_init(sgl_multi* m, int32_t k, const double* w_init, uint64_t synth_seed);
/* c_linked_nmf on the team: the link matrices of the WHOLE matrix (arguments as sgl_set_links); link_h's columns follow
 * their cells to the ranks.  Call after sgl_multi_fit_init.  (One process per GPU: sgl_set_links on the rank's context with
 * the columns of link_h that belong to its cells.) */
SGL_API int sgl_multi_set_links(sgl_multi* m, const double* link_h, int32_t link_h_rows, int32_t link_h_cols,
                                const double* link_w, int32_t link_w_rows, int32_t link_w_cols);
/* sgl_set_links_grouped on the team: group_h holds one id per cell of the WHOLE matrix and is dealt out with the cells, as
 * sgl_multi_set_links deals out the columns of link_h; the tables and group_w go to every rank, whose gene block reads
 * group_w from its first gene on.  Both lists are checked before any rank is touched. */
SGL_API int sgl_multi_set_links_grouped(sgl_multi* m, const double* table_h, int32_t rows_h, int32_t groups_h, const int32_t* group_h,
                                        const double* table_w, int32_t rows_w, int32_t groups_w, const int32_t* group_w);
/* sgl_group_means of the H of the team's fit (group: one id per cell of the whole matrix): every rank sums its own cells
 * in the order sgl_group_means defines for its block, the host adds the rank partials in rank order and divides by the
 * counts over all ranks.  Equal to the one-context means to the rounding of the different order (same first-order
 * bound); the counts are exact.  SGL_ESTATE without a fit. */
SGL_API int sgl_multi_group_means(sgl_multi* m, const int32_t* group, int32_t n_groups, double* means, int64_t* counts);
/* sgl_evaluate on the team's fit (cell_loss: all cells of the whole matrix in global order; mse divides by nrow * all
 * cells).  Every rank, on its own thread, computes the losses of its cells, their sum in sgl_evaluate's order over its
 * block, and -- when gene_loss is asked for -- the UNCLAMPED partial of every gene over its own cells; no collective is
 * needed, every rank holds the same w and d.  The host adds the ranks' cell sums in rank order for sse, and adds the gene
 * partials in rank order, then clamps.  Equal to the one-context result to the rounding of the different order (the same
 * first-order bound); exact on inputs whose sums are exact.  SGL_ESTATE without a matrix or a fit.  Process-per-GPU
 * teams (sgl_comm_init_rank) have no such call: sgl_evaluate refuses on their contexts. */
SGL_API int sgl_multi_evaluate(sgl_multi* m, double* sse, double* mse, double* cell_loss, double* gene_loss);
/* c_gcnmf on the team (src/singlet.cpp:1668-1730): the cell graph of the WHOLE matrix (arguments, checks and messages as
 * sgl_set_graph; all-NULL slots clear it; sgl_multi_fit_init drops it).  Rank r keeps the columns of its own cells.  The
 * rows of those columns that name another rank's cells are that rank's "exports"; E = the longest export list of the
 * team.  Per iteration and side every rank packs its exported columns of the k x cells operand -- the right-hand sides B
 * of the H-update (gcnmf_update_h, :1668-1690), the unscaled h of the W-update (gcnmf_update_w, :1693-1710; the row
 * scaling commutes with the convolution) -- into its block of a slab of team size x E x k doubles, ONE in-place all-gather
 * of k x E doubles per rank fills the other blocks (phase comm), and the convolution reads [own block of cells | slab].
 * Sums keep the stored order of every column, so the fit equals the one-GPU sgl_c_gcnmf to the rounding of the team path.
 * With E = 0 (no edge crosses a rank boundary) no halo step is issued.  Refused next to link matrices, after a dense
 * upload and by sgl_multi_ard_run.  The process-per-GPU team (sgl_comm_init_rank) still refuses a graph: its ranks do
 * not know each other's cell blocks. */
SGL_API int sgl_multi_set_graph(sgl_multi* m, const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t G_nrow,
                                int32_t G_ncol);
/* out[0..4] = entries of G, entries whose row lives on another rank than their column, E, sum of the export list lengths,
 * bytes one rank contributes to one halo all-gather (8 k E); all 0 without a graph. */
SGL_API int sgl_multi_graph_info(sgl_multi* m, int64_t* out);
/* The plan behind sgl_multi_set_graph, host only (no device is touched): for an n x n graph (row indices Gi, offsets Gp)
 * and the n_ranks + 1 block boundaries cell_lo, export_ptr[0 .. n_ranks] / export_idx (room for n entries) receive every
 * rank's export list (global cell indices, ascending), Gi_local (may be NULL; as long as Gi) the rewritten row indices --
 * row - cell_lo[r] for a row of the column's own rank r, n_local_r + s * E + (position in rank s's export list) for a row
 * owned by rank s -- and info[0..3] = entries, crossing entries, E, sum of the export list lengths. */
SGL_API int sgl_graph_halo_plan(const int32_t* Gi, const int32_t* Gp, int32_t n, int n_ranks, const int64_t* cell_lo,
                                int32_t* Gi_local, int64_t* export_ptr, int32_t* export_idx, int64_t* info);
SGL_API int sgl_multi_iterate(sgl_multi* m, double L1_w, double L1_h, double L2_w, double L2_h, double* tol);
SGL_API int sgl_multi_nmf_run(sgl_multi* m, double tol, int32_t maxit, double L1_w, double L1_h, double L2_w, double L2_h,
                              int32_t* n_iter, double* tol_trace, const sgl_callbacks* cb);
/* c_ard_nmf_base on the team (arguments as sgl_ard_run).  The W-update needs, per gene, sums over ALL cells of
 * the right-hand side and of the Gram downdate over the cells masked for that gene: one grouped collective
 * reduce-scatters [k x genes | k x k x genes] by gene blocks (600 MB at k = 50, 30 000 genes -- as a
 * reduce-scatter each rank moves (N-1)/N of it once) and all-reduces the k x k Gram; mse_test adds one
 * all-reduced double per trace.  scale(h, d) keeps the reference's order (k row sums all-reduced first). */
SGL_API int sgl_multi_ard_run(sgl_multi* m, double tol, int32_t maxit, double L1, double L2,
                              uint64_t seed, uint64_t inv_density, double overfit_threshold, int32_t trace_test_mse,
                              double* test_mse, int32_t* iter, double* tol_out, double* score_overfit, int32_t* n_trace,
                              int32_t* n_iter, const sgl_callbacks* cb);
/* w k x nrow, d k, h k x ncol (all cells, in matrix order); any may be NULL. */
SGL_API int sgl_multi_get_factors(sgl_multi* m, double* w, double* d, double* h);
/* (b) one process per GPU (torch.distributed.run, MPI ...): rank 0 makes an id, the host broadcasts
 *     its SGL_COMM_ID_BYTES bytes, every rank joins with its context BEFORE sgl_fit_init.  The
 *     collectives run on the context's stream; sgl_nmf_iterate / sgl_nmf_run then do the team
 *     iteration.  The communicator is destroyed with the context. */
#define SGL_COMM_ID_BYTES 128
SGL_API int sgl_comm_unique_id(void* id);
SGL_API int sgl_comm_init_rank(sgl_ctx* ctx, int nranks, int rank, const void* id);
/* sgl_comm_init_rank is collective (it blocks until all nranks have joined), so a rank that cannot bind RCCL must be
 * found BEFORE anyone calls it: every rank calls sgl_comm_available (no communication; 0 or SGL_ECOMM; path_out, may
 * be NULL, receives the library name that was opened -- SGL_RCCL_PATH in the environment names it, e.g. the librccl
 * the host process has already loaded), the host agrees on the result, and only then all ranks join. */
SGL_API int sgl_comm_available(char* path_out, int path_len);
/* What the library's own communicator of this context reports: *nranks = ncclCommCount (the team size for ranks that
 * share a device; 1 without a team), *is_rccl = 1 when the exchange runs over RCCL, path_out = the RCCL library bound. */
SGL_API int sgl_comm_info(sgl_ctx* ctx, int32_t* nranks, int32_t* is_rccl, char* path_out, int path_len);
/* The cell split sgl_multi_upload_csc uses: lo[0..n] boundaries of n contiguous blocks of (nearly) equal non-zero
 * count, each at least one cell (p = the dgCMatrix p slot, ncol + 1 entries; ncol >= n).  Host only. */
SGL_API int sgl_split_cells_by_nnz(const int32_t* p, int32_t ncol, int n, int64_t* lo);

/* ------------------------------------------------------------------------
 * 3. Single operators, exposed for the parity tests (each is one kernel
 *    family of the path) and for profiling.
 * ---------------------------------------------------------------------- */
/* rng::rand(i, j) (src/singlet.cpp:47-64) for n (i, j) pairs, on the device. */
SGL_API int sgl_op_rand(sgl_ctx* ctx, uint64_t state, const uint64_t* i, const uint64_t* j, int64_t n, uint64_t* out);
/* draw(cell, gene, inv_density) (src/singlet.cpp:91-95) for the block
 * cells [cell0, cell0+ncells) x genes [0, ngenes): out[c * ngenes + g]. */
SGL_API int sgl_op_mask(sgl_ctx* ctx, uint64_t state, uint64_t inv_density, int64_t cell0, int32_t ncells, int32_t ngenes,
                uint8_t* out);
/* AAt (src/singlet.cpp:200-206): G = F F^T (+1e-15 on the diagonal), F k x cols. */
SGL_API int sgl_op_gram(sgl_ctx* ctx, const double* F, int32_t k, int64_t cols, double* G);
/* The per-column Gram downdate of predict_mask (src/singlet.cpp:458-463): for the columns c in [0, ncols)
 * out[c] (k x k) = G - (AAt(F[:, idx_c]) + 1e-15 I), idx_c = the rows r in [0, nrow) with draw(...) true
 * (mask_t = 0: draw(cell = c + col_offset, gene = r + row_offset); 1: draw(cell = r + row_offset, gene = c + col_offset));
 * G = NULL: the plain sum AAt(F[:, idx_c]) without ridge (the partial a shard contributes).  F is nrow x k row-major
 * (k x nrow column-major).  use_lists = 0: the rows are hashed inside the kernel; 1: from the mask lists built first. */
SGL_API int sgl_op_mask_gram(sgl_ctx* ctx, const double* F, const double* G, int32_t k, int32_t nrow, int64_t ncols, uint64_t seed,
                uint64_t inv_density, int mask_t, int64_t col_offset, int64_t row_offset, int use_lists, double* out);
/* Right-hand sides of predict (src/singlet.cpp:341-343) for the resident
 * shard: which = 0: B = F * A (F k x nrow, B k x ncol); which = 1: B = F * At;
 * which = 2 / 3: the same two products through the LDS-tiled kernel (k <= 128) that the
 * fit uses, instead of the plain CSC kernel. */
SGL_API int sgl_op_rhs(sgl_ctx* ctx, int which, const double* F, int32_t k, double* B);
/* nnls (src/singlet.cpp:229-250) on ncols independent columns sharing G:
 * B k x ncols (destroyed on the device, not written back), X k x ncols in/out. */
SGL_API int sgl_op_nnls(sgl_ctx* ctx, const double* G, const double* B, double* X, int32_t k, int64_t ncols,
                double L1, double L2, int32_t* sweeps_out);
/* Rebuild the resident t(A) from A on the device, sorting at most max_batch_entries non-zeros at a time (0: the default,
 * 2^31 - 1; a column with more entries than the cap is a batch of its own).  Any cap gives the same t(A); a small one
 * sends a small matrix through many batches, as a matrix past 2^31 non-zeros goes.  A running fit is dropped. */
SGL_API int sgl_op_transpose(sgl_ctx* ctx, int64_t max_batch_entries);
/* scale (src/singlet.cpp:219-225) and cor (:184-197). */
SGL_API int sgl_op_scale(sgl_ctx* ctx, double* F, int32_t k, int64_t cols, double* d);
SGL_API int sgl_op_cor(sgl_ctx* ctx, const double* x, const double* y, int64_t n, double* out);
/* The graph convolution of c_gcnmf (src/singlet.cpp:1684-1688) over the graph set by sgl_set_graph:
 * Y(:, j) = sum over column j of G, in stored order, of G(r, j) * X(:, r); X, Y k x n column-major, n = the cells of the
 * resident matrix.  Needs a fit of rank k with a graph (SGL_ESTATE without one, SGL_EINVAL for another k); the fit's
 * factors are not touched.  Refused (SGL_EINVAL) on a rank of a native team, whose convolution reads a halo. */
SGL_API int sgl_op_graph_conv(sgl_ctx* ctx, const double* X, int32_t k, double* Y);
/* mse_test (src/singlet.cpp:536-568) on the resident shard with the current factors. */
SGL_API int sgl_op_mse_test(sgl_ctx* ctx, uint64_t seed, uint64_t inv_density, double* out);
/* The three other device stages of one masked half-step (predict_mask, src/singlet.cpp:436-466, and mse_test), each through
 * the internal entry the fit calls; none touches a fit's factors, right-hand sides, entry streams or stream value arrays. */
/* Masked right-hand sides (src/singlet.cpp:449-457) for the resident shard: sgl_op_rhs with the entries drawn by the mask
 * left out.  which = 0 / 1: A / t(A) by the plain CSC kernel hashing every entry; 2 / 3: the same through a temporary entry
 * stream whose value array has zeros at the drawn entries.  The hash sees draw(cell, gene) with the context's cell_offset
 * added to the cell (the column of A, the row of t(A)), as the fit's masked steps do.  SGL_EINVAL for inv_density = 0 and,
 * tiled, at a rank without entry streams. */
SGL_API int sgl_op_rhs_masked(sgl_ctx* ctx, int which, const double* F, int32_t k, uint64_t seed, uint64_t inv_density, double* B);
/* The stages of sgl_variable_features, one at a time (the rules and the summation order are stated there).  All four only
 * read the context: they need a resident matrix (SGL_ESTATE without) and run over its gene-side image t(A) whatever it
 * holds (counts or not, a shard or not); SGL_EINVAL for a NULL array.
 *  - sgl_op_gene_mean: mean[g] = S_g / (double)ncol and count[g] = c_g, nrow of each.
 *  - sgl_op_gene_var: var[g] = (Q_g + Z_g) / (double)(ncol - 1) about the given mu (nrow doubles).
 *  - sgl_op_gene_var_std: the variance of the counts standardised by mu and sd and clipped at vmax (taken as it is:
 *    only the composite replaces vmax <= 0); +0.0 where sd[g] == 0.
 *  - sgl_op_loess_direct: fitted[i] = the local fit at x[i] of y on x with windows of q points; x, y, fitted hold n doubles,
 *    x already sorted.  SGL_EINVAL when x is not ascending (or not finite), for q < 1, q > n and n >= 2^31. */
SGL_API int sgl_op_gene_mean(sgl_ctx* ctx, double* mean, int64_t* count);
SGL_API int sgl_op_gene_var(sgl_ctx* ctx, const double* mu, double* var);
SGL_API int sgl_op_gene_var_std(sgl_ctx* ctx, const double* mu, const double* sd, double vmax, double* out);
SGL_API int sgl_op_loess_direct(sgl_ctx* ctx, const double* x, const double* y, int64_t n, int64_t q, double* fitted);
/* The stages of sgl_markers, one at a time (the rules are stated there; the same refusals, the same read-only contract).
 *  - sgl_op_marker_sums: pos, nz (int64) and sum (double), each nrow x n_groups column-major; any may be NULL.
 *  - sgl_op_marker_ranks: rank2 (int64, nrow x n_groups) and tie (uint64, nrow); max_batch_entries = the entries of a batch
 *    of the long path, 0: the default (2^27), negative: SGL_EINVAL.  The results do not depend on it. */
SGL_API int sgl_op_marker_sums(sgl_ctx* ctx, const int32_t* labels, int32_t n_groups, int transform, int64_t* pos, int64_t* nz, double* sum);
SGL_API int sgl_op_marker_ranks(sgl_ctx* ctx, const int32_t* labels, int32_t n_groups, int64_t max_batch_entries, int64_t* rank2,
                                uint64_t* tie);
/* The stages of sgl_signature_scores (the rules are stated there; the same refusals, the same read-only contract), with the
 * knobs that force every path at small shapes.  A knob of 0 means the default, a negative one is SGL_EINVAL, one above the
 * default is the default; the results do not depend on any of them.
 *  - lds_cap: the stored non-zero entries up to which a cell is sorted in LDS (default 4096; the small instance takes the
 *    cells up to min(lds_cap, 1024)); max_batch_entries: the entries of a batch of the long path (default 2^27);
 *    pass_sets: the sets of one pass (default 1024).
 *  - sgl_op_cell_ranks: rank2_entry_out[q] (uint64, one per stored entry, in storage order) = the doubled capped midrank
 *    r2' of stored entry q within its cell; a stored zero gets the zero block's value.  zero2_out[c] (uint64, ncol) = the
 *    zero block's value of cell c, or 0 when Z = 0.  Either may be NULL.
 *  - sgl_op_signature_scores: sgl_signature_scores with the three knobs before the outputs. */
SGL_API int sgl_op_cell_ranks(sgl_ctx* ctx, int32_t max_rank, int64_t lds_cap, int64_t max_batch_entries, uint64_t* rank2_entry_out,
                              uint64_t* zero2_out);
SGL_API int sgl_op_signature_scores(sgl_ctx* ctx, const int64_t* set_ptr, const int32_t* set_genes, int32_t n_sets, int32_t max_rank,
                                    int64_t lds_cap, int64_t max_batch_entries, int32_t pass_sets, uint64_t* rank2_out,
                                    double* score_out);
/* The merge of sgl_simulate_doublets alone (the rules are stated there), over the matrix of ctx, which is only read: S comes
 * back as CSC slots -- p_out n_sim + 1 offsets (int64), i_out / x_out p_out[n_sim] entries.  With i_out == NULL and
 * x_out == NULL only p_out is written: the caller sizes the second call from p_out[n_sim] (the two-call pattern of the
 * neighbour graphs).  lds_cap forces the path split: a pair goes to the LDS path when la + lb <= lds_cap; 0 is the default
 * of 4096, a larger value is the default, a negative one SGL_EINVAL; the result does not depend on it, and
 * sgl_doublets_info says what ran.  The refusals of sgl_simulate_doublets that concern one context apply (SGL_ESTATE: no
 * matrix, a team member, a hook, a shard; SGL_EINVAL: n_sim, a NULL list, a parent out of range, NULL p_out, one of i_out /
 * x_out without the other).  A non-finite sum is NOT refused here: it comes back as it is. */
SGL_API int sgl_op_pair_columns(sgl_ctx* ctx, const int32_t* parent_a, const int32_t* parent_b, int64_t n_sim, int64_t lds_cap,
                                int64_t* p_out, int32_t* i_out, double* x_out);
/* The stages of sgl_c_gsea, one at a time (the rules and the refusals are stated there).  They use the context's device,
 * stream and pool only: no resident matrix is needed, nothing of the context changes but what sgl_gsea_info reports.
 *  - sgl_op_gsea_es: the observed scores of the given sets under all three score types, each n_sets x k column-major; any
 *    may be NULL.
 *  - sgl_op_gsea_null: the null scores of the given sizes (strictly ascending, each in [1, min(m - 1, 4096)]) for the
 *    permutations [r0, r1), 0 <= r0 < r1 <= 2^20, in batches of `batch` permutations (0: by the memory budget; negative:
 *    SGL_EINVAL): null_out[(f n_sizes + si) (r1 - r0) + (r - r0)], and sample[(r - r0) s_max + t] = the gene at place t of
 *    permutation r's order by (key, gene), s_max = the largest size; either may be NULL.  The results do not depend on
 *    `batch`. */
SGL_API int sgl_op_gsea_es(sgl_ctx* ctx, const double* w, int32_t m, int32_t k, const int64_t* set_ptr, const int32_t* set_genes,
                           int32_t n_sets, double* es_pos, double* es_neg, double* es_std);
SGL_API int sgl_op_gsea_null(sgl_ctx* ctx, const double* w, int32_t m, int32_t k, const int32_t* sizes, int32_t n_sizes,
                             int score_type, uint64_t seed, int32_t r0, int32_t r1, int32_t batch, double* null_out,
                             int32_t* sample);
/* nnls on ncols independent columns, each against its OWN Gram: Gcols = ncols blocks of k x k, B / X as in sgl_op_nnls;
 * col_nnz (int64 [ncols], or NULL): columns with a zero there are skipped -- X keeps its input, no sweeps are counted.
 * The dispatch of every masked half-step (four columns per wave on LDS triangles or on the Grams in global memory, one
 * wave per column above), 1 <= k <= 1024. */
SGL_API int sgl_op_nnls_percol(sgl_ctx* ctx, const double* Gcols, const double* B, double* X, const int64_t* col_nnz, int32_t k,
                int64_t ncols, double L1, double L2, int32_t* sweeps_out);
/* mse_test per cell, before the sum: losses[c] = mean over the drawn genes g of cell c of ((W diag(d) h_c)[g] - A(g, c))^2,
 * 0 for a cell without a drawn gene; ncol doubles.  variant names the kernel family: 0 hashing inside the kernel; 1 from
 * the cell-side mask lists, the matrix values found through the sliding window; 2 from the lists with the matrix values
 * listed first.  1 and 2 select (build, when they are not there) the context's cell-side lists for this mask, as a masked
 * H-update does: SGL_EINVAL above k = 128, SGL_ENOMEM when the lists (or, for 2, the values) are refused.  Needs a fit. */
SGL_API int sgl_op_mse_test_cells(sgl_ctx* ctx, uint64_t seed, uint64_t inv_density, int variant, double* losses);

/* ------------------------------------------------------------------------
 * 4. Timing (hipEvent based, on the context's stream).
 * ---------------------------------------------------------------------- */
#define SGL_PH_GRAM 0      /* AAt kernels */
#define SGL_PH_RHS_H 1     /* sparse accumulate, H-update (over A) */
#define SGL_PH_NNLS_H 2
#define SGL_PH_RHS_W 3     /* sparse accumulate, W-update (over At) */
#define SGL_PH_NNLS_W 4
#define SGL_PH_SCALE 5     /* row sums, scale, cor, copies */
#define SGL_PH_COMM 6      /* all-reduce callback */
#define SGL_PH_MASK 7      /* masked path: the per-column Gram downdates of predict_mask (src/singlet.cpp:458-463), mask lists */
#define SGL_PH_MSE 8       /* masked path: mse_test (src/singlet.cpp:536-568), one call per trace row */
#define SGL_PH_COUNT 9
/* Enable/disable per-phase timing (costs two event records per kernel group). */
SGL_API int sgl_timing_enable(sgl_ctx* ctx, int on);
/* ms[SGL_PH_COUNT] accumulated since the last reset, calls[SGL_PH_COUNT] launches. */
SGL_API int sgl_timing_get(sgl_ctx* ctx, double* ms, int64_t* calls, int reset);
/* NNLS sweep totals since the last reset: [0] sweeps summed over the columns of
 * the H solves, [1] same for the W solves; [2], [3] sweeps each 64-column wave
 * actually executed (the maximum over its columns), summed over the waves of
 * the H / W solves -- the number that drives the kernel's run time. */
SGL_API int sgl_sweeps_get(sgl_ctx* ctx, int64_t* out4, int reset);
/* HBM layout of the current fit's entry streams (DESIGN.md "Data layout"), for
 * the roofline report: per orientation (A then At) five numbers --
 * entries stored (non-zeros + padding), row tiles T, rows per tile TR, tile
 * ranges R (blockIdx.y slabs), column blocks of 64.  out10 all zero when the
 * fit runs on the plain CSC kernel (k > 128). */
SGL_API int sgl_layout_get(sgl_ctx* ctx, int64_t* out10);
/* How many times derived data of the resident matrix has been (re)written on this context, out4 = entry stream of A, of
 * At, mask lists of the cell side, of the gene side.  A fit at an unchanged rank reuses the streams (sgl_fit_init above);
 * a masked fit (src/singlet.cpp:436-466, the test set rng(seed).draw(inv_density, ...)) whose (seed, inv_density) was
 * among the last SGL_MASK_KEEP + 1 (default 3: R's n_replicates, R/ard_nmf.R:20) reuses the lists of drawn entries --
 * the mask does not depend on the rank. */
SGL_API int sgl_layout_builds(sgl_ctx* ctx, int64_t* out4);
/* Drawn (cell, gene) pairs of the mask the current fit runs under -- the entries predict_mask leaves out and mse_test scores
 * (src/singlet.cpp:445-448: rng(seed).draw(inv_density, ...) true), as this shard's lists hold them: out2 = pairs listed
 * per cell (H-update), per gene (W-update); 0 where the lists are not built (no masked pass yet, or the hashing kernels run).
 * One masked iteration forms out2[0] + out2[1] rank-one downdates w_r w_r^T: the work unit of the measurement in bench.py. */
SGL_API int sgl_mask_pairs(sgl_ctx* ctx, int64_t* out2);
/* Host wall-clock seconds of the calling thread's LAST one-shot call (sgl_c_nmf / sgl_c_ard_nmf: what an R caller of
 * run_nmf -> .Call(_singlet_c_nmf), R/run_nmf.R:39-59, src/RcppExports.cpp:98-116, waits for around the iterations).  Up to n of
 * out[0] host -> device copies of the dgCMatrix slots, [1] validation kernels (ascending rows, finite values), [2] device transpose
 * (At = NULL), [3] sgl_fit_init (entry streams, w), [4] the ALS loop, [5] factors back to the host, [6] bytes copied in,
 * [7] 1.0 when SINGLET_HIP_CACHE served the resident matrix of the previous call (nothing uploaded), [8] the whole call. */
SGL_API int sgl_call_times_get(double* out, int32_t n);
/* Device memory the library keeps for reuse (round 6): blocks of 64 MB and more that a context frees -- the matrix slots, the
 * entry streams, the factors of a one-shot call -- are cached per device and serve the next request they fit instead of going
 * back to the driver, whose hipMalloc right after such a free takes seconds (3 s for config 3's 22 GB streams: as long as the
 * fit; R's ard_nmf makes tens of such calls, R/ard_nmf.R:95-160).  *cached_bytes = bytes cached on the current device.  They
 * stay reserved by the process until sgl_cache_release(); SGL_POOL=0 in the environment switches the caching off,
 * SGL_POOL_MAX_GB caps it (default: 70 % of the device memory). */
SGL_API int sgl_pool_info(int64_t* cached_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SINGLET_HIP_H */
