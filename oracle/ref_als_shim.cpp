// C shim around the REFERENCE's own ALS functions (src/singlet.cpp), compiled from the reference tree where it lies:
// oracle/make_ref.sh cuts the functions out at build time into the git-ignored oracle/_ref/als_functions.inc (never
// committed) and compiles this file against it and against oracle/standin/ (own text: the few Eigen / Rcpp names
// those functions use) -> oracle/_ref/libals_ref.so and libals_ref_b.so.  This file holds no reference text.
// Test infrastructure only.
//
// Every export has the C signature of its ora_* counterpart in singlet_oracle.c (factor matrices k x cols
// column-major, CSC as x / i / p), so oracle/reference.py can drive either library through one binding.  Where the
// reference returns less than the oracle does, the difference is stated at the export.
#include <cstdint>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "standin/rcpp_standin.h"
#include "_ref/rng_class.inc"
#include "_ref/als_functions.inc"

#define REF_API extern "C" __attribute__((visibility("default")))

namespace {
typedef Eigen::MatrixXd Mat;
typedef Rcpp::SparseMatrix Csc;

Mat mat_in(const double* p, size_t r, size_t c) {
    Mat m(r, c);
    if (p && r * c) std::memcpy(m.v.data(), p, sizeof(double) * r * c);
    return m;
}
void mat_out(const Mat& m, double* p) {
    if (m.size()) std::memcpy(p, m.v.data(), sizeof(double) * m.size());
}
void vec_out(const Eigen::VectorXd& v, double* p) {
    for (size_t q = 0; q < v.size(); ++q) p[q] = v(q);
}
// the drivers print one "%4d | %8.2e" line per iteration when verbose; that is the only place the reference tells how
// many iterations it ran.  Returns their count; tol_trace (optional) receives the PRINTED tolerances (three digits).
int parse_iterations(double* tol_trace) {
    std::string out;
    out.swap(standin_output());
    int n = 0;
    size_t pos = 0;
    while (pos < out.size()) {
        size_t end = out.find('\n', pos);
        if (end == std::string::npos) end = out.size();
        int it;
        double t;
        if (std::sscanf(out.substr(pos, end - pos).c_str(), "%d | %lf", &it, &t) == 2) {
            if (tol_trace) tol_trace[n] = t;
            ++n;
        }
        pos = end + 1;
    }
    return n;
}
Rcpp::List list_in(int n, const double* const* x, const int32_t* const* i, const int32_t* const* p, const int32_t* ncol, int32_t nrow) {
    Rcpp::List l;
    for (int q = 0; q < n; ++q) l.items.push_back(Csc(x[q], i[q], p[q], nrow, ncol[q]));
    return l;
}
int trace_out(Rcpp::List& r, double* test_mse, int32_t* iter, double* fit_tol, double* score_overfit) {
    const int nt = (int)r.iter.size();
    for (int q = 0; q < nt; ++q) {
        test_mse[q] = r.test_mse[q];
        iter[q] = r.iter[q];
        fit_tol[q] = r.tol[q];
        score_overfit[q] = r.score_overfit[q];
    }
    return nt;
}
}  // namespace

REF_API int ref_variant(void) {
#ifdef STANDIN_DESCENDING
    return 1;
#else
    return 0;
#endif
}

REF_API double ref_cor(const double* x, const double* y, size_t n) {
    Mat X = mat_in(x, n, 1), Y = mat_in(y, n, 1);
    return cor(X, Y);
}

REF_API void ref_aat(const double* F, int k, int64_t cols, double* G) { mat_out(AAt(mat_in(F, k, cols)), G); }

REF_API void ref_scale(double* F, int k, int64_t cols, double* d) {
    Mat W = mat_in(F, k, cols);
    Eigen::VectorXd D = Eigen::VectorXd::Ones(k);
    scale(W, D);
    mat_out(W, F);
    vec_out(D, d);
}

// the reference's nnls returns nothing: -1 stands where ora_nnls returns its sweep count
REF_API int ref_nnls(const double* a, double* b, double* x, int k, double L1, double L2) {
    Mat A = mat_in(a, k, k), X = mat_in(x, k, 1);
    Eigen::VectorXd B(k);
    for (int q = 0; q < k; ++q) B(q) = b[q];
    nnls(A, B, X, 0, L1, L2);
    vec_out(B, b);
    mat_out(X, x);
    return -1;
}

REF_API void ref_predict(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol, const double* F,
                         double* X, int k, double L1, double L2, int threads) {
    Mat w = mat_in(F, k, nrow), h = mat_in(X, k, ncol);
    predict(Csc(Ax, Ai, Ap, nrow, ncol), w, h, L1, L2, threads);
    mat_out(h, X);
}

REF_API void ref_predict_dense(const double* A, int32_t nrow, int32_t ncol, const double* F, double* X, int k, double L1,
                               double L2, int threads) {
    Mat w = mat_in(F, k, nrow), h = mat_in(X, k, ncol);
    predict(mat_in(A, nrow, ncol), w, h, L1, L2, threads);
    mat_out(h, X);
}

REF_API void ref_predict_mask(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol, uint64_t seed,
                              uint64_t inv_density, const double* F, double* X, int k, double L1, double L2, int threads,
                              int mask_t) {
    Mat w = mat_in(F, k, nrow), h = mat_in(X, k, ncol);
    predict_mask(Csc(Ax, Ai, Ap, nrow, ncol), rng(seed), inv_density, w, h, L1, L2, threads, mask_t != 0);
    mat_out(h, X);
}

REF_API double ref_mse_test(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol, const double* w,
                            const double* d, const double* h, int k, uint64_t seed, uint64_t inv_density, int threads) {
    Mat W = mat_in(w, k, nrow), H = mat_in(h, k, ncol);
    Eigen::VectorXd D(k);
    for (int q = 0; q < k; ++q) D(q) = d[q];
    return mse_test(Csc(Ax, Ai, Ap, nrow, ncol), W, D, H, rng(seed), inv_density, (uint16_t)threads);
}

// returns the iteration count read off the verbose lines; tol_trace holds the printed tolerances; phase_sec / sweeps
// (the oracle's timing extras) are left untouched
REF_API int ref_c_nmf(const double* Ax, const int32_t* Ai, const int32_t* Ap, const double* Atx, const int32_t* Ati,
                      const int32_t* Atp, int32_t m, int32_t n, double tol, int maxit, double L1_w, double L1_h, double L2_w,
                      double L2_h, int threads, int k, double* w, double* h, double* d, double* tol_trace, double* phase_sec,
                      int64_t* sweeps) {
    (void)phase_sec; (void)sweeps;
    Csc A(Ax, Ai, Ap, m, n), At(Atx, Ati, Atp, n, m);
    standin_output().clear();
    Rcpp::List r = c_nmf(A, At, tol, (uint16_t)maxit, true, L1_w, L1_h, L2_w, L2_h, (uint16_t)threads, mat_in(w, k, m));
    mat_out(r.w, w); mat_out(r.h, h); vec_out(r.d, d);
    return parse_iterations(tol_trace);
}

REF_API int ref_c_nmf_dense(const double* A, const double* At, int32_t m, int32_t n, double tol, int maxit, double L1_w,
                            double L1_h, double L2_w, double L2_h, int threads, int k, double* w, double* h, double* d,
                            double* tol_trace) {
    Mat a = mat_in(A, m, n), at = mat_in(At, n, m);
    standin_output().clear();
    Rcpp::List r = c_nmf_dense(a, at, tol, (uint16_t)maxit, true, L1_w, L1_h, L2_w, L2_h, (uint16_t)threads, mat_in(w, k, m));
    mat_out(r.w, w); mat_out(r.h, h); vec_out(r.d, d);
    return parse_iterations(tol_trace);
}

// a NULL link becomes a 0 x 0 matrix, whose column count matches no side
REF_API int ref_c_linked_nmf(const double* Ax, const int32_t* Ai, const int32_t* Ap, const double* Atx, const int32_t* Ati,
                             const int32_t* Atp, int32_t m, int32_t n, double tol, int maxit, double L1, double L2, int threads,
                             int k, double* w, const double* link_h, int32_t link_h_rows, int32_t link_h_cols,
                             const double* link_w, int32_t link_w_rows, int32_t link_w_cols, double* h, double* d,
                             double* tol_trace) {
    Csc A(Ax, Ai, Ap, m, n), At(Atx, Ati, Atp, n, m);
    Mat lh = link_h ? mat_in(link_h, link_h_rows, link_h_cols) : Mat();
    Mat lw = link_w ? mat_in(link_w, link_w_rows, link_w_cols) : Mat();
    standin_output().clear();
    Rcpp::List r = c_linked_nmf(A, At, tol, (uint16_t)maxit, true, L1, L2, (uint16_t)threads, mat_in(w, k, m), lh, lw);
    mat_out(r.w, w); mat_out(r.h, h); vec_out(r.d, d);
    return parse_iterations(tol_trace);
}

REF_API int ref_c_project_model(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t m, int32_t n, const double* w_in,
                                int32_t w_rows, int32_t w_cols, double L1, double L2, int threads, double* h, double* d) {
    Rcpp::List r = c_project_model(Csc(Ax, Ai, Ap, m, n), mat_in(w_in, w_rows, w_cols), L1, L2, threads);
    mat_out(r.h, h); vec_out(r.d, d);
    return (int)r.h.rows();
}

// Rcpp_predict has no ora_* counterpart (oracle.py composes it): same arguments as c_project_model without d
REF_API int ref_rcpp_predict(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t m, int32_t n, const double* w_in,
                             int32_t w_rows, int32_t w_cols, double L1, double L2, int threads, double* h) {
    Mat H = Rcpp_predict(Csc(Ax, Ai, Ap, m, n), mat_in(w_in, w_rows, w_cols), L1, L2, threads);
    mat_out(H, h);
    return (int)H.rows();
}

// the return value is -1: the reference does not tell the iteration count apart from the `iter` vector
REF_API int ref_c_ard_nmf(const double* Ax, const int32_t* Ai, const int32_t* Ap, const double* Atx, const int32_t* Ati,
                          const int32_t* Atp, int32_t m, int32_t n, double tol, int maxit, double L1, double L2, int threads,
                          int k, double* w, double* h, double* d, uint64_t rng_seed, uint64_t inv_density,
                          double overfit_threshold, int trace_test_mse, double* test_mse, int32_t* iter, double* fit_tol,
                          double* score_overfit, int32_t* n_trace) {
    Csc A(Ax, Ai, Ap, m, n), At(Atx, Ati, Atp, n, m);
    Rcpp::List r = c_ard_nmf(A, At, tol, (uint16_t)maxit, false, L1, L2, (uint16_t)threads, mat_in(w, k, m), rng_seed, inv_density,
                             overfit_threshold, (uint16_t)trace_test_mse);
    mat_out(r.w, w); mat_out(r.h, h); vec_out(r.d, d);
    *n_trace = trace_out(r, test_mse, iter, fit_tol, score_overfit);
    return -1;
}

REF_API int ref_c_ard_nmf_dense(const double* A, const double* At, int32_t m, int32_t n, double tol, int maxit, double L1,
                                double L2, int threads, int k, double* w, double* h, double* d, uint64_t rng_seed,
                                uint64_t inv_density, double overfit_threshold, int trace_test_mse, double* test_mse,
                                int32_t* iter, double* fit_tol, double* score_overfit, int32_t* n_trace) {
    Mat a = mat_in(A, m, n), at = mat_in(At, n, m);
    Rcpp::List r = c_ard_nmf_dense(a, at, tol, (uint16_t)maxit, false, L1, L2, (uint16_t)threads, mat_in(w, k, m), rng_seed,
                                   inv_density, overfit_threshold, (uint16_t)trace_test_mse);
    mat_out(r.w, w); mat_out(r.h, h); vec_out(r.d, d);
    *n_trace = trace_out(r, test_mse, iter, fit_tol, score_overfit);
    return -1;
}

REF_API int ref_c_nmf_sparse_list(int nA, const double* const* Ax, const int32_t* const* Ai, const int32_t* const* Ap,
                                  const int32_t* Ancol, int nAt, const double* const* Atx, const int32_t* const* Ati,
                                  const int32_t* const* Atp, const int32_t* Atncol, int32_t m, int32_t n, double tol, int maxit,
                                  double L1, double L2, int threads, int k, double* w, double* h, double* d, double* tol_trace) {
    Rcpp::List A = list_in(nA, Ax, Ai, Ap, Ancol, m), At = list_in(nAt, Atx, Ati, Atp, Atncol, n);
    standin_output().clear();
    Rcpp::List r = c_nmf_sparse_list(A, At, tol, (uint16_t)maxit, true, L1, L2, (uint16_t)threads, mat_in(w, k, m));
    mat_out(r.w, w); mat_out(r.h, h); vec_out(r.d, d);
    return parse_iterations(tol_trace);
}

REF_API int ref_c_ard_nmf_sparse_list(int nA, const double* const* Ax, const int32_t* const* Ai, const int32_t* const* Ap,
                                      const int32_t* Ancol, int nAt, const double* const* Atx, const int32_t* const* Ati,
                                      const int32_t* const* Atp, const int32_t* Atncol, int32_t m, int32_t n, double tol, int maxit,
                                      double L1, double L2, int threads, int k, double* w, double* h, double* d,
                                      uint64_t rng_seed, uint64_t inv_density, double overfit_threshold, int trace_test_mse,
                                      double* test_mse, int32_t* iter, double* fit_tol, double* score_overfit, int32_t* n_trace) {
    Rcpp::List A = list_in(nA, Ax, Ai, Ap, Ancol, m), At = list_in(nAt, Atx, Ati, Atp, Atncol, n);
    Rcpp::List r = c_ard_nmf_sparse_list(A, At, tol, (uint16_t)maxit, false, L1, L2, (uint16_t)threads, mat_in(w, k, m), rng_seed,
                                         inv_density, overfit_threshold, (uint16_t)trace_test_mse);
    mat_out(r.w, w); mat_out(r.h, h); vec_out(r.d, d);
    *n_trace = trace_out(r, test_mse, iter, fit_tol, score_overfit);
    return -1;
}

// c_gcnmf: w_in in R orientation (w_rows x w_cols column-major).  w_out: m x k column-major (the reference returns
// the transpose of its working w), h: k x n, d: k.  Returns the iteration count; *k_out the rank it worked with.
REF_API int ref_c_gcnmf(const double* Ax, const int32_t* Ai, const int32_t* Ap, const double* Atx, const int32_t* Ati,
                        const int32_t* Atp, const double* Gx, const int32_t* Gi, const int32_t* Gp, int32_t m, int32_t n,
                        double tol, int maxit, double L1, double L2, int threads, const double* w_in, int32_t w_rows,
                        int32_t w_cols, double* w_out, double* h, double* d, double* tol_trace, int32_t* k_out) {
    Csc A(Ax, Ai, Ap, m, n), At(Atx, Ati, Atp, n, m), G(Gx, Gi, Gp, n, n);
    standin_output().clear();
    Rcpp::List r = c_gcnmf(A, At, G, tol, (uint16_t)maxit, true, L1, L2, (uint16_t)threads, mat_in(w_in, w_rows, w_cols));
    mat_out(r.w, w_out); mat_out(r.h, h); vec_out(r.d, d);
    *k_out = (int32_t)r.h.rows();
    return parse_iterations(tol_trace);
}

// spatial_graph: p (n + 1), i / x (room for n * max_k entries).  Returns the number of stored entries.
REF_API int64_t ref_spatial_graph(const double* c1, const double* c2, int64_t n, double max_dist, int64_t max_k, int32_t* p,
                                  int32_t* i, double* x) {
    Rcpp::S4 g = spatial_graph(std::vector<double>(c1, c1 + n), std::vector<double>(c2, c2 + n), max_dist, (size_t)max_k, 0);
    for (size_t q = 0; q < g.p.size(); ++q) p[q] = g.p[q];
    for (size_t q = 0; q < g.x.size(); ++q) { i[q] = g.i[q]; x[q] = g.x[q]; }
    return (int64_t)g.x.size();
}

// row-wise compression: out is floor(nrow / n) x ncol column-major.  Returns 1 where the reference indexes outside a
// matrix (R would not notice; the stand-in's NumericMatrix does), 0 otherwise.
REF_API int ref_rowwise_compress_sparse(const double* Ax, const int32_t* Ai, const int32_t* Ap, int32_t nrow, int32_t ncol,
                                        int64_t n, double* out) {
    Csc A(Ax, Ai, Ap, nrow, ncol);
    try {
        Rcpp::NumericMatrix r = rowwise_compress_sparse(A, (size_t)n, 0);
        if (!r.v.empty()) std::memcpy(out, r.v.data(), sizeof(double) * r.v.size());
    } catch (const std::out_of_range&) {
        return 1;
    }
    return 0;
}

REF_API int ref_rowwise_compress_dense(const double* A, int32_t nrow, int32_t ncol, int64_t n, double* out) {
    Rcpp::NumericMatrix a(nrow, ncol);
    if (!a.v.empty()) std::memcpy(a.v.data(), A, sizeof(double) * a.v.size());
    try {
        Rcpp::NumericMatrix r = rowwise_compress_dense(a, (size_t)n, 0);
        if (!r.v.empty()) std::memcpy(out, r.v.data(), sizeof(double) * r.v.size());
    } catch (const std::out_of_range&) {
        return 1;
    }
    return 0;
}
