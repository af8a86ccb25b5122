/*
 * singlet_hip_graph_shim.c -- .Call bodies of the three spatial graph entry points, registered by
 * singlet_hip_shim.c's call_entries table.  Same names and arity as the reference's Rcpp glue
 * (src/RcppExports.cpp:465-467: _singlet_spatial_graph, 5 args; _singlet_c_LKNN, 10 args; _singlet_c_SNN, 3 args), so that
 * R/FindLocalNeighbors.R:95-98 and singlet:::spatial_graph work unchanged.  They need two R API pieces the main shim does not: the string of
 * `metric`, and a new Matrix::dgCMatrix object for the result.
 *
 * Compiled and executed here against the emulated R C API of tests/r_emul/ together with singlet_hip_shim.c (see its header;
 * tests/test_r_shim_emulated.py, tests/test_gpu_r_shim.py); a build against R's own headers remains unverified.
 */
#include <R.h>
#include <Rinternals.h>
#include <math.h>
#include <stdint.h>

#include "singlet_hip.h"

SEXP _singlet_c_LKNN(SEXP m_, SEXP coord_x_, SEXP coord_y_, SEXP k_, SEXP radius_, SEXP metric_, SEXP similarity_,
                     SEXP max_dist_, SEXP verbose_, SEXP threads_);
SEXP _singlet_c_SNN(SEXP G_, SEXP min_similarity_, SEXP threads_);
SEXP _singlet_spatial_graph(SEXP c1_, SEXP c2_, SEXP max_dist_, SEXP max_k_, SEXP threads_);

static void graph_fail_if(int rc) {
    if (rc != SGL_OK) Rf_error("singlet HIP back end: %s", sgl_last_error());
}

/* new("dgCMatrix", i = , p = , x = , Dim = c(n, n)) from the two-call output of sgl_c_lknn / sgl_c_snn / sgl_spatial_graph. */
typedef int (*graph_call)(void* args, int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap);

static SEXP graph_result(graph_call fn, void* args, int n) {
    SEXP p = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)n + 1));
    int64_t nnz = 0;
    graph_fail_if(fn(args, INTEGER(p), &nnz, NULL, NULL, 0));
    SEXP i = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)nnz)), x = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)nnz));
    int32_t dummy_i = 0;
    double dummy_x = 0;
    graph_fail_if(fn(args, INTEGER(p), &nnz, nnz ? INTEGER(i) : &dummy_i, nnz ? REAL(x) : &dummy_x, nnz));
    SEXP dim = PROTECT(Rf_allocVector(INTSXP, 2));
    INTEGER(dim)[0] = n;
    INTEGER(dim)[1] = n;
    SEXP cls = PROTECT(R_do_MAKE_CLASS("dgCMatrix"));
    SEXP out = PROTECT(R_do_new_object(cls));
    R_do_slot_assign(out, Rf_install("i"), i);
    R_do_slot_assign(out, Rf_install("p"), p);
    R_do_slot_assign(out, Rf_install("x"), x);
    R_do_slot_assign(out, Rf_install("Dim"), dim);
    UNPROTECT(6);
    return out;
}

typedef struct {
    const double* m;
    int m_rows, m_cols;
    const double *cx, *cy;
    int n;
    int64_t k;
    double radius, max_dist;
    const char* metric;
    int similarity;
} lknn_args;

static int lknn_call(void* a_, int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap) {
    const lknn_args* a = (const lknn_args*)a_;
    return sgl_c_lknn(a->m, a->m_rows, a->m_cols, a->cx, a->cy, a->n, a->k, a->radius, a->metric, a->similarity, a->max_dist,
                      p_out, nnz_out, i_out, x_out, cap);
}

/* ---- c_LKNN(m, coord_x, coord_y, k, radius, metric, similarity, max_dist, verbose, threads) ---- *
 * (src/singlet.cpp:1491-1603).  m: numeric matrix (factors x cells, or cells x factors: transposed by the reference's
 * rule); coordinates: numeric vectors.  Prints the reference's three lines when verbose. */
SEXP _singlet_c_LKNN(SEXP m_, SEXP coord_x_, SEXP coord_y_, SEXP k_, SEXP radius_, SEXP metric_, SEXP similarity_,
                     SEXP max_dist_, SEXP verbose_, SEXP threads_) {
    (void)threads_;
    if (!Rf_isMatrix(m_) || TYPEOF(m_) != REALSXP) Rf_error("m must be a numeric matrix");
    if (TYPEOF(coord_x_) != REALSXP || TYPEOF(coord_y_) != REALSXP) Rf_error("coordinates must be numeric vectors");
    if (!Rf_isString(metric_) || XLENGTH(metric_) < 1) Rf_error("metric must be a string");
    lknn_args a;
    a.m = REAL(m_);
    a.m_rows = Rf_nrows(m_);
    a.m_cols = Rf_ncols(m_);
    a.cx = REAL(coord_x_);
    a.cy = REAL(coord_y_);
    a.n = (int)XLENGTH(coord_x_);
    const int m_cols_t = (a.m_cols != a.m_rows && a.m_rows == a.n) ? a.m_rows : a.m_cols;   /* l.1492 */
    if (m_cols_t != a.n) Rf_error("number of columns in 'm' must be equal to number of coordinates");
    if (XLENGTH(coord_y_) != XLENGTH(coord_x_)) Rf_error("length of coordinate vectors must be equivalent");
    a.k = (int64_t)Rf_asReal(k_);
    a.radius = Rf_asReal(radius_);
    a.metric = R_CHAR(STRING_ELT(metric_, 0));
    a.similarity = Rf_asLogical(similarity_);
    a.max_dist = Rf_asReal(max_dist_);
    const int verbose = Rf_asLogical(verbose_);
    if (verbose) {   /* l.1497, 1506: the slots per point, computed as the reference does */
        const float base = (float)a.radius * 2.0f + 1.0f;
        const double nme = ceil((double)base * (double)base) - 1.0;
        Rprintf("number of edges per node: %u\n", (unsigned)(uint64_t)nme);
        Rprintf("filtering %llu edges\n", (unsigned long long)((uint64_t)a.n * (uint64_t)nme));
    }
    SEXP out = PROTECT(graph_result(lknn_call, &a, a.n));
    if (verbose) Rprintf("selected %llu edges\n", (unsigned long long)INTEGER(R_do_slot(out, Rf_install("p")))[a.n]);
    UNPROTECT(1);
    return out;
}

typedef struct {
    const int32_t *i, *p;
    int nrow, ncol;
    double min_similarity;
} snn_args;

static int snn_call(void* a_, int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap) {
    const snn_args* a = (const snn_args*)a_;
    return sgl_c_snn(a->i, a->p, a->nrow, a->ncol, a->min_similarity, p_out, nnz_out, i_out, x_out, cap);
}

/* ---- c_SNN(G, min_similarity, threads) ---- *
 * (src/singlet.cpp:1606-1665).  G: dgCMatrix; only its pattern is read. */
SEXP _singlet_c_SNN(SEXP G_, SEXP min_similarity_, SEXP threads_) {
    (void)threads_;
    SEXP names[3] = {Rf_install("i"), Rf_install("p"), Rf_install("Dim")};
    for (int q = 0; q < 3; ++q)
        if (!R_has_slot(G_, names[q])) Rf_error("G: not a dgCMatrix (missing slot)");
    SEXP i = R_do_slot(G_, names[0]), p = R_do_slot(G_, names[1]), dim = R_do_slot(G_, names[2]);
    if (TYPEOF(i) != INTSXP || TYPEOF(p) != INTSXP || TYPEOF(dim) != INTSXP || XLENGTH(dim) != 2) Rf_error("G: not a dgCMatrix (slot types)");
    snn_args a;
    a.i = INTEGER(i);
    a.p = INTEGER(p);
    a.nrow = INTEGER(dim)[0];
    a.ncol = INTEGER(dim)[1];
    if (a.ncol < 0 || XLENGTH(p) != (R_xlen_t)a.ncol + 1) Rf_error("G: not a dgCMatrix (length(p) != ncol + 1)");
    if ((R_xlen_t)a.p[a.ncol] > XLENGTH(i)) Rf_error("G: not a dgCMatrix (p[ncol] > length(i))");   /* the library reads p[ncol] entries of i */
    a.min_similarity = Rf_asReal(min_similarity_);
    return graph_result(snn_call, &a, a.ncol);
}

typedef struct {
    const double *c1, *c2;
    int n;
    double max_dist;
    int64_t max_k;
} spatial_args;

static int spatial_call(void* a_, int32_t* p_out, int64_t* nnz_out, int32_t* i_out, double* x_out, int64_t cap) {
    const spatial_args* a = (const spatial_args*)a_;
    return sgl_spatial_graph(a->c1, a->c2, a->n, a->max_dist, a->max_k, p_out, nnz_out, i_out, x_out, cap);
}

/* A numeric vector as doubles, as Rcpp's std::vector<double> takes it: integers are widened (NA_integer_ becomes NaN, which
 * sgl_spatial_graph refuses). */
static SEXP as_doubles(SEXP v, const char* what) {
    if (TYPEOF(v) == REALSXP) return v;
    if (TYPEOF(v) != INTSXP) Rf_error("%s must be a numeric vector", what);
    const R_xlen_t n = XLENGTH(v);
    SEXP out = PROTECT(Rf_allocVector(REALSXP, n));
    const int* src = INTEGER(v);
    double* dst = REAL(out);
    for (R_xlen_t e = 0; e < n; ++e) dst[e] = src[e] == INT32_MIN ? NAN : (double)src[e];
    UNPROTECT(1);
    return out;
}

/* ---- spatial_graph(c1, c2, max_dist, max_k, threads) ---- *
 * (src/singlet.cpp:1365-1414).  c1, c2: numeric vectors of one length; max_k truncates toward zero as Rcpp's size_t
 * conversion does (NA and negative values refused). */
SEXP _singlet_spatial_graph(SEXP c1_, SEXP c2_, SEXP max_dist_, SEXP max_k_, SEXP threads_) {
    (void)threads_;
    SEXP c1 = PROTECT(as_doubles(c1_, "c1")), c2 = PROTECT(as_doubles(c2_, "c2"));
    if (XLENGTH(c1) != XLENGTH(c2)) Rf_error("spatial_graph: c1 and c2 differ in length");
    if (XLENGTH(c1) > 2147483647) Rf_error("spatial_graph: too many points for a dgCMatrix");
    const double k = Rf_asReal(max_k_);
    if (ISNAN(k) || k < 0) Rf_error("spatial_graph: max_k must be a non-negative number");
    spatial_args a;
    a.c1 = REAL(c1);
    a.c2 = REAL(c2);
    a.n = (int)XLENGTH(c1);
    a.max_dist = Rf_asReal(max_dist_);
    a.max_k = k >= 9.2e18 ? INT64_MAX : (int64_t)k;   /* above n it acts as n */
    SEXP out = graph_result(spatial_call, &a, a.n);
    UNPROTECT(2);
    return out;
}
