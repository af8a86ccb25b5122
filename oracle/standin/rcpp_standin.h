// Stand-in for the few Rcpp names the reference's ALS functions use, and for the reference's own Rcpp::SparseMatrix
// (inst/include/singlet.h), restated as a view on raw CSC pointers.  See eigen_standin.h for the purpose.
// Written from the documented meaning of each name; holds no line of the reference.  Test infrastructure only.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "eigen_standin.h"

namespace Rcpp {
template <class T> struct Vector {
    std::vector<T> v;
    Vector() {}
    explicit Vector(size_t n) : v(n) {}
    Vector(size_t n, T fill) : v(n, fill) {}
    void push_back(T x) { v.push_back(x); }
    size_t size() const { return v.size(); }
    T& operator()(size_t i) { return v[i]; }
    T& operator[](size_t i) { return v[i]; }
    const T& operator[](size_t i) const { return v[i]; }
};
typedef Vector<double> NumericVector;
typedef Vector<int> IntegerVector;
inline double min(const NumericVector& x) {
    double m = x.v[0];
    for (double e : x.v) m = e < m ? e : m;
    return m;
}

// column-major numeric matrix, zero-filled.  Unlike R's, an index outside the matrix throws: the row-wise compression
// indexes past the end when its bin size does not divide the row count, and the shim reports that instead of
// corrupting the heap.
struct NumericMatrix {
    std::vector<double> v;
    size_t r = 0, c = 0;
    NumericMatrix() {}
    NumericMatrix(size_t r_, size_t c_) : v(r_ * c_), r(r_), c(c_) {}
    size_t rows() const { return r; }
    size_t cols() const { return c; }
    double& operator()(size_t i, size_t j) {
        if (i >= r || j >= c) throw std::out_of_range("NumericMatrix index");
        return v[i + j * r];
    }
};

// the four slots of a dgCMatrix that the reference wraps a result in
struct S4 {
    NumericVector x;
    IntegerVector i, p, Dim;
};

// CSC matrix: a view on x / i / p of the caller, or on slots it owns (built from vectors, as spatial_graph does)
struct SparseMatrix {
    const double* x = nullptr;
    const int* i = nullptr;
    const int* p = nullptr;
    int Dim[2] = {0, 0};
    std::shared_ptr<S4> own;
    SparseMatrix() {}
    SparseMatrix(const double* x_, const int* i_, const int* p_, int nrow, int ncol) : x(x_), i(i_), p(p_) { Dim[0] = nrow; Dim[1] = ncol; }
    SparseMatrix(const NumericVector& x_, const IntegerVector& i_, const IntegerVector& p_, const IntegerVector& Dim_)
        : own(new S4{x_, i_, p_, Dim_}) {
        x = own->x.v.data(); i = own->i.v.data(); p = own->p.v.data();
        Dim[0] = Dim_[0]; Dim[1] = Dim_[1];
    }
    unsigned int rows() { return Dim[0]; }
    unsigned int cols() { return Dim[1]; }
    S4 wrap() { return *own; }
    struct InnerIterator {
        SparseMatrix& m;
        int index, max_index;
        InnerIterator(SparseMatrix& m_, int col) : m(m_), index(m_.p[col]), max_index(m_.p[col + 1]) {}
        operator bool() const { return index < max_index; }
        InnerIterator& operator++() { ++index; return *this; }
        double value() const { return m.x[index]; }
        int row() const { return m.i[index]; }
    };
};

// Named("w") = value: a (name, value) pair for List::create
struct Named {
    const char* n;
    Named(const char* n_) : n(n_) {}
    template <class T> std::pair<std::string, T> operator=(const T& t) { return {n, t}; }
    std::pair<std::string, Eigen::MatrixXd> operator=(Eigen::Transposed<double> t) { return {n, Eigen::MatrixXd(t)}; }
};

// a list of sparse matrices on the way in (iterated by the chunk-list drivers), named results on the way out
struct List {
    std::vector<SparseMatrix> items;
    std::vector<SparseMatrix>::iterator begin() { return items.begin(); }
    std::vector<SparseMatrix>::iterator end() { return items.end(); }

    Eigen::MatrixXd w, h;
    Eigen::VectorXd d;
    NumericVector test_mse, tol, score_overfit;
    IntegerVector iter;
    void put(const std::string& n, const Eigen::MatrixXd& m) {
        if (n == "w") w = m; else if (n == "h") h = m; else throw std::invalid_argument("List: matrix " + n);
    }
    void put(const std::string& n, const Eigen::VectorXd& x) {
        if (n == "d") d = x; else throw std::invalid_argument("List: vector " + n);
    }
    void put(const std::string& n, const NumericVector& x) {
        if (n == "test_mse") test_mse = x; else if (n == "tol") tol = x; else if (n == "score_overfit") score_overfit = x;
        else throw std::invalid_argument("List: numeric " + n);
    }
    void put(const std::string& n, const IntegerVector& x) {
        if (n == "iter") iter = x; else throw std::invalid_argument("List: integer " + n);
    }
    template <class... P> static List create(const P&... p) { List l; (l.put(p.first, p.second), ...); return l; }
};

inline void checkUserInterrupt() {}
}  // namespace Rcpp

// Rprintf appends to a buffer that the shim reads the drivers' iteration lines from
inline std::string& standin_output() { static thread_local std::string s; return s; }
inline void Rprintf(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    standin_output() += buf;
}
