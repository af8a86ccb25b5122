// Stand-in for the few Eigen names the reference's ALS functions use (src/singlet.cpp), so that the reference's own
// statements -- cut out of its tree at build time by oracle/make_ref.sh, never committed -- compile without Eigen.
// Written from the Eigen documentation's meaning of each call, not from Eigen's source.  Test infrastructure only.
//
// No expression templates: every operation evaluates at once, in the order written.  Storage is column-major, as
// Eigen's default.  No bounds checks beyond what Eigen's release build does (none), except where noted.
//
// What this header OWNS, i.e. arithmetic the reference delegates to Eigen and that is therefore not the reference's
// text: the reductions (rank update, row-wise sum, sum, row * column, matrix * column).  Their summation order is
// selectable at compile time: ascending by default (the order oracle/singlet_oracle.c uses), descending with
// -DSTANDIN_DESCENDING.  Two libraries are built from one cut; their difference measures this header's freedom.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace Eigen {
enum { Lower = 1, Upper = 2 };

#ifdef STANDIN_DESCENDING
#define STANDIN_REDUCE(q, n) for (size_t q##_ = (n), q = q##_ - 1; q##_ > 0; --q##_, q = q##_ - 1)
#else
#define STANDIN_REDUCE(q, n) for (size_t q = 0; q < (n); ++q)
#endif

// s * column (either operand order): consumed by `+=` / `-=` of a vector or a column
struct ScaledCol {
    const double* p;
    size_t n;
    double s;
};
struct ArrayRef {   // x.array(): element-wise `+= scalar`, `/= scalar`
    double* p;
    size_t n, stride;
    void operator+=(double v) { for (size_t q = 0; q < n; ++q) p[q * stride] += v; }
    void operator/=(double v) { for (size_t q = 0; q < n; ++q) p[q * stride] /= v; }
};
struct ColView {
    double* p;
    size_t n;
    ColView& operator=(const ColView& o) { for (size_t q = 0; q < n; ++q) p[q] = o.p[q]; return *this; }
    ColView& operator+=(ScaledCol c) { for (size_t q = 0; q < n; ++q) p[q] += c.s * c.p[q]; return *this; }
    ArrayRef array() { return {p, n, 1}; }
    double sum() const { double s = 0; STANDIN_REDUCE(q, n) s += p[q]; return s; }
};
inline ScaledCol operator*(double s, ColView c) { return {c.p, c.n, s}; }
inline ScaledCol operator*(ColView c, double s) { return {c.p, c.n, s}; }
struct RowView {
    const double* p;
    size_t n, stride;
};
inline double operator*(RowView r, ColView c) { double s = 0; STANDIN_REDUCE(q, r.n) s += r.p[q * r.stride] * c.p[q]; return s; }
struct DiagRef {
    double* p;
    size_t n, stride;
    ArrayRef array() { return {p, n, stride}; }
};

struct VectorXd {
    std::vector<double> v;
    VectorXd() {}
    explicit VectorXd(size_t n) : v(n) {}
    static VectorXd Zero(size_t n) { return VectorXd(n); }
    static VectorXd Ones(size_t n) { VectorXd r(n); r.setOnes(); return r; }
    void setOnes() { for (auto& e : v) e = 1.0; }
    size_t size() const { return v.size(); }
    double& operator()(size_t i) { return v[i]; }
    double operator()(size_t i) const { return v[i]; }
    double& operator[](size_t i) { return v[i]; }
    double operator[](size_t i) const { return v[i]; }
    VectorXd& operator+=(ScaledCol c) { for (size_t q = 0; q < c.n; ++q) v[q] += c.s * c.p[q]; return *this; }
    VectorXd& operator-=(ScaledCol c) { for (size_t q = 0; q < c.n; ++q) v[q] -= c.p[q] * c.s; return *this; }
    ArrayRef array() { return {v.data(), v.size(), 1}; }
    double sum() const { double s = 0; STANDIN_REDUCE(q, v.size()) s += v[q]; return s; }
};

template <class T> struct Matrix;
template <class T> struct Transposed { const Matrix<T>& m; };
struct RowwiseRef { const Matrix<double>& m; VectorXd sum() const; };
struct LowerView { Matrix<double>& m; void rankUpdate(const Matrix<double>& A); };
struct UpperView { Matrix<double>& m; void operator=(Transposed<double> t); };

template <class T> struct Matrix {
    std::vector<T> v;
    size_t r = 0, c = 0;
    Matrix() {}
    Matrix(size_t r_, size_t c_) : v(r_ * c_), r(r_), c(c_) {}
    Matrix(Transposed<T> t) : v(t.m.r * t.m.c), r(t.m.c), c(t.m.r) {
        for (size_t j = 0; j < c; ++j) for (size_t i = 0; i < r; ++i) (*this)(i, j) = t.m(j, i);
    }
    static Matrix Zero(size_t r, size_t c) { return Matrix(r, c); }
    void setZero() { for (auto& e : v) e = 0; }
    size_t rows() const { return r; }
    size_t cols() const { return c; }
    size_t size() const { return r * c; }
    T* data() { return v.data(); }
    const T* data() const { return v.data(); }
    T& operator()(size_t i, size_t j) { return v[i + j * r]; }
    T operator()(size_t i, size_t j) const { return v[i + j * r]; }
    ColView col(size_t j) const { return {const_cast<T*>(v.data()) + j * r, r}; }
    RowView row(size_t i) const { return {v.data() + i, c, r}; }
    Transposed<T> transpose() const { return {*this}; }
    RowwiseRef rowwise() const { return {*this}; }
    DiagRef diagonal() { return {v.data(), r, r + 1}; }
    template <int M> LowerView selfadjointView() { return {*this}; }
    template <int M> UpperView triangularView() { return {*this}; }
    Matrix operator-(const Matrix& o) const { Matrix x(r, c); for (size_t q = 0; q < v.size(); ++q) x.v[q] = v[q] - o.v[q]; return x; }
};
typedef Matrix<double> MatrixXd;
typedef Matrix<int> MatrixXi;

// matrix * column: the columns of the matrix scaled and added in turn (a reduction this header owns)
inline VectorXd operator*(const MatrixXd& m, ColView x) {
    VectorXd b(m.r);
    STANDIN_REDUCE(j, m.c) for (size_t i = 0; i < m.r; ++i) b.v[i] += x.p[j] * m(i, j);
    return b;
}
// d(i) = sum over the columns of row i
inline VectorXd RowwiseRef::sum() const {
    VectorXd d(m.r);
    STANDIN_REDUCE(j, m.c) for (size_t i = 0; i < m.r; ++i) d.v[i] += m(i, j);
    return d;
}
// lower triangle += A * A^T
inline void LowerView::rankUpdate(const MatrixXd& A) {
    for (size_t j = 0; j < A.r; ++j)
        for (size_t i = j; i < A.r; ++i) {
            double s = 0;
            STANDIN_REDUCE(q, A.c) s += A(i, q) * A(j, q);
            m(i, j) += s;
        }
}
// strictly upper triangle = that of the transpose
inline void UpperView::operator=(Transposed<double> t) {
    for (size_t j = 0; j < m.c; ++j) for (size_t i = 0; i < j; ++i) m(i, j) = t.m(j, i);
}
}  // namespace Eigen
