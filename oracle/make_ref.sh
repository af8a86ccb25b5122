#!/bin/sh
# oracle/_ref: builds of the reference's OWN statements, cut out of its tree AT BUILD TIME into the git-ignored
# oracle/_ref/ and compiled there; no reference source is copied into the repository.
#
#   librng_ref.so     the `rng` class of src/singlet.cpp (xorshift hash behind the cross-validation mask and the
#                     synthetic generator), dependency-free C++; shim oracle/ref_rng_shim.cpp.
#   libals_ref.so     the ALS functions of src/singlet.cpp listed below, each cut from the line that starts with its
#   libals_ref_b.so   signature to the first line that starts with `}`, compiled against oracle/standin/ (own text: the
#                     few Eigen / Rcpp names those functions use) and oracle/ref_als_shim.cpp.  Variant A (libals_ref.so):
#                     the stand-in's reductions ascending, -ffp-contract=off -- the oracle's arithmetic.  Variant B
#                     (libals_ref_b.so): the same cut, reductions descending, -ffp-contract=fast with FMA where the
#                     CPU has it; A against B measures what the stand-in cannot pin (DESIGN.md "Oracle status").
#                     Both without OpenMP: the reference's `threads` is ignored, a run is repeatable.
#
# Needs the reference tree (SINGLET_REFERENCE, default /root/reference: the authoring container); elsewhere the
# prebuilt oracle/_ref/*.so travel with the snapshot and are kept.
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
REF=${SINGLET_REFERENCE:-/root/reference}
SRC="$REF/src/singlet.cpp"
if [ ! -f "$SRC" ]; then
    echo "make_ref.sh: $SRC not present (not the authoring container): keeping any prebuilt oracle/_ref" >&2
    exit 0
fi
mkdir -p "$HERE/_ref"
CXX=${CXX:-g++}
# from the line `class rng {` to the first line that is exactly `};`
awk '/^class rng \{/ {on = 1} on {print} on && /^\};/ {exit}' "$SRC" > "$HERE/_ref/rng_class.inc"
grep -q "uint64_t rand(uint64_t i, uint64_t j)" "$HERE/_ref/rng_class.inc" || { echo "make_ref.sh: rng class not found in $SRC" >&2; exit 1; }
$CXX -O2 -std=c++17 -fPIC -shared -fvisibility=hidden -w -I"$HERE" -o "$HERE/_ref/librng_ref.so" "$HERE/ref_rng_shim.cpp"
echo "built $HERE/_ref/librng_ref.so from $SRC"

# The ALS functions, by the start of their signature line.  Each prefix must start exactly one line of the source; the
# overloads of predict / predict_mask / mse_test are told apart by their first parameter.  A `template <...>` line
# directly above a signature belongs to it.
cat > "$HERE/_ref/als_prefixes.txt" <<'EOF'
Rcpp::NumericMatrix rowwise_compress_sparse(
Rcpp::NumericMatrix rowwise_compress_dense(
inline double cor(
inline Eigen::MatrixXd AAt(
inline Eigen::MatrixXd submat(
void scale(
inline void nnls(
inline void predict(Rcpp::SparseMatrix A,
Eigen::MatrixXd Rcpp_predict(
inline void predict(Eigen::MatrixXd A,
inline void predict(std::vector<Rcpp::SparseMatrix> A,
Rcpp::List c_project_model(
inline void predict_link(
inline void predict_mask(Rcpp::SparseMatrix A,
inline void predict_mask(std::vector<Rcpp::SparseMatrix>& A,
inline void predict_mask(const Eigen::MatrixXd& A,
inline double mse_test(Rcpp::SparseMatrix A,
inline double mse_test(std::vector<Rcpp::SparseMatrix> A,
inline double mse_test(const Eigen::MatrixXd& A,
Rcpp::List c_nmf_base(
Rcpp::List c_nmf(
Rcpp::List c_nmf_sparse_list(
Rcpp::List c_nmf_dense(
Rcpp::List c_linked_nmf(
Rcpp::List c_ard_nmf_base(
Rcpp::List c_ard_nmf(
Rcpp::List c_ard_nmf_sparse_list(
Rcpp::List c_ard_nmf_dense(
Rcpp::S4 spatial_graph(
inline void gcnmf_update_h(
inline void gcnmf_update_w(
Rcpp::List c_gcnmf(
EOF
awk -v list="$HERE/_ref/als_prefixes.txt" '
    BEGIN { while ((getline line < list) > 0) if (line != "") { want[++nw] = line; seen[nw] = 0 } }
    !on { for (q = 1; q <= nw; ++q) if (index($0, want[q]) == 1) { on = 1; ++seen[q]; if (prev ~ /^template </) print prev; break } }
    on { print }
    on && /^\}/ { on = 0; print "" }
    { prev = $0 }
    END {
        bad = 0
        for (q = 1; q <= nw; ++q) if (seen[q] != 1) { printf "make_ref.sh: \"%s\" starts %d lines of the source, expected 1\n", want[q], seen[q] > "/dev/stderr"; bad = 1 }
        if (on) { print "make_ref.sh: the last cut function is not closed" > "/dev/stderr"; bad = 1 }
        exit bad
    }' "$SRC" > "$HERE/_ref/als_functions.inc" || { echo "make_ref.sh: cutting the ALS functions out of $SRC failed" >&2; exit 1; }

COMMON="-O2 -std=c++17 -fPIC -shared -fvisibility=hidden -w -I$HERE"
FMA=""
if grep -qw fma /proc/cpuinfo 2>/dev/null; then FMA="-mfma"; fi
$CXX $COMMON -ffp-contract=off -o "$HERE/_ref/libals_ref.so" "$HERE/ref_als_shim.cpp"
$CXX $COMMON -DSTANDIN_DESCENDING -ffp-contract=fast $FMA -o "$HERE/_ref/libals_ref_b.so" "$HERE/ref_als_shim.cpp"
echo "built $HERE/_ref/libals_ref.so and libals_ref_b.so from $SRC ($(wc -l < "$HERE/_ref/als_functions.inc") cut lines)"
