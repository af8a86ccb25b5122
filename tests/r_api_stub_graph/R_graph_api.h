/* Prototype-only declarations of the R C API names that singlet_amd/r/singlet_hip_graph_shim.c uses beyond those of
 * tests/r_api_stub/ (which stays as it is): reading a string, building a new S4 object.  Force-included by
 * tests/test_graph_shim_on_cpu.py for a syntax check; nothing here is linked or run. */
#ifndef R_GRAPH_API_STUB_H
#define R_GRAPH_API_STUB_H
#include <Rinternals.h>
SEXP STRING_ELT(SEXP, R_xlen_t);
const char* R_CHAR(SEXP);
Rboolean Rf_isString(SEXP);
SEXP R_do_MAKE_CLASS(const char*);
SEXP R_do_new_object(SEXP);
SEXP R_do_slot_assign(SEXP, SEXP, SEXP);
#endif
