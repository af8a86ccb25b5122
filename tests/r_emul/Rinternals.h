/* A working emulation of the part of R's C API that the two sources of singlet_amd/r/ use, written from the behaviour "Writing R
 * Extensions" documents (tests/r_emul/r_emul.c holds the bodies).  The two shim sources compile against this header
 * unmodified and link into tests/r_emul/libsinglet_hip_shim_emul.so, which tests/r_shim_emul.py drives from Python.
 * It is test infrastructure: a build against R's own headers is still to be made where R exists. */
#ifndef R_EMUL_RINTERNALS_H
#define R_EMUL_RINTERNALS_H
#include <limits.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SEXPREC* SEXP;
typedef ptrdiff_t R_xlen_t;
typedef enum { FALSE = 0, TRUE } Rboolean;

#define NILSXP 0
#define SYMSXP 1
#define CHARSXP 9
#define LGLSXP 10
#define INTSXP 13
#define REALSXP 14
#define STRSXP 16
#define VECSXP 19
#define S4SXP 25

#define NA_INTEGER INT_MIN
#define NA_LOGICAL INT_MIN

extern SEXP R_NilValue;
extern SEXP R_NamesSymbol;
extern SEXP R_DimSymbol;
extern double R_NaReal;
#define NA_REAL R_NaReal

int TYPEOF(SEXP);
R_xlen_t XLENGTH(SEXP);
double* REAL(SEXP);
int* INTEGER(SEXP);
int* LOGICAL(SEXP);
SEXP VECTOR_ELT(SEXP, R_xlen_t);
SEXP SET_VECTOR_ELT(SEXP, R_xlen_t, SEXP);
SEXP STRING_ELT(SEXP, R_xlen_t);
void SET_STRING_ELT(SEXP, R_xlen_t, SEXP);
const char* R_CHAR(SEXP);

SEXP Rf_install(const char*);
SEXP Rf_mkChar(const char*);
SEXP Rf_allocVector(unsigned int, R_xlen_t);
SEXP Rf_allocMatrix(unsigned int, int, int);
SEXP Rf_protect(SEXP);
void Rf_unprotect(int);
#define PROTECT(s) Rf_protect(s)
#define UNPROTECT(n) Rf_unprotect(n)

SEXP Rf_setAttrib(SEXP, SEXP, SEXP);
SEXP Rf_getAttrib(SEXP, SEXP);
Rboolean Rf_isMatrix(SEXP);
Rboolean Rf_isString(SEXP);
int Rf_nrows(SEXP);
int Rf_ncols(SEXP);
int Rf_asLogical(SEXP);
int Rf_asInteger(SEXP);
double Rf_asReal(SEXP);

int R_has_slot(SEXP, SEXP);
SEXP R_do_slot(SEXP, SEXP);
SEXP R_do_slot_assign(SEXP, SEXP, SEXP);
SEXP R_do_MAKE_CLASS(const char*);
SEXP R_do_new_object(SEXP);

Rboolean R_ToplevelExec(void (*)(void*), void*);
void Rf_onintr(void) __attribute__((noreturn));

#ifdef __cplusplus
}
#endif
#endif
