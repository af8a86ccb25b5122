/* R.h of the emulated R C API (see Rinternals.h in this directory). */
#ifndef R_EMUL_R_H
#define R_EMUL_R_H
#include <math.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

void Rprintf(const char*, ...) __attribute__((format(printf, 1, 2)));
void Rf_error(const char*, ...) __attribute__((noreturn, format(printf, 1, 2)));
char* R_alloc(size_t, int);
#define ISNAN(x) (isnan(x) != 0)

#ifdef __cplusplus
}
#endif
#endif
