/* R_ext/Utils.h of the emulated R C API (see ../Rinternals.h). */
#ifndef R_EMUL_UTILS_H
#define R_EMUL_UTILS_H
#ifdef __cplusplus
extern "C" {
#endif
void R_CheckUserInterrupt(void);
#ifdef __cplusplus
}
#endif
#endif
