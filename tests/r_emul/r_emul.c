/*
 * r_emul.c -- a working emulation of the subset of R's C API that singlet_amd/r/singlet_hip_shim.c and
 * singlet_hip_graph_shim.c use, so that the unchanged shim sources run in a process without R.  Written from the
 * behaviour "Writing R Extensions" documents; test infrastructure only (tests/r_shim_emul.py drives it through ctypes).
 *
 * What it models, because the shim depends on it:
 *   - objects with a type, a length, data, the `dim` and `names` attributes, a class name and a slot table (S4);
 *   - the protect stack, and a collector run AT EVERY ALLOCATION ("torture"): every object that is not reachable from the
 *     protect stack, the arguments of the running call, the last returned value or the symbol table is poisoned -- payload
 *     overwritten, `alive` cleared -- and stays allocated, so that a later access is recorded as a "use after collection"
 *     event instead of crashing;
 *   - no emulated function aborts the process: an R error raised while no .Call is running (the driver calling an API
 *     function directly) is recorded as an "R error outside a call" event and the function returns a harmless value
 *     (R_NilValue, 0, a scratch buffer).  Only Rf_error and Rf_onintr themselves cannot return: the driver does not bind
 *     them, and an entry reaches them under emul_call only;
 *   - non-local exits: Rf_error and Rf_onintr long-jump to the trampoline emul_call, R_CheckUserInterrupt to the innermost
 *     R_ToplevelExec when the test armed an interrupt; the protect stack and the R_alloc memory are reset as R does;
 *   - .Call through the table R_registerRoutines received, with the registered arity enforced.
 */
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Rdynload.h>
#include <R_ext/Utils.h>

#include <setjmp.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ---- objects ------------------------------------------------------------------------------------------------------- */
#define MAX_SLOTS 8
#define CLASSDEF_TYPE 100 /* what R_do_MAKE_CLASS returns: only R_do_new_object reads it */

struct SEXPREC {
    int type;
    R_xlen_t length;
    void* data;   /* payload: doubles, ints, SEXPs (VECSXP, STRSXP) or chars (CHARSXP, SYMSXP, class definitions) */
    size_t bytes;
    SEXP dim, names;
    char* class_name;
    int nslots;
    SEXP slot_name[MAX_SLOTS], slot_value[MAX_SLOTS];
    int alive, pinned, mark;
    SEXP next;
};

static struct SEXPREC nil_object = {NILSXP, 0, NULL, 0, NULL, NULL, NULL, 0, {NULL}, {NULL}, 1, 1, 0, NULL};
static struct SEXPREC dead_object = {NILSXP, 0, NULL, 0, NULL, NULL, NULL, 0, {NULL}, {NULL}, 0, 1, 0, NULL};
SEXP R_NilValue = &nil_object;
SEXP R_NamesSymbol = NULL;
SEXP R_DimSymbol = NULL;
double R_NaReal;

static SEXP all_objects = NULL;
static long n_objects = 0, n_poisoned = 0;

/* ---- bookkeeping the tests read back ------------------------------------------------------------------------------ */
#define MAX_PROTECT 10000
static SEXP protect_stack[MAX_PROTECT];
static int protect_depth = 0;

#define MAX_EVENTS 64
static char events[MAX_EVENTS][96];
static int n_events = 0;

static char* out_text = NULL;
static size_t out_len = 0, out_cap = 0;

static long n_polls = 0, interrupt_from_poll = 0; /* 0: no interrupt pending */

enum { KIND_OK = 0, KIND_ERROR = 1, KIND_INTERRUPT = 2, KIND_REFUSED = 3 };
static char last_message[1024];
static int last_kind = KIND_OK, last_delta = 0, last_delta_at_exit = 0;
static SEXP last_value = NULL;

typedef struct ralloc_block { struct ralloc_block* next; } ralloc_block;
static ralloc_block* ralloc_top = NULL;

#define MAX_FRAMES 16
typedef struct {
    jmp_buf jb;
    int depth;
    ralloc_block* vmax;
} frame;
static frame frames[MAX_FRAMES];
static int n_frames = 0;
static int exit_depth = 0; /* protect depth at the moment of the last long jump */

static SEXP* call_args = NULL;
static int call_nargs = 0;

static const R_CallMethodDef* registered = NULL;
static int dynamic_symbols = 1;
struct _DllInfo { int unused; };
static struct _DllInfo the_dll;

static void ensure_init(void);

static void event(const char* what, const char* where) {
    if (n_events < MAX_EVENTS) snprintf(events[n_events], sizeof events[0], "%s: %s", what, where);
    ++n_events;
}

/* An R error of the emulator's own functions (defined with the non-local exits below): FAIL raises it and, where it
 * comes back because no .Call is running, returns the function's harmless value. */
static void raise_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
#define FAIL(value, ...) do { raise_error(__VA_ARGS__); return value; } while (0)

static double scratch_numbers[2];
static SEXP scratch_element;

/* every accessor goes through this: a collected object is reported, never dereferenced as if it were alive */
static SEXP use(SEXP s, const char* accessor) {
    if (s == NULL) {
        event("NULL pointer", accessor);
        return &dead_object;
    }
    if (!s->alive) event("use after collection", accessor);
    return s;
}

/* ---- the collector -------------------------------------------------------------------------------------------------- */
static void mark(SEXP s) {
    if (s == NULL || s->mark) return;
    s->mark = 1;
    mark(s->dim);
    mark(s->names);
    for (int q = 0; q < s->nslots; ++q) {
        mark(s->slot_name[q]);
        mark(s->slot_value[q]);
    }
    if ((s->type == VECSXP || s->type == STRSXP) && s->alive)
        for (R_xlen_t q = 0; q < s->length; ++q) mark(((SEXP*)s->data)[q]);
}

static void poison(SEXP s) {
    s->alive = 0;
    ++n_poisoned;
    if (s->type == VECSXP || s->type == STRSXP) {
        for (R_xlen_t q = 0; q < s->length; ++q) ((SEXP*)s->data)[q] = &dead_object;
    } else if (s->type == REALSXP) {
        const uint64_t snan = 0x7FF4DEADDEADDEADull; /* a signalling NaN */
        for (R_xlen_t q = 0; q < s->length; ++q) memcpy((double*)s->data + q, &snan, 8);
    } else if (s->type == INTSXP || s->type == LGLSXP) {
        for (R_xlen_t q = 0; q < s->length; ++q) ((int*)s->data)[q] = (int)0xDEADDEAD;
    } else if (s->data != NULL && s->bytes > 0) {
        memset(s->data, '#', s->bytes - 1);
    }
    s->dim = s->names = NULL;
    for (int q = 0; q < s->nslots; ++q) s->slot_value[q] = &dead_object;
}

static void collect(void) {
    for (SEXP s = all_objects; s != NULL; s = s->next) s->mark = 0;
    for (int q = 0; q < protect_depth; ++q) mark(protect_stack[q]);
    for (int q = 0; q < call_nargs; ++q) mark(call_args[q]);
    mark(last_value);
    for (SEXP s = all_objects; s != NULL; s = s->next)
        if (s->pinned) mark(s);
    for (SEXP s = all_objects; s != NULL; s = s->next)
        if (!s->mark && s->alive) poison(s);
}

static SEXP new_object(int type, R_xlen_t length, size_t elt) {
    ensure_init();
    collect();
    SEXP s = (SEXP)calloc(1, sizeof *s);
    if (s == NULL) FAIL(R_NilValue, "emulator: out of memory");
    s->type = type;
    s->length = length;
    s->bytes = (size_t)length * elt;
    s->data = calloc(s->bytes ? s->bytes : 1, 1);
    if (s->data == NULL) {
        free(s);
        FAIL(R_NilValue, "emulator: cannot allocate a vector of %lld bytes", (long long)((size_t)length * elt));
    }
    s->alive = 1;
    s->next = all_objects;
    all_objects = s;
    ++n_objects;
    if (type == VECSXP || type == STRSXP)
        for (R_xlen_t q = 0; q < length; ++q) ((SEXP*)s->data)[q] = R_NilValue;
    return s;
}

static SEXP new_chars(int type, const char* text) {
    const size_t n = strlen(text);
    SEXP s = new_object(type, (R_xlen_t)n, 1);
    if (s == R_NilValue) return s;
    free(s->data);
    s->data = calloc(n + 1, 1);
    s->bytes = n + 1;
    if (s->data != NULL) memcpy(s->data, text, n);
    return s;
}

static void ensure_init(void) {
    static int done = 0;
    if (done) return;
    done = 1;
    const uint64_t na = 0x7FF00000000007A2ull; /* R's NA_real_: a NaN whose low word is 1954 */
    memcpy(&R_NaReal, &na, 8);
    R_NamesSymbol = Rf_install("names");
    R_DimSymbol = Rf_install("dim");
}

/* ---- non-local exits ------------------------------------------------------------------------------------------------ */
static void release_ralloc(ralloc_block* down_to) {
    while (ralloc_top != down_to && ralloc_top != NULL) {
        ralloc_block* b = ralloc_top;
        ralloc_top = b->next;
        free(b);
    }
}

static void jump(int kind) __attribute__((noreturn));
static void jump(int kind) {
    if (n_frames == 0) { /* no .Call is running: a mistake of the test driver, which has nowhere to return to */
        fprintf(stderr, "r_emul: Rf_error / Rf_onintr called while no .Call is running: %s\n", last_message);
        abort(); /* only these two, which cannot return; see the header */
    }
    exit_depth = protect_depth;
    longjmp(frames[n_frames - 1].jb, kind);
}

/* An R error of the emulator's own functions: the long jump when a .Call is running; otherwise an event, and the caller
 * returns its harmless value. */
static void raise_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_message, sizeof last_message, fmt, ap);
    va_end(ap);
    if (n_frames > 0) jump(KIND_ERROR);
    last_kind = KIND_ERROR;
    event("R error outside a call", last_message);
}

void Rf_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_message, sizeof last_message, fmt, ap);
    va_end(ap);
    jump(KIND_ERROR);
}

void Rf_onintr(void) {
    snprintf(last_message, sizeof last_message, "interrupted");
    jump(KIND_INTERRUPT);
}

void R_CheckUserInterrupt(void) {
    ++n_polls;
    if (interrupt_from_poll > 0 && n_polls >= interrupt_from_poll) {
        snprintf(last_message, sizeof last_message, "interrupted");
        if (n_frames == 0) {
            event("interrupt outside a call", "R_CheckUserInterrupt");
            return;
        }
        jump(KIND_INTERRUPT);
    }
}

Rboolean R_ToplevelExec(void (*fn)(void*), void* data) {
    if (n_frames >= MAX_FRAMES) FAIL(FALSE, "emulator: R_ToplevelExec nested too deeply");
    frame* f = &frames[n_frames];
    f->depth = protect_depth;
    f->vmax = ralloc_top;
    ++n_frames;
    if (setjmp(f->jb) != 0) { /* an error or an interrupt inside fn: R reports both as FALSE */
        --n_frames;
        protect_depth = frames[n_frames].depth;
        release_ralloc(frames[n_frames].vmax);
        last_message[0] = 0; /* the condition ends here */
        return FALSE;
    }
    fn(data);
    --n_frames;
    return TRUE;
}

/* ---- output, transient memory --------------------------------------------------------------------------------------- */
void Rprintf(const char* fmt, ...) {
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    int n = vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (n < 0) return;
    if ((size_t)n >= sizeof buf) n = (int)sizeof buf - 1;
    if (out_len + (size_t)n + 1 > out_cap) {
        size_t cap = out_cap ? out_cap * 2 : 4096;
        while (cap < out_len + (size_t)n + 1) cap *= 2;
        char* p = (char*)realloc(out_text, cap);
        if (p == NULL) return;
        out_text = p;
        out_cap = cap;
    }
    memcpy(out_text + out_len, buf, (size_t)n);
    out_len += (size_t)n;
    out_text[out_len] = 0;
}

char* R_alloc(size_t n, int size) {
    const size_t bytes = n * (size_t)(size > 0 ? size : 0);
    ralloc_block* b = (ralloc_block*)malloc(sizeof(ralloc_block) + 16 + (bytes ? bytes : 1));
    if (b == NULL) FAIL((char*)scratch_numbers, "emulator: R_alloc of %lld bytes failed", (long long)bytes);
    b->next = ralloc_top;
    ralloc_top = b;
    return (char*)b + 16; /* sizeof(ralloc_block) <= 16: keeps the payload 16-byte aligned */
}

/* ---- allocation, protection ----------------------------------------------------------------------------------------- */
SEXP Rf_allocVector(unsigned int type, R_xlen_t n) {
    if (n < 0) FAIL(R_NilValue, "negative length vectors are not allowed");
    switch (type) {
        case REALSXP: return new_object(REALSXP, n, sizeof(double));
        case INTSXP: return new_object(INTSXP, n, sizeof(int));
        case LGLSXP: return new_object(LGLSXP, n, sizeof(int));
        case VECSXP: return new_object(VECSXP, n, sizeof(SEXP));
        case STRSXP: return new_object(STRSXP, n, sizeof(SEXP));
        default: FAIL(R_NilValue, "allocVector: type %u is not emulated", type);
    }
}

SEXP Rf_allocMatrix(unsigned int type, int nrow, int ncol) {
    if (nrow < 0 || ncol < 0) FAIL(R_NilValue, "negative extents to matrix");
    SEXP s = Rf_allocVector(type, (R_xlen_t)nrow * ncol);
    if (s == R_NilValue) return s;
    PROTECT(s);
    SEXP dim = Rf_allocVector(INTSXP, 2);
    if (dim == R_NilValue) {
        UNPROTECT(1);
        return dim;
    }
    ((int*)dim->data)[0] = nrow;
    ((int*)dim->data)[1] = ncol;
    s->dim = dim;
    UNPROTECT(1);
    return s;
}

SEXP Rf_protect(SEXP s) {
    if (protect_depth >= MAX_PROTECT) FAIL(s, "protect(): protection stack overflow");
    protect_stack[protect_depth++] = s;
    return s;
}

void Rf_unprotect(int n) {
    if (n > protect_depth) {
        event("unprotect(): stack imbalance", "Rf_unprotect");
        n = protect_depth;
    }
    protect_depth -= n;
}

SEXP Rf_install(const char* name) {
    ensure_init();
    for (SEXP s = all_objects; s != NULL; s = s->next)
        if (s->type == SYMSXP && strcmp((const char*)s->data, name) == 0) return s;
    SEXP s = new_chars(SYMSXP, name);
    s->pinned = 1; /* the symbol table is a root */
    return s;
}

SEXP Rf_mkChar(const char* text) { return new_chars(CHARSXP, text); }

/* ---- accessors ------------------------------------------------------------------------------------------------------- */
int TYPEOF(SEXP s) { return use(s, "TYPEOF")->type; }
R_xlen_t XLENGTH(SEXP s) { return use(s, "XLENGTH")->length; }

double* REAL(SEXP s) {
    s = use(s, "REAL");
    if (s->type != REALSXP) FAIL(scratch_numbers, "REAL() can only be applied to a 'numeric', not type %d", s->type);
    return (double*)s->data;
}

int* INTEGER(SEXP s) {
    s = use(s, "INTEGER");
    if (s->type != INTSXP && s->type != LGLSXP) FAIL((int*)scratch_numbers, "INTEGER() can only be applied to a 'integer', not type %d", s->type);
    return (int*)s->data;
}

int* LOGICAL(SEXP s) {
    s = use(s, "LOGICAL");
    if (s->type != LGLSXP) FAIL((int*)scratch_numbers, "LOGICAL() can only be applied to a 'logical', not type %d", s->type);
    return (int*)s->data;
}

static SEXP* element(SEXP s, R_xlen_t q, int type, const char* accessor) {
    s = use(s, accessor);
    scratch_element = R_NilValue;
    if (s->type != type) FAIL(&scratch_element, "%s() applied to an object of type %d", accessor, s->type);
    if (q < 0 || q >= s->length) FAIL(&scratch_element, "%s(): subscript %lld out of bounds (length %lld)", accessor, (long long)q, (long long)s->length);
    return (SEXP*)s->data + q;
}

SEXP VECTOR_ELT(SEXP s, R_xlen_t q) { return *element(s, q, VECSXP, "VECTOR_ELT"); }

SEXP SET_VECTOR_ELT(SEXP s, R_xlen_t q, SEXP v) {
    SEXP* slot = element(s, q, VECSXP, "SET_VECTOR_ELT");
    *slot = use(v, "SET_VECTOR_ELT (value)");
    return v;
}

SEXP STRING_ELT(SEXP s, R_xlen_t q) { return *element(s, q, STRSXP, "STRING_ELT"); }

void SET_STRING_ELT(SEXP s, R_xlen_t q, SEXP v) {
    SEXP* slot = element(s, q, STRSXP, "SET_STRING_ELT");
    v = use(v, "SET_STRING_ELT (value)");
    if (v->type != CHARSXP) FAIL(, "SET_STRING_ELT() needs a CHARSXP, not type %d", v->type);
    *slot = v;
}

const char* R_CHAR(SEXP s) {
    s = use(s, "R_CHAR");
    if (s->type != CHARSXP) FAIL("", "CHAR() can only be applied to a 'CHARSXP', not type %d", s->type);
    return (const char*)s->data;
}

/* ---- attributes ------------------------------------------------------------------------------------------------------ */
SEXP Rf_setAttrib(SEXP s, SEXP name, SEXP value) {
    s = use(s, "Rf_setAttrib");
    value = use(value, "Rf_setAttrib (value)");
    if (name == R_NamesSymbol) {
        if (value->type != STRSXP || value->length != s->length) FAIL(R_NilValue, "'names' attribute must be a character vector of the object's length");
        s->names = value;
    } else if (name == R_DimSymbol) {
        if (value->type != INTSXP) FAIL(R_NilValue, "invalid 'dim' attribute");
        R_xlen_t total = 1;
        for (R_xlen_t q = 0; q < value->length; ++q) total *= ((int*)value->data)[q];
        if (total != s->length) FAIL(R_NilValue, "dims do not match the length of object");
        s->dim = value;
    } else {
        FAIL(R_NilValue, "setAttrib: only 'names' and 'dim' are emulated");
    }
    return value;
}

SEXP Rf_getAttrib(SEXP s, SEXP name) {
    s = use(s, "Rf_getAttrib");
    SEXP v = name == R_NamesSymbol ? s->names : name == R_DimSymbol ? s->dim : NULL;
    return v != NULL ? v : R_NilValue;
}

static int is_vector_type(int t) { return t == LGLSXP || t == INTSXP || t == REALSXP || t == STRSXP || t == VECSXP; }

Rboolean Rf_isMatrix(SEXP s) {
    s = use(s, "Rf_isMatrix");
    return (is_vector_type(s->type) && s->dim != NULL && s->dim->length == 2) ? TRUE : FALSE;
}

Rboolean Rf_isString(SEXP s) { return use(s, "Rf_isString")->type == STRSXP ? TRUE : FALSE; }

int Rf_nrows(SEXP s) {
    s = use(s, "Rf_nrows");
    if (!is_vector_type(s->type)) FAIL(0, "object is not a matrix");
    if (s->dim == NULL) return (int)s->length;
    return ((int*)s->dim->data)[0];
}

int Rf_ncols(SEXP s) {
    s = use(s, "Rf_ncols");
    if (!is_vector_type(s->type)) FAIL(0, "object is not a matrix");
    if (s->dim == NULL || s->dim->length < 2) return 1;
    return ((int*)s->dim->data)[1];
}

/* ---- scalar conversions (R's coerceVector rules for length-1 logical, integer and double vectors) -------------------- */
double Rf_asReal(SEXP s) {
    s = use(s, "Rf_asReal");
    ensure_init();
    if (s->length < 1) return R_NaReal;
    if (s->type == REALSXP) return ((double*)s->data)[0];
    if (s->type == INTSXP || s->type == LGLSXP) {
        const int v = ((int*)s->data)[0];
        return v == NA_INTEGER ? R_NaReal : (double)v;
    }
    return R_NaReal;
}

int Rf_asInteger(SEXP s) {
    s = use(s, "Rf_asInteger");
    if (s->length < 1) return NA_INTEGER;
    if (s->type == INTSXP || s->type == LGLSXP) return ((int*)s->data)[0];
    if (s->type == REALSXP) {
        const double v = ((double*)s->data)[0];
        if (isnan(v) || v >= 2147483648.0 || v <= -2147483649.0) return NA_INTEGER;
        return (int)v; /* toward zero */
    }
    return NA_INTEGER;
}

int Rf_asLogical(SEXP s) {
    s = use(s, "Rf_asLogical");
    if (s->length < 1) return NA_LOGICAL;
    if (s->type == LGLSXP) return ((int*)s->data)[0];
    if (s->type == INTSXP) {
        const int v = ((int*)s->data)[0];
        return v == NA_INTEGER ? NA_LOGICAL : v != 0;
    }
    if (s->type == REALSXP) {
        const double v = ((double*)s->data)[0];
        return isnan(v) ? NA_LOGICAL : v != 0;
    }
    return NA_LOGICAL;
}

/* ---- S4: slots -------------------------------------------------------------------------------------------------------- */
static int find_slot(SEXP s, SEXP name) {
    for (int q = 0; q < s->nslots; ++q)
        if (s->slot_name[q] == name) return q;
    return -1;
}

int R_has_slot(SEXP s, SEXP name) { return find_slot(use(s, "R_has_slot"), name) >= 0; }

SEXP R_do_slot(SEXP s, SEXP name) {
    s = use(s, "R_do_slot");
    const int q = find_slot(s, name);
    if (q < 0)
        FAIL(R_NilValue, "no slot of name \"%s\" for this object of class \"%s\"", name != NULL && name->type == SYMSXP ? (const char*)name->data : "?",
                 s->class_name != NULL ? s->class_name : "?");
    return s->slot_value[q];
}

SEXP R_do_slot_assign(SEXP s, SEXP name, SEXP value) {
    s = use(s, "R_do_slot_assign");
    value = use(value, "R_do_slot_assign (value)");
    int q = find_slot(s, name);
    if (q < 0) {
        if (s->nslots >= MAX_SLOTS) FAIL(s, "emulator: more than %d slots", MAX_SLOTS);
        q = s->nslots++;
        s->slot_name[q] = name;
    }
    s->slot_value[q] = value;
    return s;
}

SEXP R_do_MAKE_CLASS(const char* name) {
    if (name == NULL) FAIL(R_NilValue, "R_do_MAKE_CLASS: C-level MAKE_CLASS macro called with NULL string pointer");
    return new_chars(CLASSDEF_TYPE, name);
}

SEXP R_do_new_object(SEXP class_def) {
    class_def = use(class_def, "R_do_new_object");
    if (class_def->type != CLASSDEF_TYPE) FAIL(R_NilValue, "C level NEW macro called with null class definition pointer");
    PROTECT(class_def);
    SEXP s = new_object(S4SXP, 0, 1);
    UNPROTECT(1);
    if (s == R_NilValue) return s;
    s->class_name = strdup((const char*)class_def->data);
    return s;
}

/* ---- registration ------------------------------------------------------------------------------------------------------ */
int R_registerRoutines(DllInfo* dll, const void* c_routines, const R_CallMethodDef* call_routines, const void* fortran_routines,
                       const void* external_routines) {
    (void)dll; (void)c_routines; (void)fortran_routines; (void)external_routines;
    registered = call_routines;
    return 1;
}

Rboolean R_useDynamicSymbols(DllInfo* dll, Rboolean value) {
    (void)dll;
    const Rboolean old = dynamic_symbols ? TRUE : FALSE;
    dynamic_symbols = value != FALSE;
    return old;
}

/* ======================================================================================================================
 * What follows is the test driver's side (ctypes): the trampoline, helpers that build and read objects, and four small
 * entries on which the emulator's own behaviour is checked.
 * ====================================================================================================================== */

typedef void (*generic_fn)(void); /* C's generic function pointer type: a cast through it is not reported */

/* self-test entries, three arguments each (called by name through emul_call like the registered ones) */
static SEXP selftest_error(SEXP a, SEXP b, SEXP c) {
    (void)b; (void)c;
    PROTECT(Rf_allocVector(REALSXP, 3));
    PROTECT(Rf_allocVector(INTSXP, 2));
    (void)R_alloc(100, sizeof(double));
    Rf_error("self-test error %d: %s", Rf_asInteger(a), "as asked");
}

static SEXP selftest_use_after(SEXP a, SEXP b, SEXP c) {
    (void)a; (void)b; (void)c;
    SEXP lost = Rf_allocVector(REALSXP, 4); /* not protected ... */
    REAL(lost)[0] = 1.0;
    SEXP kept = PROTECT(Rf_allocVector(REALSXP, 4)); /* ... so this allocation may collect it */
    REAL(kept)[0] = REAL(lost)[0];                   /* the offence */
    UNPROTECT(1);
    return kept;
}

static void selftest_poll(void* data) { (void)data; R_CheckUserInterrupt(); }

static SEXP selftest_toplevel(SEXP a, SEXP b, SEXP c) {
    (void)b; (void)c;
    const int n = Rf_asInteger(a);
    SEXP out = PROTECT(Rf_allocVector(LGLSXP, n));
    for (int q = 0; q < n; ++q) LOGICAL(out)[q] = R_ToplevelExec(selftest_poll, NULL);
    UNPROTECT(1);
    return out;
}

static SEXP selftest_leak(SEXP a, SEXP b, SEXP c) {
    (void)b; (void)c;
    SEXP v = PROTECT(Rf_allocVector(REALSXP, 1)); /* returns with one protect too many when a is TRUE */
    if (!Rf_asLogical(a)) UNPROTECT(1);
    return v;
}

static const R_CallMethodDef selftest_entries[] = {
    {"emul_selftest_error", (DL_FUNC)(generic_fn)&selftest_error, 3},
    {"emul_selftest_use_after", (DL_FUNC)(generic_fn)&selftest_use_after, 3},
    {"emul_selftest_toplevel", (DL_FUNC)(generic_fn)&selftest_toplevel, 3},
    {"emul_selftest_leak", (DL_FUNC)(generic_fn)&selftest_leak, 3},
    {NULL, NULL, 0}};

static const R_CallMethodDef* find_entry(const char* name) {
    for (int t = 0; t < 2; ++t) {
        const R_CallMethodDef* e = t == 0 ? registered : selftest_entries;
        for (; e != NULL && e->name != NULL; ++e)
            if (strcmp(e->name, name) == 0) return e;
    }
    return NULL;
}

typedef SEXP (*fn3)(SEXP, SEXP, SEXP);
typedef SEXP (*fn5)(SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*fn9)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*fn10)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*fn11)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
typedef SEXP (*fn13)(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);

static SEXP dispatch(DL_FUNC entry, int n, SEXP* a) {
    const generic_fn f = (generic_fn)entry;
    switch (n) {
        case 3: return ((fn3)f)(a[0], a[1], a[2]);
        case 5: return ((fn5)f)(a[0], a[1], a[2], a[3], a[4]);
        case 9: return ((fn9)f)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
        case 10: return ((fn10)f)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]);
        case 11: return ((fn11)f)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]);
        case 13: return ((fn13)f)(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12]);
        default: return NULL;
    }
}

/* the only frame the entry's long jumps can reach; kept apart so that no local of emul_call lives across the setjmp */
static int guarded(DL_FUNC f, int nargs, SEXP* args, SEXP* out) __attribute__((noinline));
static int guarded(DL_FUNC f, int nargs, SEXP* args, SEXP* out) {
    const int kind = setjmp(frames[0].jb);
    if (kind == 0) *out = dispatch(f, nargs, args);
    return kind;
}

/* .Call(name, args...): the result, or NULL with emul_last_kind() / emul_last_message().  The per-call bookkeeping
 * (output text, polls, events) starts afresh. */
SEXP emul_call(const char* name, int nargs, SEXP* args) {
    ensure_init();
    out_len = 0;
    if (out_text != NULL) out_text[0] = 0;
    n_polls = 0;
    n_events = 0;
    last_message[0] = 0;
    last_delta = last_delta_at_exit = 0;
    last_value = NULL;
    const R_CallMethodDef* e = find_entry(name);
    if (e == NULL) {
        last_kind = KIND_REFUSED;
        snprintf(last_message, sizeof last_message, "\"%s\" not available for .Call()", name);
        return NULL;
    }
    if (e->numArgs != nargs) {
        last_kind = KIND_REFUSED;
        snprintf(last_message, sizeof last_message, "Incorrect number of arguments (%d), expecting %d for '%s'", nargs, e->numArgs, name);
        return NULL;
    }
    if (nargs != 3 && nargs != 5 && nargs != 9 && nargs != 10 && nargs != 11 && nargs != 13) {
        last_kind = KIND_REFUSED;
        snprintf(last_message, sizeof last_message, "emulator: no trampoline for %d arguments", nargs);
        return NULL;
    }
    if (n_frames != 0) {
        last_kind = KIND_REFUSED;
        snprintf(last_message, sizeof last_message, "emulator: emul_call is not re-entrant");
        return NULL;
    }
    const int depth0 = protect_depth;
    ralloc_block* const vmax0 = ralloc_top;
    call_args = args;
    call_nargs = nargs;
    SEXP result = NULL;
    frames[0].depth = depth0;
    frames[0].vmax = vmax0;
    n_frames = 1;
    const int kind = guarded(e->fun, nargs, args, &result);
    if (kind == 0) {
        last_kind = KIND_OK;
        last_delta_at_exit = protect_depth - depth0;
        if (result == NULL) {
            event("NULL pointer", "returned from the entry");
        } else if (!result->alive) {
            event("use after collection", "returned from the entry");
        }
    } else { /* R unwinds: the protect stack goes back to its depth at entry */
        last_kind = kind;
        last_delta_at_exit = exit_depth - depth0;
        protect_depth = depth0;
        result = NULL;
    }
    n_frames = 0;
    release_ralloc(vmax0);
    last_delta = protect_depth - depth0;
    call_args = NULL;
    call_nargs = 0;
    last_value = result; /* like .Last.value: stays reachable until the next call */
    return result;
}

int emul_last_kind(void) { return last_kind; }
const char* emul_last_message(void) { return last_message; }
int emul_protect_delta(void) { return last_delta; }           /* depth after the call minus depth at entry */
int emul_protect_delta_at_exit(void) { return last_delta_at_exit; } /* ... at the return or at the long jump, before R's reset */
int emul_protect_depth(void) { return protect_depth; }
const char* emul_output(void) { return out_text != NULL ? out_text : ""; }
long emul_polls(void) { return n_polls; }
void emul_arm_interrupt(long from_poll) { interrupt_from_poll = from_poll; } /* 0 disarms */
int emul_event_count(void) { return n_events; }
const char* emul_event(int q) { return q >= 0 && q < n_events && q < MAX_EVENTS ? events[q] : ""; }
void emul_clear_events(void) { n_events = 0; }
long emul_ralloc_blocks(void) {
    long n = 0;
    for (ralloc_block* b = ralloc_top; b != NULL; b = b->next) ++n;
    return n;
}
long emul_object_count(void) { return n_objects; }
long emul_poisoned_count(void) { return n_poisoned; }
DllInfo* emul_dll(void) { return &the_dll; }
int emul_dynamic_symbols(void) { return dynamic_symbols; }

int emul_entry_count(void) {
    int n = 0;
    for (const R_CallMethodDef* e = registered; e != NULL && e->name != NULL; ++e) ++n;
    return n;
}
const char* emul_entry_name(int q) { return q >= 0 && q < emul_entry_count() ? registered[q].name : ""; }
int emul_entry_arity(int q) { return q >= 0 && q < emul_entry_count() ? registered[q].numArgs : -1; }

/* Between tests: drop the protect stack and free every object but the symbols. */
void emul_reset(void) {
    ensure_init();
    protect_depth = 0;
    last_value = NULL;
    n_events = 0;
    interrupt_from_poll = 0;
    release_ralloc(NULL);
    SEXP keep = NULL;
    for (SEXP s = all_objects; s != NULL;) {
        SEXP next = s->next;
        if (s->pinned) {
            s->next = keep;
            keep = s;
        } else {
            free(s->data);
            free(s->class_name);
            free(s);
            --n_objects;
        }
        s = next;
    }
    all_objects = keep;
}

/* ---- building objects (each helper protects what it holds across its own allocations; the caller protects the result) */
SEXP emul_make_real(const double* v, R_xlen_t n) {
    SEXP s = Rf_allocVector(REALSXP, n);
    if (s == R_NilValue) return s;
    if (n > 0) memcpy(s->data, v, (size_t)n * sizeof(double));
    return s;
}

static SEXP make_ints(int type, const int* v, R_xlen_t n) {
    SEXP s = Rf_allocVector((unsigned)type, n);
    if (s == R_NilValue) return s;
    if (n > 0) memcpy(s->data, v, (size_t)n * sizeof(int));
    return s;
}
SEXP emul_make_int(const int* v, R_xlen_t n) { return make_ints(INTSXP, v, n); }
SEXP emul_make_lgl(const int* v, R_xlen_t n) { return make_ints(LGLSXP, v, n); }

static SEXP with_dim(SEXP s, int nrow, int ncol) {
    if (s == R_NilValue) return s;
    PROTECT(s);
    SEXP dim = Rf_allocVector(INTSXP, 2);
    if (dim == R_NilValue) {
        UNPROTECT(1);
        return dim;
    }
    ((int*)dim->data)[0] = nrow;
    ((int*)dim->data)[1] = ncol;
    s->dim = dim;
    UNPROTECT(1);
    return s;
}
/* column-major values, as R keeps a matrix */
SEXP emul_make_real_matrix(const double* v, int nrow, int ncol) { return with_dim(emul_make_real(v, (R_xlen_t)nrow * ncol), nrow, ncol); }
SEXP emul_make_int_matrix(const int* v, int nrow, int ncol) { return with_dim(emul_make_int(v, (R_xlen_t)nrow * ncol), nrow, ncol); }

SEXP emul_make_string(const char* text) {
    SEXP s = PROTECT(Rf_allocVector(STRSXP, 1));
    SET_STRING_ELT(s, 0, Rf_mkChar(text));
    UNPROTECT(1);
    return s;
}

SEXP emul_make_list(R_xlen_t n) { return Rf_allocVector(VECSXP, n); }

SEXP emul_make_s4(const char* class_name) {
    SEXP def = PROTECT(R_do_MAKE_CLASS(class_name));
    SEXP s = R_do_new_object(def);
    UNPROTECT(1);
    return s;
}

void emul_set_slot(SEXP s, const char* name, SEXP value) {
    PROTECT(s);
    PROTECT(value);
    SEXP sym = Rf_install(name);
    R_do_slot_assign(s, sym, value);
    UNPROTECT(2);
}

/* new("dgCMatrix", x =, i =, p =, Dim = c(nrow, ncol)); the three lengths are free so that malformed ones can be made */
SEXP emul_make_dgc(const double* x, R_xlen_t nx, const int* i, R_xlen_t ni, const int* p, R_xlen_t np, int nrow, int ncol) {
    SEXP s = PROTECT(emul_make_s4("dgCMatrix"));
    emul_set_slot(s, "x", emul_make_real(x, nx));
    emul_set_slot(s, "i", emul_make_int(i, ni));
    emul_set_slot(s, "p", emul_make_int(p, np));
    const int dim[2] = {nrow, ncol};
    emul_set_slot(s, "Dim", emul_make_int(dim, 2));
    UNPROTECT(1);
    return s;
}

/* ---- reading objects (no allocation, no error: a collected object reads as what is left of it) ---------------------- */
int emul_type(SEXP s) { return s != NULL ? s->type : -1; }
long long emul_length(SEXP s) { return s != NULL ? (long long)s->length : -1; }
int emul_alive(SEXP s) { return s != NULL && s->alive; }
void* emul_data(SEXP s) { return s != NULL ? s->data : NULL; }
const char* emul_class(SEXP s) { return s != NULL && s->class_name != NULL ? s->class_name : ""; }
int emul_dim(SEXP s, int* out, int cap) {
    if (s == NULL || s->dim == NULL) return 0;
    for (int q = 0; q < cap && q < (int)s->dim->length; ++q) out[q] = ((int*)s->dim->data)[q];
    return (int)s->dim->length;
}
int emul_names_count(SEXP s) { return s != NULL && s->names != NULL ? (int)s->names->length : 0; }
const char* emul_name(SEXP s, int q) {
    if (s == NULL || s->names == NULL || q < 0 || q >= s->names->length) return "";
    SEXP c = ((SEXP*)s->names->data)[q];
    return c != NULL && c->type == CHARSXP ? (const char*)c->data : "";
}
SEXP emul_element(SEXP s, long long q) {
    if (s == NULL || (s->type != VECSXP && s->type != STRSXP) || q < 0 || q >= s->length) return NULL;
    return ((SEXP*)s->data)[q];
}
SEXP emul_slot(SEXP s, const char* name) {
    if (s == NULL) return NULL;
    for (int q = 0; q < s->nslots; ++q)
        if (strcmp((const char*)s->slot_name[q]->data, name) == 0) return s->slot_value[q];
    return NULL;
}
int emul_slot_count(SEXP s) { return s != NULL ? s->nslots : 0; }
const char* emul_chars(SEXP s) { return s != NULL && (s->type == CHARSXP || s->type == SYMSXP) ? (const char*)s->data : ""; }
