// pmx_error.cpp - the thread-local error message behind pmx_last_error(), and pmx_version(). Host only.
#include "pmx_error.h"

#include <cstdarg>
#include <cstdio>

static thread_local char g_err[512] = "";

int pmx_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *pmx_last_error(void) { return g_err; }
extern "C" int pmx_version(void) { return 101; }
