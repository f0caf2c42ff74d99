// pmx_error.h - the one error path of libpmx.so and libpmx_pack.so (host only): a function that fails sets the calling thread's message
// and returns its status code; pmx_last_error() hands the message out. pmx_error.cpp is compiled into both libraries.
#pragma once
#include "pmx.h"

// Formats the thread's error message (printf style, cut at 511 characters) and returns `code`.
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
int pmx_fail(int code, const char *fmt, ...);
