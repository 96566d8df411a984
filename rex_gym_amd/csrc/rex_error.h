// rex_error.h -- error reporting of the host units (rexsim.hip, rex_learner.hip): fail / failf set the calling thread's message, which
// rex_last_error() returns, and hand back the code; HIPCHK returns REX_EHIP from the enclosing function.  Defined once, in rexsim.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/rexsim.h"

int fail(int code, const char* fmt, const char* detail);
int failf(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) return fail(REX_EHIP, #expr ": %s", hipGetErrorString(_e)); \
  } while (0)
