// go1_host.h -- the host side the after-step add-on libraries share (go1_render.hip, go1_trace.hip, go1_plan.hip,
// go1_dr.hip): the calling thread's last error message and the check behind a kernel launch.  Internal linkage only;
// each library exports its own <prefix>_last_error with GO1_LAST_ERROR.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

namespace {

thread_local char g_err[256] = "";

// -1, with the formatted message left for <prefix>_last_error: `return fail("go1_x: n must be >= %d", 1);`
__attribute__((format(printf, 1, 2))) int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return -1;
}

// behind a launch by exported function `fn`: 0, or -1 with HIP's text
int launched(const char* fn) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s: launch failed: %s", fn, hipGetErrorString(e));
}

}  // namespace

#define GO1_LAST_ERROR(prefix) \
  const char* prefix##_last_error(void) { return g_err; }
