// go1_priv.hip -- the privileged-observation assembler of include/go1_priv.h: one launch per env step, after the step
// kernel and the add-ons that change what it reads.
//
// One lane per output element (env, column), row-major, 256-lane workgroups: a wave stores 64 consecutive floats, and
// the lanes that read one env's row of a plane (12 motor strengths, 3 velocities) read consecutive floats too.  The
// column table is constant for an env's life and lives in device memory (args.table, uploaded once by the caller).
// Lane c < width of every workgroup resolves column c into an LDS record -- the plane's base pointer already offset by
// the component, its stride, or the constant the column holds for every env (zero, a gravity component) -- so that
// the element pass indexes LDS only: a per-lane index into the by-value kernel arguments would put them in scratch.
// The subtraction and the multiply are two f32 operations (contraction off), the division is the correctly rounded
// one (hipcc's default for `/`), the clip is the step kernels' clampf expression.
//
// This file includes neither csrc/go1_host.h nor any other file of the package besides its own header: two existing
// tests (test_render_abi.py, test_trace_abi.py) list the four libraries that may share go1_host.h with the ray caster
// and the tracer, so the message buffer, fail() and the launch check are restated below.  To fold back into go1_host.h
// once those lists name this library.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/go1_priv.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
static_assert(GO1_PRIV_MAX_COLS <= THREADS, "one staging lane per column");

thread_local char g_err[256] = "";

__attribute__((format(printf, 1, 2))) int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return -1;
}

int launched(const char* fn) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail("%s: launch failed: %s", fn, hipGetErrorString(e));
}

struct Params {
  go1_priv_args a;
  int32_t width;
  uint32_t total;  // n_envs * width
  float clip;
};

// column c as the element pass reads it: x = base ? base[e * stride] : val
struct Rec {
  const float* base;
  int32_t stride;
  float val;
  float shift;
  float scale;
  int32_t op;
  int32_t pad;
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(THREADS) void go1_priv_step_kernel(const Params p) {
  __shared__ Rec s_rec[GO1_PRIV_MAX_COLS];
  const go1_priv_args& a = p.a;
  if ((int)threadIdx.x < p.width) {
    const go1_priv_col t = a.table[threadIdx.x];
    Rec r;
    r.base = nullptr;
    r.stride = 0;
    r.val = 0.0f;
    switch (t.src) {  // fields named one by one: uniform kernel-argument loads
      case GO1_PRIV_SRC_FRICTION: r.base = a.friction; r.stride = a.friction_stride; break;
      case GO1_PRIV_SRC_RESTITUTION: r.base = a.restitution; r.stride = a.restitution_stride; break;
      case GO1_PRIV_SRC_PAYLOADS: r.base = a.payloads; r.stride = a.payloads_stride; break;
      case GO1_PRIV_SRC_MOTOR_STRENGTH: r.base = a.motor_strength; r.stride = a.motor_strength_stride; break;
      case GO1_PRIV_SRC_MOTOR_OFFSET: r.base = a.motor_offset; r.stride = a.motor_offset_stride; break;
      case GO1_PRIV_SRC_ROOT: r.base = a.root; r.stride = a.root_stride; break;
      case GO1_PRIV_SRC_AUX: r.base = a.aux; r.stride = a.aux_stride; break;
      case GO1_PRIV_SRC_GRAVITY:
        r.val = t.comp == 0 ? a.gravities[0] : (t.comp == 1 ? a.gravities[1] : a.gravities[2]);
        break;
      default: break;  // GO1_PRIV_SRC_ZERO
    }
    if (r.base) r.base += t.comp;
    r.shift = t.shift;
    r.scale = t.scale;
    r.op = t.op;
    r.pad = 0;
    s_rec[threadIdx.x] = r;
  }
  __syncthreads();
  const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= p.total) return;
  const uint32_t w = (uint32_t)p.width;
  const uint32_t e = i / w, c = i - e * w;
  const Rec r = s_rec[c];
  const float x = r.base ? r.base[(size_t)e * (size_t)r.stride] : r.val;
  float y = x;
  if (r.op == GO1_PRIV_OP_MUL) y = (x - r.shift) * r.scale;
  else if (r.op == GO1_PRIV_OP_DIV) y = (x - r.shift) / r.scale;
  a.out[i] = clampf(y, -p.clip, p.clip);
}

const char* const SRC_NAMES[GO1_PRIV_NUM_SRC] = {"zero", "friction", "restitution", "payloads", "motor_strength",
                                                 "motor_offset", "root", "aux", "gravities"};

}  // namespace

extern "C" {

int go1_priv_abi_version(void) { return GO1_PRIV_ABI_VERSION; }

void go1_priv_abi_sizes(int64_t out[4]) {
  out[0] = sizeof(go1_priv_col);
  out[1] = sizeof(go1_priv_config);
  out[2] = sizeof(go1_priv_args);
  out[3] = GO1_PRIV_MAX_COLS;
}

const char* go1_priv_last_error(void) { return g_err; }

int go1_priv_step(const go1_priv_config* c, const go1_priv_args* a, void* stream) {
  const char* fn = "go1_priv_step";
  if (!c || !a) return fail("%s: null cfg or args", fn);
  if (c->n_envs < 0) return fail("%s: n_envs must be >= 0", fn);
  if (c->width < 1 || c->width > GO1_PRIV_MAX_COLS)
    return fail("%s: width must be 1 .. %d (GO1_PRIV_MAX_COLS), got %d", fn, GO1_PRIV_MAX_COLS, c->width);
  if ((int64_t)c->n_envs * c->width > INT32_MAX)
    return fail("%s: n_envs * width = %lld is beyond 2^31 - 1", fn, (long long)c->n_envs * c->width);
  if (!(c->clip_obs >= 0.0f)) return fail("%s: clip_obs must be >= 0", fn);
  const float* planes[GO1_PRIV_NUM_SRC] = {nullptr,           a->friction,     a->restitution, a->payloads,
                                           a->motor_strength, a->motor_offset, a->root,        a->aux,
                                           nullptr};
  const int32_t strides[GO1_PRIV_NUM_SRC] = {0,
                                             a->friction_stride,
                                             a->restitution_stride,
                                             a->payloads_stride,
                                             a->motor_strength_stride,
                                             a->motor_offset_stride,
                                             a->root_stride,
                                             a->aux_stride,
                                             3};
  for (int k = 0; k < c->width; ++k) {
    const go1_priv_col& t = c->cols[k];
    if (t.src < 0 || t.src >= GO1_PRIV_NUM_SRC) return fail("%s: column %d: unknown source %d", fn, k, t.src);
    if (t.op != GO1_PRIV_OP_MUL && t.op != GO1_PRIV_OP_DIV && t.op != GO1_PRIV_OP_RAW)
      return fail("%s: column %d: unknown operation %d", fn, k, t.op);
    if (t.op == GO1_PRIV_OP_DIV && t.scale == 0.0f) return fail("%s: column %d divides by a zero scale", fn, k);
    if (t.src == GO1_PRIV_SRC_ZERO) continue;
    if (t.src != GO1_PRIV_SRC_GRAVITY && !planes[t.src])
      return fail("%s: column %d reads the %s plane, which is NULL", fn, k, SRC_NAMES[t.src]);
    if (t.comp < 0 || t.comp >= strides[t.src])
      return fail("%s: column %d: component %d is outside a %s row of %d", fn, k, t.comp, SRC_NAMES[t.src],
                  strides[t.src]);
  }
  if (!a->table || !a->out) return fail("%s: args: table and out must be set", fn);
  if (c->n_envs == 0) return 0;
  Params p;
  p.a = *a;
  p.width = c->width;
  p.total = (uint32_t)c->n_envs * (uint32_t)c->width;
  p.clip = c->clip_obs;
  const unsigned blocks = (p.total + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(go1_priv_step_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, p);
  return launched(fn);
}

}  // extern "C"
