// go1_device.h -- device code shared by the MI355X Go1 step kernels (go1_step.hip: trajectory tracking;
// go1_velocity.hip: velocity tracking).  The one header the sources include: the ABI, the MARK instrumentation, the
// launch constants, then the parts in dependency order.  Each part sets its own FP contraction: off where the
// arithmetic is pinned bit for bit to the oracle, on for the integrator (compared with the f64 oracle within a
// tolerance).  Included by one translation unit per library.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <string>
#include <type_traits>

#include "../../include/go1_mi355x.h"
#include "go1_model_consts.h"
#include "go1_spec.h"
static_assert(GO1_MODEL_CONST_FLOATS == GO1_MODEL_FLOATS, "regenerate go1_model_consts.h");
#include "pmath.h"

// The config block through the constant address space: every uniform field read is a
// scalar (SMEM) load.  Through a generic pointer the compiler cannot prove that the
// kernel's stores leave the block unchanged, and emits vector loads, each a full memory
// round trip at its first use (inside the sub-step loop too).
typedef const __attribute__((address_space(4))) go1_config CCfg;

#define GO1_DEVICE_H  // the parts refuse to be included on their own

#ifdef GO1_ISA_MARKS  // section markers for static instruction accounting (tools/isa_sections.py)
#define MARK(x) asm volatile("; MARK " #x)
#elif defined(GO1_STAMPS)
// Diagnostic build only (tools/stamps.py): every marker records (source line, s_memtime)
// into a buffer of its own, read back by go1_debug_stamps.  Never built into the product.
#define GO1_STAMP_WAVES 4096
#define GO1_STAMP_SLOTS 320
__device__ unsigned long long g_go1_stamps[GO1_STAMP_WAVES * GO1_STAMP_SLOTS];
__shared__ unsigned s_go1_stamp_k;
__device__ __forceinline__ void go1_stamp(unsigned line) {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  const unsigned i = s_go1_stamp_k;
  if (blockIdx.x < GO1_STAMP_WAVES && i < GO1_STAMP_SLOTS)
    g_go1_stamps[blockIdx.x * GO1_STAMP_SLOTS + i] = ((unsigned long long)line << 48) | (t & 0xffffffffffffull);
  s_go1_stamp_k = i + 1;
  __builtin_amdgcn_sched_barrier(0);
}
#define MARK(x) go1_stamp(__LINE__)
#else
#define MARK(x)
#endif
#define NDOF 12
#define NB 17
#define EPB 16          // envs per block of the reset kernel (4 lanes per env)
#define TPB 64          // one wave per block
#define SEPB 4          // envs per wave of the step kernel (16 lanes per env: 4 roles x 4 legs)
#define GO1_DIVERGED 1.0e4f  // |state component| treated as a diverged integrator
#define PI_F 3.14159265358979323846f
#define TWO_PI_F 6.28318548202514648438f  // (float)(2*pi), torch's f32 scalar

#include "go1_lanes.h"       // Philox, selects, cross-lane sums
#include "go1_actuator.h"    // actuator-net MFMA groups
#include "go1_torch_math.h"  // torch-order f32 math
#include "go1_spatial.h"     // spatial algebra (contraction on from here)
#include "go1_contact.h"     // terrain and capsule contact queries
#include "go1_selfcol.h"     // self-collision
#include "go1_phys.h"        // LDS layout, Phys, phys_substep, cf_sum

#pragma clang fp contract(off)  // what follows (go1_step_shared.h, the kernels) is pinned bit for bit to the oracle
