// go1_step_shared.h -- the scaffold the trajectory step (go1_step.hip) and the velocity step (go1_velocity.hip)
// have in common: the root state I/O, the decimation loop (actuator net -> phys_substep), the contact-force
// outputs, the divergence guard, the Philox staging and the wave-level row allocation; then, under the host
// banner, the plane-table check of the two bind functions, HIP_TRY and the event-pair launch.
// Include after go1_device.h.  The arithmetic here (actuator-net inputs, torque clamp) is pinned bit for bit to
// the oracles: it is compiled with FP contraction OFF (a contracted a * b + c would change bits).  Where the two
// kernels differ, the difference arrives as an argument or a template parameter.  The per-joint prologue loads
// and epilogue write-back stay written out in each kernel (as helpers they cost registers).
#pragma once
#include "go1_device.h"

#pragma clang fp contract(off)

// =====================================================================
//                               device
// =====================================================================
// The per-joint registers of a lane (the three joints of its leg), as a view of the kernel's own arrays: one
// struct holding the arrays themselves stays in memory as a whole (scratch, 196 B/lane in the specialised
// trajectory kernel) where separate arrays are promoted to registers.  KMAX: stored lag entries kept.
template <int KMAX>
struct Joints {
  float (&act)[3], (&q)[3], (&qd)[3], (&eh)[2][3], (&vh)[2][3], (&strength)[3], (&offset)[3];
  float (&dflt)[3], (&tlim)[3], (&lag_pre)[KMAX][3];
  float (&scaled)[3], (&torque)[3], (&tgt)[3];
};

// root state row (pos, quat, lin vel, ang vel) <-> the integrator's base state
__device__ __forceinline__ void phys_load_root(Phys& P, const float* root) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    P.pos[i] = root[i];
    P.wv[i] = f2{root[10 + i], root[7 + i]};
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) P.quat[i] = root[3 + i];
}
__device__ __forceinline__ void phys_store_root(const Phys& P, float* root) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    root[i] = P.pos[i]; root[7 + i] = P.wv[i].y; root[10 + i] = P.wv[i].x;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) root[3 + i] = P.quat[i];
}

// ---------------- decimation loop (trajectory :82-88, velocity :76-82)
// The lag ring is pushed once per sim sub-step with the same scaled action
// (:973), so sub-step s reads the slot s+1 of the incoming ring and the ring
// leaves the step as [old4, old5, old6, scaled x 4].
// INJ replays the recorded joint state (A.inj_dof) instead of integrating.  s_mlp: the parked actuator-net
// fragments; s_phys / T / s_self: phys_substep's LDS model block (or nullptr), terrain and the env's
// self-collision scratch; cf_raw: the last sub-step's per-lane contact forces (cf_sum).  action_scale and
// hip_scale_reduction by value: the specialised trajectory kernel passes its compile-time constants.  leg and
// role are the caller's own values: derived here again from lane they were a second live copy (+8 AGPRs).
// dec, n_int: go1_config.decimation and n_internal by value.  FIXED: they are compile-time constants (the
// specialised trajectory kernel; both loops stay rolled); otherwise they are read here once and pinned in SGPRs.
// What a sim step's common path reads from the config right before using it (the step length, the contact and
// self-collision constants: sub_consts) is read once, in front of the loop: through the constant address space the
// compiler re-loads an invariant field at each use rather than keep it, a scalar-cache round trip with a wait per
// sim step that a single wave per SIMD cannot hide.
template <bool INJ, bool FIXED, int KMAX, class Args>
__device__ __forceinline__ void step_substeps(CCfg* c, const Args& A, const Joints<KMAX>& J, Phys& P,
                                              const float* s_mlp, const float* s_phys, const Terr& T, float* s_self,
                                              float* cf_raw, int KL, float friction, float restitution,
                                              float payload, int e, int lane, float action_scale,
                                              float hip_scale_reduction, int leg, int role, int dec, int n_int) {
  const int lq = lane >> 4, n = c->n_envs;
  if (!FIXED) { pin_s(dec); pin_s(n_int); }
  float h = c->sim_dt / (float)n_int;  // the integrator's step
  pin_s(h);
  const PhysK PK = sub_consts(c);
  Held H = {f2{0.0f, 0.0f}, {-1, -1}};  // set by the control step's first sim step (phys_substep)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    J.scaled[j] = J.act[j] * action_scale;
    if (j == 0) J.scaled[j] = J.scaled[j] * hip_scale_reduction;
  }
#pragma unroll 1
  for (int sub = 0; sub < dec; ++sub) {
    MARK(sub_begin);
    // _compute_torques (:957-996)
    {
#ifndef GO1_ABL_NO_MLP
      // the parked fragments' reads first: they land under the input preparation below
      MlpFrag Fs;
      mlp_unpark(Fs, s_mlp, lane);
#endif
      // inputs of this lane's three joints ...
      // the ring's oldest slot after this sub-step's push (:973-974) is old slot sub + 1, i.e. the
      // scaled action of `back` steps ago (stored entry KL - back), or this step's for back = 0
      const int m = 6 - sub;
      const int back = m <= 0 ? 0 : (m + dec - 1) / dec;  // wave-uniform: scalar selects below
      float xin[3][6];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        float lg = J.scaled[j];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) lg = back == KL - k ? J.lag_pre[k][j] : lg;
        J.tgt[j] = lg + J.dflt[j];
        const float err = J.q[j] - J.tgt[j] + J.offset[j];
        xin[j][0] = err; xin[j][1] = J.eh[0][j]; xin[j][2] = J.eh[1][j];
        xin[j][3] = J.qd[j]; xin[j][4] = J.vh[0][j]; xin[j][5] = J.vh[1][j];
      }
      // ... -> 3 MFMA groups per wave: group j holds joint j of the 16 (env, leg) items
      // of the wave in column 4 env + leg; row (= role) q supplies inputs q and 4 + q of
      // its own leg and receives the item's torque in place.
      MARK(mlp_begin);
      float tq[3] = {0.0f, 0.0f, 0.0f};
      float b0[3], b1v[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float* y = xin[j];
        b0[j] = sel4(lq, y[0], y[1], y[2], y[3]);
        b1v[j] = sel4(lq, y[4], y[5], 0.0f, 0.0f);
      }
#ifdef GO1_ABL_NO_MLP
#pragma unroll
      for (int j = 0; j < 3; ++j) tq[j] = 0.0f * (b0[j] + b1v[j]);  // ablation build only: no actuator net
#else
      mlp_group3(Fs, b0, b1v, tq);
#endif
#ifdef GO1_ABL_NO_MLP
#pragma unroll
      for (int j = 0; j < 3; ++j) tq[j] += -20.0f * xin[j][0] - 0.5f * xin[j][3];  // PD stand-in
#endif
      MARK(mlp_done);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        J.eh[1][j] = J.eh[0][j];
        J.eh[0][j] = xin[j][0];
        J.vh[1][j] = J.vh[0][j];
        J.vh[0][j] = J.qd[j];
        const float t = tq[j] * J.strength[j];
        const float lim = J.tlim[j];
        J.torque[j] = clampf(t, -lim, lim);
      }
    }
    if (INJ) {
      const float* id = A.inj_dof + ((size_t)sub * n + e) * NDOF * 2;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        J.q[j] = id[(leg * 3 + j) * 2];
        J.qd[j] = id[(leg * 3 + j) * 2 + 1];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) { P.q[j] = J.q[j]; P.qd[j] = J.qd[j]; }
      MARK(phys_call);
#ifndef GO1_ABL_NO_PHYS
#pragma unroll 1
      for (int k = 0; k < n_int; ++k) {
        const bool last = (sub == dec - 1) && (k == n_int - 1);
        phys_substep(c, PK, H, s_phys, P, J.torque, h, A.sim_gravity, friction, restitution, payload, T, leg, role,
                     last, cf_raw, s_self, sub == 0 && k == 0);
      }
#else
      P.qd[0] += 1e-4f * J.torque[0]; P.qd[1] += 1e-4f * J.torque[1]; P.qd[2] += 1e-4f * J.torque[2];
#endif
#pragma unroll
      for (int j = 0; j < 3; ++j) { J.q[j] = P.q[j]; J.qd[j] = P.qd[j]; }
      MARK(phys_returned);
    }
    if (A.dbg_torques && role == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) A.dbg_torques[((size_t)sub * n + e) * NDOF + leg * 3 + j] = J.torque[j];
    }
  }
}

// The step's reported contact forces: the last sub-step's (cf_sum), or in INJ mode the recorded ones
// (inj_contact: (n_envs, NB, 3), body order base, then hip / thigh / calf / foot per leg).
template <bool INJ>
__device__ __forceinline__ void contact_totals(const float* cf_raw, const float* inj_contact, int e,
                                               int leg, int role, float* cf_leg, float* cf_base, float* cf_hip) {
  cf_sum(cf_raw, role, cf_leg, cf_base, cf_hip);
  if (INJ) {
    const float* ic = inj_contact + (size_t)e * NB * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      cf_base[i] = ic[i];
      cf_hip[i] = ic[(1 + leg * 4) * 3 + i];
    }
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int i = 0; i < 3; ++i) cf_leg[b * 3 + i] = ic[(2 + leg * 4 + b) * 3 + i];
  }
}
// the optional contact_forces output (n_envs, NB, 3), stored by the leg's owner lane (role 0)
__device__ __forceinline__ void contact_store(float* out, int e, int leg, const float* cf_leg,
                                              const float* cf_base, const float* cf_hip) {
  float* o = out + (size_t)e * NB * 3;
  if (leg == 0) { o[0] = cf_base[0]; o[1] = cf_base[1]; o[2] = cf_base[2]; }
  float* ol = o + (1 + leg * 4) * 3;
  ol[0] = cf_hip[0]; ol[1] = cf_hip[1]; ol[2] = cf_hip[2];
#pragma unroll
  for (int i = 0; i < 9; ++i) ol[3 + i] = cf_leg[i];
}

// native-integrator divergence guard (no reference counterpart: PhysX does not
// return non-finite states): an env whose state is not finite, or beyond
// GO1_DIVERGED in any component, is reset, and nothing of its diverged state reaches
// an output (zero reward, post-reset observations).  True on every lane of such an env.
__device__ __forceinline__ bool state_diverged(const float* root, const float* q, const float* qd) {
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 13; ++i) finite = finite & (fabsf(root[i]) < GO1_DIVERGED);
#pragma unroll
  for (int j = 0; j < 3; ++j) finite = finite & (fabsf(q[j]) < GO1_DIVERGED) & (fabsf(qd[j]) < GO1_DIVERGED);
  return qsum(finite ? 0.0f : 1.0f) != 0.0f;
}

// Philox blocks first .. first + n_blocks - 1 of the env into dst[0 .. 4 n_blocks): lane sub16 < n_blocks of
// the env draws block first + sub16 (one evaluation per lane instead of one per draw) and the env's lanes
// read their slots back from LDS (one wave per block: its LDS operations complete in order)
__device__ __forceinline__ void rng_stage(const Rng& rng, int first, int n_blocks, int sub16, float* dst) {
  if (sub16 < n_blocks) {
    float uq[4];
    rng.quad(first + sub16, uq);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[4 * sub16 + k] = uq[k];
  }
}

// Rows of an append-only table for the wave's lanes with `want` (at most one per env: its lane `pos`), at one
// atomic per wave: the row of the env whose wanting lane is `pos` (valid where that env wants one), or -1
// when no lane of the wave wants a row.
__device__ __forceinline__ int wave_alloc_row(bool want, int32_t* count, int lane, int pos) {
  const uint64_t m = __ballot(want);
  if (m == 0ull) return -1;
  int base = 0;
  if (lane == 0) base = atomicAdd(count, __popcll(m));
  base = __shfl(base, 0);
  return base + __popcll(m & ((1ull << pos) - 1ull));
}

// the per-joint planes after an explicit reset (the reset kernels: one lane per leg stores its three joints)
template <class State>
__device__ __forceinline__ void joints_store_reset(const State& st, int e, int leg, int KL, const float* q,
                                                   const float* qd, const float* strength, const float* offset) {
  const size_t d0 = (size_t)e * NDOF + leg * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    st.dof_pos[d0 + j] = q[j];
    st.dof_vel[d0 + j] = qd[j];
    st.motor_strength[d0 + j] = strength[j];
    st.motor_offset[d0 + j] = offset[j];
    st.last_actions[d0 + j] = 0.0f;
    st.last_dof_vel[d0 + j] = 0.0f;
    for (int k = 0; k < KL; ++k) st.lag[(size_t)e * 12 * KL + k * 12 + leg * 3 + j] = 0.0f;
  }
}

// =====================================================================
//                                host
// =====================================================================
// One row per state plane, in state-struct order (go1_bind / go1_vel_bind check the caller's descriptors
// against it).  cols 0: config-dependent, filled in by the caller; rows 0: n_envs.
struct PlaneRow {
  const char* name;
  size_t ptr_off;  // offset of the plane's pointer in the state struct
  int64_t cols;
  int dtype;
  int64_t rows;
};
#define GO1_PLANE(S, f, cols, dtype) {#f, offsetof(S, f), cols, dtype, 0}
#define GO1_PLANE_INDEX(S, f) (offsetof(S, f) / sizeof(void*))  // the state structs hold one pointer per plane

// `fail(code, message)`: the library's own error sink (the two libraries keep separate last-error strings)
static const char* const DTYPE_NAME[] = {"float32", "int32", "float64"};  // by GO1_DTYPE_*
template <size_t N, class Fail>
static int check_planes(const char* fn, const void* state, const PlaneRow (&table)[N], const go1_plane* planes,
                        int64_t n_envs, Fail fail) {
  for (size_t i = 0; i < N; ++i) {
    const PlaneRow& r = table[i];
    const go1_plane& d = planes[i];
    const int64_t rows = r.rows ? r.rows : n_envs;
    const std::string who = std::string(fn) + ": state plane " + r.name;
    const void* p;
    memcpy(&p, (const char*)state + r.ptr_off, sizeof(p));
    if (!p) return fail(GO1_E_ARG, who + " is null");
    if (d.rows != rows || d.cols != r.cols || d.dtype != r.dtype)
      return fail(GO1_E_ARG, who + " must be (" + std::to_string(rows) + ", " + std::to_string(r.cols) + ") " +
                                 DTYPE_NAME[r.dtype]);
    if (d.col_stride != 1 || (d.rows > 1 && d.row_stride != d.cols))
      return fail(GO1_E_ARG, who + " is not dense row-major (strides " + std::to_string(d.row_stride) + ", " +
                                 std::to_string(d.col_stride) + "): pass a contiguous tensor");
  }
  return GO1_OK;
}

#define GO1_HIP_TRY(fail, x)                                                            \
  do {                                                                                  \
    hipError_t _e = (x);                                                                \
    if (_e != hipSuccess) return fail(GO1_E_HIP, std::string(#x ": ") + hipGetErrorString(_e)); \
  } while (0)

// Launch with an optional event pair attached to the kernel's own dispatch (hipExtLaunchKernelGGL: the
// events take the dispatch packet's start / end timestamps, as a profiler's kernel trace does),
// so ev_end - ev_begin is the kernel's duration without the queue work of separate event records.
template <class Kern, class... Args>
static void launch_timed(Kern kern, dim3 grid, dim3 block, hipStream_t s, void* ev_begin, void* ev_end, Args... args) {
  hipEvent_t e0 = (hipEvent_t)ev_begin, e1 = (hipEvent_t)ev_end;
  if (e0 || e1) hipExtLaunchKernelGGL(kern, grid, block, 0, s, e0, e1, 0, args...);
  else hipLaunchKernelGGL(kern, grid, block, 0, s, args...);
}
