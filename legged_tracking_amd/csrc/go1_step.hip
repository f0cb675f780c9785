// go1_step.hip -- MI355X (gfx950) fused Go1 trajectory-tracking step + C ABI.
//
// One launch = one LeggedRobot.step() for every env
// (go1_gym/envs/base/legged_robot_trajectory_tracking.py:64-169):
//   4 x [actuator-net torques (:957-996, :1311-1320) -> native articulated-body
//        integrator (replaces gym.simulate / fetch_results / refresh, :82-88)]
//   -> post-physics: kinematics (:130-136), height scan (:1918-1970), target and
//      command logic (:774-932), terminations (:198-216), reward terms of both containers
//      (:320-355), reset_idx (:218-296), observations (:357-475), epilogue (:148-153).
//
// Decomposition: 16 lanes per env = 4 legs x 4 roles, lane = 16 role + 4 env + leg; a 64-lane
// wave carries 4 envs and a block is one wave (4096 envs -> 1024 waves, one per SIMD).  The four
// roles of a leg run that leg's kinematics and articulated-body passes redundantly (the 3-link
// chain is sequential) and split the parallel work: the leg's contact points, the actuator-net
// MFMA columns (a role is one row of the 16 x 4 B operand), the height-scan gathers and the
// stores.  Leg sums use DPP quad_perm, role sums v_permlane16/32_swap; both are butterflies, so
// every lane of an env holds bit-identical base quantities and solves the base 6 x 6 system.
// State is SoA row-major (n_envs, width) in HBM.  LDS holds the Go1 model block and per-joint
// config (ds_write after the prologue loads), the env's 20 x 16 (floor, ceiling) terrain patch
// (LDS-DMA, global_load_lds, at step start) and the per-env reward-term table.  See DESIGN.md 5.
// Numerics: the post-physics section is compiled with FP contraction OFF and
// uses the deterministic transcendentals of pmath.h, so it is bit-identical to
// the CPU oracle (oracle/go1_oracle.c) given the same physical state; the
// integrator uses FMA contraction and native sin/cos (f32, compared with the
// oracle's f64 integrator within a tolerance).
// This file is the host side (the handle, the plane table, the C ABI); the kernels are in its parts
// go1_traj_step.h and go1_traj_aux.h, on the device layer of go1_device.h.
#include "go1_device.h"
#include "go1_step_shared.h"

#define GO1_STEP_HIP  // the parts refuse to be included on their own
#include "go1_traj_step.h"  // HOLD_N, KArgs, traj_waypoint, reset_env, write_trajectory, CI, go1_step_kernel
#include "go1_traj_aux.h"   // the finalize, reset, bucket and actuator kernels

// =====================================================================
//                                C ABI
// =====================================================================
struct go1_handle {
  go1_config cfg;
  go1_config* d_cfg = nullptr;
  go1_state st;
  go1_terrain ter;
  bool bound = false, has_terrain = false;
  int32_t* d_flags = nullptr;  // 3 "some env reset in step k" words (k mod 3)
  float* d_bucket_r = nullptr;    // global reward bucketing scratch (indefinite_slots != 0)
  double* d_bucket_sum = nullptr; // 2 banks x GO1_MAX_TERMS
  uint64_t count = 0;          // go1_step calls so far
  bool spec = false;           // every GO1_SPEC_FIELDS value matches: the specialised kernel runs
  bool streamed = false;       // the streamed height scan runs (any grid but 21 x 11, or go1_scan_mode)
  const uint8_t* prev_time_out = nullptr;
  uint8_t* prev_extras = nullptr;
};

static thread_local std::string g_err;

#define P(f, cols, dt) GO1_PLANE(go1_state, f, cols, GO1_DTYPE_##dt)
static const PlaneRow STATE_PLANES[] = {
    P(root, 13, F32), P(dof_pos, 12, F32), P(dof_vel, 12, F32), P(last_actions, 12, F32), P(last_dof_vel, 12, F32),
    P(lag, 0, F32), P(pos_err_hist, 24, F32), P(vel_hist, 24, F32), P(motor_strength, 12, F32),
    P(motor_offset, 12, F32), P(friction, 1, F32), P(restitution, 1, F32), P(payload, 1, F32),
    P(episode_length, 1, I32), P(curr_pose_index, 1, I32), P(trajectory, 0, F32), P(base_rotation, 3, F32),
    P(collision_count, 1, I32), P(episode_sums, 0, F32), P(joint_pos_target, 12, F32), P(feet_air_time, 4, F32),
    P(last_contacts, 4, F32)};
#undef P
static_assert(sizeof(STATE_PLANES) / sizeof(STATE_PLANES[0]) == GO1_STATE_PLANES &&
                  sizeof(go1_state) == GO1_STATE_PLANES * sizeof(void*), "go1_state planes");

// the specialised kernel's values must match bit for bit (-0.0 and 0.0 are different constants)
template <class T>
static bool spec_eq(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }
static bool spec_match(const go1_config& c) {
  bool m = true;
#define GO1_SPEC_CHECK(f, v) m = m && spec_eq(c.f, (decltype(c.f))(v));
  GO1_SPEC_FIELDS(GO1_SPEC_CHECK)
#undef GO1_SPEC_CHECK
  // the specialised kernel keeps GO1_LAG_STEPS(4) = 2 stored lag entries in registers
  static_assert(GO1_LAG_STEPS(GO1_SPEC_decimation) == 2, "go1_step_kernel<SPEC>: KMAX = KL = 2");
  return m;
}
// the scan counts with kernels that keep the scan in registers (KPTS 7 / 15); any other grid is streamed
static bool scan_compiled_in(const go1_config& c) { return c.scan_nx == GO1_GRID_X && c.scan_ny == GO1_GRID_Y; }

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(x) GO1_HIP_TRY(fail, x)
// the library's other translation units (go1_terrain.hip) report through the same message
int go1_internal_fail(int code, const std::string& msg) { return fail(code, msg); }

// go1_create's device allocations and their first contents.  On an error the handle keeps what was allocated
// so far: the caller releases it through go1_destroy.
static int create_device(go1_handle* h, const go1_config* cfg) {
  if (hipMalloc(&h->d_cfg, sizeof(go1_config)) != hipSuccess || hipMalloc(&h->d_flags, 3 * sizeof(int32_t)) != hipSuccess)
    return fail(GO1_E_HIP, "go1_create: hipMalloc failed");
  HIP_TRY(hipMemcpy(h->d_cfg, cfg, sizeof(go1_config), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(h->d_flags, 0, 3 * sizeof(int32_t)));
  if (cfg->indefinite_slots) {
    HIP_TRY(hipMalloc(&h->d_bucket_r, (size_t)cfg->n_envs * GO1_MAX_TERMS * sizeof(float)));
    HIP_TRY(hipMalloc(&h->d_bucket_sum, 2 * GO1_MAX_TERMS * sizeof(double)));
    HIP_TRY(hipMemset(h->d_bucket_r, 0, (size_t)cfg->n_envs * GO1_MAX_TERMS * sizeof(float)));
    HIP_TRY(hipMemset(h->d_bucket_sum, 0, 2 * GO1_MAX_TERMS * sizeof(double)));
  }
  return GO1_OK;
}

extern "C" {
#ifdef GO1_STAMPS
int go1_debug_stamps(void* host, size_t bytes) {
  if (bytes > sizeof(g_go1_stamps)) bytes = sizeof(g_go1_stamps);
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_go1_stamps), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
// zero the stamp buffer (before the launch to be read: a wave records only as many slots as it executes
// markers, so slots of an earlier launch with more markers would otherwise survive behind them)
int go1_debug_stamps_clear(void) {
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_go1_stamps)) != hipSuccess) return 1;
  if (hipMemset(p, 0, sizeof(g_go1_stamps)) != hipSuccess) return 1;
  return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
#endif

int go1_abi_version(void) { return GO1_ABI_VERSION; }

void go1_abi_sizes(int64_t out[4]) {
  out[0] = sizeof(go1_config);
  out[1] = sizeof(go1_state);
  out[2] = sizeof(go1_terrain);
  out[3] = sizeof(go1_step_args);
}

const char* go1_last_error(void) { return g_err.c_str(); }

int go1_create(const go1_config* cfg, go1_handle** out) {
  if (!cfg || !out) return fail(GO1_E_ARG, "go1_create: null argument");
  if (cfg->n_envs <= 0) return fail(GO1_E_ARG, "go1_create: n_envs must be > 0");
  if (cfg->decimation <= 0 || cfg->n_internal <= 0) return fail(GO1_E_ARG, "go1_create: decimation/n_internal");
  if (cfg->terrain_kind == 1 && (cfg->hf_nx < 2 || cfg->hf_ny < 2)) return fail(GO1_E_ARG, "go1_create: tile shape");
  // the capsules' deepest-point search (go1_contact.h seg_deepest) takes at most 3 grid lines per direction and 4 cell
  // diagonals per half link (0.1065 m), and 1 line per direction and 2 diagonals for the hip capsule (0.04 m,
  // SEG_SHORT_MAX; seg_deepest2's short pass): cells of at least 0.05 m
  if (cfg->terrain_kind == 1 && !(cfg->horizontal_scale >= SEG_MIN_HS))
    return fail(GO1_E_ARG, "go1_create: horizontal_scale < 0.05 m is not supported by the capsule contact search");
  if (cfg->rand_interval <= 0) return fail(GO1_E_ARG, "go1_create: rand_interval");
  // a partial last wave exists in the streamed kernel only (any scan grid but 21 x 11)
  if (cfg->n_envs % EPB != 0 && scan_compiled_in(*cfg))
    return fail(GO1_E_ARG, "go1_create: n_envs must be a multiple of 16 (one wave = 16 envs x 4 legs)");
  if (cfg->n_terms < 0 || cfg->n_terms > GO1_MAX_TERMS) return fail(GO1_E_ARG, "go1_create: n_terms");
  for (int k = 0; k < cfg->n_terms; ++k)
    if (cfg->term_ids[k] != GO1_T_NONE && (cfg->term_ids[k] < 0 || cfg->term_ids[k] >= GO1_T_COUNT))
      return fail(GO1_E_ARG, "go1_create: bad term id");
  if (cfg->traj_length < 1 || cfg->traj_length > GO1_MAX_TRAJ || cfg->traj_kind < 0 || cfg->traj_kind > 2 ||
      (cfg->traj_kind == 1 && (cfg->traj_interp < 1 || cfg->traj_length % cfg->traj_interp != 0)))
    return fail(GO1_E_ARG, "go1_create: trajectory shape");
  if (cfg->scan_nx < 1 || cfg->scan_nx > GO1_MAX_SCAN_X || cfg->scan_ny < 1 || cfg->scan_ny > GO1_MAX_SCAN_Y)
    return fail(GO1_E_ARG, "go1_create: scan_nx x scan_ny must be within 1 x 1 .. GO1_MAX_SCAN_X x GO1_MAX_SCAN_Y");
  if (cfg->measure_front_half && cfg->scan_nx < 3)
    return fail(GO1_E_ARG, "go1_create: measure_front_half keeps no row of a scan with fewer than 3 x rows");
  if (scan_compiled_in(*cfg) &&
      (memcmp(cfg->scan_x, cfg->height_grid_x, sizeof(cfg->height_grid_x)) != 0 ||
       memcmp(cfg->scan_y, cfg->height_grid_y, sizeof(cfg->height_grid_y)) != 0))
    return fail(GO1_E_ARG, "go1_create: a 21 x 11 scan needs scan_x / scan_y equal to height_grid_x / height_grid_y");
  {
    const int x_start = cfg->measure_front_half ? cfg->scan_nx / 2 + 1 : 0;
    const int n_pts = (cfg->scan_nx - x_start) * cfg->scan_ny;
    const int width = 41 + (cfg->timestep_in_obs ? 1 : 0) + (cfg->observe_heights ? 2 * n_pts : 0);
    if (cfg->num_obs != width) return fail(GO1_E_ARG, "go1_create: num_obs does not match the observation layout");
    const int traj_u = cfg->traj_kind == 1 ? 6 * (cfg->traj_length / cfg->traj_interp + 1)
                                           : (cfg->traj_kind == 2 ? 3 : 0);
    if (cfg->u_per_env != GO1_U_NOISE + width + traj_u) return fail(GO1_E_ARG, "go1_create: u_per_env");
  }
  for (int leg = 0; leg < 4; ++leg)  // joint offsets must have the sparsity the kernel exploits
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k)
        if (!((offset_mask(j) >> k) & 1) && cfg->model[13 * 10 + leg * 9 + j * 3 + k] != 0.0f)
          return fail(GO1_E_ARG, "go1_create: joint offsets must be hip (x, y, 0), thigh (0, y, 0), calf (0, 0, z)");
  // the integrator's model constants are compiled in (go1_model_consts.h): the block must match
  if (memcmp(cfg->model, GO1_MODEL_F32, sizeof(GO1_MODEL_F32)) != 0)
    return fail(GO1_E_ARG, "go1_create: model block differs from the compiled Go1 model "
                           "(regenerate csrc/go1_model_consts.h with tools/gen_model_consts.py)");
  for (int leg = 1; leg < 4; ++leg)  // the integrator reads leg 0's joint limits for every leg
    for (int k = 0; k < 6; ++k)
      if (cfg->hard_limits[leg * 6 + k] != cfg->hard_limits[k])
        return fail(GO1_E_ARG, "go1_create: hard joint limits must be the same for every leg");
  go1_handle* h = new (std::nothrow) go1_handle();
  if (!h) return fail(GO1_E_ARG, "go1_create: out of host memory");
  h->cfg = *cfg;
  h->streamed = !scan_compiled_in(*cfg);
  h->spec = !h->streamed && spec_match(*cfg);
  if (int rc = create_device(h, cfg)) {
    go1_destroy(h);  // the one clean-up path: the handle and whatever was allocated before the failure
    return rc;
  }
  *out = h;
  return GO1_OK;
}

int go1_bind(go1_handle* h, const go1_state* s, const go1_plane* planes) {
  if (!h || !s || !planes) return fail(GO1_E_ARG, "go1_bind: null argument (state and plane descriptors required)");
  PlaneRow table[GO1_STATE_PLANES];
  memcpy(table, STATE_PLANES, sizeof(table));
  table[GO1_PLANE_INDEX(go1_state, lag)].cols = 12 * GO1_LAG_STEPS(h->cfg.decimation);
  table[GO1_PLANE_INDEX(go1_state, trajectory)].cols = 6 * (int64_t)h->cfg.traj_length;
  table[GO1_PLANE_INDEX(go1_state, episode_sums)].cols = h->cfg.n_terms + 3;
  if (int rc = check_planes("go1_bind", s, table, planes, h->cfg.n_envs, fail)) return rc;
  h->st = *s;
  h->bound = true;
  return GO1_OK;
}

int go1_set_terrain(go1_handle* h, const go1_terrain* t) {
  if (!h || !t) return fail(GO1_E_ARG, "go1_set_terrain: null argument");
  if (!t->env_origins || !t->env_terrain_origin || !t->env_tile)
    return fail(GO1_E_ARG, "go1_set_terrain: env_origins / env_terrain_origin / env_tile required");
  if (h->cfg.terrain_kind == 1 && (!t->tiles || t->n_tiles <= 0))
    return fail(GO1_E_ARG, "go1_set_terrain: tunnel terrain needs tiles");
  h->ter = *t;
  h->has_terrain = true;
  return GO1_OK;
}

int go1_step(go1_handle* h, const go1_step_args* a, void* stream) {
  if (!h || !a) return fail(GO1_E_ARG, "go1_step: null argument");
  if (!h->bound || !h->has_terrain) return fail(GO1_E_STATE, "go1_step: call go1_bind and go1_set_terrain first");
  if (!a->actions || !a->obs || !a->priv || !a->rew || !a->reset || !a->time_out || !a->extras_time_outs)
    return fail(GO1_E_ARG, "go1_step: actions and every output buffer are required");
  bool inj = a->inj_dof != nullptr;
  if (inj && (!a->inj_root || !a->inj_contact)) return fail(GO1_E_ARG, "go1_step: partial injected state");
  hipStream_t s = (hipStream_t)stream;
  const int n = h->cfg.n_envs;
  KArgs K;
  K.st = h->st;
  K.ter = h->ter;
  K.a = *a;
  K.flags = h->d_flags;
  K.cur = (int)(h->count % 3);
  K.prv = (int)((h->count + 2) % 3);
  K.nxt = (int)((h->count + 1) % 3);
  K.prev_time_out = h->prev_time_out;
  K.prev_extras = h->prev_extras;
  const int bank = (int)(h->count & 1);
  K.bucket_r = h->d_bucket_r;
  K.bucket_sum = h->d_bucket_sum ? h->d_bucket_sum + bank * GO1_MAX_TERMS : nullptr;
  dim3 grid((n + SEPB - 1) / SEPB), block(TPB);  // n % 16 == 0 but for the streamed kernel (go1_create)
  const bool full = !h->cfg.measure_front_half;  // 231 scanned points: 15 per lane instead of 7
  if (a->episode_log_count && (!a->episode_log || a->episode_log_cap < 0 || h->cfg.indefinite_slots))
    return fail(GO1_E_ARG, "go1_step: a compact episode log needs episode_log, a capacity >= 0 and no indefinite "
                           "reward slots (their bucket pass rewrites rows by env)");
  auto go = [&](auto kern) { launch_timed(kern, grid, block, s, a->ev_begin, a->ev_end, h->d_cfg, K); };
  if (h->streamed) {  // any scan grid: no scan registers, the epilogue streams the points
    if (inj) go(go1_step_kernel<true, 0, false>);
    else go(go1_step_kernel<false, 0, false>);
  } else if (inj) {  // parity mode: the README configuration replays through the specialised kernel too
    if (full) go(go1_step_kernel<true, 15, false>);
    else if (h->spec) go(go1_step_kernel<true, 7, true>);
    else go(go1_step_kernel<true, 7, false>);
  } else if (h->spec) {  // the README configuration (go1_spec.h): measure_front_half, 7 points per lane
    go(go1_step_kernel<false, 7, true>);
  } else {
    if (full) go(go1_step_kernel<false, 15, false>);
    else go(go1_step_kernel<false, 7, false>);
  }
  HIP_TRY(hipGetLastError());
  if (h->cfg.indefinite_slots) {
    hipLaunchKernelGGL(go1_bucket_kernel, dim3((n + 255) / 256), dim3(256), 0, s, h->d_cfg, h->st, h->d_bucket_r,
                       h->d_bucket_sum + bank * GO1_MAX_TERMS, h->d_bucket_sum + (bank ^ 1) * GO1_MAX_TERMS,
                       a->reset, a->rew, a->episode_log);
    HIP_TRY(hipGetLastError());
  }
  h->prev_time_out = a->time_out;
  h->prev_extras = a->extras_time_outs;
  h->count++;
  return GO1_OK;
}

int go1_specialize(go1_handle* h, int enable) {
  if (!h) return fail(GO1_E_ARG, "go1_specialize: null handle");
  if (enable && !spec_match(h->cfg)) return fail(GO1_E_ARG, "go1_specialize: the config differs from the specialised one (go1_spec.h)");
  if (enable && h->streamed) return fail(GO1_E_ARG, "go1_specialize: the handle runs the streamed height scan (go1_scan_mode)");
  h->spec = enable != 0;
  return GO1_OK;
}

int go1_is_specialized(go1_handle* h) { return h && h->spec ? 1 : 0; }

int go1_scan_mode(go1_handle* h, int streamed) {
  if (!h) return fail(GO1_E_ARG, "go1_scan_mode: null handle");
  if (!streamed && !scan_compiled_in(h->cfg))
    return fail(GO1_E_ARG, "go1_scan_mode: only a 21 x 11 scan has register-resident kernels");
  // (a 21 x 11 handle has n_envs % 16 == 0, go1_create: both paths take it)
  h->streamed = streamed != 0;
  h->spec = !h->streamed && spec_match(h->cfg);
  return GO1_OK;
}

int go1_is_streamed(go1_handle* h) { return h && h->streamed ? 1 : 0; }

int go1_sync_time_outs(go1_handle* h, void* stream) {
  if (!h) return fail(GO1_E_ARG, "go1_sync_time_outs: null handle");
  if (!h->prev_time_out) return GO1_OK;  // no step yet
  const int n = h->cfg.n_envs;
  hipLaunchKernelGGL(go1_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n,
                     h->d_flags + (h->count + 2) % 3, h->prev_time_out, h->prev_extras);
  HIP_TRY(hipGetLastError());
  return GO1_OK;
}

int go1_time_outs_pending(go1_handle* h, int64_t out[3]) {
  if (!h || !out) return fail(GO1_E_ARG, "go1_time_outs_pending: null argument");
  out[0] = out[1] = out[2] = 0;
  if (!h->prev_time_out) return GO1_OK;  // no step yet: extras_time_outs is current
  out[0] = (int64_t)(uintptr_t)(h->d_flags + (h->count + 2) % 3);
  out[1] = (int64_t)(uintptr_t)h->prev_time_out;
  out[2] = (int64_t)(uintptr_t)h->prev_extras;
  return GO1_OK;
}

int go1_reset_envs(go1_handle* h, const uint8_t* mask, const float* uniforms, uint64_t rng_seed, uint64_t rng_step,
                   void* stream) {
  if (!h || !mask) return fail(GO1_E_ARG, "go1_reset_envs: null argument");
  if (!h->bound || !h->has_terrain) return fail(GO1_E_STATE, "go1_reset_envs: bind state and terrain first");
  const int n = h->cfg.n_envs;
  hipLaunchKernelGGL(go1_reset_kernel, dim3((n + EPB - 1) / EPB), dim3(TPB), 0, (hipStream_t)stream, h->d_cfg,
                     h->st, h->ter, mask, nullptr, 0, uniforms, rng_seed, rng_step);
  HIP_TRY(hipGetLastError());
  return GO1_OK;
}

int go1_reset_idx(go1_handle* h, const int32_t* ids, int32_t n_ids, const float* uniforms, uint64_t rng_seed,
                  uint64_t rng_step, void* stream) {
  if (!h || (!ids && n_ids > 0) || n_ids < 0) return fail(GO1_E_ARG, "go1_reset_idx: bad argument");
  if (!h->bound || !h->has_terrain) return fail(GO1_E_STATE, "go1_reset_idx: bind state and terrain first");
  if (n_ids == 0) return GO1_OK;  // reset_idx returns early on an empty list (:220-221)
  hipLaunchKernelGGL(go1_reset_kernel, dim3((n_ids + EPB - 1) / EPB), dim3(TPB), 0, (hipStream_t)stream, h->d_cfg,
                     h->st, h->ter, nullptr, ids, n_ids, uniforms, rng_seed, rng_step);
  HIP_TRY(hipGetLastError());
  return GO1_OK;
}

int go1_actuator_net(go1_handle* h, const float* x, float* out, int32_t n_rows, void* stream) {
  if (!h || !x || !out || n_rows < 0) return fail(GO1_E_ARG, "go1_actuator_net: bad argument");
  if (n_rows == 0) return GO1_OK;
  const int groups = (n_rows + 15) / 16;
  hipLaunchKernelGGL(go1_actuator_kernel, dim3(groups < 4096 ? groups : 4096), dim3(64), 0, (hipStream_t)stream,
                     h->d_cfg, x, out, n_rows);
  HIP_TRY(hipGetLastError());
  return GO1_OK;
}

int go1_destroy(go1_handle* h) {
  if (!h) return GO1_OK;
  if (h->d_cfg) (void)hipFree(h->d_cfg);
  if (h->d_flags) (void)hipFree(h->d_flags);
  if (h->d_bucket_r) (void)hipFree(h->d_bucket_r);
  if (h->d_bucket_sum) (void)hipFree(h->d_bucket_sum);
  delete h;
  return GO1_OK;
}

}  // extern "C"
