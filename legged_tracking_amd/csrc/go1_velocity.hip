// go1_velocity.hip -- MI355X (gfx950) fused Go1 velocity-tracking step + C ABI (include/go1_velocity.h).
//
// One go1_vel_step = one VelocityTrackingEasyEnv.step + HistoryWrapper.step
// (go1_gym/envs/base/legged_robot_velocity_tracking.py, bare :N below) in two launches:
//   go1_vel_step_kernel: 4 x [actuator-net torques (:925-964) -> the native articulated-body integrator
//     of go1_phys.h (phys_substep, plane terrain)] -> post-physics (:108-154): kinematics, the gait
//     clock (_step_contact_targets :844-923), DR (:714-717), terminations (:156-166), the CoRL reward
//     terms and command sums (:281-318, go1_gym/envs/rewards/corl_rewards.py), reset_idx's state part
//     (:168-257), observations (:320-509), the epilogue (:144-149) and the appended obs_history row.
//   go1_vel_curriculum_kernel: workgroups 0 .. nblk - 1 run _resample_commands (:728-842) for the envs the
//     step reset (RewardThresholdCurriculum.update, Curriculum.sample: go1_gym/envs/base/curriculum.py) and
//     patch their observed commands, then the interval resample of the next step ahead of time, the per-env
//     draws split over the workgroups; the other workgroups shift the history (obs_history[:, 70:] -> the
//     new buffer) when the sliding window rewinds.
// Lane layout of the step kernel as in go1_step.hip: 16 lanes per env = 4 legs x 4 roles, four envs per
// one-wave block.  Post-physics arithmetic is f32 with contraction off in torch's operation order, the
// transcendentals of the gait clock and the rewards via f64 (correctly rounded f32 but for rare double
// roundings), so the results match oracle/vel_oracle.py to the ulp of numpy's own exp / sin / erf.
// This file is the host side (the handle, the plane table, the C ABI); the kernels are in its parts
// go1_vel_step.h and go1_vel_curriculum.h, on the device layer of go1_device.h.
#include "go1_device.h"
#include "go1_step_shared.h"
#include "../../include/go1_velocity.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

#define GO1_VELOCITY_HIP  // the parts refuse to be included on their own
#include "go1_vel_step.h"        // f32 helpers, foot_state, vel_reset_env, VArgs, the step / reset / mask kernels
#include "go1_vel_curriculum.h"  // RngD, CArgs, CkShared, resample_*, hist_shift, the curriculum / list kernels

// =====================================================================
//                                C ABI
// =====================================================================
#ifdef GO1_VEL_STAMPS
extern "C" int go1_vel_stamps(void* host, int reset) {
  if (host && hipMemcpyFromSymbol(host, HIP_SYMBOL(g_vstamps), sizeof(g_vstamps), 0, hipMemcpyDeviceToHost) != hipSuccess)
    return 1;
  if (reset) {
    static const unsigned long long z[2][16] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_vstamps), z, sizeof(z), 0, hipMemcpyHostToDevice) != hipSuccess) return 1;
  }
  return 0;
}
#endif
struct go1_vel_handle {
  go1_config cfg;
  go1_vel_config vcfg;
  go1_config* d_cfg = nullptr;
  go1_vel_config* d_vcfg = nullptr;
  double* d_grid = nullptr;
  double* d_cdf = nullptr;
  int32_t* d_cdf_ok = nullptr;
  uint8_t* d_mask = nullptr;  // reset_idx's env mask (stream-ordered reuse)
  int32_t* d_adj_ptr = nullptr;  // neighbourhood table of the curriculum update (CSR over the bins)
  int32_t* d_adj_idx = nullptr;
  int32_t* d_done = nullptr;     // completion count of the curriculum workgroups (zero between launches)
  CkRec* d_clist = nullptr;      // selection lists: 3 slots (steps alternate 0 / 1, explicit resamples 2) x (B, A)
  unsigned long long* d_ccnt = nullptr;  // their lengths per slot (B low word, A high word)
  int slot = 0;                  // the next step's slot
  uint32_t ck_delay = 0;         // CArgs.delay (GO1_VEL_CK_DELAY at create; tests only)
  go1_vel_state st;
  const float* env_origins = nullptr;
  bool bound = false;
};

static thread_local std::string g_verr;
static int vfail(int code, const std::string& msg) {
  g_verr = msg;
  return code;
}
#define VHIP_TRY(x) GO1_HIP_TRY(vfail, x)

#define P(f, cols, dt) GO1_PLANE(go1_vel_state, f, cols, GO1_DTYPE_##dt)
static const PlaneRow VEL_STATE_PLANES[] = {
    P(root, 13, F32), P(dof_pos, 12, F32), P(dof_vel, 12, F32), P(last_actions, 12, F32), P(last_dof_vel, 12, F32),
    P(lag, 12 * VLAG, F32), P(pos_err_hist, 24, F32), P(vel_hist, 24, F32), P(motor_strength, 12, F32),
    P(motor_offset, 12, F32), P(friction, 1, F32), P(restitution, 1, F32), P(payload, 1, F32),
    P(episode_length, 1, I32), P(last_last_actions, 12, F32), P(last_joint_pos_target, 12, F32),
    P(last_last_joint_pos_target, 12, F32), P(commands, GO1_VEL_NUM_COMMANDS, F32), P(gait_indices, 1, F32),
    P(last_contacts, 4, F32), P(command_sums, 0, F32), P(episode_sums, 0, F32), P(command_bins, 1, I32),
    P(command_categories, 1, I32), {"curriculum_weights", offsetof(go1_vel_state, curriculum_weights), 0,
                                    GO1_DTYPE_F64, GO1_VEL_N_CATEGORIES}};
#undef P
static_assert(sizeof(VEL_STATE_PLANES) / sizeof(VEL_STATE_PLANES[0]) == GO1_VEL_STATE_PLANES &&
                  sizeof(go1_vel_state) == GO1_VEL_STATE_PLANES * sizeof(void*), "go1_vel_state planes");

// curriculum workgroups: the per-env sampling splits over them (a 4096-env resample: 256 envs each)
static int curriculum_blocks(int n) { return std::max(1, std::min(16, n / 256)); }

static CArgs curriculum_args(go1_vel_handle* h) {
  CArgs K;
  memset(&K, 0, sizeof(K));
  K.st = h->st;
  K.episode_length = h->st.episode_length;
  K.grid = h->d_grid;
  K.adj_ptr = h->d_adj_ptr;
  K.adj_idx = h->d_adj_idx;
  K.cdf = h->d_cdf;
  K.cdf_ok = h->d_cdf_ok;
  K.n_envs = h->cfg.n_envs;
  K.env_id_offset = h->cfg.env_id_offset;
  K.nb = h->vcfg.n_bins;
  K.R = h->vcfg.resample_interval;
  K.nblk = curriculum_blocks(h->cfg.n_envs);
  K.done = h->d_done;
  K.delay = h->ck_delay;
  return K;
}

// go1_vel_create's device allocations and their first contents.  On an error the handle keeps what was allocated
// so far: the caller releases it through go1_vel_destroy.
static int vel_create_device(go1_vel_handle* h, const go1_config* cfg, const go1_vel_config* vel, const double* grid) {
  const size_t gsz = (size_t)GO1_VEL_N_KEYS * vel->n_bins * sizeof(double);
  const size_t csz = (size_t)GO1_VEL_N_CATEGORIES * vel->n_bins * sizeof(double);
  if (hipMalloc(&h->d_cfg, sizeof(go1_config)) != hipSuccess || hipMalloc(&h->d_vcfg, sizeof(go1_vel_config)) != hipSuccess ||
      hipMalloc(&h->d_grid, gsz) != hipSuccess || hipMalloc(&h->d_cdf, csz) != hipSuccess ||
      hipMalloc(&h->d_cdf_ok, GO1_VEL_N_CATEGORIES * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&h->d_mask, cfg->n_envs) != hipSuccess || hipMalloc(&h->d_done, sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&h->d_clist, (size_t)6 * cfg->n_envs * sizeof(CkRec)) != hipSuccess ||
      hipMalloc(&h->d_ccnt, 3 * sizeof(unsigned long long)) != hipSuccess) {
    return vfail(GO1_E_HIP, "go1_vel_create: hipMalloc failed");
  }

  VHIP_TRY(hipMemcpy(h->d_cfg, cfg, sizeof(go1_config), hipMemcpyHostToDevice));
  VHIP_TRY(hipMemcpy(h->d_vcfg, vel, sizeof(go1_vel_config), hipMemcpyHostToDevice));
  VHIP_TRY(hipMemcpy(h->d_grid, grid, gsz, hipMemcpyHostToDevice));
  {  // get_local_bins (curriculum.py:123-133): cell j is adjacent to bin b when every key is within
     // local_range -- the numpy comparisons grid[:, j] >= grid[:, b] - r and <= grid[:, b] + r in f64
    const int nb = vel->n_bins;
    std::vector<int32_t> ptr(nb + 1, 0), idx;
    for (int b = 0; b < nb; ++b) {
      for (int j = 0; j < nb; ++j) {
        bool adj = true;
        for (int k = 0; k < GO1_VEL_N_KEYS && adj; ++k) {
          const double gb = grid[(size_t)k * nb + b], gj = grid[(size_t)k * nb + j], r = vel->local_range[k];
          adj = gj >= gb - r && gj <= gb + r;
        }
        if (adj) idx.push_back(j);
      }
      ptr[b + 1] = (int32_t)idx.size();
    }
    if (idx.empty()) idx.push_back(0);
    VHIP_TRY(hipMalloc(&h->d_adj_ptr, ptr.size() * sizeof(int32_t)));
    VHIP_TRY(hipMalloc(&h->d_adj_idx, idx.size() * sizeof(int32_t)));
    VHIP_TRY(hipMemcpy(h->d_adj_ptr, ptr.data(), ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    VHIP_TRY(hipMemcpy(h->d_adj_idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  VHIP_TRY(hipMemset(h->d_cdf_ok, 0, GO1_VEL_N_CATEGORIES * sizeof(int32_t)));
  VHIP_TRY(hipMemset(h->d_done, 0, sizeof(int32_t)));
  VHIP_TRY(hipMemset(h->d_ccnt, 0, 3 * sizeof(unsigned long long)));
  VHIP_TRY(hipMemset(h->d_clist, 0, (size_t)6 * cfg->n_envs * sizeof(CkRec)));
  return GO1_OK;
}

extern "C" {
int go1_vel_abi_version(void) { return GO1_VEL_ABI_VERSION; }

void go1_vel_abi_sizes(int64_t out[3]) {
  out[0] = sizeof(go1_vel_config);
  out[1] = sizeof(go1_vel_state);
  out[2] = sizeof(go1_vel_step_args);
}

const char* go1_vel_last_error(void) { return g_verr.c_str(); }

int go1_vel_create(const go1_config* cfg, const go1_vel_config* vel, const double* grid, go1_vel_handle** out) {
  if (!cfg || !vel || !grid || !out) return vfail(GO1_E_ARG, "go1_vel_create: null argument");
  if (cfg->n_envs <= 0 || cfg->n_envs % EPB != 0)
    return vfail(GO1_E_ARG, "go1_vel_create: n_envs must be a positive multiple of 16");
  if (vel->n_envs != cfg->n_envs) return vfail(GO1_E_ARG, "go1_vel_create: n_envs differs between the configs");
  if (cfg->terrain_kind != 0) return vfail(GO1_E_ARG, "go1_vel_create: the velocity step runs on the plane");
  if (cfg->n_internal <= 0 || GO1_LAG_STEPS(cfg->decimation) != VLAG)
    return vfail(GO1_E_ARG, "go1_vel_create: decimation must be 4..6 (two stored lag steps)");
  if (vel->n_terms < 0 || vel->n_terms > GO1_VEL_MAX_TERMS) return vfail(GO1_E_ARG, "go1_vel_create: n_terms");
  for (int k = 0; k < vel->n_terms; ++k)
    if (vel->term_ids[k] < 0 || vel->term_ids[k] >= GO1_VT_COUNT) return vfail(GO1_E_ARG, "go1_vel_create: term id");
  if (vel->n_bins <= 0 || vel->n_bins > GO1_VEL_MAX_BINS) return vfail(GO1_E_ARG, "go1_vel_create: n_bins");
  if (vel->resample_interval <= 0 || vel->rand_interval <= 0)
    return vfail(GO1_E_ARG, "go1_vel_create: resample / rand interval");
  if (vel->n_task < 0 || vel->n_task > 4) return vfail(GO1_E_ARG, "go1_vel_create: n_task");
  if (vel->history_len < 1) return vfail(GO1_E_ARG, "go1_vel_create: history_len");
  if (memcmp(cfg->model, GO1_MODEL_F32, sizeof(GO1_MODEL_F32)) != 0)
    return vfail(GO1_E_ARG, "go1_vel_create: model block differs from the compiled Go1 model");
  go1_vel_handle* h = new (std::nothrow) go1_vel_handle();
  if (!h) return vfail(GO1_E_ARG, "go1_vel_create: out of host memory");
  h->cfg = *cfg;
  h->vcfg = *vel;
  if (const char* d = getenv("GO1_VEL_CK_DELAY")) h->ck_delay = (uint32_t)strtoul(d, nullptr, 10);
  if (int rc = vel_create_device(h, cfg, vel, grid)) {
    go1_vel_destroy(h);  // the one clean-up path: the handle and whatever was allocated before the failure
    return rc;
  }
  *out = h;
  return GO1_OK;
}

int go1_vel_bind(go1_vel_handle* h, const go1_vel_state* s, const go1_plane* planes) {
  if (!h || !s || !planes) return vfail(GO1_E_ARG, "go1_vel_bind: null argument");
  PlaneRow table[GO1_VEL_STATE_PLANES];
  memcpy(table, VEL_STATE_PLANES, sizeof(table));
  table[GO1_PLANE_INDEX(go1_vel_state, command_sums)].cols = h->vcfg.n_terms + GO1_VEL_SUM_EXTRA;
  table[GO1_PLANE_INDEX(go1_vel_state, episode_sums)].cols = h->vcfg.n_terms + 1;
  table[GO1_PLANE_INDEX(go1_vel_state, curriculum_weights)].cols = h->vcfg.n_bins;
  if (int rc = check_planes("go1_vel_bind", s, table, planes, h->cfg.n_envs, vfail)) return rc;
  h->st = *s;
  h->bound = true;
  VHIP_TRY(hipMemset(h->d_cdf_ok, 0, GO1_VEL_N_CATEGORIES * sizeof(int32_t)));  // new weights plane
  return GO1_OK;
}

int go1_vel_set_origins(go1_vel_handle* h, const float* env_origins) {
  if (!h || !env_origins) return vfail(GO1_E_ARG, "go1_vel_set_origins: null argument");
  h->env_origins = env_origins;
  return GO1_OK;
}

int go1_vel_step(go1_vel_handle* h, const go1_vel_step_args* a, void* stream) {
  if (!h || !a) return vfail(GO1_E_ARG, "go1_vel_step: null argument");
  if (!h->bound || !h->env_origins) return vfail(GO1_E_STATE, "go1_vel_step: bind the state and set the origins first");
  if (!a->actions || !a->obs || !a->priv || !a->rew || !a->reset || !a->time_out || !a->extras_time_outs)
    return vfail(GO1_E_ARG, "go1_vel_step: actions and every output buffer are required");
  const bool inj = a->inj_dof != nullptr;
  if (inj && (!a->inj_root || !a->inj_contact || !a->inj_feet))
    return vfail(GO1_E_ARG, "go1_vel_step: partial injected state");
  if ((a->uniforms == nullptr) != (a->uniforms_f64 == nullptr))
    return vfail(GO1_E_ARG, "go1_vel_step: parity mode needs both uniform arrays");
  if (a->resample_next && a->uniforms && (!a->uniforms_next || !a->uniforms_f64_next))
    return vfail(GO1_E_ARG, "go1_vel_step: parity mode resamples ahead with the next step's uniforms");
  const int hist_w = GO1_VEL_NUM_OBS * h->vcfg.history_len;
  const int64_t ld_in = a->obs_history_in_ld ? a->obs_history_in_ld : hist_w;
  const int64_t ld_out = a->obs_history_out_ld ? a->obs_history_out_ld : hist_w;
  if ((a->obs_history_in == nullptr) != (a->obs_history_out == nullptr) ||
      (a->obs_history_in && a->obs_history_in == a->obs_history_out))
    return vfail(GO1_E_ARG, "go1_vel_step: obs_history in and out are two distinct buffers (or both NULL)");
  if (a->obs_history_in && (ld_in < hist_w || ld_out < hist_w || (hist_w & 1) || (ld_in & 1) || (ld_out & 1) ||
                            ((uintptr_t)a->obs_history_in & 7) || ((uintptr_t)a->obs_history_out & 7)))
    return vfail(GO1_E_ARG, "go1_vel_step: obs_history row strides >= 70 x history_len, even, rows 8-byte aligned");
  // out = in + 70 with the same stride: a sliding window, new[:, :W - 70] IS old[:, 70:] (no shift)
  const bool window = a->obs_history_in && ld_in == ld_out && a->obs_history_out == a->obs_history_in + GO1_VEL_NUM_OBS;
  if (a->episode_log_count && (!a->episode_log || a->episode_log_cap < 0))
    return vfail(GO1_E_ARG, "go1_vel_step: a compact episode log needs episode_log and a capacity");
  hipStream_t s = (hipStream_t)stream;
  const int n = h->cfg.n_envs;
  VArgs K;
  K.st = h->st;
  K.a = *a;
  K.env_origins = h->env_origins;
  K.hist_w = hist_w;
  K.hist_ld = ld_out;
  const int slot = h->slot;
  h->slot ^= 1;
  K.clist = h->d_clist + (size_t)slot * 2 * n;
  K.ccnt = h->d_ccnt + slot;
  K.czero = h->d_ccnt + (slot ^ 1);
  K.doA = a->resample_next ? 1 : 0;
  CArgs C = curriculum_args(h);
  C.list = K.clist;
  C.cnt = K.ccnt;
  C.hist_in = window ? nullptr : a->obs_history_in;
  C.hist_out = a->obs_history_out;
  C.ld_in = ld_in;
  C.ld_out = ld_out;
  C.hist_w = K.hist_w;
  C.hist_aligned = C.hist_w % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && ((uintptr_t)C.hist_in % 16) == 0 &&
                   ((uintptr_t)C.hist_out % 16) == 0;
  auto go = [&](auto kern) {
    launch_timed(kern, dim3(n / SEPB), dim3(TPB), s, a->ev_begin, a->ev_end, h->d_cfg, h->d_vcfg, K);
  };
  if (inj) go(go1_vel_step_kernel<true>);
  else go(go1_vel_step_kernel<false>);
  VHIP_TRY(hipGetLastError());
  C.seed = a->rng_seed;
  C.maskB = a->reset;
  C.UB = a->uniforms;
  C.UDB = a->uniforms_f64;
  C.stepB = a->rng_step;
  C.doA = a->resample_next ? 1 : 0;
  C.UA = a->uniforms_next;
  C.UDA = a->uniforms_f64_next;
  C.stepA = a->rng_step + 1;
  C.time_out = a->time_out;
  C.extras_time_outs = a->extras_time_outs;
  C.obs = a->obs;
  // workgroups nblk..: the history shift, one per remaining CU (the launch's LDS allows one workgroup per
  // CU), four 16-byte chunks in flight per lane; fewer for small batches
  const size_t chunks = (size_t)n * (size_t)((K.hist_w - GO1_VEL_NUM_OBS) / 4 + 64);
  const int shift_blocks =
      C.hist_in ? (int)std::min<size_t>(256 - C.nblk, std::max<size_t>(1, (chunks + 4 * CK_THREADS - 1) / (4 * CK_THREADS)))
                : 0;
  hipLaunchKernelGGL(go1_vel_curriculum_kernel, dim3(C.nblk + shift_blocks), dim3(CK_THREADS), 0, s, h->d_vcfg, C.n_envs, C.nb,
                     C.cnt, C.list, C.cdf, C.cdf_ok, C);
  VHIP_TRY(hipGetLastError());
  return GO1_OK;
}

int go1_vel_resample(go1_vel_handle* h, const uint8_t* mask, const float* uniforms, const double* uniforms_f64,
                     uint64_t rng_seed, uint64_t rng_step, void* stream) {
  if (!h) return vfail(GO1_E_ARG, "go1_vel_resample: null handle");
  if (!h->bound) return vfail(GO1_E_STATE, "go1_vel_resample: bind the state first");
  if ((uniforms == nullptr) != (uniforms_f64 == nullptr))
    return vfail(GO1_E_ARG, "go1_vel_resample: parity mode needs both uniform arrays");
  CArgs C = curriculum_args(h);
  C.seed = rng_seed;
  if (mask) {
    C.maskB = mask;
    C.UB = uniforms;
    C.UDB = uniforms_f64;
    C.stepB = rng_step;
  } else {
    C.doA = 1;
    C.UA = uniforms;
    C.UDA = uniforms_f64;
    C.stepA = rng_step;
  }
  // the lists (slot 2) from the mask / the interval condition, then the curriculum on them
  C.list = h->d_clist + (size_t)4 * C.n_envs;
  C.cnt = h->d_ccnt + 2;
  hipLaunchKernelGGL(go1_vel_list_kernel, dim3(1), dim3(CK_THREADS), 0, (hipStream_t)stream, h->d_vcfg, C,
                     const_cast<CkRec*>(C.list), const_cast<unsigned long long*>(C.cnt));
  hipLaunchKernelGGL(go1_vel_curriculum_kernel, dim3(C.nblk), dim3(CK_THREADS), 0, (hipStream_t)stream, h->d_vcfg, C.n_envs, C.nb,
                     C.cnt, C.list, C.cdf, C.cdf_ok, C);
  VHIP_TRY(hipGetLastError());
  return GO1_OK;
}

int go1_vel_reset_idx(go1_vel_handle* h, const int32_t* ids, int32_t n_ids, const float* uniforms,
                      const double* uniforms_f64, uint64_t rng_seed, uint64_t rng_step, float* episode_log,
                      int32_t* episode_log_count, int32_t episode_log_cap, int32_t episode_log_tag, void* stream) {
  if (!h || (!ids && n_ids > 0) || n_ids < 0) return vfail(GO1_E_ARG, "go1_vel_reset_idx: bad argument");
  if (!h->bound || !h->env_origins) return vfail(GO1_E_STATE, "go1_vel_reset_idx: bind the state and origins first");
  if (n_ids == 0) return GO1_OK;  // (:178-179)
  if (episode_log_count && !episode_log) return vfail(GO1_E_ARG, "go1_vel_reset_idx: episode_log missing");
  hipStream_t s = (hipStream_t)stream;
  const int n = h->cfg.n_envs;
  // _resample_commands first (:182): a mask of the ids for the curriculum launch
  uint8_t* mask = h->d_mask;
  VHIP_TRY(hipMemsetAsync(mask, 0, n, s));
  hipLaunchKernelGGL(go1_vel_mask_kernel, dim3((n_ids + 255) / 256), dim3(256), 0, s, ids, n_ids, n, mask);
  int rc = go1_vel_resample(h, mask, uniforms, uniforms_f64, rng_seed, rng_step, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(go1_vel_reset_kernel, dim3((n_ids + EPB - 1) / EPB), dim3(TPB), 0, s, h->d_vcfg, h->st,
                     h->env_origins, ids, n_ids, n, uniforms, rng_seed, rng_step, h->cfg.env_id_offset, episode_log,
                     episode_log_count, episode_log_cap, episode_log_tag);
  VHIP_TRY(hipGetLastError());
  return GO1_OK;
}

int go1_vel_destroy(go1_vel_handle* h) {
  if (!h) return GO1_OK;
  if (h->d_done) (void)hipFree(h->d_done);
  if (h->d_clist) (void)hipFree(h->d_clist);
  if (h->d_ccnt) (void)hipFree(h->d_ccnt);
  if (h->d_cfg) (void)hipFree(h->d_cfg);
  if (h->d_vcfg) (void)hipFree(h->d_vcfg);
  if (h->d_grid) (void)hipFree(h->d_grid);
  if (h->d_cdf) (void)hipFree(h->d_cdf);
  if (h->d_cdf_ok) (void)hipFree(h->d_cdf_ok);
  if (h->d_mask) (void)hipFree(h->d_mask);
  if (h->d_adj_ptr) (void)hipFree(h->d_adj_ptr);
  if (h->d_adj_idx) (void)hipFree(h->d_adj_idx);
  delete h;
  return GO1_OK;
}
}  // extern "C"
