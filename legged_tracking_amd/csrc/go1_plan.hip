// go1_plan.hip -- the local target planner of include/go1_plan.h: one launch per env step, after the step kernel.
//
// One workgroup of 256 lanes per env.  Every lane computes the cheap part (the relative pose of the global target,
// the plan decision) from uniform loads; unless the env plans with its goal further than 1 m away, lanes 1 .. 255
// leave there and lane 0 finishes the env: at plan_interval = 100 that is 99 steps in 100.  A planning env stages
// its 2 nx ny measured heights and the grid coordinates in LDS, then
//   1. one work item per (grid row, footprint) -- a footprint is a unique row of what enters the ellipsoid test --
//      walks the row's points, both layers of a grid point in one trip, and leaves at the first point inside the
//      ellipsoid; the lanes of a wave work on the same row, so every LDS read is a broadcast;
//   2. every lane takes the lexicographic minimum of (key, index) over its share of the candidates with a valid
//      footprint; a wave reduces with lane shuffles, the four waves through LDS.  No sort: the minimum of
//      (key, index) is the first valid entry of a stable argsort by key.
// The relative poses use the step kernel's own functions (go1_torch_math.h, contraction off), so a local target
// equal to the global one gives the commands the step kernel wrote, bit for bit.  The error message and the launch
// check are go1_host.h's, shared with the other add-on libraries.
#include "../../include/go1_plan.h"
#include "go1_device.h"
#include "go1_host.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_PTS = GO1_PLAN_MAX_X * GO1_PLAN_MAX_Y;

struct Params {
  go1_plan_config c;
  go1_plan_tables t;
  go1_plan_state s;
  go1_plan_args a;
};

// quat_apply_yaw (math_utils.py:12-16): normalize((0, 0, qz, qw)), then quat_apply in torch's order
__device__ __forceinline__ void quat_apply_yaw_f(const float* q, const float* b, float* out) {
  float z = q[2], w = q[3];
  float n = sqrtf(fmaf(w, w, fmaf(z, z, 0.0f)));
  if (n < 1e-9f) n = 1e-9f;
  z = z / n;
  w = w / n;
  const float t0 = (0.0f * b[2] - z * b[1]) * 2.0f, t1 = (z * b[0] - 0.0f * b[2]) * 2.0f, t2 = 0.0f;
  out[0] = b[0] + w * t0 + (0.0f * t2 - z * t1);
  out[1] = b[1] + w * t1 + (z * t0 - 0.0f * t2);
  out[2] = b[2] + w * t2;
}

// _compute_relative_target_pose (:922-932), as post_kin of the step kernel has it
__device__ __forceinline__ void relative_pose(const float* root, const float* rpy, const float* pose, float* lin,
                                              float* rot) {
  const float qb[4] = {root[3], root[4], root[5], root[6]};
  const float rel_in[3] = {pose[0] - root[0], pose[1] - root[1], pose[2] - root[2]};
  quat_apply_yaw_inverse_f(qb, rel_in, lin);
#pragma unroll
  for (int i = 0; i < 3; ++i) rot[i] = wrap_to_pi_f(pose[3 + i] - rpy[i]);
}

__device__ __forceinline__ bool better(float k, int i, float bk, int bi) { return k < bk || (k == bk && i < bi); }

__global__ __launch_bounds__(THREADS) void go1_plan_step_kernel(const Params p) {
  const go1_plan_config& c = p.c;
  const go1_plan_state& s = p.s;
  const go1_plan_args& a = p.a;
  const int t = threadIdx.x;
  const int e = blockIdx.x;

  __shared__ float s_h[2 * MAX_PTS];
  __shared__ float s_gx[GO1_PLAN_MAX_X], s_gy[GO1_PLAN_MAX_Y];
  __shared__ uint8_t s_valid[GO1_PLAN_MAX_CAND];
  __shared__ float s_key[WAVES];
  __shared__ int s_idx[WAVES];

  float* o = a.obs + (size_t)e * a.obs_stride;
  float* oh = a.obs_history ? a.obs_history + (size_t)e * a.obs_stride : nullptr;
  float* cm = a.commands ? a.commands + (size_t)e * a.commands_stride : nullptr;

  if (a.reset[e]) {  // reset_idx (:252-254)
    if (t == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) s.local_rel_lin[e * 3 + i] = s.local_rel_rot[e * 3 + i] = 0.0f;
      o[3] = o[4] = 0.0f;
      if (oh) oh[3] = oh[4] = 0.0f;
      if (cm) cm[0] = cm[1] = 0.0f;
      // the reference planned at the pre-reset pose and dropped the result; its bookkeeping survives
      const int pl = s.plan_length[e] + 1;
      const bool replan = pl % c.plan_interval == 0;
      s.plan_length[e] = (s.ep_prev[e] == 0 || (replan && s.plan_buf[e] != 0)) ? 0 : pl;
      s.replan[e] = replan;
      s.plan_buf[e] = 1;
      s.idx_prev[e] = 0;
      s.ep_prev[e] = 0;
      s.chosen[e] = GO1_PLAN_NOT_PLANNED;
    }
    return;
  }

  float root[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) root[i] = a.root[(size_t)e * 13 + i];
  int idx = s.idx_prev[e];
  idx = idx < 0 ? 0 : (idx > c.traj_length - 1 ? c.traj_length - 1 : idx);  // a corrupt state cannot index outside
  float target[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) target[i] = a.trajectory[((size_t)e * c.traj_length + idx) * 6 + i];
  const float qb[4] = {root[3], root[4], root[5], root[6]};
  const float rel_in[3] = {target[0] - root[0], target[1] - root[1], target[2] - root[2]};
  float rel_lin[3];
  quat_apply_yaw_inverse_f(qb, rel_in, rel_lin);
  const bool close = norm2_f(rel_lin[0], rel_lin[1]) < 1.0f;
  int plan_length = s.plan_length[e] + 1;
  const bool replan = plan_length % c.plan_interval == 0;
  const bool plan = a.episode_length[e] == 1 || (replan && s.plan_buf[e] != 0);
  const bool search = plan && !close;  // uniform over the workgroup
  if (!search && t != 0) return;

  int chosen = GO1_PLAN_NOT_PLANNED;
  if (plan) {
    plan_length = 0;
    chosen = GO1_PLAN_CLOSE;
  }
  if (search) {
    const int NX = c.scan_nx, NY = c.scan_ny, NP = NX * NY;
    const float* h = a.heights + (size_t)e * 2 * NP;
    for (int i = t; i < 2 * NP; i += THREADS) s_h[i] = h[i];
    if (t < NX) s_gx[t] = c.scan_x[t];
    if (t >= 64 && t - 64 < NY) s_gy[t - 64] = c.scan_y[t - 64];
    __syncthreads();
    // 1. validity of every footprint: one work item per (grid row, footprint), footprint fastest, so the lanes of a
    // wave share the row.  The test is quat_rotate_inverse_f with q = (0, 0, qz, qw), written out without the
    // products by the zero components (the same bits): x and y of the rotated point do not depend on its height, so
    // both layers share them, and a point further than the ellipsoid in x, y alone passes whatever its (finite) height.
    const float rs0 = c.robot_size[0], rs1 = c.robot_size[1], rs2 = c.robot_size[2];
    const int NF = c.n_foot;
    for (int f = t; f < NF; f += THREADS) s_valid[f] = 1;
    __syncthreads();
    for (int it = t; it < NF * NX; it += THREADS) {
      const int i = it / NF, f = it - i * NF;
      const float* fp = p.t.foot + (size_t)f * GO1_PLAN_FOOT;
      const float fx = fp[0], fy = fp[1], fz = fp[2], qz = fp[3], qw = fp[4];
      const float sc = 2.0f * (qw * qw) - 1.0f;
      const float dx = s_gx[i] - fx;
      const float a0 = dx * sc, b1 = qz * dx * qw * 2.0f;
      bool ok = true;
      for (int j = 0; j < NY && ok; ++j) {
        const float dy = s_gy[j] - fy;
        const float b0 = (0.0f - qz * dy) * qw * 2.0f;
        const float x = (a0 - b0) / rs0, y = (dy * sc - b1) / rs1;
        const float xy = fmaf(y, y, x * x);
        if (xy > 1.0001f) continue;
#pragma unroll
        for (int layer = 0; layer < 2; ++layer) {
          const float dz = s_h[layer * NP + i * NY + j] - fz;
          const float z = (dz * sc + qz * (qz * dz) * 2.0f) / rs2;
          ok = ok && sqrtf(fmaf(z, z, xy)) > 1.0f;
        }
      }
      if (!ok) s_valid[f] = 0;  // lanes of several rows may write the same 0
    }
    __syncthreads();
    // 2. the valid candidate with the smallest (key, index)
    const float gx = target[0] - root[0], gy = target[1] - root[1];
    float bk = INFINITY;
    int bi = INT32_MAX;
    for (int k = t; k < c.n_cand; k += THREADS) {
      if (!s_valid[(unsigned)p.t.cand_foot[k] % GO1_PLAN_MAX_CAND]) continue;
      const float key = norm2_f(p.t.cand[(size_t)k * 6] - gx, p.t.cand[(size_t)k * 6 + 1] - gy) + p.t.key_rot[k];
      if (better(key, k, bk, bi)) { bk = key; bi = k; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float okey = __shfl_xor(bk, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (better(okey, oi, bk, bi)) { bk = okey; bi = oi; }
    }
    if ((t & 63) == 0) { s_key[t >> 6] = bk; s_idx[t >> 6] = bi; }
    __syncthreads();
    if (t != 0) return;
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
      if (better(s_key[w], s_idx[w], bk, bi)) { bk = s_key[w]; bi = s_idx[w]; }
    chosen = bi == INT32_MAX ? GO1_PLAN_NONE_VALID : bi;
    if (chosen == GO1_PLAN_NONE_VALID) atomicAdd(s.no_valid_count, 1u);
  }

  // lane 0: the env's local target, relative poses, commands and flags
  float rpy[3];
  quat_to_rpy_f(qb, rpy);
  float lt[6];
  if (chosen >= 0) {
    float cand[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) cand[i] = p.t.cand[(size_t)chosen * 6 + i];
    float w[3];
    quat_apply_yaw_f(qb, cand, w);
    lt[0] = w[0] + root[0];
    lt[1] = w[1] + root[1];
    lt[2] = cand[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) lt[3 + i] = wrap_to_pi_f(cand[3 + i] + rpy[i]);
  } else if (plan) {
#pragma unroll
    for (int i = 0; i < 6; ++i) lt[i] = target[i];
  } else {
#pragma unroll
    for (int i = 0; i < 6; ++i) lt[i] = s.local_target[(size_t)e * 6 + i];
  }
  float lin[3], rot[3];
  relative_pose(root, rpy, lt, lin, rot);
  if (plan) {
#pragma unroll
    for (int i = 0; i < 6; ++i) s.local_target[(size_t)e * 6 + i] = lt[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    s.local_rel_lin[e * 3 + i] = lin[i];
    s.local_rel_rot[e * 3 + i] = rot[i];
  }
  const float c0 = clampf(lin[0], -c.clip_obs, c.clip_obs), c1 = clampf(lin[1], -c.clip_obs, c.clip_obs);
  o[3] = c0;
  o[4] = c1;
  if (oh) { oh[3] = c0; oh[4] = c1; }
  if (cm) { cm[0] = lin[0]; cm[1] = lin[1]; }
  s.plan_buf[e] = norm2_f(lin[0], lin[1]) < c.switch_dist && fabsf(rot[2]) < c.switch_yaw;
  s.plan_length[e] = plan_length;
  s.idx_prev[e] = a.curr_pose_index[e];
  s.ep_prev[e] = a.episode_length[e];
  s.replan[e] = replan;
  s.chosen[e] = chosen;
}

}  // namespace

extern "C" {

int go1_plan_abi_version(void) { return GO1_PLAN_ABI_VERSION; }

void go1_plan_abi_sizes(int64_t out[6]) {
  out[0] = sizeof(go1_plan_config);
  out[1] = sizeof(go1_plan_tables);
  out[2] = sizeof(go1_plan_state);
  out[3] = sizeof(go1_plan_args);
  out[4] = GO1_PLAN_MAX_CAND;
  out[5] = GO1_PLAN_FOOT;
}

GO1_LAST_ERROR(go1_plan)

int go1_plan_step(const go1_plan_config* c, const go1_plan_tables* t, const go1_plan_state* s, const go1_plan_args* a,
                  void* stream) {
  if (!c || !t || !s || !a) return fail("go1_plan_step: null cfg, tables, state or args");
  if (c->n_envs < 1) return fail("go1_plan_step: n_envs must be >= 1");
  if (c->traj_length < 1 || c->traj_length > GO1_MAX_TRAJ) return fail("go1_plan_step: traj_length must be in 1 .. GO1_MAX_TRAJ");
  if (c->plan_interval < 1)
    return fail("go1_plan_step: plan_interval must be >= 1 (the reference raises NameError: ep_start, :867)");
  if (c->scan_nx < 1 || c->scan_nx > GO1_PLAN_MAX_X || c->scan_ny < 1 || c->scan_ny > GO1_PLAN_MAX_Y)
    return fail("go1_plan_step: scan_nx x scan_ny must be within 1 x 1 .. GO1_PLAN_MAX_X x GO1_PLAN_MAX_Y");
  if (c->n_cand < 1 || c->n_cand > GO1_PLAN_MAX_CAND) return fail("go1_plan_step: n_cand must be in 1 .. GO1_PLAN_MAX_CAND");
  if (c->n_foot < 1 || c->n_foot > c->n_cand) return fail("go1_plan_step: n_foot must be in 1 .. n_cand");
  for (int i = 0; i < 3; ++i)
    if (!(c->robot_size[i] > 0.0f)) return fail("go1_plan_step: robot_size must be positive");
  if (!t->cand || !t->cand_foot || !t->key_rot || !t->foot)
    return fail("go1_plan_step: tables: cand, cand_foot, key_rot and foot must be set");
  if (!s->local_target || !s->plan_buf || !s->plan_length || !s->idx_prev || !s->ep_prev || !s->local_rel_lin || !s->local_rel_rot ||
      !s->replan || !s->chosen || !s->no_valid_count)
    return fail("go1_plan_step: state: every pointer must be set");
  if (!a->root || !a->trajectory || !a->curr_pose_index || !a->episode_length || !a->reset || !a->heights || !a->obs)
    return fail("go1_plan_step: args: root, trajectory, curr_pose_index, episode_length, reset, heights and obs must be set");
  if (a->obs_stride < 5) return fail("go1_plan_step: obs_stride must be >= 5 (the commands are columns 3 and 4)");
  if (a->commands && a->commands_stride < 2) return fail("go1_plan_step: commands_stride must be >= 2");
  Params p;
  p.c = *c;
  p.t = *t;
  p.s = *s;
  p.a = *a;
  hipLaunchKernelGGL(go1_plan_step_kernel, dim3((unsigned)c->n_envs), dim3(THREADS), 0, (hipStream_t)stream, p);
  return launched("go1_plan_step");
}

}  // extern "C"
