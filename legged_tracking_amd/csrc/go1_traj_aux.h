// go1_traj_aux.h -- the small kernels beside the trajectory step: go1_finalize_kernel (the extras["time_outs"]
// rebinding, legged_robot_trajectory_tracking.py:289-291), go1_reset_kernel (reset_idx, :218-296),
// go1_bucket_kernel (global pos / neg reward bucketing, :330-344) and go1_actuator_kernel (the actuator net alone).
// A part of go1_step.hip, included after go1_traj_step.h.
#pragma once
#ifndef GO1_STEP_HIP
#error "include this part from go1_step.hip: its parts are not self-contained"
#endif
#pragma clang fp contract(off)  // pinned bit for bit to the oracle

// extras["time_outs"] = time_out of the last step, if any env reset in it (go1_sync_time_outs:
// the rebinding of that step, applied on demand; idempotent).
__global__ void go1_finalize_kernel(int n, const int32_t* __restrict__ flag, const uint8_t* __restrict__ time_out,
                                    uint8_t* __restrict__ extras) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n && *flag) extras[e] = time_out[e];
}

// reset_idx (:218-296) of masked envs, or of a list of env ids (ids != nullptr: slot k of the
// list -> env ids[k]; out-of-range ids skipped)
__global__ __launch_bounds__(TPB) void go1_reset_kernel(const go1_config* __restrict__ c_gen, go1_state st,
                                                        go1_terrain ter, const uint8_t* __restrict__ mask,
                                                        const int32_t* __restrict__ ids, int n_ids,
                                                        const float* __restrict__ U, uint64_t seed, uint64_t step) {
  CCfg* __restrict__ c = (CCfg*)c_gen;
  const int leg = threadIdx.x & 3;
  const int slot = blockIdx.x * EPB + (threadIdx.x >> 2);
  int e;
  if (ids) {
    if (slot >= n_ids) return;
    e = ids[slot];
    if (e < 0 || e >= c->n_envs) return;
  } else {
    e = slot;
    if (e >= c->n_envs || !mask[e]) return;
  }
  const Rng rng = {U, seed, step, e, e + c->env_id_offset, c->u_per_env};
  float root[13], q[3], qd[3], strength[3], offset[3], traj[6];
  const float eo[3] = {ter.env_origins[(size_t)e * 3], ter.env_origins[(size_t)e * 3 + 1],
                       ter.env_origins[(size_t)e * 3 + 2]};
  reset_env(c, rng, rng, eo, leg, c_gen->default_dof_pos, root, q, qd, strength, offset, traj);
  joints_store_reset(st, e, leg, GO1_LAG_STEPS(c->decimation), q, qd, strength, offset);
  write_trajectory(c, rng, root, st.trajectory + (size_t)e * 6 * c->traj_length, leg, 4);
  st.feet_air_time[(size_t)e * 4 + leg] = 0.0f;  // (:248)
  const int ns = c->n_terms + 3;
  for (int k = leg; k < ns; k += 4) st.episode_sums[(size_t)e * ns + k] = 0.0f;
  if (leg == 0) {
#pragma unroll
    for (int i = 0; i < 13; ++i) st.root[(size_t)e * 13 + i] = root[i];
    st.episode_length[e] = 0;
    st.curr_pose_index[e] = 0;
    st.collision_count[e] = 0;
  }
  (void)traj;
}

// Global pos / neg bucketing (:330-336) when some reward slot has no fixed sign: the step kernel
// recorded every env's scaled slot rewards and their sums over envs (f64); here each env's
// rew_buf_pos / rew_buf_neg are rebuilt in slot order with the reference's bucket test on the sum's
// sign, added to total_pos / total_neg (the state's episode sums, or the episode-log row of an env
// the step reset), and the ji22-style reward is formed (:343-344).
__global__ void go1_bucket_kernel(const go1_config* __restrict__ c, go1_state st, const float* __restrict__ r_all,
                                  const double* __restrict__ bsum, double* __restrict__ bsum_next,
                                  const uint8_t* __restrict__ reset, float* __restrict__ rew,
                                  float* __restrict__ episode_log) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int nt = c->n_terms, ns = nt + 3;
  if (blockIdx.x == 0 && threadIdx.x < GO1_MAX_TERMS) bsum_next[threadIdx.x] = 0.0;
  if (e >= c->n_envs) return;
  float pos = 0.0f, neg = 0.0f;
  for (int k = 0; k < nt; ++k) {
    if (c->term_ids[k] == GO1_T_NONE) continue;
    const float r = r_all[(size_t)e * GO1_MAX_TERMS + k];
    const double S = bsum[k];
    if (S >= 0.0) pos = pos + r;
    else if (S <= 0.0) neg = neg + r;
  }
  float* t = (reset[e] && episode_log) ? episode_log + (size_t)e * (nt + 6) + nt
                                       : (reset[e] ? nullptr : st.episode_sums + (size_t)e * ns + nt);
  if (c->reward_mode == 2) {
    const float rw = pos * expf(neg / c->sigma_rew_neg);
    rew[e] = rw;
    if (t) t[0] = t[0] + rw;
  }
  if (t) {
    t[1] = t[1] + pos;
    t[2] = t[2] + neg;
  }
}

__global__ __launch_bounds__(64) void go1_actuator_kernel(const go1_config* __restrict__ c,
                                                         const float* __restrict__ x, float* __restrict__ out,
                                                         int n) {
  const int lane = threadIdx.x & 63, q = lane >> 4;
  MlpFrag F;
  mlp_load(c->actuator, lane, F);
  const int n_groups = (n + 15) / 16;
  for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {  // uniform per wave: all lanes stay active
    const int row = g * 16 + (lane & 15);
    const float* r = x + (size_t)min(row, n - 1) * 6;
    const float b0 = r[q];
    const float b1v = q < 2 ? r[4 + q] : 0.0f;
    const float t = mlp_group(F, b0, b1v);
    if (q == 0 && row < n) out[row] = t;
  }
}
