// go1_vel_step.h -- the velocity-tracking step's device code: the torch-order f32 helpers of the post-physics
// section, foot_state, vel_reset_env, VArgs, go1_vel_step_kernel, and the explicit reset's kernels
// (go1_vel_reset_kernel, go1_vel_mask_kernel).  Restates VelocityTrackingEasyEnv.step + HistoryWrapper.step
// (go1_gym/envs/base/legged_robot_velocity_tracking.py, bare :N below): the actuator net (:925-964), post-physics
// (:108-154), the gait clock (:844-923), DR (:714-717), terminations (:156-166), the CoRL reward terms and command
// sums (:281-318, go1_gym/envs/rewards/corl_rewards.py), reset_idx's state part (:168-257), observations (:320-509)
// and the epilogue (:144-149).  A part of go1_velocity.hip, included after go1_device.h and go1_step_shared.h.
#pragma once
#ifndef GO1_VELOCITY_HIP
#error "include this part from go1_velocity.hip: its parts are not self-contained"
#endif
#pragma clang fp contract(off)  // pinned bit for bit to the oracle

typedef const __attribute__((address_space(4))) go1_vel_config VCfg;
#define VLAG 2  // GO1_LAG_STEPS(decimation) for decimation 4..6 (go1_vel_create checks it)
#define SQRT2_F 1.41421353816986083984f  // (float)math.sqrt(2)
#define CAT_PRONK 0
#define CAT_TROT 1
#define CAT_PACE 2
#define CAT_BOUND 3

// ---------------------------------------------------------------- f32 helpers (torch order)
__device__ __forceinline__ float sin_rn(float x) { return (float)sin((double)x); }
__device__ __forceinline__ float cos_rn(float x) { return (float)cos((double)x); }
__device__ __forceinline__ float exp_rn(float x) { return (float)exp((double)x); }
__device__ __forceinline__ float erf_rn(float x) { return (float)erf((double)x); }
// torch.distributions.Normal(0, kappa).cdf: 0.5 (1 + erf((x - 0) (1 / kappa) / sqrt(2)))
__device__ __forceinline__ float normal_cdf(float x, float inv_kappa) {
  return 0.5f * (1.0f + erf_rn((x - 0.0f) * inv_kappa / SQRT2_F));
}
__device__ __forceinline__ float norm4_f(float a, float b, float c, float d) {
  return sqrtf(fmaf(d, d, fmaf(c, c, fmaf(b, b, a * a))));
}
// isaacgym.torch_utils.quat_apply: b + w t + xyz x t, t = 2 (xyz x b)
__device__ __forceinline__ void quat_apply_f(const float* a, const float* b, float* o) {
  float t[3] = {(a[1] * b[2] - a[2] * b[1]) * 2.0f, (a[2] * b[0] - a[0] * b[2]) * 2.0f,
                (a[0] * b[1] - a[1] * b[0]) * 2.0f};
  float c[3] = {a[1] * t[2] - a[2] * t[1], a[2] * t[0] - a[0] * t[2], a[0] * t[1] - a[1] * t[0]};
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (b[i] + a[3] * t[i]) + c[i];
}
__device__ __forceinline__ void normalize4_f(float* q) {
  float n = norm4_f(q[0], q[1], q[2], q[3]);
  if (n < 1e-9f) n = 1e-9f;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = q[i] / n;
}
// quat_from_angle_axis for a unit coordinate axis (then quat_unit)
__device__ __forceinline__ void quat_from_axis_f(float angle, int axis, float* q) {
  const float th = angle / 2.0f, s = sin_rn(th), c = cos_rn(th);
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = (i == axis ? 1.0f : 0.0f) * s;
  q[3] = c;
  normalize4_f(q);
}
// isaacgym.torch_utils.quat_mul (the factored product)
__device__ __forceinline__ void quat_mul_f(const float* a, const float* b, float* o) {
  const float x1 = a[0], y1 = a[1], z1 = a[2], w1 = a[3], x2 = b[0], y2 = b[1], z2 = b[2], w2 = b[3];
  const float ww = (z1 + x1) * (x2 + y2), yy = (w1 - y1) * (w2 + z2), zz = (w1 + y1) * (w2 - z2);
  const float xx = ww + yy + zz;
  const float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
  o[3] = qq - ww + (z1 - y1) * (y2 - z2);
  o[0] = qq - xx + (x1 + w1) * (x2 + w2);
  o[1] = qq - yy + (w1 - x1) * (y2 + z2);
  o[2] = qq - zz + (z1 + y1) * (w2 - x2);
}
// the value of leg I's lane of this lane's quad (the legs of an (env, role)), DPP quad_perm broadcast
template <int I>
__device__ __forceinline__ float quad_at(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), I * 0x55, 0xF, 0xF, true));
}
// (((0 + t0) + t1) + t2) + t3: the reference's `reward = 0; for i: reward += t_i` over the four feet
__device__ __forceinline__ float quad_seq_sum(float v) {
  return (((0.0f + quad_at<0>(v)) + quad_at<1>(v)) + quad_at<2>(v)) + quad_at<3>(v);
}
// obs column without noise (noise_vec 0): v + (2u - 1) * 0 changes only a -0.0 (to +0.0 for u >= 0.5)
__device__ __forceinline__ float noise_free(float v, bool add_noise, const Rng& rng, int slot) {
  if (add_noise && v == 0.0f && signbit(v)) {
    if (rng(slot) >= 0.5f) v = 0.0f;
  }
  return v;
}

// World position and velocity of this leg's foot body origin (rigid_body_state[:, feet, 0:3 / 7:10])
// from the base state and the leg's joints: motion transforms down the chain (xm), then the foot
// offset in the calf frame (point_kin).
__device__ void foot_state(const float* root, const float* q, const float* qd, int leg, float* fp, float* fv) {
  const float sx = (leg & 2) ? -1.0f : 1.0f, sy = (leg & 1) ? -1.0f : 1.0f;
  float Rp[9], pp[3] = {root[0], root[1], root[2]}, vb[6];
  quat_to_R(root + 3, Rp);
  mat3T_vec(Rp, root + 10, vb);
  mat3T_vec(Rp, root + 7, vb + 3);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int i = 30 + 3 * j + k, sp = GO1_LEG_SIGN[i];
      o[k] = GO1_LEG_FL[i] * (sp == 0 ? 1.0f : (sp == 1 ? sx : (sp == 2 ? sy : sx * sy)));
    }
    const int ax = j == 0 ? 0 : 1;
    float sn, cn, vj[6], rw[3];
    pm_sincosf(q[j], &sn, &cn);
    xm(ax, cn, sn, offset_mask(j), o, vb, vj);
    vj[ax] += qd[j];
    mat3_vec(Rp, o, rw);
    pp[0] += rw[0]; pp[1] += rw[1]; pp[2] += rw[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) rE(ax, cn, sn, Rp + 3 * a, Rp + 3 * a);
#pragma unroll
    for (int i = 0; i < 6; ++i) vb[i] = vj[i];
  }
  point_kin(Rp, pp, vb, GO1_MODEL_F32 + 13 * 10 + 4 * 9, fp, fv);
}

// reset_idx's state part for one env, on the lane of leg `leg` (:168-257 after _resample_commands):
// _randomize_dof_props (:663-683), _reset_dofs (:966-981), _reset_root_states (:983-1019, plane: no
// custom origins).  u(slot): the env's f32 uniforms.
template <class U>
__device__ void vel_reset_env(VCfg* v, const U& u, const float* eo, int leg, float* root, float* q, float* qd,
                              float* strength, float* offset) {
  const float s = u(GO1_VEL_U_RESET_DR) * v->strength_range + v->strength_lo;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int d = leg * 3 + j;
    strength[j] = s;
    offset[j] = u(GO1_VEL_U_RESET_DR + 1 + d) * v->offset_range + v->offset_lo;
    q[j] = v->default_dof_pos[d] * (v->reset_dof_range * u(GO1_VEL_U_RESET_DOF + d) + v->reset_dof_lo);
    qd[j] = 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 13; ++i) root[i] = v->base_init_state[i];
  root[0] = root[0] + eo[0];
  root[1] = root[1] + eo[1];
  root[2] = root[2] + eo[2];
  const float yaw = v->yaw_range * u(GO1_VEL_U_RESET_YAW) + v->yaw_lo;
  quat_from_axis_f(yaw, 2, root + 3);
#pragma unroll
  for (int i = 0; i < 6; ++i) root[7 + i] = v->reset_vel_range * u(GO1_VEL_U_RESET_VEL + i) + v->reset_vel_lo;
}

// =====================================================================
//                          the fused step kernel
// =====================================================================
struct VArgs {
  go1_vel_state st;
  go1_vel_step_args a;
  const float* env_origins;
  int hist_w;      // obs_history row width (70 x history_len)
  int64_t hist_ld; // obs_history_out row stride (floats)
  // the curriculum launch's selection lists (CkRec, B = this step's resets, A = the next step's interval
  // resample, n_envs each) and their counts (B low, A high word); czero: the other slot's counts, cleared here
  // (the launch that read them has completed, stream order)
  int4* clist;
  unsigned long long* ccnt;
  unsigned long long* czero;
  int doA;
};

template <bool INJ>
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(1, 1))) void go1_vel_step_kernel(
    const go1_config* __restrict__ c_gen, const go1_vel_config* __restrict__ v_gen, VArgs K) {
  CCfg* __restrict__ c = (CCfg*)c_gen;
  VCfg* __restrict__ v = (VCfg*)v_gen;
  const go1_vel_state& st = K.st;
  const go1_vel_step_args& A = K.a;
  const int lane = threadIdx.x & 63, leg = lane & 3;
  const int role = lane >> 4, el = (lane >> 2) & 3, sub16 = 4 * role + leg;
  const bool owner = role == 0;
  const int e = blockIdx.x * SEPB + el;  // n % 16 == 0 (go1_vel_create)
  MlpFrag F;
  mlp_load(c_gen->actuator, lane, F);
  __shared__ float s_mlp[MLP_PARK_FLOATS * 64];  // the fragments across the sub-step loop (mlp_park)
  mlp_park(F, s_mlp, lane);
  const Rng rng = {A.uniforms, A.rng_seed, A.rng_step, e, e + c->env_id_offset, GO1_VEL_U_PER_ENV};
  const size_t d0 = (size_t)e * NDOF + leg * 3;
  const int NT = v->n_terms;

  // ---------------- load (the per-joint registers; J: their view for the shared sub-step loop)
  float act[3], q[3], qd[3], eh[2][3], vh[2][3], strength[3], offset[3], dflt[3], tlim[3], lag_pre[VLAG][3];
  float scaled[3], torque[3], tgt[3];
  const Joints<VLAG> J = {act, q, qd, eh, vh, strength, offset, dflt, tlim, lag_pre, scaled, torque, tgt};
  const float* lag_in = st.lag + (size_t)e * 12 * VLAG + leg * 3;
  float ldv[3], la[3], lla[3], ljpt[3], lljpt[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    act[j] = clampf(A.actions[d0 + j], -c->clip_actions, c->clip_actions);
    q[j] = st.dof_pos[d0 + j];
    qd[j] = st.dof_vel[d0 + j];
    strength[j] = st.motor_strength[d0 + j];
    offset[j] = st.motor_offset[d0 + j];
    eh[0][j] = st.pos_err_hist[(size_t)e * 24 + leg * 3 + j];
    eh[1][j] = st.pos_err_hist[(size_t)e * 24 + 12 + leg * 3 + j];
    vh[0][j] = st.vel_hist[(size_t)e * 24 + leg * 3 + j];
    vh[1][j] = st.vel_hist[(size_t)e * 24 + 12 + leg * 3 + j];
    dflt[j] = c->default_dof_pos[leg * 3 + j];
    tlim[j] = c->torque_limits[leg * 3 + j];
#pragma unroll
    for (int k = 0; k < VLAG; ++k) lag_pre[k][j] = lag_in[k * 12 + j];
    ldv[j] = st.last_dof_vel[d0 + j];
    la[j] = st.last_actions[d0 + j];
    lla[j] = st.last_last_actions[d0 + j];
    ljpt[j] = st.last_joint_pos_target[d0 + j];
    lljpt[j] = st.last_last_joint_pos_target[d0 + j];
  }
  const float friction = st.friction[e], payload = st.payload[e], restitution = st.restitution[e];
  __shared__ __attribute__((aligned(16))) float s_self[SEPB][SELF_ENV_FLOATS];  // self-collision scratch
  const float eo_pre[3] = {K.env_origins[(size_t)e * 3], K.env_origins[(size_t)e * 3 + 1],
                           K.env_origins[(size_t)e * 3 + 2]};
  const int ep_in = st.episode_length[e];
  const float gait_in = st.gait_indices[e];
  const float lc_in = st.last_contacts[(size_t)e * 4 + leg];
  // the curriculum's record of the env (category and bin before the resample), with the prologue loads
  const int cat_in = st.command_categories[e], bin_in = st.command_bins[e];
  // reward slots: lane sub16 holds slots sub16 and 16 + sub16 (command sums: NT + 5 of them, episode sums
  // NT + 1: the terms, then "total")
  const int NC = NT + GO1_VEL_SUM_EXTRA, NE = NT + 1;
  float cs[2], es[2];
  float my_scale[2];
  int my_id[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = sub16 + 16 * h;
    cs[h] = k < NC ? st.command_sums[(size_t)e * NC + k] : 0.0f;
    es[h] = k < NE ? st.episode_sums[(size_t)e * NE + k] : 0.0f;
    my_scale[h] = k < NT ? A.reward_scales[k] : 0.0f;
    my_id[h] = k < NT ? v_gen->term_ids[k] : -1;
  }
  Phys P;
  if (!INJ) phys_load_root(P, st.root + (size_t)e * 13);
  const Terr T = {nullptr, 0, 0, 1.0f, nullptr, 0, 0};  // the plane: floor z = 0, no ceiling

  // ---------------- decimation loop (:76-82): lag ring pushed per sim step (:940-942)
  float cf_raw[CF_RAW] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cf_leg[9], cf_base[3], cf_hip[3];
  step_substeps<INJ, false>(c, A, J, P, s_mlp, nullptr, T, s_self[el], cf_raw, VLAG, friction, restitution, payload, e,
                            lane, c->action_scale, c->hip_scale_reduction, leg, role, c->decimation, c->n_internal);
  // the commands are first read by the post-physics (the gait clock): loaded here, not with the prologue, so
  // that they do not occupy 15 registers through the sub-steps (the self-collision narrow phase needs them)
  float cmd[GO1_VEL_NUM_COMMANDS];
#pragma unroll
  for (int k = 0; k < GO1_VEL_NUM_COMMANDS; ++k) cmd[k] = st.commands[(size_t)e * GO1_VEL_NUM_COMMANDS + k];
  float root[13], fp[3], fv[3];
  contact_totals<INJ>(cf_raw, A.inj_contact, e, leg, role, cf_leg, cf_base, cf_hip);
  if (INJ) {
#pragma unroll
    for (int i = 0; i < 13; ++i) root[i] = A.inj_root[(size_t)e * 13 + i];
    const float* ft = A.inj_feet + ((size_t)e * 4 + leg) * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) { fp[i] = ft[i]; fv[i] = ft[3 + i]; }
  } else {
    phys_store_root(P, root);
    foot_state(root, q, qd, leg, fp, fv);
  }
  if (A.contact_forces && owner) contact_store(A.contact_forces, e, leg, cf_leg, cf_base, cf_hip);

  // ================= post_physics_step (:108-154), contraction off =================
  const int ep = ep_in + 1;
  float blv[3], bav[3], pg[3];
  {
    const float qb[4] = {root[3], root[4], root[5], root[6]};
    quat_rotate_inverse_f(qb, root + 7, blv);
    quat_rotate_inverse_f(qb, root + 10, bav);
    quat_rotate_inverse_f(qb, A.gravity_vec, pg);
  }
  // ---- _step_contact_targets (:844-923): this lane's foot
  const float gait = remainder_f(gait_in + v->dt * cmd[4], 1.0f);
  float fi_raw;
  {
    const float ph = cmd[5], off = cmd[6], bnd = cmd[7];
    const float f0 = ((gait + ph) + off) + bnd, f1 = gait + off, f2_ = gait + bnd, f3 = gait + ph;
    fi_raw = sel4(leg, f0, f1, f2_, f3);  // (bit-test selects: an equality chain on leg compiles to a switch)
  }
  const float foot_idx = remainder_f(fi_raw, 1.0f);  // self.foot_indices
  float fiw = fi_raw;
  {
    const float dur = cmd[8], r = remainder_f(fi_raw, 1.0f);
    if (r < dur) fiw = r * (0.5f / dur);
    else if (r > dur) fiw = 0.5f + (r - dur) * (0.5f / (1.0f - dur));
  }
  const float clock = sin_rn(TWO_PI_F * fiw);
  float desired;
  {
    const float ik = 1.0f / v->kappa_gait_probs, r = remainder_f(fiw, 1.0f);
    desired = normal_cdf(r, ik) * (1.0f - normal_cdf(r - 0.5f, ik)) +
              normal_cdf(r - 1.0f, ik) * (1.0f - normal_cdf((r - 0.5f) - 1.0f, ik));
  }
  if (A.dbg_gait && owner) {
    float* g = A.dbg_gait + (size_t)e * 12;
    g[leg] = foot_idx;
    g[4 + leg] = clock;
    g[8 + leg] = desired;
  }
  // ---- DR every rand_interval (:714-717)
  // slots 2 .. 14 = Philox blocks 0 .. 3, staged through LDS (rng_stage)
  __shared__ float s_u[SEPB][48];
  const bool dr_step = ep % v->rand_interval == 0;
  if (dr_step) {
    rng_stage(rng, 0, 4, sub16, s_u[el]);
    const float sv = s_u[el][GO1_VEL_U_DR] * v->strength_range + v->strength_lo;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      strength[j] = sv;
      offset[j] = s_u[el][GO1_VEL_U_DR + 1 + leg * 3 + j] * v->offset_range + v->offset_lo;
    }
  }
  // ---- check_termination (:156-166): base contact, time-out, body height (measured_heights = 0 on a plane)
  const bool time_out = (float)ep > v->max_episode_length;
  bool reset = norm3_f(cf_base[0], cf_base[1], cf_base[2]) > 1.0f || time_out;
  if (v->use_terminal_body_height && root[2] < v->terminal_body_height) reset = true;
  bool diverged = false;
  if (!INJ) {  // the env is reset, its rewards zeroed
    diverged = state_diverged(root, q, qd);
    if (diverged) reset = true;
  }

  // ---- compute_reward (:281-318): CoRLRewards terms filed by id in an LDS row per env
  __shared__ float s_terms[SEPB][GO1_VT_COUNT];
#define PUT(id, val)                           \
  do {                                         \
    const float v_ = (val);                    \
    if (sub16 == 0) s_terms[el][(id)] = v_;    \
  } while (0)
  auto sum12 = [](const float* x) { return qsum((x[0] + x[1]) + x[2]); };
  {
    const float d0_ = cmd[0] - blv[0], d1_ = cmd[1] - blv[1];
    PUT(GO1_VT_TRACKING_LIN_VEL, exp_rn(-(d0_ * d0_ + d1_ * d1_) / v->tracking_sigma));
    const float dz = cmd[2] - bav[2];
    PUT(GO1_VT_TRACKING_ANG_VEL, exp_rn(-(dz * dz) / v->tracking_sigma_yaw));
  }
  PUT(GO1_VT_LIN_VEL_Z, blv[2] * blv[2]);
  PUT(GO1_VT_ANG_VEL_XY, bav[0] * bav[0] + bav[1] * bav[1]);
  PUT(GO1_VT_ORIENTATION, pg[0] * pg[0] + pg[1] * pg[1]);
  {
    float x[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = torque[j] * torque[j];
    PUT(GO1_VT_TORQUES, sum12(x));
#pragma unroll
    for (int j = 0; j < 3; ++j) x[j] = qd[j] * qd[j];
    PUT(GO1_VT_DOF_VEL, sum12(x));
#pragma unroll
    for (int j = 0; j < 3; ++j) { const float a = (ldv[j] - qd[j]) / v->dt; x[j] = a * a; }
    PUT(GO1_VT_DOF_ACC, sum12(x));
#pragma unroll
    for (int j = 0; j < 3; ++j) { const float a = la[j] - act[j]; x[j] = a * a; }
    PUT(GO1_VT_ACTION_RATE, sum12(x));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int d = leg * 3 + j;
      const float lo = fminf(q[j] - v->dof_pos_limits[2 * d], 0.0f);
      const float hi = fmaxf(q[j] - v->dof_pos_limits[2 * d + 1], 0.0f);
      x[j] = -lo + hi;
    }
    PUT(GO1_VT_DOF_POS_LIMITS, sum12(x));
#pragma unroll
    for (int j = 0; j < 3; ++j) { const float a = q[j] - v->default_dof_pos[leg * 3 + j]; x[j] = a * a; }
    PUT(GO1_VT_DOF_POS, sum12(x));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float a = tgt[j] - ljpt[j];
      x[j] = (a * a) * (la[j] != 0.0f ? 1.0f : 0.0f);
    }
    PUT(GO1_VT_ACTION_SMOOTHNESS_1, sum12(x));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float a = tgt[j] - 2.0f * ljpt[j] + lljpt[j];
      x[j] = ((a * a) * (la[j] != 0.0f ? 1.0f : 0.0f)) * (lla[j] != 0.0f ? 1.0f : 0.0f);
    }
    PUT(GO1_VT_ACTION_SMOOTHNESS_2, sum12(x));
  }
  {  // collision on thighs and calves (penalize_contacts_on): integer counts, exact in any order
    const float th = norm3_f(cf_leg[0], cf_leg[1], cf_leg[2]) > 0.1f ? 1.0f : 0.0f;
    const float ca = norm3_f(cf_leg[3], cf_leg[4], cf_leg[5]) > 0.1f ? 1.0f : 0.0f;
    PUT(GO1_VT_COLLISION, qsum(th) + qsum(ca));
  }
  {
    const float d = root[2] - (cmd[3] + v->base_height_target);
    PUT(GO1_VT_JUMP, -(d * d));
  }
  {
    const float ff = norm3_f(cf_leg[6], cf_leg[7], cf_leg[8]);
    const float tf = -(1.0f - desired) * (1.0f - exp_rn(-1.0f * (ff * ff) / v->gait_force_sigma));
    PUT(GO1_VT_TRACKING_CONTACTS_SHAPED_FORCE, quad_seq_sum(tf) / 4.0f);
    const float vv = norm3_f(fv[0], fv[1], fv[2]);
    const float tv = -(desired * (1.0f - exp_rn(-1.0f * (vv * vv) / v->gait_vel_sigma)));
    PUT(GO1_VT_TRACKING_CONTACTS_SHAPED_VEL, quad_seq_sum(tv) / 4.0f);
  }
  // feet_slip (corl:107-113) updates last_contacts when it is evaluated
  const bool slip_live = [&] {
    bool l = false;
    for (int k = 0; k < NT; ++k) l = l || v->term_ids[k] == GO1_VT_FEET_SLIP;
    return l;
  }();
  const bool contact = cf_leg[8] > 1.0f;
  {
    const bool filt = contact || lc_in != 0.0f;
    const float sp = norm2_f(fv[0], fv[1]);
    PUT(GO1_VT_FEET_SLIP, qsum((filt ? 1.0f : 0.0f) * (sp * sp)));
  }
  {  // feet_clearance_cmd_linear (corl:130-135)
    const float phs = 1.0f - fabsf(1.0f - clampf(foot_idx * 2.0f - 1.0f, 0.0f, 1.0f) * 2.0f);
    const float th = cmd[9] * phs + 0.02f;
    const float d = th - fp[2];
    PUT(GO1_VT_FEET_CLEARANCE_CMD_LINEAR, qsum((d * d) * (1.0f - desired)));
  }
  {  // orientation_control (corl:181-193)
    float qr[4], qp[4], dq[4], dpg[3];
    quat_from_axis_f(-cmd[11], 0, qr);
    quat_from_axis_f(-cmd[10], 1, qp);
    quat_mul_f(qr, qp, dq);
    quat_rotate_inverse_f(dq, A.gravity_vec_after, dpg);
    const float a = pg[0] - dpg[0], b = pg[1] - dpg[1];
    PUT(GO1_VT_ORIENTATION_CONTROL, a * a + b * b);
  }
  {  // raibert_heuristic (corl:195-237)
    const float rel[3] = {fp[0] - root[0], fp[1] - root[1], fp[2] - root[2]};
    float qy[4] = {0.0f, 0.0f, -root[5], root[6]};  // quat_apply_yaw(quat_conjugate(base_quat), .)
    normalize4_f(qy);
    float fb[3];
    quat_apply_f(qy, rel, fb);
    const float w = cmd[12], ln = cmd[13];
    const float ys = (leg & 1) ? -w / 2.0f : w / 2.0f;
    const float xs = (leg & 2) ? -ln / 2.0f : ln / 2.0f;
    const float phs = fabsf(1.0f - foot_idx * 2.0f) * 1.0f - 0.5f;
    const float freq = cmd[4];
    const float y_vel = cmd[2] * ln / 2.0f;
    float yo = phs * y_vel * (0.5f / freq);
    if (leg >= 2) yo = yo * -1.0f;
    const float xo = phs * cmd[0] * (0.5f / freq);
    const float ex = fabsf((xs + xo) - fb[0]), ey = fabsf((ys + yo) - fb[1]);
    PUT(GO1_VT_RAIBERT_HEURISTIC, qsum(ex * ex + ey * ey));
  }
#undef PUT
  // slot order (:289-301): rew += term * scale; pos / neg by the slot's fixed sign; episode and
  // command sums per slot lane
  __shared__ float s_r[SEPB][GO1_VEL_MAX_TERMS];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = sub16 + 16 * h;
    if (k < NT) {
      float t = s_terms[el][my_id[h]];
      if (diverged) t = 0.0f;
      if (A.dbg_terms) A.dbg_terms[(size_t)e * GO1_VEL_MAX_TERMS + k] = t;
      const float r = t * my_scale[h];
      s_r[el][k] = r;
      es[h] = es[h] + r;
      const bool shaped = my_id[h] == GO1_VT_TRACKING_CONTACTS_SHAPED_FORCE ||
                          my_id[h] == GO1_VT_TRACKING_CONTACTS_SHAPED_VEL;
      cs[h] = cs[h] + (shaped ? my_scale[h] + r : r);
    }
  }
  float rew = 0.0f, pos = 0.0f, neg = 0.0f;
  {
    const uint32_t np = v->nonpos_slots;
    for (int k = 0; k < NT; ++k) {
      const float r = s_r[el][k];
      rew = rew + r;
      if ((np >> k) & 1u) neg = neg + r; else pos = pos + r;
    }
  }
  if (v->reward_mode == 1) rew = rew < 0.0f ? 0.0f : rew;
  else if (v->reward_mode == 2) rew = pos * exp_rn(neg / v->sigma_rew_neg);
  if (diverged) rew = 0.0f;
  // episode_sums["total"] (:306) and the command-sum extras (:314-318)
  {
    const float rx = blv[0] - cmd[0], rz = bav[2] - cmd[2];
    const float extra[GO1_VEL_SUM_EXTRA] = {blv[0], bav[2], rx * rx, rz * rz, 1.0f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = sub16 + 16 * h;
      if (k == NT) es[h] = es[h] + rew;
      if (k >= NT && k < NC && !diverged) cs[h] = cs[h] + extra[min(max(k - NT, 0), GO1_VEL_SUM_EXTRA - 1)];
    }
  }

  // ---- reset_idx (:168-257) state part; the commands are resampled by the curriculum launch
  float lla_out[3], la_obs[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { la_obs[j] = la[j]; }
  float gait_out = gait;
  if (A.episode_log_count) {
    const int row = wave_alloc_row(reset && owner && leg == 0, A.episode_log_count, lane, 4 * el);
    if (reset && A.episode_log_cap > 0) {  // a ring: the newest rows overwrite the oldest
      float* lg = A.episode_log + (size_t)((uint32_t)row % (uint32_t)A.episode_log_cap) * (NE + 2);
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (sub16 + 16 * h < NE) lg[sub16 + 16 * h] = es[h];
      if (sub16 == 0) { lg[NE] = __int_as_float(A.episode_log_tag); lg[NE + 1] = (float)e; }
    }
  }
  if (reset) {
    __shared__ float s_ru[SEPB][48];
    rng_stage(rng, 3, 12, sub16, s_ru[el]);  // the reset's uniforms (slots 12 .. 59 = Philox blocks 3 .. 14)
    const float* ru = s_ru[el];
    auto u = [ru](int slot) { return ru[slot - 12]; };
    vel_reset_env(v, u, eo_pre, leg, root, q, qd, strength, offset);
#pragma unroll
    for (int j = 0; j < 3; ++j) la_obs[j] = 0.0f;
    gait_out = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) es[h] = 0.0f;
    if (diverged) {  // observe the post-reset pose; clear the actuator-net history of the diverged state
      const float qb[4] = {root[3], root[4], root[5], root[6]};
      quat_rotate_inverse_f(qb, A.gravity_vec, pg);
#pragma unroll
      for (int j = 0; j < 3; ++j) eh[0][j] = eh[1][j] = vh[0][j] = vh[1][j] = 0.0f;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) lla_out[j] = la_obs[j];  // epilogue: last_last_actions <- last_actions

  // ---- compute_observations (:320-509): role r < 3 writes joint r's four columns, role 3 leg l the
  // gravity component l (l < 3), commands l, l + 4, l + 8, l + 12 and the clock of foot l
  float* o = A.obs + (size_t)e * GO1_VEL_NUM_OBS;
  float* oh = A.obs_history_out ? A.obs_history_out + (size_t)e * K.hist_ld + (K.hist_w - GO1_VEL_NUM_OBS) : nullptr;
  const float clip = v->clip_obs;
  const bool noisy = v->add_noise != 0;
  auto put = [&](int i, float val) {
    val = clampf(val, -clip, clip);
    o[i] = val;
    if (oh) oh[i] = val;
  };
  auto noise = [&](float val, int i, float u) { return noisy ? val + (2.0f * u - 1.0f) * v->noise_vec[i] : val; };
  // the noisy columns' uniforms (gravity 0 .. 2, dof pos 18 .. 29, dof vel 30 .. 41: slots 47 .. 88 =
  // Philox blocks 11 .. 22), staged through LDS
  float uq = 0.0f, uv = 0.0f, ugr = 0.0f;
  if (noisy) {
    rng_stage(rng, 11, 12, sub16, s_u[el]);
    const int d = leg * 3 + (role < 3 ? role : 0);
    uq = s_u[el][GO1_VEL_U_NOISE + 18 + d - 44];
    uv = s_u[el][GO1_VEL_U_NOISE + 30 + d - 44];
    ugr = s_u[el][GO1_VEL_U_NOISE + (leg < 3 ? leg : 0) - 44];
  }
  static_assert(GO1_VEL_U_NOISE == 47 && GO1_VEL_U_DR + 13 <= 16, "the shared noise / DR Philox blocks");
  if (role < 3) {
    const int j = role, d = leg * 3 + j;
    const float qj = sel3(j, q), qdj = sel3(j, qd), aj = sel3(j, act), lj = sel3(j, la_obs);
    put(18 + d, noise((qj - v->default_dof_pos[d]) * v->obs_scale_dof_pos, 18 + d, uq));
    put(30 + d, noise(qdj * v->obs_scale_dof_vel, 30 + d, uv));
    put(42 + d, noise_free(aj, noisy, rng, GO1_VEL_U_NOISE + 42 + d));
    put(54 + d, noise_free(lj, noisy, rng, GO1_VEL_U_NOISE + 54 + d));
  } else {
    if (leg < 3) {
      const float g = sel3(leg, pg);
      put(leg, noise(g, leg, ugr));
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int k = leg + 4 * m;
      if (k < GO1_VEL_NUM_COMMANDS) {
        const float ck = sel4(leg, cmd[4 * m], cmd[4 * m + 1], cmd[4 * m + 2], cmd[4 * m + 3 < 15 ? 4 * m + 3 : 14]);
        put(3 + k, noise_free(ck * v->cmd_scale[k], noisy, rng, GO1_VEL_U_NOISE + 3 + k));
      }
    }
    put(66 + leg, noise_free(clock, noisy, rng, GO1_VEL_U_NOISE + 66 + leg));
  }
  if (sub16 == 0) {
    float* pv = A.priv + (size_t)e * 2;
    pv[0] = clampf((friction - v->priv_friction_shift) * v->priv_friction_scale, -clip, clip);
    pv[1] = clampf((restitution - v->priv_rest_shift) * v->priv_rest_scale, -clip, clip);
  }
  if (A.aux) {
    float* ax = A.aux + (size_t)e * GO1_VEL_AUX;
    if (role == 3 && leg == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) { ax[i] = blv[i]; ax[3 + i] = bav[i]; }
    }
    if (role == 1) {
#pragma unroll
      for (int i = 0; i < 3; ++i) ax[6 + leg * 3 + i] = fp[i];
    }
    if (owner) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        ax[18 + leg * 3 + i] = torque[i];
        ax[30 + leg * 3 + i] = tgt[i];
      }
    }
  }

  // ---- the curriculum launch's selection lists.  A record per selected env: (env, category, bin, success)
  // -- RewardThresholdCurriculum.update's inputs (:736-757, curriculum.py:135-154) over this step's command
  // sums -- so the curriculum's workgroups never read the command state they rewrite (a late
  // workgroup counting after another one's sampling).  B: this step's resets (:168 -> :182); A: the next
  // step's interval resample, (episode_length + 1) % resample_interval == 0 (:702-704).  One 64-bit atomic per
  // wave with a selected env; the lists are in atomic order (the curriculum's results do not depend on it).
  if (K.clist) {
    bool fail = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < v->n_task) {
        const int slot = v->task_slot[k];
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (sub16 + 16 * h == slot && !(cs[h] / v->curriculum_ep_len > v->task_threshold[k])) fail = true;
      }
    }
    const uint64_t fails = __ballot(fail);
    const bool ok = ((fails >> (4 * el)) & 0x000F000F000F000Full) == 0ull;
    const bool lead = lane == 4 * el;  // role 0, leg 0 of the env
    const int ep_out = reset ? 0 : ep;
    const bool selB = lead && reset, selA = lead && K.doA && (ep_out + 1) % v->resample_interval == 0;
    const uint64_t mB = __ballot(selB), mA = __ballot(selA);
    if ((mB | mA) != 0ull) {
      unsigned long long base = 0ull;
      if (lane == 0)
        base = atomicAdd(K.ccnt, (unsigned long long)__popcll(mB) | ((unsigned long long)__popcll(mA) << 32));
      const uint32_t bB = (uint32_t)__shfl((int)(uint32_t)base, 0), bA = (uint32_t)__shfl((int)(uint32_t)(base >> 32), 0);
      const uint64_t below = (1ull << lane) - 1ull;
      const int4 rec = make_int4(e, cat_in, bin_in, ok ? 1 : 0);
      if (selB) K.clist[bB + __popcll(mB & below)] = rec;
      if (selA) K.clist[(size_t)c->n_envs + bA + __popcll(mA & below)] = rec;
    }
    if (blockIdx.x == 0 && lane == 0) *K.czero = 0ull;
  }

  // ---------------- write back (epilogue :144-149)
  if (role < 3) {
    const int j = role;
    const size_t dj = d0 + j;
    st.dof_pos[dj] = sel3(j, q);
    st.dof_vel[dj] = sel3(j, qd);
    st.last_dof_vel[dj] = sel3(j, qd);
    st.last_actions[dj] = sel3(j, act);
    st.last_last_actions[dj] = sel3(j, lla_out);
    st.last_last_joint_pos_target[dj] = sel3(j, ljpt);
    st.last_joint_pos_target[dj] = sel3(j, tgt);
    if (reset || dr_step) {
      st.motor_strength[dj] = sel3(j, strength);
      st.motor_offset[dj] = sel3(j, offset);
    }
#pragma unroll
    for (int k = 0; k < VLAG; ++k)
      st.lag[(size_t)e * 12 * VLAG + k * 12 + leg * 3 + j] =
          reset ? 0.0f : (k == VLAG - 1 ? sel3(j, scaled) : sel3(j, lag_pre[k + 1 < VLAG ? k + 1 : k]));
    st.pos_err_hist[(size_t)e * 24 + leg * 3 + j] = sel3(j, eh[0]);
    st.pos_err_hist[(size_t)e * 24 + 12 + leg * 3 + j] = sel3(j, eh[1]);
    st.vel_hist[(size_t)e * 24 + leg * 3 + j] = sel3(j, vh[0]);
    st.vel_hist[(size_t)e * 24 + 12 + leg * 3 + j] = sel3(j, vh[1]);
  }
  if (role == 3 && slip_live) st.last_contacts[(size_t)e * 4 + leg] = contact ? 1.0f : 0.0f;
  if (role == 3 && leg == 0) {
#pragma unroll
    for (int i = 0; i < 13; ++i) st.root[(size_t)e * 13 + i] = root[i];
    st.episode_length[e] = reset ? 0 : ep;
    st.gait_indices[e] = gait_out;
    A.rew[e] = rew;
    A.reset[e] = reset;
    A.time_out[e] = time_out;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = sub16 + 16 * h;
    if (k < NC) st.command_sums[(size_t)e * NC + k] = cs[h];
    if (k < NE) st.episode_sums[(size_t)e * NE + k] = es[h];
  }
}

// explicit reset_idx(ids) state part (4 lanes per env, one per leg)
__global__ __launch_bounds__(TPB) void go1_vel_reset_kernel(const go1_vel_config* __restrict__ v_gen,
                                                            go1_vel_state st, const float* __restrict__ env_origins,
                                                            const int32_t* __restrict__ ids, int n_ids, int n_envs,
                                                            const float* __restrict__ U, uint64_t seed, uint64_t step,
                                                            int env_id_offset, float* episode_log,
                                                            int32_t* episode_log_count, int episode_log_cap,
                                                            int episode_log_tag) {
  VCfg* __restrict__ v = (VCfg*)v_gen;
  const int leg = threadIdx.x & 3;
  const int slot = blockIdx.x * EPB + (threadIdx.x >> 2);
  if (slot >= n_ids) return;
  const int e = ids[slot];
  if (e < 0 || e >= n_envs) return;
  const Rng rng = {U, seed, step, e, e + env_id_offset, GO1_VEL_U_PER_ENV};
  const int NE = v->n_terms + 1;
  if (leg == 0) {  // the episode log (:199-205) reads the sums, then reset_idx clears them
    if (episode_log_count) {
      const int row = atomicAdd(episode_log_count, 1);
      if (episode_log_cap > 0) {
        float* lg = episode_log + (size_t)((uint32_t)row % (uint32_t)episode_log_cap) * (NE + 2);
        for (int k = 0; k < NE; ++k) lg[k] = st.episode_sums[(size_t)e * NE + k];
        lg[NE] = __int_as_float(episode_log_tag);
        lg[NE + 1] = (float)e;
      }
    }
    for (int k = 0; k < NE; ++k) st.episode_sums[(size_t)e * NE + k] = 0.0f;
  }
  float root[13], q[3], qd[3], strength[3], offset[3];
  const float eo[3] = {env_origins[(size_t)e * 3], env_origins[(size_t)e * 3 + 1], env_origins[(size_t)e * 3 + 2]};
  vel_reset_env(v, rng, eo, leg, root, q, qd, strength, offset);
  joints_store_reset(st, e, leg, VLAG, q, qd, strength, offset);
#pragma unroll
  for (int j = 0; j < 3; ++j) st.last_last_actions[(size_t)e * NDOF + leg * 3 + j] = 0.0f;
  if (leg == 0) {
#pragma unroll
    for (int i = 0; i < 13; ++i) st.root[(size_t)e * 13 + i] = root[i];
    st.episode_length[e] = 0;
    st.gait_indices[e] = 0.0f;
  }
}

__global__ void go1_vel_mask_kernel(const int32_t* __restrict__ ids, int n_ids, int n, uint8_t* __restrict__ m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_ids && ids[i] >= 0 && ids[i] < n) m[ids[i]] = 1;
}
