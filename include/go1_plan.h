/*
 * go1_plan.h -- C ABI of the MI355X local target planner: Cfg.commands.sampling_based_planning of the reference
 * (legged_robot_trajectory_tracking.py:850-921, _plan_target_pose) as one launch after each env step.
 *
 * Every plan_interval steps, and at the first step of an episode, an env picks a local target pose from a fixed
 * candidate set: the candidate nearest the goal whose robot-sized ellipsoid contains no scanned ceiling or floor
 * point.  The policy is then commanded towards the local target: the launch overwrites the commands columns (3, 4)
 * of the step's observation row.  The step kernel itself does not change; it only stores its measured heights
 * (go1_step_args.dbg_heights), which this launch reads.
 *
 * Conventions as go1_trace.h: caller-owned device buffers, asynchronous on the caller's stream, no allocation,
 * 0 or -1 with go1_plan_last_error(), one host thread per call site.
 *
 * go1_plan_step for env e, launched after the step kernel (all planes as the step left them):
 *   reset[e] != 0 (reset_idx :252-254): local_rel_lin = local_rel_rot = 0, the commands columns 0, plan_buf = 1,
 *     idx_prev = ep_prev = 0, chosen = GO1_PLAN_NOT_PLANNED.  The reference planned this env at its pre-reset pose,
 *     which the step has overwritten, and then discarded the result; what survives is the bookkeeping, kept here:
 *     plan_length += 1, replan = plan_length % plan_interval == 0, and plan_length = 0 if the env planned
 *     (ep_prev == 0, i.e. its pre-reset episode_length was 1, or replan && plan_buf).  local_target keeps its
 *     value: the env's next step has episode_length == 1, plans and overwrites it, as in the reference.
 *   otherwise, with target = trajectory[e, idx_prev[e]] (the waypoint before this step's switch, :836-844) and
 *   relative(pose) = _compute_relative_target_pose (:922-932) at the env's root:
 *     1. plan_length += 1; close = |relative(target).linear.xy| < 1
 *     2. replan = plan_length % plan_interval == 0; plan = episode_length == 1 || (replan && plan_buf)
 *     3. if plan: plan_length = 0 and
 *          close: local_target = target, chosen = GO1_PLAN_CLOSE
 *          else:  goal_xy = target.xy - root.xy (world-aligned, as the reference has it);
 *                 key(c) = |cand[c].xy - goal_xy| + key_rot[c]; c is valid when every one of the 2 nx ny points
 *                 p = (scan_x[i], scan_y[j], heights[e, layer, i, j]) - foot.xyz, rotated by the inverse of the
 *                 footprint's yaw quaternion (0, 0, qz, qw) and divided by robot_size, has a norm > 1;
 *                 chosen = the valid candidate with the smallest key, then the smallest index (the order of a
 *                 stable argsort); local_target = (yaw(root quat) cand.xyz + root.xy, cand.z,
 *                 wrap_to_pi(cand.rpy + rpy(root quat)));
 *                 none valid: local_target = target, chosen = GO1_PLAN_NONE_VALID, no_valid_count += 1
 *        else chosen = GO1_PLAN_NOT_PLANNED
 *     4. local_rel_lin, local_rel_rot = relative(local_target)
 *     5. obs[e, 3..4] = clamp(local_rel_lin.xy, +-clip_obs) (also obs_history[e, 3..4] when given);
 *        commands[e, 0..1] = local_rel_lin.xy when given
 *     6. plan_buf = |local_rel_lin.xy| < switch_dist && |local_rel_rot.yaw| < switch_yaw (:845-847)
 *     7. idx_prev = curr_pose_index[e], ep_prev = episode_length[e]
 * The footprint table holds what enters the ellipsoid test of a candidate: x, y, z and the z, w components of
 * normalize((0, 0, qz, qw)) of quat_from_euler_xyz(roll, pitch, yaw) -- quat_apply_yaw_inverse (:897) drops the
 * quaternion's x and y, so a candidate with roll and pitch both nonzero is tested at a slightly different yaw.
 */
#ifndef GO1_PLAN_H
#define GO1_PLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1_PLAN_ABI_VERSION 1
#define GO1_PLAN_MAX_CAND 4096  /* candidates (and footprints) */
#define GO1_PLAN_MAX_X 64       /* scan points along x (GO1_MAX_SCAN_X of go1_mi355x.h) */
#define GO1_PLAN_MAX_Y 32       /* scan points along y (GO1_MAX_SCAN_Y) */
#define GO1_PLAN_FOOT 8         /* floats of a footprint row: x y z qz qw 0 0 0 */

/* go1_plan_state.chosen when it is no candidate index */
#define GO1_PLAN_CLOSE (-1)        /* planned: the global target, the env is within 1 m of it */
#define GO1_PLAN_NONE_VALID (-2)   /* planned: the global target, no candidate was valid */
#define GO1_PLAN_NOT_PLANNED (-3)  /* did not plan in this step (or was reset in it) */

typedef struct go1_plan_config {
  int32_t n_envs;
  int32_t traj_length;    /* waypoints per env */
  int32_t plan_interval;  /* >= 1 */
  int32_t scan_nx, scan_ny;
  int32_t n_cand, n_foot;
  int32_t pad;
  float switch_dist, switch_yaw;
  float clip_obs;
  float robot_size[3];    /* ellipsoid semi-axes (0.3762, 0.0935, 0.114), :1212 */
  float scan_x[GO1_PLAN_MAX_X], scan_y[GO1_PLAN_MAX_Y];
} go1_plan_config;

typedef struct go1_plan_tables {
  const float* cand;         /* (n_cand, 6) x y z roll pitch yaw, base frame */
  const int32_t* cand_foot;  /* (n_cand) footprint of each candidate, in [0, n_foot) */
  const float* key_rot;      /* (n_cand) 0.1 |rpy| in f32 (:888) */
  const float* foot;         /* (n_foot, GO1_PLAN_FOOT) */
} go1_plan_tables;

typedef struct go1_plan_state {
  float* local_target;       /* (n_envs, 6) */
  uint8_t* plan_buf;         /* (n_envs) */
  int32_t* plan_length;      /* (n_envs) */
  int32_t* idx_prev;         /* (n_envs) curr_pose_index as the previous launch left it, 0 for reset envs */
  int32_t* ep_prev;          /* (n_envs) episode_length as the previous launch left it, 0 for reset envs */
  float* local_rel_lin;      /* (n_envs, 3) out */
  float* local_rel_rot;      /* (n_envs, 3) out */
  uint8_t* replan;           /* (n_envs) out */
  int32_t* chosen;           /* (n_envs) out: candidate index or GO1_PLAN_* code */
  uint32_t* no_valid_count;  /* (1) += envs that planned without a valid candidate */
} go1_plan_state;

typedef struct go1_plan_args {
  /* the step's post-step planes and outputs */
  const float* root;               /* (n_envs, 13) */
  const float* trajectory;         /* (n_envs, 6 traj_length) */
  const int32_t* curr_pose_index;  /* (n_envs) */
  const int32_t* episode_length;   /* (n_envs) */
  const uint8_t* reset;            /* (n_envs) this step's reset output */
  const float* heights;            /* (n_envs, 2, scan_nx, scan_ny): go1_step_args.dbg_heights of this step */
  float* obs;                      /* (n_envs, obs_stride): columns 3, 4 are overwritten */
  float* obs_history;              /* the history tap's copy of obs, same stride, or NULL */
  float* commands;                 /* (n_envs, commands_stride): columns 0, 1 (the aux block's commands), or NULL */
  int32_t obs_stride, commands_stride;
} go1_plan_args;

int go1_plan_abi_version(void);
/* sizeof go1_plan_config, go1_plan_tables, go1_plan_state, go1_plan_args, GO1_PLAN_MAX_CAND, GO1_PLAN_FOOT */
void go1_plan_abi_sizes(int64_t out[6]);
const char* go1_plan_last_error(void);
int go1_plan_step(const go1_plan_config* cfg, const go1_plan_tables* tables, const go1_plan_state* state,
                  const go1_plan_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GO1_PLAN_H */
