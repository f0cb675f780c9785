/*
 * go1_dr.h -- C ABI of the MI355X after-start domain randomiser: Cfg.domain_rand.push_robots and
 * Cfg.domain_rand.randomize_rigids_after_start of the reference (legged_robot_trajectory_tracking.py: _push_robots
 * :1074-1084 called at :819, _randomize_rigid_body_props :710-732 called at :831-833 and in reset_idx :233-235; the
 * velocity env has the same lines) as one launch after each env step.
 *
 * Both change state that only the next step's physics reads, and the planes they change are per-env state the step
 * kernels load every step (root, friction, restitution), so neither needs the step kernel: it does not change.  The
 * one same-step consumer is the privileged observation (friction, restitution), which this launch rewrites.
 *
 * Conventions as go1_plan.h: caller-owned device buffers, asynchronous on the caller's stream, no allocation,
 * 0 or -1 with go1_dr_last_error(), one host thread per call site.
 *
 * go1_dr_step for env e, launched after the step kernel (all planes as the step left them), with r = reset[e] and
 * ep = episode_length[e] (0 for an env the step reset):
 *   rigid props, when rigids_after_start: if r (reset_idx :233-235) or ep % rand_interval == 0 (:822, :831-833; the
 *     set whose motors the step kernel re-randomised), each under its own randomize_* flag:
 *       payloads[e]    = u[GO1_DR_U_PAYLOAD]     * payload_range     + payload_lo      (when payloads is given)
 *       friction[e]    = u[GO1_DR_U_FRICTION]    * friction_range    + friction_lo
 *       restitution[e] = u[GO1_DR_U_RESTITUTION] * restitution_range + restitution_lo
 *     a multiply, then an add, in f32 (torch.rand(...) * (hi - lo) + lo).  The reference draws twice for an env that
 *     is due and resets in the same step; the reset's draw overwrites the other, so one draw is taken here.
 *     `payloads` is a shadow of the reference's tensor of that name: PhysX takes the body mass at creation only
 *     (:1593), so the plane the integrator reads (go1_state.payload) is never written here.
 *   privileged observation, when priv is given and the friction or restitution flag is set for a redrawn env:
 *       priv[e, 0] = clamp((friction[e]    - priv_friction_shift) * priv_friction_scale, -clip_obs, clip_obs)
 *       priv[e, 1] = clamp((restitution[e] - priv_rest_shift)     * priv_rest_scale,     -clip_obs, clip_obs)
 *     the step kernels' own expression (compute_observations runs after both call sites in the reference).
 *   pushes, when push_robots: if !r && ep % push_interval == 0,
 *       root[e, 7] = push_range * u[GO1_DR_U_PUSH_X] + push_lo, root[e, 8] likewise with GO1_DR_U_PUSH_Y
 *     (torch_rand_float(-max, max): (upper - lower) * rand + lower).  A reset env keeps the root of its reset.
 *   An env with neither is left after the loads of reset[e] and episode_length[e].
 *
 * Uniforms.  args.uniforms (n_envs, GO1_DR_U) when given (parity mode, as go1_step_args.uniforms); otherwise
 * Philox4x32-10 with key (rng_seed lo, rng_seed hi) and counter
 *       (env_id_offset + e,  GO1_DR_TAG + block,  rng_step lo,  rng_step hi),     block = slot / 4,
 * uniform = (word[slot % 4] >> 8) * 2^-24.  The step kernels and go1_reset_idx use the same key and the counter
 * (global env, block, step lo, step hi) with block < 64 (reset_idx with step = 2^62 + rng_step), so word 1 >= GO1_DR_TAG
 * keeps every draw of this library disjoint from theirs, whatever rng_step is.  A caller gives go1_dr_reset the
 * rng_step it gave go1_reset_idx and go1_dr_step the one it gave the step.
 * args.dbg_uniforms (n_envs, GO1_DR_U), optional: the uniforms of the slots an env used in this launch; rows of envs
 * without work and slots not used are left as they were.
 *
 * go1_dr_reset: the rigid-props redraw of a host reset_idx(env_ids) (:233-235) for the n_ids device int32 ids (ids
 * outside 0 .. n_envs - 1 are skipped; duplicates write the same values).  No priv write: the next step computes it.
 */
#ifndef GO1_DR_H
#define GO1_DR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1_DR_ABI_VERSION 1
#define GO1_DR_U 8                 /* uniforms per env: two Philox blocks */
#define GO1_DR_U_PAYLOAD 0         /* block 0: the rigid props */
#define GO1_DR_U_FRICTION 1
#define GO1_DR_U_RESTITUTION 2
#define GO1_DR_U_PUSH_X 4          /* block 1: the push */
#define GO1_DR_U_PUSH_Y 5
#define GO1_DR_TAG 0x44520000      /* counter word 1 = GO1_DR_TAG + block */

typedef struct go1_dr_config {
  int32_t n_envs;
  int32_t env_id_offset;           /* global id of local env 0 (go1_config.env_id_offset) */
  int32_t rand_interval;           /* >= 1 */
  int32_t push_interval;           /* >= 1 */
  int32_t rigids_after_start, push_robots;
  int32_t randomize_payload, randomize_friction, randomize_restitution;
  int32_t pad;
  float payload_range, payload_lo;          /* f32(hi - lo), f32(lo) of added_mass_range */
  float friction_range, friction_lo;
  float restitution_range, restitution_lo;
  float push_range, push_lo;                /* f32(2 max_push_vel_xy), f32(-max_push_vel_xy) */
  float priv_friction_shift, priv_friction_scale, priv_rest_shift, priv_rest_scale;
  float clip_obs;
  float pad2;
  uint64_t rng_seed;
} go1_dr_config;

typedef struct go1_dr_state {
  float* root;         /* (n_envs, 13): columns 7, 8 are written */
  float* friction;     /* (n_envs) */
  float* restitution;  /* (n_envs) */
  float* payloads;     /* (n_envs) the randomiser's own shadow, or NULL */
} go1_dr_state;

typedef struct go1_dr_args {
  const uint8_t* reset;           /* (n_envs) this step's reset output */
  const int32_t* episode_length;  /* (n_envs) */
  float* priv;                    /* (n_envs, priv_stride) this step's privileged observation, or NULL */
  int32_t priv_stride;            /* >= 2 when priv is given */
  int32_t pad;
  uint64_t rng_step;
  const float* uniforms;          /* (n_envs, GO1_DR_U) parity mode, or NULL -> Philox */
  float* dbg_uniforms;            /* (n_envs, GO1_DR_U) or NULL */
} go1_dr_args;

int go1_dr_abi_version(void);
/* sizeof go1_dr_config, go1_dr_state, go1_dr_args, GO1_DR_U */
void go1_dr_abi_sizes(int64_t out[4]);
const char* go1_dr_last_error(void);
int go1_dr_step(const go1_dr_config* cfg, const go1_dr_state* state, const go1_dr_args* args, void* stream);
int go1_dr_reset(const go1_dr_config* cfg, const go1_dr_state* state, const int32_t* ids, int32_t n_ids,
                 uint64_t rng_step, const float* uniforms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GO1_DR_H */
