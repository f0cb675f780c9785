/*
 * go1_priv.h -- C ABI of the MI355X privileged-observation assembler: the `build privileged obs` block of the
 * reference's compute_observations (legged_robot_trajectory_tracking.py:477-590) with the clip of step (:108-111), for
 * any set of Cfg.env.priv_observe_* flags, as one launch after each env step.
 *
 * The step kernel writes the two columns every Cfg of the README run has (friction, restitution) at a row stride of
 * GO1_NUM_PRIV and is not changed.  Every other column is a state plane or a host value the step leaves behind, so the
 * wider vector needs neither the step kernel nor its ABI: the host turns the flags into a column table once
 * (privileged.py), and this launch fills the (n_envs, width) output from the table.
 *
 * Conventions as go1_dr.h: caller-owned device buffers, asynchronous on the caller's stream, no allocation,
 * 0 or -1 with go1_priv_last_error(), one host thread per call site.
 *
 * go1_priv_step, for env e and column c with t = cols[c]:
 *       x = 0                                     t.src == GO1_PRIV_SRC_ZERO
 *       x = gravities[t.comp]                     t.src == GO1_PRIV_SRC_GRAVITY   (one global value, by value)
 *       x = plane[e * plane_stride + t.comp]      otherwise (the plane and the stride of t.src in go1_priv_args)
 *       y = (x - t.shift) * t.scale               t.op == GO1_PRIV_OP_MUL   (a subtraction, then a multiply, in f32)
 *       y = (x - t.shift) / t.scale               t.op == GO1_PRIV_OP_DIV   (the correctly rounded f32 division)
 *       y = x                                     t.op == GO1_PRIV_OP_RAW
 *       out[e * width + c] = y < -clip_obs ? -clip_obs : (y > clip_obs ? clip_obs : y)       (the step kernels' clampf)
 * shift and scale are the reference's get_scale_shift values, computed in double and rounded to f32 once by the
 * caller.  Every element of out is written by every launch; nothing outside it and no plane is written.
 *
 * args.table is the device copy of cfg.cols[0 .. width): the table is constant for an env's life, so the caller
 * uploads it once; a workgroup stages it in LDS.  cfg.cols itself is read on the host only (the checks below).
 *
 * Refused with a message before any launch: n_envs < 0, width outside 1 .. GO1_PRIV_MAX_COLS, n_envs * width beyond
 * 2^31 - 1, a clip_obs that is negative or NaN, a column with an unknown source or operation, a component outside its
 * plane's row (comp >= stride, 3 for the gravity), a division by a zero scale, a null plane that a column reads
 * (named in the message), a null table or output.  A null plane that no column reads is accepted.  n_envs == 0 is
 * accepted after the checks and launches nothing.
 */
#ifndef GO1_PRIV_H
#define GO1_PRIV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1_PRIV_ABI_VERSION 1
#define GO1_PRIV_MAX_COLS 48          /* the reference's full set is 45 */

#define GO1_PRIV_SRC_ZERO 0           /* com_displacements, clock_inputs, desired_contact_states: zeros in this env */
#define GO1_PRIV_SRC_FRICTION 1
#define GO1_PRIV_SRC_RESTITUTION 2
#define GO1_PRIV_SRC_PAYLOADS 3
#define GO1_PRIV_SRC_MOTOR_STRENGTH 4
#define GO1_PRIV_SRC_MOTOR_OFFSET 5
#define GO1_PRIV_SRC_ROOT 6
#define GO1_PRIV_SRC_AUX 7
#define GO1_PRIV_SRC_GRAVITY 8
#define GO1_PRIV_NUM_SRC 9

#define GO1_PRIV_OP_MUL 0
#define GO1_PRIV_OP_DIV 1
#define GO1_PRIV_OP_RAW 2

typedef struct go1_priv_col {
  int32_t src;   /* GO1_PRIV_SRC_* */
  int32_t comp;  /* column of the source's row */
  float shift;
  float scale;
  int32_t op;    /* GO1_PRIV_OP_* */
} go1_priv_col;

typedef struct go1_priv_config {
  int32_t n_envs;
  int32_t width;     /* columns of the output, 1 .. GO1_PRIV_MAX_COLS */
  float clip_obs;    /* Cfg.normalization.clip_observations */
  int32_t pad;
  go1_priv_col cols[GO1_PRIV_MAX_COLS];
} go1_priv_config;

typedef struct go1_priv_args {
  const float* friction;        /* (n_envs, friction_stride) ... each plane with its row stride in floats, or NULL */
  const float* restitution;
  const float* payloads;
  const float* motor_strength;
  const float* motor_offset;
  const float* root;
  const float* aux;
  int32_t friction_stride;
  int32_t restitution_stride;
  int32_t payloads_stride;
  int32_t motor_strength_stride;
  int32_t motor_offset_stride;
  int32_t root_stride;
  int32_t aux_stride;
  int32_t pad;
  const go1_priv_col* table;    /* device copy of cfg.cols[0 .. width) */
  float* out;                   /* (n_envs, width) */
  float gravities[3];           /* env.gravities as compute_observations of this step sees it */
  float pad2;
} go1_priv_args;

int go1_priv_abi_version(void);
/* sizeof go1_priv_col, go1_priv_config, go1_priv_args, GO1_PRIV_MAX_COLS */
void go1_priv_abi_sizes(int64_t out[4]);
const char* go1_priv_last_error(void);
int go1_priv_step(const go1_priv_config* cfg, const go1_priv_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GO1_PRIV_H */
