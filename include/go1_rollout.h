/*
 * go1_rollout.h -- C ABI of the MI355X PPO rollout kernels (legged_tracking_amd/csrc/rollout.hip).
 *
 * Replaces, for the rollout half of the hot path (go1_gym_learn/ppo_cse):
 *   go1_record_transition()  <- RolloutStorage.add_transitions     rollout_storage.py:57-71
 *                               + PPO.process_env_step bootstrap    ppo.py:79-92
 *   go1_gae()                <- RolloutStorage.compute_returns      rollout_storage.py:76-87
 *   go1_adv_normalize()      <- rollout_storage.py:89-90 (global normalisation; the
 *                               caller may all-reduce the 2 f64 statistics across ranks
 *                               between the two calls)
 *   go1_colsum()             <- the bias gradients of PPO.update's backward (ppo.py:155-157),
 *                               torch's grad_output.sum(0) in F.linear's backward
 *
 * All pointers are device pointers owned by the caller; every call is
 * asynchronous on the given HIP stream and returns 0 or a negative code.
 */
#ifndef GO1_ROLLOUT_H
#define GO1_ROLLOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1_ROLLOUT_ABI_VERSION 2
#define GO1_OK_RT 0
#define GO1_RT_E_ARG -1
#define GO1_RT_E_HIP -2

/* One transition (rows of n_envs) and the storage slot it goes to. */
typedef struct go1_transition {
  const float* obs;               /* (n, num_obs) */
  const float* privileged_obs;    /* (n, num_priv) */
  const float* obs_history;       /* (n, num_obs_history) */
  const float* actions;           /* (n, num_actions) */
  const float* mu;                /* (n, num_actions) action mean */
  const float* sigma;             /* (n, num_actions) action std */
  const float* actions_log_prob;  /* (n) */
  const float* values;            /* (n) */
  const float* rewards;           /* (n) env rewards before bootstrapping */
  const uint8_t* dones;           /* (n) bool */
  const uint8_t* time_outs;       /* (n) bool or NULL (no bootstrap) */
  float *st_obs, *st_privileged_obs, *st_obs_history, *st_actions, *st_mu, *st_sigma, *st_actions_log_prob;
  float *st_values, *st_rewards;
  uint8_t* st_dones;
  int32_t num_obs, num_priv, num_obs_history, num_actions;
  /* Deferred extras["time_outs"] rebinding (go1_step rebinds only on steps with a reset,
   * legged_robot_trajectory_tracking.py:289-291, and defers it, see go1_time_outs_pending):
   * when time_outs_flag is non-NULL and *time_outs_flag != 0, the time-outs of this transition
   * are time_outs_pending, and they are also copied into time_outs_dst (the env's
   * extras["time_outs"] tensor, current afterwards).  NULL = time_outs is used as is. */
  const int32_t* time_outs_flag;
  const uint8_t* time_outs_pending;
  uint8_t* time_outs_dst;
  int64_t obs_history_ld;         /* row stride of obs_history in floats (0: num_obs_history), e.g. a window of
                                     the velocity env's wider history rows (go1_velocity.h obs_history_out_ld) */
} go1_transition;

/* Fused policy inference (ActorCritic.act / evaluate, actor_critic.py:121-150) for the
 * default AC_Args architecture: adaptation 261 -> 256 -> 128 -> 2, actor
 * [hist, latent] -> 512 -> 256 -> 128 -> num_actions, critic [hist, priv] -> 512 -> 256
 * -> 128 -> 1, ELU, to f32 accuracy on f16 matrix cores (3xF16 split products, see rollout.hip).
 * Weights split and packed by legged_tracking_amd/rollout.py (fragment order,
 * layers: a1 a2 a3 p1 p2 p3 p4 c1 c2 c3 c4). */
#define GO1_POLICY_LAYERS 11
/* go1_policy_args.mode: which nets a launch runs (ABI 2).
 *   GO1_POLICY_FULL     act + evaluate: adaptation module, actor, critic
 *   GO1_POLICY_STUDENT  act_student (actor_critic.py:143-147): adaptation module + actor; no critic workgroup runs,
 *                       value may be NULL and is never written, privileged_obs may be NULL; every other output is
 *                       the bits GO1_POLICY_FULL writes for the same inputs (same Philox key and counter use)
 *   GO1_POLICY_TEACHER  act_teacher (actor_critic.py:149-152): actor_body(cat(hist, privileged_obs)); neither the
 *                       adaptation module nor the critic runs, the actor's latent inputs are the privileged
 *                       observations and `latent`, when non-NULL, receives that copy; value as in STUDENT */
#define GO1_POLICY_FULL 0
#define GO1_POLICY_STUDENT 1
#define GO1_POLICY_TEACHER 2
typedef struct go1_policy_layer {
  /* [n/16][k/32][64 lanes][16] f16 (n padded to 16, k to 32): each weight w split into hi = f16(w)
     and lo = f16(w - hi); record (t, g, lane = 16 q + m) = hi, then lo, of W[16 t + m][32 g + 8 q + r],
     r = 0..7 (32 bytes: the lane's A fragments of v_mfma_f32_16x16x32_f16 for both halves) */
  const void* w;
  const float* b;  /* [n padded to 16] */
  const float* wf; /* (n, k) row-major f32, the unsplit weights: the f32 fallback of a workgroup whose
                      activations leave the f16 split's range (|x| >= 65504) */
} go1_policy_layer;
typedef struct go1_policy_args {
  const float* obs_history;    /* (n, hist_dim) */
  const float* privileged_obs; /* (n, num_priv) */
  float* action_mean;          /* (n, num_actions) */
  float* value;                /* (n); mode != GO1_POLICY_FULL: may be NULL, never written */
  float* latent;               /* (n, num_priv) or NULL: the adaptation module's output */
  /* optional in-kernel Normal(mean, std).sample() + log_prob (NULL actions = skip) */
  const float* std;            /* (num_actions) */
  float* actions;              /* (n, num_actions) */
  float* action_sigma;         /* (n, num_actions) */
  float* log_prob;             /* (n) */
  uint64_t rng_seed, rng_step; /* Philox key / counter, one counter value per call */
  int32_t env_id_offset;       /* global id of row 0 (rank * n) */
  int32_t n_envs, hist_dim, num_actions;
  int32_t num_priv;            /* privileged obs = latent width, 1 .. 8.  variant 1: 257 <= hist_dim <= 288 - num_priv
                                  (it walks exactly nine packed K groups; anything else is GO1_RT_E_ARG);
                                  variant 0 streams the inputs in chunks of 288 (hist_dim + num_priv <= 16384,
                                  the groups of 32 that hold the latent inside the last chunk) */
  int32_t variant;             /* 0: per-net workgroups of 32 envs (default), 1: one workgroup of 16 envs
                                  running all three nets; identical outputs (tests/test_rollout.py) */
  int32_t* overflow;           /* optional: += workgroups that recomputed in f32 (the range guard) */
  go1_policy_layer layers[GO1_POLICY_LAYERS];
  int64_t hist_ld;             /* row stride of obs_history in floats (0: hist_dim; >= hist_dim) */
  int32_t mode;                /* GO1_POLICY_FULL / STUDENT / TEACHER; anything else is GO1_RT_E_ARG.  The range guard's
                                  f32 recomputation and `overflow` cover the nets the mode runs */
} go1_policy_args;

/* Height-map encoder of go1_gym_learn/ppo_cse_cnn (actor_critic.py:27-62, 180-198; csrc/encoder.hip): from the
 * LAST frame of every history row, policy_input = [scalars | scalars | embedding of the frame's height map], the
 * row go1_policy_forward then takes as its "history" (hist_dim = 2 n_scalar + n_embed).  A frame is n_scalar
 * scalars followed by the (2, map_x, map_y) map.  Same 3xF16 split products and range guard as the policy kernel.
 *   GO1_ENC_MLP: Linear(2 X Y -> n_feat) ELU Linear(n_feat -> n_embed) ELU
 *   GO1_ENC_CNN: Conv3x3(2 -> 16) ReLU MaxPool2 Conv3x3(16 -> 32) ReLU MaxPool2 Flatten Linear(n_feat -> n_embed),
 *                n_feat = 32 (X / 2 / 2) (Y / 2 / 2) with floor pooling, zero padding at the true map border
 * layers: MLP (linear 1, linear 2); CNN (conv 1, conv 2, linear).  A conv's weights are packed as the linear
 * layer [oc][ic * 9 + ky * 3 + kx] (K = 9 ic padded to 32); wf is the tensor as torch keeps it. */
#define GO1_ENCODER_LAYERS 3
#define GO1_ENC_MLP 0
#define GO1_ENC_CNN 1
#define GO1_ENC_MAX_EMBED 512
typedef struct go1_encoder_args {
  const float* obs_history;  /* (n, >= frame_off + num_obs), rows hist_ld floats apart */
  int64_t hist_ld;           /* row stride of obs_history in floats, >= frame_off + num_obs */
  int64_t frame_off;         /* column of the last frame: (H - 1) * num_obs */
  int32_t num_obs;           /* frame width = n_scalar + 2 * map_x * map_y */
  int32_t n_scalar;
  int32_t map_x, map_y;      /* 1 .. GO1_MAX_SCAN_X (64), 1 .. GO1_MAX_SCAN_Y (32) of go1_mi355x.h */
  int32_t mode;              /* GO1_ENC_MLP / GO1_ENC_CNN */
  int32_t n_embed;           /* E, 1 .. GO1_ENC_MAX_EMBED */
  int32_t n_feat;            /* K of the last linear layer: the MLP's hidden width, the CNN's flattened features */
  int32_t n_envs;
  go1_policy_layer layers[GO1_ENCODER_LAYERS];
  float* scratch;            /* (n, n_feat) f32: the MLP's hidden activations / the CNN's pooled features */
  float* policy_input;       /* (n, 2 n_scalar + n_embed), rows out_ld floats apart; rows >= n_envs are not written */
  int64_t out_ld;            /* >= 2 n_scalar + n_embed */
  int32_t* overflow;         /* optional: += workgroups that recomputed in f32 (the range guard) */
} go1_encoder_args;

int go1_heightmap_encode(const go1_encoder_args* args, void* stream);
/* sizeof(go1_policy_layer), sizeof(go1_encoder_args) */
void go1_encoder_abi_sizes(int64_t out[2]);

int go1_rollout_abi_version(void);
/* sizeof(go1_transition), sizeof(go1_policy_layer), sizeof(go1_policy_args): lets a foreign binding verify
 * its struct mirrors. */
void go1_rollout_abi_sizes(int64_t out[3]);
const char* go1_rollout_last_error(void);
int go1_policy_forward(const go1_policy_args* args, void* stream);
int go1_record_transition(const go1_transition* tr, int32_t n_envs, float gamma, void* stream);
/* rewards/values/returns/advantages: (T, n) f32; dones (T, n) u8; last_values (n);
 * stats: 2 f64 (sum, sum of squares of the raw advantages), overwritten. */
int go1_gae(const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
            float* returns, float* advantages, double* stats, int32_t T, int32_t n_envs, float gamma, float lam,
            void* stream);
/* advantages <- (a - mean) / (std + 1e-8); count = number of samples the stats cover (all ranks). */
int go1_adv_normalize(float* advantages, const double* stats, double count, int64_t total, void* stream);
/* out[c] = sum over rows of x[r][c], x row-major (rows, cols) f32, deterministic (fixed partition and order):
 * the PPO update's bias gradients (PPO.update, ppo.py:155-157 backward; torch's grad_output.sum(0)).
 * partial: scratch of parts x cols floats, 1 <= parts <= min(rows, 65535). */
int go1_colsum(const float* x, int64_t rows, int32_t cols, float* partial, int32_t parts, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GO1_ROLLOUT_H */
