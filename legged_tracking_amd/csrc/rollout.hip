// rollout.hip -- PPO rollout kernels for MI355X (gfx950): transition recording,
// GAE and the global advantage normalisation.  C ABI in include/go1_rollout.h.
// This file is the host side (argument checks, launches, the error record); the kernels are in its parts:
// rollout_record.h, policy_full.h, policy_split.h, rollout_colsum.h.
//
// Reference (go1_gym_learn/ppo_cse):
//   go1_record_transition <- RolloutStorage.add_transitions  rollout_storage.py:57-71
//                            + PPO.process_env_step bootstrap  ppo.py:79-92
//   go1_gae               <- RolloutStorage.compute_returns   rollout_storage.py:76-87
//   go1_adv_normalize     <- rollout_storage.py:89-90 (mean / std over every rank's samples)
//
// The GAE recursion follows torch's f32 element-wise op order (no contraction:
// built with -ffp-contract=off), so returns / advantages are bit-identical to the
// reference's compute_returns; the normalisation statistics are accumulated in f64
// and may differ from torch's f32 reductions in the last ulp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/go1_rollout.h"
#include "policy_tiles.h"
#include "split_mfma.h"

#define GO1_ROLLOUT_HIP  // the parts refuse to be included on their own

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& m) {
  g_err = m;
  return code;
}

#define RT_TRY(x)                                                                 \
  do {                                                                            \
    hipError_t _e = (x);                                                          \
    if (_e != hipSuccess) return fail(GO1_RT_E_HIP, hipGetErrorString(_e));       \
  } while (0)

// The kernels, in the parts below.  Policy inference: the building blocks (activation planes, tile loops, Normal
// draw, f32 layers) are in policy_tiles.h; policy_full.h has policy_kernel and policy_split.h policy_kernel_split,
// the two launch shapes of GO1_POLICY_FULL, and policy_kernel_split_teacher; the single-workgroup kernels of
// GO1_POLICY_STUDENT / TEACHER are in policy_actor.hip.
#include "rollout_record.h"  // gae_kernel, adv_norm_kernel, Seg, RecPlan, the two record kernels
#include "policy_full.h"     // policy_fallback, PSTAMP, policy_kernel
#include "policy_split.h"    // SPLIT_D2, SplitLds, lds_barrier, split_body, the two split kernels, SPLIT_ET_*

}  // namespace

#include "rollout_colsum.h"  // colsum_part_kernel, colsum_final_kernel

// policy_actor.hip: variant 1 of GO1_POLICY_STUDENT / TEACHER
hipError_t go1_policy_launch_actor(const go1_policy_args& P, hipStream_t stream);

// the library's error record for its other sources (encoder.hip)
int go1_rt_fail(int code, const std::string& m) { return fail(code, m); }

extern "C" {

#ifdef GO1_POLICY_STAMPS
int go1_policy_stamps(void* host, size_t bytes) {
  if (bytes > sizeof(g_pstamps)) bytes = sizeof(g_pstamps);
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_pstamps), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#endif

const char* go1_rollout_last_error(void) { return g_err.c_str(); }

int go1_rollout_abi_version(void) { return GO1_ROLLOUT_ABI_VERSION; }

void go1_rollout_abi_sizes(int64_t out[3]) {
  out[0] = sizeof(go1_transition);
  out[1] = sizeof(go1_policy_layer);
  out[2] = sizeof(go1_policy_args);
}

int go1_record_transition(const go1_transition* tr, int32_t n_envs, float gamma, void* stream) {
  if (!tr || n_envs <= 0) return fail(GO1_RT_E_ARG, "go1_record_transition: bad argument");
  if (!tr->rewards || !tr->dones || !tr->values || !tr->st_rewards || !tr->st_dones || !tr->st_values)
    return fail(GO1_RT_E_ARG, "go1_record_transition: rewards / dones / values are required");
  if (tr->obs_history && tr->obs_history_ld != 0 && tr->obs_history_ld < tr->num_obs_history)
    return fail(GO1_RT_E_ARG, "go1_record_transition: obs_history_ld < num_obs_history");
  go1_transition T = *tr;
  if (T.obs_history_ld == 0) T.obs_history_ld = T.num_obs_history;
  {  // the flat form when every buffer is 16-byte aligned and the history contiguous
    const Seg segs[7] = {{T.obs, T.st_obs, (int64_t)n_envs * T.num_obs},
                         {T.privileged_obs, T.st_privileged_obs, (int64_t)n_envs * T.num_priv},
                         {T.obs_history, T.st_obs_history, (int64_t)n_envs * T.num_obs_history},
                         {T.actions, T.st_actions, (int64_t)n_envs * T.num_actions},
                         {T.mu, T.st_mu, (int64_t)n_envs * T.num_actions},
                         {T.sigma, T.st_sigma, (int64_t)n_envs * T.num_actions},
                         {T.actions_log_prob, T.st_actions_log_prob, (int64_t)n_envs}};
    const char* fe = std::getenv("GO1_RECORD_FLAT");  // "0": the segment-walking kernel (A/B)
    bool flat = T.obs_history_ld == T.num_obs_history && !(fe && fe[0] == '0');
    for (int i = 0; i < 7; ++i)
      if (segs[i].src && segs[i].n > 0)
        flat = flat && ((((uintptr_t)segs[i].src) | ((uintptr_t)segs[i].dst)) & 15) == 0;
    if (flat) {
      RecPlan P;
      memset(&P, 0, sizeof(P));
      const bool alias = T.obs && T.obs_history == T.obs && T.num_obs == T.num_obs_history;
      int blk = 0;
      for (int i = 0; i < 7; ++i) {
        if (!segs[i].src || segs[i].n <= 0 || (i == 2 && alias)) continue;
        const int s = P.nseg++;
        P.src[s] = reinterpret_cast<const float4*>(segs[i].src);
        P.dst[s] = reinterpret_cast<float4*>(segs[i].dst);
        P.dst2[s] = (i == 0 && alias) ? reinterpret_cast<float4*>(T.st_obs_history) : nullptr;
        P.nf[s] = segs[i].n;
        P.first[s] = blk;
        blk += (int)std::max<int64_t>(1, ((segs[i].n >> 2) + 255) / 256);
      }
      P.first[P.nseg] = blk;
      blk += (n_envs + 255) / 256;
      hipLaunchKernelGGL(record_flat_kernel, dim3(blk), dim3(256), 0, (hipStream_t)stream, P, T, n_envs, gamma);
      RT_TRY(hipGetLastError());
      return GO1_OK_RT;
    }
  }
  int64_t big = (int64_t)n_envs * (tr->num_obs + tr->num_obs_history);
  int blocks = (int)((big / 4 + 255) / 256);
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  hipLaunchKernelGGL(record_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, T, n_envs, gamma);
  RT_TRY(hipGetLastError());
  return GO1_OK_RT;
}

int go1_gae(const float* rewards, const uint8_t* dones, const float* values, const float* last_values,
            float* returns, float* advantages, double* stats, int32_t T, int32_t n_envs, float gamma, float lam,
            void* stream) {
  if (!rewards || !dones || !values || !last_values || !returns || !advantages || !stats || T <= 0 || n_envs <= 0)
    return fail(GO1_RT_E_ARG, "go1_gae: bad argument");
  hipStream_t s = (hipStream_t)stream;
  RT_TRY(hipMemsetAsync(stats, 0, 2 * sizeof(double), s));
  hipLaunchKernelGGL(gae_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, s, rewards, dones, values, last_values,
                     returns, advantages, stats, T, n_envs, gamma, lam);
  RT_TRY(hipGetLastError());
  return GO1_OK_RT;
}

int go1_policy_forward(const go1_policy_args* args, void* stream) {
  if (!args || args->n_envs <= 0 || !args->obs_history || !args->action_mean)
    return fail(GO1_RT_E_ARG, "go1_policy_forward: bad argument");
  if (args->mode != GO1_POLICY_FULL && args->mode != GO1_POLICY_STUDENT && args->mode != GO1_POLICY_TEACHER)
    return fail(GO1_RT_E_ARG, "go1_policy_forward: mode " + std::to_string(args->mode) +
                                  " is none of GO1_POLICY_FULL (0), GO1_POLICY_STUDENT (1), GO1_POLICY_TEACHER (2)");
  // the critic's inputs and output (FULL), the teacher's latent inputs
  if ((args->mode != GO1_POLICY_STUDENT && !args->privileged_obs) || (args->mode == GO1_POLICY_FULL && !args->value))
    return fail(GO1_RT_E_ARG, "go1_policy_forward: bad argument");
  if (args->actions && (!args->std || !args->action_sigma || !args->log_prob))
    return fail(GO1_RT_E_ARG, "go1_policy_forward: actions needs std, action_sigma and log_prob");
  if (args->num_priv < 1 || args->num_priv > 8 || args->hist_dim < 1 || args->num_actions > 16)
    return fail(GO1_RT_E_ARG, "go1_policy_forward: input / latent / action width outside the compiled architecture");
  {
    // variant 1 stages all inputs at once (PIN); variant 0 streams them in chunks of PIN, and the actor's
    // groups that hold the latent must lie in the last chunk (its planes receive the latent)
    const int kin = args->hist_dim + args->num_priv, gl = args->hist_dim / 32, GL = (kin + 31) / 32;
    const int g_last = (PIN / 32) * ((GL + PIN / 32 - 1) / (PIN / 32) - 1);
    // variant 1 stages all inputs at once (kin <= PIN) and walks PIN / 32 K groups of the packed first layers
    // (compile-time G): the packing (ceil(k / 32) groups per output tile) must have exactly that many, or its
    // reads leave the buffer.  Together: 257 <= hist_dim <= 288 - num_priv.
    if (args->variant == 1 && (kin > PIN || (args->hist_dim + 31) / 32 != PIN / 32))
      return fail(GO1_RT_E_ARG, "go1_policy_forward: variant 1 needs hist_dim in 257.." +
                                    std::to_string(PIN - args->num_priv) + " (288 - num_priv; 9 packed K groups), got " +
                                    std::to_string(args->hist_dim));
    if (gl < g_last || kin > 16384)
      return fail(GO1_RT_E_ARG, "go1_policy_forward: history width not supported by the chunked first layers");
  }
  for (int i = 0; i < GO1_POLICY_LAYERS; ++i)
    if (!args->layers[i].w || !args->layers[i].b || !args->layers[i].wf)
      return fail(GO1_RT_E_ARG, "go1_policy_forward: missing layer (split, bias and f32 weights are required)");
  if (args->variant != 0 && args->variant != 1) return fail(GO1_RT_E_ARG, "go1_policy_forward: variant");
  if (args->hist_ld != 0 && args->hist_ld < args->hist_dim)
    return fail(GO1_RT_E_ARG, "go1_policy_forward: hist_ld < hist_dim");
  go1_policy_args P = *args;
  if (P.hist_ld == 0) P.hist_ld = P.hist_dim;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 block(64 * PW), g16((P.n_envs + 15) / 16), ga((P.n_envs + SE_A - 1) / SE_A);
  if (P.variant == 0) {
    if (P.mode == GO1_POLICY_FULL)
      hipLaunchKernelGGL(policy_kernel_split, dim3(ga.x + (P.n_envs + SE_C - 1) / SE_C), block, 0, s, P);
    else if (P.mode == GO1_POLICY_STUDENT)  // the actor workgroups only
      hipLaunchKernelGGL(policy_kernel_split, ga, block, 0, s, P);
    else
      hipLaunchKernelGGL(policy_kernel_split_teacher, ga, block, 0, s, P);
  } else if (P.mode == GO1_POLICY_FULL) {
    hipLaunchKernelGGL(policy_kernel, g16, block, 0, s, P);
  } else {
    RT_TRY(go1_policy_launch_actor(P, s));
  }
  RT_TRY(hipGetLastError());
  return GO1_OK_RT;
}

int go1_adv_normalize(float* advantages, const double* stats, double count, int64_t total, void* stream) {
  if (!advantages || !stats || total < 0 || count < 2.0) return fail(GO1_RT_E_ARG, "go1_adv_normalize: bad argument");
  if (total == 0) return GO1_OK_RT;
  int64_t blocks = (total + 255) / 256;
  blocks = blocks > 4096 ? 4096 : blocks;
  hipLaunchKernelGGL(adv_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, advantages, stats,
                     count, (size_t)total);
  RT_TRY(hipGetLastError());
  return GO1_OK_RT;
}

int go1_colsum(const float* x, int64_t rows, int32_t cols, float* partial, int32_t parts, float* out, void* stream) {
  if (!x || !partial || !out || rows < 1 || cols < 1 || parts < 1 || parts > 65535 || parts > rows)
    return fail(GO1_RT_E_ARG, "go1_colsum: bad argument");
  const int64_t rp = (rows + parts - 1) / parts;
  hipLaunchKernelGGL(colsum_part_kernel, dim3((unsigned)((cols + 63) / 64), (unsigned)parts), dim3(256), 0,
                     (hipStream_t)stream, x, rows, cols, rp, partial);
  RT_TRY(hipGetLastError());
  hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     partial, parts, cols, out);
  RT_TRY(hipGetLastError());
  return GO1_OK_RT;
}

}  // extern "C"
