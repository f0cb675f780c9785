// policy_actor.hip -- the single-workgroup policy kernel (go1_policy_args.variant 1) of the inference modes
// GO1_POLICY_STUDENT and GO1_POLICY_TEACHER (include/go1_rollout.h); go1_policy_forward (rollout.hip) launches it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "policy_tiles.h"

#define PSTAMP(k)  // the per-phase stamps are a diagnostic of the full kernels (policy_full.h, policy_split.h)

namespace {

// policy_kernel without the critic (GO1_POLICY_STUDENT), and with TEACHER also without the adaptation module, whose
// place in the actor's input the privileged observations take (GO1_POLICY_TEACHER).  A kernel of its own, in a source file of its
// own, so that policy_kernel's code is what it was without the modes (in one translation unit with it, these kernels
// changed its register allocation; policy_kernel is in policy_full.h, a part of rollout.hip).  The actor's tiles per
// wave, K order and partial-sum order are policy_kernel's, so STUDENT writes the same bits.
template <bool TEACHER>
__global__ __launch_bounds__(64 * PW) void policy_kernel_actor(go1_policy_args P) {
  __shared__ Act<PIN> xa;   // actor inputs (the adaptation module reads them first)
  __shared__ Act<512> h1;   // layer-1 outputs; layer 3 reuses them
  __shared__ Act<256> h2;   // layer-2 outputs; also the f32 scratch of the output layer's K-split partials
  __shared__ Act<256> had;  // the adaptation module's layer-2 outputs
  __shared__ float scr_ad[8][16][16];  // its K-split partials
  __shared__ int s_ovf;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int q = lane >> 4, c = lane & 15;
  const int e0 = blockIdx.x * 16;
  PSTAMP(0);
  const int ne = min(16, P.n_envs - e0);
  const int NP = P.num_priv, H = P.hist_dim;
  const ActV va = xa.v();
  if (tid == 0) s_ovf = 0;
  f8_t w_ad[4][1][1];
  if constexpr (!TEACHER) policy_prefetch<1, 1, PIN / 32, 4>(P.layers + 0, wave, PW, lane, w_ad);
  for (int idx = tid; idx < 16 * PIN; idx += 64 * PW) {
    const int e = idx / PIN, k = idx - e * PIN;
    float v = 0.0f;
    if (e < ne && k < H) v = P.obs_history[(size_t)(e0 + e) * P.hist_ld + k];
    if constexpr (TEACHER) {  // act_teacher: policy_info["latents"] = privileged_info
      if (e < ne && k >= H && k < H + NP) {
        v = P.privileged_obs[(size_t)(e0 + e) * NP + (k - H)];
        if (P.latent) P.latent[(size_t)(e0 + e) * NP + (k - H)] = v;
      }
    }
    act_store1(va, k, e, v, &s_ovf);
  }
  __syncthreads();
  PSTAMP(1);
  const PolicyLayer* Ls = P.layers;
  const ActV sa[1] = {va}, d1[1] = {h1.v()}, d2[1] = {h2.v()}, dad[1] = {had.v()};
  if constexpr (!TEACHER) {
    // adaptation module (xa rows >= hist_dim are still zero)
    policy_tiles_e<1, 1, 1, PIN / 32, 4, true>(Ls + 0, &sa, wave, PW, &d1, true, lane, &s_ovf, w_ad);  // 256
    __syncthreads();
    PSTAMP(2);
    {  // 256 -> 128: waves w and w + 8 take the two K halves of tile w & 7
      const int t = wave & 7, half = wave >> 3;
      f4_t acc[1];
      tile_partial_e<4, 1>(Ls[1], 8, t, 4 * half, &d1[0], lane, acc);
      if (half) {
#pragma unroll
        for (int r = 0; r < 4; ++r) scr_ad[t][4 * q + r][c] = acc[0][r];
      }
      __syncthreads();
      if (!half) {
        const f4_t b = *reinterpret_cast<const f4_t*>(Ls[1].b + 16 * t + 4 * q);
        f4_t v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = elu((b[r] + acc[0][r]) + scr_ad[t][4 * q + r][c]);
        act_store4(dad[0], 4 * t + q, c, v, &s_ovf);
      }
    }
    __syncthreads();
    PSTAMP(3);
    {  // 128 -> num_priv (the latent): one K group per wave (4 waves), partials summed by wave 0
      if (wave < 4) {
        f4_t acc[1];
        tile_partial_e<1, 1>(Ls[2], 4, 0, wave, &dad[0], lane, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) scr_ad[wave][4 * q + r][c] = acc[0][r];
      }
      __syncthreads();
      if (wave == 0 && q < 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 4 * q + r;  // latent feature f: also the actor's input hist_dim + f
          if (f < NP) {
            float l = Ls[2].b[f];
#pragma unroll
            for (int w = 0; w < 4; ++w) l += scr_ad[w][f][c];
            act_store1(va, H + f, c, l, &s_ovf);
            if (c < ne && P.latent) P.latent[(size_t)(e0 + c) * NP + f] = l;
          }
        }
      }
    }
    __syncthreads();
  }
  PSTAMP(4);
  policy_tiles_e<2, 1, 1, PIN / 32, 2>(Ls + 3, &sa, wave, PW, &d1, true, lane, &s_ovf);  // 512
  __syncthreads();
  PSTAMP(5);
  policy_tiles_e<1, 1, 1, 512 / 32, 3>(Ls + 4, &d1, wave, PW, &d2, true, lane, &s_ovf);  // 256
  __syncthreads();
  PSTAMP(6);
  if (wave < 8) policy_tiles_e<1, 1, 1, 256 / 32, 4>(Ls + 5, &d2, wave, 8, &d1, true, lane, &s_ovf);  // 128
  __syncthreads();
  PSTAMP(7);
  // 128 -> num_actions: one K group per wave (4 waves), partials through LDS (h2, free now)
  float(*scr)[16][16] = reinterpret_cast<float(*)[16][16]>(&h2);
  if (wave < 4) {
    f4_t part[1];
    tile_partial_e<1, 1>(Ls[6], 4, 0, wave, &d1[0], lane, part);
#pragma unroll
    for (int r = 0; r < 4; ++r) scr[wave][4 * q + r][c] = part[0][r];
  }
  __syncthreads();
  if (wave == 0) {
    f4_t acc = *reinterpret_cast<const f4_t*>(Ls[6].b + 4 * q);
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] += scr[w][4 * q + r][c];
    if (P.actions) {  // Normal(mean, std).sample() and its log_prob, as policy_kernel draws them
      float lp = 0.0f;
      f4_t a4, s4;
      float z4[4];
      normal4((uint32_t)(e0 + c + P.env_id_offset), q, P.rng_step, P.rng_seed, z4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 4 * q + r;
        const bool real = f < P.num_actions;
        const float sd = real ? P.std[f] : 1.0f;
        const float z = z4[r];
        a4[r] = acc[r] + sd * z;
        s4[r] = sd;
        if (real) lp += -0.5f * z * z - __logf(sd) - 0.91893853320467274f;  // log sqrt(2 pi)
      }
      auto x = __builtin_amdgcn_permlane16_swap(__float_as_uint(lp), __float_as_uint(lp), false, false);
      lp = __uint_as_float(x[0]) + __uint_as_float(x[1]);
      auto y = __builtin_amdgcn_permlane32_swap(__float_as_uint(lp), __float_as_uint(lp), false, false);
      lp = __uint_as_float(y[0]) + __uint_as_float(y[1]);
      if (c < ne) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 4 * q + r;
          if (f < P.num_actions) {
            P.actions[(size_t)(e0 + c) * P.num_actions + f] = a4[r];
            P.action_sigma[(size_t)(e0 + c) * P.num_actions + f] = s4[r];
          }
        }
        if (q == 0) P.log_prob[e0 + c] = lp;
      }
    }
    if (c < ne) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 4 * q + r;
        if (f < P.num_actions) P.action_mean[(size_t)(e0 + c) * P.num_actions + f] = acc[r];
      }
    }
  }
  PSTAMP(8);
  __syncthreads();
  if (s_ovf) policy_fallback_actor<TEACHER>(P, e0, ne, reinterpret_cast<float*>(&h1));
}

}  // namespace

// the launch for go1_policy_forward, which has checked the arguments (variant 1, mode STUDENT or TEACHER)
hipError_t go1_policy_launch_actor(const go1_policy_args& P, hipStream_t stream) {
  const dim3 grid((P.n_envs + 15) / 16), block(64 * PW);
  if (P.mode == GO1_POLICY_TEACHER)
    hipLaunchKernelGGL(policy_kernel_actor<true>, grid, block, 0, stream, P);
  else
    hipLaunchKernelGGL(policy_kernel_actor<false>, grid, block, 0, stream, P);
  return hipGetLastError();
}
