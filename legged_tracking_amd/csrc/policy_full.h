// policy_full.h -- policy_kernel, the one-launch shape of GO1_POLICY_FULL (every workgroup runs the adaptation
// module, the actor and the critic of 16 envs: ActorCritic.act / evaluate, go1_gym_learn/ppo_cse/actor_critic.py),
// with policy_fallback (the f32 recomputation of rows that left the f16 range) and the PSTAMP diagnostic stamps.
// A part of rollout.hip, included inside its anonymous namespace after policy_tiles.h and split_mfma.h.
#pragma once
#ifndef GO1_ROLLOUT_HIP
#error "include this part from rollout.hip: its parts are not self-contained"
#endif

// The envs [e0, e0 + ne) of a workgroup whose split activations left the f16 range, recomputed in f32
// from the unsplit weights (layers[].wf): the adaptation module + actor (+ the Normal sample with the
// same Philox draws) and / or the critic.  `buf`: >= hist_dim + num_priv (rounded up to 32) + 768 floats of
// LDS no longer in use.
__device__ void policy_fallback(const go1_policy_args& P, int e0, int ne, bool actor, bool critic, float* buf) {
  const go1_policy_layer* L = P.layers;
  const int H = P.hist_dim, NP = P.num_priv, NA = P.num_actions;
  float* x = buf;
  float* ya = buf + ((H + NP + 31) & ~31);
  float* yb = ya + 512;
  for (int e = 0; e < ne; ++e) {
    const size_t ge = (size_t)(e0 + e);
    for (int k = threadIdx.x; k < H; k += blockDim.x) x[k] = P.obs_history[ge * P.hist_ld + k];
    __syncthreads();
    if (actor) {
      dense_f32(L[0].wf, L[0].b, 256, H, x, ya, true);
      dense_f32(L[1].wf, L[1].b, 128, 256, ya, yb, true);
      dense_f32(L[2].wf, L[2].b, NP, 128, yb, x + H, false);  // the latent, appended to the actor's input
      if (P.latent && (int)threadIdx.x < NP) P.latent[ge * NP + threadIdx.x] = x[H + threadIdx.x];
      dense_f32(L[3].wf, L[3].b, 512, H + NP, x, ya, true);
      dense_f32(L[4].wf, L[4].b, 256, 512, ya, yb, true);
      dense_f32(L[5].wf, L[5].b, 128, 256, yb, ya, true);
      dense_f32(L[6].wf, L[6].b, NA, 128, ya, yb, false);
      if (threadIdx.x == 0) {
        float lp_q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float zq[4];
        for (int f = 0; f < NA; ++f) {
          P.action_mean[ge * NA + f] = yb[f];
          if (P.actions) {
            const float sd = P.std[f];
            if ((f & 3) == 0) normal4((uint32_t)(ge + P.env_id_offset), f >> 2, P.rng_step, P.rng_seed, zq);
            const float z = zq[f & 3];
            P.actions[ge * NA + f] = yb[f] + sd * z;
            P.action_sigma[ge * NA + f] = sd;
            lp_q[f >> 2] += -0.5f * z * z - __logf(sd) - 0.91893853320467274f;
          }
        }
        if (P.actions) P.log_prob[ge] = (lp_q[0] + lp_q[1]) + (lp_q[2] + lp_q[3]);
      }
      __syncthreads();
    }
    if (critic) {
      for (int k = threadIdx.x; k < NP; k += blockDim.x) x[H + k] = P.privileged_obs[ge * NP + k];
      __syncthreads();
      dense_f32(L[7].wf, L[7].b, 512, H + NP, x, ya, true);
      dense_f32(L[8].wf, L[8].b, 256, 512, ya, yb, true);
      dense_f32(L[9].wf, L[9].b, 128, 256, yb, ya, true);
      dense_f32(L[10].wf, L[10].b, 1, 128, ya, yb, false);
      if (threadIdx.x == 0) P.value[ge] = yb[0];
      __syncthreads();
    }
  }
  if (threadIdx.x == 0 && P.overflow) atomicAdd(P.overflow, 1);
}

#ifdef GO1_POLICY_STAMPS  // diagnostic build only (tools/policy_stamps.py): s_memtime per wave per phase
#define PSTAMP_SLOTS 12
__device__ unsigned long long g_pstamps[512 * 16 * PSTAMP_SLOTS];
#define PSTAMP(k)                                                                                   \
  do {                                                                                              \
    unsigned long long t_;                                                                          \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                   \
    if (blockIdx.x < 512) g_pstamps[(blockIdx.x * 16 + (threadIdx.x >> 6)) * PSTAMP_SLOTS + (k)] = t_; \
  } while (0)
#else
#define PSTAMP(k)
#endif

__global__ __launch_bounds__(64 * PW) void policy_kernel(go1_policy_args P) {
  __shared__ Act<PIN> xa, xc;  // actor / critic inputs (the adaptation module reads xa)
  __shared__ Act<512> h1[2];   // layer-1 outputs (actor, critic); layer 3 reuses them
  __shared__ Act<256> h2[2];   // layer-2 outputs; also the f32 scratch of the K-split partials
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int e0 = blockIdx.x * 16;
  PSTAMP(0);
  const int ne = min(16, P.n_envs - e0);
  const int NP = P.num_priv;
  const ActV va = xa.v(), vc = xc.v();
  __shared__ int s_ovf;
  if (tid == 0) s_ovf = 0;
  // the adaptation module's first weight groups are in flight while the inputs are staged
  f8_t w_ad[4][1][1];
  policy_prefetch<1, 1, PIN / 32, 4>(P.layers + 0, wave, PW, lane, w_ad);
  for (int idx = tid; idx < 16 * PIN; idx += 64 * PW) {
    const int e = idx / PIN, k = idx - e * PIN;
    float v = 0.0f;
    if (e < ne && k < P.hist_dim) v = P.obs_history[(size_t)(e0 + e) * P.hist_ld + k];
    act_store1(va, k, e, v, &s_ovf);
    act_store1(vc, k, e,
               (e < ne && k >= P.hist_dim && k < P.hist_dim + NP)
                   ? P.privileged_obs[(size_t)(e0 + e) * NP + (k - P.hist_dim)] : v, &s_ovf);
  }
  __syncthreads();
  PSTAMP(1);
  const PolicyLayer* Ls = P.layers;
  // the shared helpers take [env tile][layer] planes: one env tile here
  const ActV vh1[2] = {h1[0].v(), h1[1].v()}, vh2[2] = {h2[0].v(), h2[1].v()};
  const ActV sa[1] = {va}, da[1] = {vh1[0]};
  // adaptation module (xa rows >= hist_dim are still zero)
  policy_tiles_e<1, 1, 1, PIN / 32, 4, true>(Ls + 0, &sa, wave, PW, &da, true, lane, &s_ovf, w_ad);  // 256
  __syncthreads();
  PSTAMP(2);
  // 256 -> 128: waves w and w + 8 take the two K halves of tile w & 7; the upper half's partial
  // goes through LDS (h2[1], free until the actor/critic's second layer)
  {
    float(*scr)[16][16] = reinterpret_cast<float(*)[16][16]>(&h2[1]);
    const int q = lane >> 4, c = lane & 15, t = wave & 7, half = wave >> 3;
    f4_t acc[1];
    tile_partial_e<4, 1>(Ls[1], 8, t, 4 * half, &vh1[0], lane, acc);
    if (half) {
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[t][4 * q + r][c] = acc[0][r];
    }
    __syncthreads();
    if (!half) {
      const f4_t b = *reinterpret_cast<const f4_t*>(Ls[1].b + 16 * t + 4 * q);
      f4_t v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = elu((b[r] + acc[0][r]) + scr[t][4 * q + r][c]);
      act_store4(vh2[0], 4 * t + q, c, v, &s_ovf);
    }
  }
  __syncthreads();
  PSTAMP(3);
  // 128 -> num_priv (the latent): one K group per wave (4 waves), partials summed by wave 0
  {
    float(*scr)[16][16] = reinterpret_cast<float(*)[16][16]>(&h2[1]);
    const int q = lane >> 4, c = lane & 15;
    if (wave < 4) {
      f4_t acc[1];
      tile_partial_e<1, 1>(Ls[2], 4, 0, wave, &vh2[0], lane, acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[wave][4 * q + r][c] = acc[0][r];
    }
    __syncthreads();
    if (wave == 0 && q < 2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 4 * q + r;  // latent feature f: also the actor's input hist_dim + f
        if (f < NP) {
          float l = Ls[2].b[f];
#pragma unroll
          for (int w = 0; w < 4; ++w) l += scr[w][f][c];
          act_store1(va, P.hist_dim + f, c, l, &s_ovf);
          if (c < ne && P.latent) P.latent[(size_t)(e0 + c) * NP + f] = l;
        }
      }
    }
  }
  __syncthreads();
  PSTAMP(4);
  // actor and critic, layer by layer; wave w takes tiles w, w + 16, ... of both nets
  const PolicyLayer LA1[2] = {Ls[3], Ls[7]}, LA2[2] = {Ls[4], Ls[8]};
  {
    const ActV s1[2] = {va, vc};
    policy_tiles_e<2, 2, 1, PIN / 32, 2>(LA1, &s1, wave, PW, &vh1, true, lane, &s_ovf);  // 512
  }
  __syncthreads();
  PSTAMP(5);
  policy_tiles_e<1, 2, 1, 512 / 32, 3>(LA2, &vh1, wave, PW, &vh2, true, lane, &s_ovf);  // 256
  __syncthreads();
  PSTAMP(6);
  {  // 256 -> 128, one tile per wave: waves 0-7 the actor's, 8-15 the critic's
    const bool critic = wave >= 8;
    const PolicyLayer L3 = critic ? Ls[9] : Ls[5];
    const ActV src[1] = {critic ? h2[1].v() : h2[0].v()}, dst[1] = {critic ? h1[1].v() : h1[0].v()};
    policy_tiles_e<1, 1, 1, 256 / 32, 4>(&L3, &src, wave & 7, 8, &dst, true, lane, &s_ovf);
  }
  __syncthreads();
  PSTAMP(7);
  // 128 -> num_actions (actor, waves 0-3) and 128 -> 1 (critic, waves 8-11): one K group per
  // wave, partials through LDS (h2, free once the third layer has read it)
  {
    float(*scr)[16][16] = reinterpret_cast<float(*)[16][16]>(&h2[0]);
    const int q = lane >> 4, c = lane & 15;
    const bool critic = wave >= 8;
    if ((wave & 7) < 4) {
      f4_t part[1];
      const ActV src = critic ? h1[1].v() : h1[0].v();
      tile_partial_e<1, 1>(Ls[critic ? 10 : 6], 4, 0, wave & 7, &src, lane, part);
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[wave][4 * q + r][c] = part[0][r];
    }
  }
  __syncthreads();
  if (wave < 2) {
    const int q = lane >> 4, c = lane & 15;
    const PolicyLayer L = Ls[wave == 0 ? 6 : 10];
    f4_t acc = *reinterpret_cast<const f4_t*>(L.b + 4 * q);
    {
      float(*scr)[16][16] = reinterpret_cast<float(*)[16][16]>(&h2[0]);
#pragma unroll
      for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += scr[8 * wave + w][4 * q + r][c];
    }
    if (wave == 0 && P.actions) {
      // Normal(mean, std).sample() and its log_prob summed over the actions
      // (actor_critic.py:137-145), Box-Muller on Philox4x32-10 uniforms keyed by
      // (global env, action group q, step): row q, element r is action f = 4 q + r of env c (normal4)
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
      // sum over the four rows (actions 0-3, 4-7, 8-11, 12-15 of the env)
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
        if (wave == 0 && f < P.num_actions) P.action_mean[(size_t)(e0 + c) * P.num_actions + f] = acc[r];
        if (wave == 1 && f == 0) P.value[e0 + c] = acc[r];
      }
    }
  }
  PSTAMP(8);
  __syncthreads();
  if (s_ovf) policy_fallback(P, e0, ne, true, true, reinterpret_cast<float*>(&h1[0]));
}
