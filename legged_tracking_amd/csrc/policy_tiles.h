// policy_tiles.h -- the building blocks of the policy kernels (rollout.hip, policy_actor.hip): the split activation
// planes in LDS, the weight-fragment prefetch and the MFMA tile loops, the in-kernel Normal draw, and the f32
// fallback of the range guard.
#ifndef GO1_POLICY_TILES_H
#define GO1_POLICY_TILES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/go1_rollout.h"
#include "split_mfma.h"

namespace {

// Philox4x32-10 (Salmon et al. 2011), as in the env step kernel
__device__ __forceinline__ void philox4x32(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// ------------------------------------------------------------------ policy inference
// ActorCritic.act / evaluate (actor_critic.py:121-150) for 16 envs per workgroup of 16 waves:
//   adaptation: hist(261) -> 256 -> 128 -> 2 (latent)
//   actor:      [hist, latent](263) -> 512 -> 256 -> 128 -> 12 (action mean)
//   critic:     [hist, priv](263)   -> 512 -> 256 -> 128 -> 1  (value)
// ELU between layers.  f32 accuracy from f16 matrix cores ("3xF16"): every f32 weight and
// activation x is split into hi = f16(x) and lo = f16(x - hi) (22 significant bits together),
// and each 32-deep K group of a dot product is three v_mfma_f32_16x16x32_f16,
//   acc += Whi Xhi + Whi Xlo + Wlo Xhi
// with products exact in f32 and f32 accumulation; the dropped Wlo Xlo term is ~2^-22 of the
// product, below the f32 rounding of the sums.  On gfx950 a 16x16x32 f16 MFMA issues in the 16
// cycles of a 16x16x16 one (tools/probes/mfma_rate.hip: 16.3 cycles each, one wave), so the K=32 form
// does twice the work per MFMA cycle.  Weights are split and packed on the host into fragment order:
// 32 bytes per lane per (tile, K group) = 8 hi + 8 lo halves, L2-resident (2.8 MB for all three
// nets).  Activations live in LDS already split, as [k/8][env][8] halves (hi plane, then lo plane): a
// B fragment (k = 32 g + 8 q + r, env c) is one 16-byte read per plane, and a layer's output tile
// (rows 4 q + r of env c) one 8-byte write.
constexpr int PIN = 288;  // 261 / 263 inputs padded to a multiple of 32
constexpr int PW = 16;    // waves per workgroup (four per SIMD)

typedef go1_policy_layer PolicyLayer;  // w packed [n/16][k/32][64 lanes][8 hi + 8 lo halves], b [n padded to 16]

// split activation planes in LDS: element (k, env c) at [k / 8][c][k % 8] of hi, and of lo
struct ActV {
  h8_t* hi;
  h8_t* lo;
};
template <int K>
struct Act {
  h8_t hi[K / 8][16];
  h8_t lo[K / 8][16];
  __device__ ActV v() { return ActV{&hi[0][0], &lo[0][0]}; }
};

// Normal(0, 1) draws of actions 4 q .. 4 q + 3 of global env gid: one Philox4x32-10 block keyed by
// (env, action group, step), two Box-Muller pairs on the hardware log2 / sqrt / sin / cos (v_sin / v_cos
// take revolutions).  The samples are the kernel's own stream (the reference draws from torch's generator).
__device__ __forceinline__ void normal4(uint32_t gid, int q, uint64_t step, uint64_t seed, float z[4]) {
  uint32_t ctr[4] = {gid, (uint32_t)q, (uint32_t)step, (uint32_t)(step >> 32)};
  philox4x32(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    // (0, 1]: from 2^23 on the + 0.5f is not representable and rounds to even, so the top mantissa gives exactly
    // 1.0, where r = 0 and z = +-0 (never NaN); tests/normal_ref.py restates the draw
    const float u1 = ((float)(ctr[2 * p] >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = (float)(ctr[2 * p + 1] >> 8) * (1.0f / 16777216.0f);  // [0, 1)
    const float r = __builtin_amdgcn_sqrtf(-2.0f * 0.69314718055994531f * __builtin_amdgcn_logf(u1));
    z[2 * p] = r * __builtin_amdgcn_cosf(u2);
    z[2 * p + 1] = r * __builtin_amdgcn_sinf(u2);
  }
}

// four consecutive features 4 kq .. 4 kq + 3 of env c, split into the two planes
__device__ __forceinline__ void act_store4(ActV d, int kq, int c, f4_t v, int* ovf) {
  h4_t h, l;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ovf_check(v[r], ovf);
    h[r] = (_Float16)v[r];
    l[r] = (_Float16)(v[r] - (float)h[r]);
  }
  reinterpret_cast<h4_t*>(d.hi)[((kq >> 1) * 16 + c) * 2 + (kq & 1)] = h;
  reinterpret_cast<h4_t*>(d.lo)[((kq >> 1) * 16 + c) * 2 + (kq & 1)] = l;
}
__device__ __forceinline__ void act_store1(ActV d, int k, int c, float v, int* ovf) {
  ovf_check(v, ovf);
  const _Float16 h = (_Float16)v;
  reinterpret_cast<_Float16*>(d.hi)[((k >> 3) * 16 + c) * 8 + (k & 7)] = h;
  reinterpret_cast<_Float16*>(d.lo)[((k >> 3) * 16 + c) * 8 + (k & 7)] = (_Float16)(v - (float)h);
}

template <int NT, int NL>
__device__ __forceinline__ void policy_load(const PolicyLayer* L, int G, int g, int tile0, int tstride, int lane,
                                            f8_t (&w)[NL][NT]) {
#pragma unroll
  for (int l = 0; l < NL; ++l)
#pragma unroll
    for (int i = 0; i < NT; ++i)
      w[l][i] = reinterpret_cast<const f8_t*>(L[l].w)[((size_t)(tile0 + i * tstride) * G + g) * 64 + lane];
  // keep the prefetch where it is written: otherwise the scheduler sinks the loads next to
  // their MFMAs and the waits become vmcnt(1), exposing the L2 latency every group
  __builtin_amdgcn_sched_barrier(0);
}

// the first D weight groups of a policy_tiles_e phase, issued early: they depend on nothing the
// workgroup computes, so the adaptation module's can be in flight while the inputs are staged
template <int NT, int NL, int G, int D>
__device__ __forceinline__ void policy_prefetch(const PolicyLayer* L, int tile0, int tstride, int lane,
                                                f8_t (&w)[D][NL][NT]) {
#pragma unroll
  for (int g = 0; g < D && g < G; ++g) policy_load<NT, NL>(L, G, g, tile0, tstride, lane, w[g]);
}

// NT output tiles (tile0 + i * tstride) of NL layers at the same depth (the actor and the critic
// advance together) for ET env tiles of 16 envs that share every weight fragment (src / dst [et][l]):
// acc = b + W x, ELU (act), store split to dst.  The G K groups are unrolled and the weight fragments
// run D groups ahead of the MFMAs: with three 8-cycle f16 MFMAs per fragment the layers are bound by
// the L2 -> CU weight stream, which needs ~12 16-byte loads in flight per lane (64 B/clk/CU x the L2
// latency, 16 waves).
template <int NT, int NL, int ET>
__device__ __forceinline__ void policy_group_e(const f8_t (&w)[NL][NT], const ActV (*src)[NL], int g, int q, int c,
                                               f4_t (&acc)[ET][NL][NT]) {
#pragma unroll
  for (int l = 0; l < NL; ++l)
#pragma unroll
    for (int et = 0; et < ET; ++et) {
      const h8_t xh = src[et][l].hi[(4 * g + q) * 16 + c], xl = src[et][l].lo[(4 * g + q) * 16 + c];
#pragma unroll
      for (int i = 0; i < NT; ++i) acc[et][l][i] = mfma3(w[l][i], xh, xl, acc[et][l][i]);
    }
}

template <int NT, int NL, int ET, int G, int D, bool PREFETCHED = false>
__device__ __forceinline__ void policy_tiles_e(const PolicyLayer* L, const ActV (*src)[NL], int tile0, int tstride,
                                               const ActV (*dst)[NL], bool act, int lane, int* ovf,
                                               f8_t (*pre)[NL][NT] = nullptr) {
  const int q = lane >> 4, c = lane & 15;
  f4_t acc[ET][NL][NT];
  f8_t w[D][NL][NT];
#pragma unroll
  for (int l = 0; l < NL; ++l)
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const f4_t b = *reinterpret_cast<const f4_t*>(L[l].b + 16 * (tile0 + i * tstride) + 4 * q);
#pragma unroll
      for (int et = 0; et < ET; ++et) acc[et][l][i] = b;
    }
  if constexpr (PREFETCHED) {
#pragma unroll
    for (int g = 0; g < D; ++g)
#pragma unroll
      for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int i = 0; i < NT; ++i) w[g][l][i] = pre[g][l][i];
  } else {
    policy_prefetch<NT, NL, G, D>(L, tile0, tstride, lane, w);
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    policy_group_e<NT, NL, ET>(w[g % D], src, g, q, c, acc);
    if (g + D < G) policy_load<NT, NL>(L, G, g + D, tile0, tstride, lane, w[g % D]);
  }
#pragma unroll
  for (int et = 0; et < ET; ++et)
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        f4_t v = acc[et][l][i];
        if (act) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = elu(v[r]);
        }
        act_store4(dst[et][l], 4 * (tile0 + i * tstride) + q, c, v, ovf);
      }
}

// the NG weight fragments of a tile_partial_e, loaded ahead (they depend on nothing the workgroup computes)
template <int NG>
__device__ __forceinline__ void partial_load(const PolicyLayer& L, int Gs, int tile, int g0, int lane, f8_t (&w)[NG]) {
#pragma unroll
  for (int i = 0; i < NG; ++i) w[i] = reinterpret_cast<const f8_t*>(L.w)[((size_t)tile * Gs + g0 + i) * 64 + lane];
}

// Partial products of one output tile over K groups [g0, g0 + NG) for ET env tiles, no bias: the
// K-split form of the narrow layers (one wave walking all of K would run a serial MFMA chain behind
// one L2 round trip per group).  All NG weight fragments are loaded up front (one round trip), or
// taken from `pre`.
template <int NG, int ET>
__device__ __forceinline__ void tile_partial_e(const PolicyLayer& L, int Gs, int tile, int g0, const ActV* src, int lane,
                                               f4_t (&acc)[ET], const f8_t* pre = nullptr) {
  const int q = lane >> 4, c = lane & 15;
  f8_t w[NG];
  if (pre) {
#pragma unroll
    for (int i = 0; i < NG; ++i) w[i] = pre[i];
  } else {
    partial_load<NG>(L, Gs, tile, g0, lane, w);
  }
#pragma unroll
  for (int et = 0; et < ET; ++et) acc[et] = f4_t{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < NG; ++i)
#pragma unroll
    for (int et = 0; et < ET; ++et)
      acc[et] = mfma3(w[i], src[et].hi[(4 * (g0 + i) + q) * 16 + c], src[et].lo[(4 * (g0 + i) + q) * 16 + c], acc[et]);
}

// ---------------------------------------------------------------- range guard: f32 fallback
// y = act(W x + b) for one env, W (n_out, k_in) row-major f32, by the workgroup (output o on thread o)
__device__ void dense_f32(const float* __restrict__ W, const float* __restrict__ b, int n_out, int k_in,
                          const float* x, float* y, bool act) {
  for (int o = threadIdx.x; o < n_out; o += blockDim.x) {
    float acc = b[o];
    const float* w = W + (size_t)o * k_in;
    for (int k = 0; k < k_in; ++k) acc = fmaf(w[k], x[k], acc);
    y[o] = act ? elu(acc) : acc;
  }
  __syncthreads();
}

// policy_fallback's actor for the kernels of GO1_POLICY_STUDENT / TEACHER.  TEACHER: no adaptation module, the
// actor's latent inputs (and `latent`) are the privileged observations.  A function of its own: policy_fallback stays
// in policy_full.h (rollout.hip's translation unit) with the GO1_POLICY_FULL kernels, whose code the modes leave as it
// was.
template <bool TEACHER>
__device__ void policy_fallback_actor(const go1_policy_args& P, int e0, int ne, float* buf) {
  const go1_policy_layer* L = P.layers;
  const int H = P.hist_dim, NP = P.num_priv, NA = P.num_actions;
  float* x = buf;
  float* ya = buf + ((H + NP + 31) & ~31);
  float* yb = ya + 512;
  for (int e = 0; e < ne; ++e) {
    const size_t ge = (size_t)(e0 + e);
    for (int k = threadIdx.x; k < H; k += blockDim.x) x[k] = P.obs_history[ge * P.hist_ld + k];
    if constexpr (TEACHER) {
      for (int k = threadIdx.x; k < NP; k += blockDim.x) x[H + k] = P.privileged_obs[ge * NP + k];
      __syncthreads();
    } else {
      __syncthreads();
      dense_f32(L[0].wf, L[0].b, 256, H, x, ya, true);
      dense_f32(L[1].wf, L[1].b, 128, 256, ya, yb, true);
      dense_f32(L[2].wf, L[2].b, NP, 128, yb, x + H, false);  // the latent, appended to the actor's input
    }
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
  if (threadIdx.x == 0 && P.overflow) atomicAdd(P.overflow, 1);
}

}  // namespace

#endif  // GO1_POLICY_TILES_H
