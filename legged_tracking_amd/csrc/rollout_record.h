// rollout_record.h -- GAE, the advantage normalisation and the two transition-record kernels: gae_kernel
// (RolloutStorage.compute_returns, go1_gym_learn/ppo_cse/rollout_storage.py:76-87), adv_norm_kernel (:89-90), Seg,
// RecPlan, record_kernel and record_flat_kernel (add_transitions :57-71 + PPO.process_env_step's bootstrap,
// ppo.py:79-92).  A part of rollout.hip, included inside its anonymous namespace.
#pragma once
#ifndef GO1_ROLLOUT_HIP
#error "include this part from rollout.hip: its parts are not self-contained"
#endif

// One thread per env: the reverse scan over T steps.  Reads rewards / dones /
// values once (coalesced along envs at each step), writes returns and raw
// advantages, and reduces (sum, sum of squares) of the advantages in f64.
__global__ __launch_bounds__(256) void gae_kernel(const float* __restrict__ rewards, const uint8_t* __restrict__ dones,
                                                  const float* __restrict__ values,
                                                  const float* __restrict__ last_values, float* __restrict__ returns,
                                                  float* __restrict__ advantages, double* __restrict__ stats, int T,
                                                  int n, float gamma, float lam) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  double s = 0.0, s2 = 0.0;
  if (e < n) {
    float adv = 0.0f;
    float next_v = last_values[e];
    for (int t = T - 1; t >= 0; --t) {
      const size_t i = (size_t)t * n + e;
      const float v = values[i];
      const float nt = 1.0f - (float)dones[i];
      // delta = r + nt * gamma * next_v - v   (torch: ((nt * gamma) * next_v), then +, then -)
      const float delta = (rewards[i] + (nt * gamma) * next_v) - v;
      // advantage = delta + nt * gamma * lam * advantage
      adv = delta + ((nt * gamma) * lam) * adv;
      const float ret = adv + v;
      returns[i] = ret;
      const float a = ret - v;  // advantages = returns - values (:89)
      advantages[i] = a;
      s += (double)a;
      s2 += (double)a * (double)a;
      next_v = v;
    }
  }
  // wave reduction, then one f64 atomic pair per wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    s2 += __shfl_xor(s2, o);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(stats, s);
    atomicAdd(stats + 1, s2);
  }
}

// (a - mean) / (std + 1e-8) with the unbiased std of torch.std over `count` samples.
__global__ __launch_bounds__(256) void adv_norm_kernel(float* __restrict__ adv, const double* __restrict__ stats,
                                                       double count, size_t total) {
  const double mean_d = stats[0] / count;
  double var = (stats[1] - count * mean_d * mean_d) / (count - 1.0);
  var = var > 0.0 ? var : 0.0;
  const float mean = (float)mean_d;
  const float den = (float)sqrt(var) + 1e-8f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    adv[i] = (adv[i] - mean) / den;
}

struct Seg {
  const float* src;
  float* dst;
  int64_t n;  // floats
};

// All per-step copies of add_transitions in one launch; the reward column gets the
// time-out bootstrap r + gamma * (v * time_out) (ppo.py:85-87), dones become u8.
__global__ __launch_bounds__(256) void record_kernel(go1_transition tr, int n, float gamma) {
  const Seg segs[7] = {{tr.obs, tr.st_obs, (int64_t)n * tr.num_obs},
                       {tr.privileged_obs, tr.st_privileged_obs, (int64_t)n * tr.num_priv},
                       {tr.obs_history, tr.st_obs_history, (int64_t)n * tr.num_obs_history},
                       {tr.actions, tr.st_actions, (int64_t)n * tr.num_actions},
                       {tr.mu, tr.st_mu, (int64_t)n * tr.num_actions},
                       {tr.sigma, tr.st_sigma, (int64_t)n * tr.num_actions},
                       {tr.actions_log_prob, tr.st_actions_log_prob, (int64_t)n}};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t hld = tr.obs_history_ld, hw = tr.num_obs_history;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const Seg g = segs[s];
    if (!g.src) continue;
    if (s == 2 && hld != hw) {  // a row-strided history window: rows of hw floats, hld apart
      if (((hw | hld) & 1) == 0 && ((((uintptr_t)g.src) | ((uintptr_t)g.dst)) & 7) == 0) {
        const int64_t w2 = hw >> 1, n2 = (int64_t)n * w2;
        for (int64_t i = tid; i < n2; i += stride) {
          const int64_t r = i / w2, c = i - r * w2;
          reinterpret_cast<float2*>(g.dst)[i] = *reinterpret_cast<const float2*>(g.src + r * hld + 2 * c);
        }
      } else {
        for (int64_t i = tid; i < g.n; i += stride) {
          const int64_t r = i / hw;
          g.dst[i] = g.src[r * hld + (i - r * hw)];
        }
      }
      continue;
    }
    const bool vec = ((((uintptr_t)g.src) | ((uintptr_t)g.dst)) & 15) == 0;
    if (vec) {
      const int64_t n4 = g.n >> 2;
      const float4* s4 = reinterpret_cast<const float4*>(g.src);
      float4* d4 = reinterpret_cast<float4*>(g.dst);
      for (int64_t i = tid; i < n4; i += stride) d4[i] = s4[i];
      for (int64_t i = (n4 << 2) + tid; i < g.n; i += stride) g.dst[i] = g.src[i];
    } else {
      for (int64_t i = tid; i < g.n; i += stride) g.dst[i] = g.src[i];
    }
  }
  const bool rebind = tr.time_outs_flag && *tr.time_outs_flag != 0;
  for (int64_t e = tid; e < n; e += stride) {
    const float v = tr.values[e];
    float r = tr.rewards[e];
    const uint8_t* to = rebind ? tr.time_outs_pending : tr.time_outs;
    if (to) {
      const uint8_t t = to[e];
      if (rebind && tr.time_outs_dst) tr.time_outs_dst[e] = t;
      r = r + gamma * (v * (t ? 1.0f : 0.0f));
    }
    tr.st_rewards[e] = r;
    tr.st_values[e] = v;
    tr.st_dones[e] = tr.dones[e] ? 1 : 0;
  }
}

// The same copies with one 16-byte chunk per thread and each workgroup on one segment (block ranges per
// segment, chosen on the host when every buffer is 16-byte aligned and the history is contiguous): every
// thread issues its single load at once instead of walking the segments one round trip after the other.
#define REC_MAX_SEGS 8
struct RecPlan {
  const float4* src[REC_MAX_SEGS];
  float4* dst[REC_MAX_SEGS];
  float4* dst2[REC_MAX_SEGS];  // a second destination (obs_history aliasing obs: one read feeds both rows)
  int64_t nf[REC_MAX_SEGS];    // floats
  int first[REC_MAX_SEGS + 1]; // first workgroup of each segment; first[nseg] = the env columns' first
  int nseg;
};
__global__ __launch_bounds__(256) void record_flat_kernel(RecPlan P, go1_transition tr, int n, float gamma) {
  const int b = blockIdx.x, t = threadIdx.x;
  if (b >= P.first[P.nseg]) {  // per-env columns: bootstrap reward, value, done
    const int64_t e = (int64_t)(b - P.first[P.nseg]) * 256 + t;
    if (e >= n) return;
    // every column requested before any is used (both time-out arrays: the flag picks one afterwards)
    const float v = tr.values[e];
    float r = tr.rewards[e];
    const uint8_t d = tr.dones[e];
    const uint8_t* tn_p = tr.time_outs ? tr.time_outs : tr.dones;
    const uint8_t* tp_p = tr.time_outs_pending ? tr.time_outs_pending : tr.dones;
    const uint8_t tn = tn_p[e], tp = tp_p[e];
    const bool rebind = tr.time_outs_flag && *tr.time_outs_flag != 0;
    if (rebind ? tr.time_outs_pending != nullptr : tr.time_outs != nullptr) {
      const uint8_t tt = rebind ? tp : tn;
      if (rebind && tr.time_outs_dst) tr.time_outs_dst[e] = tt;
      r = r + gamma * (v * (tt ? 1.0f : 0.0f));
    }
    tr.st_rewards[e] = r;
    tr.st_values[e] = v;
    tr.st_dones[e] = d ? 1 : 0;
    return;
  }
  int s = 0;  // the workgroup's segment (uniform)
  while (s + 1 < P.nseg && b >= P.first[s + 1]) ++s;
  const int64_t k = (int64_t)(b - P.first[s]) * 256 + t, n4 = P.nf[s] >> 2;
  const float4* src = P.src[s];
  float4* dst = P.dst[s];
  float4* dst2 = P.dst2[s];
  if (k < n4) {
    const float4 v = src[k];
    dst[k] = v;
    if (dst2) dst2[k] = v;
  }
  const int rem = (int)(P.nf[s] & 3);
  if (b == P.first[s] && t < rem) {  // the last nf % 4 floats
    const float x = reinterpret_cast<const float*>(src)[4 * n4 + t];
    reinterpret_cast<float*>(dst)[4 * n4 + t] = x;
    if (dst2) reinterpret_cast<float*>(dst2)[4 * n4 + t] = x;
  }
}
