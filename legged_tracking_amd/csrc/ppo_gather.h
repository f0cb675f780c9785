// ppo_gather.h -- part of ppo_update.hip: the mini-batch rows gathered from the storage, and the embedding's
// gradient of the encoder module (the sum of the three first layers' products).
#pragma once

namespace {

// ------------------------------------------------------------------ the mini-batch rows of the storage
// One thread per element (no per-row dependent loads):
//   G[m] = [obs_history[idx[m]] (H), latent (P, written by adapt_kernel<0>), privileged_obs[idx[m]] (P), 0 ...]
//   B[m] = [actions (A), mu (A), sigma (A), actions_log_prob, advantages, returns, values]   (the head's inputs)
// G is the first layers' operand in 16-byte-loadable rows: the actor reads [hist, latent] (H + P columns), the
// critic [hist, latent, priv] against weights whose latent columns are zero, the adaptation module [hist].
struct GatherArgs {
  const float* hist;
  int64_t hld;
  const float *priv, *act, *mu, *sigma, *logp, *adv, *ret, *val;
  const int64_t* idx;
  int32_t M, H, P, A, ldg, bw;
  float* G;
  float* B;
  uint32_t* mx;
  // ENC: the heads' input columns of G are [embedding E (written by the encoder) | scalars S | scalars S], H = E + 2 S,
  // the scalars those of the last frame (columns foff .. foff + S of a history row); its map (the NM columns after
  // the scalars) goes to Mp rows of ldm floats, zero-padded
  int32_t E, S, foff, NM, ldm;
  float* Mp;
  uint32_t* mxmap;
};

// A wave gathers four rows at a time (rows strided over the grid): the four storage indices come in one load,
// then every element load of the four rows is issued (clamped addresses, selects afterwards) before any store.
// One atomicMax per workgroup: a max per row-block would serialise ~M atomics on one address.
constexpr int GATHER_BLOCKS_MAX = 1024;
template <bool ENC>
__global__ __launch_bounds__(256) void gather_kernel(GatherArgs g) {
  __shared__ uint32_t red[4];
  __shared__ uint32_t redm[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int M = g.M, H = g.H, P = g.P, A = g.A, ldg = g.ldg, bw = g.bw;
  const int nwaves = gridDim.x * 4;
  uint32_t mb = 0u, mm = 0u;
  for (int m0 = (blockIdx.x * 4 + w) * 4; m0 < M; m0 += nwaves * 4) {
    const int64_t ri = g.idx[min(m0 + (lane & 3), M - 1)];
    int64_t r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __shfl(ri, j);
    for (int k0 = ENC ? g.E : 0; k0 < ldg; k0 += 64) {  // E is a multiple of 128
      const int k = k0 + lane;
      const int ks = k - g.E - (k - g.E >= g.S ? g.S : 0);  // ENC: the scalar of column k (both copies)
      const int kh = ENC ? g.foff + min(max(ks, 0), max(g.S - 1, 0)) : min(k, H - 1);
      const int kp = min(max(k - H - P, 0), P - 1);
      const bool in_h = k < H, in_p = k >= H + P && k < H + 2 * P;
      float vh[4], vp[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vh[j] = g.hist[r[j] * g.hld + kh];
        vp[j] = g.priv[r[j] * P + kp];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = in_h ? vh[j] : (in_p ? vp[j] : 0.0f);
        if (m0 + j < M && k < ldg) {
          g.G[(size_t)(m0 + j) * ldg + k] = v;
          mb = max(mb, absbits(v));
        }
      }
    }
    if (ENC) {
      for (int k0 = 0; k0 < g.ldm; k0 += 64) {
        const int k = k0 + lane;
        const int km = g.foff + g.S + min(k, g.NM - 1);
        float vm[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) vm[j] = g.hist[r[j] * g.hld + km];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = k < g.NM ? vm[j] : 0.0f;
          if (m0 + j < M && k < g.ldm) {
            g.Mp[(size_t)(m0 + j) * g.ldm + k] = v;
            mm = max(mm, absbits(v));
          }
        }
      }
    }
    // B rows: [actions A, mu A, sigma A, logp, adv, ret, values, 0 ...] (bw <= 64 columns)
    {
      const int k = lane;
      const int seg = k < A ? 0 : (k < 2 * A ? 1 : (k < 3 * A ? 2 : 3));
      const int ka = min(k - seg * A, A - 1);
      const float* srcA = seg == 0 ? g.act : (seg == 1 ? g.mu : g.sigma);
      const int t = k - 3 * A;  // 0: logp, 1: adv, 2: ret, 3: values
      const float* srcS = t == 0 ? g.logp : (t == 1 ? g.adv : (t == 2 ? g.ret : g.val));
      float va[4], vs[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        va[j] = srcA[r[j] * A + max(ka, 0)];
        vs[j] = srcS[r[j]];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = seg < 3 ? va[j] : (t < 4 ? vs[j] : 0.0f);
        if (m0 + j < M && k < bw) g.B[(size_t)(m0 + j) * bw + k] = v;
      }
    }
  }
  mb = wave_max_u32(mb);
  if (ENC) mm = wave_max_u32(mm);
  if (lane == 0) {
    red[w] = mb;
    if (ENC) redm[w] = mm;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mb = max(max(red[0], red[1]), max(red[2], red[3]));
    if (mb) atomicMax(g.mx, mb);
    if (ENC) {
      mm = max(max(redm[0], redm[1]), max(redm[2], redm[3]));
      if (mm) atomicMax(g.mxmap, mm);
    }
  }
}

// ------------------------------------------------------------------ the embedding's gradient (phase 0)
// d emb = (t_p + t_c + t_a) * ELU'(emb): the three products W[:, emb]^T delta1 of the actor, the critic and the
// adaptation module (xw<LIN> outputs, summed in that order), with the column sums (the encoder's output bias
// gradient) per 128-row tile in a fixed order and max |d emb|.  Grid (row tiles, E / 128); a thread owns four
// columns of the rows rl, rl + 8, ... of its tile.
struct EmbArgs {
  const float *tp, *tc, *ta;  // [M][E]
  const float* emb;           // the forward embedding (G's leading columns), row stride lde
  int64_t lde;
  float* demb;                // [M][E]
  float* colsum;              // [tiles_m][E]
  uint32_t* dmax;
  int32_t M, E;
  // the CNN encoder's embedding has no activation (act 0: no ELU' factor); its phase 1 has the adaptation module's
  // term alone (nsrc 1: t_a; t_p and t_c are not read)
  int32_t act, nsrc;
};

__global__ __launch_bounds__(256) void embgrad_kernel(EmbArgs a) {
  __shared__ f4_t red[8][32];
  __shared__ uint32_t smax[4];
  const int tid = threadIdx.x, c4 = tid & 31, rl = tid >> 5;
  const int mt = blockIdx.x, n = blockIdx.y * TB + 4 * c4;
  f4_t cs = (f4_t){0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t mx = 0u;
#pragma unroll 4
  for (int i = 0; i < TB / 8; ++i) {
    const int m = mt * TB + rl + 8 * i;
    const bool in = m < a.M;
    const size_t o = (size_t)min(m, a.M - 1) * a.E + n;
    const f4_t ta = *reinterpret_cast<const f4_t*>(a.ta + o);
    f4_t tp = ta, tc = ta, e = ta;
    if (a.nsrc == 3) {  // uniform
      tp = *reinterpret_cast<const f4_t*>(a.tp + o);
      tc = *reinterpret_cast<const f4_t*>(a.tc + o);
    }
    if (a.act) e = *reinterpret_cast<const f4_t*>(a.emb + (size_t)min(m, a.M - 1) * a.lde + n);
    f4_t v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = a.nsrc == 3 ? (tp[j] + tc[j]) + ta[j] : ta[j];
      v[j] = in ? (a.act ? t * delu_from_out(e[j]) : t) : 0.0f;
      mx = max(mx, absbits(v[j]));
    }
    cs += v;
    if (in) *reinterpret_cast<f4_t*>(a.demb + o) = v;
  }
  red[rl][c4] = cs;
  mx = wave_max_u32(mx);
  if ((tid & 63) == 0) smax[tid >> 6] = mx;
  __syncthreads();
  if (rl == 0) {
    f4_t s = red[0][c4];
#pragma unroll
    for (int j = 1; j < 8; ++j) s += red[j][c4];
    *reinterpret_cast<f4_t*>(a.colsum + (size_t)mt * a.E + n) = s;
  }
  if (tid == 0) atomicMax(a.dmax, max(max(smax[0], smax[1]), max(smax[2], smax[3])));
}

}  // namespace
