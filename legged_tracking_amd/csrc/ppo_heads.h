// ppo_heads.h -- part of ppo_update.hip: the layers that are not 128-wide GEMM tiles.  head_kernel: the actor's and
// the critic's output layers with the PPO loss and its gradient; adapt_kernel: the adaptation module's output layer
// (the latent), forward, with the adaptation loss, and backward from the actor's first layer.
#pragma once

namespace {

// ------------------------------------------------------------------ the actor / critic heads and the loss
// A half-wave per mini-batch row (two rows per wave step, rows strided over the grid), lanes along the 128
// features of a3 (4 per lane, lane + 32 j).  mu = W4 a3 + b4, V = W4c a3c + b4c (half-wave sums), then
// Normal(mu, std).log_prob, the ratio, the clipped surrogate, the clipped value loss and the KL (ppo.py:107-158)
// and their gradients with torch's semantics (max / clamp backward: ties split the gradient in halves, clamp
// passes it on the closed interval); lane a < A owns action a.  Backward through L4: delta3 = (W4^T dmu) *
// ELU'(a3) for the lane's features, with per-lane sums of dW4, db3 (and the critic's) over the rows; the block's
// eight half-waves are summed (in a fixed order) into one partial row [block][HSTR] for reduce_kernel.
struct HeadArgs {
  int32_t M, A, bw;
  const float* B;  // gathered [actions, mu, sigma, logp, adv, ret, values] rows
  const float* a3p;
  const float* a3c;
  const float* w4p;
  const float* b4p;
  const float* w4c;
  const float* b4c;
  const float* std_;
  const go1_ppo_hyper* hyper;
  float* d3p;
  float* d3c;
  uint32_t* d3pmax;
  uint32_t* d3cmax;
  float* part;
  int32_t hstr;
};
// partial layout: dW4p [A][128], db4p [A], db3p [128], dW4c [128], db4c, db3c [128], dstd [A], Ls, Lv, KL
__host__ __device__ constexpr int head_stride(int A) { return A * 128 + A + 128 + 128 + 1 + 128 + A + 3; }
constexpr int HEAD_BLOCKS = 512;
struct HeadPart {  // host: the offsets of that layout (head_kernel's o_*)
  int dW4p = 0, db4p, db3p, dW4c, db4c, db3c, dstd, loss;
  explicit HeadPart(int A)
      : db4p(A * 128), db3p(db4p + A), dW4c(db3p + 128), db4c(dW4c + 128), db3c(db4c + 1), dstd(db3c + 128),
        loss(dstd + A) {}
};

template <int NA>
__global__ __launch_bounds__(256) void head_kernel(HeadArgs H) {
  __shared__ float red[4][head_stride(NA)];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, half = lane >> 5, l = lane & 31;
  const int gw = blockIdx.x * 4 + wv, nw = gridDim.x * 4;
  const int A = H.A;
  const go1_ppo_hyper hp = *H.hyper;
  const float invM = 1.0f / (float)H.M, eps = hp.clip_param;
  const float LOG_SQRT_2PI = 0.91893853320467274f;  // math.log(math.sqrt(2 * math.pi))
  const float* __restrict__ a3p = H.a3p;
  const float* __restrict__ a3c = H.a3c;
  const float* __restrict__ Bv = H.B;
  float w4[4][NA], w4c[4], gw4[4][NA], gw4c[4], db3[4], db3c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      w4[j][a] = a < A ? H.w4p[a * H3 + l + 32 * j] : 0.0f;
      gw4[j][a] = 0.0f;
    }
    w4c[j] = H.w4c[l + 32 * j];
    gw4c[j] = db3[j] = db3c[j] = 0.0f;
  }
  const float sgm = l < A ? H.std_[l] : 1.0f;  // lane a's std
  const float b4 = l < A ? H.b4p[l] : 0.0f, b4c = H.b4c[0];
  float db4 = 0.0f, dstd = 0.0f, db4cs = 0.0f, ls = 0.0f, lv = 0.0f, kls = 0.0f;
  uint32_t mxp = 0u, mxc = 0u;
  for (int m = 2 * gw + half; m < H.M + half; m += 2 * nw) {
    const bool valid = m < H.M;
    const int mr = valid ? m : H.M - 1;  // an out-of-range half computes row M - 1 and discards it
    float x[4], y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = a3p[(size_t)mr * H3 + l + 32 * j];
      y[j] = a3c[(size_t)mr * H3 + l + 32 * j];
    }
    const float* br = Bv + (size_t)mr * H.bw;
    const float xa = l < A ? br[l] : 0.0f, om = l < A ? br[A + l] : 0.0f, os = l < A ? br[2 * A + l] : 1.0f;
    const float old_logp = br[3 * A], adv = br[3 * A + 1], ret = br[3 * A + 2], tvv = br[3 * A + 3];
    float mua = 0.0f;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      float s = 0.0f;
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf(w4[j][a], x[j], s);
      s = half_sum(s);
      if (a == l) mua = s;
    }
    mua += b4;
    float V = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) V = fmaf(w4c[j], y[j], V);
    V = half_sum(V) + b4c;
    float lpa = 0.0f, kla = 0.0f, dx = 0.0f;
    if (l < A) {
      dx = xa - mua;
      const float var = sgm * sgm;
      // Normal.log_prob: -((value - loc) ** 2) / (2 * var) - log(scale) - log(sqrt(2 pi))
      lpa = (-(dx * dx) / (2.0f * var) - logf(sgm)) - LOG_SQRT_2PI;
      // KL (ppo.py:121-124): log(sigma / old_sigma + 1e-5) + (old_sigma^2 + (old_mu - mu)^2) / (2 sigma^2) - 0.5
      const float dm = om - mua;
      kla = (logf(sgm / os + 1.0e-5f) + (os * os + dm * dm) / (2.0f * (sgm * sgm))) - 0.5f;
    }
    const float logp = half_sum(lpa), kl = half_sum(kla);
    const float ratio = expf(logp - old_logp);
    const float s1 = -adv * ratio;
    const float rc = fminf(fmaxf(ratio, 1.0f - eps), 1.0f + eps);
    const float s2 = -adv * rc;
    const float w1 = s1 > s2 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
    const float w2 = s2 > s1 ? 1.0f : (s1 == s2 ? 0.5f : 0.0f);
    const float inr = (ratio >= 1.0f - eps && ratio <= 1.0f + eps) ? 1.0f : 0.0f;
    const float dlogp = valid ? (invM * (w1 * -adv + w2 * (-adv * inr))) * ratio : 0.0f;
    float dmu_a = 0.0f;
    if (l < A) {
      const float var = sgm * sgm;
      dmu_a = dlogp * (dx / var);
      dstd += dlogp * ((dx * dx) / (var * sgm) - 1.0f / sgm);
      db4 += dmu_a;
    }
    float dV, vl;
    if (hp.use_clipped_value_loss != 0.0f) {
      const float vc = tvv + fminf(fmaxf(V - tvv, -eps), eps);
      const float e1 = V - ret, e2 = vc - ret;
      const float l1 = e1 * e1, l2 = e2 * e2;
      vl = fmaxf(l1, l2);
      const float u1 = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f);
      const float u2 = l2 > l1 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f);
      const float dvi = V - tvv;
      const float vin = (dvi >= -eps && dvi <= eps) ? 1.0f : 0.0f;
      dV = hp.value_loss_coef * invM * (u1 * 2.0f * e1 + u2 * 2.0f * e2 * vin);
    } else {
      const float e = ret - V;
      vl = e * e;
      dV = hp.value_loss_coef * invM * (-2.0f * e);
    }
    if (!valid) dV = 0.0f;
    if (l == 0 && valid) {
      ls += fmaxf(s1, s2);
      lv += vl;
      kls += kl;
      db4cs += dV;
    }
    // backward through L4: every lane needs every dmu_a of its half
    float g[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) g[a] = a < A ? __shfl(dmu_a, a, 32) : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float tt = 0.0f;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        tt = fmaf(w4[j][a], g[a], tt);
        gw4[j][a] = fmaf(g[a], x[j], gw4[j][a]);
      }
      const float dp = tt * delu_from_out(x[j]);
      const float dc = (w4c[j] * dV) * delu_from_out(y[j]);
      gw4c[j] = fmaf(dV, y[j], gw4c[j]);
      db3[j] += dp;
      db3c[j] += dc;
      if (valid) {
        H.d3p[(size_t)m * H3 + l + 32 * j] = dp;
        H.d3c[(size_t)m * H3 + l + 32 * j] = dc;
        mxp = max(mxp, absbits(dp));
        mxc = max(mxc, absbits(dc));
      }
    }
  }
  mxp = wave_max_u32(mxp);
  mxc = wave_max_u32(mxc);
  if (lane == 0) {
    atomicMax(H.d3pmax, mxp);
    atomicMax(H.d3cmax, mxc);
  }
  // the two halves of the wave, then the block's four waves in LDS (fixed order)
  auto comb = [](float v) { return v + __shfl_xor(v, 32); };
  const int o_db4p = A * 128, o_db3p = o_db4p + A, o_dW4c = o_db3p + 128, o_db4c = o_dW4c + 128,
            o_db3c = o_db4c + 1, o_dstd = o_db3c + 128, o_loss = o_dstd + A;
  float* rw = red[wv];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = l + 32 * j;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const float v = comb(gw4[j][a]);
      if (half == 0 && a < A) rw[a * 128 + k] = v;
    }
    const float v1 = comb(db3[j]), v2 = comb(gw4c[j]), v3 = comb(db3c[j]);
    if (half == 0) {
      rw[o_db3p + k] = v1;
      rw[o_dW4c + k] = v2;
      rw[o_db3c + k] = v3;
    }
  }
  const float s_db4 = comb(db4), s_dstd = comb(dstd), s_db4c = comb(db4cs), s_ls = comb(ls), s_lv = comb(lv),
              s_kl = comb(kls);
  if (half == 0 && l < A) {
    rw[o_db4p + l] = s_db4;
    rw[o_dstd + l] = s_dstd;
  }
  if (lane == 0) {
    rw[o_db4c] = s_db4c;
    rw[o_loss + 0] = s_ls;
    rw[o_loss + 1] = s_lv;
    rw[o_loss + 2] = s_kl;
  }
  __syncthreads();
  float* part = H.part + (size_t)blockIdx.x * H.hstr;
  for (int e = threadIdx.x; e < H.hstr; e += 256) {
    float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    // the entropy term -entropy_coef * mean(sum_a (0.5 + 0.5 log 2 pi + log std_a)): d / d std_a = -coef / std_a
    if (blockIdx.x == 0 && e >= o_dstd && e < o_dstd + A) v += -hp.entropy_coef / H.std_[e - o_dstd];
    part[e] = v;
  }
}

// ------------------------------------------------------------------ the adaptation module's output layer
// MODE 0: latent = W3a a2a + b3a, written into the latent columns of G (the actor's input).  MODE 1 (phase 1):
// the same, then F.mse_loss against privileged_obs (G's priv columns) on rows < num_train (test loss on the
// rest) and its gradient.  MODE 0 / 1: a quarter-wave per row (four rows per wave step), lanes along the 128
// features of a2a (8 consecutive per lane).  MODE 2 (phase 0): d latent = W1p[:, hist:]^T delta1p (the actor's
// first layer, latent columns): a wave per row, lanes along its 512 outputs (8 per lane), two rows per step.
// MODE 1 / 2 then back-propagate through W3a: delta2a = (W3a^T g) * ELU'(a2a) with partial sums of dW3a, db3a,
// db2a.  Partial row [block][LSTR]: dW3a [P][128], db3a [P], db2a [128], loss train, loss test.
struct AdaptArgs {
  int32_t M, P, hist, num_train, ldg;
  const float* a2a;
  const float* w3a;
  const float* b3a;
  float* G;           // latent columns at hist .. hist + P (MODE 0 writes), priv at hist + P .. (MODE 1 reads)
  uint32_t* latmax;
  const float* d1p;   // MODE 2: [M][512]
  const float* w1p;   // MODE 2: (512, hist + P)
  const go1_ppo_hyper* hyper;
  float* d2a;
  uint32_t* d2amax;
  float* part;
  int32_t lstr;
};
__host__ __device__ constexpr int adapt_stride(int P) { return P * 128 + P + 128 + 2; }
constexpr int ADAPT_BLOCKS = 512;
struct AdaptPart {  // host: the offsets of that layout (adapt_kernel's o_*)
  int dW3a = 0, db3a, db2a, loss;
  explicit AdaptPart(int P) : db3a(P * 128), db2a(db3a + P), loss(db2a + 128) {}
};

template <int MODE>
__global__ __launch_bounds__(256) void adapt_kernel(AdaptArgs D) {
  __shared__ float red[4][adapt_stride(8)];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gw = blockIdx.x * 4 + wv, nw = gridDim.x * 4;
  const int P = D.P;
  const go1_ppo_hyper hp = *D.hyper;
  const int nsel = hp.selective != 0.0f ? 1 : P;
  const float* __restrict__ a2a = D.a2a;
  // MODE 0 / 1: quarter q4 = lane >> 4 owns a row, lane l = lane & 15 features 8 l .. 8 l + 7;
  // MODE 2: the wave owns a row pair, lane features k = lane, lane + 64 of a2a, outputs 8 lane .. of delta1p
  const int q4 = lane >> 4, l = lane & 15;
  constexpr int NF = MODE == 2 ? 2 : 8;  // a2a features per lane
  float w3[NF][8], gw3[NF][8], db2[NF];
#pragma unroll
  for (int u = 0; u < NF; ++u) {
    const int k = MODE == 2 ? lane + 64 * u : 8 * l + u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      w3[u][j] = j < P ? D.w3a[j * HA2 + k] : 0.0f;
      gw3[u][j] = 0.0f;
    }
    db2[u] = 0.0f;
  }
  float db3 = 0.0f, lt = 0.0f, lte = 0.0f;  // db3: lane j < P (MODE 2) / quarter-lane j < P (MODE 0 / 1)
  uint32_t mx = 0u;
  if (MODE == 0 || MODE == 1) {
    float b3[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b3[j] = j < P ? D.b3a[j] : 0.0f;
    const float inv = 1.0f / (float)(D.num_train * nsel);
    for (int m = 4 * gw + q4; m < D.M + q4; m += 4 * nw) {
      const bool valid = m < D.M;
      const int mr = valid ? m : D.M - 1;
      const f4_t x0 = *reinterpret_cast<const f4_t*>(a2a + (size_t)mr * HA2 + 8 * l);
      const f4_t x1 = *reinterpret_cast<const f4_t*>(a2a + (size_t)mr * HA2 + 8 * l + 4);
      const float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
      float yl = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float s = 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u) s = fmaf(w3[u][j], x[u], s);
        s = quarter_sum(s) + b3[j];
        if (j == l) yl = s;
      }
      float* grow = D.G + (size_t)mr * D.ldg + D.hist;
      if (MODE == 0) {
        if (valid && l < P) {
          grow[l] = yl;
          mx = max(mx, absbits(yl));
        }
        continue;
      }
      // F.mse_loss(pred[:nt, sel], target[:nt, sel]) (ppo.py:187-190): sel = every column, or column 0
      float gl = 0.0f;
      if (valid && l < nsel) {
        const float e = yl - grow[P + l];
        if (m < D.num_train) {
          gl = 2.0f * e * inv;
          lt += e * e;
        } else {
          lte += e * e;
        }
      }
      db3 += gl;
      float g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = j < P ? __shfl(gl, j, 16) : 0.0f;
      float d[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float tt = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          tt = fmaf(w3[u][j], g[j], tt);
          gw3[u][j] = fmaf(g[j], x[u], gw3[u][j]);
        }
        d[u] = tt * delu_from_out(x[u]);
        db2[u] += d[u];
        mx = max(mx, valid ? absbits(d[u]) : 0u);
      }
      if (valid) {
        *reinterpret_cast<f4_t*>(D.d2a + (size_t)m * HA2 + 8 * l) = (f4_t){d[0], d[1], d[2], d[3]};
        *reinterpret_cast<f4_t*>(D.d2a + (size_t)m * HA2 + 8 * l + 4) = (f4_t){d[4], d[5], d[6], d[7]};
      }
    }
  } else {
    float w1l[8][8];  // W1p[n][hist + j] for the lane's 8 outputs n = 8 lane .. 8 lane + 7
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) w1l[u][j] = j < P ? D.w1p[(size_t)(8 * lane + u) * (D.hist + P) + D.hist + j] : 0.0f;
    const float* __restrict__ d1p = D.d1p;
    for (int m0 = gw; m0 < D.M; m0 += 2 * nw) {
      const int mb = m0 + nw;
      const bool vb = mb < D.M;
      const int rows[2] = {m0, vb ? mb : m0};
      float dd[2][8], x[2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const f4_t d0 = *reinterpret_cast<const f4_t*>(d1p + (size_t)rows[t] * H1 + 8 * lane);
        const f4_t d1 = *reinterpret_cast<const f4_t*>(d1p + (size_t)rows[t] * H1 + 8 * lane + 4);
        dd[t][0] = d0[0]; dd[t][1] = d0[1]; dd[t][2] = d0[2]; dd[t][3] = d0[3];
        dd[t][4] = d1[0]; dd[t][5] = d1[1]; dd[t][6] = d1[2]; dd[t][7] = d1[3];
        x[t][0] = a2a[(size_t)rows[t] * HA2 + lane];
        x[t][1] = a2a[(size_t)rows[t] * HA2 + lane + 64];
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t == 1 && !vb) break;
        float g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float s = 0.0f;
#pragma unroll
          for (int u = 0; u < 8; ++u) s = fmaf(w1l[u][j], dd[t][u], s);
          g[j] = j < P ? wave_sum(s) : 0.0f;
          if (j == lane) db3 += g[j];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          float tt = 0.0f;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            tt = fmaf(w3[u][j], g[j], tt);
            gw3[u][j] = fmaf(g[j], x[t][u], gw3[u][j]);
          }
          const float d = tt * delu_from_out(x[t][u]);
          db2[u] += d;
          D.d2a[(size_t)rows[t] * HA2 + lane + 64 * u] = d;
          mx = max(mx, absbits(d));
        }
      }
    }
  }
  mx = wave_max_u32(mx);
  if (MODE == 0) {
    if (lane == 0) atomicMax(D.latmax, mx);
    return;
  }
  if (lane == 0) atomicMax(D.d2amax, mx);
  // quarters (MODE 1) combined by xor 16, 32; then the block's waves in LDS
  auto comb = [](float v) {
    if (MODE == 1) {
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
    }
    return v;
  };
  const int o_db3 = P * 128, o_db2 = o_db3 + P, o_loss = o_db2 + 128;
  float* rw = red[wv];
  const bool writer = MODE == 2 || q4 == 0;
#pragma unroll
  for (int u = 0; u < NF; ++u) {
    const int k = MODE == 2 ? lane + 64 * u : 8 * l + u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = comb(gw3[u][j]);
      if (writer && j < P) rw[j * 128 + k] = v;
    }
    const float v = comb(db2[u]);
    if (writer) rw[o_db2 + k] = v;
  }
  const float s_db3 = comb(db3), s_lt = comb(lt), s_lte = comb(lte);
  if (writer && (MODE == 2 ? lane : l) < P) rw[o_db3 + (MODE == 2 ? lane : l)] = s_db3;
  if (lane == 0) {
    rw[o_loss] = MODE == 1 ? s_lt : 0.0f;
    rw[o_loss + 1] = MODE == 1 ? s_lte : 0.0f;
  }
  if (MODE == 1) {  // the loss sums live on lanes l < nsel of each quarter: sum them across the quarter too
    float a = quarter_sum(l < nsel ? lt : 0.0f), b = quarter_sum(l < nsel ? lte : 0.0f);
    a += __shfl_xor(a, 16);
    a += __shfl_xor(a, 32);
    b += __shfl_xor(b, 16);
    b += __shfl_xor(b, 32);
    if (lane == 0) {
      rw[o_loss] = a;
      rw[o_loss + 1] = b;
    }
  }
  __syncthreads();
  float* part = D.part + (size_t)blockIdx.x * D.lstr;
  for (int e = threadIdx.x; e < D.lstr; e += 256) part[e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

}  // namespace
