// encoder.hip -- the height-map encoder of go1_gym_learn/ppo_cse_cnn for MI355X (gfx950): go1_heightmap_encode of
// include/go1_rollout.h, a second source of libgo1_rollout.so.
//
// Reference (ppo_cse_cnn/actor_critic.py):
//   HeightMapEncoder                 :27-62   MLP: Linear ELU Linear ELU; CNN: Conv ReLU Pool Conv ReLU Pool Linear
//   ActorCritic.process_obs_history  :180-198 policy_input = [scalars | scalars | embedding] of the last frame
//
// Two kernels, both on the 3xF16 split product of split_mfma.h (f32 accuracy on v_mfma_f32_16x16x32_f16):
//   enc_conv_kernel    one workgroup per env: map -> LDS, conv1 + ReLU + pool -> LDS, conv2 + ReLU + pool -> the
//                      feature scratch.  A conv is the GEMM [oc] x [ic * 9 + ky * 3 + kx] x [pixel]; the 16 pixel
//                      columns of an MFMA tile are four 2x2 pool windows, so bias, ReLU and the max stay in
//                      registers (two lane exchanges).
//   enc_linear_kernel  y = act(W x + b) for 32 envs x 128 outputs per workgroup (the weights are read n / 32
//                      times): the MLP's two layers and the CNN's linear; the last launch also copies the two
//                      scalar blocks of policy_input.
// Range guard as in the policy kernel: a workgroup that meets |x| >= 65504 (or a NaN) among the values it splits
// recomputes its outputs in f32 from the unsplit weights and counts itself in `overflow`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/go1_mi355x.h"
#include "../../include/go1_rollout.h"
#include "split_mfma.h"

int go1_rt_fail(int code, const std::string& m);  // rollout.hip: the library's error record

namespace {

constexpr int MAXX = GO1_MAX_SCAN_X, MAXY = GO1_MAX_SCAN_Y;
constexpr int C1 = 16, C2 = 32;            // conv channels (actor_critic.py:38, 41)
constexpr int K1 = 2 * 9, K2 = C1 * 9;     // conv GEMM depths: 18 (one K group), 144 (five)
constexpr int G2 = (K2 + 31) / 32;
constexpr int MAP_F = 2 * (MAXX + 2) * (MAXY + 2);               // the zero-bordered map
constexpr int P1_F = C1 * (MAXX / 2 + 2) * (MAXY / 2 + 2);       // the zero-bordered pooled conv1 output

__device__ __forceinline__ void split8(const float (&v)[8], h8_t& h, h8_t& l) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    h[r] = (_Float16)v[r];
    l[r] = (_Float16)(v[r] - (float)h[r]);
  }
}

// max over the four lanes of a pool window (lanes 4 w .. 4 w + 3 of the 16 pixel columns)
__device__ __forceinline__ float pool4(float v) {
  v = fmaxf(v, __shfl_xor(v, 1));
  return fmaxf(v, __shfl_xor(v, 2));
}

struct ConvArgs {
  const float* hist;  // obs_history + frame_off + n_scalar: the map of the last frame
  int64_t hist_ld;
  int X, Y;
  const void *w1, *w2;          // packed split weights
  const float *b1, *b2;         // biases padded to 16
  const float *wf1, *wf2;       // (16, 2, 3, 3), (32, 16, 3, 3) f32
  float* feat;                  // (n, n_feat)
  int n_feat;
  int* overflow;
};

// conv + ReLU + pool in f32 for the whole env (the range guard's path): src zero-bordered (IC, SX + 2, SY + 2),
// one (channel, window) per thread at a time; dst either the zero-bordered LDS plane set or the flattened features
template <int IC, int OC, bool TO_LDS>
__device__ __noinline__ void conv_pool_f32(const float* src, int SX, int SY, const float* __restrict__ wf,
                              const float* __restrict__ b, float* dst) {
  const int PX = SX / 2, PY = SY / 2, SYP = SY + 2, plane = (SX + 2) * SYP;
  for (int i = threadIdx.x; i < OC * PX * PY; i += blockDim.x) {
    const int oc = i / (PX * PY), w = i - oc * (PX * PY), wx = w / PY, wy = w - wx * PY;
    float best = 0.0f;  // ReLU: max(0, the window's values)
    for (int d = 0; d < 4; ++d) {
      const int x = 2 * wx + (d >> 1), y = 2 * wy + (d & 1);
      float acc = b[oc];
#pragma unroll 1
      for (int ic = 0; ic < IC; ++ic)
        for (int t = 0; t < 9; ++t)
          acc = fmaf(wf[(oc * IC + ic) * 9 + t], src[ic * plane + (x + t / 3) * SYP + y + t % 3], acc);
      best = acc > best || acc != acc ? acc : best;  // a NaN stays
    }
    if (TO_LDS)
      dst[oc * (PX + 2) * (PY + 2) + (wx + 1) * (PY + 2) + wy + 1] = best;
    else
      dst[i] = best;
  }
}

// two workgroups per CU (57 KB of LDS each): the kernel is a chain of LDS gathers, conversions and dependent MFMAs,
// and a second wave per SIMD fills the waits of the first; the rare f32 path stays out of line and rolled so that
// it does not set the register count
__global__ __launch_bounds__(256, 2) void enc_conv_kernel(ConvArgs A) {
  __shared__ float mp[MAP_F];
  __shared__ float p1[P1_F];
  __shared__ int ovf;
  const int env = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  const int X = A.X, Y = A.Y, YP = Y + 2, plane0 = (X + 2) * YP;
  const int X1 = X / 2, Y1 = Y / 2, Y1P = Y1 + 2, plane1 = (X1 + 2) * Y1P;
  const int X2 = X1 / 2, Y2 = Y1 / 2;
  if (tid == 0) ovf = 0;
  for (int i = tid; i < 2 * plane0; i += 256) mp[i] = 0.0f;
  for (int i = tid; i < C1 * plane1; i += 256) p1[i] = 0.0f;
  __syncthreads();
  {
    const float* src = A.hist + (int64_t)env * A.hist_ld;
    int bad = 0;
    for (int i = tid; i < 2 * X * Y; i += 256) {
      const int ch = i / (X * Y), r = i - ch * (X * Y), x = r / Y, y = r - x * Y;
      const float v = src[i];
      ovf_check(v, &bad);
      mp[ch * plane0 + (x + 1) * YP + y + 1] = v;
    }
    if (bad) ovf = 1;
  }
  // this lane's gather offsets: k = 32 g + 8 q + r -> (ic, ky, kx), relative to the pixel's top-left neighbour in the
  // zero-bordered source.  A padding k reads that neighbour itself (offset 0): a value inside the range guard
  // under a zero weight adds an exact 0, and the loads stay unconditional (a select per load made the compiler
  // branch around every one of them)
  int off1[8], off2[G2][8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int k = 8 * q + r;
    off1[r] = k < K1 ? (k / 9) * plane0 + ((k % 9) / 3) * YP + k % 3 : 0;
#pragma unroll
    for (int g = 0; g < G2; ++g) {
      const int k2 = 32 * g + k;
      off2[g][r] = k2 < K2 ? (k2 / 9) * plane1 + ((k2 % 9) / 3) * Y1P + k2 % 3 : 0;
    }
  }
  // the lane's pixel inside its window: the 16 columns of a tile are windows 4 t .. 4 t + 3, (dy, dx) in the low bits
  const int wsub = c >> 2, dy = (c >> 1) & 1, dx = c & 1;
  const f8_t w1 = reinterpret_cast<const f8_t*>(A.w1)[lane];
  const f4_t bias1 = *reinterpret_cast<const f4_t*>(A.b1 + 4 * q);
  __syncthreads();
  if (!ovf) {  // conv1: (2, X, Y) -> ReLU -> pool -> p1 (16, X1, Y1)
    const int nw = X1 * Y1;
    int bad = 0;
    // two tiles (t, t + 4) per pass: two independent gather -> split -> MFMA -> pool chains in flight; a tile
    // past the last window computes window 0 again and stores nothing
    for (int t = wave; 4 * t < nw; t += 8) {
      int w[2], wx[2], wy[2];
      f4_t acc[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        w[i] = 4 * (t + 4 * i) + wsub;
        const int wc = w[i] < nw ? w[i] : 0;
        wx[i] = wc / Y1;
        wy[i] = wc - wx[i] * Y1;
        const int base = (2 * wx[i] + dy) * YP + 2 * wy[i] + dx;
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mp[base + off1[r]];
        h8_t xh, xl;
        split8(v, xh, xl);
        acc[i] = mfma3(w1, xh, xl, bias1);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float m = fmaxf(pool4(acc[i][r]), 0.0f);
          if ((c & 3) == 0 && w[i] < nw) {
            ovf_check(m, &bad);
            p1[(4 * q + r) * plane1 + (wx[i] + 1) * Y1P + wy[i] + 1] = m;
          }
        }
    }
    if (bad) ovf = 1;
  }
  __syncthreads();
  float* feat = A.feat + (int64_t)env * A.n_feat;
  if (ovf) {  // uniform: read after the barrier that follows every write
    conv_pool_f32<2, C1, true>(mp, X, Y, A.wf1, A.b1, p1);
    __syncthreads();
    conv_pool_f32<C1, C2, false>(p1, X1, Y1, A.wf2, A.b2, feat);
    if (tid == 0 && A.overflow) atomicAdd(A.overflow, 1);
    return;
  }
  // conv2: (16, X1, Y1) -> ReLU -> pool -> features (32, X2, Y2), flattened as torch's Flatten
  f8_t w2[2][G2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int g = 0; g < G2; ++g) w2[j][g] = reinterpret_cast<const f8_t*>(A.w2)[(j * G2 + g) * 64 + lane];
  const f4_t bias2[2] = {*reinterpret_cast<const f4_t*>(A.b2 + 4 * q), *reinterpret_cast<const f4_t*>(A.b2 + 16 + 4 * q)};
  const int nw = X2 * Y2;
  for (int t = wave; 4 * t < nw; t += 4) {
    const int w = 4 * t + wsub, wc = w < nw ? w : 0, wx = wc / Y2, wy = wc - wx * Y2;
    const int base = (2 * wx + dy) * Y1P + 2 * wy + dx;
    f4_t acc[2] = {bias2[0], bias2[1]};
#pragma unroll
    for (int g = 0; g < G2; ++g) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = p1[base + off2[g][r]];
      h8_t xh, xl;
      split8(v, xh, xl);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = mfma3(w2[j][g], xh, xl, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float m = fmaxf(pool4(acc[j][r]), 0.0f);
        if ((c & 3) == 0 && w < nw) feat[(16 * j + 4 * q + r) * nw + w] = m;
      }
  }
}

// ------------------------------------------------------------------ linear layers
constexpr int LE = 32;       // envs per workgroup (two MFMA column tiles)
constexpr int LT = 8;        // output tiles of 16 per workgroup: two per wave
constexpr int LG = 8;        // K groups of 32 staged at a time (32 KB of split activations)

struct LinArgs {
  const float* in;   // (n, K) rows in_ld apart
  int64_t in_ld;
  int K, N;
  const void* w;     // packed [N / 16][K / 32][64][16] halves
  const float* b;    // padded to 16
  const float* wf;   // (N, K) f32
  int act;           // ELU on the outputs
  float* out;        // (n, N) rows out_ld apart
  int64_t out_ld;
  int n;
  int* overflow;
  // the two scalar blocks of policy_input (sc_n = 0: none): dst[e][0 .. S) = dst[e][S .. 2 S) = src[e][0 .. S)
  const float* sc_src;
  int64_t sc_ld;
  float* sc_dst;
  int64_t sc_dst_ld;
  int sc_n;
};

__global__ __launch_bounds__(256) void enc_linear_kernel(LinArgs A) {
  __shared__ h8_t xhi[4 * LG][LE];
  __shared__ h8_t xlo[4 * LG][LE];
  __shared__ int ovf;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  const int e0 = blockIdx.x * LE, K = A.K, N = A.N, G = (K + 31) / 32, NT = (N + 15) / 16;
  if (tid == 0) ovf = 0;
  if (A.sc_n > 0 && blockIdx.y == 0) {
    for (int i = tid; i < LE * A.sc_n; i += 256) {
      const int e = i / A.sc_n, j = i - e * A.sc_n;
      if (e0 + e < A.n) {
        const float v = A.sc_src[(int64_t)(e0 + e) * A.sc_ld + j];
        float* d = A.sc_dst + (int64_t)(e0 + e) * A.sc_dst_ld;
        d[j] = v;
        d[A.sc_n + j] = v;
      }
    }
  }
  int tile[2];
  bool live[2];
  f4_t acc[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int t = blockIdx.y * LT + wave + 4 * j;
    live[j] = t < NT;
    tile[j] = live[j] ? t : NT - 1;
    const f4_t b = *reinterpret_cast<const f4_t*>(A.b + 16 * tile[j] + 4 * q);
    acc[j][0] = b;
    acc[j][1] = b;
  }
  int bad = 0;
  for (int g0 = 0; g0 < G; g0 += LG) {
    // the chunk's weight fragments first: they depend on nothing staged, so they fly under the staging
    f8_t w[LG][2];
#pragma unroll
    for (int i = 0; i < LG; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int g = g0 + i < G ? g0 + i : G - 1;
        w[i][j] = reinterpret_cast<const f8_t*>(A.w)[((size_t)tile[j] * G + g) * 64 + lane];
      }
    __syncthreads();  // the previous chunk's planes are consumed (first pass: ovf = 0 is visible)
#pragma unroll
    for (int it = 0; it < 4 * LG * LE / 256; ++it) {
      const int item = tid + 256 * it, oct = item & (4 * LG - 1), e = item / (4 * LG);
      const int k0 = 32 * g0 + 8 * oct, row = e0 + e;
      float v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        v[r] = (row < A.n && k0 + r < K) ? A.in[(int64_t)row * A.in_ld + k0 + r] : 0.0f;
        ovf_check(v[r], &bad);
      }
      h8_t h, l;
      split8(v, h, l);
      xhi[oct][e] = h;
      xlo[oct][e] = l;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < LG; ++i) {
      if (g0 + i < G) {  // uniform
#pragma unroll
        for (int et = 0; et < 2; ++et) {
          const h8_t xh = xhi[4 * i + q][16 * et + c], xl = xlo[4 * i + q][16 * et + c];
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[j][et] = mfma3(w[i][j], xh, xl, acc[j][et]);
        }
      }
    }
  }
  if (bad) ovf = 1;
  __syncthreads();
  if (ovf) {  // f32 from the unsplit weights: this workgroup's envs x its outputs
    for (int i = tid; i < LE * LT * 16; i += 256) {
      const int o = blockIdx.y * LT * 16 + (i & (LT * 16 - 1)), row = e0 + i / (LT * 16);
      if (row >= A.n || o >= N) continue;
      const float* x = A.in + (int64_t)row * A.in_ld;
      const float* wr = A.wf + (size_t)o * K;
      float s = A.b[o];
      for (int k = 0; k < K; ++k) s = fmaf(wr[k], x[k], s);
      A.out[(int64_t)row * A.out_ld + o] = A.act ? elu(s) : s;
    }
    if (tid == 0 && A.overflow) atomicAdd(A.overflow, 1);
    return;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int et = 0; et < 2; ++et) {
      const int row = e0 + 16 * et + c;
      if (!live[j] || row >= A.n) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 16 * tile[j] + 4 * q + r;
        const float v = acc[j][et][r];
        if (o < N) A.out[(int64_t)row * A.out_ld + o] = A.act ? elu(v) : v;
      }
    }
}

int launch_linear(const LinArgs& L, hipStream_t s) {
  const dim3 grid((L.n + LE - 1) / LE, ((L.N + 15) / 16 + LT - 1) / LT);
  hipLaunchKernelGGL(enc_linear_kernel, grid, dim3(256), 0, s, L);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? GO1_OK_RT : go1_rt_fail(GO1_RT_E_HIP, hipGetErrorString(e));
}

}  // namespace

extern "C" {

void go1_encoder_abi_sizes(int64_t out[2]) {
  out[0] = sizeof(go1_policy_layer);
  out[1] = sizeof(go1_encoder_args);
}

int go1_heightmap_encode(const go1_encoder_args* args, void* stream) {
  const char* F = "go1_heightmap_encode: ";
  if (!args || args->n_envs <= 0 || !args->obs_history || !args->scratch || !args->policy_input)
    return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "bad argument");
  const go1_encoder_args& a = *args;
  if (a.mode != GO1_ENC_MLP && a.mode != GO1_ENC_CNN) return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "mode");
  if (a.map_x < 1 || a.map_x > MAXX)
    return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "map_x outside 1 .. GO1_MAX_SCAN_X");
  if (a.map_y < 1 || a.map_y > MAXY)
    return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "map_y outside 1 .. GO1_MAX_SCAN_Y");
  if (a.n_embed < 1 || a.n_embed > GO1_ENC_MAX_EMBED)
    return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "n_embed outside 1 .. 512");
  const int n_map = 2 * a.map_x * a.map_y;
  if (a.n_scalar < 0 || a.num_obs != a.n_scalar + n_map)
    return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "num_obs is not n_scalar + 2 * map_x * map_y");
  if (a.frame_off < 0) return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "frame_off < 0");
  if (a.hist_ld < a.frame_off + a.num_obs)
    return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "hist_ld < frame_off + num_obs");
  if (a.out_ld < 2 * (int64_t)a.n_scalar + a.n_embed)
    return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "out_ld < 2 * n_scalar + n_embed");
  if (a.mode == GO1_ENC_CNN) {
    const int feat = C2 * (a.map_x / 2 / 2) * (a.map_y / 2 / 2);
    if (feat < 1 || feat != a.n_feat)
      return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "the twice-pooled map has " + std::to_string(feat) +
                                           " features, the linear layer takes n_feat = " + std::to_string(a.n_feat));
  } else if (a.n_feat < 1 || a.n_feat > 4096) {
    return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "n_feat (the hidden width) outside 1 .. 4096");
  }
  const int nl = a.mode == GO1_ENC_CNN ? 3 : 2;
  for (int i = 0; i < nl; ++i)
    if (!a.layers[i].w || !a.layers[i].b || !a.layers[i].wf)
      return go1_rt_fail(GO1_RT_E_ARG, std::string(F) + "missing layer (split, bias and f32 weights are required)");
  hipStream_t s = (hipStream_t)stream;
  const float* frame = a.obs_history + a.frame_off;
  LinArgs last{};  // the layer that writes the embedding, and the scalar blocks with it
  last.in = a.scratch;
  last.in_ld = a.n_feat;
  last.K = a.n_feat;
  last.N = a.n_embed;
  last.w = a.layers[nl - 1].w;
  last.b = a.layers[nl - 1].b;
  last.wf = a.layers[nl - 1].wf;
  last.act = a.mode == GO1_ENC_MLP;
  last.out = a.policy_input + 2 * a.n_scalar;
  last.out_ld = a.out_ld;
  last.n = a.n_envs;
  last.overflow = a.overflow;
  last.sc_src = frame;
  last.sc_ld = a.hist_ld;
  last.sc_dst = a.policy_input;
  last.sc_dst_ld = a.out_ld;
  last.sc_n = a.n_scalar;
  if (a.mode == GO1_ENC_CNN) {
    ConvArgs cv{};
    cv.hist = frame + a.n_scalar;
    cv.hist_ld = a.hist_ld;
    cv.X = a.map_x;
    cv.Y = a.map_y;
    cv.w1 = a.layers[0].w;
    cv.b1 = a.layers[0].b;
    cv.wf1 = a.layers[0].wf;
    cv.w2 = a.layers[1].w;
    cv.b2 = a.layers[1].b;
    cv.wf2 = a.layers[1].wf;
    cv.feat = a.scratch;
    cv.n_feat = a.n_feat;
    cv.overflow = a.overflow;
    hipLaunchKernelGGL(enc_conv_kernel, dim3(a.n_envs), dim3(256), 0, s, cv);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return go1_rt_fail(GO1_RT_E_HIP, hipGetErrorString(e));
  } else {
    LinArgs first{};
    first.in = frame + a.n_scalar;
    first.in_ld = a.hist_ld;
    first.K = n_map;
    first.N = a.n_feat;
    first.w = a.layers[0].w;
    first.b = a.layers[0].b;
    first.wf = a.layers[0].wf;
    first.act = 1;
    first.out = a.scratch;
    first.out_ld = a.n_feat;
    first.n = a.n_envs;
    first.overflow = a.overflow;
    const int rc = launch_linear(first, s);
    if (rc) return rc;
  }
  return launch_linear(last, s);
}

}  // extern "C"
