// ppo_xw.h -- part of ppo_update.hip: the "xw" GEMM, activations x weights^T with the forward (bias, ELU / none) and
// backward (* ELU', column sums) epilogues, its problem builder and its launch.
#pragma once

namespace {

// ------------------------------------------------------------------ xw: C = act(A W^T + b) / (A W^T) * ELU'
// A: activations (M rows, row stride lda, k0 columns; the first layers read the gathered mini-batch rows G).
// W: the weight image of the pack kernel, [K / 32 groups][plane hi, lo][q = 0..3][n rows][8 halves]: lane (q, c)
// of a 16-row tile reads its A fragment of v_mfma_f32_16x16x32_f16 (row c, k = 8 q .. 8 q + 7) as one 16-byte
// load per plane.  MFMA roles: weights are the A operand (16 features), activations the B operand (16 rows); a
// lane's accumulator holds features 4 q .. 4 q + 3 of row c, stored as one 16-byte row-major write.
// Staging: the next 32-deep K group of the 128-row A tile is loaded (16-byte loads) while the current one is
// multiplied, split into hi / lo planes [q][row][8] in LDS; the weight fragments of a group are loaded at its
// start.  About 150 registers: two or three workgroups per CU overlap each other's loads and MFMAs.
struct XwProb {
  const float* a;
  int64_t lda;
  int32_t k0;                   // real columns (elements k >= k0 of a row are read as 0)
  const uint32_t* amax;
  const uint32_t* amax2;        // optional second max (G's latent columns)
  const h8_t* w;
  const int32_t* wexp;
  int32_t G;                    // K groups of 32 in the weight image
  int32_t n;                    // output features (multiple of TB)
  const float* bias;            // F epilogue
  const float* aprev;           // D epilogue: the forward activation whose ELU' multiplies
  int64_t ldp;
  float* c;
  int64_t ldc;
  uint32_t* cmax;
  float* colsum;                // D: [tiles_m][n] column sums of C
  int32_t tiles_n, tile0;
};
struct XwLaunch {
  XwProb p[2];
  int32_t nprob, M, total;
};

enum { EPI_LIN = 0, EPI_ELU = 1, EPI_DELU = 2 };

#ifdef PPO_STAMPS  // diagnostic build only (tools/xw_stamps.py): s_memrealtime per workgroup at kernel start,
                   // after the first staged group, after the K loop and after the epilogue
__device__ unsigned long long g_xw_stamps[8192][4];
#define XW_STAMP(i)                                                                                   \
  do {                                                                                                \
    if (threadIdx.x == 0 && blockIdx.x < 8192) g_xw_stamps[blockIdx.x][i] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define XW_STAMP(i)
#endif

template <int EPI>
__global__ __launch_bounds__(256, 2) void xw_kernel(XwLaunch L) {
  XW_STAMP(0);
  __shared__ h8_t sA[2][2][4][TB];  // [buffer][plane][q][row]: 32 KiB
  __shared__ float sRed[2][64];
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c = lane & 15;
  int t = blockIdx.x;
  if ((L.total & 7) == 0) t = (t & 7) * (L.total >> 3) + (t >> 3);  // one XCD walks consecutive row tiles
  const XwProb& P = (L.nprob > 1 && t >= L.p[1].tile0) ? L.p[1] : L.p[0];
  const int lt = t - P.tile0, mt = lt / P.tiles_n, nt = lt - mt * P.tiles_n;
  const int wm = w & 1, wn = w >> 1, M = L.M;
  int eA = 0, eW = 0;  // the operands' scale exponents: read after the first group's loads are issued
  float sa = 1.0f;
  // staging: per instruction 8 rows x 32 k; lane -> row (lane >> 1) & 7, float4 k4 = 2 (lane >> 4) + (lane & 1)
  const int srow = (lane >> 1) & 7, k4 = ((lane >> 4) << 1) | (lane & 1);
  const int mrow0 = mt * TB + w * 32 + srow;  // row of instruction it: mrow0 + 8 it
  // every load is unconditional (rows clamped to M - 1, columns to the row's last 16 bytes) and out-of-range
  // values are zeroed afterwards: a load under a branch makes hipcc wait for it (vmcnt(0)) right away
  const float* arow[4];
  float rmask[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int m = mrow0 + 8 * it;
    arow[it] = P.a + (size_t)min(m, M - 1) * P.lda;
    rmask[it] = m < M ? 1.0f : 0.0f;
  }
  const int kmax = (int)P.lda - 4;
  f4_t st[4];
  int stk = 0;  // first column of the staged group: the masks are applied in store(), after the MFMAs, so that the
                // loads stay in flight across them
  auto load = [&](int g) {
    const int k = g * 32 + 4 * k4, kc = min(k, kmax);
    stk = k;
#pragma unroll
    for (int it = 0; it < 4; ++it) st[it] = *reinterpret_cast<const f4_t*>(arow[it] + kc);
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      f4_t v = st[it];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (stk + i < P.k0) ? v[i] * rmask[it] : 0.0f;
      h4_t hi, lo;
      split4(v, sa, hi, lo);
      const int row = w * 32 + it * 8 + srow;
      reinterpret_cast<h4_t*>(&sA[buf][0][k4 >> 1][row])[k4 & 1] = hi;
      reinterpret_cast<h4_t*>(&sA[buf][1][k4 >> 1][row])[k4 & 1] = lo;
    }
  };
  const size_t npad = (size_t)P.n;
  const h8_t* wrow = P.w + (size_t)q * npad + nt * TB + wn * 64 + c;  // + (g * 2 + plane) * 4 * npad + 16 tn
  f4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (f4_t){0.0f, 0.0f, 0.0f, 0.0f};
  // the F epilogue's bias, loaded now: a load at the epilogue would be waited for right there
  f4_t bias4[4];
#pragma unroll
  for (int tn = 0; tn < 4; ++tn)
    bias4[tn] = EPI != EPI_DELU ? *reinterpret_cast<const f4_t*>(P.bias + nt * TB + wn * 64 + tn * 16 + 4 * q)
                                : (f4_t){0.0f, 0.0f, 0.0f, 0.0f};
  const int G = P.G;
  auto loadw = [&](int g, h8_t (&wh)[4], h8_t (&wl)[4]) {
    const h8_t* wg = wrow + (size_t)g * 8 * npad;
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
      wh[tn] = wg[tn * 16];
      wl[tn] = wg[4 * npad + tn * 16];
    }
  };
  auto mma = [&](int cur, const h8_t (&wh)[4], const h8_t (&wl)[4]) {
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
      const h8_t xh = sA[cur][0][q][wm * 64 + tm * 16 + c];
      const h8_t xl = sA[cur][1][q][wm * 64 + tm * 16 + c];
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) acc[tn][tm] = mfma3(wh[tn], wl[tn], xh, xl, acc[tn][tm]);
    }
  };
  load(0);
  // weight fragments and the A tile of the next group in flight across this group's MFMAs: every load is
  // unconditional (the last group re-loads itself), the LDS store of the staged group follows the MFMAs
  h8_t wh0[4], wl0[4], wh1[4], wl1[4];
  loadw(0, wh0, wl0);
  // the max |x| records (one dependent round trip) after the first group's loads are in flight
  eA = scale_exp(P.amax2 ? max(*P.amax, *P.amax2) : *P.amax);
  eW = *P.wexp;
  sa = pow2f(eA);
  store(0);
  __syncthreads();
  auto body = [&](int g, int cur, h8_t (&wh)[4], h8_t (&wl)[4], h8_t (&nwh)[4], h8_t (&nwl)[4]) {
    const int gn = min(g + 1, G - 1);
    loadw(gn, nwh, nwl);
    load(gn);
    mma(cur, wh, wl);
    store(cur ^ 1);
    __syncthreads();
  };
  XW_STAMP(1);
  for (int g = 0; g < G; g += 2) {
    body(g, 0, wh0, wl0, wh1, wl1);
    if (g + 1 < G) body(g + 1, 1, wh1, wl1, wh0, wl0);
  }
  XW_STAMP(2);
  // epilogue.  The D form's ELU' operand: the next column block's rows are requested while this one is
  // finished (clamped rows, unconditional: a load under the row test would be waited for at once); rows past
  // M only skip their store.
  const int sh = -(eA + eW);
  uint32_t amax = 0u;
  f4_t csum[4];
  f4_t ap[2][4];
  auto load_ap = [&](int tn, f4_t (&a)[4]) {
    const int n = nt * TB + wn * 64 + tn * 16 + 4 * q;
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
      const int mc = min(mt * TB + wm * 64 + tm * 16 + c, M - 1);
      a[tm] = *reinterpret_cast<const f4_t*>(P.aprev + (size_t)mc * P.ldp + n);
    }
  };
  if (EPI == EPI_DELU) load_ap(0, ap[0]);
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) {
    if (EPI == EPI_DELU && tn + 1 < 4) load_ap(tn + 1, ap[(tn + 1) & 1]);
    csum[tn] = (f4_t){0.0f, 0.0f, 0.0f, 0.0f};
    const int n = nt * TB + wn * 64 + tn * 16 + 4 * q;
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
      const int m = mt * TB + wm * 64 + tm * 16 + c;
      const bool in = m < M;
      f4_t v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = ldexpf(acc[tn][tm][i], sh);
      if (EPI == EPI_DELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = in ? v[i] * delu_from_out(ap[tn & 1][tm][i]) : 0.0f;
        csum[tn] += v;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float z = v[i] + bias4[tn][i];
          v[i] = EPI == EPI_ELU ? elu(z) : z;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) amax = max(amax, in ? absbits(v[i]) : 0u);
      if (in) *reinterpret_cast<f4_t*>(P.c + (size_t)m * P.ldc + n) = v;
    }
  }
  amax = wave_max_u32(amax);
  if (lane == 0) sMax[w] = amax;  // one atomic per workgroup (a single address takes them one at a time)
  __syncthreads();
  if (tid == 0 && P.cmax) atomicMax(P.cmax, max(max(sMax[0], sMax[1]), max(sMax[2], sMax[3])));
  XW_STAMP(3);
  if (EPI == EPI_DELU && P.colsum) {
    // column sums of this tile in a fixed order: the 16 rows of a lane group (xor tree), then wm = 0 + wm = 1
#pragma unroll
    for (int tn = 0; tn < 4; ++tn)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = csum[tn][i];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 8);
        csum[tn][i] = s;
      }
    if (wm == 1 && c == 0)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn)
#pragma unroll
        for (int i = 0; i < 4; ++i) sRed[wn][tn * 16 + 4 * q + i] = csum[tn][i];
    __syncthreads();
    if (wm == 0 && c == 0)
#pragma unroll
      for (int tn = 0; tn < 4; ++tn)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int f = tn * 16 + 4 * q + i;
          P.colsum[(size_t)mt * P.n + nt * TB + wn * 64 + f] = csum[tn][i] + sRed[wn][f];
        }
  }
}

// ------------------------------------------------------------------ host: one problem, one launch
// c (rows of ldc floats, n columns) from a's k columns against the image of an (n, k) weight.  The epilogue's
// operands (bias; aprev / ldp / colsum) are the caller's to add.
XwProb xw_prob(Opnd a, int k, const h8_t* img, const int32_t* wexp, int n, float* c, int64_t ldc, uint32_t* cmax) {
  XwProb p{};
  p.a = a.p;
  p.lda = a.ld;
  p.k0 = k;
  p.amax = a.mx;
  p.amax2 = a.mx2;
  p.w = img;
  p.wexp = wexp;
  p.G = cdiv(k, 32);
  p.n = n;
  p.c = c;
  p.ldc = ldc;
  p.cmax = cmax;
  p.tiles_n = n / TB;
  return p;
}

// one launch over the M rows of one problem or of two of the same epilogue (actor and critic)
int launch_xw(hipStream_t s, int M, int epi, const XwProb& p0, const XwProb* p1 = nullptr) {
  XwLaunch L{};
  L.p[0] = p0;
  L.p[0].tile0 = 0;
  L.nprob = 1;
  L.M = M;
  int total = cdiv(M, TB) * p0.tiles_n;
  if (p1) {
    L.p[1] = *p1;
    L.p[1].tile0 = total;
    L.nprob = 2;
    total += cdiv(M, TB) * p1->tiles_n;
  }
  L.total = total;
  if (epi == EPI_ELU)
    hipLaunchKernelGGL(xw_kernel<EPI_ELU>, dim3(total), dim3(256), 0, s, L);
  else if (epi == EPI_DELU)
    hipLaunchKernelGGL(xw_kernel<EPI_DELU>, dim3(total), dim3(256), 0, s, L);
  else
    hipLaunchKernelGGL(xw_kernel<EPI_LIN>, dim3(total), dim3(256), 0, s, L);
  PPO_TRY(hipGetLastError());
  return GO1_PPO_OK;
}

}  // namespace
