// ppo_wgrad.h -- part of ppo_update.hip: the grouped weight-gradient GEMM (delta^T x activations, split over row
// chunks into partials), its problem builder and its launch.
#pragma once

namespace {

// ------------------------------------------------------------------ wgrad: partial[s] = sum over a row chunk of
// delta[m]^T x[m].  Both operands are row-major with the reduction (row) index strided, so they are staged as
// split f16 row-major LDS images [32 rows][128 columns] (16-byte chunks XOR-swizzled per row) and read back
// transposed with ds_read_b64_tr_b16: lane i of a 16-lane group receives column i of a 4-row block, i.e. 4
// consecutive rows (the MFMA K index) of one column.  MFMA roles: x columns (k) are the A operand rows,
// delta columns (n) the B operand columns: a lane's accumulator holds k = 4 q .. 4 q + 3 of one n, stored as
// one 16-byte write into partial[s][n][k].
struct WgProb {
  const float* x;
  int64_t ldx;
  int32_t k0;         // real x columns
  const uint32_t* xmax;
  const uint32_t* xmax2;  // optional second max (G's latent columns)
  const float* d;
  int64_t ldd;
  const uint32_t* dmax;
  float* part;        // [S][n][kpad]
  int64_t pstride;    // floats per chunk s
  int32_t kpad;       // row length of the partial (multiple of TB)
  int32_t tiles_k, tiles_n, tile0;
};
constexpr int MAX_WG = 10;  // phase 0 with an encoder: six head layers, two adaptation layers, two encoder layers
struct WgLaunch {
  WgProb p[MAX_WG];
  int32_t nprob, M, S, chunk, total;
};

typedef __fp16 v4hp_t __attribute__((__vector_size__(8)));  // the ds_read_tr16 builtin's operand type
typedef __attribute__((address_space(3))) v4hp_t lds_v4hp_t;

__device__ __forceinline__ int swz(int r) { return ((r & 3) | ((r >> 1) & 4)) << 1; }
// byte offset of the 4 halves at (row r, column 4 j) in a [32][128-half] image with swizzled 16-byte chunks
__device__ __forceinline__ int img_off(int r, int j4) { return r * 256 + 16 * ((j4 >> 1) ^ swz(r)) + 8 * (j4 & 1); }

__device__ __forceinline__ h8_t tr_frag(const char* base, int col0, int q, int i) {
  // rows 8 q .. 8 q + 7 of column col0 + i: two transposed 4-row reads
  const int r = i >> 2, p = i & 3;
  const int j4 = (col0 >> 2) + p;
  const h4_t a = __builtin_bit_cast(
      h4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_v4hp_t*)(base + img_off(8 * q + r, j4))));
  const h4_t b = __builtin_bit_cast(
      h4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_v4hp_t*)(base + img_off(8 * q + 4 + r, j4))));
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256, 2) void wgrad_kernel(WgLaunch L) {
  __shared__ __attribute__((aligned(16))) char sX[2][2][32 * 256];  // [buffer][plane] 8 KiB images
  __shared__ __attribute__((aligned(16))) char sD[2][2][32 * 256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, q = lane >> 4, c = lane & 15;
  int b = blockIdx.x, s, t;
  if ((L.S & 7) == 0) {
    const int bb = b >> 3;
    s = (b & 7) + 8 * (bb / L.total);
    t = bb % L.total;
  } else {
    s = b / L.total;
    t = b % L.total;
  }
  int pi = 0;
#pragma unroll
  for (int i = 1; i < MAX_WG; ++i)
    if (i < L.nprob && t >= L.p[i].tile0) pi = i;
  const WgProb& P = L.p[pi];
  const int lt = t - P.tile0, tk = lt / P.tiles_n, tn = lt - tk * P.tiles_n;
  const int wk = w & 1, wn = w >> 1;
  const int m_lo = s * L.chunk, m_hi = min(L.M, m_lo + L.chunk);
  const int eX = scale_exp(P.xmax2 ? max(*P.xmax, *P.xmax2) : *P.xmax), eD = scale_exp(*P.dmax);
  const float sx = pow2f(eX), sd = pow2f(eD);
  // k-tiles of this wave that hold real columns (the first layers' K is not a multiple of 128)
  const int kw0 = tk * TB + wk * 64;
  const int nkt = max(0, min(4, (P.k0 - kw0 + 15) >> 4));
  // staging: instruction j covers rows 2 j, 2 j + 1 of the wave's 8; lane -> row + (lane >> 5), float4 lane & 31
  const int col4 = lane & 31;
  const int kx = tk * TB + 4 * col4, kxc = min(kx, (int)P.ldx - 4);
  const int rsub = w * 8 + (lane >> 5);  // + 2 j
  const float* xb = P.x + kxc;
  const float* db = P.d + tn * TB + 4 * col4;
  // two register slots: the rows of group g + 1 are in flight while group g is multiplied, and group g + 2 is
  // requested before group g + 1 is split into LDS (every load unconditional: rows clamped, the last group
  // re-loaded past the end; out-of-range values zeroed in store(), after the MFMAs)
  f4_t sxv[2][4], sdv[2][4];
  int sm0[2] = {0, 0};
  const int ng = (m_hi - m_lo + 31) >> 5;
  auto load = [&](int slot, int g) {
    const int m0 = m_lo + min(g, ng - 1) * 32;
    sm0[slot] = m0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int mc = min(m0 + rsub + 2 * j, L.M - 1);
      sxv[slot][j] = *reinterpret_cast<const f4_t*>(xb + (size_t)mc * P.ldx);
      sdv[slot][j] = *reinterpret_cast<const f4_t*>(db + (size_t)mc * P.ldd);
    }
  };
  auto store = [&](int slot, int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = rsub + 2 * j;
      const float rm = sm0[slot] + r < m_hi ? 1.0f : 0.0f;
      f4_t vx = sxv[slot][j], vd = sdv[slot][j];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        vx[i] = kx + i < P.k0 ? vx[i] * rm : 0.0f;
        vd[i] = vd[i] * rm;
      }
      const int off = img_off(r, col4);
      h4_t hi, lo;
      split4(vx, sx, hi, lo);
      *reinterpret_cast<h4_t*>(&sX[buf][0][off]) = hi;
      *reinterpret_cast<h4_t*>(&sX[buf][1][off]) = lo;
      split4(vd, sd, hi, lo);
      *reinterpret_cast<h4_t*>(&sD[buf][0][off]) = hi;
      *reinterpret_cast<h4_t*>(&sD[buf][1][off]) = lo;
    }
  };
  f4_t acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int bq = 0; bq < 4; ++bq) acc[a][bq] = (f4_t){0.0f, 0.0f, 0.0f, 0.0f};
  auto mma = [&](int cur) {
    if (nkt > 0) {
      h8_t dh[4], dl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dh[j] = tr_frag(sD[cur][0], wn * 64 + j * 16, q, c);
        dl[j] = tr_frag(sD[cur][1], wn * 64 + j * 16, q, c);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < nkt) {
          const h8_t xh = tr_frag(sX[cur][0], wk * 64 + i * 16, q, c);
          const h8_t xl = tr_frag(sX[cur][1], wk * 64 + i * 16, q, c);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = mfma3(xh, xl, dh[j], dl[j], acc[i][j]);
        }
      }
    }
  };
  if (ng > 0) {
    load(0, 0);
    store(0, 0);
    load(1, 1);
    __syncthreads();
    for (int g = 0; g < ng; g += 2) {
      // slot 1 holds group g + 1; slot 0 is free
      load(0, g + 2);
      mma(0);
      store(1, 1);
      __syncthreads();
      if (g + 1 < ng) {
        // slot 0 holds group g + 2; slot 1 is free
        load(1, g + 3);
        mma(1);
        store(0, 0);
        __syncthreads();
      }
    }
  }
  const int sh = -(eX + eD);
  float* part = P.part + (size_t)s * P.pstride;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= nkt) continue;
    const int k = kw0 + i * 16 + 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = tn * TB + wn * 64 + j * 16 + c;
      f4_t v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ldexpf(acc[i][j][e], sh);
      *reinterpret_cast<f4_t*>(part + (size_t)n * P.kpad + k) = v;
    }
  }
}

// ------------------------------------------------------------------ host: one problem, one grouped launch
// partials [S][n][kpad] of delta^T x: x's k real columns, delta's n columns
WgProb wg_prob(Opnd x, int k, Opnd d, int n, float* part) {
  WgProb p{};
  p.x = x.p;
  p.ldx = x.ld;
  p.k0 = k;
  p.xmax = x.mx;
  p.xmax2 = x.mx2;
  p.d = d.p;
  p.ldd = d.ld;
  p.dmax = d.mx;
  p.part = part;
  p.kpad = cdiv(k, TB) * TB;
  p.pstride = (int64_t)n * p.kpad;
  p.tiles_k = p.kpad / TB;
  p.tiles_n = n / TB;
  return p;
}

// the problems' tiles times S row chunks of `chunk` rows
int launch_wg(hipStream_t s, int M, int S, int chunk, const WgProb* ps, int np) {
  WgLaunch L{};
  int total = 0;
  for (int i = 0; i < np; ++i) {
    L.p[i] = ps[i];
    L.p[i].tile0 = total;
    total += ps[i].tiles_k * ps[i].tiles_n;
  }
  L.nprob = np;
  L.M = M;
  L.S = S;
  L.chunk = chunk;
  L.total = total;
  hipLaunchKernelGGL(wgrad_kernel, dim3(total * S), dim3(256), 0, s, L);
  PPO_TRY(hipGetLastError());
  return GO1_PPO_OK;
}

}  // namespace
