// ppo_conv.h -- part of ppo_update.hip: the CNN height-map encoder's convolution stack (ppo_cse_cnn/actor_critic.py:36-44)
// forward and backward for the update engine.  conv_pack_kernel (the filters' f16 fragment images) and conv_kernel.
//
//   map (2, 61, 31) -> conv1 3x3 pad 1 (2 -> 16) -> ReLU -> pool 2 -> (16, 30, 15)
//                   -> conv2 3x3 pad 1 (16 -> 32) -> ReLU -> pool 2 -> (32, 15, 7) = 3360 features
//
// conv_kernel: a workgroup takes a strip of consecutive rows and works on one row at a time entirely in LDS
// (128,492 bytes, 125.5 KiB of the CU's 160: one workgroup per CU).  No activation is stored per row: the forward is computed again
// from the map, the features leave as a by-product (`feat`), and the gradient of the features comes back through it:
//   1 map -> LDS (zero border), max |map|, max |d feat|
//   2 conv1 on MFMA, bias, pool winner, ReLU -> p1 (zero border) and the winner's index per window (arg1)
//   3 conv2 on MFMA, bias, pool winner, ReLU -> feat; d feat to the winner's pixel of dz (zero border, the
//     gradient before conv2's ReLU and pool; the window's other pixels take 0)
//   4 conv2 weight gradient  dW2[oc][ic ky kx] = sum_pixel dz[oc][pixel] p1[ic][pixel + (ky, kx) - 1]  on MFMA,
//     K = 30 x 16 pixel slots in 15 groups of 32 (the sixteenth y of a line is dz's zero border); bias gradient
//   5 conv2 data gradient  dp1[ic][pixel] = sum_{oc ky kx} W2[oc][ic][ky][kx] dz[oc][pixel - (ky, kx) + 1]  on MFMA,
//     K = 288 in 9 groups, over p1 (read for the last time in 4)
//   6 conv1 weight and bias gradient on the VALU: per window the winner's 18-value patch of the map times dp1.  K = 18
//     is a thin GEMM and the patch depends on the output channel (each has its own winner), so it is no GEMM on the
//     450 windows; on the 1800 pixels it would be one with 3/4 zero operands
// The GEMM operands are split into f16 hi / lo halves (ppo_split.h: mfma3) after an exact power-of-two scaling: the
// filters' by their tensor maximum (conv_pack_kernel), the map's, p1's and dz's by the row's maximum taken in LDS.
// The products are unscaled per row before they join the strip's f32 sums, so rows of any magnitude mix.
// Weight and bias gradients accumulate over the strip in registers and leave as one partial per workgroup
// ([dW2 | db2 | dW1 | db1], CV_PART floats); reduce_kernel sums the partials in workgroup order.  No float atomics:
// the result does not depend on the order in which workgroups or waves run.
// Pool ties take torch's rule: the first maximum in the order (0,0) (0,1) (1,0) (1,1), replaced only on strictly
// greater.  ReLU's gradient at 0 is 0.
#pragma once

namespace {

constexpr int CV_X = 61, CV_Y = 31;                  // the reference's map (2, 61, 31)
constexpr int CV_C1 = 16, CV_C2 = 32;                // conv channels
constexpr int CV_K1 = 2 * 9, CV_K2 = CV_C1 * 9;      // forward GEMM depths: 18 (one group of 32), 144 (five)
constexpr int CV_G2 = (CV_K2 + 31) / 32;
constexpr int CV_GD = CV_C2 * 9 / 32;                // the data gradient's depth 288: nine groups
constexpr int CV_X1 = CV_X / 2, CV_Y1 = CV_Y / 2;    // 30 x 15 after pool 1
constexpr int CV_X2 = CV_X1 / 2, CV_Y2 = CV_Y1 / 2;  // 15 x 7 after pool 2
constexpr int CV_NW1 = CV_X1 * CV_Y1, CV_NW2 = CV_X2 * CV_Y2;  // pool windows per channel: 450, 105
constexpr int CV_NMAP = 2 * CV_X * CV_Y, CV_NFEAT = CV_C2 * CV_NW2;  // 3782, 3360
constexpr int CV_MY = CV_Y + 2, CV_MPL = (CV_X + 2) * CV_MY;   // the zero-bordered map: line and plane stride
// the zero-bordered 30 x 15 planes (p1, dz): lines of 17, planes of 32 x 17 + 1.  The odd plane stride spreads the
// channels over the LDS banks; the extra element is the one a gather of the sixteenth y of the last line reaches
constexpr int CV_PY = CV_Y1 + 2, CV_PL = (CV_X1 + 2) * CV_PY + 1;
constexpr int CV_PART = CV_C2 * CV_K2 + CV_C2 + CV_C1 * CV_K1 + CV_C1;  // a workgroup's partial: 4944 floats
constexpr int CV_OFF_DB2 = CV_C2 * CV_K2, CV_OFF_DW1 = CV_OFF_DB2 + CV_C2, CV_OFF_DB1 = CV_OFF_DW1 + CV_C1 * CV_K1;
constexpr int CV_WG = 256;                           // workgroups of a launch at most: one per CU
// the filters' fragment images, 64 lanes x (hi, lo) h8 each: conv1 | conv2 [oc tile][group] | data gradient [group]
constexpr int CV_IMG1 = 0, CV_IMG2 = 2 * 64, CV_IMGD = CV_IMG2 + 2 * CV_G2 * 2 * 64;
constexpr int CV_IMG_N = CV_IMGD + CV_GD * 2 * 64;   // 2560 h8: 40 KiB

__device__ __forceinline__ void split8(const float (&v)[8], float s, h8_t& hi, h8_t& lo) {
  h4_t h0, l0, h1, l1;
  split4((f4_t){v[0], v[1], v[2], v[3]}, s, h0, l0);
  split4((f4_t){v[4], v[5], v[6], v[7]}, s, h1, l1);
  hi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
  lo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The pool window of a lane: the four lanes 4 w .. 4 w + 3 hold its pixels in the order (0,0) (0,1) (1,0) (1,1).
// Returns the window's maximum and the index of the first pixel that reaches it (torch: replaced on strictly greater)
__device__ __forceinline__ float pool_first_max(float z, int lane, int& idx) {
  const int b = lane & ~3;
  const float v0 = __shfl(z, b), v1 = __shfl(z, b + 1), v2 = __shfl(z, b + 2), v3 = __shfl(z, b + 3);
  float best = v0;
  idx = 0;
  if (v1 > best) best = v1, idx = 1;
  if (v2 > best) best = v2, idx = 2;
  if (v3 > best) best = v3, idx = 3;
  return best;
}

// ------------------------------------------------------------------ the filters' images
// MFMA A fragments (16 rows x 32 k; lane (q, c) holds row c, k = 8 q .. 8 q + 7), one 16-byte load per plane:
//   conv1  row oc, k = ic 9 + ky 3 + kx (18, zero beyond)          conv2  the same per 16 channels and K group
//   data gradient  row ic, k = oc 9 + ky 3 + kx (288): W2[oc][ic][ky][kx], the filters read across their outputs
struct ConvPack {
  const float *w1, *w2;  // (16, 2, 3, 3), (32, 16, 3, 3)
  h8_t* img;             // CV_IMG_N
  int32_t* wexp;         // [2] the filters' scale exponents
};

__global__ __launch_bounds__(256) void conv_pack_kernel(ConvPack P) {
  __shared__ uint32_t red[2][4];
  const int tid = threadIdx.x;
  uint32_t m1 = 0u, m2 = 0u;
  for (int i = tid; i < CV_C1 * CV_K1; i += 256) m1 = max(m1, absbits(P.w1[i]));
  for (int i = tid; i < CV_C2 * CV_K2; i += 256) m2 = max(m2, absbits(P.w2[i]));
  m1 = wave_max_u32(m1);
  m2 = wave_max_u32(m2);
  if ((tid & 63) == 0) red[0][tid >> 6] = m1, red[1][tid >> 6] = m2;
  __syncthreads();
  const int e1 = scale_exp(max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3])));
  const int e2 = scale_exp(max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));
  if (tid == 0) P.wexp[0] = e1, P.wexp[1] = e2;
  for (int i = tid; i < CV_IMG_N / 2; i += 256) {
    const int lane = i & 63, f = i >> 6, q = lane >> 4, c = lane & 15;
    float v[8];
    int es = e2;
    if (f == 0) {
      es = e1;
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = 8 * q + r < CV_K1 ? P.w1[c * CV_K1 + 8 * q + r] : 0.0f;
    } else if (f <= 2 * CV_G2) {
      const int j = (f - 1) / CV_G2, g = (f - 1) % CV_G2;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int k = 32 * g + 8 * q + r;
        v[r] = k < CV_K2 ? P.w2[(16 * j + c) * CV_K2 + k] : 0.0f;
      }
    } else {
      const int g = f - 1 - 2 * CV_G2;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int k = 32 * g + 8 * q + r, oc = k / 9, t = k - 9 * oc;
        v[r] = P.w2[(oc * CV_C1 + c) * 9 + t];
      }
    }
    h8_t hi, lo;
    split8(v, pow2f(es), hi, lo);
    P.img[f * 128 + lane] = hi;
    P.img[f * 128 + 64 + lane] = lo;
  }
}

// ------------------------------------------------------------------ forward and backward of a strip of rows
struct ConvArgs {
  const float* map;    // rows of CV_NMAP floats, ldm apart
  int64_t ldm;
  const float* dfeat;  // the loss gradient of the features, rows of CV_NFEAT, ldd apart; NULL: the forward alone
  int64_t ldd;         // (passes 1 - 3 without the gradient's part; no partial is written)
  float* feat;         // rows of CV_NFEAT, ldf apart; NULL: not wanted
  int64_t ldf;
  uint32_t* featmax;   // max feat joins this record (one atomic per wave and launch); NULL: not wanted
  const h8_t* img;     // conv_pack_kernel's
  const int32_t* wexp;
  const float *b1, *b2;
  float* part;         // [workgroups][CV_PART]
  int32_t rows, strip; // workgroup b takes rows b strip .. min(rows, (b + 1) strip)
};

__global__ __launch_bounds__(256, 1) void conv_kernel(ConvArgs A) {
  __shared__ float mp[2 * CV_MPL + 2];
  __shared__ float p1[CV_C1 * CV_PL];  // conv1's pooled output; from pass 5 on its gradient
  __shared__ float dz[CV_C2 * CV_PL];  // the gradient before conv2's ReLU and pool; at the end the scratch of dW1's sum
  __shared__ uint8_t arg1[CV_C1 * CV_NW1];  // pool 1: the winner's index, 4: stopped by the ReLU
  __shared__ uint32_t smax[3];         // the row's max |map|, max p1, max |d feat|
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, q = lane >> 4, c = lane & 15;
  const int wsub = c >> 2, dy = (c >> 1) & 1, dx = c & 1, dme = c & 3;
  for (int i = tid; i < 2 * CV_MPL + 2; i += 256) mp[i] = 0.0f;
  for (int i = tid; i < CV_C1 * CV_PL; i += 256) p1[i] = 0.0f;
  for (int i = tid; i < CV_C2 * CV_PL; i += 256) dz[i] = 0.0f;
  // gather offsets of this lane's k = 32 g + 8 q + r, relative to the pixel's top-left neighbour in the zero-bordered
  // source.  A padding k reads that neighbour itself under a zero weight
  int off1[8], off2[CV_G2][8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int k = 8 * q + r;
    off1[r] = k < CV_K1 ? (k / 9) * CV_MPL + ((k % 9) / 3) * CV_MY + k % 3 : 0;
#pragma unroll
    for (int g = 0; g < CV_G2; ++g) {
      const int k2 = 32 * g + k;
      off2[g][r] = k2 < CV_K2 ? (k2 / 9) * CV_PL + ((k2 % 9) / 3) * CV_PY + k2 % 3 : 0;
    }
  }
  const int e1 = A.wexp[0], e2 = A.wexp[1];
  const h8_t w1h = A.img[CV_IMG1 + lane], w1l = A.img[CV_IMG1 + 64 + lane];
  f4_t bias1, bias2[2];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    bias1[r] = A.b1[4 * q + r];
    bias2[0][r] = A.b2[4 * q + r];
    bias2[1][r] = A.b2[16 + 4 * q + r];
  }
  // the strip's sums.  dW2: this wave's k tiles wave, wave + 4 (, 8) x both channel tiles; db2: channel tid >> 3 (the
  // lanes with tid & 7 == 0 hold it); dW1, db1: channel tid & 15 over the windows = tid >> 4 (mod 16)
  f4_t tw2[3][2];
#pragma unroll
  for (int i = 0; i < 3; ++i) tw2[i][0] = tw2[i][1] = (f4_t){0.0f, 0.0f, 0.0f, 0.0f};
  float tb2 = 0.0f, tb1 = 0.0f, tw1[CV_K1];
#pragma unroll
  for (int k = 0; k < CV_K1; ++k) tw1[k] = 0.0f;

  const bool bwd = A.dfeat != nullptr;
  uint32_t fm = 0u;
  const int row0 = blockIdx.x * A.strip, row1 = min(A.rows, row0 + A.strip);
  for (int row = row0; row < row1; ++row) {
    const float* map = A.map + (int64_t)row * A.ldm;
    const float* dfeat = bwd ? A.dfeat + (int64_t)row * A.ldd : nullptr;
    __syncthreads();  // the previous row is done with mp, p1 and arg1 (first row: the buffers are cleared)
    if (tid < 3) smax[tid] = 0u;
    __syncthreads();
    // ---- 1 the map and the two maxima
    {
      uint32_t mm = 0u, md = 0u;
      for (int i = tid; i < CV_NMAP; i += 256) {
        const int ch = i / (CV_X * CV_Y), r = i - ch * (CV_X * CV_Y), x = r / CV_Y, y = r - x * CV_Y;
        const float v = map[i];
        mm = max(mm, absbits(v));
        mp[ch * CV_MPL + (x + 1) * CV_MY + y + 1] = v;
      }
      if (bwd)
        for (int i = tid; i < CV_NFEAT; i += 256) md = max(md, absbits(dfeat[i]));
      mm = wave_max_u32(mm);
      md = wave_max_u32(md);
      if (lane == 0) {
        atomicMax(&smax[0], mm);
        atomicMax(&smax[2], md);
      }
    }
    __syncthreads();
    // ---- 2 conv1: the 16 pixel columns of a tile are four pool windows x (dy, dx)
    {
      const int eM = scale_exp(smax[0]), sh = -(eM + e1);
      const float sM = pow2f(eM);
      uint32_t pm = 0u;
      for (int t = wave; 4 * t < CV_NW1; t += 4) {
        const int w = 4 * t + wsub, wc = w < CV_NW1 ? w : 0, wx = wc / CV_Y1, wy = wc - wx * CV_Y1;
        const int base = (2 * wx + dy) * CV_MY + 2 * wy + dx;
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = mp[base + off1[r]];
        h8_t xh, xl;
        split8(v, sM, xh, xl);
        const f4_t acc = mfma3(w1h, w1l, xh, xl, (f4_t){0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int idx;
          const float best = pool_first_max(ldexpf(acc[r], sh) + bias1[r], lane, idx);
          if (dme == 0 && w < CV_NW1) {
            const float m = best > 0.0f ? best : 0.0f;
            pm = max(pm, absbits(m));
            p1[(4 * q + r) * CV_PL + (wx + 1) * CV_PY + wy + 1] = m;
            arg1[(4 * q + r) * CV_NW1 + w] = (uint8_t)(best > 0.0f ? idx : 4);
          }
        }
      }
      pm = wave_max_u32(pm);
      if (lane == 0) atomicMax(&smax[1], pm);
    }
    __syncthreads();
    const int eP = scale_exp(smax[1]), eD = scale_exp(smax[2]);
    const float sP = pow2f(eP), sD = pow2f(eD);
    // ---- 3 conv2, the features, and d feat to the winners' pixels
    {
      const int sh = -(eP + e2);
      h8_t w2h[2][CV_G2], w2l[2][CV_G2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < CV_G2; ++g) {
          w2h[j][g] = A.img[CV_IMG2 + (j * CV_G2 + g) * 128 + lane];
          w2l[j][g] = A.img[CV_IMG2 + (j * CV_G2 + g) * 128 + 64 + lane];
        }
      float* feat = A.feat ? A.feat + (int64_t)row * A.ldf : nullptr;
      for (int t = wave; 4 * t < CV_NW2; t += 4) {
        const int w = 4 * t + wsub, wc = w < CV_NW2 ? w : 0, wx = wc / CV_Y2, wy = wc - wx * CV_Y2;
        const int base = (2 * wx + dy) * CV_PY + 2 * wy + dx;
        f4_t acc[2] = {(f4_t){0.0f, 0.0f, 0.0f, 0.0f}, (f4_t){0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int g = 0; g < CV_G2; ++g) {
          float v[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = p1[base + off2[g][r]];
          h8_t xh, xl;
          split8(v, sP, xh, xl);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[j] = mfma3(w2h[j][g], w2l[j][g], xh, xl, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int idx;
            const float best = pool_first_max(ldexpf(acc[j][r], sh) + bias2[j][r], lane, idx);
            if (w < CV_NW2) {
              const int oc = 16 * j + 4 * q + r;
              const bool win = idx == dme && best > 0.0f;
              if (bwd)
                dz[oc * CV_PL + (2 * wx + dy + 1) * CV_PY + 2 * wy + dx + 1] = win ? dfeat[oc * CV_NW2 + w] : 0.0f;
              const float m = best > 0.0f ? best : 0.0f;
              fm = max(fm, absbits(m));
              if (dme == 0 && feat) feat[oc * CV_NW2 + w] = m;
            }
          }
      }
    }
    if (!bwd) continue;  // uniform; the barriers at the head of the loop order the next row's writes
    __syncthreads();
    // ---- 4 conv2's bias and weight gradient
    {
      const float* zp = dz + (tid >> 3) * CV_PL + (tid & 7) * 68;  // 8 x 68 = the plane's 32 lines of 17
      float s = 0.0f;
      for (int i = 0; i < 68; ++i) s += zp[i];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 4);
      tb2 += s;
      f4_t acc[3][2];
#pragma unroll
      for (int i = 0; i < 3; ++i) acc[i][0] = acc[i][1] = (f4_t){0.0f, 0.0f, 0.0f, 0.0f};
      int offb[3];  // the B operand's column: k = 16 kt + c -> (ic, ky, kx)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int k = min(16 * (wave + 4 * i) + c, CV_K2 - 1);
        offb[i] = (k / 9) * CV_PL + ((k % 9) / 3) * CV_PY + k % 3;
      }
      for (int g = 0; g < CV_X1 / 2; ++g) {  // K group: the pixels (2 g + (q >> 1), 8 (q & 1) + r)
        const int pix = (2 * g + (q >> 1)) * CV_PY + 8 * (q & 1);
        h8_t ah[2], al[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float v[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = dz[(16 * j + c) * CV_PL + pix + CV_PY + 1 + r];
          split8(v, sD, ah[j], al[j]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          if (wave + 4 * i >= CV_K2 / 16) continue;  // uniform in the wave
          float v[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = p1[offb[i] + pix + r];
          h8_t bh, bl;
          split8(v, sP, bh, bl);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mfma3(ah[j], al[j], bh, bl, acc[i][j]);
        }
      }
      const int sh = -(eD + eP);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) tw2[i][j][r] += ldexpf(acc[i][j][r], sh);
    }
    __syncthreads();
    // ---- 5 conv2's data gradient over p1: a tile is the line x, y = c (the sixteenth is dropped)
    {
      const int sh = -(eD + e2);
      for (int x = wave; x < CV_X1; x += 4) {
        f4_t acc = (f4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int g = 0; g < CV_GD; ++g) {
          float v[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const int k = 32 * g + 8 * q + r, oc = k / 9, t = k - 9 * oc;
            v[r] = dz[oc * CV_PL + (x + 2 - t / 3) * CV_PY + c + 2 - t % 3];
          }
          h8_t xh, xl;
          split8(v, sD, xh, xl);
          acc = mfma3(A.img[CV_IMGD + g * 128 + lane], A.img[CV_IMGD + g * 128 + 64 + lane], xh, xl, acc);
        }
        if (c < CV_Y1)
#pragma unroll
          for (int r = 0; r < 4; ++r) p1[(4 * q + r) * CV_PL + (x + 1) * CV_PY + c + 1] = ldexpf(acc[r], sh);
      }
    }
    __syncthreads();
    // ---- 6 conv1's weight and bias gradient: the winner's patch of the map times the window's gradient
    {
      const int oc = tid & 15;
      for (int w = tid >> 4; w < CV_NW1; w += 16) {
        const int a = arg1[oc * CV_NW1 + w];
        if (a == 4) continue;
        const int wx = w / CV_Y1, wy = w - wx * CV_Y1;
        const float d = p1[oc * CV_PL + (wx + 1) * CV_PY + wy + 1];
        const float* src = mp + (2 * wx + (a >> 1)) * CV_MY + 2 * wy + (a & 1);
        tb1 += d;
#pragma unroll
        for (int k = 0; k < CV_K1; ++k)
          tw1[k] = fmaf(d, src[(k / 9) * CV_MPL + ((k % 9) / 3) * CV_MY + k % 3], tw1[k]);
      }
    }
  }
  if (A.featmax) {
    fm = wave_max_u32(fm);
    if (lane == 0) atomicMax(A.featmax, fm);
  }
  if (!bwd) return;
  // ---- the strip's partial
  float* part = A.part + (size_t)blockIdx.x * CV_PART;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int kt = wave + 4 * i;
    if (kt >= CV_K2 / 16) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(16 * j + 4 * q + r) * CV_K2 + 16 * kt + c] = tw2[i][j][r];
  }
  if ((tid & 7) == 0) part[CV_OFF_DB2 + (tid >> 3)] = tb2;
  __syncthreads();  // dz is free: [windows mod 16][channel][18 + 1]
  {
    float* sc = dz + ((tid >> 4) * CV_C1 + (tid & 15)) * (CV_K1 + 1);
#pragma unroll
    for (int k = 0; k < CV_K1; ++k) sc[k] = tw1[k];
    sc[CV_K1] = tb1;
  }
  __syncthreads();
  for (int i = tid; i < CV_C1 * (CV_K1 + 1); i += 256) {
    const int oc = i / (CV_K1 + 1), k = i - oc * (CV_K1 + 1);
    float s = 0.0f;
    for (int p = 0; p < 16; ++p) s += dz[(p * CV_C1 + oc) * (CV_K1 + 1) + k];
    part[k < CV_K1 ? CV_OFF_DW1 + oc * CV_K1 + k : CV_OFF_DB1 + oc] = s;
  }
}

// host: the launch's strip and workgroups for `rows` rows
inline int conv_strip(int rows) { return cdiv(rows, CV_WG); }
inline int conv_groups(int rows) { return cdiv(rows, conv_strip(rows)); }

int launch_conv(hipStream_t s, const ConvArgs& a) {
  hipLaunchKernelGGL(conv_kernel, dim3(conv_groups(a.rows)), dim3(256), 0, s, a);
  PPO_TRY(hipGetLastError());
  return GO1_PPO_OK;
}

}  // namespace
