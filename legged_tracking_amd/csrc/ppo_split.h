// ppo_split.h -- part of ppo_update.hip (the PPO update engine): the vector types and tile constants of its kernels,
// the power-of-two operand scaling and the 3xF16 split behind its GEMMs, the cross-lane reductions and ELU.
// (split_mfma.h is the rollout library's split: another ELU and another mfma3; the two are not interchangeable.)
#pragma once

namespace {

typedef float f4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef __fp16 hp2_t __attribute__((ext_vector_type(2)));

constexpr int TB = 128;      // GEMM tile: 128 rows x 128 features per workgroup (4 waves of 64 x 64)
constexpr int HA1 = GO1_PPO_HA1, HA2 = GO1_PPO_HA2, H1 = GO1_PPO_H1, H2 = GO1_PPO_H2, H3 = GO1_PPO_H3;
constexpr int NAUX = GO1_PPO_AUX;

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// A GEMM operand as the host hands it to the xw / wgrad problem builders: rows of 16-byte-loadable floats and the
// record(s) of max |x| its scale is derived from (mx2: an optional second record, G's computed columns).
struct Opnd {
  const float* p;
  int64_t ld;
  const uint32_t* mx;
  const uint32_t* mx2;
};

// ------------------------------------------------------------------ scaling and the 3xF16 split
// max |x| is tracked as the bit pattern of a non-negative float (ordered like an unsigned int; a NaN's bits
// exceed inf's, so a NaN operand disables the scaling and propagates).  scale exponent: max * 2^e in [2^14, 2^15).
__device__ __forceinline__ int scale_exp(uint32_t bits) {
  if (bits == 0u || bits >= 0x7f800000u) return 0;
  const int ef = (int)(bits >> 23);
  const int e = ef ? ef - 127 : (31 - __clz((int)bits)) - 149;
  const int s = 14 - e;
  return s < -126 ? -126 : (s > 126 ? 126 : s);
}
__device__ __forceinline__ float pow2f(int e) { return __int_as_float((e + 127) << 23); }  // e in [-126, 127]

__device__ __forceinline__ uint32_t absbits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// x * s split into f16 hi / lo halves.  hi rounds toward zero (v_cvt_pkrtz: one instruction per pair), so
// x - hi is exact and |lo| < ulp16(hi); lo rounds toward zero too: |x - hi - lo| < 2^-21 |x|.
__device__ __forceinline__ void split4(f4_t v, float s, h4_t& hi, h4_t& lo) {
  v *= s;
  const hp2_t h01 = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]);
  const hp2_t h23 = __builtin_amdgcn_cvt_pkrtz(v[2], v[3]);
  const hp2_t l01 = __builtin_amdgcn_cvt_pkrtz(v[0] - (float)h01[0], v[1] - (float)h01[1]);
  const hp2_t l23 = __builtin_amdgcn_cvt_pkrtz(v[2] - (float)h23[0], v[3] - (float)h23[1]);
  hi = __builtin_bit_cast(h4_t, __builtin_shufflevector(h01, h23, 0, 1, 2, 3));
  lo = __builtin_bit_cast(h4_t, __builtin_shufflevector(l01, l23, 0, 1, 2, 3));
}

__device__ __forceinline__ f4_t mfma3(h8_t wh, h8_t wl, h8_t xh, h8_t xl, f4_t acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc, 0, 0, 0);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ELU (alpha = 1) as torch's kernel: x > 0 ? x : expm1(x); its derivative from the output a: 1 or a + 1 = exp(x)
// expm1 for z <= 0 in ~14 instructions (ocml's expm1f is ~40, which made the ELU epilogue VALU-bound):
// z in [-0.5, 0]: degree-9 Taylor polynomial (truncation < 2^-27 relative); z < -0.5: exp(z) - 1 on v_exp_f32
// (|result| > 0.39, so the exp's ~1 ulp error stays ~2^-23 relative).  Within 2 ulp of expm1f on z <= 0.
__device__ __forceinline__ float expm1_neg(float z) {
  float p = 1.0f / 362880.0f;
  p = fmaf(p, z, 1.0f / 40320.0f);
  p = fmaf(p, z, 1.0f / 5040.0f);
  p = fmaf(p, z, 1.0f / 720.0f);
  p = fmaf(p, z, 1.0f / 120.0f);
  p = fmaf(p, z, 1.0f / 24.0f);
  p = fmaf(p, z, 1.0f / 6.0f);
  p = fmaf(p, z, 0.5f);
  const float small = fmaf(p * z, z, z);
  const float big = __builtin_amdgcn_exp2f(z * 1.44269504f) - 1.0f;
  return z >= -0.5f ? small : big;
}
__device__ __forceinline__ float elu(float z) {
  const float e = expm1_neg(fminf(z, 0.0f));  // unconditionally: a select, not a branch per value
  return z > 0.0f ? z : e;
}
__device__ __forceinline__ float delu_from_out(float a) { return a > 0.0f ? 1.0f : a + 1.0f; }

__device__ __forceinline__ float half_sum(float v) {  // sum over the 32 lanes of a half-wave
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}
__device__ __forceinline__ float quarter_sum(float v) {  // sum over the 16 lanes of a quarter-wave
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

}  // namespace
