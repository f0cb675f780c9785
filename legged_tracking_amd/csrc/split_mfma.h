// split_mfma.h -- the "3xF16" product of the rollout library's kernels (rollout.hip, encoder.hip): f32 accuracy
// from the f16 matrix cores of gfx950.  Every f32 weight and activation x is split into hi = f16(x) and
// lo = f16(x - hi) (22 significant bits together), and each 32-deep K group of a dot product is three
// v_mfma_f32_16x16x32_f16, acc += Whi Xhi + Whi Xlo + Wlo Xhi, with products exact in f32 and f32 accumulation;
// the dropped Wlo Xlo term is ~2^-22 of the product.
#ifndef GO1_SPLIT_MFMA_H
#define GO1_SPLIT_MFMA_H

#include <hip/hip_runtime.h>

namespace {

typedef float f4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h16_t __attribute__((ext_vector_type(16)));
typedef float f8_t __attribute__((ext_vector_type(8)));  // one lane's weight fragment (32 bytes)

// ELU's negative branch through the hardware exponential (v_exp_f32): exp(x) - 1 loses relative accuracy
// only where |x| is tiny, where its absolute error stays ~6e-8 (the outputs are checked at 2e-5 of their
// scale against f64); expm1f's range reduction cost ~25 instructions per value on the workgroups' tails
__device__ __forceinline__ float elu(float x) { return x > 0.0f ? x : __expf(x) - 1.0f; }

// Range guard of the split: f16(x) overflows for |x| >= 65520 (and a NaN / inf input has no split), so a
// value outside (-65504, 65504) sets the workgroup's flag; the workgroup then recomputes its envs in
// f32 from the unsplit weights at its end.  One compare per stored value.
__device__ __forceinline__ void ovf_check(float v, int* ovf) {
  if (!(fabsf(v) < 65504.0f)) *ovf = 1;
}

// acc += W x over one 32-deep K group: w = (8 hi, 8 lo) halves of the lane's A fragment (row lane & 15 of the
// 16-row weight tile, k = 8 (lane >> 4) + 0..7), xh / xl the lane's B fragment (column lane & 15, the same k);
// acc[r] is row 4 (lane >> 4) + r of column lane & 15
__device__ __forceinline__ f4_t mfma3(f8_t w, h8_t xh, h8_t xl, f4_t acc) {
  const h16_t wv = __builtin_bit_cast(h16_t, w);
  const h8_t wh = __builtin_shufflevector(wv, wv, 0, 1, 2, 3, 4, 5, 6, 7);
  const h8_t wl = __builtin_shufflevector(wv, wv, 8, 9, 10, 11, 12, 13, 14, 15);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc, 0, 0, 0);
}

}  // namespace
#endif  // GO1_SPLIT_MFMA_H
