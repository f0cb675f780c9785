// go1_actuator.h -- the actuator net on the matrix cores: weight fragments, their LDS parking, the MFMA groups.
#pragma once
#ifndef GO1_DEVICE_H
#error "include go1_device.h: its parts are not self-contained"
#endif
#pragma clang fp contract(off)  // pinned bit for bit to the oracle: torques are bit-identical

// ---------------------------------------------------------------- actuator net
// eval_actuator_network (:1311-1320) on the matrix cores.  One "group" = 16
// (env, joint) items; each item is carried by the 4 lanes {i, 16+i, 32+i, 48+i}
// of a wave (i = lane & 15, q = lane >> 4), exactly the v_mfma_f32_16x16x4_f32
// B-operand layout (B[k = q][item i]) and C/D layout (rows 4q..4q+3, column i).
//   layer 1: D = W1pad(32x8) . X(8x16): 2 M-tiles x 2 K-steps = 4 MFMA
//   layer 2: D = W2(32x32) . H1(32x16): each lane's layer-1 rows ARE its layer-2
//            B operand when the K-steps run over (m, r) with k = 16 m + 4 q + r,
//            so no data moves between the layers: 2 M-tiles x 8 K-steps = 16 MFMA
//   layer 3: per-lane fma over its 8 rows, then two xor-shuffles (16, 32).
// f32-input MFMA is bit-for-bit a k-ordered fmaf chain, and the oracle uses the
// same k order (oracle/go1_oracle.c go1o_actuator_eval): torques are bit-identical.

struct MlpFrag {
  float w1[2][2];  // [mo][s] = W1[16 mo + i][4 s + q]  (0 for k >= 6)
  float w2[2][8];  // [mo][4 m + r] = W2[16 mo + i][16 m + 4 q + r]
  f4 b1[2], b2[2]; // rows 4 q + r of tile mo
  float w3[2][4];  // w3[16 mo + 4 q + r]
  float b3;
};

__device__ __forceinline__ void mlp_load(const float* __restrict__ W, int lane, MlpFrag& F) {
  const int i = lane & 15, q = lane >> 4;
#pragma unroll
  for (int mo = 0; mo < 2; ++mo) {
#pragma unroll
    for (int sk = 0; sk < 2; ++sk) {
      const int k = 4 * sk + q;
      F.w1[mo][sk] = k < 6 ? W[(16 * mo + i) * 6 + k] : 0.0f;
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) F.w2[mo][4 * m + r] = W[224 + (16 * mo + i) * 32 + 16 * m + 4 * q + r];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      F.b1[mo][r] = W[192 + 16 * mo + 4 * q + r];
      F.b2[mo][r] = W[1248 + 16 * mo + 4 * q + r];
      F.w3[mo][r] = W[1280 + 16 * mo + 4 * q + r];
    }
  }
  F.b3 = W[1312];
}

// The fragments wait out each sub-step's physics in LDS (round 6): the loop's register peak (the self-collision narrow
// phase, the capsule search, the trunk faces) is at the VGPR + AGPR limit, and 45 values held across it made the
// compiler spill.  mlp_unpark re-reads them through an opaque pointer before each evaluation (48 x 64 floats per wave).
#define MLP_PARK_FLOATS ((int)(sizeof(MlpFrag) / sizeof(float)))
__device__ __forceinline__ void mlp_park(const MlpFrag& F, float* s, int lane) {
  const float* f = reinterpret_cast<const float*>(&F);
#pragma unroll
  for (int k = 0; k < MLP_PARK_FLOATS; ++k) s[k * 64 + lane] = f[k];
}
__device__ __forceinline__ void mlp_unpark(MlpFrag& F, const float* s, int lane) {
  // an opaque lane index: no forwarding of the parked values (they would stay live in registers).  (An opaque
  // pointer would hide that s is LDS: the reads then compile to flat loads, with their longer latency.)
  asm volatile("" : "+v"(lane));
  float* f = reinterpret_cast<float*>(&F);
#pragma unroll
  for (int k = 0; k < MLP_PARK_FLOATS; ++k) f[k] = s[k * 64 + lane];
}

// b0 = X[k = q][item], b1v = X[k = 4 + q][item] (0 for q >= 2).  Returns the torque
// of item (lane & 15) in all four lanes of the item.  Needs all 64 lanes active.
__device__ __forceinline__ float mlp_group(const MlpFrag& F, float b0, float b1v) {
  f4 a1[2];
#pragma unroll
  for (int mo = 0; mo < 2; ++mo) {
    a1[mo] = __builtin_amdgcn_mfma_f32_16x16x4f32(F.w1[mo][0], b0, F.b1[mo], 0, 0, 0);
    a1[mo] = __builtin_amdgcn_mfma_f32_16x16x4f32(F.w1[mo][1], b1v, a1[mo], 0, 0, 0);
  }
  float h1[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const f2 h = pm_softsign2(f2{a1[m][r], a1[m][r + 1]});
      h1[m][r] = h.x;
      h1[m][r + 1] = h.y;
    }
  f4 a2[2] = {F.b2[0], F.b2[1]};
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int mo = 0; mo < 2; ++mo)
        a2[mo] = __builtin_amdgcn_mfma_f32_16x16x4f32(F.w2[mo][4 * m + r], h1[m][r], a2[mo], 0, 0, 0);
  float h2[2][4];
#pragma unroll
  for (int mo = 0; mo < 2; ++mo)
#pragma unroll
    for (int r = 0; r < 4; r += 2) {
      const f2 h = pm_softsign2(f2{a2[mo][r], a2[mo][r + 1]});
      h2[mo][r] = h.x;
      h2[mo][r + 1] = h.y;
    }
  float p = 0.0f;
#pragma unroll
  for (int mo = 0; mo < 2; ++mo)
#pragma unroll
    for (int r = 0; r < 4; ++r) p = fmaf(F.w3[mo][r], h2[mo][r], p);
  return rowsum4(p) + F.b3;
}

// The three groups of a sub-step (joints 0..2) at once, layer by layer: 6 independent
// accumulator chains per layer keep the matrix pipe busy (one v_mfma_f32_16x16x4_f32 per
// 32 cycles per SIMD), and the softsign VALU of one group issues under the MFMAs of the
// next.  Each chain's k order is mlp_group's, so the torques are bit-identical to it.
__device__ __forceinline__ void mlp_group3(const MlpFrag& F, const float* b0, const float* b1v, float* t) {
  f4 a1[3][2];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int mo = 0; mo < 2; ++mo) a1[g][mo] = __builtin_amdgcn_mfma_f32_16x16x4f32(F.w1[mo][0], b0[g], F.b1[mo], 0, 0, 0);
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int mo = 0; mo < 2; ++mo) a1[g][mo] = __builtin_amdgcn_mfma_f32_16x16x4f32(F.w1[mo][1], b1v[g], a1[g][mo], 0, 0, 0);
  float h1[3][2][4];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const f2 h = pm_softsign2(f2{a1[g][m][r], a1[g][m][r + 1]});
        h1[g][m][r] = h.x;
        h1[g][m][r + 1] = h.y;
      }
  f4 a2[3][2];
#pragma unroll
  for (int g = 0; g < 3; ++g) { a2[g][0] = F.b2[0]; a2[g][1] = F.b2[1]; }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int mo = 0; mo < 2; ++mo)
          a2[g][mo] = __builtin_amdgcn_mfma_f32_16x16x4f32(F.w2[mo][4 * m + r], h1[g][m][r], a2[g][mo], 0, 0, 0);
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    float p = 0.0f;
#pragma unroll
    for (int mo = 0; mo < 2; ++mo)
#pragma unroll
      for (int r = 0; r < 4; r += 2) {
        const f2 h = pm_softsign2(f2{a2[g][mo][r], a2[g][mo][r + 1]});
        p = fmaf(F.w3[mo][r], h.x, p);
        p = fmaf(F.w3[mo][r + 1], h.y, p);
      }
    t[g] = rowsum4(p) + F.b3;
  }
  // the matrix pipe takes one v_mfma_f32_16x16x4_f32 per 32 cycles and the wave may issue ~6 VALU
  // instructions in that gap: layer 1 first, then each layer-2 MFMA followed by softsign work
#pragma unroll
  for (int i = 0; i < 12; ++i) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
#pragma unroll
  for (int i = 0; i < 48; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
  }
}
