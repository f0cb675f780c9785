// go1_lanes.h -- Philox, lane-indexed selects and the cross-lane reductions (DPP quad moves, v_permlane16/32_swap).
// No arithmetic here can contract, so the integrator's quad helpers live here too.
#pragma once
#ifndef GO1_DEVICE_H
#error "include go1_device.h: its parts are not self-contained"
#endif
#pragma clang fp contract(off)  // pinned bit for bit to the oracle

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- Philox
__device__ __forceinline__ void philox4x32(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one v_mad_u64_u32 per product gives both halves (instead of v_mul_lo + v_mul_hi)
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t l0 = (uint32_t)p0, h0 = (uint32_t)(p0 >> 32), l1 = (uint32_t)p1, h1 = (uint32_t)(p1 >> 32);
    uint32_t n0 = h1 ^ c[1] ^ k0, n2 = h0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = l1; c[2] = n2; c[3] = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

struct Rng {
  const float* U;  // parity-mode uniforms or nullptr
  uint64_t seed, step;
  int e;    // local env index (parity-mode uniforms)
  int gid;  // global env id (Philox counter): local index + go1_config.env_id_offset
  int ustride;  // parity-mode uniform row width (go1_config.u_per_env)
  __device__ float operator()(int slot) const {
    if (U) return U[(size_t)e * ustride + slot];
    uint32_t c[4] = {(uint32_t)gid, (uint32_t)slot >> 2, (uint32_t)step, (uint32_t)(step >> 32)};
    philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(c[slot & 3] >> 8) * (1.0f / 16777216.0f);
  }
  // the four uniforms of slots 4 blk .. 4 blk + 3 (one Philox block), as operator() returns them
  __device__ void quad(int blk, float* u) const {
    if (U) {
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = U[(size_t)e * ustride + 4 * blk + k];
      return;
    }
    uint32_t c[4] = {(uint32_t)gid, (uint32_t)blk, (uint32_t)step, (uint32_t)(step >> 32)};
    philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = (float)(c[k] >> 8) * (1.0f / 16777216.0f);
  }
};

// ---------------------------------------------------------------- lane-indexed selects
// a[i] for a lane-dependent i in 0..3 as two levels of bit-test selects (v_cndmask): an
// equality chain (i == 0 ? .. : i == 1 ? ..) is turned into a switch with divergent branches
__device__ __forceinline__ float sel4(int i, float a0, float a1, float a2, float a3) {
  const bool lo = i & 1, hi = i & 2;
  return hi ? (lo ? a3 : a2) : (lo ? a1 : a0);
}
__device__ __forceinline__ float sel3(int i, const float* a) { return sel4(i, a[0], a[1], a[2], a[2]); }

// ---------------------------------------------------------------- quad helpers
// sum over the quad (lanes xor 1, 2) in the order (l0 + l1) + (l2 + l3); DPP quad_perm
// moves stay in the VALU (no LDS round trip)
__device__ __forceinline__ float qsum(float v) {
  // update_dpp(0, ., bound_ctrl) lets the compiler fold the move into the add (v_add_f32_dpp)
  v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));  // [1,0,3,2]
  v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));  // [2,3,0,1]
  return v;
}

// sum over the four 16-lane rows, (r0 + r1) + (r2 + r3): gfx950 v_permlane16/32_swap
__device__ __forceinline__ float rowsum4(float p) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(p), __float_as_uint(p), false, false);
  p = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(p), __float_as_uint(p), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// N independent row sums stage by stage (all permlane16 swaps, then their adds, then the
// permlane32 stage): one value at a time, every sum paid a register copy, a hazard nop and
// the full swap latency, twice
template <int N>
__device__ __forceinline__ void rowsum4_n(float* v) {
  float a[N], b[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i]), false, false);
    a[i] = __uint_as_float(r[0]);
    b[i] = __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = a[i] + b[i];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i]), false, false);
    a[i] = __uint_as_float(r[0]);
    b[i] = __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = a[i] + b[i];
}

// N values that two bodies split between the row pairs (body L on rows 0-1, body H on rows 2-3):
// the permlane16 stage sums each pair, then one permlane32 swap hands every lane both results --
// its two outputs are the low-half value (rows 0-1) and the high-half value (rows 2-3) on every
// lane.  Three VALU per value where two full row sums cost eight.
template <int N>
__device__ __forceinline__ void pairsum_rows_n(const float* v, float* lo, float* hi) {
  float a[N], b[N], s[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i]), false, false);
    a[i] = __uint_as_float(r[0]);
    b[i] = __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) s[i] = a[i] + b[i];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(s[i]), __float_as_uint(s[i]), false, false);
    lo[i] = __uint_as_float(r[0]);
    hi[i] = __uint_as_float(r[1]);
  }
}

// Role "sums" of values that only some rows hold.  v_permlane16_swap(v, v) returns (rows 0 0 2 2, rows 1 1 3 3) of
// v: its second output already carries the odd rows, so these take no select to zero the other rows and no add of
// those zeros (x + 0 = x; only a -0 keeps its sign here, where 0 + -0 gave +0).
// N values of row 1 onto every lane: one v_permlane32_swap spreads the second output's rows 0-1.
template <int N>
__device__ __forceinline__ void row1_bcast_n(const float* v, float* out) {
  float b[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i]), false, false);
    b[i] = __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(b[i]), __float_as_uint(b[i]), false, false);
    out[i] = __uint_as_float(r[0]);
  }
}
// N sums row 1 + row 3 on every lane (rowsum4_n's order with rows 0 and 2 zero)
template <int N>
__device__ __forceinline__ void oddrows_sum_n(float* v) {
  float a[N], b[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i]), false, false);
    b[i] = __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(b[i]), __float_as_uint(b[i]), false, false);
    a[i] = __uint_as_float(r[0]);
    b[i] = __uint_as_float(r[1]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = a[i] + b[i];
}

// min / max / or over the quad and the value of lane ^ D within it (DPP quad_perm)
__device__ __forceinline__ float quad_min(float v) {
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true)));
  return fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true)));
}
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true)));
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true)));
}
template <int D>
__device__ __forceinline__ float quad_xor(float v) {  // the value of lane ^ D within the quad (DPP quad_perm)
  constexpr int c = D == 1 ? 0xB1 : (D == 2 ? 0x4E : 0x1B);
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), c, 0xF, 0xF, true));
}
__device__ __forceinline__ int quad_or(int v) {
  v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
  return v | __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
}
