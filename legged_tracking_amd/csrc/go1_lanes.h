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

// ---------------------------------------------------------------- role sums, two values per swap
// By 16-lane row, v_permlane16_swap(x, y) returns ([x0 y0 x2 y2], [x1 y1 x3 y3]) and v_permlane32_swap(x, y)
// returns ([x0 x1 y0 y1], [x2 x3 y2 y3]).  Called as swap(v, v) an exchange moves one value, wastes half of what it
// carries and costs a register copy (the instruction overwrites both operands).  The _n helpers below therefore
// take their N values two at a time, (x, y) = (v[2 j], v[2 j + 1]); an odd last value takes the (v, v) form.  They
// stay batched stage by stage (all swaps of a stage, then its adds), so no swap's latency or hazard nop is exposed.
// On every lane whose result is read, each addition has the operands, in the order, of the one-value forms:
// (r0 + r1) + (r2 + r3), or r1 + r3 with no zero added -- the bits are the same, signs of zero included.  Lanes of
// rows that hold the other member's partial sums compute sums nobody reads.
struct LanePair { float a, b; };
__device__ __forceinline__ LanePair swap16(float x, float y) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  return {__uint_as_float(r[0]), __uint_as_float(r[1])};
}
__device__ __forceinline__ LanePair swap32(float x, float y) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
  return {__uint_as_float(r[0]), __uint_as_float(r[1])};
}

// N independent row sums (r0 + r1) + (r2 + r3) on every lane.  Per pair: s = sum(swap16(x, y)) holds by row
// [x0 + x1, y0 + y1, x2 + x3, y2 + y3]; t = sum(swap32(s, s)) holds [X, Y, X, Y]; swap16(t, t) returns (X, Y) on
// every row.  3 swaps and 2 adds per pair where two values alone cost 4 and 4.
template <int N>
__device__ __forceinline__ void rowsum4_n(float* v) {
  constexpr int P = N / 2, M = P + (N & 1);  // pairs; pairs and the odd tail
  float s[M], t[M];
  LanePair r[M];
#pragma unroll
  for (int j = 0; j < P; ++j) r[j] = swap16(v[2 * j], v[2 * j + 1]);
  if (N & 1) r[P] = swap16(v[N - 1], v[N - 1]);
#pragma unroll
  for (int j = 0; j < M; ++j) s[j] = r[j].a + r[j].b;
#pragma unroll
  for (int j = 0; j < M; ++j) r[j] = swap32(s[j], s[j]);
#pragma unroll
  for (int j = 0; j < M; ++j) t[j] = r[j].a + r[j].b;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const LanePair o = swap16(t[j], t[j]);
    v[2 * j] = o.a;
    v[2 * j + 1] = o.b;
  }
  if (N & 1) v[N - 1] = t[P];
}

// N values that two bodies split between the row pairs (body L on rows 0-1, body H on rows 2-3): lo = r0 + r1 and
// hi = r2 + r3 on every lane.  Per pair: s = sum(swap16(x, y)) as above; (p, q) = swap32(s, s) are its rows
// [s0 s1 s0 s1] and [s2 s3 s2 s3]; swap16(p, p) returns (lo_x, lo_y) and swap16(q, q) (hi_x, hi_y) on every row.
// 4 swaps and 1 add per pair (4 and 2 for two values alone).
template <int N>
__device__ __forceinline__ void pairsum_rows_n(const float* v, float* lo, float* hi) {
  constexpr int P = N / 2, M = P + (N & 1);
  float s[M];
  LanePair r[M];
#pragma unroll
  for (int j = 0; j < P; ++j) r[j] = swap16(v[2 * j], v[2 * j + 1]);
  if (N & 1) r[P] = swap16(v[N - 1], v[N - 1]);
#pragma unroll
  for (int j = 0; j < M; ++j) s[j] = r[j].a + r[j].b;
#pragma unroll
  for (int j = 0; j < M; ++j) r[j] = swap32(s[j], s[j]);
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const LanePair l = swap16(r[j].a, r[j].a);
    lo[2 * j] = l.a;
    lo[2 * j + 1] = l.b;
  }
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const LanePair h = swap16(r[j].b, r[j].b);
    hi[2 * j] = h.a;
    hi[2 * j + 1] = h.b;
  }
  if (N & 1) { lo[N - 1] = r[P].a; hi[N - 1] = r[P].b; }
}

// Role "sums" of values that only some rows hold: no select zeroes the other rows and no zero is added (x + 0 = x;
// only a -0 keeps its sign here, where 0 + -0 gave +0).  What the other rows hold never reaches a result.
// N values of row 1 onto every lane.  Per pair: p = swap32(x, y)[0] = [x0 x1 y0 y1]; r = swap16(p, p)[1] =
// [x1 x1 y1 y1]; swap32(r, r) returns (x1, y1) on every row.  3 swaps per pair (4 for two values alone).
template <int N>
__device__ __forceinline__ void row1_bcast_n(const float* v, float* out) {
  constexpr int P = N / 2, M = P + (N & 1);
  float p[M];
#pragma unroll
  for (int j = 0; j < P; ++j) p[j] = swap32(v[2 * j], v[2 * j + 1]).a;
  if (N & 1) p[P] = v[N - 1];  // (the one-value form: rows 1 1 3 3 of v, then its rows 0-1)
#pragma unroll
  for (int j = 0; j < M; ++j) p[j] = swap16(p[j], p[j]).b;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const LanePair o = swap32(p[j], p[j]);
    out[2 * j] = o.a;
    out[2 * j + 1] = o.b;
  }
  if (N & 1) out[N - 1] = swap32(p[P], p[P]).a;
}
// N sums row 1 + row 3 on every lane (rowsum4_n's order with rows 0 and 2 absent).  Per pair: s = sum(swap32(x, y))
// holds x1 + x3 on row 1 and y1 + y3 on row 3; r = swap16(s, s)[1] = [s1 s1 s3 s3]; swap32(r, r) returns the two
// sums on every row.  3 swaps and 1 add per pair (4 and 2 for two values alone).
template <int N>
__device__ __forceinline__ void oddrows_sum_n(float* v) {
  constexpr int P = N / 2, M = P + (N & 1);
  float s[M];
  LanePair r[M];
#pragma unroll
  for (int j = 0; j < P; ++j) r[j] = swap32(v[2 * j], v[2 * j + 1]);
#pragma unroll
  for (int j = 0; j < P; ++j) s[j] = r[j].a + r[j].b;
  if (N & 1) s[P] = v[N - 1];  // (the one-value form: rows 1 1 3 3 of v, then row 1 + row 3)
#pragma unroll
  for (int j = 0; j < M; ++j) s[j] = swap16(s[j], s[j]).b;
#pragma unroll
  for (int j = 0; j < M; ++j) r[j] = swap32(s[j], s[j]);
#pragma unroll
  for (int j = 0; j < P; ++j) {
    v[2 * j] = r[j].a;
    v[2 * j + 1] = r[j].b;
  }
  if (N & 1) v[N - 1] = r[P].a + r[P].b;
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
