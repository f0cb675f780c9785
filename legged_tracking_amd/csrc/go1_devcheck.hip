// go1_devcheck.hip -- TEST-ONLY library (libgo1_devcheck.so, tests/devcheck.py): thin kernels that apply one device
// function of go1_device.h per thread -- per wave for the lane helpers and the terrain queries -- to arrays, so the
// suite can compare the step kernels' building blocks with references on their own.  Not API: no public header, and
// nothing in the product loads it.  The headers keep their own fp-contract pragmas; what is written here is
// contract-off (go1_device.h ends that way) and does no arithmetic of its own beyond loads, stores and the
// d = P1 - P0 the callers of seg_closest form.
#include "go1_device.h"

#define DC_KERNEL extern "C" __global__ void __launch_bounds__(64)
#define DC_LAUNCH(kern, n, stream, ...)                                                   \
  do {                                                                                    \
    if ((n) <= 0) return 0;                                                               \
    hipLaunchKernelGGL(kern, dim3(((n) + 63) / 64), dim3(64), 0, (hipStream_t)(stream), __VA_ARGS__); \
    return hipGetLastError() == hipSuccess ? 0 : -1;                                      \
  } while (0)

// ---------------------------------------------------------------- portable math (contract off: bit for bit)
DC_KERNEL dc_pm1(int fn, const float* x, float* o0, float* o1, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  if (fn == 0) {
    float s, c;
    pm_sincosf(x[i], &s, &c);
    o0[i] = s;
    o1[i] = c;
  } else if (fn == 1) {
    o0[i] = pm_asinf(x[i]);
  } else if (fn == 2) {
    o0[i] = pm_atanf(x[i]);
  } else if (fn == 3) {
    o0[i] = pm_softsign(x[i]);
  } else if (fn == 4) {
    o0[i] = wrap_to_pi_f(x[i]);
  } else {  // hardware sin / cos of the integrator (contract on in its header; no a * b + c in it)
    float s, c;
    hw_sincosf(x[i], &s, &c);
    o0[i] = s;
    o1[i] = c;
  }
}
// fn 0: pm_atan2f(a, b), 1: remainder_f(a, b)
DC_KERNEL dc_pm2(int fn, const float* a, const float* b, float* o, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  o[i] = fn == 0 ? pm_atan2f(a[i], b[i]) : remainder_f(a[i], b[i]);
}
// pm_softsign2 on the pairs (x[2 i], x[2 i + 1])
DC_KERNEL dc_softsign2(const float* x, float* o, int npairs) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= npairs) return;
  const pm_f2 r = pm_softsign2(pm_f2{x[2 * i], x[2 * i + 1]});
  o[2 * i] = r.x;
  o[2 * i + 1] = r.y;
}
// fn 0: quat_rotate_inverse_f(q, v) -> o (n, 3); 1: quat_to_rpy_f(q) -> o (n, 3)
DC_KERNEL dc_quat(int fn, const float* q, const float* v, float* o, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float qq[4] = {q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
  float r[3];
  if (fn == 0) {
    const float vv[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    quat_rotate_inverse_f(qq, vv, r);
  } else {
    quat_to_rpy_f(qq, r);
  }
  o[3 * i] = r[0];
  o[3 * i + 1] = r[1];
  o[3 * i + 2] = r[2];
}

extern "C" int go1dc_pm1(int fn, const float* x, float* o0, float* o1, int n, void* stream) {
  if (fn < 0 || fn > 5) return -1;
  DC_LAUNCH(dc_pm1, n, stream, fn, x, o0, o1, n);
}
extern "C" int go1dc_pm2(int fn, const float* a, const float* b, float* o, int n, void* stream) {
  if (fn < 0 || fn > 1) return -1;
  DC_LAUNCH(dc_pm2, n, stream, fn, a, b, o, n);
}
extern "C" int go1dc_softsign2(const float* x, float* o, int npairs, void* stream) {
  DC_LAUNCH(dc_softsign2, npairs, stream, x, o, npairs);
}
extern "C" int go1dc_quat(int fn, const float* q, const float* v, float* o, int n, void* stream) {
  if (fn < 0 || fn > 1) return -1;
  DC_LAUNCH(dc_quat, n, stream, fn, q, v, o, n);
}

// ---------------------------------------------------------------- solve6p
// A: (n, 6, 6) symmetric, row-major; b, x: (n, 6); G: (n, 6, 6), what sip_get reads back from the packing.
// The packing: the two symmetric diagonal blocks in the halves of ac (xx xy xz yy yz zz), the upper right block in b.
DC_KERNEL dc_solve6(const float* A, const float* b, float* x, float* G, int n) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= n) return;
  const float* a = A + 36 * (size_t)e;
  SIP M;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) M.ac[s3i(i, j)] = f2{a[6 * i + j], a[6 * (i + 3) + (j + 3)]};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M.b[3 * i + j] = a[6 * i + (j + 3)];
  float bb[6], xx[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) bb[i] = b[6 * e + i];
  solve6p(M, bb, xx);
#pragma unroll
  for (int i = 0; i < 6; ++i) x[6 * e + i] = xx[i];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) G[36 * (size_t)e + 6 * i + j] = sip_get(M, i, j);
}
extern "C" int go1dc_solve6(const float* A, const float* b, float* x, float* G, int n, void* stream) {
  DC_LAUNCH(dc_solve6, n, stream, A, b, x, G, n);
}

// ---------------------------------------------------------------- lanes: one full wave per value set
// in: (nsets, 3, 64) floats; out: (nsets, DC_LANE_OUTS, 64) floats (quad_or's int as its bits), in the order
// qsum, rowsum4, rowsum4_n<3> x3, pairsum_rows_n<3> lo x3 hi x3, row1_bcast_n<2> x2, oddrows_sum_n<3> x3,
// quad_min, quad_max, quad_xor<1,2,3>, quad_or (of the bits of value 0)
#define DC_LANE_OUTS 22
DC_KERNEL dc_lanes(const float* in, float* out) {
  const int lane = threadIdx.x;
  const float* v = in + (size_t)blockIdx.x * 3 * 64;
  float* o = out + (size_t)blockIdx.x * DC_LANE_OUTS * 64 + lane;
  const float v0 = v[lane], v1 = v[64 + lane], v2 = v[128 + lane];
  int k = 0;
  o[64 * k++] = qsum(v0);
  o[64 * k++] = rowsum4(v0);
  {
    float w[3] = {v0, v1, v2};
    rowsum4_n<3>(w);
    for (int i = 0; i < 3; ++i) o[64 * k++] = w[i];
  }
  {
    const float w[3] = {v0, v1, v2};
    float lo[3], hi[3];
    pairsum_rows_n<3>(w, lo, hi);
    for (int i = 0; i < 3; ++i) o[64 * k++] = lo[i];
    for (int i = 0; i < 3; ++i) o[64 * k++] = hi[i];
  }
  {
    const float w[2] = {v0, v1};
    float r[2];
    row1_bcast_n<2>(w, r);
    for (int i = 0; i < 2; ++i) o[64 * k++] = r[i];
  }
  {
    float w[3] = {v0, v1, v2};
    oddrows_sum_n<3>(w);
    for (int i = 0; i < 3; ++i) o[64 * k++] = w[i];
  }
  o[64 * k++] = quad_min(v0);
  o[64 * k++] = quad_max(v0);
  o[64 * k++] = quad_xor<1>(v0);
  o[64 * k++] = quad_xor<2>(v0);
  o[64 * k++] = quad_xor<3>(v0);
  o[64 * k++] = __int_as_float(quad_or(__float_as_int(v0)));
  static_assert(DC_LANE_OUTS == 22, "the list above");
}
extern "C" int go1dc_lanes(const float* in, float* out, int nsets, void* stream) {
  if (nsets <= 0) return 0;
  hipLaunchKernelGGL(dc_lanes, dim3(nsets), dim3(64), 0, (hipStream_t)stream, in, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The role sums at the sizes the step kernels instantiate them with (they take their values two per swap: a lone
// value, one pair, and the kernels' even and odd counts).  in: (nsets, DC_LANEN_VALS, 64); out: (nsets, DC_LANEN_OUTS,
// 64), every call on the set's first N values, in the order rowsum4_n<1, 2, 6, 15>, pairsum_rows_n<1, 2, 27> (each: its
// N lo, then its N hi), row1_bcast_n<1, 2, 27>, oddrows_sum_n<1, 2, 21>
#define DC_LANEN_VALS 27
#define DC_LANEN_OUTS 138
template <int N>
__device__ __forceinline__ void dc_load_n(const float* v, int lane, float* w) {
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = v[64 * i + lane];
}
template <int N>
__device__ __forceinline__ float* dc_store_n(float* o, const float* w) {
#pragma unroll
  for (int i = 0; i < N; ++i) o[64 * i] = w[i];
  return o + 64 * N;
}
template <int N>
__device__ __forceinline__ float* dc_rowsum4_n(const float* v, int lane, float* o) {
  float w[N];
  dc_load_n<N>(v, lane, w);
  rowsum4_n<N>(w);
  return dc_store_n<N>(o, w);
}
template <int N>
__device__ __forceinline__ float* dc_pairsum_n(const float* v, int lane, float* o) {
  float w[N], lo[N], hi[N];
  dc_load_n<N>(v, lane, w);
  pairsum_rows_n<N>(w, lo, hi);
  return dc_store_n<N>(dc_store_n<N>(o, lo), hi);
}
template <int N>
__device__ __forceinline__ float* dc_row1_n(const float* v, int lane, float* o) {
  float w[N], r[N];
  dc_load_n<N>(v, lane, w);
  row1_bcast_n<N>(w, r);
  return dc_store_n<N>(o, r);
}
template <int N>
__device__ __forceinline__ float* dc_oddrows_n(const float* v, int lane, float* o) {
  float w[N];
  dc_load_n<N>(v, lane, w);
  oddrows_sum_n<N>(w);
  return dc_store_n<N>(o, w);
}
DC_KERNEL dc_lanes_n(const float* in, float* out) {
  const int lane = threadIdx.x;
  const float* v = in + (size_t)blockIdx.x * DC_LANEN_VALS * 64;
  float* o = out + (size_t)blockIdx.x * DC_LANEN_OUTS * 64 + lane;
  o = dc_rowsum4_n<1>(v, lane, o);
  o = dc_rowsum4_n<2>(v, lane, o);
  o = dc_rowsum4_n<6>(v, lane, o);
  o = dc_rowsum4_n<15>(v, lane, o);
  o = dc_pairsum_n<1>(v, lane, o);
  o = dc_pairsum_n<2>(v, lane, o);
  o = dc_pairsum_n<27>(v, lane, o);
  o = dc_row1_n<1>(v, lane, o);
  o = dc_row1_n<2>(v, lane, o);
  o = dc_row1_n<27>(v, lane, o);
  o = dc_oddrows_n<1>(v, lane, o);
  o = dc_oddrows_n<2>(v, lane, o);
  o = dc_oddrows_n<21>(v, lane, o);
  static_assert((1 + 2 + 6 + 15) + 2 * (1 + 2 + 27) + (1 + 2 + 27) + (1 + 2 + 21) == DC_LANEN_OUTS, "the list above");
}
extern "C" int go1dc_lanes_n(const float* in, float* out, int nsets, void* stream) {
  if (nsets <= 0) return 0;
  hipLaunchKernelGGL(dc_lanes_n, dim3(nsets), dim3(64), 0, (hipStream_t)stream, in, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------- segment geometry (contract on in go1_selfcol.h)
// P0, P1, Q0, Q1: (n, 3); st: (n, 2)
DC_KERNEL dc_seg_closest(const float* P0, const float* P1, const float* Q0, const float* Q1, float* st, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float p0[3] = {P0[3 * i], P0[3 * i + 1], P0[3 * i + 2]}, q0[3] = {Q0[3 * i], Q0[3 * i + 1], Q0[3 * i + 2]};
  // the directions as self_pair_force forms them
  const float d1[3] = {P1[3 * i] - p0[0], P1[3 * i + 1] - p0[1], P1[3 * i + 2] - p0[2]};
  const float d2[3] = {Q1[3 * i] - q0[0], Q1[3 * i + 1] - q0[1], Q1[3 * i + 2] - q0[2]};
  float s, t;
  seg_closest(p0, d1, q0, d2, s, t);
  st[2 * i] = s;
  st[2 * i + 1] = t;
}
// P0, P1: (n, 3); R: (n, 9) row-major base-to-world; pos: (n, 3); th: (3) half extents; t: (n)
DC_KERNEL dc_seg_box_t(const float* P0, const float* P1, const float* R, const float* pos, const float* th, float* t,
                       int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float p0[3], p1[3], r[9], ps[3];
  const float h[3] = {th[0], th[1], th[2]};
  for (int k = 0; k < 3; ++k) { p0[k] = P0[3 * i + k]; p1[k] = P1[3 * i + k]; ps[k] = pos[3 * i + k]; }
  for (int k = 0; k < 9; ++k) r[k] = R[9 * i + k];
  t[i] = seg_box_t(p0, p1, r, ps, h);
}
extern "C" int go1dc_seg_closest(const float* P0, const float* P1, const float* Q0, const float* Q1, float* st, int n,
                                 void* stream) {
  DC_LAUNCH(dc_seg_closest, n, stream, P0, P1, Q0, Q1, st, n);
}
extern "C" int go1dc_seg_box_t(const float* P0, const float* P1, const float* R, const float* pos, const float* th,
                               float* t, int n, void* stream) {
  DC_LAUNCH(dc_seg_box_t, n, stream, P0, P1, R, pos, th, t, n);
}

// ---------------------------------------------------------------- terrain queries: one wave per "env"
// Each env has its own tile view and patch corner; the wave stages its PSZX x PSZY patch in a plain loop under the
// product's convention (go1_step.hip: cell (li, lj) holds (floor = layer 1, ceiling = layer 0) of the tile at the
// clamped (pi0 + li, pj0 + lj)) -- from `stage`, which a test may point at another tile than the one the queries
// fall back to, to see which of the two a query read.  mode 0: patch and tile; 1: tile only (patch == nullptr);
// 2: the plane (tile == nullptr).  Lane l of env e runs queries e * 64 * nq + k * 64 + l, k < nq.
// env_i: (nenv, 5) ints: float offset of the tile in `tiles`, nx, ny, pi0, pj0.  pt: (N, 2); A, B: (N, 3); r: (N).
// hq: (N, 9): h floor, h ceiling, gx x2, gy x2, a, b, up.  seg_t: (N); seg_cell: (N) ints.
// hqc: (N, 6): hq_fetch_cell + hq_finish at the segment's chosen point and cell: h x2, gx x2, gy x2.
DC_KERNEL dc_terrain(int mode, const float* tiles, const float* stage, const int* env_i, float hs, int nq,
                     const float* pt, const float* A, const float* B, const float* r, float* hq, float* seg_t,
                     int* seg_cell, float* hqc) {
  __shared__ float2 s_patch[PSZX * PSZY];
  const int lane = threadIdx.x, e = blockIdx.x;
  const int off = env_i[5 * e], nx = env_i[5 * e + 1], ny = env_i[5 * e + 2], pi0 = env_i[5 * e + 3],
            pj0 = env_i[5 * e + 4];
  const float* st = stage + off;
  for (int c = lane; c < PSZX * PSZY; c += 64) {
    const int gi = min(max(pi0 + c / PSZY, 0), nx - 1), gj = min(max(pj0 + c % PSZY, 0), ny - 1);
    s_patch[c] = make_float2(st[((size_t)nx + gi) * ny + gj], st[(size_t)gi * ny + gj]);
  }
  __syncthreads();
  Terr T;
  T.tile = mode == 2 ? nullptr : tiles + off;
  T.nx = nx;
  T.ny = ny;
  T.hs = hs;
  T.patch = mode == 0 ? s_patch : nullptr;
  T.pi0 = pi0;
  T.pj0 = pj0;
  for (int k = 0; k < nq; ++k) {  // (a uniform trip count: every lane stays active for the wave votes)
    const size_t i = ((size_t)e * nq + k) * 64 + lane;
    {
      HQ q;
      f2 h, gx, gy;
      hq_fetch(T, pt[2 * i], pt[2 * i + 1], q);
      hq_finish(T, q, h, gx, gy);
      float* o = hq + 9 * i;
      o[0] = h.x; o[1] = h.y; o[2] = gx.x; o[3] = gx.y; o[4] = gy.x; o[5] = gy.y;
      o[6] = q.a; o[7] = q.b; o[8] = q.up ? 1.0f : 0.0f;
    }
    {
      const float a[3] = {A[3 * i], A[3 * i + 1], A[3 * i + 2]}, b[3] = {B[3 * i], B[3 * i + 1], B[3 * i + 2]};
      int cell;
      const float t = seg_deepest(T, a, b, r[i], cell);
      seg_t[i] = t;
      seg_cell[i] = cell;
      HQ q;
      f2 h, gx, gy;
      hq_fetch_cell(T, a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), cell, q);
      hq_finish(T, q, h, gx, gy);
      float* o = hqc + 6 * i;
      o[0] = h.x; o[1] = h.y; o[2] = gx.x; o[3] = gx.y; o[4] = gy.x; o[5] = gy.y;
    }
  }
}
extern "C" int go1dc_terrain(int mode, const float* tiles, const float* stage, const int* env_i, float hs, int nenv,
                             int nq, const float* pt, const float* A, const float* B, const float* r, float* hq,
                             float* seg_t, int* seg_cell, float* hqc, void* stream) {
  if (mode < 0 || mode > 2 || !(hs > 0.0f)) return -1;
  if (nenv <= 0 || nq <= 0) return 0;
  hipLaunchKernelGGL(dc_terrain, dim3(nenv), dim3(64), 0, (hipStream_t)stream, mode, tiles, stage, env_i, hs, nq, pt, A,
                     B, r, hq, seg_t, seg_cell, hqc);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------- the lane's segment pair: one wave per "env"
// The product's seg_deepest2 with the Terr set-up and modes of dc_terrain.  Lane l of env e passes its two segments
// (x, y halves) as the sub-step does, its role being l / 16: the x halves of rows 0 and 2 and both halves of their y
// take the full search, the others the short one (at most SEG_SHORT_MAX long).  A, B: (nenv * 64, 2, 3); r, seg_t:
// (nenv * 64, 2); seg_cell: (nenv * 64, 2) ints.  The radii reach the search's row layout by the exchange the ends
// take (the sub-step selects the model's there).
DC_KERNEL dc_seg_pair(int mode, const float* tiles, const float* stage, const int* env_i, float hs, const float* A,
                      const float* B, const float* r, float* seg_t, int* seg_cell) {
  __shared__ float2 s_patch[PSZX * PSZY];
  const int lane = threadIdx.x, e = blockIdx.x;
  const int off = env_i[5 * e], nx = env_i[5 * e + 1], ny = env_i[5 * e + 2], pi0 = env_i[5 * e + 3],
            pj0 = env_i[5 * e + 4];
  const float* st = stage + off;
  for (int c = lane; c < PSZX * PSZY; c += 64) {
    const int gi = min(max(pi0 + c / PSZY, 0), nx - 1), gj = min(max(pj0 + c % PSZY, 0), ny - 1);
    s_patch[c] = make_float2(st[((size_t)nx + gi) * ny + gj], st[(size_t)gi * ny + gj]);
  }
  __syncthreads();
  Terr T;
  T.tile = mode == 2 ? nullptr : tiles + off;
  T.nx = nx;
  T.ny = ny;
  T.hs = hs;
  T.patch = mode == 0 ? s_patch : nullptr;
  T.pi0 = pi0;
  T.pj0 = pj0;
  const size_t i = (size_t)e * 64 + lane;
  f2 a[3], b[3];
  for (int k = 0; k < 3; ++k) {
    a[k] = f2{A[6 * i + k], A[6 * i + 3 + k]};
    b[k] = f2{B[6 * i + k], B[6 * i + 3 + k]};
  }
  const f2 rr = f2{r[2 * i], r[2 * i + 1]};
  const LanePair rp = swap16(rr.x, rr.y);
  int cell[2];
  const f2 t = seg_deepest2(T, a, b, rr, f2{rp.a, rp.b}, cell);
  seg_t[2 * i] = t.x;
  seg_t[2 * i + 1] = t.y;
  seg_cell[2 * i] = cell[0];
  seg_cell[2 * i + 1] = cell[1];
}
extern "C" int go1dc_seg_pair(int mode, const float* tiles, const float* stage, const int* env_i, float hs, int nenv,
                              const float* A, const float* B, const float* r, float* seg_t, int* seg_cell,
                              void* stream) {
  if (mode < 0 || mode > 2 || !(hs >= SEG_MIN_HS)) return -1;
  if (nenv <= 0) return 0;
  hipLaunchKernelGGL(dc_seg_pair, dim3(nenv), dim3(64), 0, (hipStream_t)stream, mode, tiles, stage, env_i, hs, A, B, r,
                     seg_t, seg_cell);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
