// go1_spatial.h -- spatial algebra of the native articulated-body integrator (f32): fast reciprocals and sin / cos,
// joint rotations and transforms, the packed (f2) spatial inertia and its 6 x 6 solve.
// FMA contraction is on in every integrator header, so in the helpers inlined into phys_substep too (a pragma inside
// phys_substep alone does not reach them).
#pragma once
#ifndef GO1_DEVICE_H
#error "include go1_device.h: its parts are not self-contained"
#endif
#pragma clang fp contract(on)  // integrator code, compared with the f64 oracle within a tolerance

// Spatial vectors (angular; linear).  6x6 symmetric articulated inertia stored as
// [[A, B], [B^T, C]], A and C symmetric (xx xy xz yy yz zz), B row-major 3x3.
struct SI {
  float a[6], b[9], c[6];
};

// Integrator-only fast math (hardware v_rcp_f32 / v_rsq_f32, ~1 ulp): the f32
// integrator is compared with the f64 oracle within a tolerance, never bitwise.
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
// hardware v_sin_f32 / v_cos_f32 on the angle in revolutions reduced to [0, 1) by v_fract_f32:
// 5 issue slots instead of the portable polynomial's ~25 (integrator only; absolute error 7.3e-7 over the joint
// range |x| <= 8, growing by 2^-22 |x| -- the rounding of x / 2 pi, which fract cannot recover: measured in
// tests/test_gpu_device_math.py; the step is compared with the f64 oracle within a tolerance)
__device__ __forceinline__ void hw_sincosf(float x, float* s, float* c) {
  const float r = __builtin_amdgcn_fractf(x * 0.159154943091895336f);
  *s = __builtin_amdgcn_sinf(r);
  *c = __builtin_amdgcn_cosf(r);
}
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }

__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
  float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}

// rigid-body spatial inertia about the link origin
__device__ __forceinline__ void rigid_si(const float* body, float mscale, SI& I) {
  float m = body[0] * mscale;
  float c0 = body[1], c1 = body[2], c2 = body[3];
  float cc = c0 * c0 + c1 * c1 + c2 * c2;
  I.a[0] = body[4] * mscale + m * (cc - c0 * c0);
  I.a[1] = body[5] * mscale - m * c0 * c1;
  I.a[2] = body[6] * mscale - m * c0 * c2;
  I.a[3] = body[7] * mscale + m * (cc - c1 * c1);
  I.a[4] = body[8] * mscale - m * c1 * c2;
  I.a[5] = body[9] * mscale + m * (cc - c2 * c2);
  // B = m c~
  // structural zeros as -0.0: the compiler folds x + (-0.0) = x in sip_add, not x + (+0.0)
  I.b[0] = -0.0f; I.b[1] = -m * c2; I.b[2] = m * c1;
  I.b[3] = m * c2; I.b[4] = -0.0f; I.b[5] = -m * c0;
  I.b[6] = -m * c1; I.b[7] = m * c0; I.b[8] = -0.0f;
  I.c[0] = m; I.c[1] = -0.0f; I.c[2] = -0.0f; I.c[3] = m; I.c[4] = -0.0f; I.c[5] = m;
}

// Rigid-body bias force v x* (I v) of a body (mass m, COM c, inertia Ic about the COM; model layout) from its
// momentum, without building the 6x6 inertia:
//   p = m (v + w x c),  L = Ic w + c x p,  v x* (L, p) = (w x L + v x p, w x p).
// The velocity and the result are (angular, linear) pairs: the two products with w, w x L and w x p, run as one
// packed cross product of w with the (L, p) pairs
__device__ __forceinline__ void rigid_bias2(const float* body, const f2* vel, f2* o, float mscale = 1.0f) {
  const float m = body[0] * mscale;
  const float* c = body + 1;
  const float w[3] = {vel[0].x, vel[1].x, vel[2].x}, v[3] = {vel[0].y, vel[1].y, vel[2].y};
  float wc[3], p[3], L[3], cp[3], b[3];
  cross3(w, c, wc);
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = m * (v[i] + wc[i]);
  const float ixx = body[4] * mscale, ixy = body[5] * mscale, ixz = body[6] * mscale;
  const float iyy = body[7] * mscale, iyz = body[8] * mscale, izz = body[9] * mscale;
  cross3(c, p, cp);
  L[0] = ixx * w[0] + ixy * w[1] + ixz * w[2] + cp[0];
  L[1] = ixy * w[0] + iyy * w[1] + iyz * w[2] + cp[1];
  L[2] = ixz * w[0] + iyz * w[1] + izz * w[2] + cp[2];
  const f2 X[3] = {f2{L[0], p[0]}, f2{L[1], p[1]}, f2{L[2], p[2]}};
  cross3(v, p, b);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    const f2 wx = w[i1] * X[i2] - w[i2] * X[i1];
    o[i] = f2{wx.x + b[i], wx.y};
  }
}

// Revolute joint about coordinate axis ax (0 = x, 1 = y) by q: E = Rot(ax, q)^T maps
// parent coordinates to child coordinates.  Only (c, s) is kept; every product with E
// mixes two components.
__device__ __forceinline__ void rE(int ax, float c, float s, const float* v, float* o) {  // o = E v
  if (ax == 0) {
    float y = c * v[1] + s * v[2], z = c * v[2] - s * v[1];
    o[0] = v[0]; o[1] = y; o[2] = z;
  } else {
    float x = c * v[0] - s * v[2], z = s * v[0] + c * v[2];
    o[0] = x; o[1] = v[1]; o[2] = z;
  }
}

__device__ __forceinline__ void rET(int ax, float c, float s, const float* v, float* o) {  // o = E^T v
  if (ax == 0) {
    float y = c * v[1] - s * v[2], z = s * v[1] + c * v[2];
    o[0] = v[0]; o[1] = y; o[2] = z;
  } else {
    float x = c * v[0] + s * v[2], z = c * v[2] - s * v[0];
    o[0] = x; o[1] = v[1]; o[2] = z;
  }
}

__device__ __forceinline__ void mat3_vec(const float* E, const float* v, float* o) {
  float x = E[0] * v[0] + E[1] * v[1] + E[2] * v[2];
  float y = E[3] * v[0] + E[4] * v[1] + E[5] * v[2];
  float z = E[6] * v[0] + E[7] * v[1] + E[8] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}

__device__ __forceinline__ void mat3T_vec(const float* E, const float* v, float* o) {
  float x = E[0] * v[0] + E[3] * v[1] + E[6] * v[2];
  float y = E[1] * v[0] + E[4] * v[1] + E[7] * v[2];
  float z = E[2] * v[0] + E[5] * v[1] + E[8] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}

// Joint offsets are sparse in the Go1 model (go1_create checks it): hip (x, y, 0), thigh
// (0, y, 0), calf (0, 0, z).  `M` = mask of the components of r that may be non-zero
// (bit i = component i), a constant after inlining and unrolling, so the products with
// the zero components are never emitted (not even as 0 * x, which IEEE forbids folding).
__host__ __device__ __forceinline__ constexpr int offset_mask(int j) { return j == 0 ? 3 : (j == 1 ? 2 : 4); }
// which components of a x b can be non-zero, a and b with masks ma, mb
__device__ __forceinline__ constexpr int cross_mask(int ma, int mb) {
  int m = 0;
  for (int i = 0; i < 3; ++i) {
    const int p = (i + 1) % 3, q = (i + 2) % 3;
    if ((((ma >> p) & 1) && ((mb >> q) & 1)) || (((ma >> q) & 1) && ((mb >> p) & 1))) m |= 1 << i;
  }
  return m;
}
// component i of a x b (a_p b_q - a_q b_p) with only the terms the masks allow
__device__ __forceinline__ float cross_c(int ma, int mb, int i, const float* a, const float* b) {
  const int p = (i + 1) % 3, q = (i + 2) % 3;
  const bool t1 = ((ma >> p) & 1) && ((mb >> q) & 1), t2 = ((ma >> q) & 1) && ((mb >> p) & 1);
  if (t1 && t2) return a[p] * b[q] - a[q] * b[p];
  if (t1) return a[p] * b[q];
  if (t2) return -(a[q] * b[p]);
  return 0.0f;
}

// motion transform parent -> child: (w, v) -> (E w, E (v - r x w)), r with mask M
__device__ __forceinline__ void xm(int ax, float c, float s, int M, const float* r, const float* vin, float* vout) {
  const int cm = cross_mask(M, 7);
  float t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = ((cm >> i) & 1) ? vin[3 + i] - cross_c(M, 7, i, r, vin) : vin[3 + i];
  rE(ax, c, s, vin, vout);
  rE(ax, c, s, t, vout + 3);
}

// Q = E^T M E for a full 3x3 M (row-major): rows of M E are E^T(row of M), then E^T per column.
__device__ __forceinline__ void rot_congruence(int ax, float c, float s, const float* M, float* Q) {
  float N[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) rET(ax, c, s, M + 3 * i, N + 3 * i);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float col[3] = {N[j], N[3 + j], N[6 + j]}, out[3];
    rET(ax, c, s, col, out);
    Q[j] = out[0]; Q[3 + j] = out[1]; Q[6 + j] = out[2];
  }
}

// ---- packed articulated-body algebra.  One wave alone issues a v_pk_fma_f32 (two FMAs) as
// fast as a v_fma_f32 (tools/probes/pk_rate.hip), and a spatial quantity pairs up by itself:
// a spatial vector is three (angular_i, linear_i) pairs, and a spatial inertia keeps its two
// symmetric 3 x 3 blocks as six (A_t, C_t) pairs -- every rotation, rank-1 update and sum of the
// articulated-body passes treats the two halves alike.  B (general 3 x 3) stays scalar.
struct SIP {
  f2 ac[6];
  float b[9];
};
__host__ __device__ __forceinline__ constexpr int s3i(int i, int j) {
  return i == 0 ? j : (i == 1 ? (j == 0 ? 1 : j + 2) : (j == 0 ? 2 : (j == 1 ? 4 : 5)));
}

__device__ __forceinline__ void rigid_sip(const float* body, float mscale, SIP& I) {
  SI s;
  rigid_si(body, mscale, s);
#pragma unroll
  for (int t = 0; t < 6; ++t) I.ac[t] = f2{s.a[t], s.c[t]};
#pragma unroll
  for (int i = 0; i < 9; ++i) I.b[i] = s.b[i];
}

__device__ __forceinline__ void sip_add(SIP& A, const SIP& B) {
#pragma unroll
  for (int t = 0; t < 6; ++t) A.ac[t] += B.ac[t];
#pragma unroll
  for (int i = 0; i < 9; ++i) A.b[i] += B.b[i];
}

// column ax of the 6 x 6 matrix as pairs: (A(i, ax), B^T(i, ax) = B(ax, i))
__device__ __forceinline__ f2 sip_col(const SIP& M, int ax, int i) { return f2{M.ac[s3i(i, ax)].x, M.b[ax * 3 + i]}; }

// y = M v for a v whose pair ax is zero (c_j of a joint about axis ax); v, y as pairs
__device__ __forceinline__ void sip_mul_sparse(const SIP& M, const f2* v, int ax, f2* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f2 st = f2{0.0f, 0.0f};
    bool first = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j == ax) continue;
      st = first ? M.ac[s3i(i, j)] * v[j] : st + M.ac[s3i(i, j)] * v[j];
      first = false;
    }
    float s = st.x, t = st.y;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j == ax) continue;
      s = s + M.b[i * 3 + j] * v[j].y;
      t = t + M.b[j * 3 + i] * v[j].x;
    }
    o[i] = f2{s, t};
  }
}

// E v (rE) and E^T v (rET) on pairs: both halves rotate by the same joint rotation
__device__ __forceinline__ void rE2(int ax, float c, float s, const f2* v, f2* o) {
  if (ax == 0) {
    const f2 y = c * v[1] + s * v[2], z = c * v[2] - s * v[1];
    o[0] = v[0]; o[1] = y; o[2] = z;
  } else {
    const f2 x = c * v[0] - s * v[2], z = s * v[0] + c * v[2];
    o[0] = x; o[1] = v[1]; o[2] = z;
  }
}
__device__ __forceinline__ void rET2(int ax, float c, float s, const f2* v, f2* o) {
  if (ax == 0) {
    const f2 y = c * v[1] - s * v[2], z = s * v[1] + c * v[2];
    o[0] = v[0]; o[1] = y; o[2] = z;
  } else {
    const f2 x = c * v[0] + s * v[2], z = c * v[2] - s * v[0];
    o[0] = x; o[1] = v[1]; o[2] = z;
  }
}

// motion transform parent -> child on pairs: (w, v) -> (E w, E (v - r x w)), r with mask M
__device__ __forceinline__ void xm2(int ax, float c, float s, int M, const float* r, const f2* vin, f2* vout) {
  const int cm = cross_mask(M, 7);
  const float w[3] = {vin[0].x, vin[1].x, vin[2].x};
  f2 t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = f2{w[i], ((cm >> i) & 1) ? vin[i].y - cross_c(M, 7, i, r, w) : vin[i].y};
  rE2(ax, c, s, t, vout);
}

// force transform child -> parent on pairs: (n, f) -> (E^T n + r x E^T f, E^T f), r with mask M
__device__ __forceinline__ void xfT2(int ax, float c, float s, int M, const float* r, const f2* fin, f2* fout) {
  const int cm = cross_mask(M, 7);
  f2 nf[3];
  rET2(ax, c, s, fin, nf);
  const float f[3] = {nf[0].y, nf[1].y, nf[2].y};
#pragma unroll
  for (int i = 0; i < 3; ++i) fout[i] = f2{((cm >> i) & 1) ? nf[i].x + cross_c(M, 7, i, r, f) : nf[i].x, f[i]};
}

// X^T Ia X for X = [[E, 0], [-E r~, E]]: rotate the blocks by E^T(.)E (A and C together as pairs), then translate
// by r (mask M):  A'' = A' + r~ B'^T - B' r~ - r~ C' r~ ,  B'' = B' + r~ C' ,  C'' = C'.
// RC = r~ C' has non-zero rows mc, BR = B' r~ non-zero columns mb, RCR = RC r~ both.
__device__ __forceinline__ void xform_inertia2(int ax, float cq, float sq, int M, const float* r, const SIP& In,
                                               SIP& Out) {
  const float sp = ax == 0 ? sq : -sq;
  const float c2 = cq * cq - sp * sp, s2 = 2.0f * cq * sp;
  // Q = E^T M E for the symmetric (A, C) pairs stored (xx xy xz yy yz zz).  E^T rotates the two indices (p, r)
  // other than the axis f by R = [[c, -s'], [s', c]] (s' = s for x, -s for y), so with c2 = c^2 - s'^2, s2 = 2 c s',
  // h = (Mpp + Mrr) / 2, d = (Mpp - Mrr) / 2:
  //   Qff = Mff, Qfp = c Mfp - s' Mfr, Qfr = s' Mfp + c Mfr,
  //   Qpp = h + d c2 - Mpr s2, Qrr = h - d c2 + Mpr s2, Qpr = d s2 + Mpr c2.
  const int f = ax, pI = ax == 0 ? 1 : 0, rI = 2;
  const f2 mff = In.ac[s3i(f, f)], mfp = In.ac[s3i(f, pI)], mfr = In.ac[s3i(f, rI)];
  const f2 mpp = In.ac[s3i(pI, pI)], mrr = In.ac[s3i(rI, rI)], mpr = In.ac[s3i(pI, rI)];
  const f2 h = 0.5f * (mpp + mrr), d = 0.5f * (mpp - mrr);
  const f2 qfp = cq * mfp - sp * mfr, qfr = sp * mfp + cq * mfr;
  const f2 qpp = h + d * c2 - mpr * s2, qrr = h - d * c2 + mpr * s2, qpr = d * s2 + mpr * c2;
  f2 Q[9];
  Q[f * 3 + f] = mff;
  Q[f * 3 + pI] = qfp; Q[pI * 3 + f] = qfp;
  Q[f * 3 + rI] = qfr; Q[rI * 3 + f] = qfr;
  Q[pI * 3 + pI] = qpp; Q[rI * 3 + rI] = qrr;
  Q[pI * 3 + rI] = qpr; Q[rI * 3 + pI] = qpr;
  float B[9], C[9];
  rot_congruence(ax, cq, sq, In.b, B);
#pragma unroll
  for (int i = 0; i < 9; ++i) C[i] = Q[i].y;
  // translation by r, with (M r~) row i = (row i of M) x r and r~ B'^T = -(B' r~)^T:
  // A'' = A' - BR^T - BR - RCR (upper triangle; zero terms are skipped), B'' = B' + RC, C'' = C'
  const int mc = cross_mask(M, 7), mb = cross_mask(7, M);
  float RC[9], BR[9], RCR[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float col[3] = {C[j], C[3 + j], C[6 + j]};
#pragma unroll
    for (int i = 0; i < 3; ++i) RC[3 * i + j] = ((mc >> i) & 1) ? cross_c(M, 7, i, r, col) : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      BR[3 * i + j] = ((mb >> j) & 1) ? cross_c(7, M, j, B + 3 * i, r) : 0.0f;
      RCR[3 * i + j] = ((mc >> i) & (mb >> j) & 1) ? cross_c(7, M, j, RC + 3 * i, r) : 0.0f;
    }
  const int II[6] = {0, 0, 0, 1, 1, 2}, JJ[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    const int i = II[t], j = JJ[t];
    float v = Q[i * 3 + j].x;
    if ((mb >> i) & 1) v -= BR[j * 3 + i];
    if ((mb >> j) & 1) v -= BR[i * 3 + j];
    if ((mc >> i) & (mb >> j) & 1) v -= RCR[i * 3 + j];
    Out.ac[t] = f2{v, C[i * 3 + j]};
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Out.b[3 * i + j] = ((mc >> i) & 1) ? B[3 * i + j] + RC[3 * i + j] : B[3 * i + j];
}

__device__ __forceinline__ float sip_get(const SIP& M, int i, int j) {
  if (i < 3 && j < 3) return M.ac[s3i(i, j)].x;
  if (i >= 3 && j >= 3) return M.ac[s3i(i - 3, j - 3)].y;
  if (i < 3) return M.b[i * 3 + (j - 3)];
  return M.b[j * 3 + (i - 3)];
}

// 6x6 SPD solve (Cholesky) of the packed inertia, identical instruction stream in every lane
__device__ __forceinline__ void solve6p(const SIP& M, const float* b, float* x) {
  float L[21];
#define LI(i, j) L[(i) * ((i) + 1) / 2 + (j)]
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      float s = sip_get(M, i, j);
#pragma unroll
      for (int k = 0; k < j; ++k) s -= LI(i, k) * LI(j, k);
      if (i == j) LI(i, i) = frsq(fmaxf(s, 1e-30f));  // holds 1 / L_ii
      else LI(i, j) = s * LI(j, j);
    }
  float y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    float s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= LI(i, k) * y[k];
    y[i] = s * LI(i, i);
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    float s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= LI(k, i) * x[k];
    x[i] = s * LI(i, i);
  }
#undef LI
}

__device__ __forceinline__ void quat_to_R(const float* q, float* R) {
  float x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
