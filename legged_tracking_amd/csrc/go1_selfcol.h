// go1_selfcol.h -- self-collision of the integrator: the primitives' LDS records, the closest-point kernels, the
// narrow phase (self_narrow) and the broad phase in registers (self_broad).
#pragma once
#ifndef GO1_DEVICE_H
#error "include go1_device.h: its parts are not self-contained"
#endif
#pragma clang fp contract(on)  // integrator code, compared with the f64 oracle within a tolerance

// ---- self-collision (asset.self_collisions == 0, go1_crawling.py:44: Isaac Gym collides every pair of bodies no
// joint connects; oracle/go1_oracle.c phys_substep).  Round 6: the links as capsules over their full length
// (the sphere chains of rounds 3-5 had 46-55 mm holes).  Primitive 4 leg + k, owned by the lane of role
// k: 0 thigh capsule (thigh joint .. knee), 1 hip capsule, 2 calf capsule (knee .. foot), 3 foot sphere.  Pairs:
// every primitive of leg la against every primitive of leg lb (16 per leg pair); within a leg the links two joints
// apart (hip vs calf and foot, thigh vs foot); the thigh and calf capsules and the foot against the trunk box (the
// hip is the trunk's neighbour).  A pair acts at the closest points of its two segments as two spheres of the
// capsules' radii there (seg_closest), a capsule against the box at its point nearest the box (seg_box_t).
// Explicit penalty springs on the overlap, fn = ks pen - ds vn (compressive only), no friction, no added mass (the
// bodies sit in different ABA chains, or two joints apart).
// Broad phase in registers: each lane bounds its leg (thigh joint, knee, foot, hip-capsule ends, grown by their
// radii) by an AABB in the trunk frame, swaps the four legs' boxes over the quad (DPP) and tests the six leg pairs,
// the trunk box and the leg's own folded links; a wave whose envs have no candidate is done.  Otherwise, per env in
// LDS: the 16 primitives as (P0, r), (P1, 0), (V0, 0), (V1, 0) (segment ends and their velocities, world), and each
// lane sums the forces on its own primitive from its candidate partners (self_narrow).
// (+ 36 floats of padding: they held the control step's face vertices and capsule parameters, now registers
// (go1_phys.h Held), and keep the four envs' records 4 banks apart as before)
#define SELF_ENV_FLOATS (16 * 16 + 4 + 32)

// the lane's own primitive into this env's LDS scratch; rb: the radius of its bounding sphere about the segment's middle
// (half the segment plus r), for the narrow phase's first test
__device__ __forceinline__ void self_put(float* sc, int leg, int role, const float* P0, const float* P1, float r,
                                         float rb) {
  float4* Q = reinterpret_cast<float4*>(sc) + 4 * (4 * leg + role);
  Q[0] = make_float4(P0[0], P0[1], P0[2], r);
  Q[1] = make_float4(P1[0], P1[1], P1[2], rb);
}
// the velocity half of the record: only the spring of a touching pair reads it, so it is written (by every lane of
// the wave, on a wave-uniform condition) when the first pair of the sub-step touches -- one entering wave in ten
__device__ __forceinline__ void self_put_vel(float* sc, int leg, int role, const float* V0, const float* V1) {
  float4* Q = reinterpret_cast<float4*>(sc) + 4 * (4 * leg + role);
  Q[2] = make_float4(V0[0], V0[1], V0[2], 0.0f);
  Q[3] = make_float4(V1[0], V1[1], V1[2], 0.0f);
}

// closest points of the segments P0 + s d1 and Q0 + t d2 (s, t in [0, 1]; a = |d1|^2, e = |d2|^2; a point has a
// or e = 0): Ericson's clamped construction, branch-free (oracle/go1_oracle.c seg_seg_closest), the lines' s formed
// without cancellation as (n . (d2 x r)) / (n . n), n = d1 x d2 (for nearly parallel links a e - b^2 cancels to a few
// ulps and would place the closest points anywhere along them)
__device__ __forceinline__ void seg_closest(const float* P0, const float* d1, const float* Q0, const float* d2,
                                            float& s, float& t) {
  const float r[3] = {P0[0] - Q0[0], P0[1] - Q0[1], P0[2] - Q0[2]};
  const float a = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2], e = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
  const float b = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
  const float c = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2], f = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2];
  float n[3], m[3];
  cross3(d1, d2, n);
  cross3(d2, r, m);
  const float den = n[0] * n[0] + n[1] * n[1] + n[2] * n[2], num = n[0] * m[0] + n[1] * m[1] + n[2] * m[2];
  const bool pa = a > 1e-12f, pe = e > 1e-12f;
  const float ia = pa ? frcp(a) : 0.0f, ie = pe ? frcp(e) : 0.0f;
  // every candidate computed, then selected (v_med3 clamps): as ternaries around the clamps the compiler had
  // made exec-mask branches of them, one wave paying each arm plus the hazard nops
  const float s0 = den > 1e-10f * a * e ? __builtin_amdgcn_fmed3f(num * frcp(den), 0.0f, 1.0f) : 0.0f;
  const float tt = (b * s0 + f) * ie;
  const float s_lo = __builtin_amdgcn_fmed3f(-c * ia, 0.0f, 1.0f), s_hi = __builtin_amdgcn_fmed3f((b - c) * ia, 0.0f, 1.0f);
  const float ss = tt < 0.0f ? s_lo : (tt > 1.0f ? s_hi : s0);
  const float t_pt = __builtin_amdgcn_fmed3f(f * ie, 0.0f, 1.0f);
  s = !pa ? 0.0f : (!pe ? s_lo : ss);
  t = !pe ? 0.0f : (!pa ? t_pt : __builtin_amdgcn_fmed3f(tt, 0.0f, 1.0f));
}

// the point of the segment P0 -> P1 (world) nearest the trunk box, deepest inside it: bisection on the sign of the
// derivative of the box's signed distance along the segment (convex), SEG_BISECT halvings (oracle/go1_oracle.c
// seg_box_t, which explains the sign); no square roots, and every midpoint an exact binary fraction
#define SEG_BISECT 20
__device__ __forceinline__ float seg_box_t(const float* P0, const float* P1, const float* R, const float* pos,
                                           const float* th) {
  float a0[3], d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    a0[i] = R[i] * (P0[0] - pos[0]) + R[3 + i] * (P0[1] - pos[1]) + R[6 + i] * (P0[2] - pos[2]);
    d[i] = R[i] * (P1[0] - P0[0]) + R[3 + i] * (P1[1] - P0[1]) + R[6 + i] * (P1[2] - P0[2]);
  }
  float lo = 0.0f, hi = 1.0f;
#pragma unroll
  for (int it = 0; it < SEG_BISECT; ++it) {
    const float m = 0.5f * (lo + hi);
    float so = 0.0f, qmax = -1e30f, sin = 0.0f;
    bool out = false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float c = a0[i] + m * d[i], sd = c >= 0.0f ? d[i] : -d[i], q = fabsf(c) - th[i];
      so += q > 0.0f ? q * sd : 0.0f;
      out = out || q > 0.0f;
      sin = q > qmax ? sd : sin;
      qmax = fmaxf(qmax, q);
    }
    const float sl = out ? so : sin;
    lo = sl < 0.0f ? m : lo;
    hi = sl < 0.0f ? hi : m;
  }
  return 0.5f * (lo + hi);
}

// The force of a pair on one of its primitives: the pair is evaluated in its canonical order (A = the lower primitive
// index), spheres of the two radii at the closest points s (on A), t (on B); the force on A, or its negative on B
// (own_first false), and the own primitive's point (world).  A, B: (P0 r, P1, V0, V1) records in LDS, so the two
// lanes of a pair compute the same bits and apply exactly opposite forces.
// need_vel: called (wave-uniformly) before the velocity records are read.
template <class NV>
__device__ __forceinline__ void self_pair_force(const float4* A, const float4* B, bool own_first, bool act, float ks,
                                                float ds, float* F, float* pown, bool& touch, NV need_vel) {
  const float4 a0 = A[0], a1 = A[1], b0 = B[0], b1 = B[1];
  const float pa0[3] = {a0.x, a0.y, a0.z}, da[3] = {a1.x - a0.x, a1.y - a0.y, a1.z - a0.z};
  const float pb0[3] = {b0.x, b0.y, b0.z}, db[3] = {b1.x - b0.x, b1.y - b0.y, b1.z - b0.z};
  float s, t;
  seg_closest(pa0, da, pb0, db, s, t);
  const float pa[3] = {pa0[0] + s * da[0], pa0[1] + s * da[1], pa0[2] + s * da[2]};
  const float pb[3] = {pb0[0] + t * db[0], pb0[1] + t * db[1], pb0[2] + t * db[2]};
  const float d0 = pa[0] - pb[0], d1 = pa[1] - pb[1], d2 = pa[2] - pb[2];
  const float dd = d0 * d0 + d1 * d1 + d2 * d2, rs = a0.w + b0.w;
#pragma unroll
  for (int i = 0; i < 3; ++i) { pown[i] = own_first ? pa[i] : pb[i]; F[i] = 0.0f; }
  // act: the lane has a pair this trip (an idle lane is handed its own leg's primitive 0 -- for a thigh lane itself,
  // at distance 0 -- and must not count as touching)
  touch = act & (dd < rs * rs);
  // the spring only where some lane of the wave has an overlap (most pairs the boxes let through do not touch; a
  // pair that does not has no force, so skipping it changes nothing)
  if (!__any(touch)) return;
  need_vel();
  const float inv = dd > 1e-18f ? frsq(dd) : 0.0f;
  const float n0 = dd > 1e-18f ? d0 * inv : 0.0f, n1 = dd > 1e-18f ? d1 * inv : 0.0f, n2 = dd > 1e-18f ? d2 * inv : 1.0f;
  const float pen = rs - dd * inv;
  const float4 va0 = A[2], va1 = A[3], vb0 = B[2], vb1 = B[3];
  const float vr0 = (va0.x + s * (va1.x - va0.x)) - (vb0.x + t * (vb1.x - vb0.x));
  const float vr1 = (va0.y + s * (va1.y - va0.y)) - (vb0.y + t * (vb1.y - vb0.y));
  const float vr2 = (va0.z + s * (va1.z - va0.z)) - (vb0.z + t * (vb1.z - vb0.z));
  const float vn = vr0 * n0 + vr1 * n1 + vr2 * n2;
  float fn = ks * pen - ds * vn;
  fn = (touch & (fn > 0.0f)) ? fn : 0.0f;
  fn = own_first ? fn : -fn;
  F[0] = fn * n0; F[1] = fn * n1; F[2] = fn * n2;
}

// sphere A (centre, radius in w) against the trunk box (half extents th about the base origin): the force on A (world)
// added to F and the trunk's reaction wrench (base frame, (moment, force) about the base origin) added to wb
__device__ __forceinline__ void self_box_force(const float4 A, const float4 Av, const float* R, const float* pos,
                                               const float* vb, const float* th, float ks, float ds, float* F,
                                               float* wb) {
  const float w0 = A.x - pos[0], w1 = A.y - pos[1], w2 = A.z - pos[2];
  float c[3], q[3], d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = R[i] * w0 + R[3 + i] * w1 + R[6 + i] * w2;
#pragma unroll
  for (int i = 0; i < 3; ++i) { q[i] = fminf(fmaxf(c[i], -th[i]), th[i]); d[i] = c[i] - q[i]; }
  const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  float nb[3], pen;
  if (dd > 0.0f) {
    const float inv = frsq(dd);
#pragma unroll
    for (int i = 0; i < 3; ++i) nb[i] = d[i] * inv;
    pen = A.w - dd * inv;
  } else {  // centre inside: out through the nearest face (lowest axis on ties), the depths compared quantised
    // to 0.1 mm (oracle BOX_Q): a segment's deepest point inside the box often has two faces equally near
    const float m0 = th[0] - fabsf(c[0]), m1 = th[1] - fabsf(c[1]), m2 = th[2] - fabsf(c[2]);
    const int q0 = (int)floorf(fminf(fmaxf(m0, -1.0f), 1.0f) * 1.0e4f), q1 = (int)floorf(fminf(fmaxf(m1, -1.0f), 1.0f) * 1.0e4f),
              q2 = (int)floorf(fminf(fmaxf(m2, -1.0f), 1.0f) * 1.0e4f);
    const int ax = ((q0 <= q1) & (q0 <= q2)) ? 0 : (q1 <= q2 ? 1 : 2);
    const float sg = c[ax] >= 0.0f ? 1.0f : -1.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) nb[i] = i == ax ? sg : 0.0f;
    q[ax] = sg * th[ax];
    pen = A.w + (ax == 0 ? m0 : (ax == 1 ? m1 : m2));
  }
  // the trunk's velocity at q (base frame v + w x q), relative normal velocity in the base frame
  const float vq0 = vb[3] + (vb[1] * q[2] - vb[2] * q[1]);
  const float vq1 = vb[4] + (vb[2] * q[0] - vb[0] * q[2]);
  const float vq2 = vb[5] + (vb[0] * q[1] - vb[1] * q[0]);
  float va[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) va[i] = R[i] * Av.x + R[3 + i] * Av.y + R[6 + i] * Av.z;
  const float vn = (va[0] - vq0) * nb[0] + (va[1] - vq1) * nb[1] + (va[2] - vq2) * nb[2];
  float fn = ks * pen - ds * vn;
  fn = ((dd < A.w * A.w) & (fn > 0.0f)) ? fn : 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) F[i] += fn * (R[3 * i] * nb[0] + R[3 * i + 1] * nb[1] + R[3 * i + 2] * nb[2]);
  const float f0 = -fn * nb[0], f1 = -fn * nb[1], f2v = -fn * nb[2];
  wb[0] += q[1] * f2v - q[2] * f1;
  wb[1] += q[2] * f0 - q[0] * f2v;
  wb[2] += q[0] * f1 - q[1] * f0;
  wb[3] += f0; wb[4] += f1; wb[5] += f2v;
}

// leg pairs lp: (0,1) = 0, (0,2) = 1, (0,3) = 2, (1,2) = 3, (1,3) = 4, (2,3) = 5

// Narrow phase (a wave whose broad phase found a candidate).  sc: this env's LDS scratch, the primitives already
// written (self_put).  Each lane sums the forces on its own primitive from its candidate partners: per candidate
// partner leg (tested where some lane of the wave has that partner; own_lo, own_hi: the own primitive's world box),
// the leg's four primitives (the own leg's two-joints-apart ones for d = 0) into a per-lane work list walked with
// ctz (the pair loop runs as often as the lane with the longest list needs), each pair evaluated in its canonical
// order (the lower primitive index first), so the two lanes of a pair compute the same bits and apply exactly
// opposite forces, every sum in a fixed order.  Then the trunk box for a folded leg.  Output: the world force Fo on
// the own primitive and its moment Mo about the own body's origin pb; wb: the trunk reaction of the lane's box
// contact (base frame).  vel(V0, V1): the velocities of the own primitive's ends (world), computed only in a wave
// and a sub-step that reads them -- a touching pair (then every lane writes its record first) or a box contact.
template <class VF>
__device__ __forceinline__ void self_narrow(CCfg* __restrict__ cfg, float* sc, int leg, int role, int mask,
                                           const float* R, const float* pos, const float* vb, const float* th,
                                           const float* pb, const float* own_lo, const float* own_hi, float* Fo,
                                           float* Mo, float* wb, VF vel) {
  const float ks = cfg->self_stiffness, ds = cfg->self_damping;
  const float4* Pr = reinterpret_cast<const float4*>(sc);
  const int io = 4 * leg + role;
  bool vel_put = false;  // wave-uniform: the velocity records of this sub-step are in LDS
  auto need_vel = [&]() {
    if (!vel_put) {
      float V0[3], V1[3];
      vel(V0, V1);
      self_put_vel(sc, leg, role, V0, V1);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the other lanes' records, as after self_put
      vel_put = true;
    }
  };
  const int lp1 = (leg >> 1) ? 5 : 0, lp2 = (leg & 1) ? 4 : 1, lp3 = (leg == 0 || leg == 3) ? 2 : 3;
  // candidate partner legs, bit d: leg ^ d (d = 0: the own leg's links two joints apart, when folded)
  unsigned cand = ((mask >> (10 + leg)) & 1) | (((mask >> lp1) & 1) << 1) | (((mask >> lp2) & 1) << 2) |
                  (((mask >> lp3) & 1) << 3);
  // the own leg's partners of primitive `role`: thigh - foot, hip - calf / foot, calf - hip, foot - thigh / hip
  const unsigned keep_same = (0x32C8u >> (4 * role)) & 0xFu;  // role 0: 0x8, 1: 0xC, 2: 0x2, 3: 0x3
  auto acc = [&](const float* p, const float* F) {  // force F (world) on the own primitive at p
    const float p0 = p[0] - pb[0], p1 = p[1] - pb[1], p2 = p[2] - pb[2];
    Fo[0] += F[0]; Fo[1] += F[1]; Fo[2] += F[2];
    Mo[0] += p1 * F[2] - p2 * F[1];
    Mo[1] += p2 * F[0] - p0 * F[2];
    Mo[2] += p0 * F[1] - p1 * F[0];
  };
  // first the bounding boxes (the segment's ends grown by the radius, world axes) of the candidate legs' primitives
  // into a per-lane work list (bit 4 d + m: primitive m of leg ^ d), then the pairs of the list.  The boxes travel
  // in registers: every lane holds its own, the row swaps hand it the four roles' boxes of its leg, and per partner
  // leg d that some lane of the wave has as a candidate (wave-uniform) a DPP quad_perm fetches leg ^ d's -- no LDS
  // round trip, the same boxes and the same list as from the records
  unsigned work = 0u;
  {
#ifdef GO1_ABL_NO_TESTLOOP  // ablation build only: no partner tests (and so no pairs)
    cand = 0u;
#endif
#ifdef GO1_ABL_RT_NO_TESTLOOP  // ablation build only: the same, decided at run time (the code stays)
    cand = cfg->self_stiffness > 1e30f ? cand : 0u;
#endif
    float rbx[4][6];  // (lo xyz, hi xyz) of primitive m of the own leg
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const uint32_t v = __float_as_uint(k < 3 ? own_lo[k] : own_hi[k - 3]);
      auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);        // rows (0 0 2 2), (1 1 3 3)
      auto e = __builtin_amdgcn_permlane32_swap(a[0], a[0], false, false);  // row 0, row 2 on every lane
      auto o = __builtin_amdgcn_permlane32_swap(a[1], a[1], false, false);  // row 1, row 3
      rbx[0][k] = __uint_as_float(e[0]); rbx[2][k] = __uint_as_float(e[1]);
      rbx[1][k] = __uint_as_float(o[0]); rbx[3][k] = __uint_as_float(o[1]);
    }
    auto test = [&](auto dtag) {
      constexpr int D = decltype(dtag)::value;
      if (!__any((cand >> D) & 1u)) return;
      unsigned bits = 0u;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        float q[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          if constexpr (D == 0) q[k] = rbx[m][k];
          else q[k] = quad_xor<D>(rbx[m][k]);
        }
        const bool ox = (q[0] <= own_hi[0]) & (own_lo[0] <= q[3]);
        const bool oy = (q[1] <= own_hi[1]) & (own_lo[1] <= q[4]);
        const bool oz = (q[2] <= own_hi[2]) & (own_lo[2] <= q[5]);
        bits |= (ox & oy & oz) ? 1u << m : 0u;
      }
      const unsigned keep = ((cand >> D) & 1u) ? (D == 0 ? keep_same : 0xFu) : 0u;
      work |= (bits & keep) << (4 * D);
    };
    test(std::integral_constant<int, 0>{});
    test(std::integral_constant<int, 1>{});
    test(std::integral_constant<int, 2>{});
    test(std::integral_constant<int, 3>{});
  }
  MARK(self_tests_done);
#ifdef GO1_ABL_NO_PAIRLOOP  // ablation build only: the pairs tested but never evaluated
  work = 0u;
#endif
#ifdef GO1_ABL_RT_NO_PAIRLOOP  // ablation build only: the same, decided at run time (the code stays)
  work = cfg->self_stiffness > 1e30f ? work : 0u;
#endif
  while (__any(work != 0u)) {
    const bool act = work != 0u;
    const int bit = act ? __builtin_ctz(work) : 0;
    work &= work - 1u;
    const int ip = 4 * (leg ^ (bit >> 2)) + (bit & 3);
    const bool first = io < ip;
    float F[3], p[3];
    bool touch;
    self_pair_force(Pr + 4 * min(io, ip), Pr + 4 * max(io, ip), first, act, ks, ds, F, p, touch, need_vel);
    if (__any(touch)) {
      const float Fw[3] = {act ? F[0] : 0.0f, act ? F[1] : 0.0f, act ? F[2] : 0.0f};
      acc(p, Fw);
    }
  }
  MARK(self_pairs_done);
  // the trunk box, for a folded leg's thigh, calf and foot (the hip is the trunk's neighbour) whose segment's
  // trunk-frame AABB, grown by its radius, meets the box (the fold gate is coarse: most folded links are far from
  // the trunk, and a link that misses the grown box has no force -- skipping it changes nothing)
#ifdef GO1_ABL_NO_BOXPHASE  // ablation build only: no capsule-box pairs
  bool on = false;
#else
  bool on = ((mask >> (6 + leg)) & 1) & (role != 1);
#endif
  if (!__any(on)) {  // no folded leg in the wave (the workload's every wave): not even the transform below
    MARK(self_box_done);
    return;
  }
  const float4 O0 = Pr[4 * io], O1 = Pr[4 * io + 1];
  {
    const float w0[3] = {O0.x - pos[0], O0.y - pos[1], O0.z - pos[2]}, w1[3] = {O1.x - pos[0], O1.y - pos[1], O1.z - pos[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float c0 = R[i] * w0[0] + R[3 + i] * w0[1] + R[6 + i] * w0[2];
      const float c1 = R[i] * w1[0] + R[3 + i] * w1[1] + R[6 + i] * w1[2];
      on = on & (fminf(c0, c1) - O0.w <= th[i]) & (fmaxf(c0, c1) + O0.w >= -th[i]);  // (&: && branches)
    }
  }
  if (__any(on)) {
    // the own ends' velocities from registers (the same bits as the record a touching pair may have written)
    float V0[3], V1[3];
    vel(V0, V1);
    const float4 O2 = make_float4(V0[0], V0[1], V0[2], 0.0f), O3 = make_float4(V1[0], V1[1], V1[2], 0.0f);
    const float P0[3] = {O0.x, O0.y, O0.z}, P1[3] = {O1.x, O1.y, O1.z};
    const float u = role == 3 ? 0.0f : seg_box_t(P0, P1, R, pos, th);
    const float4 C = make_float4(O0.x + u * (O1.x - O0.x), O0.y + u * (O1.y - O0.y), O0.z + u * (O1.z - O0.z), O0.w);
    const float4 Cv = make_float4(O2.x + u * (O3.x - O2.x), O2.y + u * (O3.y - O2.y), O2.z + u * (O3.z - O2.z), 0.0f);
    float F[3] = {0.0f, 0.0f, 0.0f}, w6[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    self_box_force(C, Cv, R, pos, vb, th, ks, ds, F, w6);
#pragma unroll
    for (int i = 0; i < 6; ++i) wb[i] += on ? w6[i] : 0.0f;
    const float Fb[3] = {on ? F[0] : 0.0f, on ? F[1] : 0.0f, on ? F[2] : 0.0f};
    const float pc[3] = {C.x, C.y, C.z};
    acc(pc, Fb);
  }
  MARK(self_box_done);
}

// Broad phase, in registers, in the trunk frame (where the legs keep their places whatever the trunk's
// pose; world-axis boxes of a yawed trunk overlap every leg): bit lp of the result = leg pair lp's boxes overlap,
// bits 6 + leg and 10 + leg = the leg is folded past its joint band (its trunk-box and same-leg pairs are
// tested); the pair bits on the env's 16 lanes.  pth, pkn, pft: the thigh joint, knee and foot (world); hc0, hc1:
// the hip capsule's ends in the trunk frame; q: the leg's joints.
__device__ __forceinline__ int self_broad(int leg, const float* pth, const float* pkn, const float* pft, float rmax,
                                          const float* hc0, const float* hc1, float rhip,
                                          const float* R, const float* pos, const float* th, const float* q) {
  float b[3][3];  // the three points in the trunk frame, R^T (p - pos)
  const float* pts[3] = {pth, pkn, pft};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float w0 = pts[k][0] - pos[0], w1 = pts[k][1] - pos[1], w2 = pts[k][2] - pos[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) b[k][i] = R[i] * w0 + R[3 + i] * w1 + R[6 + i] * w2;
  }
  // (bitwise &, |: short-circuit operators around the convergent DPP moves compile to exec-mask branches)
  bool o1 = true, o2 = true, o3 = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float clo = fminf(b[1][i], b[2][i]) - rmax, chi = fmaxf(b[1][i], b[2][i]) + rmax;  // knee .. foot
    const float tlo = fminf(b[0][i], clo), thi = fmaxf(b[0][i], chi);                       // + the thigh joint
    const float hlo = fminf(hc0[i], hc1[i]) - rhip, hhi = fmaxf(hc0[i], hc1[i]) + rhip;     // the hip capsule
    const float lo = fminf(tlo, hlo), hi = fmaxf(thi, hhi);
    const float lo1 = quad_xor<1>(lo), hi1 = quad_xor<1>(hi), lo2 = quad_xor<2>(lo), hi2 = quad_xor<2>(hi);
    const float lo3 = quad_xor<3>(lo), hi3 = quad_xor<3>(hi);
    o1 = o1 & (lo <= hi1) & (lo1 <= hi);
    o2 = o2 & (lo <= hi2) & (lo2 <= hi);
    o3 = o3 & (lo <= hi3) & (lo3 <= hi);
  }
  // the leg's own links two joints apart and the trunk box: out of reach while every joint of the leg is within
  // 0.1 rad of its URDF range (inside the band the capsules keep 8.6 mm same-leg and 14.8 mm box clearance;
  // tests/test_self_collision.py::test_fold_gate_is_sound), so only a leg outside that band goes to the narrow
  // phase for them (no branch here: the broad phase shares a basic block with the terrain contacts)
  const bool wild = (fabsf(q[0]) > 0.9029f) | (q[1] < -1.1472f) | (q[1] > 4.2888f) | (q[2] < -2.7966f) |
                    (q[2] > -0.8163f);
  const int fold = wild ? ((64 << leg) | (1024 << leg)) : 0;  // the narrow phase tests them exactly
  const int lp1 = (leg >> 1) ? 5 : 0;                         // (0,1) / (2,3)
  const int lp2 = (leg & 1) ? 4 : 1;                          // (0,2) / (1,3)
  const int lp3 = (leg == 0 || leg == 3) ? 2 : 3;             // (0,3) / (1,2)
  const int mask = (o1 ? 1 << lp1 : 0) | (o2 ? 1 << lp2 : 0) | (o3 ? 1 << lp3 : 0) | fold;
  return quad_or(mask);
}
