// go1_phys.h -- the native articulated-body integrator with implicit penalty contacts: the LDS layout of the model
// and per-joint config, the per-lane state (Phys), one integrator step (phys_substep), the reported contact forces.
#pragma once
#ifndef GO1_DEVICE_H
#error "include go1_device.h: its parts are not self-contained"
#endif
#pragma clang fp contract(on)  // integrator code, compared with the f64 oracle within a tolerance

// LDS copy of the per-joint config arrays, contiguous in go1_config from default_dof_pos
// (checked at go1_create): default_dof_pos, dof_pos_limits, torque_limits, hard_limits,
// height_grid_x, height_grid_y, after the model block
#define LDS_DDP (GO1_MODEL_FLOATS)
#define LDS_DPL (LDS_DDP + 12)
#define LDS_TL (LDS_DPL + 24)
#define LDS_HL (LDS_TL + 12)
#define LDS_GX (LDS_HL + 24)
#define LDS_GY (LDS_GX + GO1_GRID_X)
#define LDS_FLOATS (LDS_GY + GO1_GRID_Y)
static_assert(offsetof(go1_config, height_grid_y) - offsetof(go1_config, default_dof_pos) ==
                  (LDS_GY - LDS_DDP) * sizeof(float),
              "per-joint config arrays must be contiguous in go1_config");

// Physical state of one env as held by one lane of its quad.
struct Phys {
  float pos[3], quat[4];  // base (replicated on the 16 lanes of the env)
  f2 wv[3];               // base angular and linear velocity (world) as (w_i, v_i) pairs
  float q[3], qd[3];                   // this lane's leg
};

// A wave-uniform value pinned in an SGPR: opaque from here on, so the compiler keeps it (in the SGPR, or spilled to
// a VGPR lane and read back with v_readlane, no memory wait) where it would otherwise re-load a config field.
template <class V>
__device__ __forceinline__ void pin_s(V& v) {
  static_assert(sizeof(V) == 4, "one SGPR");
  // (readfirstlane: a value the VALU computed, such as the step length's division, lives in a VGPR)
  int s = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v));
  asm volatile("" : "+s"(s));
  v = __builtin_bit_cast(V, s);
}
// The config scalars every integrator step reads, read once per launch (sub_consts) in front of the decimation
// loop.  They stay run-time values: as compile-time constants they would move the integrator's FMA contractions.
struct PhysK {
  float kc, dc, df, rest_t, bounce;  // contact_stiffness, contact_damping, friction_damping, terrain_restitution,
                                     // bounce_threshold (CP)
  float self_k;                      // self_stiffness
};  // (the joint limits' constants are left to the compiler: it loads them far ahead of the backward pass)
__device__ __forceinline__ PhysK sub_consts(CCfg* __restrict__ cfg) {
  PhysK K = {cfg->contact_stiffness, cfg->contact_damping, cfg->friction_damping, cfg->terrain_restitution,
             cfg->bounce_threshold, cfg->self_stiffness};
  pin_s(K.kc); pin_s(K.dc); pin_s(K.df); pin_s(K.rest_t); pin_s(K.bounce); pin_s(K.self_k);
  return K;
}
// What the control step's first sim step chooses and the later ones reuse, in registers of the lane (both were
// round trips through the env's LDS scratch on every sim step): the deepest-point parameters of the lane's two
// capsule segments (seg_deepest2; the lane's own values) and the trunk faces' two vertices (face_scan; face_key_max
// leaves the same choice on all 16 lanes of the env).
struct Held {
  f2 ts;
  int face[2];
};

// One integrator step of length h for the env of this lane.  Lane layout (16 per env): lane = 16 role + 4 env +
// leg.  The four roles of a leg compute the leg's kinematics and ABA passes redundantly (base quantities on all 16
// lanes), and split the leg's contact geometry two per lane (x, y halves of f2), each a capsule segment acting at
// its deepest point (seg_deepest2; a point is a degenerate segment):
//   role 0: thigh half at the thigh joint, thigh half at the knee   (body: thigh, thigh)
//   role 1: hip capsule, trunk corner 2 leg                          (body: hip, trunk)
//   role 2: calf half at the knee, calf half at the foot             (body: calf, calf)
//   role 3: foot sphere, trunk corner 2 leg + 1                      (body: calf, trunk)
// so each wave has four envs and the whole grid fills every SIMD.  The lane's self-collision primitive is its x
// half's link (thigh, hip, calf, foot).
// The capsule search alone runs in another layout (seg_deepest2): the x and y halves change rows (swap16), so that
// rows 0-3 hold thigh upper, thigh lower, calf upper, calf lower in one half -- the four half links, searched with
// the full candidate set -- and hip capsule, corner, foot, corner in the other, searched with the short one; t and
// cell come home through the same exchange, and H.ts, cell[] hold the lane's own halves as everywhere else.
// cf_raw: this lane's reported contact forces (x half with the own primitive's self-contact force, y half, the
// trunk's self-collision reaction of the lane's box contact and, on one lane, the trunk faces').
// K: sub_consts(cfg); H: the control step's held choices, written when face_scan_now and read otherwise.
__device__ __forceinline__ void phys_substep(CCfg* __restrict__ cfg, const PhysK& K, Held& H, const float* lds,
                                             Phys& S, const float* tau,
                                             float h, const float* g, float friction, float restitution,
                                             float payload, const Terr& T, int leg, int role, bool cf_out,
                                             float* cf_raw, float* self_sc, bool face_scan_now) {
#pragma clang fp contract(on)
  // Model constants are compile-time literals (go1_model_consts.h, checked against the
  // model block by go1_create): no LDS reads or waits for them inside the sub-step loop.
  // Per-leg floats are the FL values times the leg's mirror signs (loop-invariant products).
  (void)lds;
  const float* model = GO1_MODEL_F32;
  const float msx = (leg & 2) ? -1.0f : 1.0f, msy = (leg & 1) ? -1.0f : 1.0f, msxy = msx * msy;
  float LC[39];
#pragma unroll
  for (int i = 0; i < 39; ++i) {
    const int p = GO1_LEG_SIGN[i];
    LC[i] = p == 0 ? GO1_LEG_FL[i] : GO1_LEG_FL[i] * (p == 1 ? msx : (p == 2 ? msy : msxy));
  }
  MARK(phys_begin);
  const CP C = {K.kc, K.dc, K.df, friction, 0.5f * (restitution + K.rest_t), K.bounce};
  float R[9];
  quat_to_R(S.quat, R);
  f2 vbp[3];  // base-frame (angular, linear) velocity pairs: R^T on both halves at once
#pragma unroll
  for (int i = 0; i < 3; ++i) vbp[i] = R[i] * S.wv[0] + R[3 + i] * S.wv[1] + R[6 + i] * S.wv[2];
  const float vb[6] = {vbp[0].x, vbp[1].x, vbp[2].x, vbp[0].y, vbp[1].y, vbp[2].y};
  const float* th = model + 13 * 10 + 4 * 9 + 3 + 1;  // trunk half extents
#ifndef GO1_ABL_NO_FACES
  // the trunk faces' vertices of the control step (face_scan), chosen here where few values are live yet (wave-uniform
  // condition) and held for every sim step's face_force below
  if (T.patch && face_scan_now) face_scan(T, R, S.pos, th, 4 * role + leg, H.face);
#endif
  // ---- this leg: kinematics, rigid bias forces and gravity (hip -> calf)
  const float* origin = LC + 30;
  const float* foot = model + 13 * 10 + 4 * 9;
  const float foot_r = foot[3];
  const float thigh_r = model[13 * 10 + 4 * 9 + 3 + 1 + 3];
  const float calf_r = model[13 * 10 + 4 * 9 + 3 + 1 + 3 + 1];
  const float hip_r = model[13 * 10 + 4 * 9 + 3 + 1 + 3 + 2];
  const float hip_y0 = model[13 * 10 + 4 * 9 + 3 + 1 + 3 + 3], hip_y1 = model[13 * 10 + 4 * 9 + 3 + 1 + 3 + 4];
  float cs[3][2];
  // the lane's two bodies (x, y halves of the contact pass), selected as the chain passes them: x half thigh (role
  // 0), hip (1), calf (2, 3); y half thigh (0), calf (2), trunk (odd rows)
  const bool even = (role & 1) == 0;
  f2 Rs[9], ps[3], vs[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rs[i] = f2{0.0f, R[i]};
#pragma unroll
  for (int i = 0; i < 3; ++i) { ps[i] = f2{0.0f, S.pos[i]}; vs[i] = f2{0.0f, vb[i]}; vs[3 + i] = f2{0.0f, vb[3 + i]}; }
  float pth[3], pkn[3], pft[3];  // the thigh joint, the knee and the foot centre (world), for the broad phase
  f2 cjp[3][3], pAp[3][3];  // c_j and the articulated bias force as (angular, linear) pairs
  {
    // link frame: rows 0 and 1 of the rotation as pairs over the column (row0_k, row1_k)
    f2 R01[3], pp01 = f2{S.pos[0], S.pos[1]};
    float R2[3], pp2 = S.pos[2];
    f2 vp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { R01[k] = f2{R[k], R[3 + k]}; R2[k] = R[6 + k]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) vp[i] = vbp[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int ax = j == 0 ? 0 : 1;
      const float* r = origin + j * 3;
      float sn, cn;
      hw_sincosf(S.q[j], &sn, &cn);
      cs[j][0] = cn; cs[j][1] = sn;
      f2 vj[3];
      xm2(ax, cn, sn, offset_mask(j), r, vp, vj);
      vj[ax].x += S.qd[j];
      // c_j = v_j x (S qd), S = unit axis ax: pair ax is exactly zero and never read
      {
        const float qdj = S.qd[j];
        const int p1 = (ax + 1) % 3, p2 = (ax + 2) % 3;  // (w x e_ax)_p1 = w_p2, (.)_p2 = -w_p1
        cjp[j][ax] = f2{0.0f, 0.0f};
        cjp[j][p1] = vj[p2] * qdj;
        cjp[j][p2] = -(vj[p1] * qdj);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k)  // pp += Rp r over the components r may have
        if ((offset_mask(j) >> k) & 1) { pp01 += R01[k] * r[k]; pp2 += R2[k] * r[k]; }
      rE2(ax, cn, sn, R01, R01);
      rE(ax, cn, sn, R2, R2);
      // rigid bias force v x* I v about the link origin (gravity: a base acceleration, below)
      rigid_bias2(LC + 10 * j, vj, pAp[j]);
      const bool sx = j == 0 ? role == 1 : (j == 1 ? role == 0 : role >= 2);  // this link is the x half's
      const bool sy = j == 1 ? role == 0 : (j == 2 ? role == 2 : false);      // ... the y half's
      if (j > 0) {
        (j == 1 ? pth : pkn)[0] = pp01.x; (j == 1 ? pth : pkn)[1] = pp01.y; (j == 1 ? pth : pkn)[2] = pp2;
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float lr[3] = {R01[k].x, R01[k].y, R2[k]};  // column k of the link rotation
#pragma unroll
        for (int row = 0; row < 3; ++row) {
          Rs[3 * row + k].x = sx ? lr[row] : Rs[3 * row + k].x;
          Rs[3 * row + k].y = sy ? lr[row] : Rs[3 * row + k].y;
        }
      }
      const float pv[3] = {pp01.x, pp01.y, pp2};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        ps[i].x = sx ? pv[i] : ps[i].x;
        ps[i].y = sy ? pv[i] : ps[i].y;
        vs[i].x = sx ? vj[i].x : vs[i].x;
        vs[i].y = sy ? vj[i].x : vs[i].y;
        vs[3 + i].x = sx ? vj[i].y : vs[3 + i].x;
        vs[3 + i].y = sy ? vj[i].y : vs[3 + i].y;
      }
      if (j == 2) {  // the foot centre (world), for the broad phase
        pft[0] = pp01.x + R01[0].x * foot[0] + R01[1].x * foot[1] + R01[2].x * foot[2];
        pft[1] = pp01.y + R01[0].y * foot[0] + R01[1].y * foot[1] + R01[2].y * foot[2];
        pft[2] = pp2 + R2[0] * foot[0] + R2[1] * foot[1] + R2[2] * foot[2];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) vp[i] = vj[i];
    }
  }
  MARK(leg_kin_done);
  // ---- contacts: the lane's two segments (x, y halves) in the body frame of their link, their deepest points
  //      against the heightfields, the explicit force there and the added mass of the implicit contact
  // per lane: the body-frame wrench of the x half's link (thigh, hip or calf) and of the even rows' y half (the
  // same link), the trunk's share (odd rows' y halves, the box reactions)
  float fx[6], fy[6], fbase[6];
  f2 Fpt[3];          // world forces of the lane's two contact points
  float Fo[3] = {0.0f, 0.0f, 0.0f};  // the own primitive's self-contact force (world)
  float Fbs[3] = {0.0f, 0.0f, 0.0f};  // world reaction force on the trunk of the lane's self-collision box contact
  SIP cin[2];
#ifndef GO1_ABL_NO_CONTACT
  {
    f2 lpA[3], lpB[3], rr;
    {
      // segment ends in the link frame: halves walked from their outer ends (a link lying flat is carried at both)
      const float* kn = origin + 6;  // the knee: the calf joint's origin in the thigh frame
      const int cA = leg * 2, cB = leg * 2 + 1;  // this leg's trunk corners (roles 1, 3)
      const float crn[2][3] = {{(cA & 1) ? th[0] : -th[0], (cA & 2) ? th[1] : -th[1], (cA & 4) ? th[2] : -th[2]},
                               {(cB & 1) ? th[0] : -th[0], (cB & 2) ? th[1] : -th[1], (cB & 4) ? th[2] : -th[2]}};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float hyA = i == 1 ? msy * hip_y0 : 0.0f, hyB = i == 1 ? msy * hip_y1 : 0.0f;
        // (sel4: bit-test selects; equality chains on role compile to divergent branches)
        const float xa = sel4(role, 0.0f, hyA, 0.0f, foot[i]);
        const float xb = sel4(role, 0.5f * kn[i], hyB, 0.5f * foot[i], foot[i]);
        const float ya = sel4(role, kn[i], crn[0][i], foot[i], crn[1][i]);
        const float yb = sel4(role, 0.5f * kn[i], crn[0][i], 0.5f * foot[i], crn[1][i]);
        lpA[i] = f2{xa, ya};
        lpB[i] = f2{xb, yb};
      }
      rr = f2{sel4(role, thigh_r, hip_r, calf_r, foot_r), sel4(role, thigh_r, 0.0f, calf_r, 0.0f)};
    }
    // self-collision first (few values live yet): the broad phase, and the narrow phase in a wave with a candidate
    float wb[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, Mo[3] = {0.0f, 0.0f, 0.0f};
    MARK(self_begin);
#ifndef GO1_ABL_NO_SELF  // ablation build only: no self-collision
    const bool self_on = K.self_k > 0.0f;
    int mask;
    {
      // the hip capsule's ends in the trunk frame: the hip joint + Rx(q) (0, y, 0)
      const f2 hy = msy * f2{hip_y0, hip_y1};
      const f2 hcy = origin[1] + cs[0][0] * hy, hcz = origin[2] + cs[0][1] * hy;
      const float hc0[3] = {origin[0], hcy.x, hcz.x}, hc1[3] = {origin[0], hcy.y, hcz.y};
      mask = self_broad(leg, pth, pkn, pft, fmaxf(foot_r, fmaxf(thigh_r, calf_r)), hc0, hc1, hip_r, R, S.pos, th,
                        S.q);
      mask = self_on ? mask : 0;
    }
#else
    const bool self_on = false;
    const int mask = 0;
#endif
    MARK(self_broad_done);
#ifdef GO1_ABL_NO_NARROW  // ablation build only: the broad phase runs, the narrow phase never does
    if (__any(mask != 0) && mask == 12345) {
#else
    if (__any(mask != 0)) {
#endif
      // the lane's own primitive (its x half's link): the whole segment, ends and their velocities (world)
      float P0[3], P1[3];
      f2 e[3];  // (end 0, end 1) in the link frame
      {
        const float* kn = origin + 6;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float hy0 = i == 1 ? msy * hip_y0 : 0.0f, hy1 = i == 1 ? msy * hip_y1 : 0.0f;
          e[i] = f2{sel4(role, 0.0f, hy0, 0.0f, foot[i]), sel4(role, kn[i], hy1, foot[i], foot[i])};
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const f2 p = ps[i].x + Rs[3 * i].x * e[0] + Rs[3 * i + 1].x * e[1] + Rs[3 * i + 2].x * e[2];
          P0[i] = p.x; P1[i] = p.y;
        }
      }
      // the ends' velocities, for self_narrow where it reads them (a touching pair, a box contact)
      auto vel = [&](float* V0, float* V1) {
        const float w[3] = {vs[0].x, vs[1].x, vs[2].x};
        const f2 wl[3] = {w[1] * e[2] - w[2] * e[1], w[2] * e[0] - w[0] * e[2], w[0] * e[1] - w[1] * e[0]};
        const f2 vlin[3] = {vs[3].x + wl[0], vs[4].x + wl[1], vs[5].x + wl[2]};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const f2 v = Rs[3 * i].x * vlin[0] + Rs[3 * i + 1].x * vlin[1] + Rs[3 * i + 2].x * vlin[2];
          V0[i] = v.x; V1[i] = v.y;
        }
      };
      // bounding radius: half the link's segment (thigh, calf: half the knee / foot offset; hip: half the capsule's
      // segment; foot: a point) plus its radius
      const float half = sel4(role, 0.5f * fabsf(origin[8]), 0.5f * (hip_y1 - hip_y0), 0.5f * fabsf(foot[2]), 0.0f);
      self_put(self_sc, leg, role, P0, P1, rr.x, half + rr.x);
      // the block is this one wave (TPB 64): the other lanes' primitives are visible once the wave's own LDS
      // writes completed -- no s_barrier, and above all no vmcnt(0) drain of the terrain loads in flight
      static_assert(TPB == 64, "self-collision LDS exchange assumes one wave per block");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      MARK(self_put_done);
      const float pb[3] = {ps[0].x, ps[1].x, ps[2].x};
      // the own primitive's world-axis box (its segment's ends grown by its radius), for the partner tests
      float own_lo[3], own_hi[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) { own_lo[i] = fminf(P0[i], P1[i]) - rr.x; own_hi[i] = fmaxf(P0[i], P1[i]) + rr.x; }
      self_narrow(cfg, self_sc, leg, role, mask, R, S.pos, vb, th, pb, own_lo, own_hi, Fo, Mo, wb, vel);
      // the next sub-step's self_put must not overtake this one's partner reads of other lanes' records
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      MARK(self_narrow_done);
    }
    // world positions of the segment ends, the deepest point of each segment, its point kinematics
    f2 lp[3], pw[3], vw[3];
    HQ qa, qb;
    int cell[2];
    {
      f2 wA[3], wB[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        wA[i] = ps[i] + Rs[3 * i] * lpA[0] + Rs[3 * i + 1] * lpA[1] + Rs[3 * i + 2] * lpA[2];
        wB[i] = ps[i] + Rs[3 * i] * lpB[0] + Rs[3 * i + 1] * lpB[1] + Rs[3 * i + 2] * lpB[2];
      }
      MARK(seg_begin);
      // the search once per control step (wave-uniform), its t held (H.ts) for the other sim steps
      f2 ts;
      if (face_scan_now) {
#ifdef GO1_ABL_NO_WALK  // ablation build only: every segment at its first end
        ts = f2{0.0f, 0.0f} * (wA[0] + wB[0]);
        cell[0] = SEG_CELL((int)floorf(wA[0].x / T.hs), (int)floorf(wA[1].x / T.hs), false);
        cell[1] = SEG_CELL((int)floorf(wA[0].y / T.hs), (int)floorf(wA[1].y / T.hs), false);
#else
        // (the radii in the search's row layout: the half links' by row pair; hip, corner, foot, corner)
        const f2 rs = f2{(role & 2) ? calf_r : thigh_r, sel4(role, hip_r, 0.0f, foot_r, 0.0f)};
        ts = seg_deepest2(T, wA, wB, rr, rs, cell);
#endif
        H.ts = ts;
      } else {
        ts = H.ts;
      }
      MARK(seg_done);
#pragma unroll
      for (int i = 0; i < 3; ++i) lp[i] = lpA[i] + ts * (lpB[i] - lpA[i]);
      // point kinematics: v = R (v_lin + w x lp), p = p_body + R lp
      const f2 wl[3] = {vs[1] * lp[2] - vs[2] * lp[1], vs[2] * lp[0] - vs[0] * lp[2], vs[0] * lp[1] - vs[1] * lp[0]};
      const f2 vlin[3] = {vs[3] + wl[0], vs[4] + wl[1], vs[5] + wl[2]};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        pw[i] = ps[i] + Rs[3 * i] * lp[0] + Rs[3 * i + 1] * lp[1] + Rs[3 * i + 2] * lp[2];
        vw[i] = Rs[3 * i] * vlin[0] + Rs[3 * i + 1] * vlin[1] + Rs[3 * i + 2] * vlin[2];
      }
    }
    // the terrain contacts at the segments' deepest points: on the search step on the triangle the search chose, later
    // on the triangle under the point
    if (face_scan_now) {
      hq_fetch_cell(T, pw[0].x, pw[1].x, cell[0], qa);
      hq_fetch_cell(T, pw[0].y, pw[1].y, cell[1], qb);
    } else {
      hq_fetch(T, pw[0].x, pw[1].x, qa);
      hq_fetch(T, pw[0].y, pw[1].y, qb);
    }
    float Fa[3], Fb2[3], Ma[6], Mb[6];
    {
      const float pa[3] = {pw[0].x, pw[1].x, pw[2].x}, va[3] = {vw[0].x, vw[1].x, vw[2].x};
      const float pb[3] = {pw[0].y, pw[1].y, pw[2].y}, vb2[3] = {vw[0].y, vw[1].y, vw[2].y};
      sphere_contact_im(T, qa, C, pa, va, rr.x, h, Fa, Ma);
      sphere_contact_im(T, qb, C, pb, vb2, rr.y, h, Fb2, Mb);
    }
    if (self_on) {
#pragma unroll
      for (int i = 0; i < 3; ++i) Fbs[i] = R[3 * i] * wb[3] + R[3 * i + 1] * wb[4] + R[3 * i + 2] * wb[5];
    }
    const f2 F[3] = {f2{Fa[0], Fb2[0]}, f2{Fa[1], Fb2[1]}, f2{Fa[2], Fb2[2]}};
    // the ABA below solves for accelerations relative to free fall (gravity as a base
    // acceleration), so the added mass would respond to a - g: the force it sees is F - Mp g
    f2 Fd[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      Fd[i] = F[i] - (f2{Ma[s3i(i, 0)], Mb[s3i(i, 0)]} * g[0] + f2{Ma[s3i(i, 1)], Mb[s3i(i, 1)]} * g[1] +
                      f2{Ma[s3i(i, 2)], Mb[s3i(i, 2)]} * g[2]);
    // body-frame force f = R^T Fd and moment lp x f; the own primitive's self-contact wrench (R^T Fo, R^T Mo) joins
    // the x half (its link)
    f2 f6[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) f6[3 + j] = Rs[j] * Fd[0] + Rs[3 + j] * Fd[1] + Rs[6 + j] * Fd[2];
    f6[0] = lp[1] * f6[5] - lp[2] * f6[4];
    f6[1] = lp[2] * f6[3] - lp[0] * f6[5];
    f6[2] = lp[0] * f6[4] - lp[1] * f6[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      f6[j].x += Rs[j].x * Mo[0] + Rs[3 + j].x * Mo[1] + Rs[6 + j].x * Mo[2];
      f6[3 + j].x += Rs[j].x * Fo[0] + Rs[3 + j].x * Fo[1] + Rs[6 + j].x * Fo[2];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      fx[i] = f6[i].x;
      fy[i] = even ? f6[i].y : 0.0f;
      fbase[i] = (even ? 0.0f : f6[i].y) + wb[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) Fpt[i] = F[i];
    // added masses into the body frame, M = Rs^T Mp Rs (both points as halves), then about the
    // body origin: A = S M S^T, B = S M, C = M, S = lp~ (S v = lp x v)
    const f2 Mw[6] = {f2{Ma[0], Mb[0]}, f2{Ma[1], Mb[1]}, f2{Ma[2], Mb[2]},
                      f2{Ma[3], Mb[3]}, f2{Ma[4], Mb[4]}, f2{Ma[5], Mb[5]}};
    f2 MR[9];  // Mp Rs (3 x 3, row-major)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        MR[3 * i + j] = Mw[s3i(i, 0)] * Rs[j] + Mw[s3i(i, 1)] * Rs[3 + j] + Mw[s3i(i, 2)] * Rs[6 + j];
    f2 M[9];  // Rs^T (Mp Rs), symmetric
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) {
        M[3 * i + j] = Rs[i] * MR[j] + Rs[3 + i] * MR[3 + j] + Rs[6 + i] * MR[6 + j];
        M[3 * j + i] = M[3 * i + j];
      }
    f2 SM[9];  // lp~ M: row i = lp x (column of M) components
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      SM[j] = lp[1] * M[6 + j] - lp[2] * M[3 + j];
      SM[3 + j] = lp[2] * M[j] - lp[0] * M[6 + j];
      SM[6 + j] = lp[0] * M[3 + j] - lp[1] * M[j];
    }
    const int II[6] = {0, 0, 0, 1, 1, 2}, JJ[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = II[k], j = JJ[k];
      const f2* r = SM + 3 * i;
      // (S M S^T)_ij = sum_l (SM)_il S_jl, S_j = (0, -lz, ly), (lz, 0, -lx), (-ly, lx, 0)
      const f2 a = j == 0 ? r[2] * lp[1] - r[1] * lp[2] : (j == 1 ? r[0] * lp[2] - r[2] * lp[0] : r[1] * lp[0] - r[0] * lp[1]);
      cin[0].ac[k][0] = a.x; cin[1].ac[k][0] = a.y;
      cin[0].ac[k][1] = M[3 * i + j].x; cin[1].ac[k][1] = M[3 * i + j].y;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) { cin[0].b[i] = SM[i].x; cin[1].b[i] = SM[i].y; }
  }
#else  // ablation build only: no contacts
  (void)th; (void)foot_r; (void)thigh_r; (void)calf_r; (void)hip_r; (void)hip_y0; (void)hip_y1; (void)C; (void)T;
  (void)Rs; (void)ps; (void)vs; (void)pth; (void)pkn; (void)pft;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int t = 0; t < 6; ++t) cin[k].ac[t] = f2{0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 9; ++i) cin[k].b[i] = 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) { fx[i] = 0.0f; fy[i] = 0.0f; fbase[i] = 0.0f; }
#pragma unroll
  for (int i = 0; i < 3; ++i) Fpt[i] = f2{0.0f, 0.0f};
#endif
  // the lane's contributions per body, summed over the leg's roles: thigh (rows 0-1: role 0's halves), calf (rows
  // 2-3: role 2's halves and role 3's foot) in one pair reduction; hip (role 1's x half) and the trunk (odd rows'
  // y halves, the box reactions) in a second
  SIP ci_th, ci_ca, ci_hp, ci_bs;
  {
    const bool hip_lane = role == 1;
    auto term = [&](int h, int k) -> float {  // value k of the lane's half h: the wrench (6), then the 21 inertia terms
      if (k < 6) return h == 0 ? fx[k] : fy[k];
      const int m = k - 6;
      return m < 12 ? cin[h].ac[m >> 1][m & 1] : cin[h].b[m - 12];
    };
    {  // thigh (rows 0-1) and calf (rows 2-3)
      float lg[6 + 21], th6[6 + 21], ca6[6 + 21];
#pragma unroll
      for (int k = 0; k < 27; ++k) lg[k] = (hip_lane ? 0.0f : term(0, k)) + (even ? term(1, k) : 0.0f);
      pairsum_rows_n<6 + 21>(lg, th6, ca6);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        pAp[1][i] -= f2{th6[i], th6[3 + i]};
        pAp[2][i] -= f2{ca6[i], ca6[3 + i]};
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        ci_th.ac[k] = f2{th6[6 + 2 * k], th6[6 + 2 * k + 1]};
        ci_ca.ac[k] = f2{ca6[6 + 2 * k], ca6[6 + 2 * k + 1]};
      }
#pragma unroll
      for (int i = 0; i < 9; ++i) { ci_th.b[i] = th6[18 + i]; ci_ca.b[i] = ca6[18 + i]; }
    }
    {  // the hip capsule (row 1's x half): a value that only row 1 holds, handed to every lane
      float hp[6 + 21], lo[6 + 21];
#pragma unroll
      for (int k = 0; k < 27; ++k) hp[k] = term(0, k);
      row1_bcast_n<6 + 21>(hp, lo);
#pragma unroll
      for (int i = 0; i < 3; ++i) pAp[0][i] -= f2{lo[i], lo[3 + i]};
#pragma unroll
      for (int k = 0; k < 6; ++k) ci_hp.ac[k] = f2{lo[6 + 2 * k], lo[6 + 2 * k + 1]};
#pragma unroll
      for (int i = 0; i < 9; ++i) ci_hp.b[i] = lo[18 + i];
    }
    {  // the trunk: this leg's corners (odd rows' y halves) and the box reactions
      // (the 21 added-mass values on rows 1 and 3 only: the odd rows' sum; the six forces on every row)
      float bs[6 + 21];
#pragma unroll
      for (int k = 0; k < 27; ++k) bs[k] = k < 6 ? fbase[k] : term(1, k);
      rowsum4_n<6>(bs);
      oddrows_sum_n<21>(bs + 6);
#pragma unroll
      for (int i = 0; i < 6; ++i) fbase[i] = bs[i];
#pragma unroll
      for (int k = 0; k < 6; ++k) ci_bs.ac[k] = f2{bs[6 + 2 * k], bs[6 + 2 * k + 1]};
#pragma unroll
      for (int i = 0; i < 9; ++i) ci_bs.b[i] = bs[18 + i];
    }
  }
  MARK(leg_kin_contacts_done);
  // ---- backward pass calf -> hip (articulated inertias with the contact added masses, bias
  //      forces with the explicit contact forces); the hip's inertia goes to the base
  f2 Up[3][3];  // U = column ax of the articulated inertia, (angular, linear) pairs
  float D[3], u[3];
  SIP Ip;
  f2 pp6[3];
  {
    SIP IA;
    rigid_sip(LC + 20, 1.0f, IA);
    sip_add(IA, ci_ca);
#pragma unroll
    for (int j = 2; j >= 0; --j) {
      const int ax = j == 0 ? 0 : 1;
      float t = tau[j];
      // joint-limit spring-damper, implicit in the joint: the torque at the end of the
      // sub-step, -k (q + h qd') - d qd' with qd' = qd + h qdd, moves (h d + h^2 k) qdd
      // into the joint inertia D (unconditionally stable for any k, d)
      const float lo = cfg->hard_limits[2 * j], hi = cfg->hard_limits[2 * j + 1];  // leg-uniform (go1_create)
      const bool lim_on = S.q[j] > hi || S.q[j] < lo;
      const float ex = S.q[j] > hi ? S.q[j] - hi : S.q[j] - lo;
      const float kl = cfg->limit_stiffness, dl = cfg->limit_damping;
      t -= lim_on ? kl * (ex + h * S.qd[j]) + dl * S.qd[j] : 0.0f;
#pragma unroll
      for (int i = 0; i < 3; ++i) Up[j][i] = sip_col(IA, ax, i);
      D[j] = IA.ac[s3i(ax, ax)].x + (lim_on ? h * dl + h * h * kl : 0.0f);
      u[j] = t - pAp[j][ax].x;
      const float invD = frcp(D[j]);
      D[j] = invD;  // the forward pass only needs 1 / D
      f2 V[3];  // U / D
#pragma unroll
      for (int i = 0; i < 3; ++i) V[i] = Up[j][i] * invD;
      SIP Ia;  // IA - U U^T / D: the A and C blocks as pairs, B scalar
      const int II[6] = {0, 0, 0, 1, 1, 2}, JJ[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
      for (int k = 0; k < 6; ++k) Ia.ac[k] = IA.ac[k] - Up[j][II[k]] * V[JJ[k]];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) Ia.b[a * 3 + b] = IA.b[a * 3 + b] - Up[j][a].x * V[b].y;
      f2 Iac[3], pa[3], pt[3];
      sip_mul_sparse(Ia, cjp[j], ax, Iac);
      const float ud = u[j] * invD;
#pragma unroll
      for (int i = 0; i < 3; ++i) pa[i] = pAp[j][i] + Iac[i] + Up[j][i] * ud;
      SIP It;
      xform_inertia2(ax, cs[j][0], cs[j][1], offset_mask(j), origin + j * 3, Ia, It);
      xfT2(ax, cs[j][0], cs[j][1], offset_mask(j), origin + j * 3, pa, pt);
      if (j > 0) {
        rigid_sip(LC + 10 * (j - 1), 1.0f, IA);
        sip_add(IA, It);
        sip_add(IA, j == 2 ? ci_th : ci_hp);  // the thigh's / the hip capsule's contact added masses
#pragma unroll
        for (int i = 0; i < 3; ++i) pAp[j - 1][i] += pt[i];
      } else {
        Ip = It;
        sip_add(Ip, ci_bs);  // this leg's trunk corners: summed over the legs with the hips below
#pragma unroll
        for (int i = 0; i < 3; ++i) pp6[i] = pt[i];
      }
    }
  }
  MARK(backward_done);
  // ---- the trunk faces (face_scan / face_force): the vertices once per control step, the force every sim step
  f2 wface[3] = {f2{0.0f, 0.0f}, f2{0.0f, 0.0f}, f2{0.0f, 0.0f}};
  float Fface[3] = {0.0f, 0.0f, 0.0f};
#ifdef GO1_ABL_NO_FACES  // ablation build only: no trunk faces
  if (false) {
#else
  if (T.patch) {  // the tunnel; on the plane the corners are the faces' deepest points
#endif
    // the vertices chosen at the control step's first sim step (at the top of phys_substep)
    face_force(T, C, R, S.pos, vb, th, H.face, wface, Fface);
  }
  MARK(faces_done);
  // ---- base: rigid inertia + quad sum of the four legs and the trunk corners
  const float* bb = model;
  const float mscale = (bb[0] + payload) * frcp(bb[0]);
  SIP I0;
  rigid_sip(bb, mscale, I0);
  f2 p0[3];
  float gb[3];
  rigid_bias2(bb, vbp, p0, mscale);
  mat3T_vec(R, g, gb);  // gravity in the base frame: added to the relative base acceleration below
#pragma unroll
  for (int k = 0; k < 6; ++k) Ip.ac[k] = f2{qsum(Ip.ac[k].x), qsum(Ip.ac[k].y)};
#pragma unroll
  for (int i = 0; i < 3; ++i) pp6[i] = f2{qsum(pp6[i].x - fbase[i]), qsum(pp6[i].y - fbase[3 + i])} - wface[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) Ip.b[i] = qsum(Ip.b[i]);
  sip_add(I0, Ip);
  float rhs[6], a0[6];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    rhs[i] = -(p0[i].x + pp6[i].x);
    rhs[3 + i] = -(p0[i].y + pp6[i].y);
  }
#ifdef GO1_ABL_NO_BASESOLVE  // ablation build only: the base's 6x6 solve replaced by a diagonal scaling
#pragma unroll
  for (int i = 0; i < 6; ++i) a0[i] = rhs[i] * 0.05f;
  (void)I0;
#else
#ifdef GO1_ABL_NO_CHOL  // ablation build only: the Cholesky alone compiled out, its inputs kept live
  float tr = 0.0f;
#pragma unroll
  for (int k = 0; k < 6; ++k) tr += I0.ac[k].x + I0.ac[k].y;
#pragma unroll
  for (int k = 0; k < 9; ++k) tr += I0.b[k];
#pragma unroll
  for (int i = 0; i < 6; ++i) a0[i] = rhs[i] * tr * 1e-3f;
#else
  solve6p(I0, rhs, a0);
#endif
#endif
  MARK(base_solve_done);
  // ---- forward pass
  float qdd[3];
  {
    f2 ap[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ap[i] = f2{a0[i], a0[3 + i]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int ax = j == 0 ? 0 : 1;
      f2 aj[3];
      xm2(ax, cs[j][0], cs[j][1], offset_mask(j), origin + j * 3, ap, aj);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i != ax) aj[i] += cjp[j][i];  // pair ax of c_j is zero
      const f2 ua = Up[j][0] * aj[0] + Up[j][1] * aj[1] + Up[j][2] * aj[2];
      qdd[j] = (u[j] - (ua.x + ua.y)) * D[j];
      aj[ax].x += qdd[j];
#pragma unroll
      for (int i = 0; i < 3; ++i) ap[i] = aj[i];
    }
  }
  MARK(forward_done);
  // ---- semi-implicit Euler (base identical in the quad)
  float wxv[3];
  cross3(vb, vb + 3, wxv);
  // a0 is relative to free fall: the base's linear acceleration is a0_lin + g; (angular, linear)
  // body-frame accelerations as pairs, rotated to the world and integrated together
  f2 ab[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) ab[i] = f2{a0[i], a0[3 + i] + gb[i] + wxv[i]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    S.wv[i] += h * (R[3 * i] * ab[0] + R[3 * i + 1] * ab[1] + R[3 * i + 2] * ab[2]);
    S.pos[i] += h * S.wv[i].y;
  }
  {
    const float w[3] = {S.wv[0].x, S.wv[1].x, S.wv[2].x};
    const float wn2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const float iwn = frsq(fmaxf(wn2, 1e-30f));
    const float wn = wn2 * iwn;
    const float thh = 0.5f * h * wn;
    float sth, cth;
    hw_sincosf(thh, &sth, &cth);
    const float sc = thh > 1e-12f ? sth * iwn : 0.5f * h;
    const float dq[4] = {w[0] * sc, w[1] * sc, w[2] * sc, cth};
    float* q = S.quat;
    float nq[4];
    nq[3] = dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2];
    nq[0] = dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1];
    nq[1] = dq[3] * q[1] - dq[0] * q[2] + dq[1] * q[3] + dq[2] * q[0];
    nq[2] = dq[3] * q[2] + dq[0] * q[1] - dq[1] * q[0] + dq[2] * q[3];
    const float inv = frsq(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = nq[i] * inv;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    S.qd[j] += h * qdd[j];
    S.q[j] += h * S.qd[j];
  }
  MARK(integrate_done);
  // this lane's contact forces of the sub-step (the last sub-step's survive the loop); summed
  // over the roles once, after the loop (cf_sum): no branch and no cross-lane work here
  (void)cf_out;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    cf_raw[i] = Fpt[i].x + Fo[i];
    cf_raw[3 + i] = Fpt[i].y;
    cf_raw[6 + i] = Fbs[i] + (role == 0 && leg == 0 ? Fface[i] : 0.0f);  // summed over the env's lanes (cf_sum)
  }
}

// reported contact forces from the last sub-step's per-lane values: thigh, calf, foot and hip of the lane's leg
// (role sums), the base (role and leg sums).  cf_raw: world forces of the lane's x half (with its primitive's
// self-contact force) and y half -- rows 0 (thigh, thigh), 1 (hip, corner), 2 (calf, calf), 3 (foot, corner) --
// then the trunk's self-collision reaction and faces
#define CF_RAW 9
__device__ __forceinline__ void cf_sum(const float* cf_raw, int role, float* cf_leg, float* cf_base, float* cf_hip) {
  float v[15];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float x = cf_raw[i], y = cf_raw[3 + i];
    v[i] = role == 0 ? x + y : 0.0f;                      // thigh
    v[3 + i] = role == 2 ? x + y : 0.0f;                  // calf
    v[6 + i] = role == 3 ? x : 0.0f;                      // foot
    v[9 + i] = role == 1 ? x : 0.0f;                      // hip
    v[12 + i] = ((role & 1) ? y : 0.0f) + cf_raw[6 + i];  // trunk corners, self-collision reactions, faces
  }
  rowsum4_n<15>(v);
#pragma unroll
  for (int i = 0; i < 9; ++i) cf_leg[i] = v[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    cf_base[i] = qsum(v[12 + i]);
    cf_hip[i] = v[9 + i];
  }
}
