// go1_contact.h -- the integrator's contact queries: the terrain view and its LDS patch, the linearly implicit point
// contact, the capsules' deepest-point search, the patch placement, the trunk faces.
#pragma once
#ifndef GO1_DEVICE_H
#error "include go1_device.h: its parts are not self-contained"
#endif
#pragma clang fp contract(on)  // integrator code, compared with the f64 oracle within a tolerance

// Terrain view of one env.  `patch` is an LDS copy of the PSZX x PSZY cells around
// the env's base at the start of the step, floor and ceiling interleaved, filled
// once per step by the whole block; the integrator's contact queries hit it and
// fall back to the HBM tile outside it (identical values: a pure cache).
// 20 rows (x) x 16 columns (y): the legs' bounding box spans up to 14 cells in x and 12 in y
// (p99 under N(0, 1) actions), the patch is placed on its centre, and the rows leave room for
// the motion during the step
#define PSZX 20
#define PSZY 16
static_assert(PSZY == 16 && PSZX % 2 == 0, "the LDS-DMA patch staging maps 2 rows of 16 cells to a wave");
struct Terr {
  const float* tile;  // (2, nx, ny) or nullptr
  int nx, ny;
  float hs;             // queries are relative to the env's terrain origin
  const float2* patch;  // LDS, PSZX x PSZY (floor, ceiling) or nullptr
  int pi0, pj0;
};

__device__ __forceinline__ float tile_at(const Terr& T, int layer, int i, int j) {
  i = min(max(i, 0), T.nx - 1);
  j = min(max(j, 0), T.ny - 1);
  return T.tile[((size_t)layer * T.nx + i) * T.ny + j];
}

struct CP {
  float k, d, kf, mu;
  float e, vb;  // restitution (the env's and the terrain's, averaged) and the bounce threshold
};

// ---- packed (v_pk_*_f32) contact: one wave issues a v_pk_fma_f32 (two FMAs) as fast as a
// v_fma_f32 (tools/probes/pk_rate.hip), so the floor and ceiling layers of a point are
// carried as the two halves of an f2 all the way from the mesh triangle to the force.

// (floor, ceiling) at the four corners of cell (i, j): the LDS patch, or the tile outside it
// (the patch read unconditionally, the tile only in a wave with a lane outside the patch: as an if / else per lane
// the two paths were exec-mask branches every call)
__device__ __forceinline__ void cell_fetch(const Terr& T, int i, int j, f2& c00, f2& c10, f2& c01, f2& c11) {
  const unsigned li = (unsigned)(i - T.pi0), lj = (unsigned)(j - T.pj0);
  const bool in = (T.patch != nullptr) & (li < (unsigned)(PSZX - 1)) & (lj < (unsigned)(PSZY - 1));
  if (T.patch) {
    const float2* pp = T.patch + (in ? (int)(li * PSZY + lj) : 0);
    const float2 q00 = pp[0], q01 = pp[1], q10 = pp[PSZY], q11 = pp[PSZY + 1];
    c00 = f2{q00.x, q00.y}; c01 = f2{q01.x, q01.y}; c10 = f2{q10.x, q10.y}; c11 = f2{q11.x, q11.y};
  }
  if (__any(!in)) {
    if (!in) {
      c00 = f2{tile_at(T, 1, i, j), tile_at(T, 0, i, j)};
      c10 = f2{tile_at(T, 1, i + 1, j), tile_at(T, 0, i + 1, j)};
      c01 = f2{tile_at(T, 1, i, j + 1), tile_at(T, 0, i, j + 1)};
      c11 = f2{tile_at(T, 1, i + 1, j + 1), tile_at(T, 0, i + 1, j + 1)};
    }
  }
}

// (floor, ceiling) heights and gradients at world (x, y) in two halves, so that the corner reads are issued early and
// land while independent work runs: hq_fetch reads the cell's four (floor, ceiling) corners -- the LDS patch stores
// (floor, ceiling) per cell, i.e. already in f2 layout; the HBM tile outside it -- and hq_finish evaluates the
// triangle's plane.
struct HQ {
  f2 c00, c10, c01, c11;
  float a, b;
  bool up;  // the cell's upper triangle (a < b): (i, j), (i + 1, j + 1), (i, j + 1); else (i, j), (i + 1, j), (i + 1, j + 1)
};
__device__ __forceinline__ void hq_fetch(const Terr& T, float x, float y, HQ& q) {
  if (!T.tile) {
    q.c00 = q.c10 = q.c01 = q.c11 = f2{0.0f, 1e9f};
    q.a = q.b = 0.0f;
    q.up = false;
    return;
  }
  const float ihs = frcp(T.hs);
  const float u = fminf(fmaxf(x * ihs, -4.0f), (float)(T.nx + 4));
  const float v = fminf(fmaxf(y * ihs, -4.0f), (float)(T.ny + 4));
  const float fu = floorf(u), fv = floorf(v);
  q.a = u - fu;
  q.b = v - fv;
  q.up = q.a < q.b;
  cell_fetch(T, (int)fu, (int)fv, q.c00, q.c10, q.c01, q.c11);
}
// the cell and triangle of a capsule's deepest point (SEG_CELL, seg_deepest2): a = u - i, b = v - j on that triangle's
// plane, so at a mesh edge the normal is the one of the triangle the search chose, not whichever side floor() of a
// rounded coordinate lands on (which the f32 kernel and the f64 oracle would decide differently)
__device__ __forceinline__ void hq_fetch_cell(const Terr& T, float x, float y, int cell, HQ& q) {
  if (!T.tile) {
    q.c00 = q.c10 = q.c01 = q.c11 = f2{0.0f, 1e9f};
    q.a = q.b = 0.0f;
    q.up = false;
    return;
  }
  const float ihs = frcp(T.hs);
  const float u = fminf(fmaxf(x * ihs, -4.0f), (float)(T.nx + 4));
  const float v = fminf(fmaxf(y * ihs, -4.0f), (float)(T.ny + 4));
  const int i = (cell >> 16) - 16384, j = (cell & 0x7fff) - 16384;
  q.a = u - (float)i;
  q.b = v - (float)j;
  q.up = (cell >> 15) & 1;
  cell_fetch(T, i, j, q.c00, q.c10, q.c01, q.c11);
}
// height and gradient of (floor, ceiling) on the triangle.  Round 6: the surface is the heightfield's triangle mesh,
// as the reference collides with it (mesh_type 'trimesh'; tunnel.py:139-147 builds it with isaacgym terrain_utils.
// convert_heightfield_to_trimesh: every cell split along its (i, j) - (i + 1, j + 1) diagonal); oracle tri_query
__device__ __forceinline__ void hq_finish(const Terr& T, const HQ& q, f2& h, f2& gx, f2& gy) {
  const float ihs = frcp(T.hs);
  const f2 da = q.up ? q.c11 - q.c01 : q.c10 - q.c00, db = q.up ? q.c01 - q.c00 : q.c11 - q.c10;
  h = q.c00 + q.a * da + q.b * db;
  gx = da * ihs;
  gy = db * ihs;
}

// Restitution.  PhysX bounces a contact whose relative velocity exceeds the bounce threshold with the
// coefficient e (the average of the two shapes').  A penalty contact has no impact event to attach a velocity
// target to (no per-contact state), so e acts on the dissipation of the rebound: while a point separates
// faster than the threshold, the explicit part of the normal force gets + e (h k + d) vn, i.e. the fraction e
// of the linearly implicit contact's damping (the physical d and the h k of the implicit spring) is handed
// back; the added mass h (h k + d) n n^T stays, so the velocity update keeps a contraction factor
// (m + e c) / (m + c) <= 1 (c = h (h k + d)): no e in [0, 1] adds energy (tests/test_self_collision.py).
// e = 0 leaves the force bit for bit as before.
__device__ __forceinline__ f2 restitute(const CP& C, float h, f2 vn, f2 fn) {
  const float cr = (h * C.k + C.d) * C.e;
  return f2{(C.e > 0.0f & vn.x > C.vb) ? fn.x + cr * vn.x : fn.x, (C.e > 0.0f & vn.y > C.vb) ? fn.y + cr * vn.y : fn.y};
}

// The same contact, linearly implicit in the point velocity (the integrator's scheme: one 5 ms step
// per sim step, like PhysX's substeps = 1).  For an active layer the force at the end of the step,
// k (depth - h vn') - d vn' (normal) and -c_t vt' (regularised friction, c_t = min(kf, mu fn / |vt|)
// from the current state), with v' = v + h a_p, splits into an explicit force F and an added mass
//   Mp = h (h k + d) n n^T + h c_t (I - n n^T)
// on the point (world frame, summed over floor and ceiling; xx xy xz yy yz zz), which the caller
// puts into the link's articulated inertia, so the ABA accelerations include the contact response.
// oracle/go1_oracle.c sphere_contact_im is the f64 restatement.
__device__ __forceinline__ void sphere_contact_im(const Terr& T, const HQ& q, const CP& C, const float* p,
                                                  const float* pv, float r, float h, float* F, float* Mp) {
  f2 hh, gx, gy;
  hq_finish(T, q, hh, gx, gy);
  const f2 sg = f2{1.0f, -1.0f};
  const f2 dv = sg * (hh - p[2]) + r;  // floor: h + r - z, ceiling: z + r - h
  f2 nx = -sg * gx, ny = -sg * gy;
  f2 inv = nx * nx + ny * ny + 1.0f;
  inv = f2{frsq(inv.x), frsq(inv.y)};
  nx = nx * inv;
  ny = ny * inv;
  const f2 nz = sg * inv;
  const f2 depth = dv * inv;
  const f2 vn = pv[0] * nx + pv[1] * ny + pv[2] * nz;
  const f2 fn0 = C.k * depth - C.d * vn;          // activation: compressive at the current state
  const f2 fn = restitute(C, h, vn, fn0 - (h * C.k) * vn);  // k depth - (h k + d) vn [+ e (h k + d) vn]
  const f2 vtx = pv[0] - vn * nx, vty = pv[1] - vn * ny, vtz = pv[2] - vn * nz;
  const f2 vt2 = vtx * vtx + vty * vty + vtz * vtz;
  const f2 ivt = f2{frsq(fmaxf(vt2.x, 1e-18f)), frsq(fmaxf(vt2.y, 1e-18f))};
  const f2 vtn = vt2 * ivt;
  const f2 cm = C.mu * fn0;
  // c_t = min(kf, mu fn0 / |vt|); kf in the viscous limit |vt| -> 0
  const f2 ct = f2{(C.kf * vtn.x > cm.x & vtn.x > 1e-9f) ? cm.x * ivt.x : C.kf,
                   (C.kf * vtn.y > cm.y & vtn.y > 1e-9f) ? cm.y * ivt.y : C.kf};
  const bool ax = dv.x > 0.0f & fn0.x > 0.0f, ay = dv.y > 0.0f & fn0.y > 0.0f;
  const f2 fa = f2{ax ? fn.x : 0.0f, ay ? fn.y : 0.0f};
  const f2 sc = f2{ax ? ct.x : 0.0f, ay ? ct.y : 0.0f};
  const f2 Fx = fa * nx - sc * vtx, Fy = fa * ny - sc * vty, Fz = fa * nz - sc * vtz;
  F[0] = Fx.x + Fx.y;
  F[1] = Fy.x + Fy.y;
  F[2] = Fz.x + Fz.y;
  const float cn = h * (h * C.k + C.d);
  const f2 cd = h * sc, cnd = f2{ax ? cn : 0.0f, ay ? cn : 0.0f} - cd;  // (cn - cd) on active layers
  const f2 a = cnd * nx, b = cnd * ny, c = cnd * nz;
  const f2 mxx = a * nx + cd, mxy = a * ny, mxz = a * nz, myy = b * ny + cd, myz = b * nz, mzz = c * nz + cd;
  Mp[0] = mxx.x + mxx.y; Mp[1] = mxy.x + mxy.y; Mp[2] = mxz.x + mxz.y;
  Mp[3] = myy.x + myy.y; Mp[4] = myz.x + myz.y; Mp[5] = mzz.x + mzz.y;
}

__device__ __forceinline__ void point_kin(const float* Rb, const float* pb, const float* vb, const float* lp, float* pw,
                                          float* vw) {
  float wl[3], vl[3];
  cross3(vb, lp, wl);
  vl[0] = vb[3] + wl[0]; vl[1] = vb[4] + wl[1]; vl[2] = vb[5] + wl[2];
  float t[3];
  mat3_vec(Rb, lp, t);
  pw[0] = pb[0] + t[0]; pw[1] = pb[1] + t[1]; pw[2] = pb[2] + t[2];
  mat3_vec(Rb, vl, vw);
}

// ---- capsules against the heightfield meshes (round 6; oracle/go1_oracle.c seg_deepest is the f64 restatement).  A
// capsule (segment A -> B, radius r) acts at the deepest point of its segment: the t in [0, 1] that maximises the
// vertical gap of either layer, floor h_f + r - z and ceiling z + r - h_c.  Both layers are triangle meshes over the
// grid (hq_finish), so along the segment the gaps are piecewise linear in t and their maximum lies at an end or where
// the segment's (x, y) projection crosses a mesh edge: a grid line u = k or v = k, or a cell diagonal u - v = k.  The
// candidates are exactly those (on an edge the height interpolates its two vertices): exact, and no serial walk --
// every candidate's reads are independent.  A half link of 0.1065 m crosses at most 3 lines of each grid direction
// and 4 diagonals at 0.05 m cells (go1_create rejects finer grids).  Each candidate carries the cell and triangle on
// the segment's incoming side of its edge; the contact takes that triangle's plane (hq_fetch_cell).  A candidate's
// key is its deeper layer's gap quantised to 1e-5 m, ties to the smaller t (the segment's first end; the link halves
// start at their outer ends, so a link lying flat is carried at both): this f32 search and the oracle's f64 one
// choose the same point.  On the plane: the lower end (ties: A).  The search runs once per control step; the chosen t
// is held for the control step's sim steps (phys_substep), as the trunk faces' vertices are.
#define SEG_QI 1.0e5f  // 1 / SEG_Q of the oracle
__device__ __forceinline__ int seg_quant(float g) { return (int)floorf(fminf(fmaxf(g, -1.0f), 1.0f) * SEG_QI); }
// cell (i, j in [-4, n + 4]) and triangle (up: the upper one) packed into a positive int
#define SEG_CELL(i, j, up) ((((i) + 16384) << 16) | ((up) ? 0x8000 : 0) | ((j) + 16384))
struct SegBest {
  int key;   // the best candidate's key: quantised gap (the deeper layer) x 4096 + the earlier t (4095 - 4095 t)
  float t;   // its t
  int cell;  // and its cell and triangle
};
__device__ __forceinline__ void seg_offer(SegBest& sb, f2 h, float z, float r, float t, int cell, bool valid) {
  const int q = seg_quant(fmaxf((h.x - z) + r, (z - h.y) + r));  // (the quantisation is monotone: = the max of both)
  const int key = q * 4096 + (4095 - (int)floorf(t * 4095.0f));
  const bool up = valid & (key > sb.key);  // an equal key (a vertex on several edges) keeps the first offer
  sb.key = up ? key : sb.key;
  sb.t = up ? t : sb.t;
  sb.cell = up ? cell : sb.cell;
}
// the (floor, ceiling) mesh vertices (vi, vj): the LDS patch in one batch of reads, then the HBM tile for the rare
// ones outside it (a wave-uniform branch), so the wave waits for the patch once per batch
template <int N>
__device__ __forceinline__ void verts_fetch(const Terr& T, const int* vi, const int* vj, f2* h) {
  unsigned out = T.patch ? 0u : (1u << N) - 1u;
  if (T.patch) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
      // (unsigned: a negative offset is out of range too; outside the patch read cell 0, replaced below)
      const unsigned li = (unsigned)(vi[n] - T.pi0), lj = (unsigned)(vj[n] - T.pj0);
      const bool in = (li < (unsigned)PSZX) & (lj < (unsigned)PSZY);
      const float2 q = T.patch[in ? (int)(li * PSZY + lj) : 0];
      h[n] = f2{q.x, q.y};
      out |= in ? 0u : 1u << n;
    }
  }
  if (__any(out != 0u)) {
#pragma unroll
    for (int n = 0; n < N; ++n)
      if ((out >> n) & 1u) h[n] = f2{tile_at(T, 1, vi[n], vj[n]), tile_at(T, 0, vi[n], vj[n])};
  }
}
// the plane: the lower end (ties: A)
__device__ __forceinline__ float seg_plane(const float* A, const float* B, float r, int& cell) {
  cell = SEG_CELL(0, 0, false);
  return seg_quant(r - B[2]) > seg_quant(r - A[2]) ? 1.0f : 0.0f;
}
// deepest point of one segment (world ends A, B): t and SEG_CELL.  The candidates, offered in this order (seg_offer
// keeps the first of equal keys): end A, end B, NU lines u = k, NV lines v = k, ND diagonals.  <3, 3, 4> holds every
// crossing of a half link (above); <1, 1, 2> those of a segment shorter than one cell (SEG_SHORT_MAX).  Two batches
// of candidates (the ends and the lines u = k; the lines v = k and the diagonals), each gathering its mesh vertices
// (verts_fetch) before comparing them -- or, ONE_BATCH, all 6 + 2 (NU + NV + ND) vertices in one gather with one wait
struct SegLine {  // the segment in cell units, its first end's cell
  float uA, vA, uB, vB, du, dv, dw, dz, zA, zB, r;
  int iA, jA;
};
// the first batch's candidates -- the ends (vertices c00, c11 and c01 on the upper triangle / c10) and the grid lines
// u = k (the edge (k, j) - (k, j + 1), entered from cell k - 1 (du > 0) or k) -- and their 6 + 2 NU vertices
template <int NU>
struct SegFirst {
  float ca[2 + NU], cb[2], ct[NU];
  int ccell[2 + NU];
  bool cup[2], cval[NU];
};
template <int NU>
__device__ __forceinline__ void seg_first(const SegLine& L, SegFirst<NU>& c, int* vi, int* vj) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float u = e ? L.uB : L.uA, v = e ? L.vB : L.vA;
    const float fu = floorf(u), fv = floorf(v);
    const int i = (int)fu, j = (int)fv;
    c.ca[e] = u - fu;
    c.cb[e] = v - fv;
    c.cup[e] = c.ca[e] < c.cb[e];
    c.ccell[e] = SEG_CELL(i, j, c.cup[e]);
    vi[3 * e] = i; vj[3 * e] = j;
    vi[3 * e + 1] = i + 1; vj[3 * e + 1] = j + 1;
    vi[3 * e + 2] = c.cup[e] ? i : i + 1; vj[3 * e + 2] = c.cup[e] ? j + 1 : j;
  }
  const int k0 = (int)floorf(fminf(L.uA, L.uB)) + 1;
  const float hi = fmaxf(L.uA, L.uB), rdu = L.du != 0.0f ? frcp(L.du) : 0.0f;
#pragma unroll
  for (int m = 0; m < NU; ++m) {
    const int k = k0 + m, n = 6 + 2 * m;
    const bool valid = (float)k < hi;
    const float t = valid ? ((float)k - L.uA) * rdu : 0.0f, v = L.vA + L.dv * t, fv = floorf(v), b = v - fv;
    const int j = (int)fv, i = L.du > 0.0f ? k - 1 : k;
    c.ct[m] = t; c.ca[2 + m] = b; c.cval[m] = valid;
    c.ccell[2 + m] = SEG_CELL(i, j, (float)(k - i) < b);
    // an invalid candidate (beyond the segment's crossings) reads A's cell instead of an edge up to 4 cells off,
    // which could leave the LDS patch
    vi[n] = valid ? k : L.iA; vj[n] = valid ? j : L.jA;
    vi[n + 1] = vi[n]; vj[n + 1] = vj[n] + 1;
  }
}
template <int NU>
__device__ __forceinline__ void seg_first_offer(const SegLine& L, const SegFirst<NU>& c, const f2* h, SegBest& sb) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const f2 c00 = h[3 * e], c11 = h[3 * e + 1], cx = h[3 * e + 2];
    const f2 da = c.cup[e] ? c11 - cx : cx - c00, db = c.cup[e] ? cx - c00 : c11 - cx;
    seg_offer(sb, c00 + c.ca[e] * da + c.cb[e] * db, e ? L.zB : L.zA, L.r, (float)e, c.ccell[e], true);
  }
#pragma unroll
  for (int m = 0; m < NU; ++m) {
    const f2 p0 = h[6 + 2 * m], p1 = h[7 + 2 * m];
    seg_offer(sb, p0 + c.ca[2 + m] * (p1 - p0), L.zA + L.dz * c.ct[m], L.r, c.ct[m], c.ccell[2 + m], c.cval[m]);
  }
}
// the second batch's -- the grid lines v = k (the edge (i, k) - (i + 1, k), entered from cell k - 1 (dv > 0) or k)
// and the cell diagonals u - v = k (the point (i + a, j + a) of cell (i, j), i - j = k, entered from the upper
// triangle (dw > 0: u - v grows through k, a < b before) or the lower) -- and their 2 (NV + ND) vertices
template <int NL>
struct SegSecond {
  float ca[NL], ct[NL];
  int ccell[NL];
  bool cval[NL];
};
template <int NV, int ND>
__device__ __forceinline__ void seg_second(const SegLine& L, SegSecond<NV + ND>& c, int* vi, int* vj) {
  {
    const int k0 = (int)floorf(fminf(L.vA, L.vB)) + 1;
    const float hi = fmaxf(L.vA, L.vB), rdv = L.dv != 0.0f ? frcp(L.dv) : 0.0f;
#pragma unroll
    for (int m = 0; m < NV; ++m) {
      const int k = k0 + m, n = 2 * m;
      const bool valid = (float)k < hi;
      const float t = valid ? ((float)k - L.vA) * rdv : 0.0f, u = L.uA + L.du * t, fu = floorf(u), a = u - fu;
      const int i = (int)fu, j = L.dv > 0.0f ? k - 1 : k;
      c.ct[m] = t; c.ca[m] = a; c.cval[m] = valid;
      c.ccell[m] = SEG_CELL(i, j, a < (float)(k - j));
      vi[n] = valid ? i : L.iA; vj[n] = valid ? k : L.jA;
      vi[n + 1] = vi[n] + 1; vj[n + 1] = vj[n];
    }
  }
  {
    const float wA = L.uA - L.vA, wB = L.uB - L.vB;
    const int k0 = (int)floorf(fminf(wA, wB)) + 1;
    const float hi = fmaxf(wA, wB), rdw = L.dw != 0.0f ? frcp(L.dw) : 0.0f;
#pragma unroll
    for (int m = 0; m < ND; ++m) {
      const int k = k0 + m, cc = NV + m, n = 2 * cc;
      const bool valid = (float)k < hi;
      const float t = valid ? ((float)k - wA) * rdw : 0.0f, u = L.uA + L.du * t, fu = floorf(u), a = u - fu;
      const int i = (int)fu, j = i - k;
      c.ct[cc] = t; c.ca[cc] = a; c.cval[cc] = valid;
      c.ccell[cc] = SEG_CELL(i, j, L.dw > 0.0f);
      vi[n] = valid ? i : L.iA; vj[n] = valid ? j : L.jA;
      vi[n + 1] = vi[n] + 1; vj[n + 1] = vj[n] + 1;
    }
  }
}
template <int NL>
__device__ __forceinline__ void seg_second_offer(const SegLine& L, const SegSecond<NL>& c, const f2* h, SegBest& sb) {
#pragma unroll
  for (int k = 0; k < NL; ++k) {
    const f2 p0 = h[2 * k], p1 = h[2 * k + 1];
    seg_offer(sb, p0 + c.ca[k] * (p1 - p0), L.zA + L.dz * c.ct[k], L.r, c.ct[k], c.ccell[k], c.cval[k]);
  }
}
template <int NU = 3, int NV = 3, int ND = 4, bool ONE_BATCH = false>
__device__ __forceinline__ float seg_deepest(const Terr& T, const float* A, const float* B, float r, int& cell) {
  if (!T.tile) return seg_plane(A, B, r, cell);
  constexpr int N1 = 6 + 2 * NU, N2 = 2 * (NV + ND);
  const float ihs = frcp(T.hs);
  SegLine L;
  L.uA = fminf(fmaxf(A[0] * ihs, -4.0f), (float)(T.nx + 4)); L.vA = fminf(fmaxf(A[1] * ihs, -4.0f), (float)(T.ny + 4));
  L.uB = fminf(fmaxf(B[0] * ihs, -4.0f), (float)(T.nx + 4)); L.vB = fminf(fmaxf(B[1] * ihs, -4.0f), (float)(T.ny + 4));
  L.du = L.uB - L.uA; L.dv = L.vB - L.vA; L.dw = L.du - L.dv; L.dz = B[2] - A[2]; L.zA = A[2]; L.zB = B[2];
  L.r = r;
  L.iA = (int)floorf(L.uA); L.jA = (int)floorf(L.vA);
  SegBest sb;
  sb.key = -2147483647 - 1;
  sb.t = 0.0f;
  sb.cell = SEG_CELL(0, 0, false);
  if constexpr (ONE_BATCH) {
    int vi[N1 + N2], vj[N1 + N2];
    SegFirst<NU> c1;
    SegSecond<NV + ND> c2;
    seg_first<NU>(L, c1, vi, vj);
    seg_second<NV, ND>(L, c2, vi + N1, vj + N1);
    f2 h[N1 + N2];
    verts_fetch<N1 + N2>(T, vi, vj, h);
    seg_first_offer<NU>(L, c1, h, sb);
    seg_second_offer<NV + ND>(L, c2, h + N1, sb);
  } else {
    {
      int vi[N1], vj[N1];
      SegFirst<NU> c;
      seg_first<NU>(L, c, vi, vj);
      f2 h[N1];
      verts_fetch<N1>(T, vi, vj, h);
      seg_first_offer<NU>(L, c, h, sb);
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      int vi[N2], vj[N2];
      SegSecond<NV + ND> c;
      seg_second<NV, ND>(L, c, vi, vj);
      f2 h[N2];
      verts_fetch<N2>(T, vi, vj, h);
      seg_second_offer<NV + ND>(L, c, h, sb);
    }
  }
  cell = sb.cell;
  return sb.t;
}
// The short pass's bound.  A segment of SEG_SHORT_MAX metres on cells of at least SEG_MIN_HS (go1_create refuses
// finer grids) spans less than one cell, so it crosses at most 1 line u = k, 1 line v = k and, u - v moving by less
// than sqrt 2 cells, 2 diagonals: seg_deepest<1, 1, 2> offers every crossing it has.  The hip capsule is the longest
// such segment of the model (go1_create pins the model block bit for bit to go1_model_consts.h).
#define SEG_MIN_HS 0.0499f
#define SEG_SHORT_MAX (GO1_MODEL_F32[177] - GO1_MODEL_F32[176])  // hip_y1 - hip_y0
static_assert(SEG_SHORT_MAX > 0.0f && SEG_SHORT_MAX / SEG_MIN_HS < 1.0f, "the hip capsule crosses at most 1 grid line");
static_assert(SEG_SHORT_MAX / SEG_MIN_HS * 1.41421357f < 2.0f, "the hip capsule crosses at most 2 cell diagonals");
// The lane's two segments (x, y halves of the contact pass; lane = 16 role + ...).  Of a leg's eight (role, half)
// slots only four are half links, the length the full candidate set is for:
//   role 0: thigh half | thigh half     role 1: hip capsule (SEG_SHORT_MAX) | trunk corner (a point)
//   role 2: calf half  | calf half      role 3: foot (a point)              | trunk corner (a point)
// so the halves change rows first: swap16(x, y) holds by row a = [x0 y0 x2 y2], the four half links, and b =
// [x1 y1 x3 y3], the short segments.  One full pass over a and one short, single-batch pass over b then do the work
// of two full passes, and swap16(a, b) takes (t, cell) home.  rs: the radii of (a, b) on this lane, which are the
// model's by row and need no exchange.  Every candidate is computed on some lane exactly as before.
// The short pass runs first: in the other order the README-config kernel needs 498 registers instead of 494 and the
// generic kernels spill.
// The plane has no candidates and stays in place with no exchange where the view is the plane at compile time (the
// velocity kernel).  A run-time test here -- a branch around both passes -- cost the step kernels 45 to 75 spilled
// registers; there a plane config takes the exchange and seg_deepest's own test, with the same result.
__device__ __forceinline__ f2 seg_deepest2(const Terr& T, const f2* A, const f2* B, f2 r, f2 rs, int* cell) {
  if (__builtin_constant_p(T.tile == nullptr) && !T.tile) {
    const float a0[3] = {A[0].x, A[1].x, A[2].x}, b0[3] = {B[0].x, B[1].x, B[2].x};
    const float a1[3] = {A[0].y, A[1].y, A[2].y}, b1[3] = {B[0].y, B[1].y, B[2].y};
    const float tx = seg_plane(a0, b0, r.x, cell[0]), ty = seg_plane(a1, b1, r.y, cell[1]);
    return f2{tx, ty};
  }
  LanePair sA[3], sB[3];  // all swaps first, then their uses
#pragma unroll
  for (int i = 0; i < 3; ++i) sA[i] = swap16(A[i].x, A[i].y);
#pragma unroll
  for (int i = 0; i < 3; ++i) sB[i] = swap16(B[i].x, B[i].y);
  const float a0[3] = {sA[0].a, sA[1].a, sA[2].a}, b0[3] = {sB[0].a, sB[1].a, sB[2].a};
  const float a1[3] = {sA[0].b, sA[1].b, sA[2].b}, b1[3] = {sB[0].b, sB[1].b, sB[2].b};
  int ca, cb;
  const float tb = seg_deepest<1, 1, 2, true>(T, a1, b1, rs.y, cb);
  __builtin_amdgcn_sched_barrier(0);  // one segment's vertex batch live at a time
  const float ta = seg_deepest<3, 3, 4, false>(T, a0, b0, rs.x, ca);
  const LanePair t = swap16(ta, tb);
  const auto c = __builtin_amdgcn_permlane16_swap((uint32_t)ca, (uint32_t)cb, false, false);
  cell[0] = (int)c[0];
  cell[1] = (int)c[1];
  return f2{t.a, t.b};
}

// World position of this leg's foot body origin (rigid_body_state[:, feet, 0:3] after
// the last sim step), the kinematic chain of phys_substep without velocities.
__device__ void foot_world(const float* __restrict__ model, const float* root, const float* q, int leg, float* out) {
  float Rp[9], pp[3] = {root[0], root[1], root[2]};
  quat_to_R(root + 3, Rp);
  const float* origin = model + 13 * 10 + leg * 9;
  const float* foot = model + 13 * 10 + 4 * 9;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int ax = j == 0 ? 0 : 1;
    float rw[3], sn, cn;
    mat3_vec(Rp, origin + j * 3, rw);
    pp[0] += rw[0]; pp[1] += rw[1]; pp[2] += rw[2];
    pm_sincosf(q[j], &sn, &cn);
#pragma unroll
    for (int a = 0; a < 3; ++a) rE(ax, cn, sn, Rp + 3 * a, Rp + 3 * a);
  }
  float fw[3];
  mat3_vec(Rp, foot, fw);
  out[0] = pp[0] + fw[0]; out[1] = pp[1] + fw[1]; out[2] = pp[2] + fw[2];
}

// Centre (x, y) of the bounding box of the env's hips, knees and feet at the start of the
// step: the terrain patch is placed on it rather than on the base (16 x 16 cells around the
// base left ~6 % of the envs with a leg outside it, and one such lane sends its whole wave
// through the HBM fallback of every contact query).  Hardware sin / cos: only the placement
// of the patch depends on this, and the patch is a pure cache of the tile.
__device__ __forceinline__ void legs_bbox_centre(const float* pos, const float* quat, const float* q, int leg,
                                                 float* cx, float* cy) {
  const float sx = (leg & 2) ? -1.0f : 1.0f, sy = (leg & 1) ? -1.0f : 1.0f;
  float Rp[9], pp[3] = {pos[0], pos[1], pos[2]};
  quat_to_R(quat, Rp);
  float xmin = 1e30f, xmax = -1e30f, ymin = 1e30f, ymax = -1e30f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int i = 30 + 3 * j + k, sp = GO1_LEG_SIGN[i];
      o[k] = GO1_LEG_FL[i] * (sp == 0 ? 1.0f : (sp == 1 ? sx : (sp == 2 ? sy : sx * sy)));
    }
    float rw[3];
    mat3_vec(Rp, o, rw);
    pp[0] += rw[0]; pp[1] += rw[1]; pp[2] += rw[2];  // hip, thigh, calf (knee) origins
    if (j != 1) {
      xmin = fminf(xmin, pp[0]); xmax = fmaxf(xmax, pp[0]);
      ymin = fminf(ymin, pp[1]); ymax = fmaxf(ymax, pp[1]);
    }
    float sn, cn;
    __sincosf(q[j], &sn, &cn);
#pragma unroll
    for (int a = 0; a < 3; ++a) rE(j == 0 ? 0 : 1, cn, sn, Rp + 3 * a, Rp + 3 * a);
  }
  float fw[3];
  mat3_vec(Rp, GO1_MODEL_F32 + 13 * 10 + 4 * 9, fw);  // foot offset in the calf frame
  const float fx = pp[0] + fw[0], fy = pp[1] + fw[1];
  xmin = quad_min(fminf(xmin, fx)); xmax = quad_max(fmaxf(xmax, fx));
  ymin = quad_min(fminf(ymin, fy)); ymax = quad_max(fmaxf(ymax, fy));
  *cx = 0.5f * (xmin + xmax);
  *cy = 0.5f * (ymin + ymax);
}

// ---- the trunk box's faces against the heightfields (go1.urdf:53-58, the 0.3762 x 0.0935 x 0.114
// box; tunnel_fn.py:99-163, the ceiling's downward wedges).  The 8 box corners are contact points of the sub-step
// (above); a wedge apex or ridge that enters a face between its corners is a grid vertex of the heightfield
// inside the face's footprint (mesh triangles: a face's deepest point against them is a vertex or on the
// footprint's boundary).  Once per control step the env's 16 lanes scan the 10 x 10 vertices around the trunk
// (offsets -4 .. +5 on both axes: they hold the footprint's +-0.166 m at any yaw wherever the centre sits in its
// cell; 7 per lane, both layers in the halves: floor against the bottom face, ceiling against the top
// face) and keep, per face, the vertex inside the footprint nearest to (or deepest in) the face -- its signed
// depth, so a vertex that enters during the control step is already chosen -- compared quantised
// to 1e-5 m, ties to the lowest window position: a lexicographic maximum (associative: the same in any reduction
// order, and the oracle's).  Every sim step a penalty force acts at the two chosen vertices where they penetrate
// (face_force).  Scanning every sim step measured +3.7 k cycles per sim step per wave; the held choice is bounded
// by tests/test_held_contacts.py (held vs every sim step in the f64 oracle).
#define FACE_Q 1.0e-5f
#define FACE_W 10
__device__ __forceinline__ int face_key_max(int v) {  // max over the env's 16 lanes (quad, then the rows)
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));
  v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));
  auto a = __builtin_amdgcn_permlane16_swap((uint32_t)v, (uint32_t)v, false, false);
  v = max((int)a[0], (int)a[1]);
  auto b = __builtin_amdgcn_permlane32_swap((uint32_t)v, (uint32_t)v, false, false);
  return max((int)b[0], (int)b[1]);
}
#define FACE_SIGNED 0.1f  // signed depths from -0.1 m (a vertex farther from the face cannot reach it in a control step)
__device__ __forceinline__ void face_scan(const Terr& T, const float* R, const float* pos, const float* th, int sub16,
                                          int* sel) {
  const float ihs = frcp(T.hs);
  const int ci = (int)floorf(fminf(fmaxf(pos[0] * ihs, -16000.0f), 16000.0f));
  const int cj = (int)floorf(fminf(fmaxf(pos[1] * ihs, -16000.0f), 16000.0f));
  int key[2] = {-1, -1};
  // the lane's seven window vertices: every read issued, then one wait (read and used in one loop, each read was
  // waited for by itself: seven LDS round trips in a row)
  constexpr int NU = (FACE_W * FACE_W + 15) / 16;
  static_assert(NU == 7, "the operand list below");
  float2 hw[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int v = sub16 + 16 * u;
    const int li = ci + v % FACE_W - 4 - T.pi0, lj = cj + v / FACE_W - 4 - T.pj0;
    hw[u] = T.patch[min(max(li, 0), PSZX - 1) * PSZY + min(max(lj, 0), PSZY - 1)];
  }
  asm volatile("" : "+v"(hw[0].x), "+v"(hw[0].y), "+v"(hw[1].x), "+v"(hw[1].y), "+v"(hw[2].x), "+v"(hw[2].y),
                    "+v"(hw[3].x), "+v"(hw[3].y), "+v"(hw[4].x), "+v"(hw[4].y), "+v"(hw[5].x), "+v"(hw[5].y),
                    "+v"(hw[6].x), "+v"(hw[6].y));
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int v = sub16 + 16 * u;
    const int i = ci + v % FACE_W - 4, j = cj + v / FACE_W - 4;
    const int li = i - T.pi0, lj = j - T.pj0;
    const bool inp = (v < FACE_W * FACE_W) & (li >= 0) & (li < PSZX) & (lj >= 0) & (lj < PSZY);
    const float2 hv = hw[u];
    const float dx = (float)i * T.hs - pos[0], dy = (float)j * T.hs - pos[1];
    const f2 dz = f2{hv.x, hv.y} - pos[2];
    const f2 cx = (R[0] * dx + R[3] * dy) + R[6] * dz, cy = (R[1] * dx + R[4] * dy) + R[7] * dz,
             cz = (R[2] * dx + R[5] * dy) + R[8] * dz;
    const f2 pen = f2{cz.x + th[2], th[2] - cz.y};  // floor vertex above the bottom face / ceiling below the top
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const bool in = inp & (fabsf(cx[hh]) <= th[0]) & (fabsf(cy[hh]) <= th[1]) & (pen[hh] > -FACE_SIGNED);
      const int q = (int)floorf(fminf(pen[hh] + FACE_SIGNED, 10.0f) * (1.0f / FACE_Q));  // signed depth, offset
      const int k = in ? (q << 7) | (127 - v) : -1;
      key[hh] = max(key[hh], k);
    }
  }
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const int k = face_key_max(key[hh]);
    const int v = 127 - (k & 127);
    const int i = ci + v % FACE_W - 4, j = cj + v / FACE_W - 4;
    sel[hh] = k < 0 ? -1 : ((i + 16384) << 16) | (j + 16384);
  }
}
// the penalty force of the two chosen vertices at the current pose (explicit: the trunk's 5 kg keep h sqrt(k / m)
// = 0.3 and h d / m = 0.08): normal k depth - d vn along the face normal (base frame +z on the bottom face, -z on
// the top), regularised Coulomb friction as the point contacts, nothing when the vertex left the footprint.
// Adds the base-frame wrench (angular, linear pairs) to w and the world force to Fw.
__device__ __forceinline__ void face_force(const Terr& T, const CP& C, const float* R, const float* pos, const float* vb,
                                           const float* th, const int* sel, f2* w, float* Fw) {
  f2 cx, cy, cz;
  bool ok[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const int i = (sel[hh] >> 16) - 16384, j = (sel[hh] & 0xffff) - 16384;
    const int li = i - T.pi0, lj = j - T.pj0;
    ok[hh] = sel[hh] >= 0 & li >= 0 & li < PSZX & lj >= 0 & lj < PSZY;
    const float2 hv = T.patch[min(max(li, 0), PSZX - 1) * PSZY + min(max(lj, 0), PSZY - 1)];
    const float dx = (float)i * T.hs - pos[0], dy = (float)j * T.hs - pos[1], dz = (hh == 0 ? hv.x : hv.y) - pos[2];
    cx[hh] = (R[0] * dx + R[3] * dy) + R[6] * dz;
    cy[hh] = (R[1] * dx + R[4] * dy) + R[7] * dz;
    cz[hh] = (R[2] * dx + R[5] * dy) + R[8] * dz;
  }
  const f2 pen = f2{cz.x + th[2], th[2] - cz.y};
  bool act[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) act[hh] = ok[hh] & (fabsf(cx[hh]) <= th[0]) & (fabsf(cy[hh]) <= th[1]) & (pen[hh] > 0.0f);
  if (!__any(act[0] || act[1])) return;
  const f2 nz = f2{1.0f, -1.0f};
  // the trunk's velocity at the vertex, base frame: v + w x c
  const f2 vx = vb[3] + (vb[1] * cz - vb[2] * cy), vy = vb[4] + (vb[2] * cx - vb[0] * cz), vz = vb[5] + (vb[0] * cy - vb[1] * cx);
  const f2 depth = f2{fminf(pen.x, 2.0f * th[2]), fminf(pen.y, 2.0f * th[2])};
  const f2 vn = vz * nz;
  const f2 fn = C.k * depth - C.d * vn;
  const f2 vt2 = vx * vx + vy * vy;
  const f2 ivt = f2{frsq(fmaxf(vt2.x, 1e-18f)), frsq(fmaxf(vt2.y, 1e-18f))};
  const f2 vtn = vt2 * ivt, cm = C.mu * fn;
  const f2 ct = f2{(C.kf * vtn.x > cm.x & vtn.x > 1e-9f) ? cm.x * ivt.x : C.kf,
                   (C.kf * vtn.y > cm.y & vtn.y > 1e-9f) ? cm.y * ivt.y : C.kf};
  const bool ax = act[0] & (fn.x > 0.0f), ay = act[1] & (fn.y > 0.0f);
  const f2 fa = f2{ax ? fn.x : 0.0f, ay ? fn.y : 0.0f}, sc = f2{ax ? ct.x : 0.0f, ay ? ct.y : 0.0f};
  const f2 Fx = -(sc * vx), Fy = -(sc * vy), Fz = fa * nz;
  const f2 mx = cy * Fz - cz * Fy, my = cz * Fx - cx * Fz, mz = cx * Fy - cy * Fx;
  w[0] += f2{mx.x + mx.y, Fx.x + Fx.y};
  w[1] += f2{my.x + my.y, Fy.x + Fy.y};
  w[2] += f2{mz.x + mz.y, Fz.x + Fz.y};
  const float F[3] = {Fx.x + Fx.y, Fy.x + Fy.y, Fz.x + Fz.y};
#pragma unroll
  for (int i = 0; i < 3; ++i) Fw[i] += R[3 * i] * F[0] + R[3 * i + 1] * F[1] + R[3 * i + 2] * F[2];
}
