// go1_render.hip -- ray caster of the collision scene (include/go1_render.h).
//
// One 256-thread workgroup draws one 16 x 16 pixel tile of one view.  Its first lanes pose the robot's 17
// primitives and the camera from the env's state planes into LDS, all lanes stage the env's terrain tile in LDS
// (when it fits), then every lane traces one ray: analytic ray / capsule, sphere and box tests for the waves
// whose rays pass the robot's bounding sphere, and a 2-D grid walk over the terrain cells along the ray's (x, y)
// projection that tests both triangles of both layers in each cell.
//
// Non-finite inputs, by construction:
//  * a view whose camera basis, root state or joint angles are not all finite is written as background before
//    any geometry is touched (Shared::ok, set by lane 17 of render_kernel);
//  * the grid walk's trip count is the integer hf_nx + hf_ny + 2; no loop bound is computed from a float;
//  * every cell index is clamped to [0, n - 2] as a float before its conversion and again as an integer before the
//    loads (cell_h), env ids, tile ids, marker counts and the frame slot are clamped integers;
//  * every hit test has the form (t > 0 && t < best), false for a NaN.
// The error message and the launch check are go1_host.h's, shared with the other add-on libraries.
#include "../../include/go1_render.h"
#include "go1_host.h"

namespace {

constexpr int TILE = 16;
constexpr int NPRIM = 17;
constexpr int LDS_TILE_MAX = 48 * 1024;  // bytes of terrain staged in LDS; larger tiles are read from global memory
constexpr float BIG = 3.0e38f;

struct f3 {
  float x, y, z;
};
__device__ inline f3 mk(float x, float y, float z) { return {x, y, z}; }
__device__ inline f3 operator+(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline f3 operator-(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline f3 operator*(float s, f3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ inline float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline f3 cross(f3 a, f3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline f3 normalize(f3 a) { return (1.0f / sqrtf(dot(a, a))) * a; }
__device__ inline bool finite3(f3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

struct M3 {
  f3 r0, r1, r2;  // rows
};
__device__ inline f3 mul(const M3& m, f3 v) { return {dot(m.r0, v), dot(m.r1, v), dot(m.r2, v)}; }
__device__ inline f3 mulT(const M3& m, f3 v) { return v.x * m.r0 + v.y * m.r1 + v.z * m.r2; }
__device__ inline M3 mul(const M3& a, const M3& b) {
  f3 c0 = mul(a, mk(b.r0.x, b.r1.x, b.r2.x)), c1 = mul(a, mk(b.r0.y, b.r1.y, b.r2.y)),
     c2 = mul(a, mk(b.r0.z, b.r1.z, b.r2.z));
  return {{c0.x, c1.x, c2.x}, {c0.y, c1.y, c2.y}, {c0.z, c1.z, c2.z}};
}
__device__ inline M3 rot_x(float q) {
  float c = cosf(q), s = sinf(q);
  return {{1, 0, 0}, {0, c, -s}, {0, s, c}};
}
__device__ inline M3 rot_y(float q) {
  float c = cosf(q), s = sinf(q);
  return {{c, 0, s}, {0, 1, 0}, {-s, 0, c}};
}
__device__ inline M3 quat_to_R(const float* q) {
  float x = q[0], y = q[1], z = q[2], w = q[3];
  return {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
          {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
          {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
}

// what one workgroup shares
struct Shared {
  float prim[NPRIM - 1][8];  // capsules in the world frame: a[3], b[3], radius, segment length
  float marker[GO1_RENDER_MAX_MARKERS + 1][4];
  f3 pos, fwd, right, up;    // camera
  f3 root;                   // trunk box frame
  M3 R;
  int n_marker;
  int ok;
};

struct Hit {
  float t;
  float shade;  // |n . dir|
  int prim;
  float fu, fv;  // terrain: frac(u), frac(v) at the hit
};

__device__ inline void take(Hit& h, float t, float shade, int prim) {
  bool c = t > 0.0f && t < h.t;
  h.t = c ? t : h.t;
  h.shade = c ? shade : h.shade;
  h.prim = c ? prim : h.prim;
}

// [enter, exit] of the ray in the sphere (c, r); enter > exit: missed
__device__ inline void sphere_span(f3 o, f3 d, f3 c, float r, float& lo, float& hi) {
  f3 oc = o - c;
  float b = dot(oc, d);
  f3 q = oc - b * d;
  float disc = r * r - dot(q, q);
  float s = sqrtf(fmaxf(disc, 0.0f));
  bool ok = disc >= 0.0f;
  lo = ok ? -b - s : BIG;
  hi = ok ? -b + s : -BIG;
}

// first hit with a capsule a -> b (length L; L = 0: a sphere), two-sided.  The capsule is convex, so the ray
// meets it in one interval: [min of the parts' entries, max of their exits] over the two end spheres and the
// cylinder between the end planes.
__device__ inline void capsule_hit(Hit& h, f3 o, f3 d, const float* p, int prim) {
  f3 a = mk(p[0], p[1], p[2]), b = mk(p[3], p[4], p[5]);
  float r = p[6], L = p[7];
  float lo, hi, l2, h2;
  sphere_span(o, d, a, r, lo, hi);
  sphere_span(o, d, b, r, l2, h2);
  lo = fminf(lo, l2);
  hi = fmaxf(hi, h2);
  bool seg = L > 1e-9f;
  f3 u = (1.0f / fmaxf(L, 1e-9f)) * (b - a);
  f3 oc = o - a;
  float ocu = dot(oc, u), du = dot(d, u);
  f3 op = oc - ocu * u, dp = d - du * u;
  float A = dot(dp, dp);
  bool par = A < 1e-12f;  // the ray runs along the axis: inside the cylinder for every t, or never
  float tm = -dot(op, dp) / fmaxf(A, 1e-12f);
  f3 q = op + tm * dp;
  float disc = r * r - dot(q, q);
  float half = sqrtf(fmaxf(disc, 0.0f) / fmaxf(A, 1e-12f));
  float c0 = par ? -BIG : tm - half, c1 = par ? BIG : tm + half;
  bool cyl = seg && disc >= 0.0f;
  // between the end planes: 0 <= ocu + t du <= L
  bool flat = fabsf(du) < 1e-12f;
  float inv = 1.0f / (flat ? 1.0f : du);
  float s0 = (0.0f - ocu) * inv, s1 = (L - ocu) * inv;
  float smin = flat ? -BIG : fminf(s0, s1), smax = flat ? BIG : fmaxf(s0, s1);
  cyl = cyl && !(flat && (ocu < 0.0f || ocu > L));
  c0 = fmaxf(c0, smin);
  c1 = fminf(c1, smax);
  cyl = cyl && c0 <= c1;
  lo = cyl ? fminf(lo, c0) : lo;
  hi = cyl ? fmaxf(hi, c1) : hi;
  bool any = lo <= hi;
  float t = lo > 0.0f ? lo : hi;
  t = any ? t : -1.0f;
  // normal: from the closest point of the segment
  f3 P = o + t * d;
  float s = fminf(fmaxf(dot(P - a, u), 0.0f), L);
  f3 n = (1.0f / r) * (P - (a + s * u));
  take(h, t, fabsf(dot(n, d)), prim);
}

// the trunk box in its own frame (half extents e), two-sided
__device__ inline void box_hit(Hit& h, f3 o, f3 d, const float* e) {
  float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
  float lo = -BIG, hi = BIG, nlo = 0.0f, nhi = 0.0f;
  bool miss = false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    bool flat = fabsf(dd[i]) < 1e-12f;
    float inv = 1.0f / (flat ? 1.0f : dd[i]);
    float t1 = (-e[i] - oo[i]) * inv, t2 = (e[i] - oo[i]) * inv;
    float tn = flat ? -BIG : fminf(t1, t2), tf = flat ? BIG : fmaxf(t1, t2);
    miss = miss || (flat && fabsf(oo[i]) > e[i]);
    nlo = tn > lo ? fabsf(dd[i]) : nlo;
    lo = fmaxf(lo, tn);
    nhi = tf < hi ? fabsf(dd[i]) : nhi;
    hi = fminf(hi, tf);
  }
  bool any = !miss && lo <= hi;
  bool front = lo > 0.0f;
  float t = any ? (front ? lo : hi) : -1.0f;
  take(h, t, front ? nlo : nhi, GO1_PRIM_TRUNK);
}

struct Terrain {
  const float* h;  // (2, nx, ny): LDS or global
  int nx, ny;
  float ox, oy, hs;
  bool ceiling;
};

__device__ inline float cell_h(const Terrain& T, int layer, int i, int j) {
  i = min(max(i, 0), T.nx - 1);
  j = min(max(j, 0), T.ny - 1);
  return T.h[(layer * T.nx + i) * T.ny + j];
}

__device__ inline float fracf(float x) { return x - floorf(x); }

// both triangles of one layer in cell (ci, cj): a = u - ci, b = v - cj along the ray are a0 + t du, b0 + t dv
__device__ inline void cell_hit(Hit& h, const Terrain& T, int layer, int ci, int cj, float a0, float b0, float du,
                                float dv, float oz, float dz, int prim) {
  const float EPS = 1e-5f;  // the triangles overlap by this much (cell units), so no ray slips between two of them
  float h00 = cell_h(T, layer, ci, cj), h10 = cell_h(T, layer, ci + 1, cj);
  float h01 = cell_h(T, layer, ci, cj + 1), h11 = cell_h(T, layer, ci + 1, cj + 1);
#pragma unroll
  for (int up = 0; up < 2; ++up) {
    float da = up ? h11 - h01 : h10 - h00, db = up ? h01 - h00 : h11 - h10;
    float den = dz - du * da - dv * db;
    float t = (h00 + a0 * da + b0 * db - oz) / den;  // den = 0: inf or NaN, refused below
    float a = a0 + t * du, b = b0 + t * dv;
    bool in = up ? (a >= -EPS && b <= 1.0f + EPS && a <= b + EPS) : (b >= -EPS && a <= 1.0f + EPS && a + EPS >= b);
    float gx = da / T.hs, gy = db / T.hs;
    float shade = fabsf(den) / sqrtf(gx * gx + gy * gy + 1.0f);  // |(-gx, -gy, 1) . dir| / |n|; du = dir.x / hs
    bool c = in && t > 0.0f && t < h.t;
    h.t = c ? t : h.t;
    h.shade = c ? shade : h.shade;
    h.prim = c ? prim : h.prim;
    h.fu = c ? fracf(a) : h.fu;
    h.fv = c ? fracf(b) : h.fv;
  }
}

__device__ inline void terrain_hit(Hit& h, const Terrain& T, f3 o, f3 d) {
  float ou = (o.x - T.ox) / T.hs, ov = (o.y - T.oy) / T.hs;
  float du = d.x / T.hs, dv = d.y / T.hs;
  // where the ray is over the vertex grid [0, nx - 1] x [0, ny - 1]
  float t0 = 0.0f, t1 = BIG;
  bool miss = false;
  bool flat_u = fabsf(du) < 1e-9f, flat_v = fabsf(dv) < 1e-9f;
  {
    float inv = 1.0f / (flat_u ? 1.0f : du);
    float ta = (0.0f - ou) * inv, tb = ((float)(T.nx - 1) - ou) * inv;
    t0 = flat_u ? t0 : fmaxf(t0, fminf(ta, tb));
    t1 = flat_u ? t1 : fminf(t1, fmaxf(ta, tb));
    miss = miss || (flat_u && (ou < 0.0f || ou > (float)(T.nx - 1)));
  }
  {
    float inv = 1.0f / (flat_v ? 1.0f : dv);
    float ta = (0.0f - ov) * inv, tb = ((float)(T.ny - 1) - ov) * inv;
    t0 = flat_v ? t0 : fmaxf(t0, fminf(ta, tb));
    t1 = flat_v ? t1 : fminf(t1, fmaxf(ta, tb));
    miss = miss || (flat_v && (ov < 0.0f || ov > (float)(T.ny - 1)));
  }
  if (miss || !(t0 <= t1)) return;
  float pu = ou + t0 * du, pv = ov + t0 * dv;
  int ci = (int)fminf(fmaxf(floorf(pu), 0.0f), (float)(T.nx - 2));
  int cj = (int)fminf(fmaxf(floorf(pv), 0.0f), (float)(T.ny - 2));
  int si = du > 0.0f ? 1 : -1, sj = dv > 0.0f ? 1 : -1;
  float tdu = flat_u ? BIG : fabsf(1.0f / du), tdv = flat_v ? BIG : fabsf(1.0f / dv);
  float tmu = flat_u ? INFINITY : ((float)(ci + (si > 0)) - ou) / du;
  float tmv = flat_v ? INFINITY : ((float)(cj + (sj > 0)) - ov) / dv;
  const int trips = T.nx + T.ny + 2;
  for (int k = 0; k < trips; ++k) {
    ci = min(max(ci, 0), T.nx - 2);
    cj = min(max(cj, 0), T.ny - 2);
    float a0 = ou - (float)ci, b0 = ov - (float)cj;
    float before = h.t;
    cell_hit(h, T, 1, ci, cj, a0, b0, du, dv, o.z, d.z, GO1_PRIM_FLOOR);
    if (T.ceiling) cell_hit(h, T, 0, ci, cj, a0, b0, du, dv, o.z, d.z, GO1_PRIM_CEILING);
    float tnext = fminf(tmu, tmv);
    // cells are visited in the order of t: a hit inside this cell ends the walk, and so does the grid's edge
    if (h.t < before || h.t <= tnext || !(tnext < t1)) break;
    bool su = tmu < tmv;
    ci += su ? si : 0;
    cj += su ? 0 : sj;
    tmu += su ? tdu : 0.0f;
    tmv += su ? 0.0f : tdv;
    if (ci < 0 || ci > T.nx - 2 || cj < 0 || cj > T.ny - 2) break;
  }
}

struct Params {
  go1_render_args a;
  const uint8_t* reset;
  int32_t* state;
  int32_t capacity;
  int32_t record;
  uint64_t step;
  int32_t lds_tile;  // the terrain tile is staged in LDS
};

__constant__ const unsigned char kColours[GO1_RC_COUNT][3] = GO1_RENDER_COLOURS;

__device__ inline int prim_class(int prim) {
  if (prim < 0) return GO1_RC_BACKGROUND;
  if (prim < 16) {
    int k = prim & 3;
    return k == 0 ? GO1_RC_THIGH : k == 1 ? GO1_RC_HIP : k == 2 ? GO1_RC_CALF : GO1_RC_FOOT;
  }
  return prim == GO1_PRIM_TRUNK ? GO1_RC_TRUNK : prim == GO1_PRIM_FLOOR ? GO1_RC_FLOOR
       : prim == GO1_PRIM_CEILING ? GO1_RC_CEILING : GO1_RC_MARKER;
}

__global__ __launch_bounds__(256) void render_kernel(const Params p) {
  extern __shared__ float s_tile[];
  __shared__ Shared S;
  const go1_render_args& A = p.a;
  const int tid = threadIdx.y * TILE + threadIdx.x;
  const int view = blockIdx.z;
  uint8_t* rgba = A.rgba;
  if (p.record) {
    // every workgroup reads the same copy of the record; one lane writes the other copy
    const int32_t* cur = p.state + 4 * (int)(p.step & 1);
    int st = cur[0], cnt = min(max(cur[1], 0), p.capacity);
    const int env0 = min(max(A.views[0].env, 0), A.n_envs - 1);
    const bool rs = p.reset[env0] != 0;
    bool draw = false;
    if (st == GO1_REC_ARMED && rs) {
      st = GO1_REC_RECORDING;
      cnt = 0;
      draw = true;
    } else if (st == GO1_REC_RECORDING) {
      if (rs) st = GO1_REC_COMPLETE;
      else draw = true;
    }
    draw = draw && cnt < p.capacity;
    const int slot = min(cnt, p.capacity - 1);
    if (draw && ++cnt >= p.capacity) st = GO1_REC_COMPLETE;
    if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
      int32_t* nxt = p.state + 4 * (int)((p.step + 1) & 1);
      nxt[0] = st;
      nxt[1] = cnt;
    }
    if (!draw) return;
    rgba += (size_t)slot * A.height * A.width * 4;
  }
  const go1_render_view V = A.views[view];
  const int env = min(max(V.env, 0), A.n_envs - 1);
  const float* root = A.root + (size_t)env * 13;
  const float* q = A.dof_pos + (size_t)env * 12;
  const go1_render_model& M = A.model;

  // ---- the first lanes pose the scene
  if (tid < 16) {
    const int l = tid >> 2, k = tid & 3;
    M3 Rb = quat_to_R(root + 3);
    f3 pb = mk(root[0], root[1], root[2]);
    M3 R0 = rot_x(q[3 * l]), R1 = mul(R0, rot_y(q[3 * l + 1])), R2 = mul(R1, rot_y(q[3 * l + 2]));
    f3 p0 = mk(M.hip_origin[l][0], M.hip_origin[l][1], M.hip_origin[l][2]);
    f3 p1 = p0 + mul(R0, mk(M.thigh_origin[l][0], M.thigh_origin[l][1], M.thigh_origin[l][2]));
    f3 p2 = p1 + mul(R1, mk(M.calf_origin[0], M.calf_origin[1], M.calf_origin[2]));
    f3 ft = p2 + mul(R2, mk(M.foot_offset[0], M.foot_offset[1], M.foot_offset[2]));
    f3 h0 = p0 + mul(R0, mk(0.0f, M.hip_capsule_y[l][0], 0.0f)), h1 = p0 + mul(R0, mk(0.0f, M.hip_capsule_y[l][1], 0.0f));
    f3 a = k == 0 ? p1 : k == 1 ? h0 : k == 2 ? p2 : ft;
    f3 b = k == 0 ? p2 : k == 1 ? h1 : ft;
    float r = k == 0 ? M.thigh_radius : k == 1 ? M.hip_radius : k == 2 ? M.calf_radius : M.foot_radius;
    f3 d = b - a;
    a = pb + mul(Rb, a);
    b = pb + mul(Rb, b);
    float* o = S.prim[tid];
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = b.x, o[4] = b.y, o[5] = b.z, o[6] = r;
    o[7] = k == 3 ? 0.0f : sqrtf(dot(d, d));
  } else if (tid == 16) {
    S.R = quat_to_R(root + 3);
    S.root = mk(root[0], root[1], root[2]);
  } else if (tid == 17) {
    f3 pos, at;
    if (V.mode == 0) {
      pos = mk(root[0] - 0.495f, root[1], 0.35f);
      at = mk(root[0], root[1], 0.25f);
    } else if (V.mode == 1) {
      pos = mk(root[0], root[1] - 1.0f, root[2] + 1.0f);
      at = mk(root[0], root[1], root[2]);
    } else {
      pos = mk(V.pos[0], V.pos[1], V.pos[2]);
      at = mk(V.look_at[0], V.look_at[1], V.look_at[2]);
    }
    f3 f = normalize(at - pos);
    f3 upv = (fabsf(f.x) < 1e-6f && fabsf(f.y) < 1e-6f) ? mk(1, 0, 0) : mk(0, 0, 1);
    f3 right = normalize(cross(f, upv));
    f3 up = cross(right, f);
    bool ok = finite3(pos) && finite3(f) && finite3(right) && finite3(up);
    for (int i = 0; i < 13; ++i) ok = ok && isfinite(root[i]);
    for (int i = 0; i < 12; ++i) ok = ok && isfinite(q[i]);
    S.pos = pos, S.fwd = f, S.right = right, S.up = up;
    S.ok = ok ? 1 : 0;
  } else if (tid == 18) {
    int m = 0;
    const int nm = A.markers ? min(max(A.n_markers, 0), GO1_RENDER_MAX_MARKERS) : 0;
    for (; m < nm; ++m)
      for (int c = 0; c < 4; ++c) S.marker[m][c] = A.markers[((size_t)view * A.n_markers + m) * 4 + c];
    if (A.wp_trajectory && A.wp_index && A.wp_length > 0) {
      int idx = min(max(A.wp_index[env], 0), A.wp_length - 1);
      const float* w = A.wp_trajectory + ((size_t)env * A.wp_length + idx) * 6;
      S.marker[m][0] = w[0], S.marker[m][1] = w[1], S.marker[m][2] = w[2], S.marker[m][3] = A.wp_radius;
      ++m;
    }
    S.n_marker = m;
  }
  // ---- every lane stages the terrain tile
  Terrain T;
  T.h = nullptr;
  T.nx = max(A.hf_nx, 2), T.ny = max(A.hf_ny, 2);
  T.hs = A.horizontal_scale;
  T.ox = T.oy = 0.0f;
  T.ceiling = !(V.flags & GO1_VIEW_NO_CEILING);
  if (A.tiles) {
    const int tile = min(max(A.env_tile[env], 0), A.n_tiles - 1);
    const float* g = A.tiles + (size_t)tile * 2 * T.nx * T.ny;
    T.ox = A.env_terrain_origin[(size_t)env * 3], T.oy = A.env_terrain_origin[(size_t)env * 3 + 1];
    if (p.lds_tile) {
      const int nf = 2 * T.nx * T.ny;
      for (int i = tid; i < nf; i += 256) s_tile[i] = g[i];
      T.h = s_tile;
    } else {
      T.h = g;
    }
  }
  __syncthreads();

  const int col = blockIdx.x * TILE + threadIdx.x, row = blockIdx.y * TILE + threadIdx.y;
  const bool inside = col < A.width && row < A.height;
  Hit h;
  h.t = INFINITY, h.shade = 1.0f, h.prim = GO1_PRIM_BACKGROUND, h.fu = h.fv = 0.5f;
  if (S.ok) {
    const float sx = 2.0f * ((float)col + 0.5f) / (float)A.width - 1.0f;
    const float sy = (1.0f - 2.0f * ((float)row + 0.5f) / (float)A.height) * ((float)A.height / (float)A.width);
    const f3 o = S.pos;
    const f3 d = normalize(S.fwd + sx * S.right + sy * S.up);
    // the robot: only the waves with a ray through its bounding sphere run the primitive tests
    f3 oc = S.root - o;
    float along = dot(oc, d);
    f3 perp = oc - along * d;
    const float br = M.bound_radius;
    bool sees = inside && dot(perp, perp) <= br * br && along > -br;
    if (__ballot(sees) != 0ull) {
#pragma unroll 1
      for (int k = 0; k < NPRIM - 1; ++k) capsule_hit(h, o, d, S.prim[k], k);
      f3 ob = mulT(S.R, o - S.root), db = mulT(S.R, d);
      box_hit(h, ob, db, M.trunk_half);
    }
    const int nm = S.n_marker;
    for (int m = 0; m < nm; ++m) {
      float lo, hi;
      f3 c = mk(S.marker[m][0], S.marker[m][1], S.marker[m][2]);
      float r = S.marker[m][3];
      sphere_span(o, d, c, r, lo, hi);
      float t = lo <= hi ? (lo > 0.0f ? lo : hi) : -1.0f;
      f3 n = (1.0f / r) * (o + t * d - c);
      take(h, t, fabsf(dot(n, d)), GO1_PRIM_MARKER);
    }
    // the terrain
    if (T.h) {
      terrain_hit(h, T, o, d);
    } else {
      float t = -o.z / d.z;
      bool c = t > 0.0f && t < h.t;
      f3 P = o + t * d;
      h.fu = c ? fracf(P.x / T.hs) : h.fu;
      h.fv = c ? fracf(P.y / T.hs) : h.fv;
      take(h, t, fabsf(d.z), GO1_PRIM_FLOOR);
    }
  }
  if (!inside) return;
  const int cls = prim_class(h.prim);
  float s = h.prim < 0 ? 1.0f : GO1_RENDER_AMBIENT + GO1_RENDER_DIFFUSE * fminf(h.shade, 1.0f);
  bool terrain = h.prim == GO1_PRIM_FLOOR || h.prim == GO1_PRIM_CEILING;
  if (terrain && (h.fu < GO1_RENDER_GRID_FRAC || h.fv < GO1_RENDER_GRID_FRAC)) s *= GO1_RENDER_GRID_DARK;
  const size_t px = ((size_t)view * A.height + row) * A.width + col;
  uchar4 c;
  c.x = (unsigned char)fminf(floorf((float)kColours[cls][0] * s + 0.5f), 255.0f);
  c.y = (unsigned char)fminf(floorf((float)kColours[cls][1] * s + 0.5f), 255.0f);
  c.z = (unsigned char)fminf(floorf((float)kColours[cls][2] * s + 0.5f), 255.0f);
  c.w = 255;
  reinterpret_cast<uchar4*>(rgba)[px] = c;
  if (A.depth) A.depth[px] = h.t;
  if (A.prim_id) A.prim_id[px] = h.prim;
}

int check_args(const go1_render_args* a) {
  if (!a) return fail("go1_render: null args");
  if (!a->root || !a->dof_pos || !a->views || !a->rgba) return fail("go1_render: root, dof_pos, views and rgba must be set");
  if (a->n_envs < 1 || a->n_views < 1 || a->n_views > 65535) return fail("go1_render: n_envs >= 1 and 1 <= n_views <= 65535");
  if (a->width < 1 || a->height < 1 || a->width > 16384 || a->height > 16384)
    return fail("go1_render: width and height must be in 1..16384");
  if (!(a->horizontal_scale > 0.0f) || !(a->horizontal_scale < 1e6f)) return fail("go1_render: horizontal_scale must be positive");
  if (a->tiles) {
    if (!a->env_tile || !a->env_terrain_origin) return fail("go1_render: tiles need env_tile and env_terrain_origin");
    if (a->hf_nx < 2 || a->hf_ny < 2 || a->hf_nx > 4096 || a->hf_ny > 4096 || a->n_tiles < 1)
      return fail("go1_render: a terrain tile has 2..4096 vertices per side and n_tiles >= 1");
  }
  if (a->markers && (a->n_markers < 0 || a->n_markers > GO1_RENDER_MAX_MARKERS))
    return fail("go1_render: at most GO1_RENDER_MAX_MARKERS markers per view");
  if (a->wp_trajectory && (!a->wp_index || a->wp_length < 1 || !(a->wp_radius > 0.0f)))
    return fail("go1_render: a waypoint marker needs wp_index, wp_length >= 1 and wp_radius > 0");
  if (!(a->model.bound_radius > 0.0f)) return fail("go1_render: model.bound_radius must be positive");
  return 0;
}

int launch(Params& p, void* stream) {
  const go1_render_args& a = p.a;
  size_t lds = 0;
  p.lds_tile = 0;
  if (a.tiles) {
    size_t bytes = (size_t)2 * a.hf_nx * a.hf_ny * sizeof(float);
    if (bytes <= (size_t)LDS_TILE_MAX) {
      lds = bytes;
      p.lds_tile = 1;
    }
  }
  dim3 grid((a.width + TILE - 1) / TILE, (a.height + TILE - 1) / TILE, a.n_views), block(TILE, TILE, 1);
  hipLaunchKernelGGL(render_kernel, grid, block, lds, (hipStream_t)stream, p);
  return launched("go1_render");
}

}  // namespace

extern "C" {

int go1_render_abi_version(void) { return GO1_RENDER_ABI_VERSION; }

void go1_render_abi_sizes(int64_t out[4]) {
  out[0] = sizeof(go1_render_model);
  out[1] = sizeof(go1_render_view);
  out[2] = sizeof(go1_render_args);
  out[3] = sizeof(go1_record_args);
}

GO1_LAST_ERROR(go1_render)

int go1_render(const go1_render_args* args, void* stream) {
  if (check_args(args)) return -1;
  Params p{};
  p.a = *args;
  return launch(p, stream);
}

int go1_render_record(const go1_record_args* args, void* stream) {
  if (!args) return fail("go1_render_record: null args");
  if (check_args(&args->r)) return -1;
  if (!args->reset || !args->state || args->capacity < 1) return fail("go1_render_record: reset, state and capacity >= 1 must be set");
  if (args->r.depth || args->r.prim_id) return fail("go1_render_record: depth and prim_id must be NULL");
  Params p{};
  p.a = args->r;
  p.a.n_views = 1;
  p.reset = args->reset;
  p.state = args->state;
  p.capacity = args->capacity;
  p.record = 1;
  p.step = args->step;
  return launch(p, stream);
}

}  // extern "C"
