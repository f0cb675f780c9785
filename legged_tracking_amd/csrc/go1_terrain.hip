// go1_terrain.hip -- the tunnel terrains (single_path, narrow_path, random_pyramid) generated on the MI355X
// (SURVEY 8(f) row 3).
//
// Replaces the reference's init-time numpy loop over sub-terrains:
//   go1_gym/utils/tunnel.py:51-126 (Terrain.__init__: one difficulty draw, then a top and a bottom
//   SubTerrain per sub-terrain, the ceiling flip and 0.05 m clamp :96-98, the 0.8 m ceiling / 0.5 m
//   floor outside the tunnel :80-81) and :189-217 (add_terrain_to_map: the tunnel placed at
//   [start_x, end_x) x [start_y, end_y) of its tile), with
//   go1_gym/utils/tunnel_fn.py:99-163 (TerrainFunctions.single_path: up to two pyramidal wedges per
//   layer, heights from vec_plane_from_points :3-21, walls on the floor's border, int truncation),
//   :44-97 (TerrainFunctions.narrow_path: the same draws, one axis-aligned box per wedge written with a Python
//   slice) and :546-581 (TerrainFunctions.random_pyramid as tunnel.py:164-183 calls it: a jittered grid of up to
//   GO1_TUNNEL_MAX_WEDGES pyramids per layer, thinned by the sub-terrain's difficulty draw, no walls).
//
// Two launches on the caller's stream:
//   1. tunnel_draw_kernel (one wave): numpy's legacy RandomState stream -- MT19937 with
//      mt19937_seed seeding, random_sample doubles (a >> 5, b >> 6) / 2^53, uniform(low, high) =
//      low + (high - low) u -- drawn in the reference's order (the draw count of a single_path /
//      narrow_path layer depends on its own p2 draw and a random_pyramid sub-terrain's on its difficulty
//      draw, so the stream is sequential); the wave twists the 624-word state in parallel batches of 64.
//      single_path / narrow_path: every lane walks the stream in lockstep.  random_pyramid: the 5 n
//      doubles of a layer are consecutive once the difficulty is known, and the lanes share them.
//      Output: one record of wedge parameters per sub-terrain (GO1_TUNNEL_REC doubles through
//      go1_tunnel_tiles, GO1_TUNNEL_SPEC_REC through go1_tunnel_generate).
//   2. tunnel_tile_kernel (one 256-thread block per sub-terrain): the block's threads build the face planes
//      in LDS (up to 2 layers x GO1_TUNNEL_MAX_WEDGES wedges x 4 faces; numpy's np.cross / np.sum operation
//      order, f64) or narrow_path's box bounds, then the block rasterises both layers of the tile (min over a
//      wedge's faces, max over wedges; boxes in draw order, the last writer wins), coalesced f32 stores.
// Every f64 operation is the one numpy performs, in numpy's order, compiled without contraction
// (-ffp-contract=off), so a seed yields the reference's tiles bit for bit
// (tests/test_gpu_terrain.py and tests/test_gpu_terrain_kinds.py against terrain.make_tunnel, itself pinned
// to the reference's tiles by tests/test_terrain.py and tests/test_terrain_kinds.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/go1_mi355x.h"

#pragma clang fp contract(off)

int go1_internal_fail(int code, const std::string& msg);  // go1_step.hip: sets go1_last_error()

namespace {

constexpr int MT_N = 624, MT_M = 397;
constexpr uint32_t MT_MATRIX_A = 0x9908b0dfu, MT_UPPER = 0x80000000u, MT_LOWER = 0x7fffffffu;

// record layout (doubles): [0] difficulty, then per layer (0 top, 1 bottom) at 1 + 16 layer:
// p1, p2, num_y, off_y[2], off_x[2], mean_x[2], mean_z[2], pw[2], pl[2], (pad)
constexpr int REC_LAYER = 16;
static_assert(1 + 2 * REC_LAYER <= GO1_TUNNEL_REC, "record layout");
// random_pyramid's record (doubles): [0] difficulty, [1] d_num, [2 + layer] the layer's wedge count, then per
// layer at PYR_BASE + PYR_LAYER layer five rows of MAXW: mean_x, mean_y, mean_z, pw, pl (wedge = iy (num_x + 2) + ix,
// the C order of the reference's meshgrid)
constexpr int MAXW = GO1_TUNNEL_MAX_WEDGES;
constexpr int PYR_BASE = 8, PYR_LAYER = 5 * MAXW;
static_assert(PYR_BASE + 2 * PYR_LAYER <= GO1_TUNNEL_SPEC_REC && GO1_TUNNEL_REC <= GO1_TUNNEL_SPEC_REC, "record layout");

// the draw kernel's MT19937 state, LDS (file scope, not pointers in MtWave: with the stream's many call sites the
// compiler keeps mt_twist out of line, and LDS addresses carried in a struct then fail to compile)
__shared__ uint32_t s_mt_key[MT_N];  // the state words
__shared__ uint32_t s_mt_out[MT_N];  // the tempered words
struct MtWave {
  int pos;  // wave-uniform
};

// mt19937_gen of numpy (randomkit): key[i] = key[i + 397 mod 624] ^ twist(key[i], key[i + 1]),
// in place and in index order.  Batches of 64 consecutive indices are exact: within a batch every
// lane reads before any lane writes (one wave, in order), key[i + 1] is still old (same or a later
// batch) except for i = 623, whose key[0] was rewritten in the first batch as in the sequential
// loop, and key[i - 227] (i >= 227) was rewritten in an earlier batch (batch length 64 < 227).
__device__ void mt_twist(MtWave& s, int lane) {
  for (int b = 0; b < MT_N; b += 64) {
    const int i = b + lane;
    uint32_t nv = 0;
    if (i < MT_N) {
      const uint32_t y = (s_mt_key[i] & MT_UPPER) | (s_mt_key[i + 1 < MT_N ? i + 1 : 0] & MT_LOWER);
      nv = s_mt_key[i + MT_M < MT_N ? i + MT_M : i + MT_M - MT_N] ^ (y >> 1) ^ ((y & 1u) ? MT_MATRIX_A : 0u);
    }
    __syncthreads();  // (one-wave block) every lane's reads of this batch are done
    if (i < MT_N) s_mt_key[i] = nv;
    __syncthreads();
  }
  for (int i = lane; i < MT_N; i += 64) {  // tempering (mt19937_next32)
    uint32_t y = s_mt_key[i];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    s_mt_out[i] = y;
  }
  __syncthreads();
  s.pos = 0;
}

__device__ uint32_t mt_next32(MtWave& s, int lane) {
  if (s.pos == MT_N) mt_twist(s, lane);
  return s_mt_out[s.pos++];
}

// legacy random_sample / next_double: (a * 2^26 + b) / 2^53
__device__ double mt_next_double(MtWave& s, int lane) {
  const int32_t a = (int32_t)(mt_next32(s, lane) >> 5), b = (int32_t)(mt_next32(s, lane) >> 6);
  return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}

// RandomState.uniform(low, high): random_uniform(lower, range) = lower + range * u with
// range = high - low (mtrand.pyx), one double per element in C order
__device__ double uniform(MtWave& s, int lane, double lo, double hi) { return lo + (hi - lo) * mt_next_double(s, lane); }

// np.linspace(start, stop, num)[k] (numpy 2.x function_base.py): k * ((stop - start) / (num - 1))
// + start, the last element exactly stop; num = 1 gives [start] (0 * delta + start, no end point written)
__device__ __forceinline__ double linspace_at(double start, double stop, int num, int k) {
  if (num == 1) return start;
  if (k == num - 1) return stop;
  const double step = (stop - start) / (double)(num - 1);
  return (double)k * step + start;
}

// d_num of Terrain.make_terrain (tunnel.py:166-171)
__device__ __forceinline__ int pyramid_d_num(double difficulty) { return difficulty < 0.25 ? 2 : (difficulty < 0.625 ? 1 : 0); }

// One random_pyramid layer (tunnel_fn.py:550-560): 5 n consecutive doubles of the stream -- the x noise over the
// (num_y + 2, num_x + 2) meshgrid in C order, then the y noise, then mean_z, then pw and pl as the two rows of one
// (2, n) draw.  n is known once the difficulty is drawn, so the lanes share the layer's draws: double j of the layer
// is the word pair at pos + 2 j of the tempered buffer (pos stays even: every draw takes two words), in chunks that
// end where the buffer does.  mean_x is spread over l = pixel_x hs and mean_y over w = pixel_y hs, as the reference
// does (the pixel grid lays them the other way round).
__device__ __forceinline__ void pyramid_draw_layer(MtWave& s, int lane, const go1_pyramid_params& c, int d_num, double l,
                                                   double w, double* __restrict__ R, int layer) {
  const int nx2 = c.num_x - d_num + 2, ny2 = c.num_y - d_num + 2, n = nx2 * ny2, total = 5 * n;
  double* L = R + PYR_BASE + PYR_LAYER * layer;
  if (lane == 0) R[2 + layer] = (double)n;
  for (int done = 0; done < total;) {
    if (s.pos == MT_N) mt_twist(s, lane);
    const int chunk = min(total - done, (MT_N - s.pos) / 2);
    for (int j = lane; j < chunk; j += 64) {
      const int q = done + j, g = q / n, i = q - g * n;  // group (x, y, z, pw, pl) and wedge
      const int32_t a = (int32_t)(s_mt_out[s.pos + 2 * j] >> 5), b = (int32_t)(s_mt_out[s.pos + 2 * j + 1] >> 6);
      const double u = ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;  // mt_next_double
      double v;
      if (g == 0) {
        v = linspace_at(-l / 2.0, l / 2.0, nx2, i % nx2) + (-c.var_x + (c.var_x - -c.var_x) * u);
        v = v < -l / 2.0 ? -l / 2.0 : v;  // mean_x.clip(-l/2, l/2)
        v = v > l / 2.0 ? l / 2.0 : v;
      } else if (g == 1) {
        v = linspace_at(-w / 2.0, w / 2.0, ny2, i / nx2) + (-c.var_y + (c.var_y - -c.var_y) * u);
        v = v < -w / 2.0 ? -w / 2.0 : v;
        v = v > w / 2.0 ? w / 2.0 : v;
      } else if (g == 2) {
        v = c.height_min + (c.height_max - c.height_min) * u;
      } else {
        v = c.length_min + (c.length_max - c.length_min) * u;
      }
      L[g * MAXW + i] = v;
    }
    s.pos += 2 * chunk;
    done += chunk;
  }
}

__global__ __launch_bounds__(64) void tunnel_draw_kernel(go1_tunnel_spec sp, int stride, double* __restrict__ rec) {
  const go1_tunnel_params& p = sp.base;
  const int lane = threadIdx.x;
  MtWave s{MT_N};
  if (lane == 0) {  // mt19937_seed (legacy seeding of an integer seed)
    uint32_t v = p.seed;
    for (int i = 0; i < MT_N; ++i) {
      s_mt_key[i] = v;
      v = 1812433253u * (v ^ (v >> 30)) + (uint32_t)(i + 1);
    }
  }
  __syncthreads();
  // SubTerrain extent in metres (tunnel_fn.py:102): l = pixel_x hs, w = pixel_y hs
  const double w = (double)p.sub_y * p.horizontal_scale;
  // mean_x = np.linspace(-w/2, w/2, 3)[1:-1] (tunnel_fn.py:127): start + 1 * step
  const double start = -w / 2.0, stop = w / 2.0;
  const double step = (stop - start) / 2.0;
  const double cx = 1.0 * step + start;
  const int n_sub = p.num_rows * p.num_cols;
  if (sp.kind == GO1_TUNNEL_RANDOM_PYRAMID) {
    const double l = (double)p.sub_x * p.horizontal_scale;
    for (int k = 0; k < n_sub; ++k) {
      double* R = rec + (size_t)k * stride;
      const double diff = uniform(s, lane, 0.0, 1.0);  // difficulty (tunnel.py:90): one draw, both layers
      const int d_num = pyramid_d_num(diff);
      if (lane == 0) { R[0] = diff; R[1] = (double)d_num; }
      for (int layer = 0; layer < 2; ++layer) pyramid_draw_layer(s, lane, layer == 0 ? sp.top : sp.bottom, d_num, l, w, R, layer);
    }
    return;
  }
  // single_path and narrow_path: the same draws (tunnel_fn.py:50-80 = :105-135)
  for (int k = 0; k < n_sub; ++k) {
    double* R = rec + (size_t)k * stride;
    const double diff = uniform(s, lane, 0.0, 1.0);  // difficulty (tunnel.py:90), unused by these two
    if (lane == 0) R[0] = diff;
    for (int layer = 0; layer < 2; ++layer) {
      const bool top = layer == 0;
      const double p1 = uniform(s, lane, 0.0, 1.0), p2 = uniform(s, lane, 0.0, 1.0);
      const int num_y = p2 < p.p_double ? 2 : 1;
      // tunnel_fn.py:111-124: offsets y then x, each a (num_y, 1) draw (register arrays, static
      // indices: the draws are uniform branches on num_y)
      const double oy = top ? 0.6 : 0.4, ox = top ? 0.3 : 0.2;
      double offy[2] = {0.0, 0.0}, offx[2] = {0.0, 0.0}, mx[2] = {0.0, 0.0}, mz[2] = {0.0, 0.0};
      double pw[2] = {0.0, 0.0}, pl[2] = {0.0, 0.0};
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (i < num_y) offy[i] = uniform(s, lane, -oy, oy);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (i < num_y) offx[i] = uniform(s, lane, -ox, ox);
      double hmax, hmin;
      if (p1 < p.p_flat) { hmax = top ? 0.4 : 0.15; hmin = top ? 0.7 : 0.3; }
      else { hmax = 0.0; hmin = 0.0; }
      const double lw_lo = top ? 0.2 : 0.1, lw_hi = top ? 0.4 : 0.3;
      // mean_x (after meshgrid) += offset_x; mean_z = uniform(mean_x) * (hmax - hmin) + hmin
      // (uniform(low=mean_x, high=1.0): range = 1.0 - mean_x, element-wise)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (i < num_y) {
          mx[i] = cx + offx[i];
          const double u = mx[i] + (1.0 - mx[i]) * mt_next_double(s, lane);
          mz[i] = u * (hmax - hmin) + hmin;
        }
      // pw, pl = uniform(lw_low, lw_high, size=(2, num_y)): row 0 then row 1
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (i < num_y) pw[i] = uniform(s, lane, lw_lo, lw_hi);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (i < num_y) pl[i] = uniform(s, lane, lw_lo, lw_hi);
      if (lane == 0) {
        double* L = R + 1 + REC_LAYER * layer;
        L[0] = p1; L[1] = p2; L[2] = (double)num_y;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          L[3 + i] = offy[i]; L[5 + i] = offx[i]; L[7 + i] = mx[i]; L[9 + i] = mz[i];
          L[11 + i] = pw[i]; L[13 + i] = pl[i];
        }
      }
    }
  }
}

struct Face {
  double dc, ac, bc;  // d / c, a / c, b / c (vec_plane_from_points :15-18)
};

// the drawn parameters of wedge `wedge` of `layer` from sub-terrain record r (either layout)
struct Wedge {
  double mx, my, mz, pw, pl;
};
// (bounded by what the LDS arrays hold, whatever the record says)
__device__ __forceinline__ int wedge_count(int kind, const double* r, int layer) {
  return kind == GO1_TUNNEL_RANDOM_PYRAMID ? min(max((int)r[2 + layer], 0), MAXW)
                                           : min(max((int)r[1 + REC_LAYER * layer + 2], 0), 2);
}
__device__ __forceinline__ Wedge wedge_at(int kind, const double* r, int layer, int wedge) {
  if (kind == GO1_TUNNEL_RANDOM_PYRAMID) {
    const double* L = r + PYR_BASE + PYR_LAYER * layer + wedge;
    return Wedge{L[0], L[MAXW], L[2 * MAXW], L[3 * MAXW], L[4 * MAXW]};
  }
  const double* L = r + 1 + REC_LAYER * layer;
  return Wedge{L[7 + wedge], L[3 + wedge], L[9 + wedge], L[11 + wedge], L[13 + wedge]};
}

// [start, stop) of the Python slice lo:hi on an axis of n elements: a negative index counts from the end, both
// ends are clamped to the axis, stop <= start selects nothing (terrain.slice_bounds on the host)
__device__ __forceinline__ void box_bounds(int lo, int hi, int n, int& start, int& stop) {
  lo = lo < 0 ? lo + n : lo;
  hi = hi < 0 ? hi + n : hi;
  start = min(max(lo, 0), n);
  stop = max(min(max(hi, 0), n), start);
}
struct Box {
  int x0, x1, y0, y1;  // height_field_raw[x0:x1, y0:y1] = z
  double z;
};

__global__ __launch_bounds__(256) void tunnel_tile_kernel(go1_tunnel_spec sp, int stride, const double* __restrict__ rec,
                                                          const int32_t* __restrict__ extents,
                                                          float* __restrict__ tiles) {
  const go1_tunnel_params& p = sp.base;
  const int kind = sp.kind;
  __shared__ Face s_face[2][MAXW][4];  // layer, wedge, face
  __shared__ Box s_box[2][2];          // narrow_path: layer, wedge
  __shared__ int s_num[2];
  const int k = blockIdx.x;
  const double* r = rec + (size_t)k * stride;
  const int tid = threadIdx.x;
  if (tid < 2) s_num[tid] = wedge_count(kind, r, tid);
  if (kind == GO1_TUNNEL_NARROW_PATH) {
    if (tid < 4) {
      const int layer = tid >> 1, wedge = tid & 1;
      if (wedge < wedge_count(kind, r, layer)) {
        // tunnel_fn.py:82-87: the loop's w, l are the drawn sizes; int() truncates towards zero
        const Wedge W = wedge_at(kind, r, layer, wedge);
        const double hs = p.horizontal_scale;
        const int x_low = (int)((W.mx - W.pw / 2.0) / hs), x_high = (int)((W.mx + W.pw / 2.0) / hs);
        const int y_low = (int)((W.my - W.pl / 2.0) / hs), y_high = (int)((W.my + W.pl / 2.0) / hs);
        Box B;
        box_bounds(x_low, x_high, p.sub_x, B.x0, B.x1);
        box_bounds(y_low, y_high, p.sub_y, B.y0, B.y1);
        B.z = W.mz;
        s_box[layer][wedge] = B;
      }
    }
  } else {
    for (int f = tid; f < 2 * MAXW * 4; f += 256) {
      const int layer = f / (MAXW * 4), wedge = (f >> 2) & (MAXW - 1), face = f & 3;
      if (wedge >= wedge_count(kind, r, layer)) continue;
      const Wedge W = wedge_at(kind, r, layer, wedge);
      const double mx = W.mx, my = W.my, mz = W.mz, pw = W.pw, pl = W.pl;
      // wedge_points (tunnel_fn.py:134-141): corners (+-pw + mean_x, +-pl + mean_y, 0), apex = means;
      // faces [[0, 1, apex], [1, 2, apex], [2, 3, apex], [3, 0, apex]] (:142-148)
      const double cxs[4] = {pw + mx, -pw + mx, -pw + mx, pw + mx};
      const double cys[4] = {pl + my, pl + my, -pl + my, -pl + my};
      const int i1 = face, i2 = (face + 1) & 3;
      const double p1[3] = {cxs[i1], cys[i1], 0.0}, p2[3] = {cxs[i2], cys[i2], 0.0}, p3[3] = {mx, my, mz};
      const double v1[3] = {p3[0] - p1[0], p3[1] - p1[1], p3[2] - p1[2]};
      const double v2[3] = {p3[0] - p2[0], p3[1] - p2[1], p3[2] - p2[2]};
      // np.cross: each component a product minus a product, rounded separately
      const double t0 = v1[1] * v2[2], u0 = v1[2] * v2[1];
      const double t1 = v1[2] * v2[0], u1 = v1[0] * v2[2];
      const double t2 = v1[0] * v2[1], u2 = v1[1] * v2[0];
      const double a = t0 - u0, b = t1 - u1, c = t2 - u2;
      // np.sum(cp * p3, axis=-1): products, then a left-to-right sum
      const double d = (a * p3[0] + b * p3[1]) + c * p3[2];
      s_face[layer][wedge][face] = Face{d / c, a / c, b / c};
    }
  }
  __syncthreads();
  const int nx = p.tile_x, ny = p.tile_y, pix = nx * ny;
  const int sx = extents[4 * k], ex = extents[4 * k + 1], sy = extents[4 * k + 2], ey = extents[4 * k + 3];
  const int px = p.sub_x, py = p.sub_y;  // SubTerrain height_field_raw shape (pixel_x, pixel_y)
  const double hs = p.horizontal_scale, vs = p.vertical_scale;
  const double l = (double)px * hs, w = (double)py * hs;
  const double unit = (double)(int64_t)(1.0 / vs);
  const double ceil_out = unit * p.ceiling_height, floor_out = 0.5 * unit;  // tunnel.py:80-81
  const double ceil_raw = p.ceiling_height / vs, ceil_min = 0.05 / vs;   // tunnel.py:96-98
  float* out = tiles + (size_t)k * 2 * pix;
  for (int idx = tid; idx < 2 * pix; idx += 256) {
    const int layer = idx / pix, x = (idx % pix) / ny, y = idx % ny;
    double v;
    if (x >= sx && x < ex && y >= sy && y < ey) {
      // tile[layer, sx + a, sy + b] = height_field_raw.T[a, b] = height_field_raw[b, a]
      const int a = x - sx, b = y - sy;
      // points_coord[b, a] = (linspace(-w/2, w/2, pixel_y)[a], linspace(-l/2, l/2, pixel_x)[b])
      const double qx = linspace_at(-w / 2.0, w / 2.0, py, a), qy = linspace_at(-l / 2.0, l / 2.0, px, b);
      double h;
      if (kind != GO1_TUNNEL_RANDOM_PYRAMID && layer == 1 && (b == 0 || b == px - 1 || a == 0 || a == py - 1)) {
        h = 0.5;  // tunnel_fn.py:89-93, 155-159 (random_pyramid has no walls)
      } else if (kind == GO1_TUNNEL_NARROW_PATH) {
        h = 0.0;  // height_field_raw[x0:x1, y0:y1] = z in draw order: the last box over a pixel wins
        for (int wd = 0; wd < s_num[layer]; ++wd) {
          const Box& B = s_box[layer][wd];
          if (b >= B.x0 && b < B.x1 && a >= B.y0 && a < B.y1) h = B.z;
        }
      } else {
        h = 0.0;
        for (int wd = 0; wd < s_num[layer]; ++wd) {
          double hm = 0.0;
          for (int f = 0; f < 4; ++f) {
            const Face& F = s_face[layer][wd][f];
            double t = F.dc - F.ac * qx;
            t = t - F.bc * qy;
            t = t < 0.0 ? 0.0 : t;  // np.clip(., 0, inf)
            hm = f == 0 ? t : (t < hm ? t : hm);  // min over the wedge's faces
          }
          h = wd == 0 ? hm : (hm > h ? hm : h);  // max over wedges
        }
      }
      const double raw = (double)(int64_t)(h / vs);  // (height_field_raw / vertical_scale).astype(int)
      if (layer == 0) {
        v = ceil_raw - raw;
        v = v < ceil_min ? ceil_min : v;
      } else {
        v = raw;
      }
    } else {
      v = layer == 0 ? ceil_out : floor_out;
    }
    out[idx] = (float)(v * vs);  // (tiles * vertical_scale).astype(np.float32)
  }
}

// argument checks and the two launches behind both entry points (`who` names the entry in go1_last_error)
int tunnel_launch(const char* who, const go1_tunnel_spec& sp, int stride, const int32_t* extents, double* records,
                  float* tiles, void* stream) {
  const std::string w = std::string(who) + ": ";
  const go1_tunnel_params* p = &sp.base;
  if (!extents || !records || !tiles) return go1_internal_fail(GO1_E_ARG, w + "null argument");
  if (p->num_rows <= 0 || p->num_cols <= 0 || p->tile_x <= 0 || p->tile_y <= 0 || p->sub_x < 2 || p->sub_y < 2)
    return go1_internal_fail(GO1_E_ARG, w + "bad grid shape");
  if (!(p->vertical_scale > 0.0) || !(p->horizontal_scale > 0.0))
    return go1_internal_fail(GO1_E_ARG, w + "scales must be > 0");
  if (sp.kind < GO1_TUNNEL_SINGLE_PATH || sp.kind > GO1_TUNNEL_RANDOM_PYRAMID)
    return go1_internal_fail(GO1_E_ARG, w + "unknown kind " + std::to_string(sp.kind));
  if (sp.kind == GO1_TUNNEL_RANDOM_PYRAMID) {
    const go1_pyramid_params* layers[2] = {&sp.top, &sp.bottom};
    for (int i = 0; i < 2; ++i) {
      const go1_pyramid_params& c = *layers[i];
      const std::string name = i == 0 ? "top" : "bottom";
      // d_num reaches 2 (difficulty < 0.25): num + 2 - d_num must stay positive
      if (c.num_x < 1 || c.num_y < 1)
        return go1_internal_fail(GO1_E_ARG, w + name + " pyramid_num_x / pyramid_num_y must be >= 1 (pyramid_num + 2 - "
                                            "d_num is not positive at d_num = 2)");
      if ((int64_t)(c.num_x + 2) * (c.num_y + 2) > GO1_TUNNEL_MAX_WEDGES)
        return go1_internal_fail(GO1_E_ARG, w + name + " layer has " + std::to_string((int64_t)(c.num_x + 2) * (c.num_y + 2)) +
                                            " pyramids, more than GO1_TUNNEL_MAX_WEDGES = " +
                                            std::to_string(GO1_TUNNEL_MAX_WEDGES));
    }
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tunnel_draw_kernel, dim3(1), dim3(64), 0, s, sp, stride, records);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(tunnel_tile_kernel, dim3(p->num_rows * p->num_cols), dim3(256), 0, s, sp, stride, records, extents,
                       tiles);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return go1_internal_fail(GO1_E_HIP, w + hipGetErrorString(e));
  return 0;
}

}  // namespace

// single_path with the record size of its own (GO1_TUNNEL_REC): the layout and meaning it always had
extern "C" int go1_tunnel_tiles(const go1_tunnel_params* p, const int32_t* extents, double* records, float* tiles,
                                void* stream) {
  if (!p) return go1_internal_fail(GO1_E_ARG, "go1_tunnel_tiles: null argument");
  go1_tunnel_spec sp = {};
  sp.base = *p;
  sp.kind = GO1_TUNNEL_SINGLE_PATH;
  return tunnel_launch("go1_tunnel_tiles", sp, GO1_TUNNEL_REC, extents, records, tiles, stream);
}

extern "C" int go1_tunnel_generate(const go1_tunnel_spec* spec, const int32_t* extents, double* records, float* tiles,
                                   void* stream) {
  if (!spec) return go1_internal_fail(GO1_E_ARG, "go1_tunnel_generate: null argument");
  return tunnel_launch("go1_tunnel_generate", *spec, GO1_TUNNEL_SPEC_REC, extents, records, tiles, stream);
}
