/*
 * go1_render.h -- C ABI of the MI355X ray caster that draws the collision scene of the Go1 envs: the video
 * recording surface of go1_gym/envs/base/legged_robot_trajectory_tracking.py (bare :N below)
 *
 *   go1_render()         <- render :1690-1699, render_all_envs :1701-1711 (one launch, any number of views)
 *   go1_render_record()  <- _render_headless :1720-1744 with the frame lists of reset_idx :1054-1062
 *
 * The picture is NOT Isaac Gym's rasterised visual meshes.  It shows exactly what the contact code collides
 * with: per env the 16 leg primitives (4 leg + k: k = 0 thigh capsule, 1 hip capsule, 2 calf capsule, 3 foot
 * sphere) and the trunk box, posed from the live `root` / `dof_pos` planes, and the env's terrain tile as two
 * triangle meshes (vertex (i, j) at (ox + i hs, oy + j hs, tile[layer, i, j]), every cell split along
 * (i, j) - (i + 1, j + 1); layer 1 floor, layer 0 ceiling; no geometry outside the vertex grid; tiles == NULL:
 * the plane z = 0 as the floor, no ceiling).
 *
 * Conventions as go1_mi355x.h: caller-owned device buffers, asynchronous on the caller's stream, no
 * allocation, 0 or -1 with go1_render_last_error(), one host thread per call site.
 *
 * Camera: pinhole, horizontal field of view 90 degrees, square pixels, a ray through the pixel centre
 * (col + 0.5, row + 0.5), row 0 at the top.  f = normalize(look_at - pos), right = normalize(f x up),
 * up' = right x f, up = +z (or +x when |f.x| and |f.y| are both below 1e-6);
 *   dir = normalize(f + sx right + sy up'),  sx = 2 (col + 0.5) / W - 1,  sy = (1 - 2 (row + 0.5) / H) H / W.
 * pos / look_at are formed on the device from the view's env root (x, y, z):
 *   mode 0 look_from_back  pos = (x - 0.495, y, 0.35), look_at = (x, y, 0.25)     (:1726-1737)
 *   mode 1 follow          pos = (x, y - 1, z + 1),    look_at = (x, y, z)        (:1692-1694, :1739-1740)
 *   mode 2 explicit        pos, look_at of the view record
 *
 * Every ray finds its first hit (ray parameter t > 0 along the unit direction); surfaces are two-sided.
 * Shading (fixed here so that a checker can restate it): colour = base[class] (0.25 + 0.75 |n . dir|), n the
 * unit normal at the hit; terrain hits are darkened by 0.8 where frac(u) < 0.04 or frac(v) < 0.04
 * (u, v = (x - ox) / hs, (y - oy) / hs; ox = oy = 0 for the plane); channel = floor(value + 0.5), alpha 255.
 * The background has no shading.  A view whose camera, root or joint angles are not finite is all background.
 */
#ifndef GO1_RENDER_H
#define GO1_RENDER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1_RENDER_ABI_VERSION 1

/* prim_id output */
#define GO1_PRIM_TRUNK 16
#define GO1_PRIM_FLOOR 17
#define GO1_PRIM_CEILING 18
#define GO1_PRIM_MARKER 19
#define GO1_PRIM_BACKGROUND (-1)

/* colour classes and their base colours (r, g, b) */
enum go1_render_class {
  GO1_RC_TRUNK = 0, GO1_RC_HIP, GO1_RC_THIGH, GO1_RC_CALF, GO1_RC_FOOT, GO1_RC_FLOOR, GO1_RC_CEILING,
  GO1_RC_MARKER, GO1_RC_BACKGROUND, GO1_RC_COUNT
};
#define GO1_RENDER_COLOURS                                                                                   \
  {{200, 60, 60}, {240, 160, 40}, {60, 160, 220}, {80, 200, 120}, {240, 240, 80}, {170, 170, 170},          \
   {110, 110, 140}, {230, 50, 230}, {135, 180, 235}}
#define GO1_RENDER_AMBIENT 0.25f
#define GO1_RENDER_DIFFUSE 0.75f
#define GO1_RENDER_GRID_FRAC 0.04f
#define GO1_RENDER_GRID_DARK 0.8f

#define GO1_RENDER_MAX_MARKERS 8
#define GO1_VIEW_NO_CEILING 1 /* go1_render_view.flags: leave the ceiling mesh out (mode 1 sits above the tunnel) */

/* recording state (go1_render_record) */
enum go1_record_state { GO1_REC_IDLE = 0, GO1_REC_ARMED, GO1_REC_RECORDING, GO1_REC_COMPLETE };

/* The robot's geometry, filled by the binding from model.py (legs FL, FR, RL, RR; trunk frame) */
typedef struct go1_render_model {
  float hip_origin[4][3];    /* hip joint in the trunk frame */
  float thigh_origin[4][3];  /* thigh joint in the hip frame */
  float calf_origin[3];      /* knee in the thigh frame */
  float foot_offset[3];      /* foot centre in the calf frame */
  float hip_capsule_y[4][2]; /* hip capsule segment ends along the hip frame's y (signed per leg) */
  float thigh_radius, hip_radius, calf_radius, foot_radius;
  float trunk_half[3];       /* half extents of the trunk box */
  float bound_radius;        /* every primitive lies within this distance of the root position */
} go1_render_model;

typedef struct go1_render_view {
  int32_t env;      /* local env id */
  int32_t mode;     /* 0 look_from_back, 1 follow, 2 explicit */
  int32_t flags;    /* GO1_VIEW_* */
  int32_t pad;
  float pos[3];     /* mode 2 */
  float look_at[3]; /* mode 2 */
} go1_render_view;

typedef struct go1_render_args {
  go1_render_model model;
  const float* root;               /* (n_envs, 13) state plane */
  const float* dof_pos;            /* (n_envs, 12) state plane */
  const float* tiles;              /* (n_tiles, 2, hf_nx, hf_ny) or NULL: the plane */
  const int32_t* env_tile;         /* (n_envs) */
  const float* env_terrain_origin; /* (n_envs, 3) */
  const float* markers;            /* (n_views, n_markers, 4) centre and radius, or NULL */
  const float* wp_trajectory;      /* (n_envs, 6 wp_length) state plane or NULL: with wp_index, the env's current */
  const int32_t* wp_index;         /* (n_envs) waypoint is one more marker sphere of radius wp_radius */
  const go1_render_view* views;    /* (n_views), device memory */
  uint8_t* rgba;                   /* (n_views, height, width, 4) */
  float* depth;                    /* (n_views, height, width) ray parameter of the first hit, +inf: none; or NULL */
  int32_t* prim_id;                /* (n_views, height, width) or NULL */
  int32_t n_envs, n_tiles, hf_nx, hf_ny;
  int32_t n_markers, wp_length, n_views, width, height;
  float horizontal_scale, wp_radius;
  int32_t pad;
} go1_render_args;

/* go1_render_record renders view 0 of `r` into slot `count` of the frame ring r.rgba (capacity, height, width, 4)
 * (r.depth / r.prim_id must be NULL) and advances the state record: int32 state[2][4], copy c = {state, count, 0, 0}.
 * The launch of step s reads copy s & 1 and one lane writes copy (s + 1) & 1, so every workgroup sees the same
 * state; the caller passes consecutive `step` values and sets BOTH copies when it arms or stops a recording.
 * With reset = reset[view 0's env] of this step (:1054-1062, :1721):
 *   ARMED + reset      -> RECORDING, count 0, and this step's frame (the reset pose) is frame 0
 *   RECORDING + reset  -> COMPLETE, no frame this step
 *   RECORDING          -> the frame goes to slot count, count + 1; count == capacity -> COMPLETE
 *   IDLE, COMPLETE     -> nothing is drawn */
typedef struct go1_record_args {
  go1_render_args r;
  const uint8_t* reset; /* (n_envs) this step's reset output */
  int32_t* state;       /* (2, 4) */
  int32_t capacity;
  int32_t pad;
  uint64_t step;
} go1_record_args;

int go1_render_abi_version(void);
/* sizeof go1_render_model, go1_render_view, go1_render_args, go1_record_args */
void go1_render_abi_sizes(int64_t out[4]);
const char* go1_render_last_error(void);
int go1_render(const go1_render_args* args, void* stream);
int go1_render_record(const go1_record_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GO1_RENDER_H */
