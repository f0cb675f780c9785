"""The scenes of the ray caster's tests, as launches (TEST INFRASTRUCTURE ONLY): tests/test_render_ref.py checks that
the checker alone finds at least 90 % of every scene's pixels stable, tests/test_gpu_render.py draws them with the
HIP kernel.  All inputs are float32 arrays, so the checker (f64) and the kernel start from the same numbers."""
import functools
from dataclasses import dataclass, field

import numpy as np

from tests import render_ref as RR

WAYPOINT_RADIUS = 0.04  # render.WAYPOINT_RADIUS


@dataclass
class Launch:
    name: str
    root: np.ndarray                 # (n, 13) f32
    q: np.ndarray                    # (n, 12) f32
    views: list                      # (env, mode, flags, pos, look_at)
    W: int
    H: int
    tiles: np.ndarray = None         # (S, 2, nx, ny) f32
    env_tile: np.ndarray = None
    env_terrain_origin: np.ndarray = None
    hs: float = 0.1
    markers: np.ndarray = None       # (n_views, m, 4) f32
    trajectory: np.ndarray = None    # (n, 6 TL) f32
    curr_pose_index: np.ndarray = None
    extra: dict = field(default_factory=dict)

    def ref_scene(self, v):
        env, _, flags = self.views[v][:3]
        s = dict(root=self.root[env], q=self.q[env], hs=self.hs, ceiling=not (flags & 1), markers=[])
        if self.tiles is not None:
            s["tile"] = self.tiles[self.env_tile[env]]
            s["origin"] = self.env_terrain_origin[env]
        if self.markers is not None:
            s["markers"] += [tuple(float(x) for x in m) for m in self.markers[v]]
        if self.trajectory is not None:
            TL = self.trajectory.shape[1] // 6
            i = int(np.clip(self.curr_pose_index[env, 0], 0, TL - 1))
            s["markers"].append(tuple(float(x) for x in self.trajectory[env, 6 * i:6 * i + 3]) + (WAYPOINT_RADIUS,))
        return s

    def ref(self):
        """The checker's pictures, one per view (RR.render); computed once."""
        if "ref" in self.extra:
            return self.extra["ref"]
        out = self.extra["ref"] = []
        for v, view in enumerate(self.views):
            mode = view[1]
            rec = (mode,) + (tuple(view[3:5]) if mode == 2 else ())
            out.append(RR.render(self.ref_scene(v), rec, self.W, self.H))
        return out


def _root(x, y, z, rpy=(0.0, 0.0, 0.0)):
    r, p, yw = (np.float64(a) / 2 for a in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(yw), np.sin(yw)
    quat = [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
            cr * cp * cy + sr * sp * sy]
    return np.array([x, y, z, *quat, 0, 0, 0, 0, 0, 0], np.float32)


# spread legs: hips abducted outwards (FL, FR, RL, RR), thighs and knees bent differently front and rear
SPREAD = np.array([0.5, 0.9, -1.7, -0.5, 0.7, -1.5, 0.4, 1.1, -1.9, -0.6, 0.8, -1.4], np.float32)
STAND = np.array([0.1, 0.8, -1.5, -0.1, 0.8, -1.5, 0.1, 1.0, -1.5, -0.1, 1.0, -1.5], np.float32)


@functools.lru_cache(None)
def closeups():
    """Scene 1: 17 mode-2 cameras 0.15 .. 0.3 m from each primitive of a spread-leg pose, on the plane.  128 x 96 and
    from above: at the issue's 64 x 48 the checker finds 82 - 94 % of the pixels stable."""
    root = _root(0.3, -0.2, 0.45, (0.15, -0.1, 0.4))[None]
    q = SPREAD[None]
    seg, _, (bc, bR, _) = RR.robot(root[0], q[0])
    views = []
    for k in range(16):
        l = k // 4
        c = seg[k].mean(0)
        sx, sy = (1, 1, -1, -1)[l], (1, -1, 1, -1)[l]
        out = np.array([0.15 * sx, 0.3 * sy, 1.0])  # from above: the floor behind is seen nearly head-on
        if k % 4 == 3:
            out = np.array([-0.35 * sx, 0.45 * sy, 1.0])  # a foot: more from the side, or its calf hides it
        out /= np.linalg.norm(out)
        dist = 0.15 if k % 4 == 3 else 0.15 + 0.01 * k  # the 0.04 m foot spheres from the near end of the range
        views.append((0, 2, 0, tuple(c + dist * out), tuple(c)))
    views.append((0, 2, 0, tuple(bc + bR @ np.array([0.12, 0.06, 0.26])), tuple(bc)))
    return Launch("closeups", root, q, views, 128, 96, hs=0.25)


@functools.lru_cache(None)
def rough_tile():
    """The synthetic rough 8 x 6 tile of scenes 3 and 5: (1, 2, 8, 6), 0.25 m cells, floor 0 .. 0.15 m, ceiling
    0.75 .. 0.9 m."""
    rng = np.random.default_rng(5)
    t = np.zeros((1, 2, 8, 6), np.float32)
    t[0, 1] = rng.uniform(0.0, 0.15, (8, 6))
    t[0, 0] = rng.uniform(0.75, 0.9, (8, 6))
    return t


ROUGH_ORIGIN = np.array([[1.0, -0.5, 0.0]], np.float32)
ROUGH_HS = 0.25


@functools.lru_cache(None)
def rough():
    """Scene 3: the rough tile at 192 x 128 (the views along the floor need it for 90 % stable pixels) from the awkward
    places: straight down (the +x up rule), exactly along +x
    and along -y from grid-aligned positions, from outside the grid, from between floor and ceiling, from under the
    floor."""
    ox, oy, hs = float(ROUGH_ORIGIN[0, 0]), float(ROUGH_ORIGIN[0, 1]), ROUGH_HS
    cx, cy = ox + 3.5 * hs, oy + 2.5 * hs
    root = _root(cx + 0.3, cy - 0.1, 0.42, (0.0, 0.1, -0.3))[None]
    views = [
        (0, 2, 0, (cx, cy, 0.7), (cx, cy, 0.0)),                                     # straight down
        (0, 2, 0, (ox + 1 * hs, oy + 2 * hs, 0.4), (ox + 2 * hs, oy + 2 * hs, 0.4)),   # along +x on a grid line
        (0, 2, 0, (ox + 3 * hs, oy + 4 * hs, 0.45), (ox + 3 * hs, oy + 3 * hs, 0.45)),  # along -y on a grid line
        (0, 2, 0, (ox - 1.0, oy - 0.7, 0.6), (cx, cy, 0.3)),                         # from outside the grid
        (0, 2, 0, (ox + 0.33, oy + 0.21, 0.5), (cx + 0.4, cy + 0.3, 0.2)),           # between floor and ceiling
        (0, 2, 0, (cx + 0.1, cy + 0.05, -0.5), (cx + 0.5, cy + 0.3, 0.5)),           # under the floor
    ]
    return Launch("rough", root, STAND[None].copy(), views, 192, 128, tiles=rough_tile(),
                  env_tile=np.zeros(1, np.int32), env_terrain_origin=ROUGH_ORIGIN, hs=hs)


@functools.lru_cache(None)
def plane():
    """Scene 4: the plane (tiles NULL) from straight above and obliquely, with a marker (the open plane seen from the
    follow or the look_from_back camera reaches the horizon: under 60 % stable pixels at any size worth testing)."""
    root = _root(2.0, 3.0, 0.33, (0.05, 0.1, 0.8))[None]
    views = [(0, 2, 0, (2.0, 3.0, 1.2), (2.0, 3.0, 0.0)), (0, 2, 0, (2.2, 2.8, 1.1), (2.0, 3.0, 0.2))]
    markers = np.array([[[2.3, 3.2, 0.3, 0.06]], [[2.4, 2.9, 0.2, 0.05]]], np.float32)
    return Launch("plane", root, STAND[None].copy(), views, 128, 96, hs=0.25, markers=markers)


@functools.lru_cache(None)
def three_views():
    """Scene 5: three views of three envs in one launch at 150 x 111 (neither a multiple of 16: partial last tiles;
    three times the issue's 50 x 37 for 90 % stable pixels), on the rough tile."""
    ox, oy, hs = float(ROUGH_ORIGIN[0, 0]), float(ROUGH_ORIGIN[0, 1]), ROUGH_HS
    root = np.stack([_root(ox + 0.9, oy + 0.6, 0.40, (0, 0, 0.2)), _root(ox + 1.1, oy + 0.7, 0.45, (0.2, 0, -0.5)),
                     _root(ox + 1.2, oy + 0.5, 0.38, (0, -0.2, 1.0))])
    q = np.stack([STAND, SPREAD, STAND * np.float32(0.8)])
    views = [(0, 2, 0, (ox + 0.8, oy + 0.5, 0.72), (ox + 0.95, oy + 0.62, 0.1)), (1, 1, 1),
             (2, 2, 1, (ox + 1.0, oy + 0.3, 1.0), (ox + 1.2, oy + 0.5, 0.3))]
    return Launch("three_views", root, q, views, 150, 111, tiles=rough_tile(), env_tile=np.zeros(3, np.int32),
                  env_terrain_origin=np.repeat(ROUGH_ORIGIN, 3, 0), hs=hs)


# Scene 2's views (env, mode, flags): both modes, the ceiling on and off, every env.  At the issue's 96 x 64 the
# checker finds 62 - 78 % of these pictures stable (along a floor seen at a grazing angle a 0.05 px shift moves the
# depth by more than 1e-3 and crosses the 0.05 m mesh lines), so the resolution is raised until 90 % are: 192 x 128,
# and 288 x 192 for the look_from_back view down the tunnel with the ceiling on.  The checker's cost grows with the
# pixels, hence one view per (mode, ceiling) pair and not all sixteen.  Env 0's look_from_back camera starts inside the
# tile-edge wall.
TUNNEL_VIEWS = ((0, 0, 0), (2, 0, 1), (1, 1, 0), (3, 1, 1))
TUNNEL_VIEWS_FINE = ((2, 0, 0),)
TUNNEL_FINE_SIZE = (288, 192)


def tunnel(root, q, td, hs, trajectory, curr_pose_index, views=TUNNEL_VIEWS, size=(192, 128)):
    """Scene 2: modes 0 and 1, ceiling on and off, of the 4 envs of a 2 x 2 single_path grid (TUNNEL_VIEWS), with the
    current waypoint and one more marker in front of each robot.  root / q: the state after 5 steps of N(0, 1)
    actions (the CPU test steps the oracle backend, the GPU test the HIP env)."""
    n = root.shape[0]
    views = list(views)
    markers = np.array([[[root[e, 0] + 0.35, root[e, 1] + 0.1, 0.3, 0.08]] for e, _, _ in views], np.float32)
    return Launch("tunnel", np.asarray(root, np.float32), np.asarray(q, np.float32), views, size[0], size[1],
                  tiles=np.asarray(td.tiles, np.float32), env_tile=np.asarray(td.env_tile[:n], np.int32),
                  env_terrain_origin=np.asarray(td.env_terrain_origin[:n], np.float32), hs=float(hs), markers=markers,
                  trajectory=np.asarray(trajectory, np.float32), curr_pose_index=np.asarray(curr_pose_index, np.int32))


def tunnel_cfg(n_envs=4):
    """The HIP step takes multiples of 16 envs: the GPU test builds 16 and draws the first 4, one per tile."""
    from legged_tracking_amd import config as CF
    return CF.readme_config(n_envs=n_envs, terrain="single_path", rows=2, cols=2)


def tunnel_actions(n_envs=4):
    return np.random.default_rng(17).normal(0, 1, (5, 16, 12)).astype(np.float32)[:, :n_envs]


STATIC = (closeups, rough, plane, three_views)
