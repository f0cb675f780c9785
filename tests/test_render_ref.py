"""The ray caster's checker (tests/render_ref.py) against closed forms, and the condition on the GPU tests' inputs:
every scene they draw has at least 90 % stable pixels in the checker alone."""
import numpy as np
import pytest
import torch

from tests import render_ref as RR, render_scenes as RS

O3 = np.zeros(3)


def one(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d))[None]


def test_sphere_seen_centrally_has_depth_d_minus_r():
    t, s = RR.sphere_hit(O3, one([1, 0, 0]), np.array([2.0, 0, 0]), 0.25)
    assert t[0] == pytest.approx(1.75, abs=1e-12) and s[0] == pytest.approx(1.0)
    # from inside: the far side (two-sided); off-centre: the chord
    t, _ = RR.sphere_hit(np.array([2.0, 0, 0]), one([0, 1, 0]), np.array([2.0, 0, 0]), 0.25)
    assert t[0] == pytest.approx(0.25)
    t, s = RR.sphere_hit(O3, one([1, 0, 0]), np.array([2.0, 0.15, 0]), 0.25)
    assert t[0] == pytest.approx(2 - 0.2) and s[0] == pytest.approx(0.8)
    assert np.isinf(RR.sphere_hit(O3, one([1, 0, 0]), np.array([2.0, 0.3, 0]), 0.25)[0][0])
    assert np.isinf(RR.sphere_hit(O3, one([-1, 0, 0]), np.array([2.0, 0, 0]), 0.25)[0][0])


def test_capsule_side_on_and_end_on():
    a, b, r = np.array([2.0, -0.5, 0]), np.array([2.0, 0.5, 0]), 0.1
    t, s = RR.capsule_hit(O3, one([1, 0, 0]), a, b, r)                   # side-on: the cylinder
    assert t[0] == pytest.approx(1.9) and s[0] == pytest.approx(1.0)
    t, _ = RR.capsule_hit(np.array([0, 0.55, 0.0]), one([1, 0, 0]), a, b, r)   # past the end plane: the cap
    assert t[0] == pytest.approx(2 - np.sqrt(0.1 ** 2 - 0.05 ** 2))
    t, s = RR.capsule_hit(np.array([2.0, -3.0, 0]), one([0, 1, 0]), a, b, r)   # end-on, along the axis
    assert t[0] == pytest.approx(3 - 0.5 - 0.1) and s[0] == pytest.approx(1.0)
    t, _ = RR.capsule_hit(np.array([2.0, 0.2, 0]), one([0, 1, 0]), a, b, r)    # from inside along the axis
    assert t[0] == pytest.approx(0.4)
    assert np.isinf(RR.capsule_hit(np.array([0, 0.7, 0.0]), one([1, 0, 0]), a, b, r)[0][0])
    # random rays: every hit lies on the capsule's surface (distance to the segment = r)
    rng = np.random.default_rng(0)
    d = rng.normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.array([1.7, 0.1, 0.2])
    t, s = RR.capsule_hit(o, d, a, b, r)
    hit = np.isfinite(t)
    assert 50 < hit.sum() < 3900
    dist, _ = RR.seg_point_dist(o + t[hit, None] * d[hit], a, b)
    np.testing.assert_allclose(dist, r, atol=1e-10)
    # and no ray that misses passes within r of the segment (sampled along the ray)
    ts = np.linspace(0, 3, 601)
    P = o + ts[None, :, None] * d[~hit][:60, None, :]
    assert RR.seg_point_dist(P.reshape(-1, 3), a, b)[0].min() > r - 1e-3


def test_box_face_and_edge():
    c, R, h = np.array([2.0, 0, 0]), np.eye(3), np.array([0.5, 0.25, 0.1])
    t, s = RR.box_hit(O3, one([1, 0, 0]), c, R, h)
    assert t[0] == pytest.approx(1.5) and s[0] == pytest.approx(1.0)
    # towards the edge x = 1.5, y = 0.25 from 45 degrees: both slabs enter at the same t
    o = np.array([1.5 - 1.0, 0.25 + 1.0, 0.0])
    t, s = RR.box_hit(o, one([1, -1, 0]), c, R, h)
    assert t[0] == pytest.approx(np.sqrt(2)) and s[0] == pytest.approx(np.sqrt(0.5))
    # rotated 90 degrees about z: the 0.25 half extent faces the ray
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    assert RR.box_hit(O3, one([1, 0, 0]), c, Rz, h)[0][0] == pytest.approx(1.75)
    assert RR.box_hit(c, one([0, 0, 1]), c, R, h)[0][0] == pytest.approx(0.1)         # from inside
    assert np.isinf(RR.box_hit(O3, one([1, 0.3, 0]), c, R, h)[0][0])


def plane_scene(**kw):
    return dict(root=np.array([50.0, 50, 0.4, 0, 0, 0, 1] + [0] * 6), q=np.zeros(12), hs=0.1, **kw)


def test_plane_straight_down_and_at_45_degrees():
    s = plane_scene()
    t, p, c = RR.trace(s, np.array([0.33, 0.27, 1.5]), np.concatenate([one([0, 0, -1]), one([1, 0, -1])]))
    assert t[0] == pytest.approx(1.5) and t[1] == pytest.approx(1.5 * np.sqrt(2))
    assert list(p) == [RR.PRIM_FLOOR, RR.PRIM_FLOOR]
    np.testing.assert_allclose(c[0], RR.COLOURS[5])                                    # |n . d| = 1, off the lines
    np.testing.assert_allclose(c[1], RR.COLOURS[5] * (0.25 + 0.75 * np.sqrt(0.5)))     # lands at x = 1.83
    # on a grid line (frac(u) < 0.04): darkened
    _, _, c = RR.trace(s, np.array([0.302, 0.27, 1.5]), one([0, 0, -1]))
    np.testing.assert_allclose(c[0], RR.COLOURS[5] * 0.8)
    # looking up: background
    t, p, c = RR.trace(s, np.array([0.33, 0.27, 1.5]), one([0, 0.2, 1]))
    assert np.isinf(t[0]) and p[0] == RR.PRIM_BACKGROUND and list(c[0]) == list(RR.COLOURS[8])


def tile44():
    t = np.zeros((2, 4, 4), np.float32)
    t[0] = 2.0
    t[1, 1, 2] = 0.5   # one raised floor vertex at (1, 2)
    return t


def tile_scene(**kw):
    return dict(root=np.array([50.0, 50, 0.4, 0, 0, 0, 1] + [0] * 6), q=np.zeros(12), hs=1.0, tile=tile44(),
                origin=(10.0, 20.0), **kw)


def test_one_raised_vertex_of_a_4x4_tile():
    s = tile_scene()
    down = one([0, 0, -1])

    def depth(x, y, z=1.5):
        return RR.trace(s, np.array([10.0 + x, 20.0 + y, z]), down)[0][0]
    assert depth(1.0, 2.0) == pytest.approx(1.0, abs=1e-9)        # the apex
    assert depth(2.5, 0.5) == pytest.approx(1.5)                  # flat
    # the six triangles around the vertex, by the (i, j) - (i + 1, j + 1) split: height 0.5 x the vertex's weight
    assert depth(1.5, 2.0) == pytest.approx(1.5 - 0.25)           # edge to (2, 2)
    assert depth(1.5, 2.5) == pytest.approx(1.5 - 0.25)           # the diagonal (1, 2) - (2, 3) carries the vertex
    assert depth(0.5, 2.5) == pytest.approx(1.5)                  # the other diagonal direction does not
    assert depth(1.25, 2.5) == pytest.approx(1.5 - 0.25)          # upper triangle of cell (1, 2): h = 0.5 (1 - (b - a)) ..
    assert depth(0.75, 1.5) == pytest.approx(1.5 - 0.25)          # cell (0, 1), lower triangle: weight a - (a - b) ...
    # the ceiling from below, and with the ceiling dropped
    t, p, _ = RR.trace(s, np.array([12.5, 20.5, 1.5]), one([0, 0, 1]))
    assert t[0] == pytest.approx(0.5) and p[0] == RR.PRIM_CEILING
    t, p, _ = RR.trace(dict(s, ceiling=False), np.array([12.5, 20.5, 1.5]), one([0, 0, 1]))
    assert np.isinf(t[0]) and p[0] == RR.PRIM_BACKGROUND


def test_ray_from_outside_the_grid_and_from_under_the_floor():
    s = tile_scene(ceiling=False)
    # from outside, level with the raised vertex's flank: enters at x = 10 and hits the slope before (1, 2)
    o = np.array([8.0, 22.0, 0.25])
    t, p, _ = RR.trace(s, o, one([1, 0, 0]))
    assert p[0] == RR.PRIM_FLOOR and t[0] == pytest.approx(2.5)     # height 0.25 on the edge (0, 2) - (1, 2) at a = 0.5
    # outside the vertex grid there is no geometry: a ray that passes beside the tile sees nothing
    t, p, _ = RR.trace(s, np.array([8.0, 19.5, 0.25]), one([1, 0, -0.01]))
    assert np.isinf(t[0]) and p[0] == RR.PRIM_BACKGROUND
    # a ray that comes down outside and would meet z = 0 outside the grid: nothing either
    t, p, _ = RR.trace(s, np.array([8.0, 21.0, 0.5]), one([1, 0, -1]))
    assert np.isinf(t[0])
    # from under the floor looking up: the floor's underside (two-sided)
    t, p, _ = RR.trace(s, np.array([12.5, 20.5, -1.0]), one([0, 0, 1]))
    assert t[0] == pytest.approx(1.0) and p[0] == RR.PRIM_FLOOR
    # and obliquely from under the floor through the raised vertex's pyramid
    t, p, _ = RR.trace(s, np.array([11.0, 22.0, -1.0]), one([0, 0, 1]))
    assert t[0] == pytest.approx(1.5)


def test_terrain_march_equals_brute_force_over_all_triangles():
    """The march visits a subset of the cells; testing every cell of the tile must give the same first hit."""
    L = RS.rough()
    for v in (0, 3, 4, 5):
        sc = L.ref_scene(v)
        cam = RR.camera(2, None, *L.views[v][3:5])
        d = RR.rays(cam, 24, 16)
        t, _, l = RR.terrain_hit(cam[0], d, sc["tile"], *sc["origin"][:2], sc["hs"])
        nx, ny = sc["tile"].shape[1:]
        bt, bl = np.full(d.shape[0], np.inf), np.full(d.shape[0], -1)
        for i in range(nx - 1):
            for j in range(ny - 1):
                tt, _, ll = RR._cells(cam[0], d, sc["tile"], float(sc["origin"][0]), float(sc["origin"][1]), sc["hs"],
                                      np.full(d.shape[0], i), np.full(d.shape[0], j), (1, 0))
                c = tt < bt
                bt, bl = np.where(c, tt, bt), np.where(c, ll, bl)
        np.testing.assert_allclose(t, bt, rtol=0, atol=1e-12)
        assert (l == bl).all()


def test_camera_basis_and_pixel_rays():
    pos, f, right, up = RR.camera(2, None, (0, 0, 2.0), (0, 0, 0.0))          # straight down: up is +x
    np.testing.assert_allclose(f, [0, 0, -1])
    np.testing.assert_allclose(right, np.cross([0, 0, -1.0], [1.0, 0, 0]))
    np.testing.assert_allclose(up, [1, 0, 0], atol=1e-15)
    cam = RR.camera(0, np.array([1.0, 2.0, 0.3]))
    np.testing.assert_allclose(cam[0], [1 - 0.495, 2, 0.35])
    d = RR.rays(cam, 4, 2).reshape(2, 4, 3)
    # 90 degrees horizontally: the outermost pixel centres are at tan = 3 / 4; row 0 looks up
    assert (d[0, 3] @ cam[2]) / (d[0, 3] @ cam[1]) == pytest.approx(0.75)
    assert (d[0, 0] @ cam[3]) / (d[0, 0] @ cam[1]) == pytest.approx(0.25)
    assert d[0, 0] @ cam[3] > 0 > d[1, 0] @ cam[3]
    cam = RR.camera(1, np.array([1.0, 2.0, 0.3]))
    np.testing.assert_allclose(cam[0], [1, 1, 1.3])


def test_robot_primitives_are_self_geoms_under_the_root_transform():
    L = RS.closeups()
    seg, r, (c, R, h) = RR.robot(L.root[0], L.q[0])
    from tests import self_geom as SG
    P, rr = SG.capsules(L.q[:1].astype(np.float64))
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-6)
    np.testing.assert_allclose((seg - c) @ R, P[0], atol=1e-12)
    assert (r == rr).all() and (seg[3, 0] == seg[3, 1]).all()


# ------------------------------------------------------------------ the condition on the GPU tests' inputs
def stable_share(launch):
    return [float(r["stable"].mean()) for r in launch.ref()]


@pytest.mark.parametrize("scene", RS.STATIC, ids=lambda f: f.__name__)
def test_static_scenes_are_at_least_90_percent_stable(scene):
    L = scene()
    share = stable_share(L)
    print(L.name, [round(s, 3) for s in share])
    assert min(share) >= 0.90, share
    if L.name == "closeups":   # every primitive fills many pixels of its own close-up
        for k, r in enumerate(L.ref()):
            # the thinnest is a calf: 0.016 m wide at <= 0.3 m is >= 3.4 px of the 64 px per radian, 1.4 px without
            # its 1 px silhouette edges, over 0.213 m (>= 45 px; foreshortened to half at worst): >= 30 px
            assert ((r["prim"] == k) & r["stable"]).sum() >= 30, k
        kinds = {int(p) for r in L.ref() for p in np.unique(r["prim"])}
        assert set(range(17)) <= kinds and RR.PRIM_FLOOR in kinds


def oracle_tunnel(**kw):
    from legged_tracking_amd import env as E
    from tests.cpu_backend import OracleBackend
    env = E.TrajectoryTrackingEnv(sim_device="cpu", headless=True, cfg=RS.tunnel_cfg(), seed=1, backend=OracleBackend)
    for a in RS.tunnel_actions():
        env.step(torch.from_numpy(a))
    st = env._sim.state
    return RS.tunnel(st["root"].numpy(), st["dof_pos"].numpy(), env.terrain, env.cfg.terrain.horizontal_scale,
                     st["trajectory"].numpy(), st["curr_pose_index"].numpy(), **kw)


def test_tunnel_scene_is_at_least_90_percent_stable():
    L = oracle_tunnel()
    fine = oracle_tunnel(views=RS.TUNNEL_VIEWS_FINE, size=RS.TUNNEL_FINE_SIZE)
    share = stable_share(L) + stable_share(fine)
    print([round(s, 3) for s in share])
    assert min(share) >= 0.90, share
    prims = np.concatenate([r["prim"].ravel() for r in L.ref() + fine.ref()])
    for p in (RR.PRIM_FLOOR, RR.PRIM_CEILING, RR.PRIM_MARKER, RR.PRIM_TRUNK):
        assert (prims == p).sum() > 50, p
