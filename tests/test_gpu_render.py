"""The HIP ray caster (csrc/go1_render.hip) against the f64 checker (tests/render_ref.py) on the scenes of
tests/render_scenes.py.  On the checker's stable pixels the prim id is equal without exception, the colour is within
2 LSB per channel and the depth within DEPTH_TOL.

DEPTH_TOL: the largest |t_gpu - t_ref| / (1 + t_ref) over the stable pixels of all scenes measured on the MI355X is
MEASURED_DEPTH_ERR; the bound is 4 x that, rounded up to one significant digit, and never above 1e-3 (the stability
criterion's own scale, above which a hit on the wrong surface could pass)."""
import numpy as np
import pytest
import torch

from tests import render_ref as RR, render_scenes as RS

pytestmark = pytest.mark.gpu

MEASURED_DEPTH_ERR = 1.154e-6   # the look_from_back view down the tunnel (288 x 192); the other scenes: <= 7.0e-7
DEPTH_TOL = 5e-6
assert DEPTH_TOL <= 1e-3


def draw(L, scene=None):
    """One go1_render launch of a Launch: rgba, depth, prim_id as numpy."""
    from legged_tracking_amd import render as R
    dev = torch.device("cuda:0")
    if scene is None:
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        scene = R.Scene(t(L.root), t(L.q), tiles=t(L.tiles), env_tile=t(L.env_tile),
                        env_terrain_origin=t(L.env_terrain_origin), horizontal_scale=L.hs, trajectory=t(L.trajectory),
                        curr_pose_index=t(L.curr_pose_index))
    views = R.views_tensor(L.views, dev)
    markers = None if L.markers is None else torch.from_numpy(L.markers).to(dev)
    out = R.render_views(scene, views, L.W, L.H, markers=markers, depth=True, prim_id=True)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def check(L, out):
    """The pass criteria on every view; returns the largest relative depth error seen."""
    rgba, depth, prim = out
    assert rgba.shape == (len(L.views), L.H, L.W, 4) and rgba.dtype == np.uint8 and (rgba[..., 3] == 255).all()
    worst = 0.0
    for v, ref in enumerate(L.ref()):
        st = ref["stable"]
        assert st.mean() >= 0.90, (L.name, v, st.mean())
        bad = st & (prim[v] != ref["prim"])
        assert not bad.any(), (L.name, v, int(bad.sum()), np.argwhere(bad)[:5], prim[v][bad][:5], ref["prim"][bad][:5])
        dc = np.abs(rgba[v, ..., :3].astype(np.int64) - ref["rgb"])[st]
        hit = st & np.isfinite(ref["depth"])
        assert np.isinf(depth[v][st & ~np.isfinite(ref["depth"])]).all()
        err = np.abs(depth[v][hit].astype(np.float64) - ref["depth"][hit]) / (1 + ref["depth"][hit])
        e = float(err.max()) if err.size else 0.0
        print(f"{L.name} view {v}: stable {st.mean():.3f} colour max {int(dc.max())} depth err {e:.3e}")
        worst = max(worst, e)
        assert dc.max() <= 2, (L.name, v, int(dc.max()))
        assert e <= DEPTH_TOL, (L.name, v, e)
    return worst


@pytest.mark.parametrize("scene", RS.STATIC, ids=lambda f: f.__name__)
def test_static_scene_matches_the_checker(scene):
    L = scene()
    check(L, draw(L))


@pytest.fixture(scope="module")
def tunnel():
    """Scene 2 on the HIP env: a 2 x 2 single_path grid after 5 steps of N(0, 1) actions (16 envs, the step kernel's
    multiple; the first 4, one per tile, are drawn), through the env's own Renderer scene (its terrain and waypoint
    planes); [(launch, its pictures)] for the 192 x 128 and the 288 x 192 launch."""
    from legged_tracking_amd import env as E, render as R
    env = E.TrajectoryTrackingEnv(sim_device="cuda:0", headless=True, cfg=RS.tunnel_cfg(16), seed=1)
    for a in RS.tunnel_actions(16):
        env.step(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    st = env._sim.state
    tiles, env_tile, eto = (x.cpu().numpy() for x in env._sim._terrain_keep[:3])

    class TD:
        pass
    TD.tiles, TD.env_tile, TD.env_terrain_origin = tiles, env_tile, eto
    args = (st["root"].cpu().numpy(), st["dof_pos"].cpu().numpy(), TD, env.cfg.terrain.horizontal_scale,
            st["trajectory"].cpu().numpy(), st["curr_pose_index"].cpu().numpy())
    scene = R.Renderer(env).scene()
    pair = [RS.tunnel(*args), RS.tunnel(*args, views=RS.TUNNEL_VIEWS_FINE, size=RS.TUNNEL_FINE_SIZE)]
    res = [(L, draw(L, scene)) for L in pair]
    env.close()
    return res


def test_tunnel_scene_matches_the_checker(tunnel):
    prims = set()
    for L, out in tunnel:
        check(L, out)
        prims |= {int(p) for p in np.unique(out[2])}
    assert {RR.PRIM_FLOOR, RR.PRIM_CEILING, RR.PRIM_MARKER, RR.PRIM_TRUNK, RR.PRIM_BACKGROUND} <= prims


def mesh_height(tile, layer, ox, oy, hs, x, y):
    """tri_locate + tri_query (oracle/go1_oracle.c:400-422) restated: the mesh height under (x, y)."""
    nx, ny = tile.shape[1:]
    u, v = np.clip((x - ox) / hs, -4.0, nx + 4.0), np.clip((y - oy) / hs, -4.0, ny + 4.0)
    ci, cj = np.floor(u).astype(int), np.floor(v).astype(int)
    up = (u - ci) < (v - cj)
    a, b = u - ci, v - cj
    at = lambda i, j: tile[layer, np.clip(i, 0, nx - 1), np.clip(j, 0, ny - 1)].astype(np.float64)  # noqa: E731
    h00, h10, h01, h11 = at(ci, cj), at(ci + 1, cj), at(ci, cj + 1), at(ci + 1, cj + 1)
    da, db = np.where(up, h11 - h01, h10 - h00), np.where(up, h01 - h00, h11 - h10)
    return h00 + a * da + b * db


def test_terrain_hits_lie_on_the_mesh_the_physics_collides_with(tunnel):
    """Every floor / ceiling hit P = o + t d of scene 2 has the contact model's mesh height at (P.x, P.y) equal to
    P.z within 1e-4 m."""
    n = 0
    for L, (_, depth, prim) in tunnel:
        for v, ref in enumerate(L.ref()):
            env = L.views[v][0]
            tile, (ox, oy) = L.tiles[L.env_tile[env]], L.env_terrain_origin[env][:2]
            for pid, layer in ((RR.PRIM_FLOOR, 1), (RR.PRIM_CEILING, 0)):
                m = prim[v] == pid
                if not m.any():
                    continue
                P = ref["cam"][0] + depth[v][m].astype(np.float64)[:, None] * ref["dirs"][m]
                h = mesh_height(tile, layer, float(ox), float(oy), L.hs, P[:, 0], P[:, 1])
                err = np.abs(h - P[:, 2])
                print(f"tunnel view {v} prim {pid}: {int(m.sum())} hits, max |h - z| {err.max():.2e}")
                assert err.max() <= 1e-4, (v, pid, float(err.max()))
                n += int(m.sum())
    assert n > 10000


def test_same_launch_twice_is_bit_identical():
    L = RS.three_views()
    a, b = draw(L), draw(L)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
