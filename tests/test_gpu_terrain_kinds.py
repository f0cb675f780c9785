"""narrow_path and random_pyramid generated on the GPU (go1_tunnel_generate) and any tile geometry through the
step, the height scan and the renderer.

  * device tiles vs the host restatement terrain.make_tunnel, bit for bit, and vs the reference's own tiles
    (tests/golden/terrain_kinds.npz) directly;
  * go1_tunnel_tiles (the old entry, now a wrapper) still bit-identical;
  * TrajectoryTrackingEnv on each new kind;
  * the height scan at (80, 40) and (160, 72) tiles from the GPU's own post-physics pose, bit-exact: what a
    transposed or mis-strided tile cannot pass;
  * one integrator step against the f64 oracle on (160, 80) tiles;
  * one render() frame on (160, 72) tiles.
"""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from legged_tracking_amd import config as CF, native, terrain as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import terrain_cases as TC  # noqa: E402

DEV = "cuda:0"
N = 64


def _device_tiles(cfg, seed):
    lay = T.tunnel_layout(cfg.terrain)
    return native.tunnel_tiles(cfg.terrain, lay, seed, torch.device(DEV)).cpu().numpy()


def _vs_host(cfg, seed, label):
    t0 = time.perf_counter()
    host, _, _ = T.make_tunnel(cfg.terrain, np.random.RandomState(seed))
    t_host = time.perf_counter() - t0
    _device_tiles(cfg, seed)  # first call loads the library
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = _device_tiles(cfg, seed)
    t_dev = time.perf_counter() - t0
    print(f"\n{label} seed {seed}: host numpy {t_host * 1e3:.1f} ms, GPU {t_dev * 1e3:.2f} ms (incl. D2H)")
    assert dev.shape == host.shape and dev.dtype == np.float32
    np.testing.assert_array_equal(dev.view(np.uint32), host.view(np.uint32))
    return dev


@pytest.mark.parametrize("kind", ["narrow_path", "random_pyramid"])
@pytest.mark.parametrize("rows,cols,seed", [(4, 4, 11), (8, 16, 3)])
def test_device_tiles_bit_exact_vs_host(kind, rows, cols, seed):
    _vs_host(TC.kind_cfg(kind, rows, cols), seed, f"{kind} {rows}x{cols}")


def test_device_pyramid_tiles_bit_exact_vs_host_full_grid():
    """The README grid (32 x 32 sub-terrains, ~70 k pyramids, the MT19937 state re-twisted ~900 times) at the
    largest seed; the printed GPU time is the figure DESIGN and the README quote."""
    _vs_host(TC.kind_cfg("random_pyramid", 32, 32), 4294967295, "random_pyramid 32x32")


def test_device_pyramid_tiles_default_geometry_vs_host():
    dev = _vs_host(TC.kind_cfg("random_pyramid", 4, 4, geometry=TC.DEFAULT_GEOMETRY), 7, "random_pyramid (160, 72)")
    assert dev.shape == (4, 4, 2, 160, 72)


@pytest.mark.parametrize("num", [(1, 1), (6, 6), (6, 1)])
def test_device_pyramid_tiles_at_the_ends_of_pyramid_num(num):
    """(1, 1): 1 / 4 / 9 pyramids a layer (one axis of np.linspace(., ., 1) at d_num = 2); (6, 6): the 64 pyramids
    GO1_TUNNEL_MAX_WEDGES holds."""
    cfg = TC.kind_cfg("random_pyramid", 4, 8, pyramid_num_x=num[0], pyramid_num_y=num[1])
    _vs_host(cfg, 5, f"random_pyramid pyramid_num {num}")


def test_device_pyramid_layers_take_their_own_parameters():
    cfg = TC.kind_cfg("random_pyramid", 4, 4)
    TC.apply_settings(cfg, dict(top=dict(pyramid_num_x=2, pyramid_num_y=4, pyramid_var_x=0.1, pyramid_height_max=0.6),
                                bottom=dict(pyramid_num_x=5, pyramid_num_y=1, pyramid_length_min=0.05,
                                            pyramid_var_y=0.0)))
    _vs_host(cfg, 21, "random_pyramid top != bottom")


@pytest.mark.parametrize("p_flat,p_double", [(0.0, 0.6), (0.9, 0.0), (0.9, 1.0)])
def test_device_narrow_tiles_variants(p_flat, p_double):
    cfg = TC.kind_cfg("narrow_path", 8, 8, geometry=dict(p_flat=p_flat, p_double=p_double))
    _vs_host(cfg, 5, f"narrow_path p_flat {p_flat} p_double {p_double}")


@pytest.mark.parametrize("name", TC.CASES)
def test_device_tiles_match_the_reference(name):
    cfg, seed, ref, _, _ = TC.case(name)
    dev = _device_tiles(cfg, seed)
    np.testing.assert_array_equal(dev.view(np.uint32), ref.view(np.uint32))


def test_old_entry_is_still_bit_identical():
    """go1_tunnel_tiles with its own record size (GO1_TUNNEL_REC), called as a foreign binding would."""
    import ctypes as C
    from legged_tracking_amd import abi
    cfg = CF.readme_config(n_envs=16, terrain="single_path", rows=4, cols=4)
    t, lay = cfg.terrain, T.tunnel_layout(cfg.terrain)
    host, _, _ = T.make_single_path(t, np.random.RandomState(11))
    p = abi.Go1TunnelParams(num_rows=4, num_cols=4, tile_x=lay.tile_x, tile_y=lay.tile_y, sub_x=lay.sub_shape[0],
                            sub_y=lay.sub_shape[1], seed=11, horizontal_scale=t.horizontal_scale,
                            vertical_scale=t.vertical_scale, ceiling_height=t.ceiling_height, p_flat=t.p_flat,
                            p_double=t.p_double)
    ext = torch.as_tensor(np.ascontiguousarray(lay.extents, np.int32)).to(DEV)
    guard = 7.25
    rec = torch.full((16 * abi.GO1_TUNNEL_REC + 64,), guard, dtype=torch.float64, device=DEV)
    tiles = torch.empty((4, 4, 2, lay.tile_x, lay.tile_y), dtype=torch.float32, device=DEV)
    lib = native.lib()
    native.check(lib, lib.go1_tunnel_tiles(C.byref(p), ext.data_ptr(), rec.data_ptr(), tiles.data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tiles.cpu().numpy().view(np.uint32), host.view(np.uint32))
    assert (rec[16 * abi.GO1_TUNNEL_REC:] == guard).all()  # the records keep their size
    # the same tiles through the new entry
    spec = abi.Go1TunnelSpec(base=p, kind=abi.GO1_TUNNEL_SINGLE_PATH)
    rec2 = torch.empty((16, abi.GO1_TUNNEL_SPEC_REC), dtype=torch.float64, device=DEV)
    tiles2 = torch.empty_like(tiles)
    native.check(lib, lib.go1_tunnel_generate(C.byref(spec), ext.data_ptr(), rec2.data_ptr(), tiles2.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(tiles, tiles2)


# ---------------------------------------------------------------------------------------------- the env
@pytest.mark.parametrize("kind", ["narrow_path", "random_pyramid"])
def test_env_on_each_new_kind(kind):
    """Tiles on the device equal terrain.build on the host; 8 steps of N(0, 1) actions give finite observations
    within the clip and time-out => reset.  (No zero-divergence assertion: random_pyramid's floor pyramids stand
    under some spawn points.)"""
    from legged_tracking_amd.env import TrajectoryTrackingEnv
    cfg = TC.kind_cfg(kind, 2, 4, n_envs=N)
    env = TrajectoryTrackingEnv(sim_device=DEV, cfg=cfg, seed=5)
    assert isinstance(env.terrain.tiles, torch.Tensor) and env.terrain.tiles.is_cuda and env.terrain.kind == kind
    host = T.build(cfg, N, np.random.RandomState(env.seed))
    np.testing.assert_array_equal(env.terrain.tiles.cpu().numpy(), host.tiles)
    np.testing.assert_array_equal(env.terrain.env_tile, host.env_tile)
    np.testing.assert_array_equal(env.terrain.env_origins, host.env_origins)
    assert (env._abi_cfg.hf_nx, env._abi_cfg.hf_ny) == (80, 40)
    env.reset()
    clip = float(cfg.normalization.clip_observations)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(8):
        obs, rew, reset, extras = env.step(torch.randn((N, 12), device=DEV, generator=gen))
        assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
        assert obs.abs().max().item() <= clip
        assert not (env.time_out_buf & ~reset).any()
    env.close()


def test_set_terrain_rejects_tiles_of_another_shape():
    cfg = TC.kind_cfg("random_pyramid", 2, 2, n_envs=N, geometry=TC.DEFAULT_GEOMETRY)
    td = T.build(cfg, N, np.random.RandomState(3))
    g = native.Go1Native(CF.build_abi_config(cfg, n_envs=N), DEV)  # hf_shape left at (80, 40)
    with pytest.raises(native.NativeError, match="hf_nx"):
        g.set_terrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    g.close()


# ---------------------------------------------------------------------------------------------- height scan
def _handle(cfg, td, n, seed):
    lay = T.tunnel_layout(cfg.terrain)
    c = CF.build_abi_config(cfg, n_envs=n, hf_shape=(lay.tile_x, lay.tile_y))
    g = native.Go1Native(c, DEV)
    g.set_terrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    rng = np.random.default_rng(seed)
    for k, (lo, hi) in {"friction": (0.1, 3.0), "restitution": (0.0, 0.4), "payload": (-1.0, 3.0)}.items():
        g.state[k].copy_(torch.from_numpy(rng.uniform(lo, hi, (n, 1)).astype(np.float32)))
    keep = g.reset_envs(torch.ones(n, dtype=torch.bool, device=DEV), rng_seed=11, rng_step=0)
    g.state["episode_length"].copy_(torch.from_numpy(rng.integers(0, 400, (n, 1)).astype(np.int32)))
    torch.cuda.synchronize()
    del keep
    return c, g


@pytest.mark.parametrize("kind,geometry,shape", [("random_pyramid", None, (80, 40)),
                                                 ("random_pyramid", TC.DEFAULT_GEOMETRY_INSIDE, (160, 72)),
                                                 ("single_path", TC.DEFAULT_GEOMETRY_INSIDE, (160, 72))])
def test_height_scan_bit_exact_from_post_physics_pose(kind, geometry, shape):
    """The numpy restatement of _get_heights (:1918-1965) of
    tests/test_gpu_full_size.py::test_full_size_height_scan_bit_exact_from_post_physics_pose, at the GPU's own
    post-physics pose, every env that did not reset, 4 steps: bit-exact at either tile geometry."""
    cfg = TC.kind_cfg(kind, 2, 4, n_envs=N, geometry=geometry)
    td = T.build(cfg, N, np.random.RandomState(11))
    assert td.tiles.shape[2:] == shape
    c, g = _handle(cfg, td, N, seed=12)
    assert (c.hf_nx, c.hf_ny) == shape
    assert g.specialized == (shape == (80, 40))  # the README specialisation is compiled for (80, 40) tiles only
    scales = CF.reward_scale_vector(CF.derived(cfg)["reward_scales"])
    grav, gvec = CF.gravity_state([0.0, 0.0, 0.0])
    dbg = native.debug_buffers(N, c.decimation, DEV)
    gx = np.array([c.height_grid_x[i] for i in range(21)], np.float32)
    gy = np.array([c.height_grid_y[i] for i in range(11)], np.float32)
    hs, nx, ny = np.float32(c.horizontal_scale), int(c.hf_nx), int(c.hf_ny)
    camx = np.float32(c.camera_offset_x) if c.camera_zero else np.float32(0.0)
    org = td.env_terrain_origin.astype(np.float32)
    tiles = td.tiles.astype(np.float32)
    gen = torch.Generator(device=DEV).manual_seed(2)
    checked, distinct = 0, set()
    for t in range(4):
        g.state["base_rotation"][:, 1] = 0.0
        g.step(torch.randn((N, 12), device=DEV, generator=gen), gvec, grav, scales, rng_seed=8, rng_step=t, debug=dbg)
        torch.cuda.synchronize()
        keepenv = ~g.reset.cpu().numpy().astype(bool)
        root = g.state["root"].cpu().numpy()
        px = (gx[None, :] + root[:, 0:1]).astype(np.float32)
        py = (gy[None, :] + root[:, 1:2]).astype(np.float32)
        if c.camera_zero:
            px = (px + camx).astype(np.float32)
            py = (py + np.float32(0.0)).astype(np.float32)
        px = (px - org[:, 0:1]).astype(np.float32)
        py = (py - org[:, 1:2]).astype(np.float32)
        fx = np.minimum(np.maximum(px / hs, np.float32(-1.0)), np.float32(nx)).astype(np.float32)
        fy = np.minimum(np.maximum(py / hs, np.float32(-1.0)), np.float32(ny)).astype(np.float32)
        ix = np.clip(np.trunc(fx).astype(np.int64), 0, nx - 2)
        iy = np.clip(np.trunc(fy).astype(np.int64), 0, ny - 2)
        tix = td.env_tile.astype(np.int64)
        want = tiles[tix[:, None, None, None], np.arange(2)[None, :, None, None], ix[:, None, :, None],
                     iy[:, None, None, :]]
        got = dbg["heights"].cpu().numpy()
        np.testing.assert_array_equal(got[keepenv], want[keepenv], err_msg=f"step {t}")
        checked += int(keepenv.sum())
        distinct.update(np.unique(want[keepenv]).tolist())
    assert checked > 3 * N
    assert len(distinct) > 8  # the scan saw obstacles, not only the flat floor and ceiling
    g.close()


# ---------------------------------------------------------------------------------------------- integrator
WIDE_SEED = 0


def wide_single_path_setup(seed, n=N):
    """single_path with the README tunnel settings on (160, 80) tiles (terrain_length 8.0, terrain_width 4.0):
    the states and actions of the one-step comparison (CPU only; the seed search runs it without a GPU)."""
    cfg = TC.kind_cfg("single_path", 2, 4, n_envs=n, geometry=dict(terrain_length=8.0, terrain_width=4.0))
    lay = T.tunnel_layout(cfg.terrain)
    assert (lay.tile_x, lay.tile_y) == (160, 80)
    c = CF.build_abi_config(cfg, n_envs=n, hf_shape=(lay.tile_x, lay.tile_y))
    td = T.build(cfg, n, np.random.RandomState(11))
    ter = O.NpTerrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    st = O.NpState(n, cfg=c)
    rng = np.random.default_rng(seed)
    st["friction"][:, 0] = rng.uniform(0.1, 3.0, n)
    st["restitution"][:, 0] = rng.uniform(0.0, 0.4, n)
    st["payload"][:, 0] = rng.uniform(-1.0, 3.0, n)
    O.reset_envs(c, st, ter, np.ones(n, np.uint8), rng_seed=seed, rng_step=0)
    st["episode_length"][:, 0] = rng.integers(0, 499, n)
    act = rng.normal(0, 1, (n, 12)).astype(np.float32)
    return cfg, c, td, ter, st, act


def test_one_step_vs_f64_oracle_on_wide_tiles():
    """One env step of the f32 HIP integrator against the f64 oracle on (160, 80) tiles, held to
    tests/test_gpu_parity.check_integrator_step as it is (its bounds, its flip cap 1 + n // 1000).

    The seed was chosen on the CPU: for seeds 0 .. 11 of wide_single_path_setup the oracle's f32 build passes this
    same check against its f64 build (no contact-set flip; seed 0: max relative error 3.5e-7 dof_pos, 3.3e-5 dof_vel,
    7.2e-6 root, 19 of the 64 envs in contact), so seed 0, the first, is used."""
    from tests.test_gpu_parity import check_integrator_step
    cfg, c, td, ter, st, act = wide_single_path_setup(WIDE_SEED)
    g = native.Go1Native(c, DEV)
    assert not g.specialized
    g.set_terrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    grav, gvec = CF.gravity_state([0.2, -0.1, 0.3])
    scales = CF.reward_scale_vector(CF.derived(cfg)["reward_scales"])
    g.state.load(st.arrays)
    g.step(torch.from_numpy(act).to(DEV), gvec, grav, scales, rng_seed=3, rng_step=100)
    torch.cuda.synchronize()
    out = O.step(c, st, ter, act, gvec, grav, scales, rng_seed=3, rng_step=100, debug=False)
    check_integrator_step(g.state.numpy(), st, g.contact_forces.cpu().numpy(), out["contact_forces"],
                          g.reset.cpu().numpy().astype(bool), out["reset"].astype(bool))
    assert (np.linalg.norm(out["contact_forces"], axis=2) > 0).any(axis=1).sum() >= 8  # the step had contacts
    assert np.isfinite(g.obs.cpu().numpy()).all()
    g.close()


# ---------------------------------------------------------------------------------------------- recording
def test_render_frame_on_wide_pyramid_tiles():
    """One render() frame of a random_pyramid env on (160, 72) tiles: bit-identical to a direct render of the same
    state (as tests/test_gpu_recording.py checks for single_path), and the picture shows terrain."""
    from legged_tracking_amd import render as R
    from legged_tracking_amd.env import TrajectoryTrackingEnv
    cfg = TC.kind_cfg("random_pyramid", 2, 2, n_envs=16, geometry=TC.DEFAULT_GEOMETRY_INSIDE)
    env = TrajectoryTrackingEnv(sim_device=DEV, headless=True, cfg=cfg, seed=3)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(2):
        env.step(0.1 * torch.randn((16, 12), device=DEV, generator=gen))
    frame = env.render()
    assert frame.shape == (240, 360, 4) and frame.dtype == np.uint8
    st, keep = env._sim.state, env._sim._terrain_keep
    assert tuple(keep[0].shape[1:]) == (2, 160, 72)
    sc = R.Scene(st["root"], st["dof_pos"], tiles=keep[0], env_tile=keep[1], env_terrain_origin=keep[2],
                 horizontal_scale=float(cfg.terrain.horizontal_scale), trajectory=st["trajectory"],
                 curr_pose_index=st["curr_pose_index"])
    views = R.views_tensor([(0, R.MODE_FOLLOW, R.VIEW_NO_CEILING)], env.device)
    rgba, prim = R.render_views(sc, views, 360, 240, prim_id=True)
    assert frame.tobytes() == rgba.cpu().numpy()[0].tobytes()
    ids = set(np.unique(prim.cpu().numpy()).tolist())
    assert R.PRIM_FLOOR in ids and ids & set(range(17))  # the terrain and the robot are in the picture
    env.close()
