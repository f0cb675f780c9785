"""narrow_path and random_pyramid on the host: terrain.make_tunnel against the reference's own tiles
(tests/golden/terrain_kinds.npz, recorded by tests/golden/make_golden_terrain.py), the box writer's slice
semantics, the config guard, the generator's argument checks and the tile geometry through to the step."""
import itertools

import numpy as np
import pytest
import torch

from legged_tracking_amd import config as CF, env as E, native, terrain as T
from tests import terrain_cases as TC
from tests.cpu_backend import OracleBackend


@pytest.mark.parametrize("name", TC.CASES)
def test_make_tunnel_equals_the_reference_bit_for_bit(name):
    cfg, seed, ref, env_origins, all_origins = TC.case(name)
    tiles, eo, ao = T.make_tunnel(cfg.terrain, np.random.RandomState(seed))
    assert tiles.dtype == np.float32 and tiles.shape == ref.shape
    np.testing.assert_array_equal(tiles.view(np.uint32), ref.view(np.uint32))
    np.testing.assert_array_equal(eo, env_origins)
    np.testing.assert_array_equal(ao, all_origins)
    # and through build(): one env per sub-terrain, origins as the env binds them
    n = ref.shape[0] * ref.shape[1]
    td = T.build(cfg, n, np.random.RandomState(seed))
    assert td.kind == cfg.terrain.terrain_type
    np.testing.assert_array_equal(td.tiles[td.env_tile], ref.reshape(n, *ref.shape[2:]))
    np.testing.assert_array_equal(td.env_origins, env_origins.reshape(n, 3).astype(np.float32))
    np.testing.assert_array_equal(td.env_terrain_origin, all_origins.reshape(n, 3).astype(np.float32))


def test_fixtures_are_not_trivial():
    """What the recorder promises: all three d_num classes among pyramid_4x4's difficulties, (160, 72) tiles in
    the default geometry, ceiling and floor boxes in narrow_4x4."""
    d = TC.fixture()
    assert {T.pyramid_d_num(x) for x in d["pyramid_4x4/difficulties"]} == {0, 1, 2}
    assert d["pyramid_default_geometry/height_samples"].shape == (2, 2, 2, 160, 72)
    assert {T.pyramid_d_num(x) for x in d["pyramid_num_1x1/difficulties"]} == {0, 1, 2}  # 1 .. 9 pyramids a layer
    hs = d["narrow_4x4/height_samples"].reshape(16, 2, 80, 40)
    inner = hs[:, :, 5:75, 11:29]  # inside the tunnel, off the floor's walls
    assert 0 < (inner[:, 0].min(axis=(1, 2)) < 160).sum() < 16    # some ceilings carry a box, some none
    assert 0 < (inner[:, 1].max(axis=(1, 2)) > 0).sum() < 16      # and some floors


def test_make_single_path_is_unchanged_by_the_dispatch():
    cfg = CF.readme_config(n_envs=16, terrain="single_path", rows=4, cols=4)
    a = T.make_single_path(cfg.terrain, np.random.RandomState(11))
    b = T.make_tunnel(cfg.terrain, np.random.RandomState(11))
    np.testing.assert_array_equal(a[0], b[0])
    # the draws are narrow_path's too: the stream is at the same position after either producer
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    T.make_tunnel(cfg.terrain, r1)
    T.make_tunnel(TC.kind_cfg("narrow_path", 4, 4).terrain, r2)
    assert r1.uniform() == r2.uniform()


BOUNDS = (-45, -41, -40, -39, -7, -1, 0, 1, 6, 19, 20, 21, 39, 40, 41, 45)


def test_box_writer_has_python_slice_semantics():
    """write_box (the bounds the device rasteriser restates) against plain numpy slicing: negative, reversed,
    past-the-end and empty index pairs on both axes of a (20, 40) field."""
    shape = (20, 40)
    pairs = list(itertools.product(BOUNDS, BOUNDS))
    assert any(lo < 0 <= hi for lo, hi in pairs) and any(lo > hi for lo, hi in pairs)
    for n in shape:
        for lo, hi in pairs:
            assert T.slice_bounds(lo, hi, n)[0] == slice(lo, hi).indices(n)[0]
            assert range(*T.slice_bounds(lo, hi, n)) == range(n)[lo:hi], (lo, hi, n)
    rng = np.random.default_rng(0)
    for _ in range(300):
        xl, xh, yl, yh = (int(rng.choice(BOUNDS)) for _ in range(4))
        want = np.zeros(shape)
        want[xl:xh, yl:yh] = 1.5
        got = np.zeros(shape)
        T.write_box(got, xl, xh, yl, yh, 1.5)
        np.testing.assert_array_equal(got, want, err_msg=str((xl, xh, yl, yh)))


def test_narrow_path_later_boxes_overwrite_earlier_ones():
    # p_double = 1: two boxes per layer; whatever they are, the field is the sequential overwrite of both
    cfg = TC.kind_cfg("narrow_path", 1, 1, geometry=dict(p_double=1.0, p_flat=1.0))
    lay = T.tunnel_layout(cfg.terrain)
    t = cfg.terrain
    for seed in range(40):
        r1, r2 = np.random.RandomState(seed), np.random.RandomState(seed)
        got = T.narrow_path_layer(lay.sub_shape, t.horizontal_scale, t.vertical_scale, 1.0, 1.0, True, r1)
        centres, ww, ll = T._path_draws(lay.sub_shape, t.horizontal_scale, 1.0, 1.0, True, r2)
        want = np.zeros(lay.sub_shape)
        for (x, y, z), w, l in zip(centres, ww, ll):
            hs = t.horizontal_scale
            want[int((x - w / 2) / hs):int((x + w / 2) / hs), int((y - l / 2) / hs):int((y + l / 2) / hs)] = z
        np.testing.assert_array_equal(got, (want / t.vertical_scale).astype(int))


@pytest.mark.parametrize("kind", CF.TUNNEL_TYPES)
def test_guard_accepts_the_three_tunnel_kinds(kind):
    cfg = CF.readme_config(n_envs=16, terrain=kind, rows=4, cols=4)
    assert cfg.terrain.terrain_type == kind and cfg.terrain.terrain_length == 4.0 and cfg.terrain.p_double == 0.6
    assert not CF.unsupported(cfg)
    assert CF.build_abi_config(cfg, n_envs=16).terrain_kind == 1


@pytest.mark.parametrize("kind", ["random", "multi_path", "test_env", "test_env_7"])
def test_guard_still_rejects_the_other_terrain_types(kind):
    cfg = CF.readme_config(n_envs=16, terrain="single_path", rows=4, cols=4)
    cfg.terrain.terrain_type = kind
    with pytest.raises(NotImplementedError, match="terrain_type"):
        CF.build_abi_config(cfg, n_envs=16)
    with pytest.raises(ValueError, match="terrain_type"):
        T.build(cfg, 16)
    with pytest.raises(ValueError):
        CF.readme_config(n_envs=16, terrain=kind, rows=4, cols=4)


def test_default_cfg_is_on_the_path():
    """make_cfg()'s terrain is the reference's default: random_pyramid with the top / bottom sections."""
    C = CF.make_cfg()
    assert C.terrain.terrain_type == "random_pyramid"
    assert (C.terrain.top.pyramid_num_x, C.terrain.bottom.pyramid_num_y, C.terrain.top.pyramid_var_x) == (3, 5, 0.5)
    assert not [b for b in CF.unsupported(C) if b[0] == "terrain.terrain_type"]
    lay = T.tunnel_layout(C.terrain)
    assert (lay.tile_x, lay.tile_y) == (160, 72)


@pytest.mark.parametrize("num, text", [((7, 6), "pyramids per layer"), ((6, 7), "pyramids per layer"),
                                       ((0, 3), "no pyramid"), ((3, -1), "no pyramid")])
def test_generator_rejects_pyramid_counts_before_any_device_work(num, text):
    """More than GO1_TUNNEL_MAX_WEDGES = 64 pyramids in a layer, or a non-positive pyramid_num + 2 - d_num:
    ValueError from native.tunnel_tiles on "cpu" (nothing touches a device), and from the host restatement."""
    cfg = TC.kind_cfg("random_pyramid", 4, 4, pyramid_num_x=num[0], pyramid_num_y=num[1])
    lay = T.tunnel_layout(cfg.terrain)
    with pytest.raises(ValueError, match=text):
        native.tunnel_tiles(cfg.terrain, lay, 11, "cpu")
    with pytest.raises(ValueError, match=text):
        T.make_tunnel(cfg.terrain, np.random.RandomState(11))
    # 6 x 6 is the largest that fits: 64 pyramids
    T.check_pyramid_params(TC.kind_cfg("random_pyramid", 1, 1, pyramid_num_x=6, pyramid_num_y=6).terrain)


def test_env_takes_the_tile_geometry_through_to_the_step():
    """random_pyramid at the default Cfg geometry on the oracle backend: go1_config.hf_nx / hf_ny are the tile
    shape (160, 72), not build_abi_config's 80 x 40 default, and one step runs."""
    cfg = TC.kind_cfg("random_pyramid", 2, 2, n_envs=16, geometry=TC.DEFAULT_GEOMETRY)
    env = E.TrajectoryTrackingEnv(sim_device="cpu", headless=True, cfg=cfg, seed=11, backend=OracleBackend)
    c = env._abi_cfg
    assert (c.hf_nx, c.hf_ny) == (160, 72) == env.terrain.tiles.shape[2:]
    assert env.terrain.kind == "random_pyramid"
    ref = TC.case("pyramid_default_geometry")[2]
    np.testing.assert_array_equal(env.terrain.tiles, ref.reshape(4, 2, 160, 72))  # same seed, same geometry
    obs, rew, reset, extras = env.step(torch.zeros(16, 12))
    assert obs.shape == (16, 261) and torch.isfinite(obs).all() and torch.isfinite(rew).all()
    # the height scan read this tile geometry: floor heights in the observation are tile values
    assert (c.hf_nx, c.hf_ny) == (env._sim.cfg.hf_nx, env._sim.cfg.hf_ny)


def test_set_terrain_rejects_a_tile_shape_the_config_does_not_index():
    """Go1Native.set_terrain's check, on a stand-in for the handle (no GPU): tiles of another shape than
    (hf_nx, hf_ny) raise instead of being mis-indexed by the kernel."""
    cfg = TC.kind_cfg("random_pyramid", 2, 2, n_envs=16, geometry=TC.DEFAULT_GEOMETRY)
    c = CF.build_abi_config(cfg, n_envs=16)  # hf_shape left at 80 x 40
    td = T.build(cfg, 16, np.random.RandomState(11))

    class Handle:  # the attributes set_terrain reads before it reaches the library
        device, cfg = torch.device("cpu"), c
    with pytest.raises(native.NativeError, match=r"hf_nx"):
        native.Go1Native.set_terrain(Handle(), td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)


def test_play_keeps_a_checkpoints_terrain_type(tmp_path):
    import pickle
    from legged_tracking_amd import play
    saved = {"terrain": {"terrain_type": "random_pyramid", "top": {"pyramid_num_x": 2}}}
    (tmp_path / "parameters.pkl").write_bytes(pickle.dumps(saved))
    cfg = play.load_cfg(str(tmp_path), 16, 64, 48)
    assert cfg.terrain.terrain_type == "random_pyramid" and cfg.terrain.top.pyramid_num_x == 2
    assert cfg.terrain.bottom.pyramid_num_x == 3
    assert play.load_cfg(str(tmp_path), 16, 64, 48, terrain="narrow_path").terrain.terrain_type == "narrow_path"
    assert play.load_cfg(str(tmp_path / "none"), 16, 64, 48).terrain.terrain_type == "single_path"


def test_library_rejects_bad_specs_without_a_gpu():
    """go1_tunnel_generate's own argument checks (they precede any HIP call, so they run here), through the ctypes
    mirror of go1_tunnel_spec: the message names the layer whose block was changed, which a mis-laid-out mirror
    would not."""
    import ctypes as C
    from legged_tracking_amd import abi
    lib = native.lib()
    cfg = TC.kind_cfg("random_pyramid", 2, 2)
    t, lay = cfg.terrain, T.tunnel_layout(cfg.terrain)
    p = abi.Go1TunnelParams(num_rows=2, num_cols=2, tile_x=lay.tile_x, tile_y=lay.tile_y, sub_x=lay.sub_shape[0],
                            sub_y=lay.sub_shape[1], seed=1, horizontal_scale=t.horizontal_scale,
                            vertical_scale=t.vertical_scale, ceiling_height=t.ceiling_height)
    buf = (C.c_double * 8)()  # never read or written: every call below is rejected before a launch
    ptr = C.addressof(buf)
    assert lib.go1_tunnel_generate(None, ptr, ptr, ptr, None) == -1 and b"null" in lib.last_error()
    for layer, num, kind, text in (("bottom", (7, 6), 2, "bottom layer has 72 pyramids"),
                                   ("top", (6, 7), 2, "top layer has 72 pyramids"),
                                   ("top", (0, 3), 2, "top pyramid_num_x / pyramid_num_y must be >= 1"),
                                   ("bottom", (3, 5), 3, "unknown kind 3"), ("bottom", (3, 5), -1, "unknown kind -1")):
        spec = abi.Go1TunnelSpec(base=p, kind=kind, top=native._pyramid_params(t.top),
                                 bottom=native._pyramid_params(t.bottom))
        getattr(spec, layer).num_x, getattr(spec, layer).num_y = num
        assert lib.go1_tunnel_generate(C.byref(spec), ptr, ptr, ptr, None) == -1  # GO1_E_ARG
        assert text in lib.last_error().decode(), lib.last_error()
    spec = abi.Go1TunnelSpec(base=p, kind=1)
    spec.base.sub_x = 1
    assert lib.go1_tunnel_generate(C.byref(spec), ptr, ptr, ptr, None) == -1 and b"grid shape" in lib.last_error()
    assert lib.go1_tunnel_tiles(C.byref(spec.base), ptr, ptr, ptr, None) == -1
    assert b"go1_tunnel_tiles: bad grid shape" in lib.last_error()
