"""The reference's narrow_path / random_pyramid tiles (tests/golden/terrain_kinds.npz, recorded by
tests/golden/make_golden_terrain.py) and the Cfgs that reproduce them; shared by the CPU and the GPU tests."""
import functools
import json
import os

import numpy as np

from legged_tracking_amd import config as CF

CASES = ("pyramid_4x4", "pyramid_default_geometry", "pyramid_num_1x1", "narrow_4x4", "narrow_p_double_0",
         "narrow_p_double_1")
# the reference's default Cfg.terrain geometry (config.py:92-96): (160, 72) tiles, (36, 80) sub-terrains
DEFAULT_GEOMETRY = dict(terrain_length=8.0, terrain_width=3.6, terrain_ratio_x=0.5, terrain_ratio_y=0.5,
                        ceiling_height=0.5, start_loc=0.4)
# the same tiles with the robots spawned inside the tunnel: at the default start_loc the env origin lies at
# x = 0.8 m, outside the tunnel (which spans x = 2 .. 6 m of the 8 m tile), on the flat 0.5 m surround
DEFAULT_GEOMETRY_INSIDE = dict(DEFAULT_GEOMETRY, start_loc=0.2)


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terrain_kinds.npz"))


def apply_settings(cfg, settings):
    for k, v in settings.items():
        if k in ("top", "bottom"):
            for kk, vv in v.items():
                setattr(getattr(cfg.terrain, k), kk, vv)
        else:
            setattr(cfg.terrain, k, v)
    return cfg


def case(name, n_envs=None):
    """(cfg, seed, tiles f32 (rows, cols, 2, L, W), env_origins, all_terrain_origins) of a recorded case."""
    d = fixture()
    s = json.loads(str(d[f"{name}/settings"]))
    n = n_envs or s["num_rows"] * s["num_cols"]
    cfg = apply_settings(CF.readme_config(n_envs=n, terrain=s["terrain_type"], rows=s["num_rows"],
                                          cols=s["num_cols"]), s)
    # height_samples_by_row_col in raw units -> metres as terrain.make_tunnel ends: (raw * vertical_scale) in
    # float64 -> float32 (the form tests/test_terrain.py pins to the reference's env_height_samples)
    tiles = (d[f"{name}/height_samples"].astype(np.float64) * s["vertical_scale"]).astype(np.float32)
    return cfg, int(d[f"{name}/seed"]), tiles, d[f"{name}/env_origins"], d[f"{name}/all_terrain_origins"]


def kind_cfg(kind, rows, cols, n_envs=None, geometry=None, **pyramid):
    """readme_config with terrain_type `kind`; `geometry` overrides tunnel settings, `pyramid` both layers'."""
    cfg = CF.readme_config(n_envs=n_envs or rows * cols, terrain=kind, rows=rows, cols=cols)
    return apply_settings(cfg, dict(geometry or {}, top=pyramid, bottom=pyramid))
