"""Record the reference's tunnel tiles for narrow_path and random_pyramid (tests/golden/terrain_kinds.npz).

Test infrastructure only: imports the reference's go1_gym.utils.tunnel.Terrain behind the offline stand-ins
(tests/golden/refstubs, as make_golden.py does), calls np.random.seed(seed) and builds Terrain(cfg.terrain)
for each case below.  What runs is the reference's own producer: Terrain.__init__ / make_terrain /
add_terrain_to_map (tunnel.py:51-217) with TerrainFunctions.narrow_path (tunnel_fn.py:44-97) and
TerrainFunctions.random_pyramid (:546-581); only visual_elevation_map (a matplotlib window for sub-terrain 0) is
replaced by a no-op.

Stored per case: height_samples_by_row_col as int16 raw height units (the recorder checks that the rounding
loses nothing once the tiles are float32 metres), env_origins, all_terrain_origins, the difficulty draws, the
seed and the terrain settings as JSON.

Usage: python tests/golden/make_golden_terrain.py --reference DIR   (DIR holds go1_gym/)
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

sys.dont_write_bytecode = True  # the reference tree is read-only
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np  # noqa: E402

# scripts/train.py:135-142 (--terrain single_path): the README tunnel geometry
README_TUNNEL = dict(terrain_length=4.0, terrain_width=2.0, terrain_ratio_x=0.9, terrain_ratio_y=0.5,
                     ceiling_height=0.8, start_loc=0.32, p_flat=0.9, p_double=0.6)
PYRAMID_KEYS = ("pyramid_num_x", "pyramid_num_y", "pyramid_var_x", "pyramid_var_y", "pyramid_length_min",
                "pyramid_length_max", "pyramid_height_min", "pyramid_height_max")

# name -> (terrain_type, rows, cols, first seed tried, settings over the reference's default Cfg.terrain,
#          pyramid settings for top and bottom, need all three d_num classes)
CASES = {
    "pyramid_4x4": ("random_pyramid", 4, 4, 11, README_TUNNEL, {}, True),
    # the reference's default Cfg geometry: 8.0 x 3.6 m, both ratios 0.5, ceiling 0.5 -> (160, 72) tiles
    "pyramid_default_geometry": ("random_pyramid", 2, 2, 11, {}, {}, False),
    "pyramid_num_1x1": ("random_pyramid", 4, 4, 11, README_TUNNEL, dict(pyramid_num_x=1, pyramid_num_y=1), False),
    "narrow_4x4": ("narrow_path", 4, 4, 11, README_TUNNEL, {}, False),
    "narrow_p_double_0": ("narrow_path", 4, 4, 11, dict(README_TUNNEL, p_double=0.0), {}, False),
    "narrow_p_double_1": ("narrow_path", 4, 4, 11, dict(README_TUNNEL, p_double=1.0), {}, False),
}


def d_num_classes(difficulties):
    return {2 if d < 0.25 else (1 if d < 0.625 else 0) for d in difficulties}


def record(name, tunnel, config):
    kind, rows, cols, seed, settings, pyramid, all_classes = CASES[name]
    while True:
        Cfg = type("Cfg", (config.Cfg,), {})  # the module's class stays untouched between cases
        t = type("terrain", (config.Cfg.terrain,), {})
        t.top = type("top", (config.Cfg.terrain.top,), dict(pyramid))
        t.bottom = type("bottom", (config.Cfg.terrain.bottom,), dict(pyramid))
        t.terrain_type, t.num_rows, t.num_cols = kind, rows, cols
        for k, v in settings.items():
            setattr(t, k, v)
        Cfg.terrain = t
        difficulties = []
        make = tunnel.Terrain.make_terrain

        def logged(self, terrain_type, difficulty, k, top=True):
            if top:
                difficulties.append(float(difficulty))
            return make(self, terrain_type, difficulty, k, top=top)

        tunnel.Terrain.make_terrain = logged
        try:
            np.random.seed(seed)
            ter = tunnel.Terrain(t, rows * cols)
        finally:
            tunnel.Terrain.make_terrain = make
        if not all_classes or d_num_classes(difficulties) == {0, 1, 2}:
            break
        seed += 1
    raw = ter.height_samples_by_row_col
    q = np.rint(raw).astype(np.int16)
    vs = t.vertical_scale
    assert np.abs(raw).max() < 32767
    # the tests compare float32 metres: the int16 rounding must not change one of them
    np.testing.assert_array_equal((raw * vs).astype(np.float32), (q * vs).astype(np.float32))
    keys = ("terrain_type", "num_rows", "num_cols", "terrain_length", "terrain_width", "terrain_ratio_x",
            "terrain_ratio_y", "ceiling_height", "start_loc", "horizontal_scale", "vertical_scale", "p_flat",
            "p_double")
    meta = {k: getattr(t, k) for k in keys if hasattr(t, k)}
    meta["top"] = {k: getattr(t.top, k) for k in PYRAMID_KEYS}
    meta["bottom"] = {k: getattr(t.bottom, k) for k in PYRAMID_KEYS}
    print(f"{name}: seed {seed}, tiles {q.shape}, d_num classes {sorted(d_num_classes(difficulties))}")
    return {f"{name}/height_samples": q, f"{name}/env_origins": ter.env_origins,
            f"{name}/all_terrain_origins": ter.all_terrain_origins, f"{name}/difficulties": np.array(difficulties),
            f"{name}/seed": np.int64(seed), f"{name}/settings": np.array(json.dumps(meta))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (the directory holding go1_gym/)")
    ap.add_argument("--out", default=os.path.join(HERE, "terrain_kinds.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, "refstubs"))
    sys.path.insert(1, a.reference)
    from go1_gym.envs.base import legged_robot_trajectory_tracking_config as config
    from go1_gym.utils import tunnel
    tunnel.visual_elevation_map = lambda *args, **kw: None
    out = {}
    for name in CASES:
        out.update(record(name, tunnel, config))
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
