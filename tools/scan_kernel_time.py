"""Time the generic step kernel (native integrator) at 4096 envs, single_path 32 x 32, per height-scan grid:
the README's 21 x 11 through the register-resident kernels and streamed (Go1Native.scan_mode), 31 x 15 and
61 x 31 streamed, front half and full scan, and the plane (sample() returns constants there: no coordinate loads,
no gathers, the same stores).  An event pair around each of LAUNCHES go1_step calls (one kernel launch each)
after WARM warm-up steps; prints one JSON line per case and writes them to OUT (default
scan_kernel_time.json; DESIGN section 5 quotes profiles/scan_grid/scan_kernel_time.json).

Usage: python tools/scan_kernel_time.py [OUT]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from legged_tracking_amd import config as CF, native, terrain as T  # noqa: E402

DEV = "cuda:0"
N, WARM, LAUNCHES = 4096, 50, 300
README_GRID = (np.linspace(-1, 1, 21), np.linspace(-0.5, 0.5, 11))
CNN_GRID = (np.linspace(-1, 2, 61), np.linspace(-0.75, 0.75, 31))


def case(name, grid, streamed, front=True, terrain="single_path"):
    x, y = grid
    cfg = CF.readme_config(n_envs=N, terrain=terrain, rows=32, cols=32)
    cfg.terrain.measure_front_half = front
    cfg.terrain.measured_points_x, cfg.terrain.measured_points_y = x, y
    rows = len(x) - (len(x) // 2 + 1) if front else len(x)
    cfg.env.num_observations = cfg.env.num_scalar_observations = 41 + 2 * rows * len(y)
    c = CF.build_abi_config(cfg)
    td = T.build(cfg, N, np.random.RandomState(11),
                 tiles_fn=None if terrain == "plane" else
                 (lambda t, lay: native.tunnel_tiles(t, lay, 11, torch.device(DEV))))
    g = native.Go1Native(c, DEV)
    if not g.streamed:
        g.specialize(False)  # the generic kernel on both sides of the comparison
    if streamed:
        g.scan_mode(True)
    g.set_terrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    g.reset_envs(torch.ones(N, dtype=torch.bool, device=DEV), rng_seed=5, rng_step=0)
    grav, gvec = CF.gravity_state([0.0, 0.0, 0.0])
    scales = CF.reward_scale_vector(CF.derived(cfg)["reward_scales"])
    gen = torch.Generator(device=DEV).manual_seed(0)
    acts = [torch.randn((N, 12), device=DEV, generator=gen) * 0.5 for _ in range(8)]
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(LAUNCHES)]
    for k in range(WARM):
        g.step(acts[k % 8], gvec, grav, scales, rng_seed=5, rng_step=1 + k, contact_forces=False)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(evs):
        a.record()
        g.step(acts[k % 8], gvec, grav, scales, rng_seed=5, rng_step=1 + WARM + k, contact_forces=False)
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in evs])
    assert torch.isfinite(g.obs).all()
    out = {"case": name, "terrain": terrain, "front_half": front, "scan": [c.scan_nx, c.scan_ny],
           "streamed": g.streamed, "specialized": g.specialized, "num_obs": c.num_obs,
           "obs_bytes_per_env_step": 4 * c.num_obs, "launches": LAUNCHES, "us_median": float(np.median(us)),
           "us_p10": float(np.percentile(us, 10)), "us_p90": float(np.percentile(us, 90)), "us_min": float(us.min())}
    print(json.dumps(out), flush=True)
    g.close()
    return out


if __name__ == "__main__":
    fine = (np.linspace(-1, 1, 31), np.linspace(-0.5, 0.5, 15))
    res = [case("21x11 compiled-in (generic)", README_GRID, False),
           case("21x11 streamed", README_GRID, True),
           case("31x15 streamed", fine, False),
           case("61x31 streamed", CNN_GRID, False),
           case("61x31 full scan streamed", CNN_GRID, False, front=False),
           case("21x11 full scan compiled-in (generic)", README_GRID, False, front=False),
           case("21x11 full scan streamed", README_GRID, True, front=False),
           case("plane 21x11 compiled-in (generic)", README_GRID, False, terrain="plane"),
           case("plane 61x31 full scan streamed", CNN_GRID, False, front=False, terrain="plane"),
           case("21x11 compiled-in (generic), again", README_GRID, False)]
    out = sys.argv[1] if len(sys.argv) > 1 else "scan_kernel_time.json"
    json.dump({"device": torch.cuda.get_device_name(0), "n_envs": N, "terrain": "single_path 32 x 32",
               "method": f"torch.cuda.Event pair around every go1_step (one kernel launch), {LAUNCHES} launches "
                         f"after {WARM} warm-up steps",
               "cases": res}, open(out, "w"), indent=1)
