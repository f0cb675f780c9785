"""Time the after-start domain randomiser (legged_tracking_amd/randomize.py) and what it costs the step, at 4096 envs.

  python tools/dr_bench.py [--envs 4096] [--steps 200] [--rounds 3]

On one GPU, all in one process so that the numbers share a session:
  step_ms_off / step_ms_on   the step kernel alone (HIP events on its dispatch, as bench.py takes them) of an env
                             with both flags off and with both on, in alternating blocks of --steps steps, --rounds
                             times (the spread is printed).  The step kernel is the same code in both: the pair shows
                             whether the launch behind it disturbs it;
  dr_us[...]                 one go1_dr_step launch over the env's own planes, mean of 300 back-to-back launches
                             between two events: "none" no env due (the launch's floor: two loads per lane),
                             "steady" episode lengths staggered so that n / rand_interval envs redraw and
                             n / push_interval envs are pushed per launch, "all" every env due for both.
Prints one JSON line.  No GPU: fails (nothing here is a CPU measurement)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as BN  # noqa: E402  (EventPairs)
from legged_tracking_amd import config as CF, env as E, randomize as RZ  # noqa: E402

LAUNCHES = 300


def make_env(n, on, dev):
    cfg = CF.readme_config(n_envs=n, terrain="single_path")
    cfg.domain_rand.push_robots = cfg.domain_rand.randomize_rigids_after_start = on
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=dev, cfg=cfg, seed=11))
    env.reset()
    return env


def step_block(env, ring, steps, every=4):
    """Mean step-kernel time (ms) over a block of steps."""
    k_ev = (steps + every - 1) // every
    ev = BN.EventPairs(k_ev)
    env.env.kernel_events.extend(ev.pair(k // every) if k % every == 0 else None for k in range(steps))
    for k in range(steps):
        env.step(ring[k % ring.shape[0]])
    torch.cuda.synchronize()
    env.env.kernel_events.clear()
    ms = float(np.mean([ev.ms(i) for i in range(k_ev)]))
    ev.close()
    return ms


def dr_launches(env, mode):
    """Mean time (us) of a go1_dr_step launch over copies of env's planes; -> (us, envs redrawn, envs pushed)."""
    base = env.env
    rz, n, st, dev = base.randomizer, base.num_envs, base._sim.state, base.device
    ri, pi = rz._cfg.rand_interval, rz._cfg.push_interval
    root, fr, rs = st["root"].clone(), st["friction"].clone(), st["restitution"].clone()
    k = torch.arange(n, dtype=torch.int32, device=dev)
    ep = {"none": torch.full((n,), ri * pi + 1, dtype=torch.int32, device=dev), "steady": k + 1,
          "all": torch.full((n,), ri * pi, dtype=torch.int32, device=dev)}[mode].reshape(n, 1).contiguous()
    reset = torch.zeros(n, dtype=torch.bool, device=dev)
    priv = torch.zeros((n, base.num_privileged_obs), device=dev)
    epn = ep[:, 0].cpu().numpy()
    redrawn, pushed = int((epn % ri == 0).sum()), int((epn % pi == 0).sum())
    for _ in range(20):
        rz.launch(root, fr, rs, ep, reset, 1, priv)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(LAUNCHES):
        rz.launch(root, fr, rs, ep, reset, 2 + i, priv)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / LAUNCHES * 1e3, redrawn, pushed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: dr_bench measures on the device only")
    dev = "cuda:0"
    off, on = (make_env(a.envs, f, dev) for f in (False, True))
    assert off.env.randomizer is None and isinstance(on.env.randomizer, RZ.Randomizer)
    ring = torch.randn((64, a.envs, 12), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    for env in (off, on):
        step_block(env, ring, 60)  # warm-up
    ms = {"off": [], "on": []}
    for _ in range(a.rounds):
        ms["off"].append(step_block(off, ring, a.steps))
        ms["on"].append(step_block(on, ring, a.steps))
    c = on.env.randomizer._cfg
    out = {"envs": a.envs, "rand_interval": c.rand_interval, "push_interval": c.push_interval,
           "steps_per_block": a.steps, "step_ms_off": ms["off"], "step_ms_on": ms["on"], "dr_us": {}}
    for mode in ("none", "steady", "all"):
        us, redrawn, pushed = dr_launches(on, mode)
        out["dr_us"][mode] = {"us": round(us, 2), "envs_redrawn": redrawn, "envs_pushed": pushed}
    print(json.dumps(out), flush=True)
    for env in (off, on):
        env.env.close()


if __name__ == "__main__":
    main()
