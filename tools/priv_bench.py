"""Time the privileged-observation assembler (legged_tracking_amd/privileged.py) and what it costs the env step, at
4096 envs.

  python tools/priv_bench.py [--envs 4096] [--steps 200] [--rounds 3]

On one GPU, all in one process so that the numbers share a session:
  loop_us[train | defaults | all]   the env.step loop (HistoryWrapper.step with fixed actions) of an env with friction
                                    and restitution only (no assembler: the parent's path), with the reference's class
                                    defaults (6 columns) and with every flag (45 columns): device time per step between
                                    two events around a block of --steps steps, in alternating blocks, --rounds times
                                    (the spread is printed).  The step kernel is the same code in all three;
  priv_us[6 | 45]                   one go1_priv_step launch over the env's own planes, mean of 300 back-to-back
                                    launches between two events.
Prints one JSON line.  No GPU: fails (nothing here is a CPU measurement)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from legged_tracking_amd import config as CF, env as E, privileged as PV  # noqa: E402

LAUNCHES = 300
READ = ("friction", "restitution", "base_mass", "com_displacement", "motor_strength", "motor_offset", "body_height",
        "body_velocity", "gravity", "clock_inputs", "desired_contact_states")
SETS = {"train": READ[:2], "defaults": READ[:4], "all": READ}


def make_env(n, name, dev):
    cfg = CF.readme_config(n_envs=n, terrain="single_path")
    for k in [k for k in dir(cfg.env) if k.startswith("priv_observe_")]:
        setattr(cfg.env, k, False)
    for k in SETS[name]:
        setattr(cfg.env, "priv_observe_" + k, True)
    cfg.env.num_privileged_obs = len(PV.columns(cfg))
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=dev, cfg=cfg, seed=11))
    env.reset()
    return env


def loop_block(env, ring, steps):
    """Device time (us) per step of a block of env steps."""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for k in range(steps):
        env.step(ring[k % ring.shape[0]])
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps * 1e3


def priv_launches(env):
    """Mean time (us) of a go1_priv_step launch over the env's planes."""
    base = env.env
    p = base.privileged
    out = torch.zeros((base.num_envs, p.width), device=base.device)
    for _ in range(20):
        p.step(out, base.gravities)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        p.step(out, base.gravities)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / LAUNCHES * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: priv_bench measures on the device only")
    dev = "cuda:0"
    envs = {name: make_env(a.envs, name, dev) for name in SETS}
    assert envs["train"].env.privileged is None
    assert [envs[k].env.privileged.width for k in ("defaults", "all")] == [6, 45]
    ring = torch.randn((64, a.envs, 12), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    for env in envs.values():
        loop_block(env, ring, 60)  # warm-up
    us = {name: [] for name in SETS}
    for _ in range(a.rounds):
        for name, env in envs.items():
            us[name].append(round(loop_block(env, ring, a.steps), 2))
    out = {"envs": a.envs, "steps_per_block": a.steps, "loop_us": us,
           "priv_us": {str(envs[k].env.privileged.width): round(priv_launches(envs[k]), 2)
                       for k in ("defaults", "all")}}
    print(json.dumps(out), flush=True)
    for env in envs.values():
        env.env.close()


if __name__ == "__main__":
    main()
