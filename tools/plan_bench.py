"""Time the local target planner (legged_tracking_amd/plan.py) and what it costs the step, at 4096 envs.

  python tools/plan_bench.py [--envs 4096] [--terrains single_path random_pyramid] [--steps 200] [--rounds 3]

Per terrain, on one GPU, all in one process so that the numbers share a session:
  step_ms_off / step_ms_on   the step kernel alone (HIP events on its dispatch, as bench.py takes them) of an env
                             without and with planning, i.e. without and with the measured-heights store, in
                             alternating blocks of --steps steps, --rounds times (the spread is printed);
  plan_us[...]               one go1_plan_step launch over the planning env's own planes (real heights), mean of 300
                             back-to-back launches between two events: "none" no env plans (the launch's floor),
                             "steady" plan_length staggered so that n / plan_interval envs plan per launch,
                             "all" every env plans (the first step of a run).
Prints one JSON line per terrain.  No GPU: fails (nothing here is a CPU measurement)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as BN  # noqa: E402  (EventPairs)
from legged_tracking_amd import config as CF, env as E, plan as P  # noqa: E402

LAUNCHES = 300


def make_env(n, terrain, planning, interval, dev):
    cfg = CF.readme_config(n_envs=n, terrain=terrain)
    cfg.commands.sampling_based_planning = planning
    cfg.commands.plan_interval = interval
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


def plan_launches(env, interval, mode):
    """Mean time (us) of a go1_plan_step launch over env's planes; -> (us, envs planning per launch, searching)."""
    base, cfg = env.env, env.env.cfg
    n, st, g = base.num_envs, base._sim.state, CF.scan_grid(cfg)
    # switch thresholds no pose misses: plan_buf stays set, so an env plans whenever its interval comes round
    pb = P.PlanBuffers(n, base.device, cfg.commands.candidate_target_poses, g["x"], g["y"], cfg.commands.traj_length,
                       {"none": 1 << 30, "steady": interval, "all": 1}[mode], 1e9, 1e9,
                       cfg.normalization.clip_observations)
    pb.mark_reset(torch.arange(n))
    pb.idx_prev.copy_(st["curr_pose_index"][:, 0])
    if mode == "steady":
        pb.plan_length_buf.copy_(torch.arange(n, dtype=torch.int32) % interval)
    ep = torch.full((n, 1), 7, dtype=torch.int32, device=base.device)  # no episode starts: the interval alone plans
    reset = torch.zeros(n, dtype=torch.bool, device=base.device)
    obs = torch.zeros((n, base.num_obs), device=base.device)
    args = (st["root"], st["trajectory"], st["curr_pose_index"], ep, reset, base.planner.heights, obs)
    for _ in range(20):
        pb.launch(*args)
    torch.cuda.synchronize()
    planned = searched = 0
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        pb.launch(*args)
    e.record()
    torch.cuda.synchronize()
    for _ in range(8):  # what a launch does, counted outside the timed window
        pb.launch(*args)
        planned += int((pb.chosen != P.NOT_PLANNED).sum())
        searched += int(((pb.chosen >= 0) | (pb.chosen == P.NONE_VALID)).sum())
    return s.elapsed_time(e) / LAUNCHES * 1e3, planned / 8, searched / 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--terrains", nargs="+", default=["single_path", "random_pyramid"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--interval", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: plan_bench measures on the device only")
    dev = "cuda:0"
    for terrain in a.terrains:
        off, on = (make_env(a.envs, terrain, p, a.interval, dev) for p in (False, True))
        ring = torch.randn((64, a.envs, 12), device=dev, generator=torch.Generator(device=dev).manual_seed(7))
        for env in (off, on):
            step_block(env, ring, 60)  # warm-up
        ms = {"off": [], "on": []}
        for _ in range(a.rounds):
            ms["off"].append(step_block(off, ring, a.steps))
            ms["on"].append(step_block(on, ring, a.steps))
        out = {"terrain": terrain, "envs": a.envs, "plan_interval": a.interval, "steps_per_block": a.steps,
               "step_ms_off": ms["off"], "step_ms_on": ms["on"], "no_valid_in_env_run": on.env.planner.no_valid(),
               "footprints": int(on.env.planner.tables["foot"].shape[0]),
               "heights_bytes_per_step": int(on.env.planner.heights.numel() * 4), "plan_us": {}}
        for mode in ("none", "steady", "all"):
            us, planned, searched = plan_launches(on, a.interval, mode)
            out["plan_us"][mode] = {"us": round(us, 2), "envs_planning": planned, "envs_searching": searched}
        print(json.dumps(out), flush=True)
        for env in (off, on):
            env.env.close()


if __name__ == "__main__":
    main()
