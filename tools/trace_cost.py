"""Cost of the episode tracer's push launch (legged_tracking_amd/trace.py) at the README size: 4096 envs on
single_path 32 x 32, full depth (max_episode_length + 1 rows per env).

  python tools/trace_cost.py steps [N]   N rollout-like env steps (random actions) with a tracer attached; run it
                                         under `rocprofv3 --kernel-trace --stats` and read the average of
                                         go1_trace_push_kernel beside the step kernel's
  python tools/trace_cost.py burst       the one push in which all 4096 envs end with a full ring, capacity 4096,
                                         timed with HIP events, beside a push in which none ends
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from legged_tracking_amd import config as CF, env as E, trace as T  # noqa: E402

DEV = "cuda:0"
N = 4096


def make_env():
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=32, cols=32)
    return E.TrajectoryTrackingEnv(sim_device=DEV, headless=True, cfg=cfg, seed=3)


def steps(n):
    env = make_env()
    env.reset()
    tracer = T.EpisodeTracer(env, capacity=256)
    env.attach_tracer(tracer)
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(n):
        env.step(torch.randn(N, env.num_actions, device=DEV, generator=g))
    torch.cuda.synchronize()
    print(json.dumps({"mode": "steps", "steps": n, "depth": tracer.depth, "counts": tracer.counts(),
                      "ring_MB": tracer.ring.numel() * 4 / 1e6}))
    env.close()


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def burst():
    env = make_env()
    env.reset()
    st = env._sim.state
    depth = int(env.max_episode_length) + 1
    out = {"mode": "burst", "depth": depth}
    none = torch.zeros(N, dtype=torch.bool, device=DEV)
    every = torch.ones(N, dtype=torch.bool, device=DEV)
    for rep in range(3):
        buf = T.TraceBuffers(st["root"], st["dof_pos"], depth, N, trajectory=st["trajectory"],
                             wp_index=st["curr_pose_index"])
        for _ in range(depth + 3):
            buf.push(none, none)
        torch.cuda.synchronize()
        plain = min(_timed(lambda: buf.push(none, none)) for _ in range(20))
        out[f"plain_push_us_{rep}"] = round(plain, 2)
        out[f"burst_push_us_{rep}"] = round(_timed(lambda: buf.push(every, every)), 2)
        assert buf.counts() == (N, 0)
        out["burst_MB"] = 2 * N * depth * T.ROW * 4 / 1e6
        del buf
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "steps"
    if mode == "steps":
        steps(int(sys.argv[2]) if len(sys.argv) > 2 else 300)
    elif mode == "burst":
        burst()
    else:
        raise SystemExit(__doc__)
