"""Cost of the ray caster's two uses on the README terrain (`render_kernel`):
  * one 360 x 240 look_from_back frame of env 0 (what a recorded step adds), through the recording launch;
  * the 16 x 640 x 480 render_all_envs batch of play.py.

  python tools/render_cost.py [reps]            hipEvent times around `reps` back-to-back launches
  python tools/render_cost.py --loop            the 4096-env VecEnv.step loop with and without a recording
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/render_cost.py    per-launch kernel times (render_kernel)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from legged_tracking_amd import config as CF, env as E, render as R  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def loop(steps=380, n=4096):
    """The VecEnv.step loop of bench.py's size with and without a recording in progress (wall time, synchronised)."""
    import time
    cfg = CF.readme_config(n_envs=n, terrain="single_path", rows=32, cols=32)
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device="cuda:0", headless=True, cfg=cfg, seed=11))
    env.reset()
    acts = [torch.randn(n, 12, device="cuda:0") for _ in range(8)]

    def run():
        for k in range(100):
            env.step(acts[k % 8])
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k in range(steps):
            env.step(acts[k % 8])
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / steps * 1e6
    off = run()
    env.start_recording()
    r = env.env._renderer
    assert steps + 102 < r.capacity
    r.state.copy_(torch.tensor([[R.REC_RECORDING, 0, 0, 0]] * 2, dtype=torch.int32))  # every step draws a frame
    env.env.cfg.env.episode_length_s = 1e9
    no_reset = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    step = env.env._record_step
    env.env._record_step = lambda reset: step(no_reset)  # env 0's own resets must not end the timed recording
    on = run()
    print("VecEnv.step loop at %d envs: %.1f us per step, %.1f us with a recording in progress (+%.1f us, %.0f %% of "
          "the recorded steps' wall time)" % (n, off, on, on - off, 100 * (on - off) / on))


def main():
    if "--loop" in sys.argv:
        return loop()
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    cfg = CF.readme_config(n_envs=16, terrain="single_path", rows=4, cols=4)  # the README's tiles, one env each
    env = E.TrajectoryTrackingEnv(sim_device="cuda:0", headless=True, cfg=cfg, seed=11)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(20):
        env.step(torch.from_numpy(rng.normal(0, 0.3, (16, 12)).astype(np.float32)).cuda())
    r = env._get_renderer()
    # the recording launch, drawing: state RECORDING with room in the ring, no reset
    r.start()
    r.state.copy_(torch.tensor([[R.REC_RECORDING, 0, 0, 0]] * 2, dtype=torch.int32))
    no_reset = torch.zeros(16, dtype=torch.bool, device=env.device)

    assert reps + 2 < r.capacity  # every timed launch draws (the ring does not fill)

    def record():
        r.record_step(no_reset)
    views = r.views(tuple(range(16)), R.MODE_LOOK_FROM_BACK, 0)
    out = torch.empty((16, 480, 640, 4), dtype=torch.uint8, device=env.device)
    one = r.views((0,), R.MODE_LOOK_FROM_BACK, 0)
    out1 = torch.empty((1, 240, 360, 4), dtype=torch.uint8, device=env.device)
    print("360x240 frame, direct launch: %.1f us" % timed(lambda: R.render_views(r.scene(), one, 360, 240, out=out1), reps))
    print("360x240 frame, recording launch: %.1f us" % timed(record, reps))
    print("16 x 640x480 batch: %.1f us" % timed(lambda: R.render_views(r.scene(), views, 640, 480, out=out), reps))
    hit = float((out[..., :3].float().mean(-1) != 0).float().mean())
    print("non-black share of the batch: %.3f" % hit)


if __name__ == "__main__":
    main()
