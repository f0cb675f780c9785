"""The velocity env end to end against a recording of itself (tests/golden/host_refactor/vel_env_16.npz).

The fixture was recorded with this file's record() before the env classes and bindings of env.py /
velocity.py / native.py were put on a shared base: HistoryWrapper(VelocityTrackingEasyEnv(num_envs=16,
seed=1)), reset(), then 40 steps of seeded actions -- past the history rewind at step HIST_WINDOW = 32.
Recorded twice; every array was bitwise equal between the two recordings and is compared bitwise here:
per step obs, rew, reset and extras["privileged_obs"], the last obs_history and the final state planes.
"""
import os

import numpy as np
import pytest
import torch

from legged_tracking_amd import velocity as VEL
from legged_tracking_amd.env import HistoryWrapper

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_refactor", "vel_env_16.npz")
N, STEPS = 16, 40


def record(device="cuda:0"):
    env = HistoryWrapper(VEL.VelocityTrackingEasyEnv(sim_device=device, num_envs=N, seed=1))
    assert env._fused and STEPS > VEL.HIST_WINDOW
    first = env.reset()
    out = {"reset/obs": first["obs"].cpu().numpy(), "reset/obs_history": first["obs_history"].cpu().numpy()}
    g = torch.Generator().manual_seed(0)
    steps = {k: [] for k in ("obs", "rew", "reset", "privileged_obs")}
    for _ in range(STEPS):
        o, rew, done, info = env.step(torch.randn(N, 12, generator=g).to(device))
        assert o["privileged_obs"] is info["privileged_obs"]
        for k, v in (("obs", o["obs"]), ("rew", rew), ("reset", done), ("privileged_obs", info["privileged_obs"])):
            steps[k].append(v.cpu().numpy())
    out.update({f"steps/{k}": np.stack(v) for k, v in steps.items()})
    out["last/obs_history"] = o["obs_history"].cpu().numpy()
    out.update({f"state/{k}": v.cpu().numpy() for k, v in env.state.items()})
    env.close()
    return out


def test_vel_env_replays_recording_bitwise():
    want = np.load(FIXTURE)
    got = record()
    assert set(want.files) <= set(got) and len(want.files) >= 30
    assert want["steps/reset"].any() and not want["steps/reset"].all()  # the run has resets and survivors
    for k in want.files:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k
