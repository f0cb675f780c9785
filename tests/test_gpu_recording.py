"""Recording on the HIP env: one episode of env 0 lands in the device frame ring, frame by frame the picture of the
state after that step, and recording changes nothing the step computes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from legged_tracking_amd import config as CF

pytestmark = pytest.mark.gpu

N, EPISODE = 16, 10
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_env():
    from legged_tracking_amd import env as E
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=2, cols=2)
    cfg.env.episode_length_s = (EPISODE - 0.5) * CF.derived(cfg)["dt"]   # max_episode_length = ceil(9.5) = 10 steps
    env = E.TrajectoryTrackingEnv(sim_device="cuda:0", headless=True, cfg=cfg, seed=3)
    assert int(env.max_episode_length) == EPISODE
    return env


def run(record, steps=40):
    """Small actions (the robot stands, so episodes end by time-out) until env 0 has reset twice; returns the
    per-step outputs, the snapshots after every step, env 0's reset steps, the frames and the final state."""
    from legged_tracking_amd import render as R
    env = make_env()
    env.reset()
    rng = np.random.default_rng(0)
    if record:
        assert env.get_complete_frames() == []
        env.start_recording()
        assert env.get_complete_frames() == []
    outs, snaps, resets = [], [], []
    for k in range(steps):
        a = torch.from_numpy(rng.normal(0, 0.1, (N, 12)).astype(np.float32)).cuda()
        obs, rew, reset, extras = env.step(a)
        outs.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), reset.cpu().numpy().copy()))
        st = env._sim.state
        snaps.append({k2: st[k2].clone() for k2 in ("root", "dof_pos", "trajectory", "curr_pose_index")})
        if outs[-1][2][0]:
            resets.append(k)
        if len(resets) == 2:
            break
    frames = env.get_complete_frames() if record else None
    final = {k2: v.cpu().numpy().copy() for k2, v in env._sim.state.t.items()}
    extra = None
    if record:
        keep = env._sim._terrain_keep
        direct = []
        for k in range(resets[0], resets[1]):
            s = snaps[k]
            sc = R.Scene(s["root"], s["dof_pos"], tiles=keep[0], env_tile=keep[1], env_terrain_origin=keep[2],
                         horizontal_scale=float(env.cfg.terrain.horizontal_scale), trajectory=s["trajectory"],
                         curr_pose_index=s["curr_pose_index"])
            direct.append(R.render_views(sc, R.views_tensor([(0, R.MODE_LOOK_FROM_BACK, 0)], env.device), 360, 240)
                          .cpu().numpy()[0])
        env.cfg.env.record_all_envs = True
        env.cfg.env.recording_width_px, env.cfg.env.recording_height_px = 64, 48
        extra = dict(direct=direct, render=env.render(), all=env.render_all_envs(),
                     again=env.get_complete_frames())
        env.pause_recording()
        extra["paused"] = env.get_complete_frames()
    env.close()
    return outs, resets, frames, final, extra


@pytest.fixture(scope="module")
def runs():
    return run(True), run(False)


def test_one_episode_is_recorded_frame_by_frame(runs):
    (outs, resets, frames, _, extra), _ = runs
    assert len(resets) == 2, resets
    assert len(frames) == resets[1] - resets[0] and 1 <= len(frames) <= EPISODE + 1
    for k, (f, d) in enumerate(zip(frames, extra["direct"])):
        assert f.shape == (240, 360, 4) and f.dtype == np.uint8
        assert f.tobytes() == d.tobytes(), k
    assert len({f.tobytes() for f in frames}) > 1      # the robot moves
    assert extra["again"] is frames or all((a == b).all() for a, b in zip(extra["again"], frames))
    assert extra["paused"] == []


def test_recording_changes_nothing_the_step_computes(runs):
    (outs, resets, _, final, _), (outs0, resets0, _, final0, _) = runs
    assert resets == resets0 and len(outs) == len(outs0)
    for k, (a, b) in enumerate(zip(outs, outs0)):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), k
    for k in final:
        assert final[k].tobytes() == final0[k].tobytes(), k


def test_render_and_render_all_envs_have_the_configured_shapes(runs):
    extra = runs[0][4]
    assert extra["render"].shape == (240, 360, 4) and extra["render"].dtype == np.uint8
    assert len(extra["all"]) == N and all(f.shape == (48, 64, 4) and f.dtype == np.uint8 for f in extra["all"])
    assert len({f.tobytes() for f in extra["all"]}) > 1


def test_render_all_envs_is_gated_by_the_config():
    env = make_env()
    assert not getattr(env.cfg.env, "record_all_envs", False)
    assert env.render_all_envs() is None
    assert env._renderer is None        # nothing was allocated
    env.close()


def test_play_writes_one_file_per_env(tmp_path):
    from legged_tracking_amd import env as E, rollout as RO
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=2, cols=2)
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device="cuda:0", headless=True, cfg=cfg, seed=3))
    runner = RO.Runner(env, device="cuda:0", save_dir=str(tmp_path / "ckpt"))
    runner.save()
    env.close()
    out = tmp_path / "videos"
    r = subprocess.run([sys.executable, "-m", "legged_tracking_amd.play", str(tmp_path / "ckpt"), "--out", str(out),
                        "--envs", "4", "--width", "64", "--height", "48", "--steps", "20"], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(os.listdir(out))
    assert len(files) == 4 and all(f.startswith("env_") for f in files), files
    for f in files:
        assert os.path.getsize(out / f) > 1000
