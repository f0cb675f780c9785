"""play and evaluate on the MI355X for the checkpoints of both learners: the env step, the fused inference kernels
(go1_heightmap_encode + go1_policy_forward in student / teacher mode) and the episode-log listener end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from legged_tracking_amd import checkpoint as CK, config as CF, env as E, evaluate as EV, play as PL, rollout as R
from legged_tracking_amd import rollout_cnn as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 41


def test_play_replays_a_checkpoint_of_the_default_learner(tmp_path, monkeypatch):
    """rollout_cnn.Runner's checkpoint (MLP encoder on the full 21 x 11 map, 503-wide frames) through the CLI."""
    cfg = CF.readme_config(n_envs=16, terrain="single_path", rows=2, cols=2)
    cfg.terrain.measure_front_half = False
    cfg.env.num_observations = cfg.env.num_scalar_observations = 503
    monkeypatch.setattr(RC.AC_Args, "height_map_shape", (2, 21, 11))
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=DEV, headless=True, cfg=cfg, seed=3))
    runner = RC.Runner(env, device=DEV, save_dir=str(tmp_path / "ckpt"))
    assert isinstance(runner.alg.actor_critic, RC.ActorCritic) and env.num_obs == 503
    runner.save()
    env.close()
    assert sorted(os.listdir(tmp_path / "ckpt")) == ["ac_weights.pt", "adaptation_module_latest.jit",
                                                     "body_latest.jit", "parameters.pkl"]
    out = tmp_path / "videos"
    r = subprocess.run([sys.executable, "-m", "legged_tracking_amd.play", str(tmp_path / "ckpt"), "--out", str(out),
                        "--envs", "4", "--width", "64", "--height", "48", "--steps", "20"], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(os.listdir(out))
    assert len(files) == 4 and all(f.startswith("env_") for f in files), files
    for f in files:
        assert os.path.getsize(out / f) > 1000


def test_play_replays_a_cnn_checkpoint_without_parameters_pkl(tmp_path):
    """A CNN checkpoint alone: the 61 x 31 scan over the README extents, one frame of history."""
    torch.manual_seed(0)
    base = CF.readme_config(n_envs=16)
    args = type("A", (RC.AC_Args,), dict(use_cnn=True, height_map_shape=(2, 61, 31), cnn_num_embedding=128))
    num_obs = S + 2 * 61 * 31
    ac = RC.ActorCritic(num_obs, base.env.num_privileged_obs, num_obs, 12, ac_args=args)
    with torch.no_grad():
        ac.std.fill_(0.5)
    os.makedirs(tmp_path / "ckpt")
    torch.save(ac.state_dict(), tmp_path / "ckpt" / "ac_weights.pt")

    def run(name, **kw):
        files = PL.play(str(tmp_path / "ckpt"), str(tmp_path / name), steps=10, envs=16, width=64, height=48,
                        device=DEV, **kw)
        assert sorted(os.path.basename(f) for f in files) == sorted(os.listdir(tmp_path / name)) and len(files) == 16
        return [open(f, "rb").read() for f in sorted(files)]

    mean = run("mean", deterministic=True)
    a, b, c = run("a", seed=5), run("b", seed=5), run("c", seed=6)
    assert a == b  # the same seed: identical frames
    assert a != mean and a != c


@pytest.fixture(scope="module")
def old_checkpoint(tmp_path_factory):
    """A random-weight ppo_cse checkpoint with its parameters.pkl: episodes of at most 49 steps."""
    d = tmp_path_factory.mktemp("old")
    cfg = CF.readme_config(n_envs=64, terrain="single_path", rows=2, cols=2)
    cfg.env.episode_length_s = 0.96
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=DEV, headless=True, cfg=cfg, seed=3))
    torch.manual_seed(1)
    R.Runner(env, device=DEV, save_dir=str(d)).save()
    env.close()
    return str(d)


def _rates(out):
    return {k: v for k, v in out.items() if k != "env_steps_per_s"}


def test_evaluate_counts_each_envs_first_two_episodes(old_checkpoint, tmp_path, capsys):
    kw = dict(envs=64, episodes_per_env=2, rows=2, cols=2, seed=7, device=DEV)
    out = EV.evaluate(old_checkpoint, **kw)
    assert out["episodes"] == 128 and out["steps"] <= 2 * 50 + 64
    assert out["success_rate"] + out["timeout_rate"] + out["fall_rate"] == pytest.approx(1.0, abs=1e-9)
    assert sum(t["episodes"] for t in out["per_tile"].values()) == 128
    assert 1 <= out["mean_episode_length"] <= 49 and out["env_steps_per_s"] > 0
    assert out["collision_free_rate"] is not None and "mean_rew_total" in out
    # the CLI with the same seed: the same dict, printed as one JSON line and written to --json
    f = tmp_path / "eval.json"
    EV.main([old_checkpoint, "--envs", "64", "--episodes-per-env", "2", "--rows", "2", "--cols", "2", "--seed", "7",
             "--json", str(f)])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    again = json.loads(lines[0])
    assert again == json.load(open(f))
    assert _rates(again) == _rates(json.loads(json.dumps(out)))
    teacher = EV.evaluate(old_checkpoint, teacher=True, **kw)
    assert teacher["episodes"] == 128 and _rates(teacher) != _rates(out)


def test_evaluate_refuses_a_velocity_checkpoint(tmp_path):
    from legged_tracking_amd import velocity_config as VC
    CK.save_parameters(VC.train_velocity_config(n_envs=16), str(tmp_path))
    torch.save(R.ActorCritic(70, 2, 2100, 12).state_dict(), tmp_path / "ac_weights.pt")
    with pytest.raises(ValueError, match="velocity env's episode log has no `reached`"):
        EV.evaluate(str(tmp_path), envs=16, device=DEV)
