"""Checkpoint formats (VERDICT r01 missing #5): what rollout.Runner writes is what
the reference's consumers read, and the reference's own trained checkpoint loads here.

Consumers restated (never the reference run on the GPU box):
  * scripts/eval.py:22-35 load_policy (TorchScript): body(cat(obs_history, adaptation_module(obs_history)));
  * scripts/eval.py:38-51 load_policy(old_ppo=True): ActorCritic(num_obs, num_privileged_obs,
    num_obs_history, num_actions).load_state_dict(torch.load(<logdir>/checkpoints/ac_weights.pt)),
    policy = actor_critic.act(obs["obs_history"]).
The reference's trained checkpoint is read from its recorded state dict (tests/golden/trained_policy.npz,
written by tests/golden/make_trained_policy.py with torch.load(weights_only=True); the reference's
TorchScript files execute code and are never loaded)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from legged_tracking_amd import rollout as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _trained_runner(tmp_path, log_wandb=False, save_dir=None):
    from tests.test_rollout import _runner
    torch.manual_seed(0)
    try:
        runner = _runner(tmp_path)
        runner.log_wandb = log_wandb
        runner.save_dir = save_dir
        runner.learn(1)
    finally:
        R.RunnerArgs.num_steps_per_env, R.PPO_Args.num_learning_epochs, R.PPO_Args.num_mini_batches = 24, 5, 4
    return runner


def test_runner_checkpoints_load_through_eval_load_policy(tmp_path):
    runner = _trained_runner(tmp_path, save_dir=str(tmp_path / "logdir" / "checkpoints"))
    logdir = str(tmp_path / "logdir")
    env = runner.env
    obs = {"obs_history": torch.randn(5, env.num_obs_history)}
    ours = runner.alg.actor_critic
    ours.eval()
    # eval.py:22-35 (TorchScript pair)
    body = torch.jit.load(logdir + "/checkpoints/body_latest.jit")
    adapt = torch.jit.load(logdir + "/checkpoints/adaptation_module_latest.jit")
    with torch.no_grad():
        latent = adapt.forward(obs["obs_history"].to("cpu"))
        action = body.forward(torch.cat((obs["obs_history"].to("cpu"), latent), dim=-1))
        np.testing.assert_allclose(action.numpy(), ours.act_student(obs["obs_history"]).numpy(), rtol=1e-5, atol=1e-6)
    # eval.py:38-51 (old_ppo: the ppo_cse ActorCritic and ac_weights.pt)
    ac = R.ActorCritic(env.num_obs, env.num_privileged_obs, env.num_obs_history, env.num_actions)
    weights = torch.load(os.path.join(logdir, "checkpoints", "ac_weights.pt"), map_location="cpu", weights_only=True)
    ac.load_state_dict(state_dict=weights)
    with torch.no_grad():
        np.testing.assert_allclose(ac.act_inference(obs).numpy(), ours.act_inference(obs).numpy(), rtol=1e-6, atol=1e-7)
        a = ac.act(obs["obs_history"])  # the eval policy samples around the same mean
        assert a.shape == (5, env.num_actions) and torch.isfinite(a).all()


def test_runner_saves_under_wandb_run_dir_and_uploads(tmp_path, monkeypatch):
    """log_wandb: checkpoints go to wandb.run.dir/checkpoints and all three files are wandb.save'd
    (ppo_cse/__init__.py:276-297); otherwise last_run/checkpoints."""
    saved = []
    fake = types.ModuleType("wandb")
    fake.run = types.SimpleNamespace(dir=str(tmp_path / "wandb_run"))
    fake.save = saved.append
    fake.log = lambda *a, **k: None
    monkeypatch.setitem(sys.modules, "wandb", fake)
    runner = _trained_runner(tmp_path, log_wandb=True)
    ck = tmp_path / "wandb_run" / "checkpoints"
    assert runner.checkpoint_dir() == str(ck)
    for f in ("ac_weights.pt", "adaptation_module_latest.jit", "body_latest.jit"):
        assert (ck / f).exists()
        assert str(ck / f) in saved
    runner.log_wandb = False
    assert runner.checkpoint_dir() == "last_run/checkpoints"


def test_reference_trained_checkpoint_loads():
    """The reference's trained 261-obs policy (runs/trajectory_tracking/run-20230904_112307-rhi1my71).
    It was trained with 6 privileged observations (adaptation_module.4: 128 -> 6, actor input 267),
    while scripts/train.py now sets num_privileged_obs = 2 (train.py:61).  As in the reference, it
    loads into an ActorCritic built with 6 privileged obs -- whose deployment path act_student /
    act_inference needs only the observation history, which this env produces (261 wide) -- and
    not into the 2-priv ActorCritic train.py builds (size mismatch, the reference fails the same
    way); the teacher / critic path would need the 4 extra privileged observations the trajectory
    env no longer computes."""
    d = np.load(os.path.join(GOLDEN, "trained_policy.npz"))
    sd = {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")}
    assert sd["adaptation_module.4.weight"].shape == (6, 128) and sd["actor_body.0.weight"].shape == (512, 267)
    ac = R.ActorCritic(261, 6, 261, 12)
    ac.load_state_dict(sd)
    hist = torch.randn(8, 261) * 0.3
    with torch.no_grad():
        a = ac.act_inference({"obs_history": hist})
        lat = ac.adaptation_module(hist)
        np.testing.assert_allclose(a.numpy(), ac.actor_body(torch.cat((hist, lat), -1)).numpy(), rtol=1e-6)
    assert torch.isfinite(a).all() and a.shape == (8, 12)
    with pytest.raises(RuntimeError, match="size mismatch"):
        R.ActorCritic(261, 2, 261, 12).load_state_dict(sd)
