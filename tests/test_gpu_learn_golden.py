"""Two learning iterations end to end against a recording of themselves (tests/golden/learn_refactor/learn_64.npz).

The fixture was recorded with this file's record() before the bindings of rollout.py / ppo_engine.py moved to
learn_abi.py and the rejected kernel variants left rollout.hip / ppo_update.hip: Runner over
HistoryWrapper(TrajectoryTrackingEnv), README configuration on a 2 x 2 single_path terrain, 64 envs, 24 steps per
env (4 mini-batches of 384 rows, 5 epochs), torch seed 0, env seed 4, the default update engine and its graph.
From iteration 1's storage: actions, mu, sigma, actions_log_prob, values (the fused policy kernel's outputs, which
depend on the initial weights only), returns and advantages; after iteration 2: every state_dict tensor, the state
of both optimizers and the learning rate.

Recorded twice; every array was bitwise equal between the two recordings (the policy kernel, the GAE scan and the
update engine reduce in a fixed order), so every array is compared bitwise here and no tolerance is in use.  The
comparison still honours a "tol/<name>" entry (four times the largest absolute difference between the two
recordings) should a later re-recording find an array that does not reproduce.  Tensors of more than DIGEST_OVER
elements (the large weight matrices and their Adam moments, 9 MB together) are kept as the SHA-256 of their bytes.
"""
import hashlib
import os
import tempfile

import numpy as np
import pytest
import torch

from legged_tracking_amd import config as CF, env as E, rollout as R

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "learn_refactor", "learn_64.npz")
N, STEPS, DIGEST_OVER = 64, 24, 4096
POLICY_OUTPUTS = ("actions", "mu", "sigma", "actions_log_prob", "values")


def record(device="cuda:0"):
    assert (R.RunnerArgs.num_steps_per_env, R.PPO_Args.num_learning_epochs, R.PPO_Args.num_mini_batches) == \
        (STEPS, 5, 4)
    torch.manual_seed(0)
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=2, cols=2)
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=device, cfg=cfg, seed=4, rank=0, world_size=1))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        runner = R.Runner(env, device=device, save_dir=tmp)
        alg = runner.alg
        assert alg.fused is not None and alg._engine_on() and alg._graph_on
        runner.learn(1)
        st = alg.storage
        for k in POLICY_OUTPUTS + ("returns", "advantages"):
            out[f"storage/{k}"] = getattr(st, k).cpu().numpy()
        runner.learn(1)
    torch.cuda.synchronize()
    for k, v in alg.actor_critic.state_dict().items():
        out[f"state_dict/{k}"] = v.cpu().numpy()
    for name, opt in (("optimizer", alg.optimizer), ("adaptation_module_optimizer", alg.adaptation_module_optimizer)):
        for i, s in sorted(opt.state_dict()["state"].items()):
            for k, v in s.items():
                out[f"{name}/{i}/{k}"] = torch.as_tensor(v).cpu().numpy()
    out["learning_rate"] = np.float64(alg.learning_rate)
    env.close()
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def pack(rec):
    """What the fixture holds of a recording: the arrays, the large ones as the SHA-256 of their bytes."""
    return {k: np.frombuffer(hashlib.sha256(v.tobytes()).digest(), np.uint8) if v.size > DIGEST_OVER else v
            for k, v in rec.items()}


def test_two_learning_iterations_replay_recording():
    want = np.load(FIXTURE)
    rec = record()
    got = pack(rec)
    names = [k for k in want.files if not k.startswith("tol/")]
    assert set(names) == set(got) and len(names) >= 7 + 23 + 3 * 23 + 3 * 6 + 1
    for k in POLICY_OUTPUTS:
        assert f"tol/storage/{k}" not in want.files, k
    for k in names:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if f"tol/{k}" in want.files:
            assert rec[k].size <= DIGEST_OVER, k
            err = np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)).max()
            print(k, "max abs difference", err, "bound", float(want[f"tol/{k}"]))
            assert err <= float(want[f"tol/{k}"]), k
        else:
            assert got[k].tobytes() == want[k].tobytes(), k
    assert np.isfinite(rec["storage/returns"]).all() and rec["storage/sigma"].min() > 0
    steps = [v.item() for k, v in rec.items() if k.endswith("/step")]
    assert len(steps) == 23 + 6 and set(steps) == {40.0}  # 2 iterations x 5 epochs x 4 mini-batches, both optimizers


if __name__ == "__main__":  # python -m tests.test_gpu_learn_golden OUT.npz: record twice, write the fixture
    import sys
    a, b = record(), record()
    fix = pack(a)
    for k in a:
        if a[k].tobytes() != b[k].tobytes():
            d = float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
            print("differs between the two recordings:", k, a[k].shape, d)
            assert k.split("/")[-1] not in POLICY_OUTPUTS or not k.startswith("storage/"), k
            assert a[k].size <= DIGEST_OVER, f"{k}: too large to keep by value"
            fix[f"tol/{k}"] = np.float64(4.0 * d)
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    np.savez_compressed(sys.argv[1], **fix)
    print("recorded", len(a), "arrays,", sum(k.startswith("tol/") for k in fix), "with a tolerance")
