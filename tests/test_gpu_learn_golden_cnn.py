"""Two learning iterations of the height-map encoder learner against a recording of themselves
(tests/golden/learner_split/learn_cnn.npz), tests/test_gpu_learn_golden.py's protocol and file shape.

The fixture was recorded with this file's __main__ before rollout.py / rollout_cnn.py were split into one module per
concern: rollout_cnn.Runner over HistoryWrapper(TrajectoryTrackingEnv), the two cases of
test_gpu_encoder.py::test_learning_iteration_end_to_end with its _env_cfg (MLP encoder: 64 envs, the 21 x 11 map, the
default history; CNN: 32 envs, the 61 x 31 map, one frame), 4 steps per env, one epoch of two mini-batches,
FUSED_DEFAULT[mode] on, torch seed 0, env seed 4, Runner.learn(1) twice.  Each case under the default switches (the
torch eager update, key "torch") and under GO1_PPO_ENCODER_ENGINE=1 (the HIP update engine and its graph, key
"engine"): four recordings, keyed "<mode>/<update>/...".  Of each: iteration 1's storage arrays (actions, mu, sigma,
actions_log_prob, values: the fused kernels' outputs on the initial weights; returns, advantages), and after
iteration 2 every state_dict tensor, the state of both optimizers and the learning rate.

Every case was recorded RECORDINGS times; the fixture holds the first recording.  An array equal in all of them is
compared bitwise, kept by value or, over DIGEST_OVER elements, as the SHA-256 of its bytes.  One that differed
carries a "tol/<name>" entry of four times the largest absolute difference between any two of the recordings and is
kept by value; over DIGEST_OVER elements, as a strided sample of at most SAMPLE of them (sample()), on which its
tolerance was measured.  No storage array may carry a tolerance, and none does.

mlp/torch, mlp/engine, cnn/engine and cnn/torch's storage arrays are bitwise.  The torch update of the CNN module
does not reproduce from run to run (MIOpen's convolution backward), which two recordings do not bound (an array of
two elements can agree in both and differ by an ulp in the next run): hence RECORDINGS.  109 of cnn/torch's 153
other arrays carry a tolerance, 3.3e-17 x 4 (a second moment) .. 1.0e-7 x 4 (a first moment), 38 of them as samples
(the 10 weight tensors over DIGEST_OVER elements, their moments in the optimizer and, for four, the adaptation one's).
Bitwise in that case too, equal in every recording: std, critic_body.6.bias (one element), the step counters and
the learning rate.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from legged_tracking_amd import env as E, rollout as R, rollout_cnn as RC
from tests.test_gpu_encoder import _env_cfg
from tests.test_gpu_learn_golden import DIGEST_OVER, pack

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "learner_split", "learn_cnn.npz")
CASES = (("mlp", 64), ("cnn", 32))
UPDATES = ("torch", "engine")
STORAGE = ("actions", "mu", "sigma", "actions_log_prob", "values", "returns", "advantages")
# state_dict tensors: the encoder's (4 of the two Linear layers, 6 of Conv2d, Conv2d, Linear) + the 23 of the heads;
# the adaptation step reaches the encoder and the adaptation module's 6
N_ENCODER = {"mlp": 4, "cnn": 6}
RECORDINGS, SAMPLE = 8, 1024


def sample(v):
    """At most SAMPLE elements of v at one stride over the whole array: what is kept of an array of more than
    DIGEST_OVER elements that does not reproduce bitwise."""
    return np.ascontiguousarray(v.ravel()[::-(-v.size // SAMPLE)])


@contextlib.contextmanager
def _settings(mode, shape, update):
    saved = [(o, k, getattr(o, k)) for o, k in ((RC.AC_Args, "height_map_shape"), (RC.AC_Args, "use_cnn"),
                                                 (R.RunnerArgs, "num_steps_per_env"),
                                                 (R.PPO_Args, "num_learning_epochs"), (R.PPO_Args, "num_mini_batches"))]
    fused, env = RC.FUSED_DEFAULT[mode], os.environ.pop("GO1_PPO_ENCODER_ENGINE", None)
    RC.AC_Args.height_map_shape, RC.AC_Args.use_cnn = shape, mode == "cnn"
    R.RunnerArgs.num_steps_per_env, R.PPO_Args.num_learning_epochs, R.PPO_Args.num_mini_batches = 4, 1, 2
    RC.FUSED_DEFAULT[mode] = True
    if update == "engine":
        os.environ["GO1_PPO_ENCODER_ENGINE"] = "1"
    try:
        yield
    finally:
        for o, k, v in saved:
            setattr(o, k, v)
        RC.FUSED_DEFAULT[mode] = fused
        os.environ.pop("GO1_PPO_ENCODER_ENGINE", None)
        if env is not None:
            os.environ["GO1_PPO_ENCODER_ENGINE"] = env


def record(mode, n, update, tmp, device="cuda:0"):
    cfg, shape = _env_cfg(n, mode == "cnn")
    out = {}
    with _settings(mode, shape, update):
        torch.manual_seed(0)
        env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=device, cfg=cfg, seed=4))
        runner = RC.Runner(env, device=device, save_dir=tmp)
        alg = runner.alg
        assert isinstance(alg.fused, RC.FusedEncoderPolicy)
        assert alg._engine_on() == (update == "engine") and not alg._graph_on and alg._engine_graph
        runner.learn(1)
        st = alg.storage
        for k in STORAGE:
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
    return {f"{mode}/{update}/{k}": np.ascontiguousarray(v) for k, v in out.items()}


@pytest.mark.parametrize("update", UPDATES)
@pytest.mark.parametrize("mode,n", CASES)
def test_two_encoder_learning_iterations_replay_recording(mode, n, update, tmp_path):
    want = np.load(FIXTURE)
    pre = f"{mode}/{update}/"
    rec = record(mode, n, update, str(tmp_path))
    got = pack(rec)
    got.update({k: sample(v) for k, v in rec.items() if v.size > DIGEST_OVER and f"tol/{k}" in want.files})
    names = [k for k in want.files if k.startswith(pre)]
    params = 23 + N_ENCODER[mode]
    assert set(names) == set(got) and len(names) == 7 + params + 3 * params + 3 * (6 + N_ENCODER[mode]) + 1
    for k in STORAGE:
        assert f"tol/{pre}storage/{k}" not in want.files, k
    missed = []
    for k in names:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if got[k].tobytes() == want[k].tobytes():
            continue
        bound = float(want[f"tol/{k}"]) if f"tol/{k}" in want.files else 0.0  # no entry: bitwise (a digest, if large)
        digest = rec[k].size > DIGEST_OVER and not bound
        err = np.inf if digest else np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)).max()
        print(k, "max abs difference", err, "bound", bound)
        if not err <= bound:
            missed.append(k)
    assert not missed, missed
    assert np.isfinite(rec[pre + "storage/returns"]).all() and rec[pre + "storage/sigma"].min() > 0
    steps = [v.item() for k, v in rec.items() if k.endswith("/step")]
    assert len(steps) == params + 6 + N_ENCODER[mode] and set(steps) == {4.0}  # 2 iterations x 1 epoch x 2 mini-batches


if __name__ == "__main__":  # python -m tests.test_gpu_learn_golden_cnn OUT.npz: record, write the fixture
    import sys
    import tempfile
    recs = [{} for _ in range(RECORDINGS)]
    for rec in recs:
        for mode, n in CASES:
            for update in UPDATES:
                with tempfile.TemporaryDirectory() as tmp:
                    rec.update(record(mode, n, update, tmp))
    a = recs[0]
    fix, bad = pack(a), []
    for k in a:
        if any(r[k].tobytes() != a[k].tobytes() for r in recs[1:]):
            keep = sample if a[k].size > DIGEST_OVER else np.asarray
            kept = np.stack([keep(r[k]).astype(np.float64) for r in recs])
            d = float((kept.max(0) - kept.min(0)).max())  # the largest difference between any two recordings
            print("differs between the recordings:", k, a[k].shape, d)
            if "/storage/" in k:
                bad.append(k)
            fix[k] = keep(a[k])
            fix[f"tol/{k}"] = np.float64(4.0 * d)
    assert not bad, f"storage arrays that do not reproduce: {bad}"
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    np.savez_compressed(sys.argv[1], **fix)
    print("recorded", len(a), "arrays,", sum(k.startswith("tol/") for k in fix), "with a tolerance")
