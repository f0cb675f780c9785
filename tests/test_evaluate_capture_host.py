"""evaluate --capture on the CPU: the join of the tracer's records to the episode-log rows, the labels, the N limit,
the (end push, env) order and the unchanged result without --capture.  The env is the oracle-backed one, the tracer
a test double that restates the push with tests/trace_ref.py from the host state, so the join's own assertion
(full_length == the log row's length for episodes begun by an in-step reset) runs against real episode-log rows."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from legged_tracking_amd import checkpoint as CK, config as CF, env as E, evaluate as EV, play as PL
from legged_tracking_amd import policy_kernels as PK
from tests import trace_ref as TR
from tests.cpu_backend import OracleBackend

N, MAXLEN = 16, 6


class RefTracer:
    """EpisodeTracer's surface over TraceRef."""
    made = []

    def __init__(self, env, depth=None, capacity=64, want=("terminated", "timeout"), eligible=None):
        self.env, self.st = env, env._sim.state
        depth = int(env.max_episode_length) + 1 if depth is None else depth
        bits = sum({"terminated": 1, "timeout": 2}[w] for w in want)
        self.ref = TR.TraceRef(env.num_envs, depth, capacity, self.st["trajectory"].shape[1], bits)
        self.ref.traj_start[:] = TR.bits(self.st["trajectory"].numpy())
        self.capacity, self.want, self.rendered = capacity, want, []
        RefTracer.made.append(self)

    def push(self, reset, time_out):
        st = self.st
        self.ref.push(st["root"].numpy(), st["dof_pos"].numpy(), reset.numpy(), time_out.numpy(),
                      wp_index=st["curr_pose_index"].numpy()[:, 0], traj=st["trajectory"].numpy())

    def mark_reset(self, env_ids):
        self.ref.mark_reset(torch.as_tensor(env_ids).tolist(), traj=self.st["trajectory"].numpy())

    def counts(self):
        return self.ref.counts()

    def episodes(self):
        meta, rows, traj = self.ref.sorted_captures()
        return [SimpleNamespace(env=int(m[0]), ordinal=int(m[1]), end_push=int(m[2]), kept=int(m[3]),
                                full_length=int(m[4]), cause=int(m[5])) for m in meta]

    def render_episode(self, i, width, height, mode=None, flags=None):
        self.rendered.append(i)
        return np.zeros((self.episodes()[i].kept, height, width, 4), np.uint8)


@pytest.fixture()
def checkpoint(tmp_path, monkeypatch):
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=2, cols=2)
    cfg.env.episode_length_s = (MAXLEN - 0.5) * CF.derived(cfg)["dt"]
    CK.save_parameters(cfg, str(tmp_path))
    (tmp_path / "ac_weights.pt").write_bytes(b"")
    monkeypatch.setattr(EV, "TrajectoryTrackingEnv", lambda sim_device, headless, cfg, seed: E.TrajectoryTrackingEnv(
        sim_device="cpu", headless=True, cfg=cfg, seed=seed, backend=OracleBackend))
    monkeypatch.setattr(PL, "load_policy_module", lambda logdir, cfg, env: None)
    monkeypatch.setattr(PK, "fused_inference", lambda ac, teacher, sample: lambda obs: torch.zeros(N, 12))
    RefTracer.made.clear()
    return str(tmp_path)


def _run(checkpoint, **kw):
    return EV.evaluate(checkpoint, envs=N, episodes_per_env=3, rows=2, cols=2, seed=5, device="cpu",
                       tracer_factory=RefTracer, **kw)


def test_capture_joins_labels_limits_and_leaves_the_rest_unchanged(checkpoint, tmp_path):
    plain = _run(checkpoint)
    assert "captured" not in plain and not RefTracer.made  # no tracer was built
    out = _run(checkpoint, capture=5, capture_out=str(tmp_path / "cap"), capture_what=("timeout",),
               capture_size=(32, 24))
    drop = ("env_steps_per_s", "captured")
    assert {k: v for k, v in out.items() if k not in drop} == {k: v for k, v in plain.items() if k not in drop}
    assert set(out) == set(plain) | {"captured"} and plain["timeout_rate"] > 0
    tracer, = RefTracer.made
    assert tracer.capacity == 20 and tuple(tracer.want) == ("timeout",) and tracer.env._tracer is None  # detached
    cap = out["captured"]
    assert len(cap) == 5 and [c["label"] for c in cap] == ["timeout"] * 5
    eps = tracer.episodes()
    assert [(e.end_push, e.env) for e in eps] == sorted((e.end_push, e.env) for e in eps)
    # zero actions on short episodes: every time-out capture is a counted timeout, so the first five that have a
    # row are taken (an episode that ended in the tracer's first push has none)
    first = [i for i, e in enumerate(eps) if e.kept > 0][:5]
    assert [(c["env"], c["rows_kept"]) for c in cap] == [(eps[i].env, eps[i].kept) for i in first]
    assert tracer.rendered == first
    for k, c in enumerate(cap):
        assert c["file"] == str(tmp_path / "cap" / f"episode_{k}_env{c['env']}_timeout.gif") and os.path.exists(c["file"])
        assert c["length"] == MAXLEN + 1 and c["tile"] == int(tracer.env.terrain.env_tile[c["env"]])
    # 20 slots over 16 envs: the join's length assertion ran on episodes begun by an in-step reset
    assert any(e.ordinal > 0 for e in eps)


def test_labels_follow_the_log_rows_not_the_cause():
    """Hand-made rows: env 0's episodes are success (a termination on the device), fall, timeout; env 1's first
    was finished before the tracer was attached (base 1)."""
    ns = 2
    rows = np.array([[0, 0, 4, 1, 0.1], [0, 0, 3, 0, 2.0], [0, 0, 7, 0, 1.0], [0, 0, 2, 0, 1.0], [0, 0, 5, 0, 1.0]],
                    np.float32)
    ids = np.array([0, 1, 0, 0, 1])
    rec = lambda env, o, push, full: SimpleNamespace(env=env, ordinal=o, end_push=push, full_length=full, kept=full)  # noqa: E731
    eps = [rec(0, 0, 4, 99), rec(1, 0, 5, 5), rec(0, 1, 11, 7), rec(0, 2, 13, 2), rec(1, 1, 20, 4), rec(2, 0, 21, 1)]
    got = EV.label_captures(eps, rows, ids, np.array([0, 1]), ns, 6)
    # env 1's ordinal 1 is its third episode (not counted), env 2 is no train env: both are left out
    assert [(ep.env, ep.ordinal, label, length) for ep, label, length in got] == [
        (0, 0, "success", 4), (1, 0, "fall", 5), (0, 1, "timeout", 7), (0, 2, "fall", 2)]
    with pytest.raises(AssertionError):  # an episode begun by an in-step reset whose pushes are not its steps
        EV.label_captures([rec(0, 1, 11, 6)], rows, ids, np.array([0, 1]), ns, 6)


def test_capture_what_is_checked(checkpoint):
    with pytest.raises(ValueError, match="capture_what"):
        _run(checkpoint, capture=1, capture_what=("success",))
