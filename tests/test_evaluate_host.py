"""Host side of evaluate / play on the CPU: the per-env episode counting rule through EpisodeLogRing.listener (a
scripted fake env and the oracle-backed env), the parameters.pkl that Runner.save() writes, and
rollout.fused_inference's fallback to the module's own methods."""
from collections import defaultdict, deque

import numpy as np
import pytest
import torch

from legged_tracking_amd import checkpoint as CK, config as CF, env as E, evaluate as EV, play as PL, rollout as R
from tests.cpu_backend import OracleBackend
from tests.rollout_ref import TorchRolloutKernels

NAMES = ["collision", "tracking"]


class ScriptedEnv:
    """No kernels: env e plays script[e] = [(length, reached, collision, tracking, goal_distance), ...] (the last
    entry repeats), logging each finished episode into a real EpisodeLogRing as the step kernel would."""

    def __init__(self, script, max_episode_length, env_tile):
        self.script = script
        self.num_envs = self.num_train_envs = len(script)
        self.reward_names = list(NAMES)
        self.sum_keys = tuple(NAMES) + ("total", "total_pos", "total_neg")
        self.max_episode_length = max_episode_length
        self.terrain = type("T", (), {"env_tile": np.asarray(env_tile)})
        self._train_ep, self._timeouts = defaultdict(lambda: deque([], 4000)), deque([], 4000)
        self._elog = E.EpisodeLogRing(self, self.num_envs, torch.device("cpu"))
        self.episode = [0] * self.num_envs
        self.age = [0] * self.num_envs

    def _obs(self):
        return {"obs": torch.zeros(self.num_envs, 3), "obs_history": torch.zeros(self.num_envs, 3)}

    def reset(self):
        return self._obs()

    def step(self, actions):
        slot = self._elog.next_slot()
        slot.zero_()
        for e, eps in enumerate(self.script):
            self.age[e] += 1
            length, reached, col, track, dist = eps[min(self.episode[e], len(eps) - 1)]
            if self.age[e] == length:
                slot[e] = torch.tensor([col, track, col + track, track, col, length, reached, dist])
                self.episode[e] += 1
                self.age[e] = 0
        self._elog.advance()
        return self._obs(), None, None, None


SCRIPT = [
    [(2, 0, -1.0, 0.5, 3.0), (2, 1, 0.0, 1.0, 0.1), (2, 1, 0.0, 9.0, 0.0)],     # env 0: five episodes by step 10
    [(5, 1, -0.5, 2.0, 0.2), (5, 0, 0.0, 1.5, 1.0), (5, 1, 0.0, 9.0, 0.0)],
    [(11, 0, 0.0, 4.0, 2.0), (4, 1, 0.0, 3.0, 0.05), (4, 1, 0.0, 9.0, 0.0)],    # env 2: its first at step 11
]


def test_each_envs_first_k_episodes_are_counted():
    env = ScriptedEnv(SCRIPT, max_episode_length=10, env_tile=[0, 0, 1])
    seen = []
    rows, ids, steps, _ = EV.run_episodes(env, lambda ob: (seen.append(1), torch.zeros(3, 12))[1], 2)
    assert env.episode[0] >= 5 and steps == len(seen) >= 15
    assert rows.shape == (6, 8) and sorted(ids.tolist()) == [0, 0, 1, 1, 2, 2]
    for e in range(3):  # each env's first two, in order
        np.testing.assert_array_equal(rows[ids == e][:, 5:],
                                      np.array([[s[0], s[1], s[4]] for s in SCRIPT[e][:2]], np.float32))
    out = EV.summarize(rows, ids, env.sum_keys, env.max_episode_length, env.terrain.env_tile)
    want = {
        "episodes": 6, "success_rate": 3 / 6, "timeout_rate": 1 / 6, "fall_rate": 2 / 6,
        "collision_free_rate": 4 / 6, "collision_free_success_rate": 2 / 6,
        "mean_episode_length": 29 / 6, "mean_goal_distance": 6.35 / 6,
        "mean_rew_collision": -1.5 / 6, "mean_rew_tracking": 12 / 6, "mean_rew_total": 10.5 / 6,
        "mean_rew_total_pos": 12 / 6, "mean_rew_total_neg": -1.5 / 6,
    }
    assert set(out) == set(want) | {"per_tile"}
    for k, v in want.items():
        assert out[k] == pytest.approx(v, rel=1e-6), k
    assert out["success_rate"] + out["timeout_rate"] + out["fall_rate"] == pytest.approx(1.0, abs=1e-12)
    assert out["per_tile"] == {"0": {"episodes": 4, "success_rate": 0.5}, "1": {"episodes": 2, "success_rate": 0.5}}
    assert env._elog.listener is None  # taken off again


def test_no_collision_slot_reports_null():
    rows = np.array([[1.0, 1.0, 1.0, 0.0, 3.0, 1.0, 0.1]], np.float32)
    out = EV.summarize(rows, np.array([0]), ("tracking", "total", "total_pos", "total_neg"), 10, [0])
    assert out["collision_free_rate"] is None and out["collision_free_success_rate"] is None


def test_the_4000_row_cap_loses_no_episode():
    """5,000 episodes over 8 envs, K = 625: the deques keep 4,000 rows, the listener's count is complete."""
    env = ScriptedEnv([[(1, e % 2, 0.0, float(e), 0.5)] for e in range(8)], max_episode_length=10, env_tile=[0] * 8)
    rows, ids, steps, _ = EV.run_episodes(env, lambda ob: torch.zeros(8, 12), 625)
    assert rows.shape[0] == 5000 and np.bincount(ids).tolist() == [625] * 8
    out = EV.summarize(rows, ids, env.sum_keys, 10, env.terrain.env_tile)
    assert out["episodes"] == 5000 and out["success_rate"] == 0.5 and out["mean_rew_tracking"] == pytest.approx(3.5)
    assert len(env._train_ep["episode_length"]) == 4000
    # one processing call with more than 4,000 rows, dense and compact form: the listener is ahead of the cut
    for form in ("dense", "compact"):
        env = ScriptedEnv([[(1, 1, 0.0, 1.0, 0.5)]] * 8, 10, [0] * 8)
        log, got = env._elog, []
        log.listener = lambda r, e, t: got.append((np.array(r), np.array(e), np.array(t)))
        dense = np.zeros((625, 8, log.W), np.float32)
        dense[:, :, 5] = 1.0
        dense[:, :, 1] = np.arange(625 * 8).reshape(625, 8)
        if form == "dense":
            log._process(dense)
        else:
            st, en = np.nonzero(dense[:, :, 5] > 0)
            compact = np.concatenate([dense[st, en], st[:, None], en[:, None]], 1).astype(np.float32)
            log._process_rows(compact[np.random.default_rng(0).permutation(5000)])
        (r, e, t), = got
        assert r.shape == (5000, log.W) and len(env._train_ep["episode_length"]) == 4000
        np.testing.assert_array_equal(r[:, 1], np.arange(5000))  # log order: step, then env
        np.testing.assert_array_equal(e, np.tile(np.arange(8), 625))
        np.testing.assert_array_equal(t, np.repeat(np.arange(625), 8))


def _oracle_env(n=16, seed=2, edit=None):
    cfg = CF.readme_config(n_envs=n, terrain="single_path", rows=2, cols=2)
    cfg.env.episode_length_s = 0.2  # 10 steps
    if edit is not None:
        edit(cfg)
    return E.TrajectoryTrackingEnv(sim_device="cpu", headless=True, cfg=cfg, seed=seed, backend=OracleBackend)


def _drive(env, steps=26):
    rng = np.random.default_rng(0)
    env.reset()
    for _ in range(steps):
        env.step(torch.from_numpy(rng.normal(0, 1, (env.num_envs, 12)).astype(np.float32)))


def test_listener_through_the_oracle_backed_env():
    plain, heard = _oracle_env(), _oracle_env()
    got = []
    heard._elog.listener = lambda r, e, t: got.append((np.array(r), np.array(e), np.array(t)))
    _drive(plain)
    _drive(heard)
    log = heard._elog
    assert 26 <= log.slot < log.R and log.half == 0 and log.done == 0  # one half, nothing processed yet
    dense = log.buf[log.half, :log.slot].numpy().copy()
    ns = len(heard.sum_keys)
    steps, envs = np.nonzero(dense[:, :heard.num_train_envs, ns] > 0)
    assert steps.size >= 2 * heard.num_envs  # every env ran out of time twice
    a, b = dict(plain.extras["train/episode"]), dict(heard.extras["train/episode"])  # drains
    rows = np.concatenate([g[0] for g in got])
    np.testing.assert_array_equal(rows, dense[steps, envs])
    np.testing.assert_array_equal(np.concatenate([g[1] for g in got]), envs)
    np.testing.assert_array_equal(np.concatenate([g[2] for g in got]), steps)
    assert set(a) == set(b) and len(a["episode_length"]) == steps.size
    for k in a:
        np.testing.assert_array_equal(np.array(a[k]), np.array(b[k]), err_msg=k)
    np.testing.assert_array_equal(np.array(plain.extras["timeouts"]), np.array(heard.extras["timeouts"]))


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert isinstance(b, dict) and set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg=path)
    else:
        assert a == b, path


def test_runner_save_writes_parameters_pkl_that_load_cfg_restores(tmp_path):
    def edit(cfg):
        cfg.terrain.terrain_type = "narrow_path"
        cfg.terrain.measured_points_x, cfg.terrain.measured_points_y = np.linspace(-1, 1, 31), np.linspace(-.5, .5, 15)
        cfg.env.num_observations = cfg.env.num_scalar_observations = CF.obs_layout(cfg)["width"]

    env = E.HistoryWrapper(_oracle_env(edit=edit))
    runner = R.Runner(env, device="cpu", kernels=TorchRolloutKernels(), save_dir=str(tmp_path))
    runner.save()
    assert (tmp_path / "parameters.pkl").exists() and (tmp_path / "ac_weights.pt").exists()
    saved = CK.cfg_to_dict(env.cfg)
    default = CK.cfg_to_dict(CF.readme_config(n_envs=16, terrain="single_path", rows=4, cols=4))
    differs = [s for s in saved if not _equal(saved[s], default[s])]
    assert {"env", "terrain"} <= set(differs)
    loaded = CK.cfg_to_dict(PL.load_cfg(str(tmp_path), 16, 64, 48))
    play_sets = {"env": {"recording_width_px", "recording_height_px", "num_envs", "look_from_back", "record_all_envs"},
                 "terrain": {"num_rows", "num_cols"}, "domain_rand": set(PL.DR_OFF)}
    for s in saved:  # every section, those that differ from readme_config among them
        drop = play_sets.get(s, set())
        _same({k: v for k, v in saved[s].items() if k not in drop},
              {k: v for k, v in loaded[s].items() if k not in drop}, s)
    assert loaded["terrain"]["terrain_type"] == "narrow_path" and len(loaded["terrain"]["measured_points_x"]) == 31
    assert loaded["env"]["episode_length_s"] == 0.2 and loaded["env"]["num_observations"] == 41 + 2 * 15 * 15
    assert all(loaded["domain_rand"][k] is False for k in PL.DR_OFF) and loaded["terrain"]["num_rows"] == 4
    # and the module comes back through the checkpoint loader on that Cfg
    ac = CK.load_actor_critic(str(tmp_path), PL.load_cfg(str(tmp_path), 16, 64, 48), env.num_obs,
                              env.num_privileged_obs, env.num_obs_history, env.num_actions, "cpu")
    assert type(ac) is R.ActorCritic


def _equal(a, b):
    try:
        _same(a, b)
    except AssertionError:
        return False
    return True


def test_fused_inference_falls_back_on_a_cpu_module():
    torch.manual_seed(0)
    ac = R.ActorCritic(30, 3, 60, 12)
    ob = {"obs": torch.randn(5, 30), "obs_history": torch.randn(5, 60), "privileged_obs": torch.randn(5, 3)}
    with torch.no_grad():
        student, teacher = R.fused_inference(ac), R.fused_inference(ac, teacher=True)
        assert student.fused is None and teacher.fused is None
        info, info_ref = {}, {}
        assert torch.equal(student(ob, info), ac.act_inference(ob, info_ref))
        assert isinstance(info["latents"], np.ndarray)
        np.testing.assert_array_equal(info["latents"], info_ref["latents"])
        info = {}
        assert torch.equal(teacher(ob, policy_info=info), ac.act_expert(ob))
        assert info["latents"] is ob["privileged_obs"]
        assert torch.equal(student(ob), ac.act_inference(ob))  # no policy_info: nothing to fill
        a, b = R.fused_inference(ac, sample=4)(ob), R.fused_inference(ac, sample=4)(ob)
        assert torch.equal(a, b) and not torch.equal(a, ac.act_inference(ob))
        student.pack()  # nothing to re-pack


def test_evaluate_refuses_a_velocity_checkpoint(tmp_path):
    from legged_tracking_amd import velocity_config as VC
    CK.save_parameters(VC.train_velocity_config(n_envs=16), str(tmp_path))
    torch.save(R.ActorCritic(70, 2, 2100, 12).state_dict(), tmp_path / "ac_weights.pt")
    with pytest.raises(ValueError, match="velocity"):
        EV.evaluate(str(tmp_path), envs=16, device="cpu")
