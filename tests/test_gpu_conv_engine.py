"""PPO.update of the CNN height-map encoder module on the HIP update engine (GO1_PPO_ENCODER_ENGINE=1 /
rollout_cnn.ENGINE_DEFAULT["cnn"]), end to end on the MI355X: one update against the float64 restatement
(tests/ppo_ref_conv.py) on the same rows and permutation at the bounds tests/test_gpu_encoder_engine.py holds the MLP
engine to, graph replay = eager, the split into graph segments = one graph, one learning iteration on the HIP env
with the fused rollout re-packed, a torch update after an engine update, the optimizer state round trip, and the
switch off = the torch path as before."""
import types

import numpy as np
import pytest
import torch

from legged_tracking_amd import ppo_engine as PE, rollout as R, rollout_cnn as RC
from tests import ppo_ref_conv as ref
from tests.test_gpu_encoder import S, _close, _env_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T, EPOCHS, MINI = 32, 4, 2, 4  # tests/cnn_cases.py's update: 8 Adam steps of both optimizers, mb = 32
E, PRIV, NA = 128, 2, 12
NUM_OBS = S + 3782
SWITCHES = ("GO1_PPO_ENGINE", "GO1_PPO_GRAPH", "GO1_PPO_SPLIT")


def _module():
    torch.manual_seed(7)
    args = type("A", (RC.AC_Args,), dict(use_cnn=True, height_map_shape=(2, 61, 31), cnn_num_embedding=E))
    return RC.ActorCritic(NUM_OBS, PRIV, NUM_OBS, NA, ac_args=args)


def _storage_values():
    """The seeded storage (T, N, ...) of one update: histories of N(0, 1) scalars and U(-5, 5) maps; actions, values
    and the old distribution from the f64 forward of the fresh module, so that the ratios and the KL are a rollout's."""
    g = torch.Generator().manual_seed(11)
    rows = T * N
    hist = torch.randn(rows, NUM_OBS, generator=g)
    hist[:, S:] = torch.rand(rows, 3782, generator=g) * 10.0 - 5.0
    priv = 0.5 * torch.randn(rows, PRIV, generator=g)
    ac64 = ref.double_copy(_module())
    with torch.no_grad():
        x = ac64.process_obs_history(hist.double())
        mu = ac64.actor_body(torch.cat((x, ac64.adaptation_module(x)), -1))
        v = ac64.critic_body(torch.cat((x, priv.double()), -1))
        std = ac64.std.detach()
        z = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
        actions = (mu + std * z(rows, NA)).float()
        logp = torch.distributions.Normal(mu, std).log_prob(actions.double()).sum(-1, keepdim=True)
        out = dict(observation_histories=hist, privileged_observations=priv, actions=actions,
                   actions_log_prob=logp + 0.1 * z(rows, 1), mu=mu + 0.05 * std * z(rows, NA),
                   sigma=(std * 1.01).expand(rows, NA), values=v + 0.1 * z(rows, 1), returns=v + z(rows, 1),
                   advantages=z(rows, 1))
    return {k: t.float().reshape(T, N, -1).contiguous() for k, t in out.items()}


def _update(mp, env):
    """One rollout.PPO.update of a fresh module on the seeded storage with the seeded permutation."""
    for k in SWITCHES + ("GO1_PPO_ENCODER_ENGINE",):
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    mp.setattr(R.PPO_Args, "num_learning_epochs", EPOCHS)
    mp.setattr(R.PPO_Args, "num_mini_batches", MINI)
    alg = R.PPO(_module(), device=DEV, kernels=R.HipRolloutKernels())
    alg.init_storage(N, T, [NUM_OBS], [PRIV], [NUM_OBS], [NA])
    vals = _storage_values()
    for k, t in vals.items():
        getattr(alg.storage, k).copy_(t)
    alg.storage.observations.copy_(vals["observation_histories"])
    alg.storage.step = T
    perm = torch.randperm(N * T, generator=torch.Generator().manual_seed(3))
    real = torch.randperm
    torch.randperm = lambda *a, **k: perm.to(k.get("device") or "cpu")
    try:
        losses = alg.update()
    finally:
        torch.randperm = real
    torch.cuda.synchronize()
    return alg, losses, perm, {k: v.detach().clone() for k, v in alg.actor_critic.state_dict().items()}


@pytest.fixture(scope="module")
def graphed():
    mp = pytest.MonkeyPatch()
    try:
        return _update(mp, {"GO1_PPO_ENCODER_ENGINE": "1"})
    finally:
        mp.undo()


def _max_dw(sd, sd64, atol_w=None, atol_max=None):
    diffs = torch.cat([(sd[k].double().cpu() - sd64[k].cpu()).abs().reshape(-1) for k in sd64])
    if atol_w is not None:
        assert float(diffs.max()) <= atol_max, float(diffs.max())
        assert float(np.percentile(diffs.numpy(), 99.99)) <= atol_w
    return float(diffs.max())


def test_update_on_the_engine_matches_the_f64_restatement(graphed, monkeypatch):
    alg, losses, perm, sd = graphed
    assert alg._engine is not None and alg._engine.enc_dims["enc_mode"] == 3 and alg._engine.graphs is not None
    assert alg._graph is None and not alg._graph_on  # the torch path's graph is not involved
    ac64 = ref.double_copy(_module().to(DEV))
    st = types.SimpleNamespace(**{k: v.to(DEV) for k, v in _storage_values().items()})
    rows = ref.rows_of(st, torch.float64)
    before = {k: v.detach().clone() for k, v in ac64.state_dict().items()}
    want, lr = ref.update(ac64, rows, perm.to(DEV), MINI, EPOCHS, ref.hyper_from_args(R.PPO_Args),
                          float(R.PPO_Args.learning_rate))
    np.testing.assert_allclose(np.array([float(x) for x in losses]), np.array(want), rtol=1e-3, atol=1e-7)
    assert abs(alg.learning_rate - lr) <= 1e-14 * lr
    sd64 = {k: v.detach() for k, v in ac64.state_dict().items()}
    assert all(k == "std" or not torch.equal(before[k], sd64[k]) for k in sd64)
    w = _max_dw(sd, sd64, atol_w=1e-4, atol_max=3e-3)
    # the torch f32 GPU path (eager autograd, MIOpen) on the same data, for scale
    t_alg, t_losses, _, t_sd = _update(monkeypatch, {"GO1_PPO_ENCODER_ENGINE": "0"})
    assert t_alg._engine is None
    print(f"\nPPO.update of the CNN module vs the f64 restatement: max |dw| engine {w:.2e}, torch f32 GPU path "
          f"{_max_dw(t_sd, sd64):.2e}")


@pytest.mark.parametrize("env", [{"GO1_PPO_GRAPH": "0"}, {"GO1_PPO_SPLIT": "1"}], ids=["eager", "split"])
def test_eager_and_split_updates_are_the_graphed_update_to_the_bit(graphed, monkeypatch, env):
    alg, losses, _, sd = _update(monkeypatch, dict(env, GO1_PPO_ENCODER_ENGINE="1"))
    eng = alg._engine
    assert eng is not None
    if "GO1_PPO_GRAPH" in env:
        assert eng.graphs is None
    else:
        assert len(eng.graphs) == 3
    for k, v in graphed[3].items():
        assert torch.equal(sd[k], v), k
    assert tuple(losses) == tuple(graphed[1]) and alg.learning_rate == graphed[0].learning_rate


def test_switch_off_is_the_torch_path(monkeypatch):
    alg, losses, _, _ = _update(monkeypatch, {})  # the default: off
    assert RC.ENGINE_DEFAULT["cnn"] is False
    assert alg._engine is None and alg._graph is None and not alg._graph_on
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    assert alg._engine_on()
    monkeypatch.setenv("GO1_PPO_ENGINE", "0")  # GO1_PPO_ENGINE=0 still wins
    assert not alg._engine_on()


def test_learning_iteration_torch_update_after_it_and_optimizer_state(monkeypatch, tmp_path):
    """rollout_cnn.Runner.learn(1) on the HIP env (64 envs, 4 steps, 2 mini-batches, the 61 x 31 scan, use_cnn) with
    the update on the engine; then an update with the switch off (release_optimizer_state over the wider slice);
    then the optimizer state_dict / load_state_dict round trip back on the engine."""
    from legged_tracking_amd import env as EV
    mp = monkeypatch
    for k in SWITCHES:
        mp.delenv(k, raising=False)
    mp.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    torch.manual_seed(0)
    cfg, shape = _env_cfg(64, True)
    assert shape == (2, 61, 31)
    mp.setattr(RC.AC_Args, "height_map_shape", shape)
    mp.setattr(RC.AC_Args, "use_cnn", True)
    mp.setitem(RC.FUSED_DEFAULT, "cnn", True)
    mp.setattr(R.RunnerArgs, "num_steps_per_env", 4)
    mp.setattr(R.PPO_Args, "num_learning_epochs", 1)
    mp.setattr(R.PPO_Args, "num_mini_batches", 2)
    env = EV.HistoryWrapper(EV.TrajectoryTrackingEnv(sim_device=DEV, cfg=cfg, seed=4))
    runner = RC.Runner(env, device=DEV, save_dir=str(tmp_path))
    alg = runner.alg
    ac = alg.actor_critic
    assert isinstance(ac, RC.ActorCritic) and isinstance(alg.fused, RC.FusedEncoderPolicy)
    assert PE.conv_encoder_supported(ac) and alg._engine_on()
    before = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    losses, update = [], alg.update

    def capture():
        losses.append(update())
        return losses[-1]

    alg.update = capture
    runner.learn(1)
    torch.cuda.synchronize()
    assert alg._engine is not None and alg._engine.enc_dims["enc_mode"] == 3
    assert len(losses) == 1 and np.isfinite(np.array([float(x) for x in losses[0]])).all(), losses
    after = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    for k in ("height_map_encoder.model.0.weight", "height_map_encoder.model.3.weight",
              "height_map_encoder.model.7.weight", "adaptation_module.0.weight", "actor_body.0.weight",
              "critic_body.0.weight", "std"):
        assert not torch.equal(before[k], after[k]), k

    def fused_matches_module():
        hist, priv = alg.storage.observation_histories[-1], alg.storage.privileged_observations[-1]
        mean, value, latent = alg.fused.forward(hist, priv)
        with torch.no_grad():
            pt = ac.process_obs_history(hist)
            lt = ac.adaptation_module(pt)
            mt = ac.actor_body(torch.cat((pt, lt), -1))
            vt = ac.critic_body(torch.cat((pt, priv), -1))
        for got, want in ((latent, lt), (mean, mt), (value, vt)):  # the updated weights: the re-pack happened
            _close(got, want, tol=1e-4)
        assert int(alg.fused.overflow.item()) == 0

    fused_matches_module()
    st = alg.storage
    st.step = st.num_transitions_per_env
    mp.setenv("GO1_PPO_ENCODER_ENGINE", "0")
    out = update()
    torch.cuda.synchronize()
    assert np.isfinite(np.array([float(x) for x in out])).all(), out
    assert all(bool(torch.isfinite(v).all()) for v in ac.state_dict().values())
    mp.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    sd0, sd1 = alg.optimizer.state_dict(), alg.adaptation_module_optimizer.state_dict()
    alg.optimizer.load_state_dict(sd0)
    alg.adaptation_module_optimizer.load_state_dict(sd1)
    st.step = st.num_transitions_per_env
    eng = alg._engine
    out = update()
    torch.cuda.synchronize()
    assert alg._engine is eng and np.isfinite(np.array([float(x) for x in out])).all(), out
    assert eng.steps.tolist() == [6.0, 6.0]  # one learn() of two mini-batches, the torch update's two, these two
    sd = alg.adaptation_module_optimizer.state_dict()["state"]
    assert len(sd) == len(PE.CONV_PARAM_NAMES) + PE.N_ADAPT_TENSORS  # encoder + adaptation module
    assert len(alg.optimizer.state_dict()["state"]) == len(eng.names)
    for s in alg.optimizer.state_dict()["state"].values():
        assert float(s["step"]) == 6.0 and bool(torch.isfinite(s["exp_avg"]).all())
    fused_matches_module()
    env.close()
