"""PPO.update of the height-map encoder module on the HIP update engine (rollout_cnn.ENGINE_DEFAULT /
GO1_PPO_ENCODER_ENGINE), end to end on the MI355X: against the reference's recorded update at the bounds the torch
GPU path is held to (tests/test_gpu_encoder.py), graph replay = eager, the split into graph segments = one graph, one
learning iteration on the HIP env with the fused rollout re-packed, a torch update after an engine update, the
optimizer state round trip, and the switch off = the torch path as before."""
import numpy as np
import pytest
import torch

from legged_tracking_amd import ppo_engine as PE, rollout as R, rollout_cnn as RC
from tests.test_actor_critic_cnn import check_update, ppo_update_from_fixture
from tests.test_gpu_encoder import S, _close, _env_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def engine_on(monkeypatch):
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    monkeypatch.delenv("GO1_PPO_ENGINE", raising=False)
    monkeypatch.delenv("GO1_PPO_GRAPH", raising=False)
    monkeypatch.delenv("GO1_PPO_SPLIT", raising=False)
    return monkeypatch


def _weights(alg):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in alg.actor_critic.state_dict().items()}


@pytest.fixture(scope="module")
def graphed():
    """The fixture's update on the engine, graph-captured (the default): shared by the comparisons below."""
    mp = pytest.MonkeyPatch()
    mp.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    for k in ("GO1_PPO_ENGINE", "GO1_PPO_GRAPH", "GO1_PPO_SPLIT"):
        mp.delenv(k, raising=False)
    try:
        d, alg, losses = ppo_update_from_fixture("mlp", DEV, R.HipRolloutKernels())
        return d, alg, losses, _weights(alg)
    finally:
        mp.undo()


def test_update_on_the_engine_matches_the_reference(graphed):
    d, alg, losses, _ = graphed
    assert alg._engine is not None and alg._engine.enc_dims and alg._engine.graphs is not None
    assert alg._graph is None and not alg._graph_on  # the torch path's graph is not involved
    w = check_update("mlp", d, alg, losses, rtol_loss=1e-3, atol_w=1e-4, atol_max=3e-3, rtol_lr=1e-14)
    print(f"\nPPO.update of the encoder module on the HIP engine vs the reference (CPU): max |dw| {w:.2e}")


@pytest.mark.parametrize("env", [{"GO1_PPO_GRAPH": "0"}, {"GO1_PPO_SPLIT": "1"}], ids=["eager", "split"])
def test_eager_and_split_updates_are_the_graphed_update_to_the_bit(graphed, engine_on, env):
    for k, v in env.items():
        engine_on.setenv(k, v)
    d, alg, losses = ppo_update_from_fixture("mlp", DEV, R.HipRolloutKernels())
    eng = alg._engine
    assert eng is not None
    if "GO1_PPO_GRAPH" in env:
        assert eng.graphs is None
    else:
        assert len(eng.graphs) == 3
    got = _weights(alg)
    for k, v in graphed[3].items():
        assert torch.equal(got[k], v), k
    assert tuple(losses) == tuple(graphed[2]) and alg.learning_rate == graphed[1].learning_rate


def test_switch_off_is_the_torch_path(engine_on):
    engine_on.setenv("GO1_PPO_ENCODER_ENGINE", "0")
    d, alg, losses = ppo_update_from_fixture("mlp", DEV, R.HipRolloutKernels())
    assert alg._engine is None and alg._graph is None and not alg._graph_on
    engine_on.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    engine_on.setenv("GO1_PPO_ENGINE", "0")  # GO1_PPO_ENGINE=0 still wins
    assert not alg._engine_on()
    engine_on.delenv("GO1_PPO_ENGINE")
    engine_on.delenv("GO1_PPO_ENCODER_ENGINE")  # the default: off
    assert RC.ENGINE_DEFAULT["mlp"] is False and not alg._engine_on()


def test_learning_iteration_torch_update_after_it_and_optimizer_state(engine_on, tmp_path):
    """rollout_cnn.Runner.learn(1) on the HIP env (64 envs, 4 steps, 2 mini-batches, the 21 x 11 map) with the update
    on the engine; then an update with the switch off (release_optimizer_state over the wider slice); then the
    optimizer state_dict / load_state_dict round trip back on the engine."""
    from legged_tracking_amd import env as E
    mp = engine_on
    torch.manual_seed(0)
    cfg, shape = _env_cfg(64, False)
    mp.setattr(RC.AC_Args, "height_map_shape", shape)
    mp.setattr(RC.AC_Args, "use_cnn", False)
    mp.setitem(RC.FUSED_DEFAULT, "mlp", True)
    mp.setattr(R.RunnerArgs, "num_steps_per_env", 4)
    mp.setattr(R.PPO_Args, "num_learning_epochs", 1)
    mp.setattr(R.PPO_Args, "num_mini_batches", 2)
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=DEV, cfg=cfg, seed=4))
    assert env.num_obs == S + int(np.prod(shape))
    runner = RC.Runner(env, device=DEV, save_dir=str(tmp_path))
    alg = runner.alg
    ac = alg.actor_critic
    assert isinstance(ac, RC.ActorCritic) and isinstance(alg.fused, RC.FusedEncoderPolicy)
    assert PE.encoder_supported(ac) and alg._engine_on()
    before = _weights(alg)
    losses, update = [], alg.update

    def capture():
        losses.append(update())
        return losses[-1]

    alg.update = capture
    runner.learn(1)
    torch.cuda.synchronize()
    assert alg._engine is not None and alg._engine.enc_dims
    assert len(losses) == 1 and np.isfinite(np.array([float(x) for x in losses[0]])).all(), losses
    after = _weights(alg)
    for k in ("height_map_encoder.model.0.weight", "adaptation_module.0.weight", "actor_body.0.weight",
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
    # ---- the rollout's storage again (update() cleared the step counter only), switch off: the torch path
    st = alg.storage
    st.step = st.num_transitions_per_env
    mp.setenv("GO1_PPO_ENCODER_ENGINE", "0")
    out = update()
    torch.cuda.synchronize()
    assert np.isfinite(np.array([float(x) for x in out])).all(), out
    assert all(bool(torch.isfinite(v).all()) for v in _weights(alg).values())
    # ---- back on the engine after an optimizer state round trip: the state is imported, the steps continue
    mp.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    sd0, sd1 = alg.optimizer.state_dict(), alg.adaptation_module_optimizer.state_dict()
    alg.optimizer.load_state_dict(sd0)
    alg.adaptation_module_optimizer.load_state_dict(sd1)
    st.step = st.num_transitions_per_env
    eng = alg._engine
    out = update()
    torch.cuda.synchronize()
    assert alg._engine is eng and np.isfinite(np.array([float(x) for x in out])).all(), out
    # one learn() of two mini-batches, the torch update's two, these two
    assert eng.steps.tolist() == [6.0, 6.0]
    sd = alg.adaptation_module_optimizer.state_dict()["state"]
    assert len(sd) == len(PE.ENC_PARAM_NAMES) + PE.N_ADAPT_TENSORS  # encoder + adaptation module
    assert len(alg.optimizer.state_dict()["state"]) == len(eng.names)
    for s in alg.optimizer.state_dict()["state"].values():
        assert float(s["step"]) == 6.0 and bool(torch.isfinite(s["exp_avg"]).all())
    fused_matches_module()
    env.close()
