"""The height-map encoder actor-critic (rollout_cnn.ActorCritic, legged_tracking_amd/actor_critic.py) against the
reference's go1_gym_learn.ppo_cse_cnn outputs (tests/golden/ppo_cnn_<case>.npz from tests/golden/make_golden_cnn.py), its
refusals, the weight packers and the C ABI of go1_heightmap_encode.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from legged_tracking_amd import learn_abi as LA, native, ppo_engine as PE, rollout as R, rollout_cnn as RC
from tests import cnn_cases as CC, golden_io as G
from tests.rollout_ref import TorchRolloutKernels


def load_case(case, device="cpu"):
    """(fixture, module with the case's seeded weights, history, privileged obs, actions)."""
    d = G.load(f"ppo_cnn_{case}.npz")
    dm = CC.dims(case)
    ac = RC.ActorCritic(dm["num_obs"], CC.NUM_PRIV, dm["num_hist"], CC.NUM_ACTIONS, ac_args=CC.ac_args(RC.AC_Args, case))
    keys = [str(k) for k in d["sd_keys"]]
    sd = CC.make_state_dict(case, keys, [d["sd_shape/" + k] for k in keys])
    # the seeded streams are the ones the fixture was recorded with
    np.testing.assert_allclose([np.abs(sd[k].astype(np.float64)).sum() for k in keys], d["sd_abs_sum"], rtol=1e-12)
    hist = CC.make_hist(case, dm["n"])
    np.testing.assert_allclose(np.abs(hist.astype(np.float64)).sum(), d["in/hist_abs_sum"], rtol=1e-12)
    assert list(ac.state_dict()) == keys
    assert [tuple(v.shape) for v in ac.state_dict().values()] == [tuple(d["sd_shape/" + k]) for k in keys]
    ac.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return (d, ac.to(device), torch.from_numpy(hist).to(device), torch.from_numpy(d["in/priv"]).to(device),
            torch.from_numpy(d["in/actions"]).to(device))


@pytest.mark.parametrize("case", CC.CASES)
def test_module_matches_reference(case):
    d, ac, hist, priv, acts = load_case(case)
    tol = dict(rtol=1e-6, atol=1e-6)
    with torch.no_grad():
        ac.update_distribution(hist)
        pin = ac.process_obs_history(hist)
        assert pin.shape == (CC.dims(case)["n"], CC.dims(case)["policy_input"]) == d["ac/policy_input"].shape
        np.testing.assert_allclose(pin.numpy(), d["ac/policy_input"], **tol)
        np.testing.assert_allclose(ac.get_student_latent(hist).numpy(), d["ac/latent"], **tol)
        np.testing.assert_allclose(ac.action_mean.numpy(), d["ac/mean"], **tol)
        np.testing.assert_array_equal(ac.action_std.numpy(), d["ac/std"])
        np.testing.assert_allclose(ac.get_actions_log_prob(acts).numpy(), d["ac/log_prob"], rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(ac.entropy.numpy(), d["ac/entropy"], rtol=1e-6)
        np.testing.assert_allclose(ac.evaluate(hist, priv).numpy(), d["ac/value"], **tol)
        np.testing.assert_allclose(ac.act_teacher(hist, priv).numpy(), d["ac/teacher_mean"], **tol)
        np.testing.assert_allclose(ac.act_student(hist).numpy(), d["ac/mean"], **tol)
        np.testing.assert_allclose(ac.act_inference({"obs_history": hist}).numpy(), d["ac/mean"], **tol)
        np.testing.assert_allclose(ac.act_expert({"obs_history": hist, "privileged_obs": priv}).numpy(),
                                   d["ac/teacher_mean"], **tol)
        # the f32 embedding against the f64 record, relative to its scale
        e64 = d["ac/embedding_f64"]
        np.testing.assert_allclose(pin.numpy()[:, 2 * CC.NUM_SCALAR:], e64, rtol=1e-5, atol=1e-5 * np.abs(e64).max())
        # the *_train forms PPO.update runs compute the same values
        ac.update_distribution_train(hist)
        np.testing.assert_allclose(ac.action_mean.numpy(), d["ac/mean"], **tol)
        np.testing.assert_allclose(ac.evaluate_train(hist, priv).numpy(), d["ac/value"], **tol)
        np.testing.assert_allclose(ac.adaptation_pred_train(hist).numpy(), d["ac/latent"], **tol)


@pytest.mark.parametrize("case", ["mlp", "cnn"])
def test_only_the_last_frame_reaches_the_heads(case):
    d, ac, hist, priv, acts = load_case(case)
    dm = CC.dims(case)
    assert dm["H"] == 2
    other = hist.clone()
    other[:, :dm["num_obs"]] = 0.0
    with torch.no_grad():
        assert torch.equal(ac.process_obs_history(hist), ac.process_obs_history(other))
        pin = ac.process_obs_history(hist)
    last = hist[:, dm["num_obs"]:]
    assert torch.equal(pin[:, :CC.NUM_SCALAR], last[:, :CC.NUM_SCALAR])
    assert torch.equal(pin[:, CC.NUM_SCALAR:2 * CC.NUM_SCALAR], last[:, :CC.NUM_SCALAR])


def ppo_update_from_fixture(case, device, kernels):
    """One rollout.PPO.update on the storage the reference's PPO.update saw, with its minibatch permutation."""
    d, ac, _, _, _ = load_case(case)
    dm = CC.dims(case)
    A = R.PPO_Args
    saved = A.num_learning_epochs, A.num_mini_batches
    A.num_learning_epochs, A.num_mini_batches = CC.UPD_EPOCHS, CC.UPD_MINI_BATCHES
    try:
        for k in ("num_learning_epochs", "num_mini_batches", "clip_param", "learning_rate", "max_grad_norm",
                  "value_loss_coef", "entropy_coef", "desired_kl", "num_adaptation_module_substeps"):
            assert float(getattr(A, k)) == float(d["upd/args/" + k]), k
        alg = R.PPO(ac, device=device, kernels=kernels)
        n, T = CC.UPD_N, CC.UPD_T
        alg.init_storage(n, T, [dm["num_obs"]], [CC.NUM_PRIV], [dm["num_hist"]], [CC.NUM_ACTIONS])
        st = alg.storage
        for k in ("privileged_observations", "actions", "values", "returns", "actions_log_prob", "advantages", "mu",
                  "sigma", "rewards"):
            getattr(st, k).copy_(torch.from_numpy(d["upd/storage/" + k]))
        hs = torch.from_numpy(CC.make_hist(case, T * n, what=1).reshape(T, n, -1))
        st.observation_histories.copy_(hs)
        st.observations.copy_(hs[..., -dm["num_obs"]:])
        st.step = T
        perm = torch.from_numpy(d["upd/perm"])
        real = torch.randperm
        torch.randperm = lambda *a, **k: perm.to(k.get("device") or "cpu")
        try:
            losses = alg.update()
        finally:
            torch.randperm = real
    finally:
        A.num_learning_epochs, A.num_mini_batches = saved
    return d, alg, losses


def check_update(case, d, alg, losses, rtol_loss, atol_w, atol_max=None, rtol_lr=0.0):
    """tests/test_rollout.py's _check_update on the fixture's kept positions of the updated weights: losses, the
    adaptive learning rate, `atol_w` on 99.99 % of the weights and `atol_max` (default atol_w) on every one.
    `rtol_lr`: the adaptive-KL schedule took the same decisions when the rate agrees (another decision changes it by
    a factor of 1.5); 0 where the rate is stepped in Python floats as in the reference."""
    np.testing.assert_allclose(np.array(losses, np.float64), d["upd/losses"], rtol=rtol_loss, atol=1e-7)
    assert abs(alg.learning_rate - float(d["upd/lr_after"])) <= rtol_lr * float(d["upd/lr_after"])
    keys = [str(k) for k in d["sd_keys"]]
    before = CC.make_state_dict(case, keys, [d["sd_shape/" + k] for k in keys])
    sd = alg.actor_critic.state_dict()
    diffs = []
    for i, k in enumerate(keys):
        got, was, want = sd[k].detach().cpu().numpy().ravel(), before[k].ravel(), d["upd/sd_after/" + k]
        if got.size > CC.SAMPLE_ABOVE:
            idx = CC.sample_index(case, i, got.size)
            got, was = got[idx], was[idx]
        diff = np.abs(got - want)
        assert diff.max() <= (atol_max or atol_w), (k, diff.max())
        assert k == "std" or not np.array_equal(want, was)  # the update moved the weights
        diffs.append(diff)
    diffs = np.concatenate(diffs)
    assert np.percentile(diffs, 99.99) <= atol_w, np.percentile(diffs, 99.99)
    return float(diffs.max())


@pytest.mark.parametrize("case", CC.UPDATE_CASES)
def test_ppo_update_matches_reference_on_cpu(case):
    """The same torch ops in the same order as ppo_cse_cnn/ppo.py (three encoder passes per mini-batch): 8 Adam
    steps with the adaptive-KL learning rate, at tests/test_rollout.py's CPU bounds."""
    d, alg, losses = ppo_update_from_fixture(case, "cpu", TorchRolloutKernels())
    assert alg._engine is None
    check_update(case, d, alg, losses, rtol_loss=1e-5, atol_w=1e-6)


def test_the_existing_module_is_unchanged():
    from tests.test_rollout import test_ppo_update_matches_reference_on_cpu as existing
    existing()
    ac = R.ActorCritic(70, 2, 261, 12)
    h = torch.randn(8, 261)
    with torch.no_grad():
        assert torch.equal(ac.adaptation_pred_train(h), ac.adaptation_module(h))
    assert R.Runner.actor_critic_class is R.ActorCritic and RC.Runner.actor_critic_class is RC.ActorCritic
    assert issubclass(RC.Runner, R.Runner) and RC.PPO is R.PPO and RC.RolloutStorage is R.RolloutStorage


def _args(**kw):
    return type("A", (RC.AC_Args,), kw)


def test_refusals_name_the_reference_line():
    with pytest.raises(NotImplementedError, match=r"use_gru.*actor_critic.py:103.*env dimension"):
        RC.ActorCritic(503, 2, 503, 12, ac_args=_args(use_gru=True, height_map_shape=(2, 21, 11)))
    with pytest.raises(ValueError, match=r"measure_front_half.*actor_critic.py:184"):
        RC.ActorCritic(261, 2, 261, 12, ac_args=_args(height_map_shape=(2, 21, 11)))
    with pytest.raises(ValueError, match=r"use_cnn.*\(2, 21, 11\).*320 features.*3360.*actor_critic.py:45"):
        RC.ActorCritic(503, 2, 503, 12, ac_args=_args(use_cnn=True, height_map_shape=(2, 21, 11)))
    with pytest.raises(NotImplementedError, match="normalize_obs"):
        RC.ActorCritic(503, 2, 503, 12, ac_args=_args(normalize_obs=True, height_map_shape=(2, 21, 11)))
    # the class defaults: the 61 x 31 map
    ac = RC.ActorCritic(41 + 3782, 2, 41 + 3782, 12)
    assert ac.policy_input_dim == 338 and not ac.use_cnn
    assert RC.ActorCritic(503, 2, 5 * 503, 12, ac_args=_args(height_map_shape=(2, 21, 11))).policy_input_dim == 338


def test_engine_and_head_kernel_support():
    for case in CC.CASES:
        ac = load_case(case)[1]
        assert not PE.supported(ac)            # parameter names differ: the update runs on torch
        assert not R.FusedPolicy.supported(ac)  # the heads alone do not take the raw history
        assert RC.FusedEncoderPolicy.supported(ac)
        assert ac.graph_capture is False
    assert not RC.FusedEncoderPolicy.supported(R.ActorCritic(70, 2, 261, 12))
    tanh = RC.ActorCritic(503, 2, 503, 12, ac_args=_args(activation="tanh", height_map_shape=(2, 21, 11)))
    assert not RC.FusedEncoderPolicy.supported(tanh)
    wide = RC.ActorCritic(503, 2, 503, 12, ac_args=_args(cnn_num_embedding=528, height_map_shape=(2, 21, 11)))
    assert not RC.FusedEncoderPolicy.supported(wide)


def _unpack(packed, n, k):
    """_pack_linear's records back to (hi, lo) f32 matrices of the padded shape."""
    T, Gk = packed.shape[0], packed.shape[1]
    assert packed.shape == (T, Gk, 4, 16, 16) and packed.dtype == torch.float16
    assert T == -(-n // 16) and Gk == -(-k // 32)
    hi, lo = packed[..., :8].float(), packed[..., 8:].float()
    back = lambda x: x.permute(0, 3, 1, 2, 4).reshape(T * 16, Gk * 32)  # noqa: E731  [t, g, q, m, r] -> [t m, g q r]
    return back(hi), back(lo)


@pytest.mark.parametrize("case", CC.CASES)
def test_packers_round_trip(case):
    """hi + lo reassembled against the f32 weight, and zero padding."""
    ac = load_case(case)[1]
    for m in RC.encoder_layers(ac):
        conv = isinstance(m, torch.nn.Conv2d)
        packed, bias = RC._pack_conv(m) if conv else R._pack_linear(m)
        W = m.weight.detach().reshape(m.weight.shape[0], -1)  # conv: [oc][ic * 9 + ky * 3 + kx]
        if conv:
            oc, ic = m.weight.shape[:2]
            assert W[oc - 1, (ic - 1) * 9 + 2 * 3 + 1] == m.weight[oc - 1, ic - 1, 2, 1]
        n, k = W.shape
        hi, lo = _unpack(packed, n, k)
        got = hi + lo
        # hi = f16(w) leaves |w - hi| <= 2^-11 |w|; lo = f16(w - hi) rounds that to 2^-11 relative again, 2^-22 |w|
        # in all, but no finer than half of f16's subnormal spacing, 2^-25, which is the floor for small weights
        err = (got[:n, :k] - W).abs()
        assert bool((err <= 2.0 ** -22 * W.abs() + 2.0 ** -25).all()), float((err - 2.0 ** -22 * W.abs()).max())
        big = (W - hi[:n, :k]).abs() >= 2.0 ** -14  # lo in f16's normal range: 2^-22 relative as it stands
        assert bool((err[big] <= 2.0 ** -22 * W.abs()[big]).all())
        assert not got[n:].any() and not got[:, k:].any()  # padding rows and K padding are zero
        assert bias.shape == (hi.shape[0],) and torch.equal(bias[:n], m.bias.detach()) and not bias[n:].any()


def test_encoder_abi_sizes_match_the_mirrors():
    l = R.lib()
    out = (C.c_int64 * 2)()
    l.go1_encoder_abi_sizes(out)
    assert list(out) == [C.sizeof(LA.PolicyLayer), C.sizeof(LA.EncoderArgs)]
    three = (C.c_int64 * 3)()
    l.go1_rollout_abi_sizes(three)  # unchanged: three entries
    assert list(three) == [C.sizeof(LA.Transition), C.sizeof(LA.PolicyLayer), C.sizeof(LA.PolicyArgs)]


def _enc_args(mode=LA.GO1_ENC_MLP, **kw):
    a = LA.EncoderArgs(num_obs=503, n_scalar=41, map_x=21, map_y=11, mode=mode, n_embed=256, n_feat=256, n_envs=16,
                       hist_ld=503, out_ld=338)
    a.obs_history = a.scratch = a.policy_input = 16  # never dereferenced: refused first
    for i in range(LA.GO1_ENCODER_LAYERS):
        a.layers[i].w = a.layers[i].b = a.layers[i].wf = 16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_encoder_argument_errors_are_reported_before_any_hip_call():
    l = R.lib()
    assert l.go1_heightmap_encode(None, None) == -1
    assert b"go1_heightmap_encode: bad argument" in l.go1_rollout_last_error()
    cnn = dict(mode=LA.GO1_ENC_CNN, num_obs=41 + 3782, map_x=61, map_y=31, n_feat=3360, hist_ld=3823)
    for a, msg in ((_enc_args(obs_history=None), b"bad argument"),
                   (_enc_args(policy_input=None), b"bad argument"),
                   (_enc_args(scratch=None), b"bad argument"),
                   (_enc_args(n_envs=0), b"bad argument"),
                   (_enc_args(map_x=65, num_obs=41 + 2 * 65 * 11, hist_ld=2000), b"GO1_MAX_SCAN_X"),
                   (_enc_args(map_y=33, num_obs=41 + 2 * 21 * 33, hist_ld=2000), b"GO1_MAX_SCAN_Y"),
                   (_enc_args(n_embed=513, out_ld=600), b"n_embed"),
                   (_enc_args(mode=2), b"mode"),
                   (_enc_args(n_scalar=40), b"num_obs"),
                   (_enc_args(hist_ld=500), b"hist_ld"),
                   (_enc_args(out_ld=337), b"out_ld"),
                   (_enc_args(frame_off=-1), b"frame_off"),
                   (_enc_args(**dict(cnn, n_feat=3328)), b"features"),
                   (_enc_args(**dict(cnn, map_x=60, num_obs=41 + 2 * 60 * 31)), None)):
        bad_layer = msg is None
        if bad_layer:  # a (2, 60, 31) map pools to the same 3360 features: accepted up to the layer check
            a.layers[2].wf = None
            msg = b"missing layer"
        assert l.go1_heightmap_encode(C.byref(a), None) == -1, msg
        assert msg in l.go1_rollout_last_error(), (msg, l.go1_rollout_last_error())
    with pytest.raises(native.NativeError, match="go1_heightmap_encode"):
        native.check(l, -1)
