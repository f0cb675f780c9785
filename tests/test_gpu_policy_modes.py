"""go1_policy_forward's inference modes on the MI355X (go1_policy_args.mode, ABI 2): GO1_POLICY_STUDENT (act_student:
adaptation module + actor, no critic) and GO1_POLICY_TEACHER (act_teacher: the actor on [history, privileged obs]),
both kernel variants, through FusedPolicy / FusedEncoderPolicy and the raw C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from legged_tracking_amd import learn_abi as LA, native, rollout as R, rollout_cnn as RC
from tests import cnn_cases as CC
from tests.test_rollout import _ac, _fixture, _trained

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLE = (123, 7, 0)
LA_E_ARG = -1  # GO1_RT_E_ARG


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(n, hist, npriv, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, hist, device=DEV, generator=g), torch.randn(n, npriv, device=DEV, generator=g)


@pytest.mark.parametrize("variant", [0, 1])
def test_student_writes_the_bits_of_the_full_mode(variant):
    """n = 37: variant 0 runs two actor workgroups (32 + 5 envs), variant 1 three (16 + 16 + 5)."""
    ac = _ac(_fixture(), DEV)
    pol = R.HipRolloutKernels().policy(ac)
    pol.variant = variant
    h, p = _inputs(37, 261, 2, 37)
    full = pol.forward(h, p, sample=SAMPLE)
    for priv in (p, None):  # privileged_obs may be NULL in student mode
        got = pol.forward(h, priv, sample=SAMPLE, mode=LA.GO1_POLICY_STUDENT)
        torch.cuda.synchronize()
        assert got[1] is None  # value = NULL is accepted
        for i, name in ((0, "mean"), (2, "latent"), (3, "actions"), (4, "sigma"), (5, "log_prob")):
            np.testing.assert_array_equal(_np(got[i]), _np(full[i]), err_msg=name)
    mean, _, latent = pol.forward(h, None, mode=LA.GO1_POLICY_STUDENT)  # and without the sample
    np.testing.assert_array_equal(_np(mean), _np(full[0]))
    np.testing.assert_array_equal(_np(latent), _np(full[2]))
    # a value buffer handed in is never written
    a = pol.args
    value = torch.full((37 + 16,), -7.5, device=DEV)
    m2 = torch.empty_like(mean)
    a.value, a.action_mean, a.actions = value.data_ptr(), m2.data_ptr(), None
    assert pol._forward(C.byref(a), pol._stream()) == 0
    torch.cuda.synchronize()
    assert bool((value == -7.5).all())
    np.testing.assert_array_equal(_np(m2), _np(full[0]))
    assert int(pol.overflow.item()) == 0


def _actor_f64(sd, x):
    """actor_body (Linear / ELU chain) in float64 from state-dict arrays."""
    x = np.asarray(x, np.float64)
    idx = sorted(int(k.split(".")[1]) for k in sd if k.startswith("actor_body.") and k.endswith(".weight"))
    for j, i in enumerate(idx):
        x = x @ np.asarray(sd[f"actor_body.{i}.weight"], np.float64).T + np.asarray(sd[f"actor_body.{i}.bias"],
                                                                                    np.float64)
        if j < len(idx) - 1:
            x = np.where(x > 0, x, np.expm1(np.minimum(x, 0)))
    return x


@pytest.mark.parametrize("rows", [None, 21])
def test_teacher_on_the_trained_checkpoint(rows):
    """actor_body(cat(h, p)) on the reference's trained weights (6 privileged values, 267 actor inputs) against the
    f64 forward of the state dict, at the bound test_fused_policy_kernel_runs_the_reference_trained_checkpoint holds
    the kernel to on these weights."""
    d, ac = _trained()
    ac = ac.to(DEV)
    sd = {k[3:]: d[k] for k in d.files if k.startswith("sd/")}
    h, p = d["in/hist"][:rows], d["in/priv"][:rows]
    want = _actor_f64(sd, np.concatenate([h, p], -1))
    pol = R.HipRolloutKernels().policy(ac)
    ht, pt = torch.from_numpy(h).to(DEV), torch.from_numpy(p).to(DEV)
    outs = []
    for variant in (0, 1):
        pol.variant = variant
        out = pol.forward(ht, pt, sample=SAMPLE, mode=LA.GO1_POLICY_TEACHER)
        torch.cuda.synchronize()
        assert out[1] is None
        np.testing.assert_allclose(_np(out[0]), want, rtol=2e-5, atol=2e-5 * np.abs(want).max())
        np.testing.assert_array_equal(_np(out[2]), p)  # the latent output is the privileged input, exactly
        outs.append([_np(t) for t in out if t is not None])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)  # the variants are bit-identical
    # the draws are those of the full mode (same Philox key and counter use): actions - mean is the same noise
    full = pol.forward(ht, pt, sample=SAMPLE)
    ulp = 4 * np.finfo(np.float32).eps * max(np.abs(outs[1][2]).max(), float(full[3].abs().max()))
    np.testing.assert_allclose(outs[1][2] - outs[1][0], _np(full[3] - full[0]), rtol=0, atol=ulp)
    assert int(pol.overflow.item()) == 0


def _f64_module(ac, hist, npriv):
    ac64 = R.ActorCritic(70, npriv, hist, 12).double()
    ac64.load_state_dict({k: v.double().cpu() for k, v in ac.state_dict().items()})
    return ac64


@pytest.mark.parametrize("hist,variants", [(2100, (0,)), (288 - 2, (0, 1))])
def test_streamed_history(hist, variants):
    """2,100 inputs stream through eight chunks of 288; with 286 the two latent inputs are the last two of the last
    K group.  Against the f64 module at test_fused_policy_kernel_streams_long_histories' bound."""
    torch.manual_seed(3)
    npriv, n = 2, 33
    ac = R.ActorCritic(70, npriv, hist, 12).to(DEV)
    pol = R.HipRolloutKernels().policy(ac)
    h, p = _inputs(n, hist, npriv, 5)
    ac64 = _f64_module(ac, hist, npriv)
    with torch.no_grad():
        h64, p64 = h.double().cpu(), p.double().cpu()
        want = {LA.GO1_POLICY_STUDENT: (ac64.act_student(h64), ac64.adaptation_module(h64)),
                LA.GO1_POLICY_TEACHER: (ac64.act_teacher(h64, p64), p64)}
    for variant in variants:
        pol.variant = variant
        for mode, (mt, lt) in want.items():
            mean, value, latent = pol.forward(h, p, mode=mode)
            torch.cuda.synchronize()
            assert value is None
            for got, w in ((mean, mt), (latent, lt)):
                w = w.numpy()
                np.testing.assert_allclose(_np(got), w, rtol=2e-5, atol=2e-5 * np.abs(w).max())
    assert int(pol.overflow.item()) == 0


def _actor_split_max(ac, h, p):
    """The largest |value| the teacher mode splits into f16: the inputs and the actor's hidden outputs."""
    vals = [h.abs().max(), p.abs().max()]
    with torch.no_grad():
        x = torch.cat((h, p), -1)
        for m in list(ac.actor_body)[:-1]:
            x = m(x)
            if not isinstance(m, torch.nn.Linear):
                vals.append(x.abs().max())
    return max(float(v) for v in vals)


@pytest.mark.parametrize("target,expect_fallback", [(5.0e4, False), (2.0e5, True)])
def test_teacher_range_guard(target, expect_fallback):
    """test_fused_policy_range_guard's construction on the actor only: its layer-1 weights scaled until the largest
    value the kernel splits is 5e4 (no fallback) / 2e5 (beyond f16: the workgroups recompute the actor in f32 from
    the unsplit weights with the privileged input)."""
    d = _fixture()
    n = 64 + 7
    g = torch.Generator(device=DEV).manual_seed(3)
    h = torch.rand(n, 261, device=DEV, generator=g) + 0.5
    p = torch.rand(n, 2, device=DEV, generator=g)
    base = _ac(d, DEV)
    with torch.no_grad():
        base.actor_body[0].weight.copy_(base.actor_body[0].weight.abs())
        base.actor_body[0].bias.zero_()
    lo, hi = 1.0, 1.0e6  # the actor alone needs a larger scale than the three nets of the original
    for _ in range(60):  # bisect the layer-1 scale for the target maximum (monotone in the scale)
        mid = (lo * hi) ** 0.5
        ac = _ac(d, DEV)
        ac.load_state_dict(base.state_dict())
        with torch.no_grad():
            ac.actor_body[0].weight.mul_(mid)
        lo, hi = (mid, hi) if _actor_split_max(ac, h, p) < target else (lo, mid)
    mx = _actor_split_max(ac, h, p)
    assert 0.95 * target < mx < 1.05 * target, mx
    with torch.no_grad():
        mt = ac.act_teacher(h, p)
    pol = R.HipRolloutKernels().policy(ac)
    for variant in (0, 1):
        pol.variant = variant
        pol.overflow.zero_()
        mean, value, latent, actions, sigma, logp = pol.forward(h, p, sample=(5, 1, 0), mode=LA.GO1_POLICY_TEACHER)
        torch.cuda.synchronize()
        np.testing.assert_allclose(_np(mean), _np(mt), rtol=1e-4, atol=1e-5 * mt.abs().max().item())
        np.testing.assert_array_equal(_np(latent), _np(p))
        assert torch.isfinite(actions).all() and torch.isfinite(logp).all()
        assert (int(pol.overflow.item()) > 0) == expect_fallback, (target, variant, int(pol.overflow.item()))


@pytest.mark.parametrize("mode", [3, -1])
@pytest.mark.parametrize("variant", [0, 1])
def test_other_modes_are_refused_and_write_nothing(mode, variant):
    ac = _ac(_fixture(), DEV)
    pol = R.HipRolloutKernels().policy(ac)
    pol.variant = variant
    h, p = _inputs(37, 261, 2, 1)
    pol.forward(h, p, sample=SAMPLE)  # packs, fills the argument struct
    a = pol.args
    bufs = {k: torch.full(s, -3.0, device=DEV) for k, s in (("action_mean", (37, 12)), ("value", (37,)),
                                                            ("latent", (37, 2)), ("actions", (37, 12)),
                                                            ("action_sigma", (37, 12)), ("log_prob", (37,)))}
    for k, t in bufs.items():
        setattr(a, k, t.data_ptr())
    a.mode = mode
    assert pol._forward(C.byref(a), pol._stream()) == LA_E_ARG
    assert "mode" in pol.lib.go1_rollout_last_error().decode()
    with pytest.raises(RuntimeError, match="mode"):
        native.check(pol.lib, LA_E_ARG)
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t == -3.0).all()), k


def _encoder_module(shape, E, use_cnn, seed=0):
    torch.manual_seed(seed)
    args = type("A", (RC.AC_Args,), dict(use_cnn=use_cnn, height_map_shape=shape, cnn_num_embedding=E))
    num_obs = CC.NUM_SCALAR + int(np.prod(shape))
    return RC.ActorCritic(num_obs, 2, num_obs, 12, ac_args=args).to(DEV)


@pytest.mark.parametrize("shape,E,use_cnn", [((2, 5, 3), 128, False), ((2, 61, 31), 128, True)])
def test_encoder_module_modes(shape, E, use_cnn):
    """FusedEncoderPolicy in student and teacher mode against the module's act_student / act_teacher, at the bound
    tests/test_gpu_encoder.py holds the fused forward to (rtol 2e-5, atol 2e-5 of the output's scale)."""
    ac = _encoder_module(shape, E, use_cnn)
    n, S = 19, CC.NUM_SCALAR
    g = torch.Generator(device=DEV).manual_seed(1)
    hist = torch.randn(n, ac.num_obs, device=DEV, generator=g)
    hist[:, S:] = torch.rand(n, ac.num_map, device=DEV, generator=g) * 10 - 5
    priv = torch.randn(n, 2, device=DEV, generator=g)
    pol = RC.FusedEncoderPolicy(ac)
    info = {}
    with torch.no_grad():
        ms = ac.act_student(hist, policy_info=info)
        mt = ac.act_teacher(hist, priv)
    for mode, want, lat in ((LA.GO1_POLICY_STUDENT, ms, info["latents"]), (LA.GO1_POLICY_TEACHER, mt, _np(priv))):
        mean, value, latent = pol.forward(hist, priv, mode=mode)
        torch.cuda.synchronize()
        assert value is None
        for got, w in ((mean, _np(want)), (latent, lat)):
            np.testing.assert_allclose(_np(got), w, rtol=2e-5, atol=2e-5 * np.abs(w).max())
    full = pol.forward(hist, priv)
    np.testing.assert_array_equal(_np(pol.forward(hist, None, mode=LA.GO1_POLICY_STUDENT)[0]), _np(full[0]))
    assert int(pol.overflow.item()) == 0


def test_fused_inference_runs_the_kernels_and_fills_policy_info():
    """rollout.fused_inference on a GPU module: the fused policy, act_inference / act_expert's results."""
    ac = _ac(_fixture(), DEV)
    h, p = _inputs(37, 261, 2, 2)
    ob = {"obs": h, "obs_history": h, "privileged_obs": p}
    with torch.no_grad():
        for teacher in (False, True):
            pol = R.fused_inference(ac, teacher=teacher)
            assert isinstance(pol.fused, R.FusedPolicy)
            info, info_ref = {}, {}
            got = pol(ob, info)
            want = ac.act_teacher(h, p, policy_info=info_ref) if teacher else ac.act_inference(ob, info_ref)
            np.testing.assert_allclose(_np(got), _np(want), rtol=1e-4, atol=1e-4)
            lat, lat_ref = info["latents"], info_ref["latents"]
            assert type(lat) is type(lat_ref)
            np.testing.assert_allclose(_np(lat) if teacher else lat, _np(lat_ref) if teacher else lat_ref,
                                       rtol=1e-4, atol=1e-4)
        a1 = R.fused_inference(ac, sample=9)(ob)
        a2 = R.fused_inference(ac, sample=9)(ob)
        assert torch.equal(a1, a2) and not torch.equal(a1, R.fused_inference(ac, sample=10)(ob))
        # pack(): the kernels read the module's new weights
        pol = R.fused_inference(ac)
        before = pol(ob).clone()
        ac.actor_body[6].bias.add_(1.0)
        assert torch.equal(pol(ob), before)
        pol.pack()
        np.testing.assert_allclose(_np(pol(ob)), _np(before) + 1.0, rtol=0, atol=1e-5)
