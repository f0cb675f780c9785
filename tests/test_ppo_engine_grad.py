"""The HIP PPO update engine (csrc/ppo_update.hip), call by call, against float64 autograd (tests/ppo_ref.py).

One mini-batch through PPOEngine's C-ABI calls -- _bind, _write_hyper, pack, idx, grad(0), step(0), grad(1),
step(1) -- on a fresh engine per case, reading `grads`, `params`, the Adam state, `steps`, `lr` and `losses`.  This
is what the end-to-end update tests cannot see: Adam normalises the gradient, so a gradient off by a constant factor,
a wrong clip coefficient below max_grad_norm or a wrong bias correction moves the weights by less than their
tolerance, and they run one shape (hist 261, priv 2, 12 actions, mb 384) only.

Kernels reached: gather_kernel (ragged mb, its grid-stride wrap, hist_ld > hist, padded ldg), adapt_kernel<0|1|2>,
head_kernel<12|16> (1, 12, 13, 16 actions, odd mb, the wrap), the EPI_DELU backward launches, the critic's
two-segment first-layer gradient copy, reduce_kernel, norm_kernel, finalize_kernel, adam_kernel.

Data (`_Case`, tests/ppo_cases.py): the stored quantities are built from the f64 forward of the same weights so that no row sits near a
clip edge in either precision and every branch of the loss holds >= 10 % of the rows (asserted from the f64 values):
ratios exp(-delta), delta cycling over {-0.5, -0.1, 0, 0.1, 0.5} (1.65, 1.105, 1, 0.905, 0.61 against the clip
[0.8, 1.2]); advantages of both signs, the last row of every group of 4 and of the mini-batch 10 x larger (a dropped
or duplicated tail row shows); V - values cycling over {0.5, 0.05, -0.05, -0.5}; a KL mean of about 0.04; idx a
permutation slice of a storage larger than the mini-batch that contains the last storage row.

Gradient bound.  Per parameter tensor e = max |g - g64| / max |g64| and the relative L2 error, for the engine and
for the yardstick: torch's f32 autograd of the same loss on the GPU (rollout.ActorCritic's own modules, hipBLASLt
GEMMs).  The engine must stay within K x the yardstick on both, tensor by tensor, and on the five aux sums; an
error below half an f32 ulp of the tensor's largest entry (2^-24 relative) counts as that: no f32 result is owed
more, and the yardstick lands on 0 by luck on the smallest tensors.  A gradient or loss sum that is a plain sum
over the rows (the last layers' biases, the aux sums; per-row terms t from f64 autograd) is owed less: its terms are
f32-rounded, so no f32 result is better than 2^-24 sum |t| in general, and the floor is 2^-24 sum |t| / |sum t|,
the condition number of the sum.  K is twice the worst measured ratio, rounded up to a power of two, and at most 32.

Measured on an MI355X (worst engine / yardstick ratio per case, over both phases, tensors and metrics; the
yardstick's own error moves by up to 1.5 x between runs): production_ragged 2.7 - 3.6, smallest 4.6 - 7.0,
head12_edge 8.55 (adaptation_module.4.bias, phase 0, L2: 1.17e-6 against 1.37e-7), head16_edge 2.8 - 3.6,
widest_head_latent 3.3 - 3.7, checkpoint_latent_padded_ldg 4.1 - 6.0, head_adapt_wrap 7.7, gather_wrap 6.4,
velocity_window1 / 2 7.1 / 5.0; the hyper-parameter variants 2.3 - 5.4.  The 3xF16 products carry 2^-21 against
f32's 2^-24, a factor 8 before any luck.  K = 32 (2 x 8.55 rounded up).  Before the condition floor the critic's
output bias read 10.3 at mb 8199 and 29.8 at mb 16389 (engine 2.55e-6, yardstick 8.6e-8 relative to a sum whose
condition number is 280: the engine at 0.15 ulp of sum |t|, the yardstick at 0.005 ulp): a finding about the
metric on one-element tensors, not about the kernel, and K was not raised for it.

The step: max |engine - f64| <= 2 max |yardstick - f64| + one f32 ulp of the buffer's largest value, per buffer.
Measured (engine / yardstick): parameters 4.8e-8 / 4.8e-8 .. 5.9e-8 / 5.9e-8, exp_avg 1.0e-9 / 1.0e-9 .. 8.9e-9 /
6.7e-9, exp_avg_sq 2.0e-12 / 2.6e-12 .. 1.7e-10 / 1.1e-10; the adaptation optimizer alike.  This test found
finalize_kernel taking 1 - beta from the f32-rounded betas (exp_avg 4 ulp, exp_avg_sq 1.3e-5 relative off torch's);
fixed in the kernel.

Mutations of the engine's source these tests were checked against (each fails the named test).  In head_kernel
(csrc/ppo_heads.h): invM from M + 1, tie weights 1, the value_loss_coef dropped from dV, the entropy term's sign
(test_gradients_* / test_hyper_parameter_branches_*); inr with < (test_rows_exactly_on_the_clip_edge_*).  In
csrc/ppo_layout.h: num_train = M * 4 / 5 (make_layout), the critic's priv-column copy from offset H (Ctx::segs)
(test_gradients_*).  In finalize_kernel (csrc/ppo_step.h): gscale without / world (test_fresh_engines_*); bc2 without
the square root (test_step_*).  The
head loop bound m < H.M instead of m < H.M + half computes the same values (the half-wave shuffles never cross the
halves; the + half only keeps the wave's trip count uniform): no test can tell it apart.
"""
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import ppo_engine as PE, rollout as R  # noqa: E402
from tests import ppo_cases, ppo_ref  # noqa: E402
from tests.ppo_cases import DELTAS, DEV, FLOOR, KL0, VOFFS, _Case, _args, _errs  # noqa: E402,F401

NAUX = PE.NAUX
K_GRAD = 32.0  # the module docstring: measured worst ratio 8.55
_compare = functools.partial(ppo_cases._compare, k_grad=K_GRAD)

SHAPES = {
    "production_ragged": (261, 2, 12, 37),
    "smallest": (1, 1, 1, 5),
    "head12_edge": (70, 2, 12, 130),
    "head16_edge": (70, 2, 13, 130),
    "widest_head_latent": (70, 8, 16, 131),
    "checkpoint_latent_padded_ldg": (261, 6, 12, 1027),
    "head_adapt_wrap": (70, 2, 12, 8199),
    "gather_wrap": (70, 2, 12, 16389),
    "velocity_window1": (2100, 2, 12, 133),
    "velocity_window2": (2100, 2, 12, 133),
}
WINDOW = {"velocity_window1": 1, "velocity_window2": 2}
VARIANTS = {
    "plain_value_loss": dict(use_clipped_value_loss=False),
    "selective": dict(selective_adaptation_module_loss=True),
    "entropy0": dict(entropy_coef=0.0),
    "entropy05": dict(entropy_coef=0.05),
    "no_kl": dict(desired_kl=None),
    # value_loss_coef off its default 1 (a factor dropped from dV is invisible at 1), on both value losses
    "value_coef": dict(value_loss_coef=0.5),
    "plain_value_coef": dict(use_clipped_value_loss=False, value_loss_coef=2.0),
}


def _check_branches(r64, clip, clipped_value):
    """Every branch of the loss holds >= 10 % of the rows, none within 0.04 of a clip edge (a condition on the
    inputs, from the f64 values)."""
    ratio, adv, dv = r64["ratio"], r64["advantages"], r64["value_minus_old"]
    n = ratio.numel()
    for name, mask in (("ratio below", ratio < 1 - clip), ("ratio inside", (ratio > 1 - clip) & (ratio < 1 + clip)),
                       ("ratio above", ratio > 1 + clip), ("adv > 0", adv > 0), ("adv < 0", adv < 0)) + \
            ((("value clip low", dv < -clip), ("value clip high", dv > clip), ("value clip off", dv.abs() < clip))
             if clipped_value else ()):
        assert int(mask.sum()) * 10 >= n, (name, int(mask.sum()), n)
    assert float(((ratio - (1 - clip)).abs().min())) > 0.04 and float((ratio - (1 + clip)).abs().min()) > 0.04
    assert float((dv.abs() - clip).abs().min()) > 0.04


def _gradient_case(shape, over):
    hist, priv, na, mb = SHAPES[shape]
    worst = [0.0, ""]
    with _args(**over):
        c = _Case(hist, priv, na, mb, window=WINDOW.get(shape, 0))
        e = c.eng
        hp = c.start()
        ac64, ac32 = c.ac64(), c.alg.actor_critic
        e.grad(0)
        torch.cuda.synchronize()
        g = e.grads.clone()
        r64 = ppo_ref.phase0(ac64, c.rows64, c.idx, hp)
        y32 = ppo_ref.phase0(ac32, c.rows32, c.idx, hp)
        _check_branches(r64, hp["clip_param"], hp["use_clipped_value_loss"])
        kl = float(r64["kl_mean"])
        assert 0.03 < kl < 0.06, kl  # far from 2 desired_kl = 0.02: the schedule divides the rate
        rt = r64["row_terms"]
        bad = _compare("phase0", PE.PARAM_NAMES, c.split(g[NAUX:]), y32["grads"], r64["grads"], worst, rt)
        aux = ("surrogate_sum", "value_sum", "kl_sum")
        bad += _compare("phase0", aux, [g[i] for i in range(3)], [y32[k] for k in aux], [r64[k] for k in aux], worst, rt)
        # ---- the step (checked against f64 in test_step_*): one optimizer step, the rate by the KL rule
        lr0 = float(e.lr.item())
        e.step(0)
        torch.cuda.synchronize()
        assert e.steps.tolist() == [1.0, 0.0]
        assert float(e.lr.item()) == ppo_ref.lr_rule(lr0, kl, hp["desired_kl"])
        # the loss means: the f32 sums (compared with f64 above) over the mini-batch's rows, one f32 division each
        losses = e.losses.tolist()
        f32 = np.float32
        a0 = g[:NAUX].cpu().numpy()
        assert losses[:2] == [float(a0[1] / f32(mb)), float(a0[0] / f32(mb))], losses
        # ---- phase 1 at the stepped parameters
        ac64 = c.ac64()
        e.grad(1)
        torch.cuda.synchronize()
        g1 = e.grads[:NAUX + e.n_adapt].clone()
        r64 = ppo_ref.phase1(ac64, c.rows64, c.idx, hp)
        y32 = ppo_ref.phase1(ac32, c.rows32, c.idx, hp)
        assert r64["num_train"] == mb // 5 * 4 > 0
        names = PE.PARAM_NAMES[:PE.N_ADAPT_TENSORS]
        rt = r64["row_terms"]
        bad += _compare("phase1", names, c.split(g1[NAUX:], True), y32["grads"], r64["grads"], worst, rt)
        aux = ("train_sum", "test_sum")
        bad += _compare("phase1", aux, [g1[3], g1[4]], [y32[k] for k in aux], [r64[k] for k in aux], worst, rt)
        if hp["selective"]:  # only column 0 is regressed: the other output rows get no gradient at all
            w4, b4 = c.split(g1[NAUX:], True)[4:6]
            assert torch.count_nonzero(w4[1:]) == 0 and torch.count_nonzero(b4[1:]) == 0
            assert torch.count_nonzero(w4[0]) > 0 and float(b4[0]) != 0.0
        e.step(1)
        torch.cuda.synchronize()
        assert e.steps.tolist() == [1.0, 1.0]
        nsel = 1 if hp["selective"] else priv
        ntr = mb // 5 * 4
        losses = e.losses.tolist()
        a1 = g1[:NAUX].cpu().numpy()
        assert losses[2:] == [float(a1[3] / f32(ntr * nsel)), float(a1[4] / f32((mb - ntr) * nsel))], losses
        assert float(r64["train_loss"]) == pytest.approx(float(r64["train_sum"]) / (ntr * nsel), rel=1e-12)
    print(f"\n[ppo-grad] {shape} {over or ''}: worst engine / yardstick error ratio {worst[0]:.2f} ({worst[1]})")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradients_and_loss_sums_against_f64(shape):
    _gradient_case(shape, {})


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", ["production_ragged", "widest_head_latent"])
def test_hyper_parameter_branches_against_f64(shape, variant):
    _gradient_case(shape, VARIANTS[variant])


# ------------------------------------------------------------------------------------------------ the step
def _ulp(x64):
    """Spacing of f32 at |x| (normal range)."""
    a = x64.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def _step_check(tag, eng, yard, ref, worst):
    """Per buffer, as the gradient metric: max |engine - f64| <= 2 max |yardstick - f64| + one f32 ulp of the
    buffer's largest value (an element-wise form would compare the two roundings of single elements: the yardstick
    lands within a tenth of an ulp on some of 700k elements by luck); the relative L2 error likewise, + 2^-24."""
    ee, ey = (eng.double() - ref).abs(), (yard.double() - ref).abs()
    ulp = float(_ulp(ref.abs().max()))
    w = (float(ee.max()) - 2 * float(ey.max())) / ulp
    if w > worst[0]:
        worst[:] = [w, tag]
    assert w <= 1.0, (tag, w, float(ee.max()), float(ey.max()))
    assert float(ee.norm() / ref.norm()) <= 2 * float(ey.norm() / ref.norm()) + FLOOR, tag
    return float(ee.max()), float(ey.max())


def _torch_adam(p0, grad, m0, v0, steps0, lr, max_norm):
    """The yardstick: clip_grad_norm_ (phase 0) and torch.optim.Adam's single-tensor form in f32 on the GPU."""
    p = torch.nn.Parameter(p0.clone())
    p.grad = grad.clone()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt = torch.optim.Adam([p], lr=lr, foreach=False, fused=False)
    opt.state[p] = {"step": torch.tensor(float(steps0)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


@pytest.mark.gpu
@pytest.mark.parametrize("preset", [False, True], ids=["fresh", "preset999"])
@pytest.mark.parametrize("clip", ["engaged", "off", "default"])
def test_step_against_f64_from_the_engines_own_gradient(clip, preset):
    """finalize_kernel + norm_kernel + adam_kernel: the KL rule, clip_grad_norm_'s coefficient, the bias
    corrections and the Adam arithmetic, both optimizers, from fresh state and from step 999 with random moments;
    max_grad_norm at half / twice the measured norm and the default."""
    hist, priv, na, mb = SHAPES["head12_edge"]
    worst = [-1e9, ""]
    c = _Case(hist, priv, na, mb, seed=1)
    e = c.eng
    with _args():
        hp = c.start()
        e.grad(0)
        torch.cuda.synchronize()
        g = e.grads[NAUX:].clone()
        norm = float(g.double().norm())
        max_norm = {"engaged": 0.5 * norm, "off": 2.0 * norm, "default": R.PPO_Args.max_grad_norm}[clip]
        max_norm = float(np.float32(max_norm))  # hyper-parameters reach the engine as f32: the same input to all three
    with _args(max_grad_norm=max_norm):
        hp = ppo_ref.hyper_from_args(R.PPO_Args)
        e._write_hyper(R.PPO_Args, 1)
        gen = torch.Generator(device=DEV).manual_seed(4)
        steps0 = 999 if preset else 0
        if preset:
            e.steps.fill_(999.0)
            for m1, m2 in ((e.exp_avg, e.exp_avg_sq), (e.ad_exp_avg, e.ad_exp_avg_sq)):
                m1.copy_(torch.randn(m1.shape, device=DEV, generator=gen) * 1e-3)
                m2.copy_(torch.rand(m2.shape, device=DEV, generator=gen) * 1e-5)
        # element 11 of every buffer: g = m = v = 0, Adam must leave the parameter alone
        e.grads[NAUX + 11] = 0.0
        e.exp_avg[11] = 0.0
        e.exp_avg_sq[11] = 0.0
        g = e.grads[NAUX:].clone()
        p0, m0, v0 = e.params.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone()
        lr0 = float(e.lr.item())
        kl_mean = float(e.grads[2]) / mb  # the engine's own KL sum
        assert kl_mean > 3 * hp["desired_kl"]
        e.step(0)
        torch.cuda.synchronize()
        lr = ppo_ref.lr_rule(lr0, kl_mean, hp["desired_kl"])
        assert float(e.lr.item()) == lr == lr0 / 1.5
        assert e.steps.tolist() == [steps0 + 1.0, float(steps0)]
        coef, norm = ppo_ref.clip_coef([g], hp["max_grad_norm"])
        if clip != "default":
            assert (coef < 1.0) == (clip == "engaged") and (coef == 1.0) == (clip == "off"), (coef, norm)
        p64, m64, v64 = p0.double(), m0.double(), v0.double()
        ppo_ref.adam_step(p64, g.double() * coef, m64, v64, steps0, lr, hp)
        py, my, vy = _torch_adam(p0, g, m0, v0, steps0, lr, hp["max_grad_norm"])
        out = [_step_check(f"phase0 {k}", a, y, r, worst) for k, a, y, r in
               (("params", e.params, py, p64), ("exp_avg", e.exp_avg, my, m64), ("exp_avg_sq", e.exp_avg_sq, vy, v64))]
        assert float(e.params[11]) == float(p0[11]) and float(e.exp_avg[11]) == 0.0 == float(e.exp_avg_sq[11])
        assert float((e.params - p0).abs().max()) > 0.1 * lr
        # ---- phase 1: adaptation_lr, no clip, the adaptation module's own state
        e.grad(1)
        torch.cuda.synchronize()
        n = e.n_adapt
        g1 = e.grads[NAUX:NAUX + n].clone()
        p1, m1, v1 = e.params[:n].clone(), e.ad_exp_avg.clone(), e.ad_exp_avg_sq.clone()
        rest = e.params[n:].clone()
        e.step(1)
        torch.cuda.synchronize()
        assert e.steps.tolist() == [steps0 + 1.0, steps0 + 1.0] and float(e.lr.item()) == lr
        assert torch.equal(e.params[n:], rest)  # the adaptation optimizer steps the adaptation module only
        p64, m64, v64 = p1.double(), m1.double(), v1.double()
        ppo_ref.adam_step(p64, g1.double(), m64, v64, steps0, hp["adaptation_lr"], hp)
        py, my, vy = _torch_adam(p1, g1, m1, v1, steps0, hp["adaptation_lr"], None)
        out += [_step_check(f"phase1 {k}", a, y, r, worst) for k, a, y, r in
                (("params", e.params[:n], py, p64), ("exp_avg", e.ad_exp_avg, my, m64),
                 ("exp_avg_sq", e.ad_exp_avg_sq, vy, v64))]
    print(f"\n[ppo-step] clip {clip}, {'step 999' if preset else 'fresh'}: worst (|engine err| - 2 |yardstick err|) "
          f"/ ulp {worst[0]:.3f} ({worst[1]}); max errors engine / yardstick "
          + ", ".join(f"{a:.1e}/{b:.1e}" for a, b in out))


# ------------------------------------------------------------------------------------------------ exact checks
@pytest.mark.gpu
@pytest.mark.parametrize("lr0,dk_factor,want", [(1e-3, 0.25, "down"), (1e-3, 8.0, "up"), (1e-3, 1.0, "same"),
                                                (1e-3, None, "same"), (1.2e-5, 0.25, "floor"), (9e-3, 8.0, "ceil")])
def test_learning_rate_decisions(lr0, dk_factor, want):
    """finalize_kernel's KL rule (ppo.py:127-130) as Python floats: desired_kl a quarter of / eight times / equal
    to the data's KL mean, None, and the clamps at 1e-5 and 1e-2."""
    hist, priv, na, mb = SHAPES["head12_edge"]
    c = _Case(hist, priv, na, mb, seed=2)
    e = c.eng
    with _args():
        kl = float(ppo_ref.phase0(c.ac64(), c.rows64, c.idx, ppo_ref.hyper_from_args(R.PPO_Args))["kl_mean"])
    dk = None if dk_factor is None else kl * dk_factor
    with _args(desired_kl=dk):
        c.start()
        e.lr.fill_(lr0)
        e.grad(0)
        e.step(0)
        torch.cuda.synchronize()
        assert abs(float(e.grads[2]) / mb - kl) < 1e-4 * kl
        got = float(e.lr.item())
        expect = {"down": lr0 / 1.5, "up": lr0 * 1.5, "same": lr0, "floor": 1e-5, "ceil": 1e-2}[want]
        assert got == expect == ppo_ref.lr_rule(lr0, kl, dk), (got, expect)
        if want in ("floor", "ceil"):
            assert lr0 / 1.5 < 1e-5 or lr0 * 1.5 > 1e-2


def _one_minibatch(case, world=1, scale=None):
    e = case.eng
    case.start(world)
    out = {}
    for phase in (0, 1):
        e.grad(phase)
        torch.cuda.synchronize()
        # phase 1 writes aux[3:5] and the adaptation slice (aux[0:3] keep phase 0's, all-reduced, sums)
        out[f"grads{phase}"] = e.grads.clone() if phase == 0 else e.grads[3:NAUX + e.n_adapt].clone()
        if scale:  # stands in for the all-reduce over `scale` identical ranks
            e.grads.mul_(scale)
        e.step(phase)
        torch.cuda.synchronize()
    for k in ("params", "exp_avg", "exp_avg_sq", "ad_exp_avg", "ad_exp_avg_sq", "steps", "lr", "losses"):
        out[k] = getattr(e, k).clone()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["production_ragged", "widest_head_latent"])
def test_fresh_engines_agree_bitwise_and_world_2_of_identical_ranks_is_world_1(shape):
    """Two fresh engines on the same inputs: bit-identical gradients, parameters and Adam state (fixed summation
    orders, no float atomics).  hyper.world = 2 with the gradient doubled in place between grad and step (the
    all-reduce of two identical ranks; every factor involved is a power of two) = world 1, to the bit: every / world
    of finalize_kernel."""
    hist, priv, na, mb = SHAPES[shape]
    with _args():
        a = _one_minibatch(_Case(hist, priv, na, mb, seed=3))
        b = _one_minibatch(_Case(hist, priv, na, mb, seed=3))
        w = _one_minibatch(_Case(hist, priv, na, mb, seed=3), world=2, scale=2.0)
    assert a["steps"].tolist() == [1.0, 1.0]
    for k, v in a.items():
        assert torch.equal(v, b[k]), ("determinism", k)
        assert torch.equal(v, w[k]), ("world 2", k)
    assert float(a["grads0"][NAUX:].abs().max()) > 0 and float(a["losses"].abs().min()) > 0


@pytest.mark.gpu
def test_rows_exactly_on_the_clip_edge_follow_torch_max_and_clamp_backward():
    """head_kernel's tie and edge rules (torch.max's backward splits a tie in halves, clamp's passes the gradient on
    the closed interval) on rows whose ratio is exactly 1 with clip_param 0, so that 1 - clip = ratio = 1 + clip:
    surrogate = surrogate_clipped (a tie) and the ratio sits on both ends of the clamp at once; the whole gradient
    -adv / M must come through.  Exactness by construction: one action, a zero last actor layer with bias 0.25 = the
    stored action, std 1, so log_prob is the f32 constant -log(sqrt(2 pi)) in the engine and in torch, and it is the
    stored actions_log_prob.  The reference here is torch's f32 autograd (in f64 the constant differs from its f32
    rounding and the rows leave the edge): it must see ratio == 1 on every row, and d loss / d std, the only
    gradient the actor receives (d mu = d log_prob * (action - mu) = 0), must agree to the rounding of a 13-term f32
    sum; an open interval or unsplit ties change it by half of sum(adv) / M."""
    hist, priv, na, mb = 70, 2, 1, 13
    with _args(clip_param=0.0, use_clipped_value_loss=False):
        c = _Case(hist, priv, na, mb, seed=4)
        ac, st, e = c.alg.actor_critic, c.storage, c.eng
        with torch.no_grad():
            ac.actor_body[6].weight.zero_()
            ac.actor_body[6].bias.fill_(0.25)
            ac.std.fill_(1.0)
        st.actions[0, c.idx] = 0.25
        st.actions_log_prob[0, c.idx] = -math.log(math.sqrt(2 * math.pi))
        hp = c.start()
        e.grad(0)
        torch.cuda.synchronize()
        y32 = ppo_ref.phase0(ac, ppo_ref.rows_of(st), c.idx, hp)
        assert bool((y32["ratio"] == 1.0).all())
        got = c.eng._views(e.grads[NAUX:])
        adv = y32["advantages"].double()
        want = float(y32["grads"][-1])
        assert abs(want - (float(adv.sum()) / mb - hp["entropy_coef"])) < 1e-6 * float(adv.abs().sum()) / mb
        assert abs(float(got["std"]) - want) <= 13 * 2.0 ** -24 * float(adv.abs().sum()) / mb, (float(got["std"]), want)
        assert float(got["actor_body.6.bias"]) == 0.0 and torch.count_nonzero(got["actor_body.6.weight"]) == 0
        assert float(e.grads[0]) == pytest.approx(float(y32["surrogate_sum"]), rel=1e-6)
