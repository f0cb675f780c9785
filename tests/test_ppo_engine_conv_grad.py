"""The HIP PPO update engine's CNN encoder path (csrc/ppo_update.hip with go1_ppo_dims.enc_mode = 3, csrc/ppo_conv.h),
call by call, against float64 autograd (tests/ppo_ref_conv.py): tests/test_ppo_engine_encoder_grad.py's method on
rollout_cnn.ActorCritic with use_cnn on the (2, 61, 31) map.

One mini-batch through PPOEngine's C-ABI calls -- _bind, _write_hyper, pack, idx, grad(0), step(0), grad(1), step(1)
-- on a fresh engine per case.  New code reached: conv_pack_kernel, conv_kernel forward (features, their maximum)
and backward (the forward again, pool routing, conv2's weight / bias / data gradient, conv1's), the linear layer's
xw<LIN> launch into G's leading columns and its problem of the grouped wgrad (K = 3360), embgrad_kernel without the
ELU' factor (three sources in phase 0, one in phase 1), d feat over the transposed image padded to 3456 columns, the
conv partials' four reduce segments, finalize_kernel's clear lists with the two new max slots, Adam and the re-pack
over the phase-1 slice [conv1 | conv2 | linear | adaptation module].

Data: tests/conv_cases.py (tests/ppo_cases.py's recipe; the mini-batch's maps screened at the parameters of both
phases, tests/conv_ref.py).  Shapes (E, frames, priv, actions, mb):
    min_mb     128  1  2  12  5     the smallest mini-batch the engine takes
    frames     256  2  2  12  37    the frame offset
    past_tile  512  1  8  16  131   a row past a 128-row tile
    ragged     128  1  2  12  257   the smallest mb at which a workgroup of conv_kernel takes two rows (a launch has
                                    at most 256 workgroups) and the last strip is ragged (129 workgroups, the last one row)
    window     128  2  2  12  37    the history stored as a strided window (hist_ld > hist)
    ties       128  1  2  12  37    three rows of exact ties: a map constant per channel, two integer plateaus, zeros

Gradient bound: tests/test_ppo_engine_encoder_grad.py's: per tensor max and relative L2 error against f64, the engine
within K x the yardstick (torch's f32 autograd of the same one-pass loss on the GPU) with the existing floors, on every
gradient tensor and the five aux sums.  K is twice the worst measured ratio rounded up to a power of two, at most 32.

Measured on an MI355X (worst engine / yardstick ratio per case, over both phases, tensors and metrics): min_mb 13.58
(adaptation_module.4.bias, phase 1, max: 1.83e-6 against 8.48e-8), frames 6.28, past_tile 9.31, ragged 13.37
(height_map_encoder.model.0.bias, phase 1, L2: 3.13e-6 against 2.34e-7), window 11.10 (the conv1 bias, phase 1),
ties 9.22 (adaptation_module.2.bias, phase 1).
K = 32 (2 x 13.58 rounded up), the cap.  The screen took 3 to 7 rounds (at first 5 of 5, 30 of 37, 109 of 131, 197
of 257, 28 of 37 rows unsafe at the parameters of either phase).

The step, determinism and world = 2: as tests/test_ppo_engine_encoder_grad.py.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import ppo_engine as PE  # noqa: E402
from tests import ppo_cases, ppo_ref_conv as ref  # noqa: E402
from tests.conv_cases import ConvCase, TieRowUnsafe  # noqa: E402
from tests.ppo_cases import DEV, _args  # noqa: E402
from tests.test_ppo_engine_grad import _check_branches, _step_check, _torch_adam  # noqa: E402

NAUX = PE.NAUX
K_GRAD = 32.0  # the module docstring
NAMES = ref.NAMES
N1 = ref.N_PHASE1_TENSORS
_compare = functools.partial(ppo_cases._compare, k_grad=K_GRAD, show="[conv-grad]")

SHAPES = {
    # name: (E, frames, priv, actions, mb, window, tie rows)
    "min_mb": (128, 1, 2, 12, 5, 0, False),
    "frames": (256, 2, 2, 12, 37, 0, False),
    "past_tile": (512, 1, 8, 16, 131, 0, False),
    "ragged": (128, 1, 2, 12, 257, 0, False),
    "window": (128, 2, 2, 12, 37, 3, False),
    "ties": (128, 1, 2, 12, 37, 0, True),
}


def _case(shape_name, seed=0, screen=False):
    """`screen`: for the comparison against f64 (tests/conv_cases.py: the maps screened at both phases' parameters,
    phase 0's step from preset moments at step 999); the step and determinism tests compare nothing across a
    ReLU or pool decision and take the rows as drawn."""
    E, frames, priv, na, mb, window, ties = SHAPES[shape_name]
    for s in range(seed, seed + 16):
        try:
            c = ConvCase(E, frames, priv, na, mb, window, s, ties=ties, screen=screen)
            break
        except TieRowUnsafe:  # the tie maps are fixed: the first seed whose filters leave them only their exact ties
            continue
    else:
        raise AssertionError("no seed in 16 leaves the tie rows safe")
    if screen:
        print(f"\n[conv-grad] {shape_name}: screen: {c.unsafe_first} of {mb} rows unsafe at first, none after "
              f"{c.rounds} redraws")
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradients_and_loss_sums_against_f64(shape):
    mb, priv = SHAPES[shape][4], SHAPES[shape][2]
    worst = [0.0, ""]
    with _args():
        c = _case(shape, screen=True)
        e = c.eng
        hp = c.start()
        ac64, ac32 = c.ac64(), c.alg.actor_critic
        e.grad(0)
        torch.cuda.synchronize()
        g = e.grads.clone()
        r64 = ref.phase0(ac64, c.rows64, c.idx, hp)
        y32 = ref.phase0(ac32, c.rows32, c.idx, hp)
        _check_branches(r64, hp["clip_param"], hp["use_clipped_value_loss"])
        kl = float(r64["kl_mean"])
        assert 0.03 < kl < 0.06, kl
        rt = r64["row_terms"]
        bad = _compare("phase0", NAMES, c.split(g[NAUX:]), y32["grads"], r64["grads"], worst, rt)
        aux = ("surrogate_sum", "value_sum", "kl_sum")
        bad += _compare("phase0", aux, [g[i] for i in range(3)], [y32[k] for k in aux], [r64[k] for k in aux], worst, rt)
        # ---- the step: one optimizer step, the rate by the KL rule, the loss means from the f32 sums
        lr0 = float(e.lr.item())
        e.step(0)
        torch.cuda.synchronize()
        assert e.steps.tolist() == [1000.0, 0.0]  # from the preset state (tests/conv_cases.py)
        assert float(e.lr.item()) == ref.lr_rule(lr0, kl, hp["desired_kl"])
        losses = e.losses.tolist()
        f32 = np.float32
        a0 = g[:NAUX].cpu().numpy()
        assert losses[:2] == [float(a0[1] / f32(mb)), float(a0[0] / f32(mb))], losses
        # ---- phase 1 at the stepped parameters: the embedding is computed again from the moved encoder
        ac64 = c.ac64()
        e.grad(1)
        torch.cuda.synchronize()
        g1 = e.grads[:NAUX + e.n_adapt].clone()
        r64 = ref.phase1(ac64, c.rows64, c.idx, hp)
        y32 = ref.phase1(ac32, c.rows32, c.idx, hp)
        assert r64["num_train"] == mb // 5 * 4 > 0
        rt = r64["row_terms"]
        bad += _compare("phase1", NAMES[:N1], c.split(g1[NAUX:], True), y32["grads"], r64["grads"], worst, rt)
        aux = ("train_sum", "test_sum")
        bad += _compare("phase1", aux, [g1[3], g1[4]], [y32[k] for k in aux], [r64[k] for k in aux], worst, rt)
        e.step(1)
        torch.cuda.synchronize()
        assert e.steps.tolist() == [1000.0, 1.0]
        ntr = mb // 5 * 4
        losses = e.losses.tolist()
        a1 = g1[:NAUX].cpu().numpy()
        assert losses[2:] == [float(a1[3] / f32(ntr * priv)), float(a1[4] / f32((mb - ntr) * priv))], losses
    print(f"\n[conv-grad] {shape}: worst engine / yardstick error ratio {worst[0]:.2f} ({worst[1]})")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("preset", [False, True], ids=["fresh", "preset999"])
def test_step_against_f64_from_the_engines_own_gradient(preset):
    """finalize_kernel + norm_kernel + adam_kernel over the CNN module's slices: every parameter in phase 0, encoder
    (two convolutions and the linear layer) + adaptation module with its own moments in phase 1; the actor, the critic
    and std untouched by step(1), all three encoder layers moved."""
    worst = [-1e9, ""]
    c = _case("frames", seed=1)
    e = c.eng
    with _args():
        hp = c.start()
        e.grad(0)
        torch.cuda.synchronize()
        gen = torch.Generator(device=DEV).manual_seed(4)
        steps0 = 999 if preset else 0
        if preset:
            e.steps.fill_(999.0)
            for m1, m2 in ((e.exp_avg, e.exp_avg_sq), (e.ad_exp_avg, e.ad_exp_avg_sq)):
                m1.copy_(torch.randn(m1.shape, device=DEV, generator=gen) * 1e-3)
                m2.copy_(torch.rand(m2.shape, device=DEV, generator=gen) * 1e-5)
        g = e.grads[NAUX:].clone()
        p0, m0, v0 = e.params.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone()
        lr0 = float(e.lr.item())
        kl_mean = float(e.grads[2]) / c.mb
        e.step(0)
        torch.cuda.synchronize()
        lr = ref.lr_rule(lr0, kl_mean, hp["desired_kl"])
        assert float(e.lr.item()) == lr == lr0 / 1.5
        assert e.steps.tolist() == [steps0 + 1.0, float(steps0)]
        coef, _ = ref.clip_coef([g], hp["max_grad_norm"])
        p64, m64, v64 = p0.double(), m0.double(), v0.double()
        ref.adam_step(p64, g.double() * coef, m64, v64, steps0, lr, hp)
        py, my, vy = _torch_adam(p0, g, m0, v0, steps0, lr, hp["max_grad_norm"])
        out = [_step_check(f"phase0 {k}", a, y, r, worst) for k, a, y, r in
               (("params", e.params, py, p64), ("exp_avg", e.exp_avg, my, m64), ("exp_avg_sq", e.exp_avg_sq, vy, v64))]
        assert float((e.params - p0).abs().max()) > 0.1 * lr
        # ---- phase 1: adaptation_lr, no clip, the slice's own state
        e.grad(1)
        torch.cuda.synchronize()
        n = e.n_adapt
        n_enc = e.offsets["adaptation_module.0.weight"]
        assert 0 < n_enc < n and e.offsets[NAMES[0]] == 0
        g1 = e.grads[NAUX:NAUX + n].clone()
        p1, m1, v1 = e.params[:n].clone(), e.ad_exp_avg.clone(), e.ad_exp_avg_sq.clone()
        rest = e.params[n:].clone()
        e.step(1)
        torch.cuda.synchronize()
        assert e.steps.tolist() == [steps0 + 1.0, steps0 + 1.0] and float(e.lr.item()) == lr
        assert torch.equal(e.params[n:], rest)  # the actor, the critic and std: bit-unchanged
        for k in (0, 2, 4):  # conv1, conv2 and the linear layer moved
            lo, hi = e.offsets[NAMES[k]], e.offsets[NAMES[k + 1]]
            assert float((e.params[lo:hi] - p1[lo:hi]).abs().max()) > 0.1 * hp["adaptation_lr"], NAMES[k]
        p64, m64, v64 = p1.double(), m1.double(), v1.double()
        ref.adam_step(p64, g1.double(), m64, v64, steps0, hp["adaptation_lr"], hp)
        py, my, vy = _torch_adam(p1, g1, m1, v1, steps0, hp["adaptation_lr"], None)
        out += [_step_check(f"phase1 {k}", a, y, r, worst) for k, a, y, r in
                (("params", e.params[:n], py, p64), ("exp_avg", e.ad_exp_avg, my, m64),
                 ("exp_avg_sq", e.ad_exp_avg_sq, vy, v64))]
    print(f"\n[conv-step] {'step 999' if preset else 'fresh'}: worst (|engine err| - 2 |yardstick err|) / ulp "
          f"{worst[0]:.3f} ({worst[1]}); max errors engine / yardstick "
          + ", ".join(f"{a:.1e}/{b:.1e}" for a, b in out))


def _one_minibatch(case, world=1, scale=None):
    e = case.eng
    case.start(world)
    out = {}
    for phase in (0, 1):
        e.grad(phase)
        torch.cuda.synchronize()
        out[f"grads{phase}"] = e.grads.clone() if phase == 0 else e.grads[3:NAUX + e.n_adapt].clone()
        if scale:  # stands in for the all-reduce over `scale` identical ranks
            e.grads.mul_(scale)
        e.step(phase)
        torch.cuda.synchronize()
    for k in ("params", "exp_avg", "exp_avg_sq", "ad_exp_avg", "ad_exp_avg_sq", "steps", "lr", "losses"):
        out[k] = getattr(e, k).clone()
    return out


@pytest.mark.gpu
def test_fresh_engines_agree_bitwise_and_world_2_of_identical_ranks_is_world_1():
    with _args():
        a = _one_minibatch(_case("frames", seed=3))
        b = _one_minibatch(_case("frames", seed=3))
        w = _one_minibatch(_case("frames", seed=3), world=2, scale=2.0)
    assert a["steps"].tolist() == [1.0, 1.0]
    for k, v in a.items():
        assert torch.equal(v, b[k]), ("determinism", k)
        assert torch.equal(v, w[k]), ("world 2", k)
    assert float(a["grads0"][NAUX:].abs().max()) > 0 and float(a["losses"].abs().min()) > 0
