"""The HIP PPO update engine's encoder path (csrc/ppo_update.hip, go1_ppo_dims.enc_mode = 1), call by call, against
float64 autograd (tests/ppo_ref_cnn.py): tests/test_ppo_engine_grad.py's method, data recipe and metric on
rollout_cnn.ActorCritic with the MLP height-map encoder.

One mini-batch through PPOEngine's C-ABI calls -- _bind, _write_hyper, pack, idx, grad(0), step(0), grad(1), step(1)
-- on a fresh engine per case.  New code reached: gather_kernel<true> (the last frame's scalars twice, the map into
its padded buffer, the frame offset, hist_ld > hist, the grid-stride wrap), the encoder's two xw<ELU> launches (the
embedding written into G's leading columns), pack_kernel's column map [embedding | scalars] <- [scalars | embedding]
and the partial transposed images, the three xw<LIN> products and embgrad_kernel (d emb, its column sums), the
encoder's xw<DELU> launches of both phases, the ten-problem grouped wgrad, the 33-segment reduce with the first
layers' column blocks mapped back, finalize_kernel's wider clear lists, Adam and the re-pack over the wider phase-1
slice (encoder + adaptation module).

Data (tests/ppo_cases.py's `_Case`): tests/test_ppo_engine_grad.py's recipe from the f64 forward of this module;
history frames of N(0, 1) scalars and U(-5, 5) map values (tests/cnn_cases.py), biases and std off their initial
values.  Shapes (map, E, frames, priv, actions, mb):
    production      2x21x11  256  2   2  12  37     production widths, the frame offset, a ragged tile
    small_map       2x5x3    128  1   8  16  131    n_map 30 < one K group and not a multiple of 4; a row past a tile
    caps            2x64x32  512  1   2  12  130    n_map 4096, E 512; S = 3: every column block of G is unaligned
    gather_wrap     2x5x3    128  1   2  12  16389  the gather's grid-stride wrap
    window          2x21x11  256  2   2  12  37     the history stored as a strided window (hist_ld > hist)

Gradient bound: per parameter tensor max |g - g64| / max |g64| and the relative L2 error, for the engine and for
the yardstick (torch's f32 autograd of the same one-pass loss on the GPU, hipBLASLt GEMMs); the engine within K x
the yardstick on both, tensor by tensor and on the five aux sums, with the 2^-24 floor and the condition floor of
plain row sums (tests/test_ppo_engine_grad.py's module docstring).  K is twice the worst measured ratio rounded up
to a power of two, at most 32 (3xF16 carries 2^-21 against f32's 2^-24: a factor 8 before luck).

Measured on an MI355X (worst engine / yardstick ratio per case, over both phases, tensors and metrics): production
3.34 (height_map_encoder.model.0.weight, phase 1, max: 1.26e-6 against 3.78e-7), small_map 4.29
(height_map_encoder.model.0.bias, phase 1), caps 5.11 (test_sum), gather_wrap 9.24 (height_map_encoder.model.2.bias,
phase 1, L2: 7.40e-7 against 8.01e-8), window 4.15.  K = 32 (2 x 9.24 rounded up), the existing file's cap.  The step
(engine / yardstick max errors): parameters 4.8e-8 / 4.8e-8, exp_avg 8.4e-10 / 2.0e-9, exp_avg_sq 1.3e-12 / 5.9e-12;
the phase-1 slice 7.3e-9 / 7.3e-9, 3.7e-10 / 3.7e-10, 1.6e-13 / 3.3e-13; worst margin 0.16 ulp (step 999).

The step: parameters and both moment buffers of both optimizers against f64 at <= 2 x yardstick + 1 f32 ulp of the
buffer's largest value, fresh and from step 999; after step(1) the actor, the critic and std are bit-unchanged and
the encoder has moved.  Determinism: two fresh engines agree to the bit; hyper.world = 2 with the gradient doubled
in place is world 1 to the bit.

Single-line mutations of the engine's source these tests were checked against (each fails
test_gradients_and_loss_sums_against_f64 on every shape unless noted).  In embgrad_kernel (csrc/ppo_gather.h): the
critic's term dropped from its sum; its ELU' taken from t_p instead of the embedding.  In csrc/ppo_layout.h: delta
e1's ELU' taken from a1a instead of e1 (the output of the W_E0 row); the first layers' gradient segment covering one
copy of the scalars only (Ctx::segs).  In csrc/ppo_update.hip: phase 1 without its encoder forward (phase 0's
embedding reused); the gather's frame offset 0 (gather_args; fails production and window, the two-frame shapes).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import ppo_engine as PE  # noqa: E402
from tests import ppo_cases, ppo_ref_cnn as ref  # noqa: E402
from tests.ppo_cases import DEV, _Case, _args  # noqa: E402
from tests.test_ppo_engine_grad import _check_branches, _step_check, _torch_adam  # noqa: E402

NAUX = PE.NAUX
K_GRAD = 32.0  # the module docstring
NAMES = ref.NAMES
N1 = ref.N_PHASE1_TENSORS
_compare = functools.partial(ppo_cases._compare, k_grad=K_GRAD, show="[enc-grad]")

SHAPES = {
    # name: (map shape, E, scalars, frames, priv, actions, mb, window)
    "production": ((2, 21, 11), 256, 41, 2, 2, 12, 37, 0),
    "small_map": ((2, 5, 3), 128, 41, 1, 8, 16, 131, 0),
    "caps": ((2, 64, 32), 512, 3, 1, 2, 12, 130, 0),
    "gather_wrap": ((2, 5, 3), 128, 41, 1, 2, 12, 16389, 0),
    "window": ((2, 21, 11), 256, 41, 2, 2, 12, 37, 3),
}


def _case(shape_name, seed=0):
    shape, E, S, frames, priv, na, mb, window = SHAPES[shape_name]
    return _Case(None, priv, na, mb, window, seed, encoder=(shape, E, S, frames))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradients_and_loss_sums_against_f64(shape):
    mb, priv = SHAPES[shape][6], SHAPES[shape][4]
    worst = [0.0, ""]
    with _args():
        c = _case(shape)
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
        assert e.steps.tolist() == [1.0, 0.0]
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
        assert e.steps.tolist() == [1.0, 1.0]
        ntr = mb // 5 * 4
        losses = e.losses.tolist()
        a1 = g1[:NAUX].cpu().numpy()
        assert losses[2:] == [float(a1[3] / f32(ntr * priv)), float(a1[4] / f32((mb - ntr) * priv))], losses
    print(f"\n[enc-grad] {shape}: worst engine / yardstick error ratio {worst[0]:.2f} ({worst[1]})")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("preset", [False, True], ids=["fresh", "preset999"])
def test_step_against_f64_from_the_engines_own_gradient(preset):
    """finalize_kernel + norm_kernel + adam_kernel over the wider slices: every parameter in phase 0, encoder +
    adaptation module with its own moments in phase 1; the actor, the critic and std untouched by step(1)."""
    worst = [-1e9, ""]
    c = _case("production", seed=1)
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
        assert float((e.params[:n_enc] - p1[:n_enc]).abs().max()) > 0.1 * hp["adaptation_lr"]  # the encoder moved
        p64, m64, v64 = p1.double(), m1.double(), v1.double()
        ref.adam_step(p64, g1.double(), m64, v64, steps0, hp["adaptation_lr"], hp)
        py, my, vy = _torch_adam(p1, g1, m1, v1, steps0, hp["adaptation_lr"], None)
        out += [_step_check(f"phase1 {k}", a, y, r, worst) for k, a, y, r in
                (("params", e.params[:n], py, p64), ("exp_avg", e.ad_exp_avg, my, m64),
                 ("exp_avg_sq", e.ad_exp_avg_sq, vy, v64))]
    print(f"\n[enc-step] {'step 999' if preset else 'fresh'}: worst (|engine err| - 2 |yardstick err|) / ulp "
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
        a = _one_minibatch(_case("production", seed=3))
        b = _one_minibatch(_case("production", seed=3))
        w = _one_minibatch(_case("production", seed=3), world=2, scale=2.0)
    assert a["steps"].tolist() == [1.0, 1.0]
    for k, v in a.items():
        assert torch.equal(v, b[k]), ("determinism", k)
        assert torch.equal(v, w[k]), ("world 2", k)
    assert float(a["grads0"][NAUX:].abs().max()) > 0 and float(a["losses"].abs().min()) > 0
