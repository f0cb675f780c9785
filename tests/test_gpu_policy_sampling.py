"""The policy kernels' in-kernel Normal draw (csrc/policy_tiles.h normal4), value by value against the float64
restatement tests/normal_ref.py, on every kernel path that draws it -- the range guard's f32 fallback included.

With the actor's last Linear zeroed the action mean is exactly 0, so with std = 1 `actions` IS the kernel's z
(0 + 1 z is exact), and with another std `actions` is f32(std z).

Measured on the MI355X (each test prints its figure before asserting it):
  max |z - z64| over 4096 envs x 3 steps x 16 actions ............ 5.63e-7  -> asserted 4 x, one digit up: 3e-6
  max |log_prob - f64 sum| (16 actions, std 1: 5.77e-6; num_actions 1 / 12 / 13 / 16 at std in [0.3, 2.5]:
  7.3e-7 / 2.92e-6 / 2.88e-6 / 3.44e-6) ............................ 5.77e-6  -> asserted 4 x, one digit up: 3e-5
The reduction of log_prob over the four action groups (permlane16_swap, permlane32_swap) groups them as
(lp0 + lp1) + (lp2 + lp3) -- established in test_log_prob_grouping -- which is the fallback's order, so the fallback's
log_prob is held to the split path's bits, not only to the bound."""
import numpy as np
import pytest
import torch

from legged_tracking_amd import learn_abi as LA, rollout as R
from tests import normal_ref as NR
from tests.test_gpu_policy_modes import _actor_split_max
from tests.test_normal_ref import DRAW_N, DRAW_SEED, DRAW_STEPS, U1_ONE
from tests.test_rollout import _ac, _fixture, _split_values_max

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z_BOUND = 3e-6    # 4 x the measured 5.63e-7, rounded up to one significant digit
LP_BOUND = 3e-5   # 4 x the measured 5.77e-6, rounded up to one significant digit
MODES = (LA.GO1_POLICY_FULL, LA.GO1_POLICY_STUDENT, LA.GO1_POLICY_TEACHER)


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(n, seed=1, npriv=2):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, 261, device=DEV, generator=g), torch.randn(n, npriv, device=DEV, generator=g)


def _zeroed(ac):
    """The actor's last Linear zeroed: the action mean is exactly 0 in every mode."""
    with torch.no_grad():
        ac.actor_body[-1].weight.zero_()
        ac.actor_body[-1].bias.zero_()
    return ac


def _module(na=12, std=None):
    torch.manual_seed(na)
    ac = _zeroed(R.ActorCritic(261, 2, 261, na))
    if std is not None:
        with torch.no_grad():
            ac.std.copy_(torch.as_tensor(std, dtype=torch.float32))
    return ac.to(DEV)


def _std(na):
    """A per-action std in [0.3, 2.5] (float32 values)."""
    return np.linspace(0.3, 2.5, 16).astype(np.float32)[::-1][:na].copy()


def _sample(pol, h, p, sample, variant=0, mode=0):
    pol.variant = variant
    out = pol.forward(h, p, sample=sample, mode=mode)
    torch.cuda.synchronize()
    return _np(out[3]), _np(out[4]), _np(out[5]), _np(out[0])


def test_draw_matches_the_float64_reference():
    """z of 4096 envs x 3 steps x 16 actions (the seed's coverage of the tails, the quadrant boundaries and u1 -> 1 is
    asserted from the reference in tests/test_normal_ref.py).  Measured max |z - z64| 5.63e-7 (the worst case that
    r <= 5.887 times the hardware sin / cos error of 7.26e-7 allows is 4.3e-6, plus the 1-ulp log and sqrt); a
    structural error -- a wrong counter word, cos for sin, another lane's group -- shows as O(1)."""
    ac = _module(16)
    pol = R.HipRolloutKernels().policy(ac)
    h, p = _inputs(DRAW_N)
    worst = 0.0
    for step in DRAW_STEPS:
        z, sigma, logp, mean = _sample(pol, h, p, (DRAW_SEED, step, 0))
        assert (mean == 0.0).all() and (sigma == 1.0).all()
        z64 = NR.normal(DRAW_SEED, step, DRAW_N)
        assert np.isfinite(z).all()
        worst = max(worst, float(np.abs(z - z64).max()))
        # and log_prob is the f64 sum over the 16 actions of the reference's own draws
        lp_err = float(np.abs(logp - NR.log_prob(z64, np.ones(16))).max())
        print(f"\nstep {step}: max |z - z64| {np.abs(z - z64).max():.3e}, max |log_prob - f64| {lp_err:.3e}")
        assert lp_err <= LP_BOUND, lp_err
    print(f"max |z - z64| over {DRAW_N} x {len(DRAW_STEPS)} x 16 draws: {worst:.3e}")
    assert worst <= Z_BOUND, worst
    assert int(pol.overflow.item()) == 0


@pytest.mark.parametrize("gid,action", U1_ONE)
def test_u1_of_exactly_one_draws_zero(gid, action):
    """The block whose u1 rounds to 1.0 (tests/test_normal_ref.py): log2(1) = 0, r = sqrt(-0), and the pair is +-0
    on the hardware as in the reference -- not NaN -- with its neighbours unharmed."""
    n, na, row = 33, 12, 20
    ac = _module(na)
    pol = R.HipRolloutKernels().policy(ac)
    h, p = _inputs(n)
    z64 = NR.normal(DRAW_SEED, 7, n, gid - row)[:, :na]
    assert z64[row, action] == 0.0 and z64[row, action + 1] == 0.0
    for variant in (0, 1):
        z, _, logp, _ = _sample(pol, h, p, (DRAW_SEED, 7, gid - row), variant)
        assert z[row, action] == 0.0 and z[row, action + 1] == 0.0
        assert np.isfinite(z).all() and np.abs(z - z64).max() <= Z_BOUND
        assert np.abs(logp - NR.log_prob(z64, np.ones(na))).max() <= LP_BOUND


def test_std_scales_the_same_draw():
    """actions = f32(std z) of the std = 1 run's z, to the bit; sigma is std."""
    n, na = 97, 12
    ac = _module(na)
    pol = R.HipRolloutKernels().policy(ac)
    h, p = _inputs(n)
    z = _sample(pol, h, p, (DRAW_SEED, 7, 0))[0]
    std = _std(na)
    with torch.no_grad():
        ac.std.copy_(torch.from_numpy(std))
    for variant in (0, 1):
        a, sigma, _, _ = _sample(pol, h, p, (DRAW_SEED, 7, 0), variant)
        np.testing.assert_array_equal(a, std[None, :] * z)
        np.testing.assert_array_equal(sigma, np.broadcast_to(std, sigma.shape))


def test_every_path_draws_the_same_stream():
    """Full and student mode, both variants: the same bits of actions, sigma and log_prob on a ragged batch (97 = 6
    tiles of 16 + 1 = 3 groups of 32 + 1).  The teacher's mean differs in general; with the last layer zeroed it is 0
    too, so its actions are the same draws: held to the reference, and to the same bits."""
    n, na = 97, 12
    std = _std(na)
    ac = _module(na, std)
    pol = R.HipRolloutKernels().policy(ac)
    h, p = _inputs(n)
    sample = (DRAW_SEED, 8, 0)
    z64 = NR.normal(*sample[:2], n)[:, :na]
    want_a, want_lp = std.astype(np.float64) * z64, NR.log_prob(z64, std)
    base = None
    for mode in MODES:
        for variant in (0, 1):
            a, sigma, logp, mean = _sample(pol, h, p, sample, variant, mode)
            assert (mean == 0.0).all()
            assert np.abs(a - want_a).max() <= std.max() * Z_BOUND + 2.0 ** -24 * np.abs(want_a).max(), (mode, variant)
            assert np.abs(logp - want_lp).max() <= LP_BOUND, (mode, variant)
            if base is None:
                base = (a, sigma, logp)
            for got, ref, name in zip((a, sigma, logp), base, ("actions", "action_sigma", "log_prob")):
                np.testing.assert_array_equal(got, ref, err_msg=f"{name}, mode {mode}, variant {variant}")
    assert int(pol.overflow.item()) == 0


@pytest.mark.parametrize("seed,step,offset", [(DRAW_SEED, 2 ** 32 + 5, 0), (2 ** 40 + 3, 7, 0), (DRAW_SEED, 7, 1000),
                                              (2 ** 40 + 3, 2 ** 32 + 5, 1000)])
def test_keys_and_counters_reach_the_block(seed, step, offset):
    """The high words of rng_step and rng_seed and env_id_offset, each against the reference (not only against
    another run): a dropped `>> 32` or offset leaves the moments alone and gives other values.  Rows of an offset
    batch are rows [offset, offset + n) of an offset-0 batch, to the bit."""
    n, na = 97, 12
    ac = _module(na)
    pol = R.HipRolloutKernels().policy(ac)
    h, p = _inputs(n)
    z64 = NR.normal(seed, step, n, offset)[:, :na]
    # the values differ from those of the truncated key / counter (the reference tells them apart)
    assert np.abs(z64 - NR.normal(seed & 0xFFFFFFFF, step & 0xFFFFFFFF, n, 0)[:, :na]).max() > 1.0
    got = []
    for mode in MODES:
        for variant in (0, 1):
            z = _sample(pol, h, p, (seed, step, offset), variant, mode)[0]
            assert np.abs(z - z64).max() <= Z_BOUND, (mode, variant, np.abs(z - z64).max())
            got.append(z)
    for z in got[1:]:
        np.testing.assert_array_equal(z, got[0])
    if offset:
        hb, pb = _inputs(offset + n, seed=2)
        for variant in (0, 1):
            zb = _sample(pol, hb, pb, (seed, step, 0), variant)[0]
            np.testing.assert_array_equal(zb[offset:], got[0])


@pytest.mark.parametrize("na", [1, 12, 13, 16])
def test_num_actions_and_padding_lanes(na):
    """The real columns are the reference's draws of actions 0 .. na - 1, and log_prob is the f64 sum over those
    only (non-unit std: a padding lane would add -z^2 / 2 - log sqrt(2 pi) of a draw no action uses)."""
    n = 97
    std = _std(na)
    ac = _module(na, std)
    pol = R.HipRolloutKernels().policy(ac)
    h, p = _inputs(n)
    sample = (DRAW_SEED, 9, 0)
    z64 = NR.normal(*sample[:2], n)
    want_a, want_lp = std.astype(np.float64) * z64[:, :na], NR.log_prob(z64, std)
    if na < 16:  # what a leaking padding lane would change, far above the bound
        assert np.abs(NR.log_prob(z64, np.concatenate([std, np.ones(16 - na)])) - want_lp).min() > 0.5
    outs = []
    for mode in MODES:
        for variant in (0, 1):
            a, sigma, logp, _ = _sample(pol, h, p, sample, variant, mode)
            assert a.shape == (n, na)
            err_a, err_lp = np.abs(a - want_a).max(), np.abs(logp - want_lp).max()
            print(f"\nna {na} mode {mode} variant {variant}: max |a - std z64| {err_a:.3e}, "
                  f"max |log_prob - f64| {err_lp:.3e}")
            assert err_a <= std.max() * Z_BOUND + 2.0 ** -24 * np.abs(want_a).max()
            assert err_lp <= LP_BOUND
            np.testing.assert_array_equal(sigma, np.broadcast_to(std, sigma.shape))
            outs.append((a, logp))
    for a, logp in outs[1:]:
        np.testing.assert_array_equal(a, outs[0][0])
        np.testing.assert_array_equal(logp, outs[0][1])


def test_log_prob_grouping():
    """Which way the lane reduction groups the four action groups' partial sums.  With std = 1 the kernel's log term
    is exactly 0 and every other operation is a single f32 operation on the kernel's own z, so numpy reproduces
    log_prob to the bit in the kernel's grouping -- and in no other.  It is (lp0 + lp1) + (lp2 + lp3), the order
    policy_fallback writes out; the sequential order differs on some row."""
    n, na = 4096, 16
    ac = _module(na)
    pol = R.HipRolloutKernels().policy(ac)
    h, p = _inputs(n)
    for variant in (0, 1):
        z, _, logp, _ = _sample(pol, h, p, (DRAW_SEED, 7, 0), variant)
        pair = NR.log_prob_f32_grouped(z, np.ones(na, np.float32), pairwise=True)
        seq = NR.log_prob_f32_grouped(z, np.ones(na, np.float32), pairwise=False)
        assert (pair != seq).any()
        np.testing.assert_array_equal(logp, pair)


# ----------------------------------------------------------------------------- the range guard's f32 fallback
def _scaled(bodies, measure, target, h, p):
    """test_fused_policy_range_guard's construction: the fixture's weights with the first layers of `bodies` made
    positive, bias-free and scaled (bisection, monotone) until the largest value the kernels split is `target`."""
    ac = _ac(_fixture(), DEV)
    with torch.no_grad():
        for name in bodies:
            body = getattr(ac, name)
            body[0].weight.copy_(body[0].weight.abs())
            body[0].bias.zero_()
        base = [getattr(ac, name)[0].weight.clone() for name in bodies]
        lo, hi = 1.0, 1.0e6
        for _ in range(48):
            mid = (lo * hi) ** 0.5
            for name, w in zip(bodies, base):
                getattr(ac, name)[0].weight.copy_(w * mid)
            lo, hi = (mid, hi) if measure(ac, h, p) < target else (lo, mid)
    mx = measure(ac, h, p)
    assert 0.95 * target < mx < 1.05 * target, mx
    return ac


ALL = ("actor_body", "critic_body", "adaptation_module")


@pytest.mark.parametrize("offset", [0, 1000])
@pytest.mark.parametrize("teacher", [False, True])
def test_fallback_draws_the_same_noise(teacher, offset):
    """Hidden activations pushed to 2e5: every workgroup recomputes its envs in f32 (policy_fallback,
    policy_fallback_actor) and must draw what the split path draws -- global env id with env_id_offset, the action's
    group, the same block.  Against the reference, against a run inside the f16 range (5e4, no fallback) with the
    same seed, step and offset to the bit, and log_prob to the bit as well: the fallback's (lp0 + lp1) + (lp2 + lp3)
    is the lane reduction's grouping (test_log_prob_grouping)."""
    n, na = 64 + 7, 16  # 16 actions: with 12 the fourth group's partial sum is 0 and every grouping gives the same bits
    g = torch.Generator(device=DEV).manual_seed(3)
    h = torch.rand(n, 261, device=DEV, generator=g) + 0.5
    p = torch.rand(n, 2, device=DEV, generator=g)
    std = _std(na)
    bodies, measure = (("actor_body",), _actor_split_max) if teacher else (ALL, _split_values_max)
    modes = (LA.GO1_POLICY_TEACHER,) if teacher else (LA.GO1_POLICY_FULL, LA.GO1_POLICY_STUDENT)
    sample = (DRAW_SEED, 2 ** 32 + 5, offset)
    z64 = NR.normal(*sample[:2], n, offset)[:, :na]
    want_a, want_lp = std.astype(np.float64) * z64, NR.log_prob(z64, std)
    runs = {}
    for target in (5.0e4, 2.0e5):
        ac = _scaled(bodies, measure, target, h, p)
        ac.actor_body[-1] = torch.nn.Linear(128, na).to(DEV)  # the fixture's 12 actions widened to 16, zeroed
        ac.std = torch.nn.Parameter(torch.from_numpy(std).to(DEV))
        _zeroed(ac)
        pol = R.HipRolloutKernels().policy(ac)
        for mode in modes:
            for variant in (0, 1):
                pol.overflow.zero_()
                a, sigma, logp, mean = _sample(pol, h, p, sample, variant, mode)
                assert (int(pol.overflow.item()) > 0) == (target > 6.0e4), (target, mode, variant)
                assert (mean == 0.0).all()
                err_a, err_lp = np.abs(a - want_a).max(), np.abs(logp - want_lp).max()
                assert err_a <= std.max() * Z_BOUND + 2.0 ** -24 * np.abs(want_a).max(), (target, mode, variant, err_a)
                assert err_lp <= LP_BOUND, (target, mode, variant, err_lp)
                runs[target, mode, variant] = (a, sigma, logp)
    ref = runs[5.0e4, modes[0], 0]
    for key, got in runs.items():
        for x, y, name in zip(got, ref, ("actions", "action_sigma", "log_prob")):
            np.testing.assert_array_equal(x, y, err_msg=f"{name} {key}")


def _net_max(ac, h, p):
    """The largest |value| split on the actor's side (adaptation module, latent, actor) and on the critic's."""
    def run(seq, x):
        m = 0.0
        for mod in list(seq)[:-1]:
            x = mod(x)
            if not isinstance(mod, torch.nn.Linear):
                m = max(m, float(x.abs().max()))
        return seq[-1](x), m
    with torch.no_grad():
        lat, ma = run(ac.adaptation_module, h)
        mb = run(ac.actor_body, torch.cat((h, lat), -1))[1]
        mc = run(ac.critic_body, torch.cat((h, p), -1))[1]
    return max(ma, mb, float(lat.abs().max())), mc


def _f64(ac, h, p):
    ac64 = R.ActorCritic(261, 2, 261, 12).double()
    ac64.load_state_dict({k: v.double().cpu() for k, v in ac.state_dict().items()})
    with torch.no_grad():
        h64, p64 = h.double().cpu(), p.double().cpu()
        lat = ac64.adaptation_module(h64)
        return (ac64.actor_body(torch.cat((h64, lat), -1)).numpy(), ac64.critic_body(torch.cat((h64, p64), -1)).numpy(),
                lat.numpy())


@pytest.mark.parametrize("variant", [0, 1])
def test_fallback_touches_only_its_workgroup(variant):
    """97 rows inside the f16 range (largest split value 2e4) and row 40 alone scaled out of it.  Only the
    workgroups that hold row 40 fall back; every output row of every other workgroup is the bits of the run without
    the outlier.  The workgroups are: variant 1, the 16-env tile [32, 48) for every output; variant 0, the 32-env
    actor group [32, 64) for mean / latent / actions / sigma / log_prob and the 48-env critic group [0, 48) for the
    value.  The rows that share a workgroup with row 40 come from the f32 fallback and agree with the f64 forward at
    the suite's 2e-5 of scale."""
    n, bad = 97, 40
    g = torch.Generator(device=DEV).manual_seed(3)
    h = torch.rand(n, 261, device=DEV, generator=g) + 0.5
    p = torch.rand(n, 2, device=DEV, generator=g)
    ac = _scaled(ALL, _split_values_max, 2.0e4, h, p)
    hb = h.clone()
    hb[bad] *= 20.0
    actor_max, critic_max = _net_max(ac, hb[bad:bad + 1], p[bad:bad + 1])
    assert actor_max > 1.0e5 and (critic_max > 1.0e5 or critic_max < 5.0e4), (actor_max, critic_max)
    critic_falls = critic_max > 1.0e5
    pol = R.HipRolloutKernels().policy(ac)
    pol.variant = variant
    sample = (DRAW_SEED, 7, 0)
    clean = [_np(t) for t in pol.forward(h, p, sample=sample)]
    torch.cuda.synchronize()
    assert int(pol.overflow.item()) == 0
    got = [_np(t) for t in pol.forward(hb, p, sample=sample)]
    torch.cuda.synchronize()
    # the tile / the actor group and, where row 40's critic leaves the range too, the critic group
    assert int(pol.overflow.item()) == (1 if variant == 1 else 1 + critic_falls)
    actor_rows = range(32, 48) if variant == 1 else range(32, 64)
    critic_rows = range(32, 48) if variant == 1 else range(0, 48) if critic_falls else range(bad, bad + 1)
    names = ("mean", "value", "latent", "actions", "sigma", "log_prob")
    for name, a, b in zip(names, got, clean):
        rows = critic_rows if name == "value" else actor_rows
        keep = np.array([r not in rows for r in range(n)])
        np.testing.assert_array_equal(a[keep], b[keep], err_msg=name)
    mean64, value64, lat64 = _f64(ac, hb, p)
    for name, a, want in (("mean", got[0], mean64), ("value", got[1], value64), ("latent", got[2], lat64)):
        err = np.abs(a - want) - 2e-5 * np.abs(want)
        print(f"\nvariant {variant} {name}: max excess over rtol {err.max():.3e}, atol {2e-5 * np.abs(want).max():.3e}")
        np.testing.assert_allclose(a, want, rtol=2e-5, atol=2e-5 * np.abs(want).max(), err_msg=name)
    # the fallback's rows still carry the reference noise: actions - mean = std z
    z64 = NR.normal(*sample[:2], n)[:, :12]
    noise = got[3].astype(np.float64) - got[0].astype(np.float64)
    tol = got[4] * Z_BOUND + 2.0 ** -23 * np.maximum(np.abs(got[3]), np.abs(got[0]))
    assert (np.abs(noise - got[4] * z64) <= tol).all()
