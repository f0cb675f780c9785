"""Rows of the policy kernels stay rows: a non-finite input changes its own env only (csrc/split_mfma.h: a NaN or
inf "has no split", the workgroup's guard recomputes its envs in f32), and the batch-size edges of the two launch
shapes (16 envs per workgroup, 32 per actor workgroup, 48 per critic workgroup) write rows [0, n) and nothing else."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from legged_tracking_amd import learn_abi as LA, rollout as R, rollout_cnn as RC
from tests import cnn_cases as CC, normal_ref as NR
from tests.test_gpu_policy_sampling import Z_BOUND
from tests.test_rollout import _ac, _fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLE = (13, 7, 0)
N = 97


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(n, seed, hist=261):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, hist, device=DEV, generator=g), torch.randn(n, 2, device=DEV, generator=g)


def _heads(ac, x, p, mode):
    """(mean, value, latent) of the three heads on policy input x in torch (value None outside the full mode)."""
    with torch.no_grad():
        if mode == LA.GO1_POLICY_TEACHER:
            return ac.actor_body(torch.cat((x, p), -1)), None, p
        lat = ac.adaptation_module(x)
        mean = ac.actor_body(torch.cat((x, lat), -1))
        value = ac.critic_body(torch.cat((x, p), -1)) if mode == LA.GO1_POLICY_FULL else None
        return mean, value, lat


def _check_rows(got, f32, f64, bad_rows, n, value_bad=()):
    """got = the kernel's (mean, value, latent, actions, sigma, log_prob).  The per-env finite pattern is torch
    f32's; every env outside `bad_rows` is finite and matches the f64 forward at 2e-5 of the output's scale, and its
    actions - mean is the reference noise.  `value_bad`: further envs whose value alone is lost."""
    good = np.array([r not in bad_rows for r in range(n)])
    for name, a, b32, b64 in zip(("mean", "value", "latent"), got[:3], f32, f64):
        if a is None:
            assert b32 is None
            continue
        a, b32, b64 = _np(a).reshape(n, -1), _np(b32).reshape(n, -1), _np(b64).reshape(n, -1)
        np.testing.assert_array_equal(np.isfinite(a), np.isfinite(b32), err_msg=name)
        ok = good & np.array([r not in value_bad for r in range(n)]) if name == "value" else good
        assert np.isfinite(a[ok]).all(), name
        np.testing.assert_allclose(a[ok], b64[ok], rtol=2e-5, atol=2e-5 * np.abs(b64[ok]).max(), err_msg=name)
    mean, actions, sigma, logp = (_np(got[i]) for i in (0, 3, 4, 5))
    z64 = NR.normal(*SAMPLE[:2], n, SAMPLE[2])[:, :mean.shape[1]]
    noise = actions[good].astype(np.float64) - mean[good].astype(np.float64)
    tol = sigma[good] * Z_BOUND + 2.0 ** -23 * np.maximum(np.abs(actions[good]), np.abs(mean[good]))
    assert (np.abs(noise - sigma[good] * z64[good]) <= tol).all()
    assert np.isfinite(logp[good]).all()
    return good


CASES = {
    # a NaN, a +inf and a -inf in three envs' histories: three tiles, three actor groups, two critic groups
    "history": (((5, 17, float("nan")), (37, 260, float("inf")), (70, 0, float("-inf"))), ()),
    # a NaN in one env's privileged observations: the critic (and the teacher's actor) of that env only
    "privileged": ((), ((50, 1, float("nan")),)),
}


@pytest.mark.parametrize("mode", [LA.GO1_POLICY_FULL, LA.GO1_POLICY_STUDENT, LA.GO1_POLICY_TEACHER])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("case", list(CASES))
def test_non_finite_rows_stay_in_their_row(case, variant, mode):
    ac = _ac(_fixture(), DEV)
    ac64 = copy.deepcopy(ac).double().cpu()
    h, p = _inputs(N, 21)
    in_h, in_p = CASES[case]
    for r, k, v in in_h:
        h[r, k] = v
    for r, k, v in in_p:
        p[r, k] = v
    pol = R.HipRolloutKernels().policy(ac)
    pol.variant = variant
    got = pol.forward(h, p, sample=SAMPLE, mode=mode)
    torch.cuda.synchronize()
    f32 = _heads(ac, h, p, mode)
    f64 = _heads(ac64, h.double().cpu(), p.double().cpu(), mode)
    hist_rows = {r for r, _, _ in in_h}
    priv_rows = {r for r, _, _ in in_p}
    # the privileged NaN reaches the actor in teacher mode only
    actor_bad = hist_rows | (priv_rows if mode == LA.GO1_POLICY_TEACHER else set())
    # the value of the env with the bad privileged obs is that env's loss only
    _check_rows(got, f32, f64, actor_bad, N, value_bad=priv_rows)
    if mode != LA.GO1_POLICY_TEACHER:  # the actor of the env with the bad privileged obs stays finite
        for r in priv_rows:
            assert np.isfinite(_np(got[0])[r]).all() and np.isfinite(_np(got[3])[r]).all()
    reaches = bool(hist_rows) or mode != LA.GO1_POLICY_STUDENT  # student mode never reads privileged_obs
    assert (int(pol.overflow.item()) > 0) == reaches


def test_non_finite_height_map_stays_in_its_row():
    """The same through FusedEncoderPolicy (the (2, 5, 3) map's MLP encoder in front of the heads): a NaN in one env's
    height map."""
    shape, S = (2, 5, 3), CC.NUM_SCALAR
    torch.manual_seed(0)
    args = type("A", (RC.AC_Args,), dict(use_cnn=False, height_map_shape=shape, cnn_num_embedding=128))
    num_obs = S + int(np.prod(shape))
    ac = RC.ActorCritic(num_obs, 2, num_obs, 12, ac_args=args).to(DEV)
    ac64 = copy.deepcopy(ac).double().cpu()
    g = torch.Generator(device=DEV).manual_seed(1)
    hist = torch.randn(N, num_obs, device=DEV, generator=g)
    hist[:, S:] = torch.rand(N, ac.num_map, device=DEV, generator=g) * 10 - 5
    priv = torch.randn(N, 2, device=DEV, generator=g)
    bad = 40
    hist[bad, S + 7] = float("nan")
    pol = RC.FusedEncoderPolicy(ac)
    got = pol.forward(hist, priv, sample=SAMPLE)
    torch.cuda.synchronize()
    with torch.no_grad():
        x32 = ac.process_obs_history(hist)
        x64 = ac64.process_obs_history(hist.double().cpu())
    assert not np.isfinite(_np(x32)[bad]).all()
    _check_rows(got, _heads(ac, x32, priv, 0), _heads(ac64, x64, priv.double().cpu(), 0), {bad}, N)
    assert int(pol.overflow.item()) > 0


# ----------------------------------------------------------------------------- batch edges
@pytest.fixture(scope="module")
def edge_policy():
    ac = _ac(_fixture(), DEV)
    return ac, copy.deepcopy(ac).double().cpu(), R.HipRolloutKernels().policy(ac)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33])
def test_batch_edges_write_their_rows_only(edge_policy, n, variant):
    """n around the 16-env tile and the 32-env actor group (all below the 48-env critic group), through
    go1_policy_forward with output buffers that carry 16 sentinel rows behind row n: rows [0, n) are the f64
    forward's at 2e-5 of each output's scale, the sentinels untouched."""
    ac, ac64, pol = edge_policy
    pol.variant = variant
    h, p = _inputs(n, 100 + n)
    pol.forward(h, p, sample=SAMPLE)  # packs, fills the argument struct
    a = pol.args
    pad, sentinel = 16, -3.0
    bufs = {k: torch.full((n + pad,) + s, sentinel, device=DEV)
            for k, s in (("action_mean", (12,)), ("value", ()), ("latent", (2,)), ("actions", (12,)),
                         ("action_sigma", (12,)), ("log_prob", ()))}
    for k, t in bufs.items():
        setattr(a, k, t.data_ptr())
    assert pol._forward(C.byref(a), pol._stream()) == 0
    torch.cuda.synchronize()
    for k, t in bufs.items():
        assert bool((t[n:] == sentinel).all()), k
    mean64, value64, lat64 = _heads(ac64, h.double().cpu(), p.double().cpu(), 0)
    for k, want in (("action_mean", mean64), ("value", value64), ("latent", lat64)):
        want = _np(want).reshape(n, -1)
        np.testing.assert_allclose(_np(bufs[k][:n]).reshape(n, -1), want, rtol=2e-5, atol=2e-5 * np.abs(want).max(),
                                   err_msg=k)
    mean, actions, sigma, logp = (_np(bufs[k][:n]) for k in ("action_mean", "actions", "action_sigma", "log_prob"))
    z64 = NR.normal(*SAMPLE[:2], n)[:, :12]
    tol = sigma * Z_BOUND + 2.0 ** -23 * np.maximum(np.abs(actions), np.abs(mean))
    assert (np.abs((actions.astype(np.float64) - mean) - sigma * z64) <= tol).all()
    assert np.isfinite(logp).all()
    assert int(pol.overflow.item()) == 0
