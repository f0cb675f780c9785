"""The float64 restatement of PPO.update's mini-batch (tests/ppo_ref.py) pinned on the CPU, before the GPU tests
(tests/test_ppo_engine_grad.py) use it as the reference of the HIP update engine.

  * all 20 mini-batches of the reference's recorded PPO.update (tests/golden/ppo_rollout.npz, its permutation)
    driven through the restatement in f64: losses, learning-rate decisions and every weight at the tolerances
    tests/test_rollout.py::test_ppo_update_matches_reference_on_gpu derives for "the same maths, another rounding";
  * its step (clip_grad_norm_'s coefficient, the single-tensor Adam) against torch.optim.Adam in f64.
"""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import rollout as R  # noqa: E402
from tests import ppo_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f64_restatement_reproduces_the_reference_update_fixture():
    from tests.test_rollout import _check_update
    d = np.load(os.path.join(REPO, "tests", "golden", "ppo_rollout.npz"))
    A = R.PPO_Args
    for k in ("num_learning_epochs", "num_mini_batches", "clip_param", "learning_rate", "max_grad_norm",
              "value_loss_coef", "entropy_coef", "desired_kl", "num_adaptation_module_substeps"):
        assert float(getattr(A, k)) == float(d["upd/args/" + k]), k
    ac = R.ActorCritic(261, 2, 261, 12)
    ac.load_state_dict({k[len("upd/sd_before/"):]: torch.from_numpy(d[k]) for k in d.files
                        if k.startswith("upd/sd_before/")})
    ac64 = ppo_ref.double_copy(ac)
    storage = types.SimpleNamespace(**{k: torch.from_numpy(d["upd/storage/" + k]) for k in ppo_ref.ROW_KEYS})
    rows = ppo_ref.rows_of(storage, torch.float64)
    perm = torch.from_numpy(d["upd/perm"]).long()
    losses, lr = ppo_ref.update(ac64, rows, perm, A.num_mini_batches, A.num_learning_epochs,
                                ppo_ref.hyper_from_args(A), float(A.learning_rate))
    alg = types.SimpleNamespace(learning_rate=lr, actor_critic=ac64)
    w = _check_update(d, alg, losses, rtol_loss=1e-3, atol_w=1e-4, atol_max=3e-3)
    print(f"\nf64 restatement vs the reference's f32 update: max |dw| {w:.2e}, lr {lr:.3e}")


@pytest.mark.parametrize("max_norm,steps0", [(0.5, 0), (100.0, 0), (0.5, 999)])
def test_restated_step_is_torch_adam_after_clip_grad_norm_in_f64(max_norm, steps0):
    g = torch.Generator().manual_seed(3)
    n = 1000
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    grad = torch.randn(n, generator=g, dtype=torch.float64) * 0.1
    m0 = torch.randn(n, generator=g, dtype=torch.float64) * 1e-2 if steps0 else torch.zeros(n, dtype=torch.float64)
    v0 = torch.rand(n, generator=g, dtype=torch.float64) * 1e-3 if steps0 else torch.zeros(n, dtype=torch.float64)
    hp = dict(beta1=0.9, beta2=0.999, eps=1e-8)
    lr = 7e-4
    # torch: clip_grad_norm_, then Adam (single-tensor form)
    p = torch.nn.Parameter(p0.clone())
    p.grad = grad.clone()
    torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt = torch.optim.Adam([p], lr=lr, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(steps0)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    opt.step()
    # the restatement
    coef, norm = ppo_ref.clip_coef([grad], max_norm)
    assert (coef < 1.0) == (norm > max_norm)
    q, m, v = p0.clone(), m0.clone(), v0.clone()
    step = ppo_ref.adam_step(q, grad * coef, m, v, steps0, lr, hp)
    assert step == steps0 + 1 == int(opt.state[p]["step"])
    for a, b in ((q, p.detach()), (m, opt.state[p]["exp_avg"]), (v, opt.state[p]["exp_avg_sq"])):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-13, atol=0)
    assert not torch.equal(q, p0)


def test_restated_lr_rule_takes_the_reference_decisions():
    f = ppo_ref.lr_rule
    assert f(1e-3, 0.03, 0.01) == 1e-3 / 1.5 and f(1e-3, 0.004, 0.01) == 1e-3 * 1.5
    assert f(1e-3, 0.01, 0.01) == 1e-3 and f(1e-3, 0.0, 0.01) == 1e-3 and f(1e-3, 0.5, None) == 1e-3
    assert f(1.2e-5, 0.03, 0.01) == 1e-5 and f(9e-3, 0.004, 0.01) == 1e-2
