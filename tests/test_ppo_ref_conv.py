"""The float64 restatement of the CNN encoder module's mini-batch (tests/ppo_ref_conv.py) pinned on the CPU against
the reference's recorded PPO.update (tests/golden/ppo_cnn_cnn.npz: E = 32, 8 Adam steps of both optimizers, mb = 32,
the adaptive-KL learning rate), before the GPU tests use it as the reference of the HIP engine's CNN path.

The bounds are tests/test_ppo_ref_cnn.py's (the same maths in another summation order: one encoder pass where the
reference runs three).  Measured here: max |dw| 1.8e-5, losses within 2.1e-7 relative, the learning rate identical.
"""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import rollout as R  # noqa: E402
from tests import cnn_cases as CC, ppo_ref_conv  # noqa: E402
from tests.test_actor_critic_cnn import check_update, load_case  # noqa: E402


def fixture_rows(case, d, dtype=torch.float64):
    """The storage the reference's PPO.update saw, as flat (rows, ...) tensors."""
    dm = CC.dims(case)
    st = types.SimpleNamespace(**{k: torch.from_numpy(d["upd/storage/" + k]) for k in ppo_ref_conv.ROW_KEYS
                                  if k != "observation_histories"})
    st.observation_histories = torch.from_numpy(CC.make_hist(case, CC.UPD_T * CC.UPD_N, what=1).reshape(
        CC.UPD_T, CC.UPD_N, -1))
    assert st.observation_histories.shape[-1] == dm["num_hist"]
    return ppo_ref_conv.rows_of(st, dtype)


def test_f64_restatement_reproduces_the_reference_update_fixture():
    d, ac, _, _, _ = load_case("cnn")
    A = R.PPO_Args
    for k in ("clip_param", "learning_rate", "max_grad_norm", "value_loss_coef", "entropy_coef", "desired_kl",
              "num_adaptation_module_substeps"):
        assert float(getattr(A, k)) == float(d["upd/args/" + k]), k
    assert (int(d["upd/args/num_learning_epochs"]), int(d["upd/args/num_mini_batches"])) == \
        (CC.UPD_EPOCHS, CC.UPD_MINI_BATCHES)
    ac64 = ppo_ref_conv.double_copy(ac)
    rows = fixture_rows("cnn", d)
    perm = torch.from_numpy(d["upd/perm"]).long()
    assert perm.numel() // CC.UPD_MINI_BATCHES == 32
    losses, lr = ppo_ref_conv.update(ac64, rows, perm, CC.UPD_MINI_BATCHES, CC.UPD_EPOCHS,
                                    ppo_ref_conv.hyper_from_args(A), float(A.learning_rate))
    alg = types.SimpleNamespace(learning_rate=lr, actor_critic=ac64)
    w = check_update("cnn", d, alg, losses, rtol_loss=1e-3, atol_w=1e-4, atol_max=3e-3, rtol_lr=1e-14)
    rel = np.abs(np.array(losses) - d["upd/losses"]).max() / np.abs(d["upd/losses"]).max()
    print(f"\nf64 one-pass restatement vs the reference's f32 update: max |dw| {w:.2e}, losses {rel:.1e}, lr {lr:.3e}")


def test_one_pass_gradient_is_the_modules_three_pass_gradient_in_f64():
    """The chain rule the restatement (and the engine) rests on: one encoder pass feeding the three heads has the
    gradient of the module's own forward, which encodes once per head, to f64 rounding."""
    d, ac, _, _, _ = load_case("cnn")
    ac64 = ppo_ref_conv.double_copy(ac)
    rows = fixture_rows("cnn", d)
    idx = torch.from_numpy(d["upd/perm"]).long()[:32]
    hp = ppo_ref_conv.hyper_from_args(R.PPO_Args)
    one = ppo_ref_conv.phase0(ac64, rows, idx, hp)
    from tests import ppo_ref
    sd = dict(ac64.named_parameters())
    b = {k: v[idx] for k, v in rows.items()}
    ac64.update_distribution(b["observation_histories"])
    value = ac64.evaluate(b["observation_histories"], b["privileged_observations"])
    logp = ac64.get_actions_log_prob(b["actions"])
    ratio = torch.exp(logp - b["actions_log_prob"].squeeze(-1))
    adv, clip = b["advantages"].squeeze(-1), hp["clip_param"]
    sur = torch.max(-adv * ratio, -adv * ratio.clamp(1 - clip, 1 + clip)).mean()
    vc = b["values"] + (value - b["values"]).clamp(-clip, clip)
    vl = torch.max((value - b["returns"]).pow(2), (vc - b["returns"]).pow(2)).mean()
    loss = sur + hp["value_loss_coef"] * vl - hp["entropy_coef"] * ac64.entropy.mean()
    three = torch.autograd.grad(loss, [sd[n] for n in ppo_ref_conv.NAMES])
    for n, a, c in zip(ppo_ref_conv.NAMES, one["grads"], three):
        assert float((a - c).abs().max()) <= 1e-13 * float(c.abs().max()), n
    assert float(one["grads"][0].abs().max()) > 0 and ppo_ref.flat(one["grads"]).numel() == sum(
        p.numel() for p in ac64.parameters())
