"""One mini-batch of PPO.update for the CNN height-map encoder module (go1_gym_learn/ppo_cse_cnn/ppo.py:107-201 on
rollout_cnn.ActorCritic with use_cnn) restated in plain torch, for float64: tests/ppo_ref_cnn.py's one-pass
restatement with the CNN's parameter names.

As there: x = process_obs_history(obs_history) = [scalars | scalars | encoder(map)] of the LAST frame is computed
once per phase for the adaptation module, the actor and the critic (the reference runs the encoder three times on
every frame and sums three weight gradients; the earlier frames add exact zeros); the gradient order is the
engine's for this module, ppo_engine.CONV_PARAM_NAMES + PARAM_NAMES; phase 1 steps encoder + adaptation module.
tests/test_ppo_ref_conv.py pins it on the recorded reference update.

Autograd computes every gradient, the convolutions' and the pools' included: nothing here is derived from the HIP
engine (csrc/ppo_update.hip, csrc/ppo_conv.h).
"""
import torch
import torch.nn.functional as F

from legged_tracking_amd import rollout_cnn as RC
from legged_tracking_amd.ppo_engine import CONV_PARAM_NAMES, N_ADAPT_TENSORS, PARAM_NAMES
from tests.ppo_ref import ROW_KEYS, adam_step, clip_coef, flat, hyper_from_args, lr_rule, rows_of, unflat  # noqa: F401

NAMES = CONV_PARAM_NAMES + PARAM_NAMES
N_PHASE1_TENSORS = len(CONV_PARAM_NAMES) + N_ADAPT_TENSORS


def double_copy(ac):
    """A float64 copy of a rollout_cnn.ActorCritic on the same device."""
    new = RC.ActorCritic(ac.num_obs, ac.num_privileged_obs, ac.num_obs_history, ac.actor_body[-1].out_features,
                         ac_args=ac.ac_args)
    new = new.double().to(next(ac.parameters()).device)
    new.load_state_dict({k: v.detach().double() for k, v in ac.state_dict().items()})
    return new


def params_of(ac, phase1_only=False):
    sd = dict(ac.named_parameters())
    return [sd[n] for n in (NAMES[:N_PHASE1_TENSORS] if phase1_only else NAMES)]


def phase0(ac, rows, idx, hp):
    """ppo.py:111-153 on the rows `idx` with one encoder pass; the keys of ppo_ref.phase0."""
    b = {k: v[idx] for k, v in rows.items()}
    priv = b["privileged_observations"]
    x = ac.process_obs_history(b["observation_histories"])
    latent = ac.adaptation_module(x)  # not detached: the adaptation module and the encoder receive the actor's gradient
    mu = ac.actor_body(torch.cat((x, latent), dim=-1))
    value = ac.critic_body(torch.cat((x, priv), dim=-1))
    dist = torch.distributions.Normal(mu, mu * 0.0 + ac.std, validate_args=False)
    logp = dist.log_prob(b["actions"]).sum(dim=-1)
    sigma, entropy = dist.stddev, dist.entropy().sum(dim=-1)
    old_mu, old_sigma = b["mu"], b["sigma"]
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / old_sigma + 1.0e-5) +
                       (torch.square(old_sigma) + torch.square(old_mu - mu)) / (2.0 * torch.square(sigma)) - 0.5,
                       axis=-1)
    clip = hp["clip_param"]
    adv = torch.squeeze(b["advantages"], -1)
    ratio = torch.exp(logp - torch.squeeze(b["actions_log_prob"], -1))
    surrogate = -adv * ratio
    surrogate_clipped = -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    surrogate_rows = torch.max(surrogate, surrogate_clipped)
    surrogate_loss = surrogate_rows.mean()
    target_v, ret = b["values"], b["returns"]
    if hp["use_clipped_value_loss"]:
        value_clipped = target_v + (value - target_v).clamp(-clip, clip)
        value_rows = torch.max((value - ret).pow(2), (value_clipped - ret).pow(2))
    else:
        value_rows = (ret - value).pow(2)
    value_loss = value_rows.mean()
    loss = surrogate_loss + hp["value_loss_coef"] * value_loss - hp["entropy_coef"] * entropy.mean()
    *grads, d_mu, d_value = torch.autograd.grad(loss, params_of(ac) + [mu, value])
    row_terms = {"actor_body.6.bias": d_mu.detach(), "critic_body.6.bias": d_value.detach(),
                 "surrogate_sum": surrogate_rows.detach()[:, None], "value_sum": value_rows.detach(),
                 "kl_sum": kl[:, None]}
    return dict(grads=[g.detach() for g in grads], row_terms=row_terms, surrogate_sum=surrogate_rows.detach().sum(),
                value_sum=value_rows.detach().sum(), kl_sum=kl.sum(), surrogate_loss=surrogate_loss.detach(),
                value_loss=value_loss.detach(), kl_mean=kl.mean(), ratio=ratio.detach(), advantages=adv,
                value_minus_old=(value.detach() - target_v).squeeze(-1), logp=logp.detach(), mu=mu.detach(),
                value=value.detach(), embedding=x.detach()[:, 2 * ac.num_scalar:])


def phase1(ac, rows, idx, hp):
    """ppo.py:165-190: the regression of adaptation_module(process_obs_history(obs_history)) on the privileged
    observations over the first mb // 5 * 4 rows; gradients of encoder + adaptation module."""
    hist, priv = rows["observation_histories"][idx], rows["privileged_observations"][idx]
    num_train = int(priv.shape[0] // 5 * 4)
    pred = ac.adaptation_module(ac.process_obs_history(hist))
    sel = 0 if hp["selective"] else slice(None)
    train = F.mse_loss(pred[:num_train, sel], priv[:num_train, sel])
    with torch.no_grad():
        test = F.mse_loss(pred[num_train:, sel], priv[num_train:, sel])
        train_sum = (pred[:num_train, sel] - priv[:num_train, sel]).pow(2).sum()
        test_sum = (pred[num_train:, sel] - priv[num_train:, sel]).pow(2).sum()
    *grads, d_pred = torch.autograd.grad(train, params_of(ac, phase1_only=True) + [pred])
    return dict(grads=[g.detach() for g in grads], row_terms={"adaptation_module.4.bias": d_pred.detach()},
                train_loss=train.detach(), test_loss=test, train_sum=train_sum, test_sum=test_sum,
                num_train=num_train)


def update(ac, rows, perm, num_mini_batches, num_epochs, hp, lr):
    """PPO.update's mini-batch loop on `ac` in place (ppo_ref.update with this module's phases and slices); fresh
    Adam state for both optimizers.  Returns the eight loss means of ppo.py:206 and the final learning rate."""
    mb = perm.numel() // num_mini_batches
    ps, pa = params_of(ac), params_of(ac, phase1_only=True)
    st0 = [torch.zeros_like(flat(ps)), torch.zeros_like(flat(ps)), 0]
    st1 = [torch.zeros_like(flat(pa)), torch.zeros_like(flat(pa)), 0]
    sums = [0.0, 0.0, 0.0, 0.0]
    for _ in range(num_epochs):
        for i in range(num_mini_batches):
            idx = perm[i * mb:(i + 1) * mb]
            r = phase0(ac, rows, idx, hp)
            lr = lr_rule(lr, float(r["kl_mean"]), hp["desired_kl"])
            coef, _ = clip_coef(r["grads"], hp["max_grad_norm"])
            with torch.no_grad():
                p = flat(ps)
                st0[2] = adam_step(p, flat(r["grads"]) * coef, st0[0], st0[1], st0[2], lr, hp)
                for dst, src in zip(ps, unflat(p, ps)):
                    dst.copy_(src)
            sums[0] += float(r["value_loss"])
            sums[1] += float(r["surrogate_loss"])
            r = phase1(ac, rows, idx, hp)
            with torch.no_grad():
                p = flat(pa)
                st1[2] = adam_step(p, flat(r["grads"]), st1[0], st1[1], st1[2], hp["adaptation_lr"], hp)
                for dst, src in zip(pa, unflat(p, pa)):
                    dst.copy_(src)
            sums[2] += float(r["train_loss"])
            sums[3] += float(r["test_loss"])
    n = num_epochs * num_mini_batches
    return (sums[0] / n, sums[1] / n, sums[2] / n, 0.0, 0.0, sums[3] / n, 0.0, 0.0), lr
