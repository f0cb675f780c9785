"""The cases of the PPO update engine's call-by-call tests (tests/test_ppo_engine_grad.py, the plain module;
tests/test_ppo_engine_encoder_grad.py, the height-map encoder module; tests/test_gpu_ppo_replay.py, both): one
`_Case` that builds either module on a storage whose mini-batch rows populate every branch of the loss, and the
gradient metric `_compare`.  The data recipe and the metric are described in tests/test_ppo_engine_grad.py's module
docstring; nothing here runs on import, and a case needs the GPU.
"""
import contextlib
import math
import types

import numpy as np
import torch

from legged_tracking_amd import ppo_engine as PE, rollout as R, rollout_cnn as RC
from tests import ppo_ref, ppo_ref_cnn

DEV = "cuda:0"
FLOOR = 2.0 ** -24

DELTAS = (-0.5, -0.1, 0.0, 0.1, 0.5)
VOFFS = (-0.5, -0.05, 0.05, 0.5)
KL0 = 0.04  # the data's KL mean (plus actions * log(1 + 1e-5))


@contextlib.contextmanager
def _args(**over):
    """PPO_Args attributes set for the duration of a case."""
    A = R.PPO_Args
    old = {k: getattr(A, k) for k in over}
    try:
        for k, v in over.items():
            setattr(A, k, v)
        yield A
    finally:
        for k, v in old.items():
            setattr(A, k, v)


class _Case:
    """A fresh engine on a storage whose mini-batch rows populate every branch of the loss
    (tests/test_ppo_engine_grad.py's module docstring).  `encoder` None: rollout.ActorCritic on a history of `hist`
    columns, restated by tests/ppo_ref.py.  `encoder` (map shape, E, scalars, frames): rollout_cnn.ActorCritic with
    the MLP height-map encoder on `frames` frames of scalars + map values (`hist` is derived and passed as None),
    restated by tests/ppo_ref_cnn.py; history frames of N(0, 1) scalars and U(-5, 5) map values."""

    def __init__(self, hist, priv, na, mb, window=0, seed=0, encoder=None):
        if encoder:
            shape, E, S, frames = encoder
            n_map = int(np.prod(shape))
            num_obs = S + n_map
            hist = frames * num_obs
        self.ref = ref = ppo_ref_cnn if encoder else ppo_ref
        g = torch.Generator().manual_seed(1000 * seed + hist + 7 * priv + 13 * na + mb + (E if encoder else 0))
        self.hist, self.priv, self.na, self.mb = hist, priv, na, mb
        rows = self.rows = mb + max(3, mb // 7)
        torch.manual_seed(seed + 5)
        if encoder:
            args = type("A", (RC.AC_Args,), dict(height_map_shape=shape, cnn_num_embedding=E))
            ac = RC.ActorCritic(num_obs, priv, hist, na, ac_args=args)
            assert PE.encoder_supported(ac)
        else:
            ac = R.ActorCritic(70, priv, hist, na)
        with torch.no_grad():  # biases and std off their initial 0 / 1, so that each one matters
            for n, p in ac.named_parameters():
                if n.endswith("bias"):
                    p.add_(0.05 * torch.randn(p.shape, generator=g))
            ac.std.copy_(0.6 + 0.8 * torch.rand(na, generator=g))
        self.alg = alg = R.PPO(ac, device=DEV)
        perm = torch.randperm(rows, generator=g)
        at = int((perm == rows - 1).nonzero())
        if at >= mb:  # the last storage row is part of the mini-batch
            perm[[mb // 2, at]] = perm[[at, mb // 2]]
        self.idx = idx = perm[:mb].to(DEV)
        assert int(idx.max()) == rows - 1 and rows > mb
        # ---- storage: random rows, then the mini-batch's rows from the f64 forward
        if encoder:
            fr = torch.randn(rows, frames, num_obs, generator=g)
            fr[:, :, S:] = torch.rand(rows, frames, n_map, generator=g) * 10.0 - 5.0
        wide = torch.randn(1, rows, hist + (350 if window else 0), generator=g)
        if encoder:
            wide[0, :, window:window + hist] = fr.reshape(rows, hist)
        wide = wide.to(DEV)
        st = types.SimpleNamespace(num_envs=rows, num_transitions_per_env=1)
        st.observation_histories = wide[:, :, window:window + hist] if window else wide
        st.privileged_observations = (0.5 * torch.randn(1, rows, priv, generator=g)).to(DEV)
        for k, w in (("actions", na), ("mu", na), ("values", 1), ("advantages", 1), ("returns", 1),
                     ("actions_log_prob", 1)):
            setattr(st, k, torch.randn(1, rows, w, generator=g).to(DEV))
        st.sigma = (0.5 + torch.rand(1, rows, na, generator=g)).to(DEV)
        ac64 = ref.double_copy(alg.actor_critic)
        m = torch.arange(mb)
        with torch.no_grad():
            h = st.observation_histories[0, idx].double()
            pv = st.privileged_observations[0, idx].double()
            x = ac64.process_obs_history(h) if encoder else h
            mu64 = ac64.actor_body(torch.cat((x, ac64.adaptation_module(x)), -1))
            v64 = ac64.critic_body(torch.cat((x, pv), -1))
            std = ac64.std.detach()
            z = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(DEV)  # noqa: E731
            actions = (mu64 + std * z(mb, na)).float()
            logp64 = torch.distributions.Normal(mu64, std).log_prob(actions.double()).sum(-1, keepdim=True)
            delta = torch.tensor(DELTAS, dtype=torch.float64)[m % 5].to(DEV)[:, None]
            sign = torch.where(m % 2 == 0, 1.0, -1.0).double().to(DEV)[:, None]
            big = torch.where((m % 4 == 3) | (m == mb - 1), 10.0, 1.0).double().to(DEV)[:, None]
            adv = sign * big * (0.5 + z(mb, 1).abs())
            voff = torch.tensor(VOFFS, dtype=torch.float64)[m % 4].to(DEV)[:, None]
            flip = torch.where(torch.rand(mb, na, generator=g) < 0.5, -1.0, 1.0).double().to(DEV)
            sig_old = std * (1.0 + 0.01 * torch.where(m % 2 == 0, 1.0, -1.0).double().to(DEV)[:, None])
            sig_old = sig_old.expand(mb, na)
            mu_old = mu64 + flip * std * math.sqrt(2.0 * KL0 / na)
            for k, v in (("actions", actions), ("actions_log_prob", logp64 + delta), ("advantages", adv),
                         ("values", v64 + voff), ("returns", v64 + z(mb, 1)), ("mu", mu_old), ("sigma", sig_old)):
                getattr(st, k)[0, idx] = v.float()
        self.storage = alg.storage = st
        self.eng = PE.PPOEngine(alg)
        if encoder:
            assert self.eng.enc_dims and self.eng.names == ref.NAMES
        self.rows32 = ref.rows_of(st)
        self.rows64 = ref.rows_of(st, torch.float64)

    def start(self, world=1):
        """_bind, _write_hyper, pack, idx: ready for grad(0).  Returns the hyper-parameter dict of the restatement."""
        e = self.eng
        e._bind(self.storage, self.mb)
        if self.storage.observation_histories.stride(1) > self.storage.observation_histories.shape[2]:
            assert e.bufs.hist_ld > e.hist  # the window reaches the engine as a strided view, not as a copy
        e._write_hyper(R.PPO_Args, world)
        e.pack()
        e.idx.copy_(self.idx)
        return self.ref.hyper_from_args(R.PPO_Args)

    def ac64(self):
        """The engine's current parameters as a float64 module."""
        torch.cuda.synchronize()
        return self.ref.double_copy(self.alg.actor_critic)

    def split(self, flat_vec, adaptation_only=False):
        """The tensors of a flat buffer (`adaptation_only`: of the adaptation optimizer's slice)."""
        return list(self.eng._views(flat_vec, adaptation_only).values())


def _errs(g, g64):
    """(max |g - g64| / max |g64|, relative L2 error) of one tensor."""
    g, g64 = g.double().reshape(-1), g64.double().reshape(-1)
    d = g - g64
    return (float(d.abs().max() / g64.abs().max()), float(d.norm() / g64.norm()))


def _compare(tag, names, eng, yard, ref, worst, row_terms, k_grad, show=None):
    """Engine within k_grad x the yardstick (both against f64), tensor by tensor, on both metrics.  `row_terms`:
    the f64 per-row terms t[r, c] of the tensors that are plain sums over the rows; their floor is 2^-24 x the
    condition number of the sum (tests/test_ppo_engine_grad.py's module docstring).  `show`: a prefix under which
    every tensor's figures are printed."""
    bad = []
    for n, a, y, r in zip(names, eng, yard, ref):
        assert float(r.double().abs().max()) > 0.0, (tag, n)
        floors = [FLOOR, FLOOR]
        if n in row_terms:
            mag = row_terms[n].double().abs().sum(0).reshape(-1)  # sum_r |t[r, c]| per output element
            r1 = r.double().reshape(-1)
            floors = [FLOOR * max(1.0, float(mag.max() / r1.abs().max())),
                      FLOOR * max(1.0, float(mag.norm() / r1.norm()))]
        for metric, ea, ey, fl in zip(("max", "l2"), _errs(a, r), _errs(y, r), floors):
            ratio = max(ea, fl) / max(ey, fl)
            if show:
                print(f"{show} {tag}:{n}:{metric} engine {ea:.2e} yardstick {ey:.2e} ratio {ratio:.2f}")
            if ratio > worst[0]:
                worst[:] = [ratio, f"{tag}:{n}:{metric} engine {ea:.2e} yardstick {ey:.2e}"]
            if not ratio <= k_grad:
                bad.append((tag, n, metric, ea, ey))
    return bad
