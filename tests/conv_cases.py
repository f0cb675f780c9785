"""The cases of the PPO update engine's CNN encoder tests (tests/test_ppo_engine_conv_grad.py): tests/ppo_cases._Case's
storage recipe on rollout_cnn.ActorCritic with use_cnn, with the mini-batch's maps screened (tests/conv_ref.py: no
pool winner and no ReLU sign decided within rounding) at the parameters of BOTH phases.  Phase 1 runs at the
parameters phase 0's step leaves, so every round of the screen takes that step in f64 (tests/ppo_ref_conv.py) and
screens the maps under the stepped filters as well; an unsafe row's map is redrawn from the seeded stream (four
candidates per round, the first safe one taken), the mini-batch's storage rows are derived again from the f64
forward, and the screen repeats (40 rounds at most; a screen that does not converge fails the test).

Phase 0's step starts from preset Adam moments at step 999 (`preset`, which the test loads into the engine before
step(0)), not from a fresh optimizer.  A fresh Adam's first step is lr x sign(g) per weight: a redrawn row flips the
sign of some filter gradients, those filters jump by 2 lr = 2e-3, every pre-activation of every row moves by ~1e-2
against decision margins of ~1e-5, and the rows that were safe are unsafe again: measured, the screen of the
5-row case did not converge in 40 rounds that way.  With moments of ~100 behind the step the stepped filters depend
on the mini-batch's gradient (<= 1e-2 after the clip) by ~1e-8, the same for every redraw, while the step itself
still moves each filter by ~lr.  Nothing here runs on import, and a case needs the GPU.
"""
import math
import types

import torch

from legged_tracking_amd import ppo_engine as PE, rollout as R, rollout_cnn as RC
from tests import conv_ref, ppo_ref_conv as ref
from tests.ppo_cases import DELTAS, DEV, KL0, VOFFS

S = 41  # scalars of a frame (tests/cnn_cases.py)
N_MAP = conv_ref.N_MAP
CONV = ["height_map_encoder.model.%d.%s" % (i, k) for i in (0, 3) for k in ("weight", "bias")]


def tie_rows():
    return conv_ref.tie_maps()


class TieRowUnsafe(AssertionError):
    """Under this case's filters a tie row has a decision within rounding besides its exact ties: another seed."""


class ConvCase:
    """A fresh engine on a storage whose mini-batch rows populate every branch of the loss.  `ties`: the first three
    mini-batch rows carry conv_ref.tie_maps() (screened like the others: exact ties of identical patches pass)."""

    def __init__(self, E, frames, priv, na, mb, window=0, seed=0, ties=False, screen=True):
        num_obs = S + N_MAP
        hist = frames * num_obs
        g = torch.Generator().manual_seed(1000 * seed + hist + 7 * priv + 13 * na + mb + E)
        self.hist, self.priv, self.na, self.mb, self.ref = hist, priv, na, mb, ref
        rows = self.rows = mb + max(3, mb // 7)
        torch.manual_seed(seed + 5)
        args = type("A", (RC.AC_Args,), dict(height_map_shape=conv_ref.MAP, cnn_num_embedding=E, use_cnn=True))
        ac = RC.ActorCritic(num_obs, priv, hist, na, ac_args=args)
        assert PE.conv_encoder_supported(ac)
        with torch.no_grad():  # biases and std off their initial values, so that each one matters
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
        fr = torch.randn(rows, frames, num_obs, generator=g)
        fr[:, :, S:] = torch.rand(rows, frames, N_MAP, generator=g) * 10.0 - 5.0
        if ties:
            fr[perm[:3], -1, S:] = tie_rows()
        wide = torch.randn(1, rows, hist + (350 if window else 0), generator=g).to(DEV)
        st = types.SimpleNamespace(num_envs=rows, num_transitions_per_env=1)
        st.observation_histories = wide[:, :, window:window + hist] if window else wide
        st.privileged_observations = (0.5 * torch.randn(1, rows, priv, generator=g)).to(DEV)
        for k, w in (("actions", na), ("mu", na), ("values", 1), ("advantages", 1), ("returns", 1),
                     ("actions_log_prob", 1)):
            setattr(st, k, torch.randn(1, rows, w, generator=g).to(DEV))
        st.sigma = (0.5 + torch.rand(1, rows, na, generator=g)).to(DEV)
        self.storage = alg.storage = st
        hp = ref.hyper_from_args(R.PPO_Args)
        ac64 = ref.double_copy(alg.actor_critic)
        self.unsafe_first, self.rounds, self.preset = None, 0, None
        if screen:
            n = sum(p.numel() for p in ac.parameters())
            self.preset = (100.0 * torch.randn(n, generator=g), 1.0e4 * (0.5 + torch.rand(n, generator=g)))

        def unsafe(maps):
            return (conv_ref.unsafe_rows(maps, *self._filters(ac64)) |
                    conv_ref.unsafe_rows(maps, *self._filters(self._stepped(ac64, hp)))).cpu()

        for self.rounds in range(40 if screen else 1):
            st.observation_histories[0] = fr.reshape(rows, hist).to(DEV)
            self._derive(ac64, g)
            if not screen:
                break
            bad = unsafe(fr[perm[:mb], -1, S:].to(DEV))
            if ties:
                if bool(bad[:3].any()):
                    raise TieRowUnsafe(f"seed {seed}: a tie row is unsafe beyond its exact ties")
            if self.unsafe_first is None:
                self.unsafe_first = int(bad.sum())
            if not bool(bad.any()):
                break
            nb = int(bad.sum())
            cand = torch.rand(4, nb, N_MAP, generator=g) * 10.0 - 5.0
            ok = ~unsafe(cand.reshape(4 * nb, N_MAP).to(DEV)).reshape(4, nb)
            first = torch.where(ok.any(0), ok.int().argmax(0), 3)  # the first safe candidate, else the last one
            fr[perm[:mb][bad], -1, S:] = cand[first, torch.arange(nb)]
        else:
            raise AssertionError("the decision screen did not converge in 40 rounds")
        self.eng = PE.PPOEngine(alg)
        assert self.eng.enc_dims["enc_mode"] == 3 and self.eng.names == ref.NAMES
        self.rows32 = ref.rows_of(st)
        self.rows64 = ref.rows_of(st, torch.float64)

    @staticmethod
    def _filters(ac):
        sd = dict(ac.named_parameters())
        return [sd[n].detach() for n in CONV]

    def _stepped(self, ac64, hp):
        """A copy of ac64 after phase 0's optimizer step in f64 from the preset moments at step 999."""
        new = ref.double_copy(ac64)
        ps = ref.params_of(new)
        r = ref.phase0(new, ref.rows_of(self.storage, torch.float64), self.idx, hp)
        lr = ref.lr_rule(float(self.alg.learning_rate), float(r["kl_mean"]), hp["desired_kl"])
        coef, _ = ref.clip_coef(r["grads"], hp["max_grad_norm"])
        with torch.no_grad():
            p = ref.flat(ps)
            m, v = (t.double().to(p.device) for t in self.preset)
            ref.adam_step(p, ref.flat(r["grads"]) * coef, m, v, 999, lr, hp)
            for dst, src in zip(ps, ref.unflat(p, ps)):
                dst.copy_(src)
        return new

    def _derive(self, ac64, g):
        """The mini-batch's storage rows from the f64 forward (tests/ppo_cases._Case)."""
        st, idx, mb, na = self.storage, self.idx, self.mb, self.na
        m = torch.arange(mb)
        with torch.no_grad():
            h = st.observation_histories[0, idx].double()
            pv = st.privileged_observations[0, idx].double()
            x = ac64.process_obs_history(h)
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

    def start(self, world=1):
        """_bind, _write_hyper, pack, idx: ready for grad(0).  Returns the hyper-parameter dict of the restatement."""
        e = self.eng
        e._bind(self.storage, self.mb)
        if self.storage.observation_histories.stride(1) > self.storage.observation_histories.shape[2]:
            assert e.bufs.hist_ld > e.hist  # the window reaches the engine as a strided view, not as a copy
        e._write_hyper(R.PPO_Args, world)
        e.pack()
        e.idx.copy_(self.idx)
        if self.preset:  # the main optimizer's state the screen assumed (the module docstring)
            e.steps[0] = 999.0
            e.exp_avg.copy_(self.preset[0])
            e.exp_avg_sq.copy_(self.preset[1])
        return ref.hyper_from_args(R.PPO_Args)

    def ac64(self):
        """The engine's current parameters as a float64 module."""
        torch.cuda.synchronize()
        return ref.double_copy(self.alg.actor_critic)

    def split(self, flat_vec, adaptation_only=False):
        return list(self.eng._views(flat_vec, adaptation_only).values())
