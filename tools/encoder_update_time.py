"""Time one PPO.update of the height-map encoder module (rollout_cnn.ActorCritic, MLP encoder on the 21 x 11 map,
503-observation frames) at 4096 envs x 24 steps, with a history of H = 1 and of H = 5 frames, on its two paths:
  engine   the HIP update engine (csrc/ppo_update.hip, go1_ppo_dims.enc_mode 1; GO1_PPO_ENCODER_ENGINE=1): one
           encoder pass on the last frame per phase, the mini-batch captured into a HIP graph
  torch    the torch autograd update, eager (the switch off: rollout_cnn.ENGINE_DEFAULT's path): every frame through
           the encoder three times per mini-batch
Both run PPO_Args' defaults (num_learning_epochs x num_mini_batches mini-batches) on the same storage contents, on
two copies of the same module.  Wall clock around PPO.update (it ends by reading the loss sums back, a device
synchronisation); the two paths alternate, BLOCKS timed updates each after WARM warm-up updates each (the engine's
first update captures its graph); the first case is measured again last.  One JSON line per case, everything into
OUT (default encoder_update_time.json; DESIGN section 5 quotes profiles/encoder/encoder_update_time.json).

Usage: python tools/encoder_update_time.py [OUT]"""
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from legged_tracking_amd import ppo_engine as PE, rollout as R, rollout_cnn as RC  # noqa: E402

DEV = "cuda:0"
N, T, WARM, BLOCKS = 4096, 24, 2, 7
S, SHAPE, E, PRIV, NA = 41, (2, 21, 11), 256, 2, 12


def _fill(st, ac, H, num_obs, g):
    """Storage contents of the right scale: N(0, 1) scalars, the env's clipped heights, old statistics near the
    module's own so that the ratios stay near 1."""
    h = torch.randn(T, N, H, num_obs, device=DEV, generator=g)
    h[..., S:] = torch.rand(T, N, H, num_obs - S, device=DEV, generator=g) * 0.06 - 0.03
    st.observation_histories.copy_(h.reshape(T, N, -1))
    st.observations.copy_(h[:, :, -1])
    st.privileged_observations.copy_(torch.randn(T, N, PRIV, device=DEV, generator=g))
    with torch.no_grad():
        for t in range(T):
            hist, priv = st.observation_histories[t], st.privileged_observations[t]
            ac.update_distribution(hist)
            mu, sigma = ac.action_mean, ac.action_std
            a = mu + sigma * torch.randn(N, NA, device=DEV, generator=g)
            st.actions[t], st.mu[t], st.sigma[t] = a, mu, sigma
            st.actions_log_prob[t] = ac.get_actions_log_prob(a)[:, None]
            v = ac.evaluate(hist, priv)
            st.values[t] = v
            st.returns[t] = v + 0.1 * torch.randn(N, 1, device=DEV, generator=g)
    st.advantages.copy_(torch.randn(T, N, 1, device=DEV, generator=g))


def case(name, H):
    torch.manual_seed(0)
    args = type("A", (RC.AC_Args,), dict(use_cnn=False, height_map_shape=SHAPE, cnn_num_embedding=E))
    num_obs = S + int(np.prod(SHAPE))
    ac = RC.ActorCritic(num_obs, PRIV, H * num_obs, NA, ac_args=args).to(DEV)
    assert PE.encoder_supported(ac)
    algs = {}
    g = torch.Generator(device=DEV).manual_seed(1)
    for k in ("engine", "torch"):
        alg = algs[k] = R.PPO(copy.deepcopy(ac), device=DEV, kernels=R.HipRolloutKernels())
        alg.init_storage(N, T, [num_obs], [PRIV], [H * num_obs], [NA])
        if k == "engine":
            _fill(alg.storage, ac, H, num_obs, g)
        else:
            for f in ("observation_histories", "observations", "privileged_observations", "actions", "mu", "sigma",
                      "actions_log_prob", "values", "returns", "advantages"):
                getattr(alg.storage, f).copy_(getattr(algs["engine"].storage, f))

    def run(k):
        os.environ["GO1_PPO_ENCODER_ENGINE"] = "1" if k == "engine" else "0"
        alg = algs[k]
        alg.storage.step = T
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = alg.update()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert (alg._engine is not None) == (k == "engine")
        assert np.isfinite(np.array([float(x) for x in out])).all(), (k, out)
        return dt * 1e3

    ms = {k: [] for k in algs}
    for _ in range(WARM):
        for k in algs:
            run(k)
    for _ in range(BLOCKS):
        for k in algs:
            ms[k].append(run(k))
    A = R.PPO_Args
    out = {"case": name, "map": list(SHAPE), "E": E, "H": H, "n_envs": N, "steps": T,
           "mini_batches": A.num_learning_epochs * A.num_mini_batches, "mb_rows": N * T // A.num_mini_batches,
           "engine_graphed": algs["engine"]._engine.graphs is not None}
    for k, v in ms.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max())}
    out["torch_over_engine"] = out["torch"]["ms_median"] / out["engine"]["ms_median"]
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("encoder_update_time.py measures on the GPU: no GPU visible")
    res = [case("mlp 21x11 H=1", 1), case("mlp 21x11 H=5", 5), case("mlp 21x11 H=1, again", 1)]
    out = sys.argv[1] if len(sys.argv) > 1 else "encoder_update_time.json"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0),
               "method": f"wall clock around PPO.update (ends in a device synchronisation), {BLOCKS} updates per path, "
                         f"the paths alternating, after {WARM} warm-up updates each; milliseconds per update",
               "cases": res}, open(out, "w"), indent=1)
