"""Time one PPO.update of the height-map encoder module (rollout_cnn.ActorCritic) at 4096 envs x 24 steps, with a
history of H = 1 and of H = 5 frames, for the MLP encoder on the 21 x 11 map (503-observation frames; the default)
or the CNN encoder on the 61 x 31 map (`cnn`), on its two paths:
  engine   the HIP update engine (csrc/ppo_update.hip, go1_ppo_dims.enc_mode 1 / 3; GO1_PPO_ENCODER_ENGINE=1): one
           encoder pass on the last frame per phase, the mini-batch captured into a HIP graph
  torch    the torch autograd update, eager (the switch off: rollout_cnn.ENGINE_DEFAULT's path): every frame through
           the encoder three times per mini-batch
Both run PPO_Args' defaults (num_learning_epochs x num_mini_batches mini-batches) on the same storage contents, on
two copies of the same module.  Wall clock around PPO.update (it ends by reading the loss sums back, a device
synchronisation); the two paths alternate, BLOCKS timed updates each after WARM warm-up updates each (the engine's
first update captures its graph); the first case is measured again last.  One JSON line per case, everything into
OUT (default encoder_update_time.json; DESIGN section 5 quotes profiles/encoder/encoder_update_time.json and, for
the CNN, profiles/encoder/encoder_update_time_cnn.json).

Usage: python tools/encoder_update_time.py [OUT [mlp | cnn [H,H,... [engine | torch]]]]
(the histories to time, default 1,5,1; one path alone, default both, alternating)"""
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
S, E, PRIV, NA = 41, 256, 2, 12
SHAPES = {"mlp": (2, 21, 11), "cnn": (2, 61, 31)}


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


def case(name, H, kind="mlp", paths=("engine", "torch")):
    torch.manual_seed(0)
    SHAPE = SHAPES[kind]
    args = type("A", (RC.AC_Args,), dict(use_cnn=kind == "cnn", height_map_shape=SHAPE, cnn_num_embedding=E))
    num_obs = S + int(np.prod(SHAPE))
    ac = RC.ActorCritic(num_obs, PRIV, H * num_obs, NA, ac_args=args).to(DEV)
    assert PE.conv_encoder_supported(ac) if kind == "cnn" else PE.encoder_supported(ac)
    algs = {}
    g = torch.Generator(device=DEV).manual_seed(1)
    for k in paths:
        alg = algs[k] = R.PPO(copy.deepcopy(ac), device=DEV, kernels=R.HipRolloutKernels())
        alg.init_storage(N, T, [num_obs], [PRIV], [H * num_obs], [NA])
        if k == paths[0]:
            _fill(alg.storage, ac, H, num_obs, g)
        else:
            for f in ("observation_histories", "observations", "privileged_observations", "actions", "mu", "sigma",
                      "actions_log_prob", "values", "returns", "advantages"):
                getattr(alg.storage, f).copy_(getattr(algs[paths[0]].storage, f))

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
        print(f"  {name}: {k} {dt * 1e3:.1f} ms", file=sys.stderr, flush=True)  # progress: a slow case shows where
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
           "engine_graphed": "engine" in algs and algs["engine"]._engine.graphs is not None}
    for k, v in ms.items():
        v = np.array(v)
        out[k] = {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max())}
    if len(algs) == 2:
        out["torch_over_engine"] = out["torch"]["ms_median"] / out["engine"]["ms_median"]
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    kind = sys.argv[2] if len(sys.argv) > 2 else "mlp"
    if kind not in SHAPES:
        raise SystemExit(f"unknown encoder {kind!r}\nUsage: python tools/encoder_update_time.py [OUT [mlp | cnn [H,H,...]]]")
    if not torch.cuda.is_available():
        raise SystemExit("encoder_update_time.py measures on the GPU: no GPU visible")
    tag = f"{kind} {SHAPES[kind][1]}x{SHAPES[kind][2]}"
    out = sys.argv[1] if len(sys.argv) > 1 else "encoder_update_time.json"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    res = []
    hs = [int(h) for h in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 5, 1]
    paths = (sys.argv[4],) if len(sys.argv) > 4 and sys.argv[4] in ("engine", "torch") else ("engine", "torch")
    for i, H in enumerate(hs):
        res.append(case(f"{tag} H={H}" + (", again" if H in hs[:i] else ""), H, kind, paths))
        # written after every case: a run that is cut short keeps what it measured
        json.dump({"device": torch.cuda.get_device_name(0),
                   "method": f"wall clock around PPO.update (ends in a device synchronisation), {BLOCKS} updates per "
                             f"path, the paths alternating, after {WARM} warm-up updates each; milliseconds per update",
                   "cases": res}, open(out, "w"), indent=1)
