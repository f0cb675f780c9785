"""Time the height-map encoder path of rollout_cnn at 4096 envs on the GPU, per encoder mode: the MLP encoder on the
21 x 11 map (E = 256, history of 1 and of 5 frames) and the CNN on the 61 x 31 map (E = 256, one frame).  Per case:
  encode          go1_heightmap_encode alone (two launches: MLP layers, or conv stage + linear)
  encode_policy   FusedEncoderPolicy.forward with sampling (the encode launches + go1_policy_forward): PPO.act's path
  torch           the same module's torch eager f32 act + log-prob + evaluate under inference_mode: PPO.act's
                  path without the kernels
The three are timed in alternating blocks of REPS calls between one event pair (BLOCKS blocks each, after WARM
warm-up calls); the figure is the per-call time of a block.  Also prints how far the fused outputs are from torch's.
One JSON line per case, and everything into OUT (default encoder_kernel_time.json; DESIGN section 5 quotes
profiles/encoder/encoder_kernel_time.json).

Usage: python tools/encoder_kernel_time.py [OUT]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from legged_tracking_amd import rollout_cnn as RC  # noqa: E402

DEV = "cuda:0"
N, WARM, BLOCKS, REPS = 4096, 10, 12, 10
S = 41
# split f16 MFMA work of conv2 per launch: 2 x (M 32 x K 160 padded x 420 pooled-in pixels padded to 27 tiles of
# 16) x 3 products x N envs
CONV2_FLOP = 2 * 32 * 160 * (27 * 16) * 3 * N


def case(name, shape, use_cnn, H, E=256):
    torch.manual_seed(0)
    args = type("A", (RC.AC_Args,), dict(use_cnn=use_cnn, height_map_shape=shape, cnn_num_embedding=E))
    num_obs = S + int(np.prod(shape))
    ac = RC.ActorCritic(num_obs, 2, H * num_obs, 12, ac_args=args).to(DEV)
    assert RC.FusedEncoderPolicy.supported(ac)
    pol = RC.FusedEncoderPolicy(ac)
    g = torch.Generator(device=DEV).manual_seed(1)
    hist = torch.randn(N, H, num_obs, device=DEV, generator=g)
    hist[:, :, S:] = torch.rand(N, H, num_obs - S, device=DEV, generator=g) * 0.06 - 0.03  # the env's clipped heights
    hist = hist.reshape(N, -1)
    priv = torch.randn(N, 2, device=DEV, generator=g)

    def torch_path():
        a = ac.act(hist)
        return a, ac.get_actions_log_prob(a), ac.evaluate(hist, priv)

    paths = {"encode": lambda: pol.encode(hist),
             "encode_policy": lambda: pol.forward(hist, priv, sample=(5, 1, 0)),
             "torch": torch_path}
    us = {k: [] for k in paths}
    with torch.inference_mode():
        for f in paths.values():
            for _ in range(WARM):
                f()
        torch.cuda.synchronize()
        for _ in range(BLOCKS):
            for k, f in paths.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(REPS):
                    f()
                b.record()
                torch.cuda.synchronize()
                us[k].append(a.elapsed_time(b) * 1e3 / REPS)
        mean, value, latent = pol.forward(hist, priv)
        pt = ac.process_obs_history(hist)
        lt = ac.adaptation_module(pt)
        mt = ac.actor_body(torch.cat((pt, lt), -1))
        vt = ac.critic_body(torch.cat((pt, priv), -1))
        err = {k: float((a - b).abs().max() / b.abs().max())
               for k, a, b in (("policy_input", pol.encode(hist), pt), ("mean", mean, mt), ("value", value, vt))}
    out = {"case": name, "map": list(shape), "mode": "cnn" if use_cnn else "mlp", "E": E, "H": H, "n_envs": N,
           "overflow": int(pol.overflow.item()), "max_err_over_scale_vs_torch_f32": err}
    for k, v in us.items():
        v = np.array(v)
        out[k] = {"us_median": float(np.median(v)), "us_min": float(v.min()), "us_max": float(v.max())}
    out["fused_beats_torch"] = out["encode_policy"]["us_median"] < out["torch"]["us_median"]
    if use_cnn:
        out["conv2_split_mfma_gflop_per_launch"] = CONV2_FLOP / 1e9
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("encoder_kernel_time.py measures on the GPU: no GPU visible")
    res = [case("mlp 21x11 H=1", (2, 21, 11), False, 1),
           case("mlp 21x11 H=5", (2, 21, 11), False, 5),
           case("cnn 61x31 H=1", (2, 61, 31), True, 1),
           case("mlp 21x11 H=1, again", (2, 21, 11), False, 1)]
    out = sys.argv[1] if len(sys.argv) > 1 else "encoder_kernel_time.json"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0), "n_envs": N,
               "method": f"one torch.cuda.Event pair around {REPS} calls, {BLOCKS} blocks per path, the paths "
                         f"alternating, after {WARM} warm-up calls each; per-call microseconds",
               "cases": res}, open(out, "w"), indent=1)
