"""Time go1_policy_forward in its three modes (full / student / teacher), both variants, at 4096 and 65,536 envs, and
the play / evaluate policy step (torch eager ac.act against rollout.fused_inference) for the three checkpoint kinds.

  python tools/policy_modes_bench.py [--other-lib PATH] [--json FILE] [--skip-steps]

tools/policy_bench.py's method: device events around LAUNCHES back-to-back launches after WARMUP untimed ones, in
microseconds per launch.  Every configuration is timed REPEATS times, the configurations of one size alternating
within each repeat, and reported as median [min .. max]: the spread of mode 0 is the yardstick the other modes are
read against.  --other-lib times mode 0 of another build of libgo1_rollout.so (e.g. the parent commit's) in the same
alternation; it is called through the raw C ABI, so a build without the trailing `mode` field runs too."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from legged_tracking_amd import learn_abi as LA, rollout as R, rollout_cnn as RC  # noqa: E402

WARMUP, LAUNCHES, REPEATS = 20, 200, 7
DEV = torch.device("cuda", 0)


def timed(fn, launches=LAUNCHES):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for k in range(launches):
        fn(k)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / launches * 1000.0


def alternate(configs, launches=LAUNCHES):
    """{name: fn(k)} -> {name: [us per launch] x REPEATS}, the configurations alternating within each repeat."""
    for fn in configs.values():
        for k in range(WARMUP):
            fn(k)
    torch.cuda.synchronize()
    out = {k: [] for k in configs}
    for _ in range(REPEATS):
        for name, fn in configs.items():
            out[name].append(timed(fn, launches))
    return out


def show(title, res):
    print(title)
    for k, v in res.items():
        print(f"  {k:34s} {statistics.median(v):8.2f} us  [{min(v):.2f} .. {max(v):.2f}]")


def kernel_times(other_lib):
    ac = R.ActorCritic(261, 2, 261, 12).to(DEV)
    pol = R.FusedPolicy(ac)
    other = None
    if other_lib:
        other = C.CDLL(other_lib)
        other.go1_policy_forward.argtypes = [C.POINTER(LA.PolicyArgs), C.c_void_p]
    results = {}
    for n in (4096, 65536):
        obs, priv = torch.randn(n, 261, device=DEV), torch.randn(n, 2, device=DEV)
        configs = {}
        for variant in (0, 1):
            for mode, name in ((0, "full"), (1, "student"), (2, "teacher")):
                def fn(k, variant=variant, mode=mode):
                    pol.variant = variant
                    pol.forward(obs, priv, sample=(1, k, 0), mode=mode)
                configs[f"variant {variant} {name}"] = fn
            if other is not None:  # the same host path, the launch through the other build's entry point
                def fo(k, variant=variant):
                    pol.variant, pol._forward = variant, other.go1_policy_forward
                    try:
                        pol.forward(obs, priv, sample=(1, k, 0))
                    finally:
                        pol._forward = pol.lib.go1_policy_forward
                configs[f"variant {variant} full (other lib)"] = fo
        with torch.inference_mode():
            results[n] = alternate(configs)
        show(f"go1_policy_forward, {n} envs (hist 261, 2 privileged, in-kernel sampling)", results[n])
    return results


def _encoder_module(shape, use_cnn, history):
    args = type("A", (RC.AC_Args,), dict(use_cnn=use_cnn, height_map_shape=shape, cnn_num_embedding=256))
    num_obs = 41 + int(np.prod(shape))
    return RC.ActorCritic(num_obs, 2, history * num_obs, 12, ac_args=args).to(DEV)


def step_times(n=4096):
    """The policy step of play / evaluate: ac.act(obs_history) in torch eager (what play ran before) against
    fused_inference's sampled student step, for the three checkpoint kinds."""
    kinds = {"ppo_cse (261-wide history)": R.ActorCritic(261, 2, 261, 12).to(DEV),
             "ppo_cse_cnn MLP (15 frames of 503)": _encoder_module((2, 21, 11), False, 15),
             "ppo_cse_cnn CNN (1 frame of 3823)": _encoder_module((2, 61, 31), True, 1)}
    results = {}
    for name, ac in kinds.items():
        ac.eval()
        ob = {"obs_history": torch.randn(n, ac.num_obs_history, device=DEV),
              "privileged_obs": torch.randn(n, 2, device=DEV)}
        pol = R.fused_inference(ac, sample=1)
        assert pol.fused is not None, name
        with torch.no_grad():
            results[name] = alternate({"torch eager ac.act": lambda k: ac.act(ob["obs_history"]),
                                       "fused_inference": lambda k: pol(ob)}, launches=50)
        show(f"policy step, {n} envs: {name}", results[name])
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    out = {"kernel_us": {str(k): v for k, v in kernel_times(a.other_lib).items()}}
    if not a.skip_steps:
        out["step_us"] = step_times()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
