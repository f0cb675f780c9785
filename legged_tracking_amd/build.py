"""Build the HIP C-ABI libraries for gfx950 in-tree (legged_tracking_amd/_build)."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(HERE, "_build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off"]

# The step kernel is VALU-issue bound.  One wave issues a v_pk_fma_f32 (two FMAs) as fast
# as a v_fma_f32 (tools/probes/pk_rate.hip), so the kernel packs by hand where the data
# pair up naturally (f2 types); the SLP auto-vectoriser stays off: its packing of scalar
# code adds register-pair moves that cost more than they save (measured -3 %).
STEP_FLAGS = ["-fno-slp-vectorize"]

# name -> (sources, extra flags); the headers a library depends on are derived from its sources (lib_files)
LIBS = {
    "libgo1_mi355x.so": (["go1_step.hip", "go1_terrain.hip"], STEP_FLAGS),
    "libgo1_rollout.so": (["rollout.hip", "policy_actor.hip", "encoder.hip"], []),
    "libgo1_ppo.so": (["ppo_update.hip"], []),
    # kernel-argument preloading: the curriculum launch's leading scalar arguments arrive in SGPRs with the wave
    # (11.75-11.78 against 12.02-12.10 us average per launch, alternating runs of one session)
    "libgo1_velocity.so": (["go1_velocity.hip"], STEP_FLAGS + ["-mllvm", "-amdgpu-kernarg-preload-count=16"]),
    # the ray caster behind the recording API (render.py); it shares no file with the step libraries
    "libgo1_render.so": (["go1_render.hip"], []),
    # the episode tracer (trace.py): a library of its own, so the render and step ABIs and their size checks stay put
    "libgo1_trace.so": (["go1_trace.hip"], []),
    # the local target planner (plan.py): one launch after the step kernel, built as the step kernels are because it
    # shares their torch-order math (go1_torch_math.h) bit for bit; with the render / trace libraries it has only go1_host.h in common
    "libgo1_plan.so": (["go1_plan.hip"], STEP_FLAGS),
    # the after-start domain randomiser (randomize.py): one launch after the step kernel, built with the planner's
    # flags: it uses the step kernels' Philox and clampf, and its u * range + lo must stay a multiply and an add
    "libgo1_dr.so": (["go1_dr.hip"], STEP_FLAGS),
    # the privileged-observation assembler (privileged.py): one launch after the step kernel, built with the
    # randomiser's flags: its (x - shift) * scale must stay a subtraction and a multiply.  Its only files are its own
    # source and header (no go1_host.h: see the note in go1_priv.hip)
    "libgo1_priv.so": (["go1_priv.hip"], STEP_FLAGS),
    # test-only: one thin kernel per device function of go1_device.h (tests/devcheck.py), built as the step kernels are
    "libgo1_devcheck.so": (["go1_devcheck.hip"], STEP_FLAGS),
}
OUT = os.path.join(BUILD, "libgo1_mi355x.so")  # the step library (kept for callers of build())


def include_closure(paths):
    """The files and everything their quoted #include "..." lines reach, transitively, in first-reached order.
    A text scan (conditional includes count too); system <...> headers are not followed."""
    seen, todo = [], [os.path.normpath(p) for p in paths][::-1]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.append(f)
        incs = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(f).read(), re.M)
        todo += [os.path.normpath(os.path.join(os.path.dirname(f), i)) for i in incs][::-1]
    return seen


def lib_files(name):
    """Every file library `name` is made of: its sources and their include closure (csrc/ and include/)."""
    return include_closure(os.path.join(CSRC, s) for s in LIBS[name][0])


def needs_build(name):
    out = os.path.join(BUILD, name)
    if not os.path.exists(out):
        return True
    return any(os.path.getmtime(d) > os.path.getmtime(out) for d in lib_files(name))


def build(force=False, verbose=False, names=None):
    os.makedirs(BUILD, exist_ok=True)
    for name in names or LIBS:
        if not force and not needs_build(name):
            continue
        srcs, flags = LIBS[name]
        cmd = [HIPCC, *FLAGS, *flags, "-o", os.path.join(BUILD, name), *(os.path.join(CSRC, s) for s in srcs)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        # the device-only feature flag is also seen (and ignored) by the host pass
        err = "\n".join(l for l in r.stderr.splitlines() if "not a recognized feature" not in l)
        if err.strip():
            print(err, file=sys.stderr)
        if r.returncode != 0:
            raise subprocess.CalledProcessError(r.returncode, cmd)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
