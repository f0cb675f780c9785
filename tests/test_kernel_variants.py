"""Every diagnostic build of the step kernels still compiles (no GPU needed).

go1_step.hip (with the device code it shares with the velocity step: go1_device.h, the part headers it includes and
go1_step_shared.h) keeps two kinds of compile-time switches, both measurement instrumentation, never
shipped: the ablation builds of tools/abl_kernel.sh (GO1_ABL_*: a section of the kernel compiled
out, to price it in situ) and the timing / accounting builds (GO1_STAMPS: s_memtime stamps for
tools/stamps.py; GO1_ISA_MARKS: section markers for tools/isa_sections.py).  Variants that were
measured and rejected are deleted from the source, not kept behind switches.  A front-end pass
(hipcc -fsyntax-only, host and gfx950 device) per variant keeps them from rotting.  go1_velocity.hip
has the curriculum launch's stamps (GO1_VEL_STAMPS, tools/vel_stamps.py); rollout.hip and ppo_update.hip keep their
stamp builds only (GO1_POLICY_STAMPS, tools/policy_stamps.py; PPO_STAMPS, tools/xw_stamps.py).  The sources hold the
host code and include their kernels as part headers, so every scan here is over a source's include closure."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from legged_tracking_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "legged_tracking_amd", "csrc")
SRC = os.path.join(CSRC, "go1_step.hip")
# go1_step.hip and every csrc header it reaches: go1_device.h, its parts, go1_step_shared.h, ...
SCANNED = [f for f in B.include_closure([SRC]) if os.path.dirname(f) == CSRC]
VEL_SRC = os.path.join(CSRC, "go1_velocity.hip")
ROLLOUT_SRC = os.path.join(CSRC, "rollout.hip")
# the sources of libgo1_rollout.so (rollout.hip, policy_actor.hip, encoder.hip)
ROLLOUT_SRCS = [os.path.join(CSRC, s) for s in B.LIBS["libgo1_rollout.so"][0]]
PPO_SRC = os.path.join(CSRC, "ppo_update.hip")
INC = os.path.join(ROOT, "include")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _switches():
    src = "".join(open(f).read() for f in SCANNED)
    return sorted(set(re.findall(r"#\s*if(?:n?def)?\s+(?:defined\()?(GO1_(?:ABL_\w+|STAMPS|ISA_MARKS))", src)))


def test_only_diagnostic_switches_remain():
    # go1_velocity.hip with every csrc header it reaches (its parts go1_vel_step.h and go1_vel_curriculum.h among them)
    vel = [f for f in B.include_closure([VEL_SRC]) if os.path.dirname(f) == CSRC]
    assert {os.path.join(CSRC, "go1_vel_step.h"), os.path.join(CSRC, "go1_vel_curriculum.h")} <= set(vel), vel
    src = "".join(open(f).read() for f in SCANNED + [f for f in vel if f not in SCANNED])
    conds = set(re.findall(r"#\s*(?:if|ifdef|ifndef|elif)\s+(?:defined\()?(\w+)", src))
    # the diagnostic switches, and the guards of the part headers (go1_device.h's, go1_step.hip's, go1_velocity.hip's)
    allowed = {"GO1_STAMPS", "GO1_ISA_MARKS", "GO1_VEL_STAMPS", "GO1_DEVICE_H", "GO1_STEP_HIP", "GO1_VELOCITY_HIP"}
    stray = {c for c in conds if c.startswith("GO1_") and c not in allowed and not c.startswith("GO1_ABL_")}
    assert not stray, f"variant switches outside the diagnostic set: {sorted(stray)}"
    # the learn libraries and their headers: the two stamp builds and the header guards, nothing else
    # (ppo_update.hip with every csrc header it reaches: a switch in one of its parts is a switch in the engine)
    ppo = [f for f in B.include_closure([PPO_SRC]) if os.path.dirname(f) == CSRC]
    assert len(ppo) > 1, ppo
    # the three sources of libgo1_rollout.so with every csrc header they reach (rollout.hip's parts among them)
    rollout = [f for f in B.include_closure(ROLLOUT_SRCS) if os.path.dirname(f) == CSRC]
    assert {os.path.join(CSRC, h) for h in ("rollout_record.h", "policy_full.h", "policy_split.h", "rollout_colsum.h",
                                            "policy_tiles.h", "split_mfma.h")} <= set(rollout), rollout
    learn = "".join(open(f).read() for f in [*rollout, *ppo, os.path.join(INC, "go1_rollout.h"),
                                             os.path.join(INC, "go1_ppo.h")])
    conds = set(re.findall(r"#\s*(?:if|ifdef|ifndef|elif)\s+!?\s*(?:defined\s*\(?\s*)?(\w+)", learn))
    # the two stamp builds and header guards: the ABI headers', rollout.hip's parts', policy_tiles.h's, split_mfma.h's
    allowed = {"GO1_POLICY_STAMPS", "PPO_STAMPS", "GO1_ROLLOUT_H", "GO1_PPO_H", "GO1_ROLLOUT_HIP", "GO1_POLICY_TILES_H",
               "GO1_SPLIT_MFMA_H"}
    stray = {c for c in conds if c.startswith(("GO1_", "PPO_")) and c not in allowed}
    assert {"GO1_POLICY_STAMPS", "PPO_STAMPS"} <= conds and not stray, \
        f"variant switches in rollout.hip / ppo_update.hip: {sorted(stray)}"


@pytest.mark.parametrize("name", B.LIBS)
def test_every_include_is_watched_by_needs_build(name):
    """A library is rebuilt when any file it is made of changes: every quoted include reachable from its sources
    exists, lies in csrc/ or include/, and is in the set needs_build compares with the library (build.lib_files).
    The scan here is the test's own, file by file."""
    watched = set(B.lib_files(name))
    assert {os.path.join(CSRC, s) for s in B.LIBS[name][0]} <= watched
    for f in sorted(watched):
        assert os.path.isfile(f) and os.path.dirname(f) in (CSRC, INC), f
        for line in open(f):
            m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
            if m:
                inc = os.path.normpath(os.path.join(os.path.dirname(f), m.group(1)))
                assert os.path.isfile(inc), f"{f} includes a missing file: {m.group(1)}"
                assert inc in watched, f"{name} is not rebuilt when {inc} changes (included by {f})"


def test_devcheck_library_is_built_as_the_step_kernels_are_and_loads():
    """The test-only device-function library (csrc/go1_devcheck.hip, tests/devcheck.py) is a row of build.LIBS with
    the step libraries' flags, made of go1_device.h and its parts, and loads without a GPU with every launcher the
    binding names; no product source names it."""
    from tests import devcheck as D
    srcs, flags = B.LIBS[D.NAME]
    assert srcs == ["go1_devcheck.hip"] and flags == B.STEP_FLAGS
    assert os.path.join(CSRC, "go1_device.h") in B.lib_files(D.NAME)
    # the device layer: every header go1_step.hip reaches but the scaffold and the source's own kernel parts
    own = ("go1_step_shared.h", "go1_traj_step.h", "go1_traj_aux.h")
    step_parts = {f for f in SCANNED if f.endswith(".h") and os.path.basename(f) not in own}
    assert step_parts == {f for f in B.include_closure([os.path.join(CSRC, "go1_device.h")]) if os.path.dirname(f) == CSRC}
    assert step_parts <= set(B.lib_files(D.NAME))
    lib = D.lib()
    for fn in ("go1dc_pm1", "go1dc_pm2", "go1dc_softsign2", "go1dc_quat", "go1dc_solve6", "go1dc_lanes",
               "go1dc_seg_closest", "go1dc_seg_box_t", "go1dc_terrain"):
        assert getattr(lib, fn) is not None
    pkg = os.path.join(ROOT, "legged_tracking_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip")) and f not in ("build.py", "go1_devcheck.hip"):
                assert "devcheck" not in open(os.path.join(dirpath, f), errors="ignore").read(), f


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_diagnostic_builds_compile():
    variants = [([], SRC)] + [([f"-D{s}"], SRC) for s in _switches()] + [(["-DGO1_VEL_STAMPS"], VEL_SRC)]
    assert len(variants) >= 10  # 8 ablations + stamps / ISA marks + the velocity stamps
    variants += [(["-DGO1_POLICY_STAMPS"], ROLLOUT_SRC), (["-DPPO_STAMPS"], PPO_SRC)]

    def one(v):
        flags, src = v
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-ffp-contract=off",
                            *flags, src], capture_output=True, text=True, cwd="/tmp")
        errs = [l for l in r.stderr.splitlines() if "error" in l]
        return flags, r.returncode, errs[:5]

    with ThreadPoolExecutor(4) as ex:
        for flags, rc, errs in ex.map(one, variants):
            assert rc == 0, (flags, errs)
