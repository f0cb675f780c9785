"""Every s_waitcnt of a step kernel's decimation loop and of the code after it, with the counter it waits on, the
nearest earlier instruction that raises that counter and the distance between the two (`oldest`: the distance to
the producer a counted wait such as lgkmcnt(2) actually waits for, the third most recent one).

The step kernels run one wave per SIMD: a wait that follows its producer by a few instructions exposes the whole
LDS or scalar-cache round trip.  CPU only; reads the gfx950 code object inside a built library the way
tests/test_kernel_isa.py does, or a saved `llvm-objdump -d` text.

  python tools/wait_audit.py [LIB.so | FILE.dis] [--kernel SYMBOL_PREFIX] [--near N] [--all]

  LIB      default legged_tracking_amd/_build/libgo1_mi355x.so
  --kernel default the specialised README-config trajectory step kernel; `vel` = the velocity step kernel
  --near   the distance (instructions) up to which a wait counts as near its producer in the summary (default 8)
  --all    also list the waits in front of the loop (the prologue)

The decimation loop is the kernel's widest backward branch.  "Earlier" is by address: a producer on a path not taken
still counts, so a distance is a lower bound of what the wave sees.  vmcnt producers: loads, stores (gfx9 counts them
in vmcnt) and LDS-DMA; lgkmcnt producers: ds_* and scalar loads."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
STEP = "_Z15go1_step_kernelILb0ELi7ELb1EEvPK10go1_config"
VEL = "_Z19go1_vel_step_kernelILb0E"

Ins = collections.namedtuple("Ins", "addr op args")


def disasm(lib):
    with tempfile.TemporaryDirectory() as t:
        fb, dev = os.path.join(t, "fb.bin"), os.path.join(t, "dev.o")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fb, lib], check=True,
                       capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fb,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + dev], check=True,
                       capture_output=True)
        return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", dev], check=True, capture_output=True,
                              text=True).stdout


def kernel_body(text, name):
    """[Ins] of the first function whose symbol starts with `name` (llvm-objdump -d text)."""
    out, on = [], False
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            if on:
                break
            on = m.group(1).startswith(name)
            continue
        if not on:
            continue
        m = re.match(r"^\s+([a-z_][\w.]*)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m:
            out.append(Ins(int(m.group(3), 16), m.group(1), m.group(2)))
    return out


def branch_target(ins):
    """Address a branch goes to (simm16 dwords from the next instruction), or None."""
    if not ins.op.startswith(("s_cbranch_", "s_branch")):
        return None
    m = re.match(r"^-?\d+", ins.args)
    if not m:
        return None
    off = int(m.group(0))
    if off >= 32768:
        off -= 65536
    return ins.addr + 4 + 4 * off


def main_loop(body):
    """(first, last) instruction indices of the widest backward branch's range, or None."""
    at = {i.addr: k for k, i in enumerate(body)}
    best = None
    for k, i in enumerate(body):
        t = branch_target(i)
        if t is not None and t <= i.addr and t in at and (best is None or k - at[t] > best[1] - best[0]):
            best = (at[t], k)
    return best


def producer_class(op):
    """The counter an instruction raises: "lgkmcnt", "vmcnt" or None."""
    if op.startswith("ds_") or op.startswith(("s_load_", "s_buffer_load_")):
        return "lgkmcnt"
    if op.startswith(("global_", "buffer_", "scratch_")):
        return "vmcnt"
    if op.startswith("flat_"):
        return "vmcnt"  # (also lgkmcnt; the step kernels have none: tests/test_kernel_isa.py)
    return None


def waited(ins):
    """{counter: value} of an s_waitcnt's named counters (expcnt left out: nothing here exports)."""
    if ins.op != "s_waitcnt":
        return {}
    return {c: int(v) for c, v in re.findall(r"(vmcnt|lgkmcnt)\((\d+)\)", ins.args)}


def audit(body):
    """[(index, region, counter, value, producer index or None, distance or None, oldest distance or None)] for
    every wait, in order.  `oldest`: the distance to the producer a counted wait lets through last, i.e. the
    (value + 1)-th most recent one (counters retire in order for LDS; equal to `distance` for a wait on 0)."""
    loop = main_loop(body)
    seen = {"lgkmcnt": [], "vmcnt": []}
    rows = []
    for k, i in enumerate(body):
        region = "pre" if loop is None or k < loop[0] else ("loop" if k <= loop[1] else "post")
        for c, v in waited(i).items():
            p = seen[c][-1] if seen[c] else None
            o = seen[c][-1 - v] if len(seen[c]) > v else None
            rows.append((k, region, c, v, p, None if p is None else k - p, None if o is None else k - o))
        c = producer_class(i.op)
        if c:
            seen[c].append(k)
    return rows, loop


def report(body, near=8, show_pre=False, out=sys.stdout):
    rows, loop = audit(body)
    w = out.write
    w(f"# {len(body)} instructions")
    if loop:
        w(f"; decimation loop {body[loop[0]].addr:#x} .. {body[loop[1]].addr:#x}: {loop[1] - loop[0] + 1} instructions, "
          f"{body[loop[1]].addr + 4 - body[loop[0]].addr} bytes")
    w("\n# address  region  wait            <- nearest earlier producer (address)            distance  oldest\n")
    for k, region, c, v, p, d, o in rows:
        if region == "pre" and not show_pre:
            continue
        prod = "-" if p is None else f"{body[p].op} ({body[p].addr:#x})"
        w(f"{body[k].addr:#9x}  {region:5s}  {c + '(' + str(v) + ')':14s}  <- {prod:44s}  {'-' if d is None else d:<8}  "
          f"{'-' if o is None else o}\n")
    for region in ("loop", "post"):
        for c in ("lgkmcnt", "vmcnt"):
            ds = [o for _, r, cc, _, _, _, o in rows if r == region and cc == c and o is not None]
            if ds:
                w(f"# {region} {c}: {len(ds)} waits, {sum(d <= near for d in ds)} within {near} instructions of the "
                  f"producer they wait for (oldest), median {sorted(ds)[len(ds) // 2]}\n")
    n_sload = sum(1 for k, i in enumerate(body) if loop and loop[0] <= k <= loop[1] and i.op.startswith("s_load_"))
    w(f"# scalar loads inside the loop: {n_sload}\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src", nargs="?", default=os.path.join(REPO, "legged_tracking_amd", "_build", "libgo1_mi355x.so"))
    ap.add_argument("--kernel", default=STEP)
    ap.add_argument("--near", type=int, default=8)
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()
    name = VEL if a.kernel == "vel" else a.kernel
    text = open(a.src).read() if not a.src.endswith(".so") else disasm(a.src)
    body = kernel_body(text, name)
    if not body:
        sys.exit(f"no kernel {name}* in {a.src}")
    print(f"# {os.path.basename(a.src)}: {name}")
    report(body, a.near, a.all)
