"""Compare the device code of two builds of one HIP source, kernel by kernel: the check behind a change that must
not move a kernel (profiles/ppo_split/asm_diff.txt, profiles/r09/learn_asm_diff.txt).

Both inputs are the assembly of `hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S`.
Per kernel (every symbol with an .amdhsa_kernel block): the instruction text from the kernel's label to its end
label, with comments and the function index of local labels stripped, and the .amdhsa_* block.  Exit status 1 when a
kernel is missing on either side or differs.

Usage: python tools/asm_diff.py BEFORE.s AFTER.s
"""
import re
import sys


def kernels(path):
    """{mangled name: (instruction lines, .amdhsa lines)}"""
    lines = open(path).read().splitlines()
    out = {}
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == name + ":")
        # the code ends where the kernel descriptor's section begins (the end label follows the descriptor)
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".section"))
        text = []
        for l in lines[start + 1:end]:
            l = re.sub(r"\s*;.*$", "", l).strip()
            l = re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+_?", r".L\1_", l)  # local labels carry the function's index
            if l:
                text.append(l)
        k0 = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", l))
        k1 = next(i for i in range(k0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        out[name] = (text, [l.strip() for l in lines[k0 + 1:k1]])
    return out


def main(before, after):
    a, b = kernels(before), kernels(after)
    print(f"{len(a)} kernels before, {len(b)} after")
    bad = sorted(set(a) ^ set(b))
    for n in bad:
        print(f"  {n}: only {'before' if n in a else 'after'}")
    for n in sorted(set(a) & set(b)):
        same_i, same_k = a[n][0] == b[n][0], a[n][1] == b[n][1]
        print(f"  {n}: instructions {'identical' if same_i else 'DIFFER'} ({len(a[n][0])} lines), "
              f".amdhsa block {'identical' if same_k else 'DIFFERS'}")
        if not (same_i and same_k):
            bad.append(n)
    print("all kernels identical" if not bad else f"{len(bad)} kernels differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
