"""Fixture of the reference's own numpy quaternion / Euler formulas (container-only test infrastructure).

go1_gym/utils/planner.py:17-78 holds numpy copies of the isaacgym.torch_utils functions the fixtures'
stub restates (quat_apply, quat_from_euler_xyz, quat_apply_inverse, get_euler_xyz, copysign).
planner.py imports ompl (absent), so the five functions are extracted from its source with `ast` and
compiled alone; nothing else of the module runs.  They are evaluated in float64 on the seeded inputs of
tests/test_oracle_math.py and only their outputs are recorded.

Usage: python tests/golden/make_golden_math.py [reference root]   (writes tests/golden/planner_math.npz)
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import test_oracle_math as TM  # noqa: E402

NAMES = ("quat_apply", "quat_from_euler_xyz", "quat_apply_inverse", "get_euler_xyz", "copysign")


def planner_funcs(path):
    tree = ast.parse(open(path).read(), path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(f.name for f in fns) == sorted(NAMES)
    ns = {"np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)  # noqa: S102 - five pure-numpy functions
    return ns


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GO1_REFERENCE_ROOT", "")
    P = planner_funcs(os.path.join(root, "go1_gym", "utils", "planner.py"))
    q, v = TM.apply_inputs()
    q2, r, p, y = TM.euler_inputs()
    with np.errstate(invalid="ignore"):  # arcsin past 1 on the gimbal rows is selected away by np.where
        euler = np.stack(P["get_euler_xyz"](q2))
    out = {"quat_apply": P["quat_apply"](q, v), "quat_apply_inverse": P["quat_apply_inverse"](q, v),
           "get_euler_xyz": euler, "quat_from_euler_xyz": P["quat_from_euler_xyz"](r, p, y)}
    out = {k: np.asarray(a, np.float64) for k, a in out.items()}
    np.savez(os.path.join(HERE, "planner_math.npz"), **out)
    print("wrote planner_math.npz", {k: a.shape for k, a in out.items()})


if __name__ == "__main__":
    main()
