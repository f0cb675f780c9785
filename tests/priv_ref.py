"""Numpy restatement of the privileged-observation assembler (include/go1_priv.h): what one go1_priv_step launch writes,
in f32 with a separate subtraction and multiply (or the f32 division), from a column table and the planes.  The fixture
tests/golden/priv_cases.npz (tests/golden/make_golden_priv.py: the reference's own compute_observations) pins it; the GPU
tests compare the kernel and the env with it."""
import os
import types

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "priv_cases.npz")
SETS = ("defaults", "train", "all", "sparse")
WIDTHS = dict(defaults=6, train=2, all=45, sparse=18)
# the header's source ids 1 .. 7 and the columns a plane needs at least
PLANES = ("friction", "restitution", "payloads", "motor_strength", "motor_offset", "root", "aux")
SRC_ZERO, SRC_GRAVITY = 0, 8
OP_MUL, OP_DIV, OP_RAW = 0, 1, 2
# fixture array of each plane (aux: its columns 0:3 are base_lin_vel)
FIXTURE_PLANES = dict(friction="friction", restitution="restitution", payloads="payloads",
                      motor_strength="motor_strength", motor_offset="motor_offset", root="root", aux="base_lin_vel")


def load():
    """The fixture as {array name: array}; per-set arrays are named "<set>/<name>"."""
    z = np.load(CASES)
    return {k: z[k] for k in z.files}


def cfg_of(d, name):
    """A Cfg-like namespace with set `name`'s priv_observe_* flags and the fixture's normalisation ranges."""
    env = types.SimpleNamespace(**{str(k): bool(v) for k, v in zip(d["flag_names"], d[name + "/flags"])})
    env.num_privileged_obs = int(d[name + "/priv"].shape[2])
    norm = types.SimpleNamespace(**{str(k): [float(v[0]), float(v[1])] for k, v in zip(d["norm_names"], d["norm"])})
    norm.clip_observations = float(d["clip_obs"])
    return types.SimpleNamespace(env=env, normalization=norm)


def planes_of(d, step):
    """The planes of one recorded step, by the header's names."""
    return {k: d[v][step] for k, v in FIXTURE_PLANES.items()}


def assemble(cols, clip_obs, n, gravities, **planes):
    """go1_priv_step: the (n, len(cols)) f32 output.  `cols`: (name, src, comp, shift, scale, op) rows, as
    privileged.columns gives them; `planes`: 2-D (or flat one-column) arrays by name, one that no column reads may be
    left out."""
    out = np.empty((n, len(cols)), F)
    clip = F(clip_obs)
    g = np.asarray(gravities, F).reshape(3)
    for k, (_, src, comp, shift, scale, op) in enumerate(cols):
        if src == SRC_ZERO:
            x = np.zeros(n, F)
        elif src == SRC_GRAVITY:
            x = np.full(n, g[comp], F)
        else:
            x = np.asarray(planes[PLANES[src - 1]], F).reshape(n, -1)[:, comp]
        if op == OP_MUL:
            y = F(x - F(shift)) * F(scale)
        elif op == OP_DIV:
            y = F(x - F(shift)) / F(scale)
        else:
            y = x
        y = y.astype(F)
        out[:, k] = np.where(y < -clip, -clip, np.where(y > clip, clip, y))  # clampf
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
