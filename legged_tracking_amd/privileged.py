"""Host binding of the privileged-observation assembler (include/go1_priv.h, legged_tracking_amd/_build/libgo1_priv.so):
the `build privileged obs` block of the reference's compute_observations (legged_robot_trajectory_tracking.py:477-590)
for any set of Cfg.env.priv_observe_* flags, clipped as step does (:108-111).

columns(cfg) turns the flags into a column table in the reference's order; check(cfg) raises the reference's own two
errors (the width assert of :589-590, the AttributeError of priv_observe_ground_friction) before a handle is built.
With exactly friction and restitution selected -- what the step kernel writes itself -- wanted(cfg) is false, nothing
is built and nothing is launched.  Otherwise Privileged enqueues one launch per env step, behind the randomiser and
behind the gravity schedule's tick, that fills the step's slot of the (OUT_RING, n, W) ring from the state planes, the
aux block and env.gravities; nothing synchronises.

torch provides the device memory and the stream; the assembly runs in the HIP kernel (no CPU fallback).  The loader,
the plane check, the stream and the return-code check are native.py's add-on shim; EnvBase issues the launch
(env_base.py, _after_tick)."""
import ctypes as C
import os

import numpy as np
import torch

from .native import AddOn, NativeError, dense, load_addon  # noqa: F401  (NativeError: importable from here)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "libgo1_priv.so")
GO1_PRIV_ABI_VERSION = 1
MAX_COLS = 48                                   # GO1_PRIV_MAX_COLS
SRC_ZERO, SRC_FRICTION, SRC_RESTITUTION, SRC_PAYLOADS, SRC_MOTOR_STRENGTH, SRC_MOTOR_OFFSET, SRC_ROOT, SRC_AUX, \
    SRC_GRAVITY = range(9)                      # GO1_PRIV_SRC_*
OP_MUL, OP_DIV, OP_RAW = range(3)               # GO1_PRIV_OP_*
PLANES = ("friction", "restitution", "payloads", "motor_strength", "motor_offset", "root", "aux")  # sources 1 .. 7
PLANE_COLS = dict(friction=1, restitution=1, payloads=1, motor_strength=12, motor_offset=12, root=13, aux=3)

I32, F32, P = C.c_int32, C.c_float, C.c_void_p
F32_T = (torch.float32,)


class Go1PrivCol(C.Structure):
    _fields_ = [("src", I32), ("comp", I32), ("shift", F32), ("scale", F32), ("op", I32)]


class Go1PrivConfig(C.Structure):
    _fields_ = [("n_envs", I32), ("width", I32), ("clip_obs", F32), ("pad", I32), ("cols", Go1PrivCol * MAX_COLS)]


class Go1PrivArgs(C.Structure):
    _fields_ = [(k, P) for k in PLANES] + [(k + "_stride", I32) for k in PLANES] + \
               [("pad", I32), ("table", P), ("out", P), ("gravities", F32 * 3), ("pad2", F32)]


_ARGTYPES = {
    "go1_priv_abi_sizes": [C.POINTER(C.c_int64)],
    "go1_priv_step": [C.POINTER(Go1PrivConfig), C.POINTER(Go1PrivArgs), C.c_void_p],
}


def abi_sizes():
    return [C.sizeof(Go1PrivCol), C.sizeof(Go1PrivConfig), C.sizeof(Go1PrivArgs), MAX_COLS]


def lib():
    """The assembler library, loaded once; its struct sizes are checked against the mirrors above."""
    return load_addon(LIB_PATH, "go1_priv", GO1_PRIV_ABI_VERSION, _ARGTYPES, abi_sizes())


# The blocks of compute_observations (:482-587) in its order: flag (without priv_observe_), source, the components it
# appends, Cfg.normalization range (None: appended raw), operation.  priv_observe_ground_friction sits between the
# first two and fails in the reference (check).  Flags the function never reads (friction_indep, joint_friction,
# Kp_factor, Kd_factor, contact_forces, contact_states, foot_height, ...) add nothing, there as here.
_BLOCKS = (
    ("friction", SRC_FRICTION, (0,), "friction_range", OP_MUL),
    ("restitution", SRC_RESTITUTION, (0,), "restitution_range", OP_MUL),
    ("base_mass", SRC_PAYLOADS, (0,), "added_mass_range", OP_MUL),
    # com_displacements stays the zeros of :1336: randomize_com_displacement is refused (config.SUPPORTED)
    ("com_displacement", SRC_ZERO, (0, 1, 2), "com_displacement_range", OP_MUL),
    ("motor_strength", SRC_MOTOR_STRENGTH, tuple(range(12)), "motor_strength_range", OP_MUL),
    ("motor_offset", SRC_MOTOR_OFFSET, tuple(range(12)), "motor_offset_range", OP_MUL),
    ("body_height", SRC_ROOT, (2,), "body_height_range", OP_MUL),      # root z, post-reset
    # base_lin_vel of :132 (aux columns 0:3), which reset_idx does not refresh: pre-reset for an env reset this step
    ("body_velocity", SRC_AUX, (0, 1, 2), "body_velocity_range", OP_MUL),
    ("gravity", SRC_GRAVITY, (0, 1, 2), "gravity_range", OP_DIV),      # the one division (:576)
    # never updated by this env after :1361 and :1247
    ("clock_inputs", SRC_ZERO, (0, 1, 2, 3), None, OP_RAW),
    ("desired_contact_states", SRC_ZERO, (0, 1, 2, 3), None, OP_RAW),
)
_TRAIN = ("friction", "restitution")            # the two columns the step kernel writes itself


def _on(cfg, flag):
    return bool(getattr(cfg.env, "priv_observe_" + flag, False))


def scale_shift(rng):
    """get_scale_shift (go1_gym/utils/math_utils.py:35-38) in Python floats, each rounded to f32 once."""
    lo, hi = float(rng[0]), float(rng[1])
    return float(np.float32(2.0 / (hi - lo))), float(np.float32((hi + lo) / 2.0))


def columns(cfg):
    """The column table of the Cfg's priv_observe_* flags, in the reference's order: a list of
    (name, src, comp, shift, scale, op) with name = (flag, index within its block)."""
    cols = []
    for flag, src, comps, rng, op in _BLOCKS:
        if not _on(cfg, flag):
            continue
        scale, shift = scale_shift(getattr(cfg.normalization, rng)) if rng is not None else (1.0, 0.0)
        cols += [((flag, i), src, comp, shift, scale, op) for i, comp in enumerate(comps)]
    return cols


def names(cfg):
    return [c[0] for c in columns(cfg)]


def check(cfg):
    """The two errors of the reference's own compute_observations, raised before any handle is built."""
    if _on(cfg, "ground_friction"):
        # :493: this env defines no _get_ground_frictions
        raise AttributeError("'LeggedRobot' object has no attribute '_get_ground_frictions'")
    w = len(columns(cfg))
    assert w == int(cfg.env.num_privileged_obs), \
        f"num_privileged_obs ({cfg.env.num_privileged_obs}) != the number of privileged observations ({w}), " \
        f"you will discard data from the student!"
    if w > MAX_COLS:
        raise NotImplementedError(f"{w} privileged columns; the assembler takes {MAX_COLS} (GO1_PRIV_MAX_COLS)")


def wanted(cfg):
    """Whether the Cfg needs the assembler's launch: any flag set other than exactly friction and restitution, the two
    columns the step kernel writes."""
    return tuple(dict.fromkeys(n[0] for n in names(cfg))) != _TRAIN


def _plane(name, t, cols, n, device):
    """(data pointer, row stride in floats) of plane `name`: n rows of at least `cols` floats, either dense (also the
    flat (n,) form of a one-column plane) or a row view of a wider allocation."""
    if t.dim() == 2 and not t.is_contiguous():
        if t.shape[0] != n or t.shape[1] < cols or t.dtype != torch.float32 or t.device != device or \
                t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            raise NativeError(f"{name} must be a ({n}, >= {cols}) torch.float32 tensor on {device} whose columns are "
                              f"adjacent (dense, or a row view of a wider allocation)")
        return t.data_ptr(), int(t.stride(0))
    if cols == 1 and t.dim() == 1:
        return dense(name, t, n, F32_T, device), 1
    width = int(t.shape[1]) if t.dim() == 2 and t.shape[1] >= cols else cols
    return dense(name, t, (n, width), F32_T, device), width


class PrivBuffers(AddOn):
    """The assembler's configuration, the device copy of its column table and the launch on `device`, over
    caller-supplied planes (no env needed).  `cols` is a columns(cfg) list, `clip_obs`
    Cfg.normalization.clip_observations."""
    WHAT = "privileged-observation assembler"

    def __init__(self, n, device, cols, clip_obs):
        cols = list(cols)
        if not 1 <= len(cols) <= MAX_COLS:
            raise ValueError(f"{len(cols)} privileged columns; the assembler takes 1 .. {MAX_COLS}")
        self._open(device, lib)
        self.n, self.width = int(n), len(cols)
        self.names = [c[0] for c in cols]
        self.reads = {PLANES[c[1] - 1] for c in cols if SRC_FRICTION <= c[1] <= SRC_AUX}  # planes a column reads
        c = self._cfg = Go1PrivConfig()
        c.n_envs, c.width, c.clip_obs = self.n, self.width, float(np.float32(clip_obs))
        for k, (_, src, comp, shift, scale, op) in enumerate(cols):
            c.cols[k] = Go1PrivCol(int(src), int(comp), float(np.float32(shift)), float(np.float32(scale)), int(op))
        self._args = Go1PrivArgs()
        self._table = None
        if self.device.type == "cuda":  # uploaded once: the table is constant for the env's life
            raw = np.frombuffer(bytes(c.cols), np.uint8)[:self.width * C.sizeof(Go1PrivCol)].copy()
            self._table = torch.from_numpy(raw).to(self.device)
            self._args.table = self._table.data_ptr()

    def launch(self, out, gravities, **planes):
        """go1_priv_step on the current stream: `out` (n, width) f32, `gravities` three host floats, and the planes
        by name (friction, restitution, payloads, motor_strength, motor_offset, root, aux); one that no column reads
        may be left out or None."""
        self._need_gpu()
        a, n, dev = self._args, self.n, self.device
        for k in PLANES:
            t = planes.get(k)
            if t is None:  # the library refuses it, by name, when a column reads it
                ptr, stride = None, 0
            else:
                ptr, stride = _plane(k, t, PLANE_COLS[k], n, dev)
            setattr(a, k, ptr)
            setattr(a, k + "_stride", stride)
        a.out = dense("out", out, (n, self.width), F32_T, dev)
        a.gravities[:] = [float(g) for g in gravities]
        self._launch("go1_priv_step", C.byref(self._cfg), C.byref(a))


class Privileged(PrivBuffers):
    """The assembler of one env (LeggedRobot builds it when privileged.wanted(cfg))."""

    def __init__(self, env):
        self.env = env
        check(env.cfg)
        super().__init__(env.num_envs, env.device, columns(env.cfg), env.cfg.normalization.clip_observations)
        self.needs_aux = "aux" in self.reads  # the step must store aux whatever set_output_demand says
        self._slots = {}  # id(out) -> (its checked data pointer, out)

    def step(self, out, gravities):
        """The launch of one env step: `out` the step's slot of the privileged ring, `gravities` env.gravities after
        the step's tick of the gravity schedule.  The planes are the env's own tensors for its whole life, so they are
        checked with the first launch into each slot; a later step writes the output pointer and the gravity only
        (the step loop is host-bound)."""
        a = self._args
        ptr = self._slots.get(id(out))
        if ptr is None:
            env = self.env
            st = env._sim.state
            self.launch(out, gravities, friction=st["friction"], restitution=st["restitution"],
                        payloads=env.payloads, motor_strength=st["motor_strength"], motor_offset=st["motor_offset"],
                        root=st["root"], aux=env._aux if self.needs_aux else None)
            self._slots[id(out)] = (a.out, out)  # the tensor is kept: its id stays its own
            return
        a.out = ptr[0]
        a.gravities[:] = gravities.tolist()
        self._launch("go1_priv_step", C.byref(self._cfg), C.byref(a))
