"""Host binding of the after-start domain randomiser (include/go1_dr.h, legged_tracking_amd/_build/libgo1_dr.so):
Cfg.domain_rand.push_robots and Cfg.domain_rand.randomize_rigids_after_start of the reference
(legged_robot_trajectory_tracking.py: _push_robots :1074-1084, _randomize_rigid_body_props :710-732 at :831-833 and in
reset_idx :233-235; the velocity env has the same lines).

Every push_interval steps of its episode an env's world-frame x and y velocity is replaced by a draw; every
rand_interval steps, and when it resets, its friction, restitution and (shadow) payload are redrawn.  Randomizer
enqueues one launch after each env step (LeggedRobot.step, VelocityTrackingEasyEnv.step) that does this for all envs
on the step's own state planes and rewrites the privileged observation of the redrawn envs; nothing synchronises.

torch provides the device memory and the stream; the draws run in the HIP kernel (no CPU fallback).  The loader, the
plane check, the stream and the return-code check are native.py's add-on shim; EnvBase issues the two launches
(env_base.py, _after_step and _after_reset_idx)."""
import ctypes as C
import os

import numpy as np
import torch

from .native import AddOn, NativeError, dense, load_addon  # noqa: F401  (NativeError: importable from here)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "libgo1_dr.so")
GO1_DR_ABI_VERSION = 1
DR_U = 8                                        # uniforms per env (GO1_DR_U)
U_PAYLOAD, U_FRICTION, U_RESTITUTION, U_PUSH_X, U_PUSH_Y = 0, 1, 2, 4, 5
DR_TAG = 0x44520000                             # Philox counter word 1 = DR_TAG + block (GO1_DR_TAG)

I32, F32, U64, P = C.c_int32, C.c_float, C.c_uint64, C.c_void_p
F32_T = (torch.float32,)


class Go1DrConfig(C.Structure):
    _fields_ = [("n_envs", I32), ("env_id_offset", I32), ("rand_interval", I32), ("push_interval", I32),
                ("rigids_after_start", I32), ("push_robots", I32), ("randomize_payload", I32),
                ("randomize_friction", I32), ("randomize_restitution", I32), ("pad", I32),
                ("payload_range", F32), ("payload_lo", F32), ("friction_range", F32), ("friction_lo", F32),
                ("restitution_range", F32), ("restitution_lo", F32), ("push_range", F32), ("push_lo", F32),
                ("priv_friction_shift", F32), ("priv_friction_scale", F32), ("priv_rest_shift", F32),
                ("priv_rest_scale", F32), ("clip_obs", F32), ("pad2", F32), ("rng_seed", U64)]


class Go1DrState(C.Structure):
    _fields_ = [("root", P), ("friction", P), ("restitution", P), ("payloads", P)]


class Go1DrArgs(C.Structure):
    _fields_ = [("reset", P), ("episode_length", P), ("priv", P), ("priv_stride", I32), ("pad", I32),
                ("rng_step", U64), ("uniforms", P), ("dbg_uniforms", P)]


_ARGTYPES = {
    "go1_dr_abi_sizes": [C.POINTER(C.c_int64)],
    "go1_dr_step": [C.POINTER(Go1DrConfig), C.POINTER(Go1DrState), C.POINTER(Go1DrArgs), C.c_void_p],
    "go1_dr_reset": [C.POINTER(Go1DrConfig), C.POINTER(Go1DrState), C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p,
                     C.c_void_p],
}


def abi_sizes():
    return [C.sizeof(Go1DrConfig), C.sizeof(Go1DrState), C.sizeof(Go1DrArgs), DR_U]


def lib():
    """The randomiser library, loaded once; its struct sizes are checked against the mirrors above."""
    return load_addon(LIB_PATH, "go1_dr", GO1_DR_ABI_VERSION, _ARGTYPES, abi_sizes())


def _flag(dr, name):
    return bool(getattr(dr, name, False))


def wanted(cfg):
    """Whether the Cfg asks for the randomiser's launch: either of its two flags."""
    return _flag(cfg.domain_rand, "push_robots") or _flag(cfg.domain_rand, "randomize_rigids_after_start")


def intervals(cfg):
    """(rand_interval, push_interval) in steps, as _parse_cfg derives them (:1868-1872): ceil(seconds / dt)."""
    dt = cfg.control.decimation * cfg.sim.dt
    dr = cfg.domain_rand
    return int(np.ceil(dr.rand_interval_s / dt)), int(np.ceil(dr.push_interval_s / dt))


def check_randomizer(cfg):
    """The Cfg of an env with push_robots or randomize_rigids_after_start: raises before any handle is built."""
    dr = cfg.domain_rand
    rigids, push = _flag(dr, "randomize_rigids_after_start"), _flag(dr, "push_robots")
    rand_interval, push_interval = intervals(cfg)
    if rigids and rand_interval < 1:
        raise ValueError(f"Cfg.domain_rand.rand_interval_s = {dr.rand_interval_s!r} gives a rand_interval of "
                         f"{rand_interval} steps; randomize_rigids_after_start needs at least 1 (:822)")
    if push and push_interval < 1:
        raise ValueError(f"Cfg.domain_rand.push_interval_s = {dr.push_interval_s!r} gives a push_interval of "
                         f"{push_interval} steps; push_robots needs at least 1 (:1078)")
    if rigids:
        for flag, name in (("randomize_base_mass", "added_mass_range"), ("randomize_friction", "friction_range"),
                           ("randomize_restitution", "restitution_range")):
            if _flag(dr, flag):
                lo, hi = getattr(dr, name)
                if hi < lo:
                    raise ValueError(f"Cfg.domain_rand.{name} = {[lo, hi]!r}: hi < lo")
        if _flag(dr, "randomize_com_displacement"):
            raise NotImplementedError(
                "Cfg.domain_rand.randomize_com_displacement with randomize_rigids_after_start: the reference redraws "
                "com_displacements after start (:716-720) but hands the COM to PhysX at creation only (:1593), and this "
                "path has no per-env trunk COM; switch one of the two flags off")
    if push and float(dr.max_push_vel_xy) < 0:
        raise ValueError(f"Cfg.domain_rand.max_push_vel_xy = {dr.max_push_vel_xy!r}: the push range has hi < lo")


def _range(flag, rng):
    """(on, f32(hi - lo), f32(lo)) of one randomize_* flag and its range, as the reference's Python floats give them."""
    lo, hi = rng
    return int(bool(flag)), float(np.float32(hi - lo)), float(np.float32(lo))


class DrBuffers(AddOn):
    """The randomiser's configuration, its payload shadow and the two launches on `device`, over caller-supplied planes
    (no env needed).  `ranges`: {"payload" | "friction" | "restitution": (lo, hi)} and "push": max_push_vel_xy;
    `flags`: {"rigids_after_start", "push_robots", "payload", "friction", "restitution": bool}; `priv`:
    (friction shift, friction scale, restitution shift, restitution scale, clip_obs)."""
    WHAT = "domain randomiser"

    def __init__(self, n, device, ranges, flags, rand_interval, push_interval, priv, env_id_offset=0, seed=0,
                 payloads=None):
        if int(rand_interval) < 1 or int(push_interval) < 1:
            raise ValueError(f"rand_interval = {rand_interval} and push_interval = {push_interval} must be >= 1")
        for k in ("payload", "friction", "restitution"):
            if ranges[k][1] < ranges[k][0]:
                raise ValueError(f"the {k} range {tuple(ranges[k])!r} has hi < lo")
        if ranges["push"] < 0:
            raise ValueError(f"max_push_vel_xy = {ranges['push']!r}: the push range has hi < lo")
        self._open(device, lib)
        dev = self.device
        self.n = n = int(n)
        c = self._cfg = Go1DrConfig()
        c.n_envs, c.env_id_offset = n, int(env_id_offset)
        c.rand_interval, c.push_interval = int(rand_interval), int(push_interval)
        c.rigids_after_start, c.push_robots = int(bool(flags["rigids_after_start"])), int(bool(flags["push_robots"]))
        c.randomize_payload, c.payload_range, c.payload_lo = _range(flags["payload"], ranges["payload"])
        c.randomize_friction, c.friction_range, c.friction_lo = _range(flags["friction"], ranges["friction"])
        c.randomize_restitution, c.restitution_range, c.restitution_lo = _range(flags["restitution"],
                                                                                ranges["restitution"])
        mv = float(ranges["push"])
        c.push_range, c.push_lo = float(np.float32(mv - (-mv))), float(np.float32(-mv))  # torch_rand_float(-mv, mv)
        c.priv_friction_shift, c.priv_friction_scale, c.priv_rest_shift, c.priv_rest_scale, c.clip_obs = \
            [float(np.float32(x)) for x in priv]
        c.rng_seed = int(seed)
        # env.payloads of the reference: redrawn after start, while the simulated mass stays the creation-time one
        self.payloads = torch.zeros((n, 1), device=dev)
        if payloads is not None:
            self.payloads.copy_(torch.as_tensor(payloads, device=dev).reshape(n, 1))
        self._state = Go1DrState()
        self._args = Go1DrArgs()
        self._keep = None

    def _bind(self, root, friction, restitution, payloads):
        self._need_gpu()
        n, dev, s = self.n, self.device, self._state
        s.root = dense("root", root, (n, 13), F32_T, dev)
        s.friction = dense("friction", friction, n, F32_T, dev)
        s.restitution = dense("restitution", restitution, n, F32_T, dev)
        s.payloads = dense("payloads", self.payloads, n, F32_T, dev) if payloads else None

    def _uniforms(self, name, u):
        return dense(name, u, (self.n, DR_U), F32_T, self.device) if u is not None else None

    def launch(self, root, friction, restitution, episode_length, reset, rng_step, priv=None, uniforms=None,
               dbg_uniforms=None, payloads=True):
        """go1_dr_step on the current stream.  The planes are the step's post-step state, `reset` its reset output,
        `priv` its privileged observation (n, >= 2) or None; `uniforms` / `dbg_uniforms` are (n, DR_U) f32 or None;
        payloads=False leaves the payload shadow out of the launch."""
        self._bind(root, friction, restitution, payloads)
        a = self._args
        a.reset = dense("reset", reset, self.n, (torch.bool, torch.uint8), self.device)
        a.episode_length = dense("episode_length", episode_length, self.n, (torch.int32,), self.device)
        if priv is not None:
            if priv.dim() != 2 or priv.shape[0] != self.n or priv.shape[1] < 2 or priv.dtype != torch.float32 or \
                    not priv.is_contiguous() or priv.device != self.device:
                raise NativeError("priv must be a contiguous (n_envs, >= 2) float32 tensor")
            a.priv, a.priv_stride = priv.data_ptr(), int(priv.shape[1])
        else:
            a.priv, a.priv_stride = None, 0
        a.rng_step = int(rng_step)
        a.uniforms, a.dbg_uniforms = self._uniforms("uniforms", uniforms), self._uniforms("dbg_uniforms", dbg_uniforms)
        self._launch("go1_dr_step", C.byref(self._cfg), C.byref(self._state), C.byref(a))

    def reset(self, root, friction, restitution, env_ids, rng_step, uniforms=None, payloads=True):
        """go1_dr_reset on the current stream: the rigid-props redraw of a host reset_idx(env_ids)."""
        self._bind(root, friction, restitution, payloads)
        ids = torch.as_tensor(env_ids, device=self.device).to(torch.int32).flatten().contiguous()
        self._keep = ids  # alive until the next call: the stream has passed it by then
        self._launch("go1_dr_reset", C.byref(self._cfg), C.byref(self._state), ids.data_ptr(), int(ids.numel()),
                     int(rng_step), self._uniforms("uniforms", uniforms))


class Randomizer(DrBuffers):
    """The randomiser of one env (LeggedRobot and VelocityTrackingEasyEnv build it when their Cfg sets push_robots or
    randomize_rigids_after_start)."""

    def __init__(self, env):
        self.env = env
        cfg, dr = env.cfg, env.cfg.domain_rand
        check_randomizer(cfg)
        rand_interval, push_interval = intervals(cfg)
        pc = env._vcfg if hasattr(env, "_vcfg") else env._abi_cfg  # the step's own priv constants
        super().__init__(
            env.num_envs, env.device,
            ranges=dict(payload=dr.added_mass_range, friction=dr.friction_range, restitution=dr.restitution_range,
                        push=dr.max_push_vel_xy),
            flags=dict(rigids_after_start=_flag(dr, "randomize_rigids_after_start"),
                       push_robots=_flag(dr, "push_robots"), payload=_flag(dr, "randomize_base_mass"),
                       friction=_flag(dr, "randomize_friction"), restitution=_flag(dr, "randomize_restitution")),
            rand_interval=max(rand_interval, 1), push_interval=max(push_interval, 1),
            priv=(pc.priv_friction_shift, pc.priv_friction_scale, pc.priv_rest_shift, pc.priv_rest_scale,
                  cfg.normalization.clip_observations),
            env_id_offset=env.rank * env.num_envs, seed=env.seed, payloads=env._sim.state["payload"])

    def step(self, reset, priv, rng_step):
        """The launch of one env step: `reset` and `priv` the step's outputs, `rng_step` the step's own."""
        st = self.env._sim.state
        self.launch(st["root"], st["friction"], st["restitution"], st["episode_length"], reset, rng_step, priv)

    def reset_idx(self, env_ids, rng_step):
        """The redraw of a host reset_idx(env_ids), with the rng_step the env gave its own reset."""
        st = self.env._sim.state
        self.reset(st["root"], st["friction"], st["restitution"], env_ids, rng_step)
