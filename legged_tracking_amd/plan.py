"""Host binding of the local target planner (include/go1_plan.h, legged_tracking_amd/_build/libgo1_plan.so):
Cfg.commands.sampling_based_planning of the reference (legged_robot_trajectory_tracking.py:850-921).

Every plan_interval steps, and at the first step of an episode, each env picks a local target pose from the fixed
candidate set Cfg.commands.candidate_target_poses: the candidate nearest the goal whose robot-sized ellipsoid is free
of every scanned ceiling and floor point.  LocalPlanner enqueues one launch after each env step (LeggedRobot.step)
that does this for all envs and overwrites the commands columns of the step's observations; nothing synchronises
until no_valid() is asked for.

torch provides the device memory and the stream; the search runs in the HIP kernel (no CPU fallback).  The loader, the
plane checks, the stream and the return-code check are native.py's add-on shim; EnvBase issues the launch
(env_base.py, _after_step)."""
import ctypes as C
import os

import numpy as np
import torch

from .native import AddOn, NativeError, dense, load_addon  # noqa: F401  (NativeError: importable from here)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "libgo1_plan.so")
GO1_PLAN_ABI_VERSION = 1
MAX_CAND, MAX_X, MAX_Y, FOOT = 4096, 64, 32, 8
CLOSE, NONE_VALID, NOT_PLANNED = -1, -2, -3
ROBOT_SIZE = (0.3762, 0.0935, 0.114)  # legged_robot_trajectory_tracking.py:1212
AUX_COMMANDS = 6                      # column of the commands in the step's aux block (go1_mi355x.h, GO1_AUX)

I32, F32, P = C.c_int32, C.c_float, C.c_void_p


class Go1PlanConfig(C.Structure):
    _fields_ = [("n_envs", I32), ("traj_length", I32), ("plan_interval", I32), ("scan_nx", I32), ("scan_ny", I32),
                ("n_cand", I32), ("n_foot", I32), ("pad", I32), ("switch_dist", F32), ("switch_yaw", F32),
                ("clip_obs", F32), ("robot_size", F32 * 3), ("scan_x", F32 * MAX_X), ("scan_y", F32 * MAX_Y)]


class Go1PlanTables(C.Structure):
    _fields_ = [("cand", P), ("cand_foot", P), ("key_rot", P), ("foot", P)]


class Go1PlanState(C.Structure):
    _fields_ = [("local_target", P), ("plan_buf", P), ("plan_length", P), ("idx_prev", P), ("ep_prev", P), ("local_rel_lin", P),
                ("local_rel_rot", P), ("replan", P), ("chosen", P), ("no_valid_count", P)]


class Go1PlanArgs(C.Structure):
    _fields_ = [("root", P), ("trajectory", P), ("curr_pose_index", P), ("episode_length", P), ("reset", P),
                ("heights", P), ("obs", P), ("obs_history", P), ("commands", P), ("obs_stride", I32),
                ("commands_stride", I32)]


_ARGTYPES = {
    "go1_plan_abi_sizes": [C.POINTER(C.c_int64)],
    "go1_plan_step": [C.POINTER(Go1PlanConfig), C.POINTER(Go1PlanTables), C.POINTER(Go1PlanState),
                      C.POINTER(Go1PlanArgs), C.c_void_p],
}


def abi_sizes():
    return [C.sizeof(Go1PlanConfig), C.sizeof(Go1PlanTables), C.sizeof(Go1PlanState), C.sizeof(Go1PlanArgs), MAX_CAND,
            FOOT]


def lib():
    """The plan library, loaded once; its struct sizes are checked against the mirrors above."""
    return load_addon(LIB_PATH, "go1_plan", GO1_PLAN_ABI_VERSION, _ARGTYPES, abi_sizes())


def check_candidates(candidates):
    """Cfg.commands.candidate_target_poses as a (K, 6) f32 array (torch.from_numpy(...).float(), :879); raises for
    what the reference fails on or the kernel does not take."""
    c = np.asarray(candidates)
    if c.ndim != 2 or c.shape[1] != 6 or c.shape[0] == 0:
        raise ValueError(f"Cfg.commands.candidate_target_poses has shape {c.shape}: a non-empty (K, 6) array of "
                         "(x, y, z, roll, pitch, yaw) is needed (:879-892)")
    if c.shape[0] > MAX_CAND:
        raise NotImplementedError(f"Cfg.commands.candidate_target_poses has {c.shape[0]} rows; the planner takes at "
                                  f"most {MAX_CAND} (GO1_PLAN_MAX_CAND)")
    return np.ascontiguousarray(c, np.float32)


def footprint_rows(cand):
    """(K, 5) f32: what enters the ellipsoid test of each candidate (:892-898).  x, y, z, and the z, w components of
    normalize((0, 0, qz, qw)) of quat_from_euler_xyz(roll, pitch, yaw): quat_apply_yaw_inverse drops the
    quaternion's x and y instead of extracting the yaw, so with roll and pitch both nonzero the test runs at
    yaw - 2 atan(tan(roll / 2) tan(pitch / 2)), 0.035 rad off for the default set's 15 degrees."""
    c = np.asarray(cand, np.float64)
    r, p, y = c[:, 3] * 0.5, c[:, 4] * 0.5, c[:, 5] * 0.5
    qz = np.sin(y) * np.cos(r) * np.cos(p) - np.cos(y) * np.sin(r) * np.sin(p)
    qw = np.cos(y) * np.cos(r) * np.cos(p) + np.sin(y) * np.sin(r) * np.sin(p)
    n = np.maximum(np.sqrt(qz * qz + qw * qw), 1e-9)
    rows = np.concatenate([c[:, :3], (qz / n)[:, None], (qw / n)[:, None]], 1).astype(np.float32)
    return rows + np.float32(0)  # -0.0 -> 0.0: equal rows have equal bits


def prepare_tables(candidates, grid_x, grid_y):
    """The kernel's tables as numpy arrays: `cand` (K, 6) f32, `foot` (F, 8) f32 the unique footprint rows (in order of
    first appearance), `cand_foot` (K,) int32 candidate -> footprint, `key_rot` (K,) f32 = 0.1 |rpy| as torch computes
    it in f32 (:888), and the scan coordinates `scan_x`, `scan_y` in f32."""
    cand = check_candidates(candidates)
    gx, gy = np.asarray(grid_x, np.float32).ravel(), np.asarray(grid_y, np.float32).ravel()
    if not 1 <= gx.size <= MAX_X or not 1 <= gy.size <= MAX_Y:
        raise NotImplementedError(f"the planner takes a scan of 1 x 1 .. {MAX_X} x {MAX_Y} points, not "
                                  f"{gx.size} x {gy.size}")
    rows = footprint_rows(cand)
    _, first, inv = np.unique(rows.view(np.int32), axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)                      # footprints in order of first appearance
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    foot = np.zeros((order.size, FOOT), np.float32)
    foot[:, :5] = rows[first[order]]
    key_rot = (torch.linalg.norm(torch.from_numpy(cand)[:, 3:], dim=1) * 0.1).numpy()
    return dict(cand=cand, foot=foot, cand_foot=rank[inv.ravel()].astype(np.int32), key_rot=key_rot, scan_x=gx,
                scan_y=gy)


class PlanBuffers(AddOn):
    """The planner's tables and state on `device` and the launch, over caller-supplied planes (no env needed)."""
    WHAT = "local planner"

    def __init__(self, n, device, candidates, grid_x, grid_y, traj_length, plan_interval, switch_dist, switch_yaw,
                 clip_obs, robot_size=ROBOT_SIZE):
        if int(plan_interval) <= 0:
            raise NameError("name 'ep_start' is not defined (Cfg.commands.plan_interval <= 0 with "
                            "sampling_based_planning, legged_robot_trajectory_tracking.py:867)")
        self._open(device, lib)
        dev = self.device
        self.n = n = int(n)
        tb = prepare_tables(candidates, grid_x, grid_y)
        self.tables = {k: torch.from_numpy(tb[k]).to(dev) for k in ("cand", "foot", "cand_foot", "key_rot")}
        self.nx, self.ny = int(tb["scan_x"].size), int(tb["scan_y"].size)
        c = self._cfg = Go1PlanConfig()
        c.n_envs, c.traj_length, c.plan_interval = n, int(traj_length), int(plan_interval)
        c.scan_nx, c.scan_ny = self.nx, self.ny
        c.n_cand, c.n_foot = int(tb["cand"].shape[0]), int(tb["foot"].shape[0])
        c.switch_dist, c.switch_yaw, c.clip_obs = float(switch_dist), float(switch_yaw), float(clip_obs)
        c.robot_size[:] = [float(x) for x in robot_size]
        c.scan_x[:self.nx] = [float(x) for x in tb["scan_x"]]
        c.scan_y[:self.ny] = [float(x) for x in tb["scan_y"]]
        self._tables = Go1PlanTables(**{k: v.data_ptr() for k, v in self.tables.items()})
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.local_target_poses = z((n, 6), torch.float32)
        self.plan_buf = z((n,), torch.bool)
        self.plan_length_buf = z((n,), torch.int32)
        self.idx_prev = z((n,), torch.int32)
        self.ep_prev = z((n,), torch.int32)
        self.local_relative_linear = z((n, 3), torch.float32)
        self.local_relative_rotation = z((n, 3), torch.float32)
        self.replan = z((n,), torch.bool)
        self.chosen = torch.full((n,), NOT_PLANNED, dtype=torch.int32, device=dev)
        self.no_valid_count = z((1,), torch.int32)
        self._state = Go1PlanState(
            local_target=self.local_target_poses.data_ptr(), plan_buf=self.plan_buf.data_ptr(),
            plan_length=self.plan_length_buf.data_ptr(), idx_prev=self.idx_prev.data_ptr(), ep_prev=self.ep_prev.data_ptr(),
            local_rel_lin=self.local_relative_linear.data_ptr(), local_rel_rot=self.local_relative_rotation.data_ptr(),
            replan=self.replan.data_ptr(), chosen=self.chosen.data_ptr(), no_valid_count=self.no_valid_count.data_ptr())
        self._args = Go1PlanArgs()

    def launch(self, root, trajectory, curr_pose_index, episode_length, reset, heights, obs, obs_history=None,
               commands=None):
        """go1_plan_step on the current stream.  The planes are the step's post-step state and outputs; `commands`
        is an (n, >= 2) f32 view whose columns 0, 1 receive the commands (the aux block's, aux[:, 6:8])."""
        self._need_gpu()
        n, dev, a = self.n, self.device, self._args
        L = self._cfg.traj_length
        f32, i32, b8 = (torch.float32,), (torch.int32,), (torch.bool, torch.uint8)
        a.root = dense("root", root, (n, 13), f32, dev)
        a.trajectory = dense("trajectory", trajectory, (n, 6 * L), f32, dev)
        a.curr_pose_index = dense("curr_pose_index", curr_pose_index, n, i32, dev)
        a.episode_length = dense("episode_length", episode_length, n, i32, dev)
        a.reset = dense("reset", reset, (n,), b8, dev)
        a.heights = dense("heights", heights, (n, 2, self.nx, self.ny), f32, dev)
        if obs is None or obs.dim() != 2 or obs.shape[0] != n or obs.shape[1] < 5 or obs.dtype != torch.float32 or \
                not obs.is_contiguous() or obs.device != dev:
            raise NativeError("obs must be a contiguous (n_envs, >= 5) float32 tensor")
        if commands is not None and (commands.dim() != 2 or commands.shape[0] != n or commands.shape[1] < 2 or
                                     commands.dtype != torch.float32 or commands.stride(1) != 1 or
                                     commands.stride(0) < 2 or commands.device != dev):
            raise NativeError("commands must be an (n_envs, >= 2) float32 view with unit column stride")
        a.obs, a.obs_stride = obs.data_ptr(), int(obs.shape[1])
        a.obs_history = dense("obs_history", obs_history, obs.shape, f32, dev) if obs_history is not None else None
        a.commands = commands.data_ptr() if commands is not None else None
        a.commands_stride = int(commands.stride(0)) if commands is not None else 0
        self._launch("go1_plan_step", C.byref(self._cfg), C.byref(self._tables), C.byref(self._state), C.byref(a))

    def mark_reset(self, env_ids):
        """A host-initiated reset of `env_ids` (reset_idx :252-254), and idx_prev = ep_prev = 0: the reset trajectory
        starts at its first waypoint, the episode at length 0."""
        ids = torch.as_tensor(env_ids, device=self.device).long().flatten()
        if ids.numel() == 0:
            return
        self.local_relative_linear[ids] = 0.0
        self.local_relative_rotation[ids] = 0.0
        self.plan_buf[ids] = True
        self.idx_prev[ids] = 0
        self.ep_prev[ids] = 0

    def no_valid(self):
        """Env-steps so far that planned without a valid candidate and fell back to the global target (the reference
        prints a line for each, :909).  The only call that waits for the device."""
        return int(self.no_valid_count.item())


class LocalPlanner(PlanBuffers):
    """The planner of one trajectory-tracking env (LeggedRobot builds it when its Cfg asks for planning)."""

    def __init__(self, env):
        from . import config as CF
        self.env = env
        cfg, cm = env.cfg, env.cfg.commands
        g = CF.scan_grid(cfg)
        super().__init__(env.num_envs, env.device, cm.candidate_target_poses, g["x"], g["y"], cm.traj_length,
                         cm.plan_interval, cm.switch_dist, cm.switch_yaw, cfg.normalization.clip_observations)
        self.heights = torch.zeros((self.n, 2, self.nx, self.ny), device=self.device)

    def step(self, out, heights, hist=None, aux=None):
        """The launch of one env step: `out` the step's outputs, `heights` the plane the step kernel stored its
        measured heights in, `hist` the history tap's copy of obs or None, `aux` the aux block or None."""
        st = self.env._sim.state
        self.launch(st["root"], st["trajectory"], st["curr_pose_index"], st["episode_length"], out["reset"], heights,
                    out["obs"], hist, aux[:, AUX_COMMANDS:AUX_COMMANDS + 2] if aux is not None else None)
