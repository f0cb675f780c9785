"""Host binding of the episode tracer (include/go1_trace.h, legged_tracking_amd/_build/libgo1_trace.so): a device-side
"flight recorder" for the envs.

An in-step reset overwrites root, dof_pos, trajectory and curr_pose_index inside the step kernel, so the poses of a
failed episode are gone when the host learns of the reset.  EpisodeTracer enqueues one small launch after each env
step (EnvBase.attach_tracer) that keeps every env's last `depth` poses in a ring on the device and, when an env's
episode ends for a wanted cause, copies the episode out of the ring into a capture buffer -- no host synchronisation
until counts() / episodes() are asked for.  A captured episode of T rows is drawn by handing its rows to the ray
caster as T "envs": render_episode is one go1_render launch for the whole episode.

torch provides the device memory and the stream; every copy is done by the HIP kernel (no CPU fallback).  The loader,
the plane check, the stream and the return-code check are native.py's add-on shim; EnvBase issues the push
(env_base.py, _after_step)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

from .native import AddOn, NativeError, dense, load_addon

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_build", "libgo1_trace.so")
GO1_TRACE_ABI_VERSION = 1
ROW, META = 26, 8
TERMINATED, TIMEOUT = 1, 2
WANT_BITS = {"terminated": TERMINATED, "timeout": TIMEOUT}
TM_ENV, TM_ORDINAL, TM_END_PUSH, TM_KEPT, TM_LENGTH, TM_CAUSE = range(6)

I32, P = C.c_int32, C.c_void_p


class Go1TraceArgs(C.Structure):
    _fields_ = [("root", P), ("dof_pos", P), ("wp_index", P), ("wp_trajectory", P), ("reset", P), ("time_out", P),
                ("eligible", P), ("ring", P), ("ep_start", P), ("ep_ordinal", P), ("traj_start", P),
                ("cap_rows", P), ("cap_traj", P), ("cap_meta", P), ("cap_count", P),
                ("n_envs", I32), ("depth", I32), ("capacity", I32), ("wp_length", I32), ("want", I32), ("pad", I32),
                ("push", C.c_uint64)]


_ARGTYPES = {
    "go1_trace_abi_sizes": [C.POINTER(C.c_int64)],
    "go1_trace_push": [C.POINTER(Go1TraceArgs), C.c_void_p],
}


def lib():
    """The trace library, loaded once; its struct size is checked against the mirror above."""
    return load_addon(LIB_PATH, "go1_trace", GO1_TRACE_ABI_VERSION, _ARGTYPES, [C.sizeof(Go1TraceArgs), ROW, META])


def want_bits(want):
    """GO1_TRACE_* bits of an int or of names ("terminated", "timeout")."""
    if isinstance(want, int):
        bits = want
    else:
        unknown = [w for w in want if w not in WANT_BITS]
        if unknown:
            raise ValueError(f"want {unknown}: {sorted(WANT_BITS)}")
        bits = sum({WANT_BITS[w] for w in want})
    if bits & ~(TERMINATED | TIMEOUT):
        raise ValueError(f"want bits {bits}: {TERMINATED} terminated, {TIMEOUT} timeout")
    return bits


class TraceBuffers(AddOn):
    """The tracer's state and capture buffers over caller-supplied planes, and the push launch (no env needed).
    `trajectory` (n, 6 x length) and `wp_index` (n,) / (n, 1) int32 are each optional."""
    WHAT = "episode tracer"

    def __init__(self, root, dof_pos, depth, capacity=64, want=TERMINATED | TIMEOUT, eligible=None, trajectory=None,
                 wp_index=None):
        self._open(root.device, lib)
        dev = self.device
        n = int(root.shape[0])
        self.n, self.depth, self.capacity = n, int(depth), int(capacity)
        if self.depth < 1 or self.capacity < 1:
            raise ValueError("depth and capacity must be >= 1")
        self.want = want_bits(want)
        dense("root", root, (n, 13), (torch.float32,))
        dense("dof_pos", dof_pos, (n, 12), (torch.float32,))
        self.root, self.dof_pos, self.trajectory, self.wp_index = root, dof_pos, trajectory, wp_index
        self.tw = 0
        if trajectory is not None:
            if trajectory.dim() != 2 or trajectory.shape[1] % 6 or trajectory.shape[1] == 0:
                raise NativeError("trajectory must be (n_envs, 6 x length)")
            dense("trajectory", trajectory, (n, trajectory.shape[1]), (torch.float32,))
            self.tw = int(trajectory.shape[1])
        if wp_index is not None:
            dense("wp_index", wp_index, n, (torch.int32,))
        if eligible is not None:
            eligible = torch.as_tensor(eligible, device=dev)
            dense("eligible", eligible, (n,), (torch.bool, torch.uint8))
        self.eligible = eligible
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.ring = z((self.depth, n, ROW), torch.int32)
        self.ep_start = z((n,), torch.int64)
        self.ep_ordinal = z((n,), torch.int32)
        self.traj_start = z((n, self.tw), torch.int32) if self.tw else None
        self.cap_rows = z((self.capacity, self.depth, ROW), torch.int32)
        self.cap_traj = z((self.capacity, self.tw), torch.int32) if self.tw else None
        self.cap_meta = z((self.capacity, META), torch.int32)
        self.cap_count = z((2,), torch.int32)
        if self.tw:  # the episodes running now began with the current trajectories
            self.traj_start.copy_(trajectory.view(torch.int32))
        self.pushes = 0
        a = self._args = Go1TraceArgs()
        a.root, a.dof_pos = root.data_ptr(), dof_pos.data_ptr()
        a.wp_index = wp_index.data_ptr() if wp_index is not None else None
        a.eligible = eligible.data_ptr() if eligible is not None else None
        a.ring, a.ep_start, a.ep_ordinal = self.ring.data_ptr(), self.ep_start.data_ptr(), self.ep_ordinal.data_ptr()
        a.cap_rows, a.cap_meta, a.cap_count = (self.cap_rows.data_ptr(), self.cap_meta.data_ptr(),
                                               self.cap_count.data_ptr())
        if self.tw:
            a.wp_trajectory, a.wp_length = trajectory.data_ptr(), self.tw // 6
            a.traj_start, a.cap_traj = self.traj_start.data_ptr(), self.cap_traj.data_ptr()
        a.n_envs, a.depth, a.capacity, a.want = n, self.depth, self.capacity, self.want

    def push(self, reset, time_out):
        """The launch of one env step on the current stream: `reset` / `time_out` are the step's (n,) outputs."""
        self._need_gpu()
        a = self._args
        b8, what = (torch.bool, torch.uint8), "the step's contiguous (n_envs,) bool output"
        a.reset = dense("reset", reset, (self.n,), b8, self.device, what)
        a.time_out = dense("time_out", time_out, (self.n,), b8, self.device, what)
        a.push = self.pushes
        self._launch("go1_trace_push", C.byref(a))
        self.pushes += 1

    def mark_reset(self, env_ids):
        """A host-initiated reset of `env_ids` (after it): the bookkeeping of an ended episode, without a capture."""
        ids = torch.as_tensor(env_ids, device=self.device).long().flatten()
        if ids.numel() == 0:
            return
        ids = torch.unique(ids)
        self.ep_ordinal[ids] += 1
        self.ep_start[ids] = self.pushes
        if self.tw:
            self.traj_start[ids] = self.trajectory.view(torch.int32)[ids]

    def counts(self):
        """(captured, dropped): the only call that waits for the device."""
        claimed, dropped = (int(x) for x in self.cap_count.tolist())
        return min(claimed, self.capacity), dropped

    def captures(self):
        """(meta (k, 8) int32, rows (k, depth, 26) int32, traj (k, 6 x length) int32, slots (k,)) on the host,
        sorted by (end push, env)."""
        k = self.counts()[0]
        meta = self.cap_meta[:k].cpu().numpy()
        order = np.lexsort((meta[:, TM_ENV], meta[:, TM_END_PUSH]))
        rows = self.cap_rows[:k].cpu().numpy()[order]
        traj = self.cap_traj[:k].cpu().numpy()[order] if self.tw else np.zeros((k, 0), np.int32)
        return meta[order], rows, traj, order


class EpisodeTracer(TraceBuffers):
    """The tracer of one env: attach it with env.attach_tracer(tracer).

    depth     rows kept per env; None: max_episode_length + 1, a whole episode begun by an in-step reset
    capacity  captured episodes kept; further candidates are counted as dropped
    want      causes captured: "terminated" (reset without time_out), "timeout"
    eligible  (n_envs,) bool mask of the envs captured, or None: every env"""

    def __init__(self, env, depth=None, capacity=64, want=("terminated", "timeout"), eligible=None):
        self.env = env
        st = env._sim.state
        kw = {}
        try:
            kw.update(trajectory=st["trajectory"], wp_index=st["curr_pose_index"])
        except KeyError:  # the velocity env has no waypoints
            pass
        if depth is None:
            depth = int(env.max_episode_length) + 1
        super().__init__(st["root"], st["dof_pos"], depth, capacity, want, eligible, **kw)

    def episodes(self):
        """The captured episodes, sorted by (end push, env): records with env, ordinal, end_push, kept, full_length,
        cause, slot, root (T, 13), dof_pos (T, 12), curr_pose_index (T,) and trajectory ((6 x length,) or None)."""
        meta, rows, traj, slots = self.captures()
        out = []
        for m, r, tr, slot in zip(meta, rows, traj, slots):
            T = int(m[TM_KEPT])
            r = np.ascontiguousarray(r[:T])
            out.append(SimpleNamespace(
                env=int(m[TM_ENV]), ordinal=int(m[TM_ORDINAL]), end_push=int(m[TM_END_PUSH]), kept=T,
                full_length=int(m[TM_LENGTH]), cause=int(m[TM_CAUSE]), slot=int(slot),
                root=np.ascontiguousarray(r[:, :13]).view(np.float32),
                dof_pos=np.ascontiguousarray(r[:, 13:25]).view(np.float32), curr_pose_index=r[:, 25].copy(),
                trajectory=np.ascontiguousarray(tr).view(np.float32) if self.tw else None))
        return out

    def render_episode(self, i, width, height, mode=None, flags=None):
        """(T, height, width, 4) uint8 frames of episode i of episodes(): one ray-cast launch in which view t draws
        row t on the env's own terrain tile, with the waypoint the env was heading for at that step."""
        from . import render as R
        meta, _, _, slots = self.captures()
        m, slot = meta[i], int(slots[i])
        e, T = int(m[TM_ENV]), int(m[TM_KEPT])
        if T == 0:
            return np.zeros((0, int(height), int(width), 4), np.uint8)
        env = self.env
        rows = self.cap_rows[slot, :T]
        kw = dict(horizontal_scale=float(getattr(env.cfg.terrain, "horizontal_scale", 0.1)))
        keep = getattr(env._sim, "_terrain_keep", None)
        if keep is not None and getattr(getattr(env, "terrain", None), "kind", "plane") != "plane":
            kw.update(tiles=keep[0], env_tile=keep[1][e:e + 1].repeat(T),
                      env_terrain_origin=keep[2][e:e + 1].repeat(T, 1))
        if self.tw:
            kw.update(trajectory=self.cap_traj[slot:slot + 1].repeat(T, 1).view(torch.float32),
                      curr_pose_index=rows[:, 25:26].contiguous())
        scene = R.Scene(rows[:, :13].contiguous().view(torch.float32), rows[:, 13:25].contiguous().view(torch.float32),
                        **kw)
        cam = env._get_renderer().camera()
        mode, flags = cam[0] if mode is None else mode, cam[1] if flags is None else flags
        views = R.views_tensor([(t, mode, flags) for t in range(T)], self.device)
        return R.render_views(scene, views, int(width), int(height)).cpu().numpy()
