"""numpy restatement of the reference's local target planner (legged_robot_trajectory_tracking.py:850-921,
_plan_target_pose, with reset_idx :252-254 and the plan_buf update :845-847) in f32 and in the reference's
operation order, with this project's tie rule (smallest key, then smallest candidate index: a stable argsort)
and its per-step contract (include/go1_plan.h).  tests/test_plan_host.py pins it to the reference's own output
(tests/golden/plan_cases.npz); the GPU tests compare the kernel with it."""
import os

import numpy as np

F = np.float32
CASES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_cases.npz")
TWO_PI = 2 * np.pi
CLOSE, NONE_VALID, NOT_PLANNED = -1, -2, -3
ROBOT_SIZE = (0.3762, 0.0935, 0.114)


def default_candidates():
    """Cfg.commands.candidate_target_poses of the reference's config (:167-175), restated."""
    return np.stack(np.meshgrid(
        np.linspace(0.5, 0.5, 1), np.array([0, -0.15, +0.15, -0.3, 0.3, -0.45, 0.45]),
        np.array([0.29, 0.27, 0.31, 0.25, 0.23]), np.array([0, -15, +15]) * np.pi / 180,
        np.array([0, -15, +15]) * np.pi / 180, np.array([0, -22.5, +22.5, -45, +45]) * np.pi / 180,
    ), axis=-1).reshape(-1, 6)


def load_set(name):
    """One case set ("default" / "small") of the fixture as {array name: array}."""
    z = np.load(CASES)
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


def angle_close(a, b, tol=2e-5):
    """Angles equal within rtol = atol = tol, compared modulo 2 pi (a wrapped angle may sit at either end)."""
    return bool(np.all(np.abs(wrap_to_pi(np.asarray(a, F) - np.asarray(b, F))) <= tol + tol * np.pi))


def normalize(x):
    return x / np.maximum(np.sqrt(np.sum(x * x, -1, dtype=F)), F(1e-9))[..., None]


def quat_rotate_inverse(q, v):
    qw, qv = q[..., 3:4], q[..., :3]
    a = v * (F(2.0) * qw ** 2 - F(1.0))
    b = np.cross(qv, v).astype(F) * qw * F(2.0)
    c = qv * np.sum(qv * v, -1, keepdims=True, dtype=F) * F(2.0)
    return a - b + c


def quat_apply(a, b):
    xyz = a[..., :3]
    t = np.cross(xyz, b).astype(F) * F(2)
    return b + a[..., 3:] * t + np.cross(xyz, t).astype(F)


def yaw_quat(q):
    qy = np.array(q, F, copy=True)
    qy[..., :2] = 0
    return normalize(qy)


def wrap_to_pi(a):
    a = np.asarray(a, F) % TWO_PI
    return (a - TWO_PI * (a > np.pi)).astype(F)


def quat_to_rpy(q):
    qx, qy, qz, qw = (q[..., i] for i in range(4))
    roll = np.arctan2(F(2.0) * (qw * qx + qy * qz), qw * qw - qx * qx - qy * qy + qz * qz)
    sinp = F(2.0) * (qw * qy - qz * qx)
    with np.errstate(invalid="ignore"):
        pitch = np.where(np.abs(sinp) >= 1, np.abs(F(np.pi / 2.0)) * np.sign(sinp), np.arcsin(sinp))
    yaw = np.arctan2(F(2.0) * (qw * qz + qx * qy), qw * qw + qx * qx - qy * qy - qz * qz)
    return wrap_to_pi(np.stack([roll % TWO_PI, pitch % TWO_PI, yaw % TWO_PI], -1).astype(F))


def quat_from_euler_xyz(roll, pitch, yaw):
    cy, sy, cr, sr = np.cos(yaw * F(0.5)), np.sin(yaw * F(0.5)), np.cos(roll * F(0.5)), np.sin(roll * F(0.5))
    cp, sp = np.cos(pitch * F(0.5)), np.sin(pitch * F(0.5))
    return np.stack([cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp,
                     cy * cr * cp + sy * sr * sp], -1).astype(F)


def relative_pose(root, pose):
    """_compute_relative_target_pose (:922-932) for (n, 13) roots and (n, 6) poses."""
    q = root[:, 3:7]
    lin = quat_rotate_inverse(yaw_quat(q), pose[:, :3] - root[:, :3])
    return lin.astype(F), wrap_to_pi(pose[:, 3:] - quat_to_rpy(q))


def norm2(v):
    return np.sqrt(np.sum(v * v, -1, dtype=F))


def keys(cand, goal_xy):
    """The f32 sort key of every candidate (:886-889)."""
    return norm2(cand[:, :2] - goal_xy) + norm2(cand[:, 3:]) * F(0.1)


def metrics(cand, grid_x, grid_y, heights, robot_size=ROBOT_SIZE):
    """(K,) the smallest scaled ellipsoid norm over the 2 nx ny scanned points per candidate (:893-898): the
    candidate is valid when it is > 1."""
    nx, ny = len(grid_x), len(grid_y)
    pts = np.zeros((2, nx, ny, 3), F)
    pts[..., 0] = np.asarray(grid_x, F)[None, :, None]
    pts[..., 1] = np.asarray(grid_y, F)[None, None, :]
    pts[..., 2] = heights
    q = yaw_quat(quat_from_euler_xyz(cand[:, 3], cand[:, 4], cand[:, 5]))
    # equal (x, y, z, yaw quaternion) rows give equal arithmetic: each distinct row is evaluated once
    rows, inv = np.unique(np.concatenate([cand[:, :3], q], 1), axis=0, return_inverse=True)
    d = pts.reshape(-1, 1, 3) - rows[None, :, :3]
    r = quat_rotate_inverse(np.broadcast_to(rows[None, :, 3:], d.shape[:2] + (4,)), d)
    return np.sqrt(np.sum((r / np.asarray(robot_size, F)) ** 2, -1, dtype=F)).min(0)[inv.ravel()]


def pick(cand, grid_x, grid_y, heights, goal_xy, robot_size=ROBOT_SIZE, threshold=1.0):
    """(chosen index or NONE_VALID, keys, validity) with the tie rule of a stable argsort."""
    k = keys(cand, goal_xy)
    valid = metrics(cand, grid_x, grid_y, heights, robot_size) > F(threshold)
    order = np.argsort(k, kind="stable")
    ok = order[valid[order]]
    return (int(ok[0]) if ok.size else NONE_VALID), k, valid


class PlanRef:
    """The planner's state and one step of it (the contract of go1_plan_step), for n envs."""

    def __init__(self, n, candidates, grid_x, grid_y, traj_length, plan_interval, switch_dist, switch_yaw,
                 clip_obs=100.0, robot_size=ROBOT_SIZE):
        self.n, self.L, self.interval = n, int(traj_length), int(plan_interval)
        self.cand = np.asarray(candidates).astype(F)
        self.gx, self.gy = np.asarray(grid_x, F), np.asarray(grid_y, F)
        self.switch_dist, self.switch_yaw, self.clip = F(switch_dist), F(switch_yaw), F(clip_obs)
        self.robot_size = robot_size
        self.local_target = np.zeros((n, 6), F)
        self.plan_buf = np.zeros(n, bool)
        self.plan_length = np.zeros(n, np.int32)
        self.idx_prev = np.zeros(n, np.int32)
        self.ep_prev = np.zeros(n, np.int32)
        self.local_rel_lin = np.zeros((n, 3), F)
        self.local_rel_rot = np.zeros((n, 3), F)
        self.replan = np.zeros(n, bool)
        self.chosen = np.full(n, NOT_PLANNED, np.int32)
        self.no_valid = 0

    def mark_reset(self, ids):
        self.local_rel_lin[ids] = 0
        self.local_rel_rot[ids] = 0
        self.plan_buf[ids] = True
        self.idx_prev[ids] = 0
        self.ep_prev[ids] = 0

    def step(self, root, trajectory, curr_pose_index, episode_length, reset, heights):
        """One launch; returns the commands columns (n, 2) written into obs."""
        n = self.n
        root = np.asarray(root, F)
        traj = np.asarray(trajectory, F).reshape(n, self.L, 6)
        reset = np.asarray(reset).astype(bool).ravel()
        ep = np.asarray(episode_length).ravel()
        live = ~reset
        target = traj[np.arange(n), self.idx_prev]
        rel_lin, _ = relative_pose(root, target)
        close = norm2(rel_lin[:, :2]) < F(1.0)
        pl = self.plan_length + 1
        replan = pl % self.interval == 0
        # a reset env's pre-reset episode length is the planner's own copy + 1: the step has zeroed the plane
        plan = np.where(live, ep == 1, self.ep_prev == 0) | (replan & self.plan_buf)
        pl[plan & reset] = 0
        chosen = np.full(n, NOT_PLANNED, np.int32)
        lt = self.local_target.copy()
        rpy = quat_to_rpy(root[:, 3:7])
        for e in np.nonzero(plan & live)[0]:
            pl[e] = 0
            lt[e] = target[e]
            chosen[e] = CLOSE
            if close[e]:
                continue
            c, _, _ = pick(self.cand, self.gx, self.gy, heights[e], target[e, :2] - root[e, :2], self.robot_size)
            chosen[e] = c
            if c < 0:
                self.no_valid += 1
                continue
            cd = self.cand[c]
            lt[e, :2] = quat_apply(yaw_quat(root[e, 3:7]), cd[:3])[:2] + root[e, :2]
            lt[e, 2] = cd[2]
            lt[e, 3:] = wrap_to_pi(cd[3:] + rpy[e])
        lin, rot = relative_pose(root, lt)
        plan_buf = (norm2(lin[:, :2]) < self.switch_dist) & (np.abs(rot[:, 2]) < self.switch_yaw)
        self.local_target[live] = lt[live]
        self.plan_length = pl.astype(np.int32)
        self.ep_prev = np.where(live, ep, 0).astype(np.int32)
        self.local_rel_lin = np.where(live[:, None], lin, F(0)).astype(F)
        self.local_rel_rot = np.where(live[:, None], rot, F(0)).astype(F)
        self.plan_buf = np.where(live, plan_buf, True)
        self.idx_prev = np.where(live, np.asarray(curr_pose_index).ravel(), 0).astype(np.int32)
        self.replan = replan
        self.chosen = np.where(live, chosen, NOT_PLANNED).astype(np.int32)
        return np.clip(self.local_rel_lin[:, :2], -self.clip, self.clip)
