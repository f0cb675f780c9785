"""Fixture of the reference's local target planner (container-only test infrastructure).

Imports the reference behind the offline stand-ins of tests/golden/refstubs, as make_golden.py does, and calls its
own LeggedRobot._plan_target_pose (legged_robot_trajectory_tracking.py:850-921) on a stub namespace that holds just
what the method reads: cfg, height_points, measured_heights, root_states, base_quat, base_pos, trajectories,
curr_pose_index, the three planner buffers, robot_size and a bound _compute_relative_target_pose.  32 envs run for 8
consecutive steps per case set; between steps this generator moves the roots, increments episode_length_buf,
restates the waypoint switch and the plan_buf update (:836-847) and reset_idx's lines (:250-254), and resets a few envs.

Each step runs twice: as it is (torch.argsort is not stable, and the key ignores z and the signs of roll, pitch and
yaw: which of several equal-key candidates wins depends on torch's build), recorded as `unstable_local_target`; and
with torch.argsort wrapped to pass stable=True, the expected output under this project's tie rule.

Recorded per step are the planes a go1_plan_step launch sees after the env step (root, trajectory, curr_pose_index,
episode_length, reset, heights) and the planner state after it.  For envs reset in a step the recorded `chosen`
follows the launch's contract (NOT_PLANNED, include/go1_plan.h): the reference plans them at the pre-reset pose, which
the step has overwritten, and discards the result; replan and plan_length are the reference's own on every env.

An env-step whose pick changes when the ellipsoid threshold moves to 1 +- 1e-5, or where another valid candidate's
key lies within 1e-5 of the pick's without being equal, is redrawn (at most 2 % of the draws, asserted).

Usage: python tests/golden/make_golden_plan.py [reference root]   (writes tests/golden/plan_cases.npz)
"""
import contextlib
import copy
import io
import os
import re
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GO1_REFERENCE_ROOT", "")  # the reference checkout

sys.dont_write_bytecode = True  # the reference tree is read-only
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, os.path.join(HERE, "refstubs"))
sys.path.insert(1, REF)
sys.path.insert(2, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import plan_ref as PR  # noqa: E402

N, STEPS = 32, 8
SWITCH_DIST, SWITCH_YAW = 0.3, 0.5  # train.py's switch_dist, the config's switch_yaw
CEILING = 0.8


def small_candidates():
    """70 candidates (not a multiple of 64), pitch 15 degrees throughout and roll 0 / 15 degrees: half of them are
    tested at the shifted yaw of quat_apply_yaw_inverse."""
    return np.stack(np.meshgrid(
        np.array([0.5]), np.array([0, -0.05, 0.05, -0.5, 0.5, -0.45, 0.45]), np.array([0.27]),
        np.array([0, 15]) * np.pi / 180, np.array([15]) * np.pi / 180,
        np.array([0, -22.5, +22.5, -45, +45]) * np.pi / 180), axis=-1).reshape(-1, 6)


SETS = {
    "default": dict(cand=PR.default_candidates(), gx=np.linspace(-1, 1, 21), gy=np.linspace(-0.5, 0.5, 11), L=1,
                    interval=4),
    "small": dict(cand=small_candidates(), gx=np.linspace(-1, 1, 5), gy=np.linspace(-0.5, 0.5, 3), L=3, interval=3),
}


def quat_of(roll, pitch, yaw):
    return PR.quat_from_euler_xyz(np.float32(roll), np.float32(pitch), np.float32(yaw))


def draw_heights(rng, nx, ny, blocked=False):
    h = np.zeros((2, nx, ny), np.float32)
    h[0] = CEILING
    if blocked:  # a slot too low for any candidate
        h[0], h[1] = 0.3, 0.25
        return h
    for _ in range(rng.integers(0, 8)):
        i0 = rng.integers(nx // 2, nx)
        j0 = rng.integers(0, ny)
        i1, j1 = i0 + rng.integers(1, max(2, nx // 4) + 1), j0 + rng.integers(1, max(2, ny // 2) + 1)
        if rng.random() < 0.5:
            h[0, i0:i1, j0:j1] = rng.uniform(0.2, 0.45)
        else:
            h[1, i0:i1, j0:j1] = rng.uniform(0.1, 0.3)
    return h


def draw_root(rng):
    r = np.zeros(13, np.float32)
    r[:3] = [rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(0.25, 0.33)]
    r[3:7] = quat_of(rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(-0.6, 0.6))
    return r


def draw_traj(rng, L, near):
    t = np.zeros((L, 6), np.float32)
    d = rng.uniform(0.4, 0.9) if near else rng.uniform(1.5, 4.0)
    for k in range(L):
        t[k] = [d * (k + 1), rng.uniform(-1.0, 1.0), rng.uniform(0.25, 0.33), rng.uniform(-0.3, 0.3),
                rng.uniform(-0.3, 0.3), rng.uniform(-0.6, 0.6)]
    return t


def fragile(ref, e, root, heights, target):
    """The redraw rule for env e, should it search in this step."""
    goal = target[:2] - root[:2]
    c, k, valid = PR.pick(ref.cand, ref.gx, ref.gy, heights, goal)
    for thr in (1 - 1e-5, 1 + 1e-5):
        if PR.pick(ref.cand, ref.gx, ref.gy, heights, goal, threshold=thr)[0] != c:
            return True
    if c >= 0:
        d = np.abs(k[valid].astype(np.float64) - float(k[c]))
        if np.any((d > 0) & (d < 1e-5)):
            return True
    return False


def run_set(name, spec, LR, seed):
    rng = np.random.default_rng(seed)
    cand, gx, gy, L, interval = spec["cand"], spec["gx"], spec["gy"], spec["L"], spec["interval"]
    nx, ny = len(gx), len(gy)
    ns = types.SimpleNamespace()
    ns.device, ns.num_actor, ns.num_envs = "cpu", 1, N
    ns.cfg = types.SimpleNamespace(commands=types.SimpleNamespace(
        sampling_based_planning=True, plan_interval=interval, candidate_target_poses=cand, traj_length=L,
        switch_dist=SWITCH_DIST, switch_yaw=SWITCH_YAW))
    pts = torch.zeros(N, nx, ny, 3)
    pts[..., 0] = torch.tensor(gx)[None, :, None].float()
    pts[..., 1] = torch.tensor(gy)[None, None, :].float()
    ns.height_points = pts
    ns.robot_size = torch.tensor([0.3762, 0.0935, 0.114]).float()
    ns.local_target_poses = torch.zeros(N, 6)
    ns.local_relative_linear = torch.zeros(N, 3)
    ns.local_relative_rotation = torch.zeros(N, 3)
    ns.plan_buf = torch.zeros(N, dtype=torch.bool)
    ns.plan_length_buf = torch.zeros(N, dtype=torch.long)
    ns.episode_length_buf = torch.zeros(N, dtype=torch.long)
    ns.curr_pose_index = torch.zeros(N, dtype=torch.long)
    ns._compute_relative_target_pose = types.MethodType(LR._compute_relative_target_pose, ns)
    near = rng.random(N) < 0.25
    ns.trajectories = torch.from_numpy(np.stack([draw_traj(rng, L, near[e]) for e in range(N)]))
    roots = np.stack([draw_root(rng) for _ in range(N)])

    ref = PR.PlanRef(N, cand, gx, gy, L, interval, SWITCH_DIST, SWITCH_YAW)
    rec = {k: [] for k in ("root", "trajectory", "curr_pose_index", "episode_length", "reset", "heights",
                           "local_target", "plan_buf", "plan_length", "local_rel_lin", "local_rel_rot", "replan",
                           "chosen", "unstable_local_target", "planned", "close")}
    draws = redraws = 0
    stable_argsort = torch.argsort
    for step in range(STEPS):
        # the "physics": roots creep forward; some envs are set down next to their local target (plan_buf comes
        # true), some next to their waypoint (the switch, and close)
        lt = ns.local_target_poses.numpy()
        tr = ns.trajectories.numpy()
        idx = ns.curr_pose_index.numpy()
        for e in range(N):
            yaw = PR.quat_to_rpy(roots[e:e + 1, 3:7])[0, 2]
            roots[e, 0] += rng.uniform(0.02, 0.1) * np.cos(yaw)
            roots[e, 1] += rng.uniform(0.02, 0.1) * np.sin(yaw)
            roots[e, 3:7] = quat_of(rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), yaw + rng.uniform(-0.05, 0.05))
            if step > 0 and e % 4 == 1 and step % 2 == 1:
                roots[e, :2] = lt[e, :2] + rng.uniform(-0.1, 0.1, 2)
                roots[e, 3:7] = quat_of(0.0, 0.0, lt[e, 5] + rng.uniform(-0.2, 0.2))
            if step in (2, 5) and e % 8 == 3:
                roots[e, :2] = tr[e, idx[e], :2] + rng.uniform(-0.1, 0.1, 2)
        ns.episode_length_buf += 1
        # heights, redrawn while the env's search would be fragile
        heights = np.zeros((N, 2, nx, ny), np.float32)
        target = tr[np.arange(N), idx]
        for e in range(N):
            blocked = name == "default" and e in (5, 21) and step in (0, 4)
            for attempt in range(50):
                heights[e] = draw_heights(rng, nx, ny, blocked)
                draws += 1
                if not fragile(ref, e, roots[e], heights[e], target[e]):
                    break
                redraws += 1
            else:
                raise AssertionError("no robust draw")
        ns.root_states = torch.from_numpy(roots.copy())
        ns.base_pos = ns.root_states[:, 0:3]
        ns.base_quat = ns.root_states[:, 3:7]
        ns.measured_heights = torch.from_numpy(heights.copy())
        plan_buf_before = ns.plan_buf.clone()
        env_ids = torch.arange(N)
        # as it is
        twin = copy.deepcopy(ns)
        twin._compute_relative_target_pose = types.MethodType(LR._compute_relative_target_pose, twin)
        with contextlib.redirect_stdout(io.StringIO()):
            LR._plan_target_pose(twin, env_ids)
        # with a stable argsort: the expected output
        torch.argsort = lambda *a, **k: stable_argsort(*a, **dict(k, stable=True))
        out = io.StringIO()
        try:
            with contextlib.redirect_stdout(out):
                LR._plan_target_pose(ns, env_ids)
        finally:
            torch.argsort = stable_argsort
        none_valid = {int(m) for m in re.findall(r"env_(\d+) has no valid local goal", out.getvalue())}
        ep_start = ns.episode_length_buf == 1
        planned = (ep_start | (ns.replan & plan_buf_before)).numpy()
        close = (torch.norm(ns.relative_linear[:, :2], dim=1) < 1.0).numpy()
        chosen = np.full(N, PR.NOT_PLANNED, np.int32)
        rpy = PR.quat_to_rpy(roots[:, 3:7])
        for e in np.nonzero(planned)[0]:
            if close[e]:
                chosen[e] = PR.CLOSE
            elif e in none_valid:
                chosen[e] = PR.NONE_VALID
            else:  # the candidate whose world pose is the reference's local target
                c32 = ref.cand
                xy = PR.quat_apply(PR.yaw_quat(roots[e, 3:7])[None], c32[:, :3])[:, :2] + roots[e, :2]
                pose = np.concatenate([xy, c32[:, 2:3], PR.wrap_to_pi(c32[:, 3:] + rpy[e])], 1)
                dang = np.abs(PR.wrap_to_pi(pose[:, 3:] - ns.local_target_poses[e, 3:].numpy()))
                d = np.maximum(np.abs(pose[:, :3] - ns.local_target_poses[e, :3].numpy()).max(1), dang.max(1))
                order = np.argsort(d)
                assert d[order[0]] < 1e-5 < 1e-3 < d[order[1]], (name, step, e, d[order[:2]])
                chosen[e] = order[0]
        # the waypoint switch and the plan_buf update (:836-847)
        switched = torch.linalg.norm(ns.relative_linear[:, :2], dim=1) < SWITCH_DIST
        ids = switched.nonzero(as_tuple=False).flatten()
        ns.curr_pose_index[ids] += 1
        ns.curr_pose_index[ids] = torch.clip(ns.curr_pose_index[ids], max=L - 1)
        lin_ok = torch.linalg.norm(ns.local_relative_linear[:, :2], dim=1) < SWITCH_DIST
        ns.plan_buf = torch.logical_and(lin_ok, torch.abs(ns.local_relative_rotation[:, 2]) < SWITCH_YAW)
        # resets (:241, :250-254): a few envs, one of them in two consecutive steps
        reset = np.zeros(N, bool)
        if step in (2, 5):
            reset[[2, 13, 27]] = True
        if step == 6:
            reset[13] = True
        rid = torch.from_numpy(np.nonzero(reset)[0])
        for e in rid.tolist():
            roots[e] = draw_root(rng)
            ns.trajectories[e] = torch.from_numpy(draw_traj(rng, L, rng.random() < 0.25))
        ns.curr_pose_index[rid] = 0
        ns.episode_length_buf[rid] = 0
        ns.local_relative_linear[rid] = 0.0
        ns.local_relative_rotation[rid] = 0.0
        ns.plan_buf[rid] = 1
        live = ~reset
        rec["root"].append(roots.copy())
        rec["trajectory"].append(ns.trajectories.numpy().reshape(N, 6 * L).copy())
        rec["curr_pose_index"].append(ns.curr_pose_index.numpy().astype(np.int32))
        rec["episode_length"].append(ns.episode_length_buf.numpy().astype(np.int32))
        rec["reset"].append(reset.copy())
        rec["heights"].append(heights)
        rec["local_target"].append(ns.local_target_poses.numpy().copy())
        rec["unstable_local_target"].append(twin.local_target_poses.numpy().copy())
        rec["plan_buf"].append(ns.plan_buf.numpy().copy())
        rec["plan_length"].append(ns.plan_length_buf.numpy().astype(np.int32))
        rec["local_rel_lin"].append(ns.local_relative_linear.numpy().copy())
        rec["local_rel_rot"].append(ns.local_relative_rotation.numpy().copy())
        rec["replan"].append(ns.replan.numpy().copy())
        rec["chosen"].append(np.where(live, chosen, PR.NOT_PLANNED).astype(np.int32))
        rec["planned"].append(planned & live)
        rec["close"].append(close.copy())
        # keep the restatement's state in step (it decides the next step's redraws)
        ref.step(roots, rec["trajectory"][-1], rec["curr_pose_index"][-1], rec["episode_length"][-1], reset, heights)
    assert redraws <= 0.02 * draws, (name, redraws, draws)
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(cand=np.asarray(cand, np.float64), grid_x=np.asarray(gx, np.float64), grid_y=np.asarray(gy, np.float64),
               traj_length=np.int32(L), plan_interval=np.int32(interval), switch_dist=np.float32(SWITCH_DIST),
               switch_yaw=np.float32(SWITCH_YAW), redraws=np.array([redraws, draws]))
    ch, pl, rp = out["chosen"], out["planned"], out["replan"]
    print(f"{name}: redraws {redraws}/{draws}; planned {int(pl.sum())}, close {int((ch == PR.CLOSE).sum())}, "
          f"none valid {int((ch == PR.NONE_VALID).sum())}, distinct picks {len(set(ch[ch >= 0].tolist()))}, "
          f"replan&planned {int((rp & pl).sum())}, replan&~planned {int((rp & ~pl).sum())}, "
          f"unstable differs on {int((np.abs(out['local_target'] - out['unstable_local_target']).max(-1) > 1e-6).sum())}")
    # every branch of the plan decision occurs
    assert (ch == PR.CLOSE).any() and (ch >= 0).any() and (rp & pl).any() and (rp & ~pl).any()
    assert name != "default" or (ch == PR.NONE_VALID).any()
    assert name != "small" or len({tuple(r) for r in out["curr_pose_index"].T.tolist()}) > 1
    return out


def main():
    from go1_gym.envs.base.legged_robot_trajectory_tracking import LeggedRobot as LR
    out = {}
    for i, (name, spec) in enumerate(SETS.items()):
        for k, v in run_set(name, spec, LR, 2024 + i).items():
            out[f"{name}/{k}"] = v
    path = os.path.join(HERE, "plan_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
