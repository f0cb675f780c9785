"""python -m legged_tracking_amd.evaluate LOGDIR [--envs 4096] [--episodes-per-env 1] [--rows R --cols C]
                                          [--terrain single_path|narrow_path|random_pyramid] [--dr off|train]
                                          [--deterministic] [--teacher] [--seed S] [--json FILE]
                                          [--capture N --capture-out DIR --capture-what fall,timeout --capture-size W H]

Numbers for a checkpoint: the success / collision bookkeeping the reference's authors sketched in their Runner
(ppo_cse/__init__.py:152-157), from the env's episode log.  The env is rebuilt from the checkpoint's Cfg
(parameters.pkl; play.checkpoint_cfg) without rendering, the policy (checkpoint.load_actor_critic, either learner)
runs through policy_kernels.fused_inference -- the student, or with --teacher the actor on the privileged observations --
until every env has finished --episodes-per-env episodes.  --dr off applies play.DR_OFF (scripts/eval.py:89-101),
--dr train keeps the trained ranges.  The result is one dict, printed as one JSON line (and written to --json).

Counting rule.  Exactly each env's first K episodes are counted (K = --episodes-per-env).  Counting "the first N
episodes overall" would over-represent short episodes, i.e. failures: an env that falls at once finishes many
episodes while another is still walking its first.  The episode log's deques drop the env id and keep the newest
4000 rows only, so the rows come from EpisodeLogRing.listener, which sees every finished episode with its env id.

Definitions, per counted episode (a row of the episode log):
  success    the row's `reached` flag: the robot reached its last waypoint
  timeout    not a success, and the episode ran out of time: its length exceeds the env's max_episode_length (the
             flag the env reports as time_outs)
  fall       neither: the episode ended in a termination (contact, body height, divergence guard)
so success_rate + timeout_rate + fall_rate = 1 by construction.
  collision-free   the episode's summed `collision` reward is exactly 0 (the term is a penalty per step in
                   collision); null when Cfg.reward_scales has no collision slot
  collision_free_success_rate   episodes that are both, over all counted episodes
mean_rew_<term> is the mean episode sum of every slot of the log (the reward terms, total, total_pos, total_neg),
per_tile the success rate and the episode count of each sub-terrain (env -> tile map of the terrain builder).
`steps` is the number of env steps taken (each of all envs), env_steps_per_s = steps x envs / wall time of the loop.

Trajectory-tracking checkpoints only: the velocity env logs no `reached`.

--capture N shows the failures the rates count.  After the evaluation's env.reset() an EpisodeTracer (trace.py) is
attached at full depth: one small launch per step keeps every env's poses on the device and copies out each episode
that ends for a wanted cause (--capture-what fall -> terminations, timeout -> time-outs), with no host
synchronisation.  Afterwards every captured episode is joined to the episode-log row of the same env and the same
per-env episode ordinal, labelled by the rule above, and the first N with a wanted label, in (end step, env) order,
are ray-cast at --capture-size (one launch per episode) and written as DIR/episode_{k}_env{e}_{label}.gif; the result
gains a "captured" list (file, env, tile, label, length, rows_kept).  The device cannot label: with
terminate_end_of_trajectory a success is a termination too and takes a capture slot before the host can tell it
from a fall, so the tracer's capacity is 4 x N; candidates past it are dropped (and counted), so fewer than N files
can come out of a run with many successes.  Without --capture nothing is attached and the result is unchanged.
"""
import argparse
import json
import os
import pickle
import time

import numpy as np
import torch

from . import config as CF, play as PL, policy_kernels as PK, trace, video
from .env import HistoryWrapper, TrajectoryTrackingEnv


class EpisodeCounter:
    """EpisodeLogRing listener: keeps each env's first K episode rows (in log order)."""

    def __init__(self, n_envs, k):
        self.k = int(k)
        self.count = np.zeros(int(n_envs), np.int64)
        self.rows, self.envs = [], []

    def __call__(self, rows, env_ids, tags):
        env_ids = np.asarray(env_ids, np.int64)
        if env_ids.size == 0:
            return
        # rank of each row among its env's rows of this call (the rows are in step order)
        order = np.argsort(env_ids, kind="stable")
        se = env_ids[order]
        first = np.r_[0, np.flatnonzero(se[1:] != se[:-1]) + 1]
        rank = np.empty(se.size, np.int64)
        rank[order] = np.arange(se.size) - np.repeat(first, np.diff(np.r_[first, se.size]))
        keep = self.count[env_ids] + rank < self.k
        if keep.any():
            self.rows.append(np.array(rows[keep], np.float32))
            self.envs.append(env_ids[keep])
        np.add.at(self.count, env_ids, 1)

    @property
    def done(self):
        return bool((self.count >= self.k).all())

    def table(self, width):
        if not self.rows:
            return np.zeros((0, width), np.float32), np.zeros(0, np.int64)
        return np.concatenate(self.rows), np.concatenate(self.envs)


def summarize(rows, env_ids, sum_keys, max_episode_length, env_tile):
    """The reported fields (module docstring) of the counted rows (m, len(sum_keys) + 3)."""
    ns = len(sum_keys)
    m = rows.shape[0]
    if m == 0:
        raise ValueError("no episode was counted")
    length, reached, dist = rows[:, ns], rows[:, ns + 1] > 0, rows[:, ns + 2]
    timeout = ~reached & (length > np.float32(max_episode_length))
    fall = ~reached & ~timeout
    out = {"episodes": int(m), "success_rate": float(reached.mean()), "timeout_rate": float(timeout.mean()),
           "fall_rate": float(fall.mean())}
    if "collision" in sum_keys:
        free = rows[:, sum_keys.index("collision")] == 0
        out["collision_free_rate"] = float(free.mean())
        out["collision_free_success_rate"] = float((free & reached).mean())
    else:
        out["collision_free_rate"] = out["collision_free_success_rate"] = None
    out["mean_episode_length"] = float(length.mean(dtype=np.float64))
    out["mean_goal_distance"] = float(dist.mean(dtype=np.float64))
    for i, k in enumerate(sum_keys):
        out["mean_rew_" + k] = float(rows[:, i].mean(dtype=np.float64))
    tiles = np.asarray(env_tile, np.int64)[env_ids]
    out["per_tile"] = {str(int(t)): {"episodes": int((tiles == t).sum()),
                                     "success_rate": float(reached[tiles == t].mean())} for t in np.unique(tiles)}
    return out


def run_episodes(env, policy, episodes_per_env, max_steps=None, after_reset=None):
    """Step `env` with `policy` until every train env has finished episodes_per_env episodes; -> (rows, env ids,
    steps taken, seconds).  The log is drained every ring half, so the loop overruns by at most that many steps.
    `after_reset(counter)` is called between the env's reset and the first step, the log drained."""
    log = env._elog
    counter = EpisodeCounter(env.num_train_envs, episodes_per_env)
    if log.listener is not None:
        raise RuntimeError("the env's episode log already has a listener")
    log.drain()  # episodes finished before the evaluation are not its own
    log.listener = counter
    try:
        obs = env.reset()
        if after_reset is not None:
            log.drain()
            after_reset(counter)
        if max_steps is None:  # K episodes of full length, and slack for the resets' own steps
            max_steps = int(episodes_per_env * (env.max_episode_length + 2)) + log.R
        steps, t0 = 0, time.perf_counter()
        with torch.no_grad():
            while not counter.done and steps < max_steps:
                obs, _, _, _ = env.step(policy(obs))
                steps += 1
                if steps % log.R == 0:
                    log.drain()
            log.drain()
        if obs["obs"].is_cuda:
            torch.cuda.synchronize(obs["obs"].device)
        dt = time.perf_counter() - t0
    finally:
        log.listener = None
    if not counter.done:
        raise RuntimeError(f"{int((counter.count < counter.k).sum())} envs finished fewer than {counter.k} episodes in "
                           f"{steps} steps")
    rows, ids = counter.table(log.W)
    return rows, ids, steps, dt


CAPTURE_CAUSES = {"fall": "terminated", "timeout": "timeout"}  # label -> the tracer cause that can carry it


def label_captures(episodes, rows, env_ids, base, n_sums, max_episode_length):
    """Join the tracer's records to the counted episode-log rows: -> [(record, label, length)] in the records' order.
    `base[e]` is the number of episodes env e had finished when the tracer was attached, so its record of ordinal o
    is the env's episode base[e] + o, the row of that rank among the env's rows (EpisodeCounter keeps them in log
    order); records of episodes that were not counted (past the env's K) are left out."""
    index, seen = {}, {}
    for j, e in enumerate(np.asarray(env_ids).tolist()):
        index[e, seen.get(e, 0)] = j
        seen[e] = seen.get(e, 0) + 1
    out = []
    for ep in episodes:
        j = index.get((ep.env, int(base[ep.env]) + ep.ordinal)) if ep.env < len(base) else None
        if j is None:
            continue
        length, reached = rows[j, n_sums], rows[j, n_sums + 1] > 0
        label = "success" if reached else "timeout" if length > np.float32(max_episode_length) else "fall"
        if ep.ordinal > 0:  # begun by an in-step reset the tracer saw: its pushes are the episode's steps
            assert ep.full_length == int(length), (ep.env, ep.ordinal, ep.full_length, float(length))
        out.append((ep, label, int(length)))
    return out


def write_captures(tracer, episodes, labelled, what, n, out_dir, size, env_tile, fps):
    """The "captured" list: the first n of `labelled` (records of `episodes` = tracer.episodes()) with a label in
    `what`, rendered and written as GIFs.  An episode that ended in the tracer's first push has no row and is skipped."""
    where = {id(ep): i for i, ep in enumerate(episodes)}
    out = []
    for ep, label, length in labelled:
        if label not in what or len(out) >= n or ep.kept == 0:
            continue
        frames = tracer.render_episode(where[id(ep)], size[0], size[1])
        path = os.path.join(out_dir, f"episode_{len(out)}_env{ep.env}_{label}.gif")
        out.append({"file": video.save_frames(frames, path, fps=fps), "env": ep.env, "tile": int(env_tile[ep.env]),
                    "label": label, "length": length, "rows_kept": ep.kept})
    return out


def _refuse_velocity(logdir):
    pkl = PL._find(logdir, "parameters.pkl")
    if pkl is None:
        return
    with open(pkl, "rb") as f:
        saved = pickle.load(f)
    if "traj_function" not in saved.get("commands", {}):
        raise ValueError(f"{logdir} is not a trajectory-tracking checkpoint: the Cfg.commands of its parameters.pkl has "
                         f"no traj_function (a velocity-tracking run).  The velocity env's episode log has no "
                         f"`reached`, so there is no success to evaluate")


def _grid(logdir, rows, cols):
    """The terrain grid: the arguments, else the checkpoint's own (parameters.pkl), else play's 4 x 4."""
    t = {}
    pkl = PL._find(logdir, "parameters.pkl")
    if pkl is not None:
        with open(pkl, "rb") as f:
            t = pickle.load(f).get("terrain", {})
    return (int(rows if rows is not None else t.get("num_rows", 4)),
            int(cols if cols is not None else t.get("num_cols", 4)))


def evaluate(logdir, envs=4096, episodes_per_env=1, rows=None, cols=None, terrain=None, dr="off",
             deterministic=False, teacher=False, seed=11, device="cuda:0", json_path=None, capture=0,
             capture_out="captures", capture_what=("fall",), capture_size=(360, 240), tracer_factory=None):
    """-> the dict of the module docstring.  `tracer_factory(env, capacity=, want=)` replaces trace.EpisodeTracer
    (a test double on the CPU)."""
    if dr not in ("off", "train"):
        raise ValueError(f"dr {dr!r}: off or train")
    if PL._find(logdir, "ac_weights.pt") is None:
        raise FileNotFoundError(f"no ac_weights.pt under {logdir}")
    _refuse_velocity(logdir)
    capture, capture_what = int(capture), tuple(capture_what)
    unknown = [w for w in capture_what if w not in CAPTURE_CAUSES]
    if unknown or (capture > 0 and not capture_what):
        raise ValueError(f"capture_what {list(capture_what)}: any of {sorted(CAPTURE_CAUSES)}")
    envs = int(envs)
    if envs % 16:
        raise ValueError(f"envs = {envs}: the HIP step takes multiples of 16 envs")
    r, c = _grid(logdir, rows, cols)
    cfg = PL.checkpoint_cfg(logdir, envs, r, c, terrain, dr_off=dr == "off")
    env = HistoryWrapper(TrajectoryTrackingEnv(sim_device=device, headless=True, cfg=cfg, seed=seed))
    try:
        ac = PL.load_policy_module(logdir, cfg, env)
        policy = PK.fused_inference(ac, teacher=teacher, sample=None if deterministic else seed)
        traced = {}

        def attach(counter):
            factory = tracer_factory if tracer_factory is not None else trace.EpisodeTracer
            traced["base"] = counter.count.copy()
            traced["tracer"] = factory(env.env, capacity=4 * capture,
                                       want=tuple(sorted({CAPTURE_CAUSES[w] for w in capture_what})))
            env.attach_tracer(traced["tracer"])

        table, ids, steps, dt = run_episodes(env, policy, episodes_per_env, after_reset=attach if capture > 0 else None)
        out = summarize(table, ids, tuple(env.sum_keys), env.max_episode_length, env.terrain.env_tile)
        out["steps"] = int(steps)
        out["env_steps_per_s"] = float(steps * env.num_envs / dt)
        if capture > 0:
            env.detach_tracer()
            tracer = traced["tracer"]
            episodes = tracer.episodes()
            labelled = label_captures(episodes, table, ids, traced["base"], len(env.sum_keys), env.max_episode_length)
            out["captured"] = write_captures(tracer, episodes, labelled, capture_what, capture, capture_out,
                                             capture_size, env.terrain.env_tile, 1.0 / float(env.dt))
    finally:
        env.close()
    if json_path:
        with open(json_path, "w") as f:
            json.dump(out, f)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("logdir")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes-per-env", type=int, default=1)
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--cols", type=int, default=None)
    ap.add_argument("--terrain", default=None, choices=list(CF.TUNNEL_TYPES))
    ap.add_argument("--dr", default="off", choices=("off", "train"))
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--teacher", action="store_true")
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--json", default=None)
    ap.add_argument("--capture", type=int, default=0, help="write the first N failed episodes as GIFs (0: off)")
    ap.add_argument("--capture-out", default="captures")
    ap.add_argument("--capture-what", default="fall", help="comma-separated labels: fall, timeout")
    ap.add_argument("--capture-size", type=int, nargs=2, default=(360, 240), metavar=("W", "H"))
    a = ap.parse_args(argv)
    out = evaluate(a.logdir, a.envs, a.episodes_per_env, a.rows, a.cols, a.terrain, a.dr, a.deterministic, a.teacher,
                   a.seed, a.device, a.json, capture=a.capture, capture_out=a.capture_out,
                   capture_what=tuple(w for w in a.capture_what.split(",") if w), capture_size=tuple(a.capture_size))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
