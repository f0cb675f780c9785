"""The episode tracer behind the envs on the MI355X: 16 envs whose episodes last 6 steps, zero actions, 30 steps, so
every env times out several times whatever the physics does.  After each step the state planes and the step's reset /
time_out outputs are copied to the host and pushed through tests/trace_ref.py; episodes() must equal that exactly,
a host reset_idx must start new episodes without a capture, and render_episode must give, byte for byte, the frames
that a live render of the same env gave after the same steps (waypoint marker included).  Then evaluate --capture."""
import json
import os

import numpy as np
import pytest
import torch

from legged_tracking_amd import config as CF, env as E, evaluate as EV, render as R, rollout as RO, trace as T
from tests import trace_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, MAXLEN, STEPS, W, H = 16, 6, 30, 32, 24


def tracking_env(extra=()):
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=4, cols=4, extra_argv=tuple(extra))
    cfg.env.episode_length_s = (MAXLEN - 0.5) * CF.derived(cfg)["dt"]
    env = E.TrajectoryTrackingEnv(sim_device=DEV, headless=True, cfg=cfg, seed=3)
    assert int(env.max_episode_length) == MAXLEN
    return env


def velocity_env():
    from legged_tracking_amd import velocity as VEL, velocity_config as VC
    cfg = VC.train_velocity_config(n_envs=N)
    cfg.env.episode_length_s = (MAXLEN - 0.5) * VC.vel_derived(cfg)["dt"]
    env = VEL.VelocityTrackingEasyEnv(sim_device=DEV, cfg=cfg, seed=1)
    assert int(env.max_episode_length) == MAXLEN
    return env


def drive(env, host_reset_at=None):
    """-> (tracer, reference, live frames (STEPS, N, H, W, 4))."""
    env.reset()
    st = env._sim.state
    has_wp = True
    try:
        st["trajectory"]
    except KeyError:
        has_wp = False
    tracer = T.EpisodeTracer(env, capacity=256)
    assert tracer.depth == MAXLEN + 1 and tracer.tw == (st["trajectory"].shape[1] if has_wp else 0)
    ref = TR.TraceRef(N, MAXLEN + 1, 256, tracer.tw)
    if has_wp:
        ref.traj_start[:] = TR.bits(st["trajectory"].cpu().numpy())
    env.attach_tracer(tracer)
    zero = torch.zeros(N, env.num_actions, device=DEV)
    live = []
    for s in range(STEPS):
        env.step(zero)
        traj = st["trajectory"].cpu().numpy() if has_wp else None
        ref.push(st["root"].cpu().numpy(), st["dof_pos"].cpu().numpy(), env.reset_buf.cpu().numpy(),
                 env.time_out_buf.cpu().numpy(),
                 wp_index=st["curr_pose_index"].cpu().numpy()[:, 0] if has_wp else None, traj=traj)
        live.append(env._get_renderer().render(tuple(range(N)), W, H, R.MODE_LOOK_FROM_BACK, 0))
        if s == host_reset_at:
            env.reset_idx([3, 7])
            ref.mark_reset([3, 7], traj=st["trajectory"].cpu().numpy() if has_wp else None)
    env.detach_tracer()
    return tracer, ref, np.stack(live)


def check(tracer, ref, live, has_wp):
    assert tracer.counts() == ref.counts() and ref.dropped == 0
    meta, rows, traj = ref.sorted_captures()
    eps = tracer.episodes()
    assert len(eps) == len(meta) >= 3 * N  # every env timed out several times
    assert any(e.cause == T.TIMEOUT and e.kept == MAXLEN + 1 == e.full_length for e in eps)
    for e, m, r, t in zip(eps, meta, rows, traj):
        assert [e.env, e.ordinal, e.end_push, e.kept, e.full_length, e.cause] == m[:6].tolist()
        k = e.kept
        np.testing.assert_array_equal(e.root.view(np.uint32), r[:k, :13])
        np.testing.assert_array_equal(e.dof_pos.view(np.uint32), r[:k, 13:25])
        np.testing.assert_array_equal(e.curr_pose_index.view(np.uint32), r[:k, 25])
        if has_wp:
            np.testing.assert_array_equal(e.trajectory.view(np.uint32), t)
        else:
            assert e.trajectory is None and not r[:, 25].any()
    np.testing.assert_array_equal(tracer.ep_start.cpu().numpy(), ref.ep_start)
    np.testing.assert_array_equal(tracer.ep_ordinal.cpu().numpy(), ref.ep_ordinal)
    np.testing.assert_array_equal(tracer.ring.cpu().numpy().view(np.uint32), ref.ring)
    # rendering: a few whole episodes, a 1-row one if there is any
    full = [i for i, e in enumerate(eps) if e.kept == MAXLEN + 1]
    pick = full[:2] + full[-1:] + [i for i, e in enumerate(eps) if 0 < e.kept < MAXLEN][:2]
    for i in pick:
        e = eps[i]
        frames = tracer.render_episode(i, W, H, R.MODE_LOOK_FROM_BACK, 0)
        assert frames.shape == (e.kept, H, W, 4) and frames.dtype == np.uint8
        want = live[e.end_push - e.kept:e.end_push, e.env]
        np.testing.assert_array_equal(frames, want)
        assert len(np.unique(frames.reshape(-1, 4), axis=0)) > 2  # a picture, not a blank
    return eps


@pytest.mark.parametrize("extra", [(), ("--random_target",)], ids=["fixed_target", "random_target"])
def test_tracking_env_episodes_equal_the_reference(extra):
    env = tracking_env(extra)
    try:
        tracer, ref, live = drive(env, host_reset_at=12)
        assert tracer.tw == (60 if extra else 6)
        eps = check(tracer, ref, live, True)
        # the host reset at push 12 began new episodes for envs 3 and 7 (ordinal + 1, no capture of the cut one)
        for e in (3, 7):
            mine = [x for x in eps if x.env == e]
            assert [x.ordinal for x in mine] != list(range(len(mine)))  # one ordinal has no capture
            assert not any(x.end_push - x.full_length < 13 < x.end_push for x in mine)
            after = [x for x in mine if x.end_push > 13]
            assert after[0].end_push - after[0].full_length == 13
    finally:
        env.close()


def test_velocity_env_episodes_equal_the_reference():
    env = velocity_env()
    try:
        tracer, ref, live = drive(env)
        check(tracer, ref, live, False)
    finally:
        env.close()


def test_no_tracer_no_launch():
    env = tracking_env()
    try:
        assert env._tracer is None
        tracer = T.EpisodeTracer(env, capacity=4)
        env.reset()
        env.step(torch.zeros(N, env.num_actions, device=DEV))
        assert tracer.pushes == 0 and tracer.counts() == (0, 0)
        env.attach_tracer(tracer)
        with pytest.raises(RuntimeError):
            env.attach_tracer(T.EpisodeTracer(env, capacity=4))
    finally:
        env.close()


def test_evaluate_capture_writes_labelled_gifs(tmp_path):
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=2, cols=2)
    cfg.env.episode_length_s = (MAXLEN - 0.5) * CF.derived(cfg)["dt"]
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=DEV, headless=True, cfg=cfg, seed=3))
    torch.manual_seed(1)
    RO.Runner(env, device=DEV, save_dir=str(tmp_path / "ckpt")).save()
    env.close()
    base = [str(tmp_path / "ckpt"), "--envs", "16", "--episodes-per-env", "2", "--rows", "2", "--cols", "2", "--seed", "7"]
    EV.main(base + ["--json", str(tmp_path / "plain.json")])
    EV.main(base + ["--json", str(tmp_path / "cap.json"), "--capture", "2", "--capture-what", "timeout",
                    "--capture-out", str(tmp_path / "gifs"), "--capture-size", "48", "32"])
    plain, cap = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "cap.json"))
    assert "captured" not in plain and set(cap) == set(plain) | {"captured"}
    drop = ("env_steps_per_s", "captured")
    assert {k: v for k, v in cap.items() if k not in drop} == {k: v for k, v in plain.items() if k not in drop}
    assert plain["timeout_rate"] > 0
    got = cap["captured"]
    assert len(got) == 2 and sorted(os.listdir(tmp_path / "gifs")) == sorted(os.path.basename(c["file"]) for c in got)
    for k, c in enumerate(got):
        assert os.path.basename(c["file"]) == f"episode_{k}_env{c['env']}_timeout.gif"
        assert c["label"] == "timeout" and c["length"] == MAXLEN + 1 and 0 < c["rows_kept"] <= MAXLEN + 1
        assert os.path.getsize(c["file"]) > 200
        from PIL import Image
        im = Image.open(c["file"])
        assert im.size == (48, 32) and 1 <= getattr(im, "n_frames", 1) <= c["rows_kept"]
