"""Cfg.commands.sampling_based_planning through the env: the plan launch changes the commands columns and nothing
else, its state follows the restatement (tests/plan_ref.py) fed with the env's own planes, a host reset_idx zeroes
the commands and re-plans, and a Runner learns on it."""
import numpy as np
import pytest
import torch

from legged_tracking_amd import config as CF, env as E, plan as P
from tests import plan_ref as PR

angle_close = PR.angle_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, STEPS, MAXLEN, INTERVAL = 32, 30, 12, 5
TOL = dict(rtol=2e-5, atol=2e-5)


def make_cfg(planning, n=N):
    cfg = CF.readme_config(n_envs=n, terrain="random_pyramid", rows=4, cols=4)
    cfg.env.episode_length_s = (MAXLEN - 0.5) * CF.derived(cfg)["dt"]
    cfg.commands.sampling_based_planning = planning
    cfg.commands.plan_interval = INTERVAL
    return cfg


class Mirror:
    """The restatement, fed through the planner's own launch and mark_reset calls with the planes they saw."""

    def __init__(self, env):
        pl, cm, g = env.planner, env.cfg.commands, CF.scan_grid(env.cfg)
        self.pl, self.steps, self.planned, self.picks = pl, 0, 0, set()
        self.ref = PR.PlanRef(env.num_envs, cm.candidate_target_poses, g["x"], g["y"], cm.traj_length, cm.plan_interval,
                              cm.switch_dist, cm.switch_yaw, env.cfg.normalization.clip_observations)
        launch, mark = pl.launch, pl.mark_reset

        def launch_and_check(root, traj, idx, ep, reset, heights, obs, hist=None, commands=None):
            launch(root, traj, idx, ep, reset, heights, obs, hist, commands)
            torch.cuda.synchronize()
            self.check(*(t.cpu().numpy() for t in (root, traj, idx, ep, reset, heights, obs)),
                       None if commands is None else commands.cpu().numpy())

        def mark_reset(ids):
            mark(ids)
            self.ref.mark_reset(torch.as_tensor(ids).cpu().numpy())

        pl.launch, pl.mark_reset = launch_and_check, mark_reset

    def check(self, root, traj, idx, ep, reset, heights, obs, commands):
        ref, pl = self.ref, self.pl
        want = ref.step(root, traj, idx, ep, reset, heights)
        live = ~reset.astype(bool)
        chosen = pl.chosen.cpu().numpy()
        np.testing.assert_array_equal(chosen, ref.chosen)
        np.testing.assert_array_equal(pl.plan_buf.cpu().numpy(), ref.plan_buf)
        np.testing.assert_array_equal(pl.replan.cpu().numpy(), ref.replan)
        np.testing.assert_array_equal(pl.plan_length_buf.cpu().numpy(), ref.plan_length)
        lt = pl.local_target_poses.cpu().numpy()
        np.testing.assert_allclose(lt[live][:, :3], ref.local_target[live][:, :3], **TOL)
        assert angle_close(lt[live][:, 3:], ref.local_target[live][:, 3:])
        np.testing.assert_allclose(pl.local_relative_linear.cpu().numpy(), ref.local_rel_lin, **TOL)
        assert angle_close(pl.local_relative_rotation.cpu().numpy(), ref.local_rel_rot)
        np.testing.assert_allclose(obs[:, 3:5], want, **TOL)
        if commands is not None:
            np.testing.assert_array_equal(commands[:, :2], pl.local_relative_linear.cpu().numpy()[:, :2])
        self.steps += 1
        self.planned += int((chosen != P.NOT_PLANNED).sum())
        self.picks |= set(chosen[chosen >= 0].tolist())


def test_planning_changes_the_commands_and_nothing_else():
    envs = [E.TrajectoryTrackingEnv(sim_device=DEV, headless=True, cfg=make_cfg(p), seed=6) for p in (True, False)]
    on, off = envs
    # the flag off: no planner, no plan launch, no heights plane
    assert off.planner is None and isinstance(on.planner, P.LocalPlanner)
    with pytest.raises(AttributeError, match="sampling_based_planning"):
        off.local_target_poses
    mirror = Mirror(on)
    for env in envs:
        env.reset()
    gen = torch.Generator().manual_seed(3)
    cols = np.r_[0:3, 5:on.num_obs]
    differ = 0
    for s in range(STEPS):
        a = (0.3 * torch.randn((N, 12), generator=gen)).to(DEV)
        (o1, r1, d1, x1), (o0, r0, d0, x0) = on.step(a), off.step(a)
        assert torch.equal(o1[:, cols].view(torch.int32), o0[:, cols].view(torch.int32)), s
        assert torch.equal(r1.view(torch.int32), r0.view(torch.int32)) and torch.equal(d1, d0), s
        assert torch.equal(on.time_out_buf, off.time_out_buf) and torch.equal(x1["privileged_obs"], x0["privileged_obs"])
        assert torch.equal(on.commands, on.local_relative_linear[:, :2])
        differ += int((o1[:, 3:5] != o0[:, 3:5]).any(1).sum())
        if s == 13:  # a host reset_idx: zeroed commands now, a re-plan at the envs' next step
            ids = torch.tensor([4, 9, 20], device=DEV)
            for env in envs:
                env.reset_idx(ids)
            assert not on.commands[ids].any() and not on.local_relative_rotation[ids].any()
            assert on.plan_buf[ids].all()
        if s == 14:
            ran = ~d1[ids]
            assert ran.any() and (on.planner.chosen[ids][ran] != P.NOT_PLANNED).all()
            assert (on.plan_length_buf[ids][ran] == 0).all()
    assert mirror.steps == STEPS + 1 and differ > 0  # reset() steps once
    # every episode times out within MAXLEN steps, so each env starts two episodes at least in these 31 steps and
    # plans at the first step of each, unless it is reset in that very step
    assert mirror.planned >= N and len(mirror.picks) > 1
    assert on.planner.no_valid() == mirror.ref.no_valid
    for env in envs:
        env.close()


def test_runner_learns_with_planning_on(tmp_path):
    from legged_tracking_amd import rollout as R
    torch.manual_seed(0)
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=DEV, cfg=make_cfg(True, 64), seed=4))
    runner = R.Runner(env, device=DEV, save_dir=str(tmp_path))
    losses, update = [], runner.alg.update

    def capture():
        losses.append(update())
        return losses[-1]

    runner.alg.update = capture
    runner.learn(3)
    torch.cuda.synchronize()
    assert len(losses) == 3 and np.isfinite(np.array([[float(x) for x in l] for l in losses])).all(), losses
    assert torch.isfinite(runner.alg.storage.observation_histories).all()
    assert torch.isfinite(env.local_target_poses).all() and torch.isfinite(env.commands).all()
    assert env.planner.local_target_poses.abs().sum() > 0  # the planner ran behind the rollout's steps
    env.close()
