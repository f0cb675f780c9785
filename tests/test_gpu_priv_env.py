"""Cfg.env.priv_observe_* through the trajectory env: after every step the privileged observation equals the restatement
(tests/priv_ref.py) evaluated on the env's own public tensors, with the randomiser redrawing, the gravity schedule
drawing and zeroing, and envs timing out; a twin with friction and restitution only is bit-identical in everything
else; the aux demand does not change the vector; and a Runner learns on the six class-default columns."""
import numpy as np
import pytest
import torch

from legged_tracking_amd import config as CF, env as E, privileged as PV
from tests import priv_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, STEPS, MAXLEN, RAND_INTERVAL, GRAV_INTERVAL = 64, 40, 25, 4, 6
READ = ("friction", "restitution", "base_mass", "com_displacement", "motor_strength", "motor_offset", "body_height",
        "body_velocity", "gravity", "clock_inputs", "desired_contact_states")
SETS = {
    "defaults": {k: True for k in ("friction", "restitution", "base_mass", "com_displacement")},
    "train": {k: True for k in ("friction", "restitution")},
    "all": {k: True for k in READ},
}
# asymmetric ranges with scales that are no powers of two, and a clip that some columns reach
NORM = dict(friction_range=[0.05, 4.5], restitution_range=[0.0, 0.7], added_mass_range=[-1.0, 3.5],
            com_displacement_range=[-0.1, 0.25], motor_strength_range=[0.9, 1.15], motor_offset_range=[-0.05, 0.03],
            body_height_range=[0.0, 0.65], body_velocity_range=[-6.0, 5.0], gravity_range=[-0.7, 1.9])
CLIP = 0.9


def make_cfg(name):
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=2, cols=2)
    dt = CF.derived(cfg)["dt"]
    for k in [k for k in dir(cfg.env) if k.startswith("priv_observe_")]:
        setattr(cfg.env, k, False)
    for k in SETS[name]:
        setattr(cfg.env, "priv_observe_" + k, True)
    cfg.env.num_privileged_obs = len(PV.columns(cfg))
    for k, v in NORM.items():
        setattr(cfg.normalization, k, list(v))
    cfg.normalization.clip_observations = CLIP
    cfg.env.episode_length_s = (MAXLEN - 0.5) * dt
    d = cfg.domain_rand
    d.randomize_rigids_after_start, d.rand_interval_s = True, (RAND_INTERVAL - 0.5) * dt
    d.randomize_base_mass = d.randomize_friction = d.randomize_restitution = True
    d.randomize_motor_strength = d.randomize_motor_offset = True
    d.randomize_gravity, d.gravity_rand_interval_s, d.gravity_impulse_duration = True, (GRAV_INTERVAL - 0.5) * dt, 0.5
    dd = CF.derived(cfg)
    assert (dd["max_episode_length"], dd["rand_interval"], dd["gravity_rand_interval"], dd["gravity_rand_duration"]) \
        == (MAXLEN, RAND_INTERVAL, GRAV_INTERVAL, 3)
    return cfg


def make_env(name, seed=9):
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=DEV, headless=True, cfg=make_cfg(name), seed=seed))
    env.reset()
    # episode lengths spread over the last steps before the time-out, so that envs time out throughout the run
    ep = torch.from_numpy(np.random.default_rng(2).integers(0, MAXLEN, N).astype(np.int32)).to(DEV)
    env.env.episode_length_buf = ep
    return env


def run(env, record=None, demand_aux=True):
    """STEPS steps of seeded actions; per step the outputs as numpy, and `record(step, priv tensor, info)`."""
    gen = torch.Generator().manual_seed(17)
    if not demand_aux:
        env.env.set_output_demand(aux=False)
    out = []
    for s in range(STEPS):
        od, rew, reset, info = env.step((0.4 * torch.randn((N, 12), generator=gen)).to(DEV))
        if record is not None:
            record(s, od, info)
        out.append(dict(obs=od["obs"].cpu().numpy().copy(), priv=od["privileged_obs"].cpu().numpy().copy(),
                        rew=rew.cpu().numpy().copy(), reset=reset.cpu().numpy().copy(),
                        time_out=env.env.time_out_buf.cpu().numpy().copy()))
    return out


def expected(env, cols):
    """The restatement on the env's own public tensors."""
    e = env.env
    planes = dict(friction=e.friction_coeffs, restitution=e.restitutions, payloads=e.payloads,
                  motor_strength=e.motor_strengths, motor_offset=e.motor_offsets, root=e.root_states,
                  aux=e.base_lin_vel)
    return PR.assemble(cols, CLIP, N, e.gravities, **{k: v.cpu().numpy() for k, v in planes.items()})


@pytest.fixture(scope="module")
def twin_run():
    """The run of the env with friction and restitution only: what every other flag set must leave unchanged."""
    env = make_env("train")
    assert env.env.privileged is None and env.env._kout is env.env._out and env.env.randomizer is not None
    out = run(env)
    env.close()
    return out


@pytest.mark.parametrize("name", ["defaults", "all"])
def test_env_follows_the_restatement(name, twin_run):
    env = make_env(name)
    e = env.env
    cols = PV.columns(e.cfg)
    w = len(cols)
    p = e.privileged
    assert isinstance(p, PV.Privileged) and p.width == w == e.num_privileged_obs == PR.WIDTHS[name]
    assert p.names == [c[0] for c in cols] and e.payloads is e.randomizer.payloads
    seen = dict(grav_on=0, grav_zeroed=0, clipped=0, inside=0)
    state = dict(grav_was_on=False, friction=e.friction_coeffs.clone(), redrawn=0)

    def record(s, od, info):
        pv = od["privileged_obs"]
        assert pv.shape == (N, w) and info["privileged_obs"].shape == (N, w)
        assert torch.equal(pv, info["privileged_obs"]) and torch.equal(pv, e.privileged_obs_buf)
        assert torch.equal(pv, env.get_observations()["privileged_obs"])
        got = pv.cpu().numpy()
        np.testing.assert_array_equal(PR.bits(got), PR.bits(expected(env, cols)), err_msg=f"{name} step {s}")
        on = bool(np.any(e.gravities != 0))
        seen["grav_on"] += on
        seen["grav_zeroed"] += state["grav_was_on"] and not on
        state["grav_was_on"] = on
        seen["clipped"] += int((np.abs(got) == np.float32(CLIP)).sum())
        seen["inside"] += int((np.abs(got) < np.float32(CLIP)).sum())
        state["redrawn"] += int((e.friction_coeffs != state["friction"]).sum())
        state["friction"] = e.friction_coeffs.clone()

    out = run(env, record)
    # the run held what it was set up for: draws and zeroings of the gravity, redraws, time-outs, both sides of the clip
    assert seen["grav_on"] and seen["grav_zeroed"] and state["redrawn"] > N and seen["clipped"] and seen["inside"]
    assert sum(int(o["time_out"].sum()) for o in out) > 0 and sum(int(o["reset"].sum()) for o in out) > N // 2
    # the twin: everything but the privileged vector bit-identical, its two columns the wide vector's first two
    for s, (a, b) in enumerate(zip(out, twin_run)):
        for k in ("obs", "rew"):
            np.testing.assert_array_equal(PR.bits(a[k]), PR.bits(b[k]), err_msg=f"{k} step {s}")
        for k in ("reset", "time_out"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{k} step {s}")
        assert b["priv"].shape == (N, 2)
        np.testing.assert_array_equal(PR.bits(a["priv"][:, :2]), PR.bits(b["priv"]), err_msg=f"priv step {s}")
    if name == "all":
        # the same run while the rollout's demand is in effect: the step keeps storing aux for the assembler, and
        # reading base_lin_vel through the env keeps raising
        again = make_env(name)
        assert again.env.privileged.needs_aux
        out2 = run(again, demand_aux=False)
        with pytest.raises(RuntimeError, match="aux"):
            again.env.base_lin_vel
        for s, (a, b) in enumerate(zip(out, out2)):
            np.testing.assert_array_equal(PR.bits(a["priv"]), PR.bits(b["priv"]), err_msg=f"aux demand, step {s}")
        again.close()
    else:
        assert not p.needs_aux
    env.close()


def test_runner_learns_on_the_class_defaults(tmp_path):
    from legged_tracking_amd import rollout as R

    class Args(R.RunnerArgs):
        num_steps_per_env = 4

    torch.manual_seed(0)
    env = make_env("defaults", seed=4)
    assert env.num_privileged_obs == 6
    runner = R.Runner(env, device=DEV, runner_args=Args, save_dir=str(tmp_path))
    assert runner.alg.fused is not None  # the fused policy kernels take 1 .. 8 privileged columns
    seen, losses = [env.get_observations()["privileged_obs"].clone()], []
    step, update = env.step, runner.alg.update

    def stepping(actions):
        ret = step(actions)
        assert ret[0]["privileged_obs"].shape == (N, 6)
        seen.append(ret[0]["privileged_obs"].clone())
        return ret

    def capture():
        losses.append(update())
        return losses[-1]

    env.step, runner.alg.update = stepping, capture
    runner.learn(2)
    torch.cuda.synchronize()
    assert len(losses) == 2 and np.isfinite(np.array([[float(x) for x in l] for l in losses])).all(), losses
    # the storage of the second iteration: what the policy acted on at step t is what the env returned before it
    st = runner.alg.storage.privileged_observations
    assert st.shape == (4, N, 6) and len(seen) == 9
    for t in range(4):
        assert torch.equal(st[t], seen[4 + t]), t
    cols = PV.columns(env.env.cfg)
    np.testing.assert_array_equal(PR.bits(seen[-1].cpu().numpy()), PR.bits(expected(env, cols)))
    env.close()
