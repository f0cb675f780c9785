"""Fixture of the reference's privileged observation (container-only test infrastructure).

Imports the reference behind the offline stand-ins of tests/golden/refstubs, as make_golden_dr.py does, and calls its
own LeggedRobot.compute_observations (legged_robot_trajectory_tracking.py:357-590) on a stub namespace that holds just
what the function reads: cfg, device, num_envs, num_actor, the tensors of the first 41 observation columns (with
observe_heights, add_noise and every other observation flag off), and the sources of the privileged block --
friction_coeffs, restitutions, payloads, com_displacements (zeros, :1336), motor_strengths, motor_offsets, root_states,
base_lin_vel, gravities, clock_inputs and desired_contact_states (zeros, :1361 and :1247).  The clip of step (:108-111)
is restated.

32 envs run for 10 steps.  Between steps this generator moves the roots, sets base_lin_vel (the value of :132),
redraws some envs' friction, restitution, payloads and motor planes, changes gravities on some steps (a draw, later
zeroed, as :826-830 does), and resets a few envs: a new root with a new z, while base_lin_vel is left as it was
(reset_idx does not refresh it).  All values are multiples of 1 / 64.  The same inputs run under four flag sets; the
normalisation ranges are asymmetric with scales that are no powers of two, and clip_observations is small enough that
some columns of every set clip.

Recorded: the input planes per step as compute_observations saw them, gravities, the reset mask, and per flag set the
clipped privileged_obs_buf.

Usage: python tests/golden/make_golden_priv.py [reference root]   (writes tests/golden/priv_cases.npz)
"""
import os
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

N, STEPS = 32, 10
CLIP_OBS = 1.0
NORM = dict(friction_range=[0.05, 4.5], ground_friction_range=[0.05, 4.5], restitution_range=[0.0, 0.7],
            added_mass_range=[-1.0, 3.5], com_displacement_range=[-0.1, 0.25], motor_strength_range=[0.9, 1.15],
            motor_offset_range=[-0.05, 0.03], body_height_range=[0.0, 0.65], body_velocity_range=[-6.0, 5.0],
            gravity_range=[-0.7, 1.9])
READ = ("friction", "restitution", "base_mass", "com_displacement", "motor_strength", "motor_offset", "body_height",
        "body_velocity", "gravity", "clock_inputs", "desired_contact_states")  # the flags the function reads (+ ground)
OBS_OFF = ("observe_heights", "timestep_in_obs", "observe_two_prev_actions", "observe_timing_parameter",
           "observe_clock_inputs", "observe_vel", "observe_only_ang_vel", "observe_only_lin_vel", "observe_yaw",
           "observe_contact_states")


def sixty_fourths(rng, lo, hi, shape):
    """Multiples of 1 / 64 in [lo, hi] (exact in f32)."""
    return torch.from_numpy((rng.integers(int(np.ceil(lo * 64)), int(np.floor(hi * 64)) + 1, shape) / 64.0)
                            .astype(np.float32))


def flag_sets(defaults):
    off = {k: False for k in defaults}
    return {
        "defaults": dict(defaults),
        "train": dict(off, priv_observe_friction=True, priv_observe_restitution=True),
        "all": dict(defaults, priv_observe_ground_friction=False, **{"priv_observe_" + k: True for k in READ}),
        "sparse": dict(off, priv_observe_motor_offset=True, priv_observe_body_velocity=True,
                       priv_observe_gravity=True),
    }


def main():
    from go1_gym.envs.base.legged_robot_trajectory_tracking import LeggedRobot as LR
    from go1_gym.envs.base.legged_robot_trajectory_tracking_config import Cfg
    defaults = {k: bool(getattr(Cfg.env, k)) for k in sorted(dir(Cfg.env)) if k.startswith("priv_observe_")}
    assert int(Cfg.env.num_privileged_obs) == 6
    sets = flag_sets(defaults)
    rng = np.random.default_rng(4200)

    ns = types.SimpleNamespace()
    ns.device, ns.num_envs, ns.num_train_envs, ns.num_actor, ns.num_actuated_dof = "cpu", N, N, 1, 12
    ns.add_noise = False
    ns.obs_scales = types.SimpleNamespace(dof_pos=1.0, dof_vel=0.05)
    ns.projected_gravity, ns.commands, ns.commands_scale = torch.zeros(N, 3), torch.zeros(N, 2), torch.ones(2)
    ns.dof_pos, ns.default_dof_pos, ns.dof_vel, ns.actions = (torch.zeros(N, 12) for _ in range(4))
    ns.com_displacements = torch.zeros(N, 3)                                   # :1336
    ns.clock_inputs, ns.desired_contact_states = torch.zeros(N, 4), torch.zeros(N, 4)  # :1361, :1247
    ns.friction_coeffs = sixty_fourths(rng, 0.1, 5.5, (N, 1))
    ns.restitutions = sixty_fourths(rng, 0.0, 1.0, (N, 1))
    ns.payloads = sixty_fourths(rng, -1.0, 3.0, (N,))
    ns.motor_strengths = sixty_fourths(rng, 0.9, 1.1, (N, 12))
    ns.motor_offsets = sixty_fourths(rng, -0.0625, 0.0625, (N, 12))
    ns.root_states = sixty_fourths(rng, -4.0, 4.0, (N, 13))
    ns.root_states[:, 2] = sixty_fourths(rng, 0.0, 1.0, (N,))
    ns.base_lin_vel = sixty_fourths(rng, -7.0, 7.0, (N, 3))
    ns.gravities = torch.zeros(N, 3)

    keys = ("friction", "restitution", "payloads", "motor_strength", "motor_offset", "root", "base_lin_vel",
            "gravities", "reset")
    rec = {k: [] for k in keys}
    priv = {name: [] for name in sets}
    for step in range(STEPS):
        # the "physics" and :130-133: every root moves, base_lin_vel is the new body-frame velocity
        ns.root_states = ns.root_states + sixty_fourths(rng, -0.125, 0.125, (N, 13))
        ns.base_lin_vel = sixty_fourths(rng, -7.0, 7.0, (N, 3))
        # the rigid props and motors of a few envs are redrawn (:822-833)
        ids = torch.from_numpy(rng.choice(N, 6, replace=False))
        ns.friction_coeffs[ids] = sixty_fourths(rng, 0.1, 5.5, (6, 1))
        ns.restitutions[ids] = sixty_fourths(rng, 0.0, 1.0, (6, 1))
        ns.payloads[ids] = sixty_fourths(rng, -1.0, 3.0, (6,))
        ns.motor_strengths[ids] = sixty_fourths(rng, 0.9, 1.1, (6, 12))
        ns.motor_offsets[ids] = sixty_fourths(rng, -0.0625, 0.0625, (6, 12))
        # the gravity schedule (:826-830): a draw on some steps, zeroed two steps later
        if step % 4 == 1:
            ns.gravities[:, :] = sixty_fourths(rng, -1.0, 1.0, (3,)).unsqueeze(0)
        elif step % 4 == 3:
            ns.gravities[:, :] = 0.0
        elif step % 4 == 2:
            ns.gravities[:, :] = sixty_fourths(rng, -1.0, 1.0, (3,)).unsqueeze(0)
        # reset_idx: a new root with a new z; base_lin_vel is not refreshed
        reset = np.zeros(N, bool)
        reset[rng.choice(N, 3, replace=False)] = True
        rid = torch.from_numpy(np.nonzero(reset)[0])
        ns.root_states[rid] = sixty_fourths(rng, -4.0, 4.0, (3, 13))
        ns.root_states[rid, 2] = sixty_fourths(rng, 0.0, 1.0, (3,))
        for k, v in (("friction", ns.friction_coeffs), ("restitution", ns.restitutions), ("payloads", ns.payloads),
                     ("motor_strength", ns.motor_strengths), ("motor_offset", ns.motor_offsets),
                     ("root", ns.root_states), ("base_lin_vel", ns.base_lin_vel), ("gravities", ns.gravities[0])):
            rec[k].append(v.numpy().copy())
        rec["reset"].append(reset)
        for name, flags in sets.items():
            env = types.SimpleNamespace(observe_command=True, num_observations=41, **{k: False for k in OBS_OFF},
                                        **flags)
            width = sum(n * flags["priv_observe_" + k] for k, n in zip(READ, (1, 1, 1, 3, 12, 12, 1, 3, 3, 4, 4)))
            env.num_privileged_obs = width
            ns.cfg = types.SimpleNamespace(env=env, normalization=types.SimpleNamespace(
                clip_observations=CLIP_OBS, **NORM))
            LR.compute_observations(ns)
            assert ns.obs_buf.shape == (N, 41) and ns.privileged_obs_buf.shape == (N, width)
            priv[name].append(torch.clip(ns.privileged_obs_buf, -CLIP_OBS, CLIP_OBS).numpy().copy())  # :108-111

    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(clip_obs=np.float64(CLIP_OBS), norm_names=np.array(sorted(NORM)),
               norm=np.array([NORM[k] for k in sorted(NORM)], np.float64), flag_names=np.array(sorted(defaults)))
    for name, flags in sets.items():
        p = np.stack(priv[name])
        assert p.dtype == np.float32
        out[name + "/flags"] = np.array([flags[k] for k in sorted(defaults)], bool)
        out[name + "/priv"] = p
        clipped, inside = int((np.abs(p) == CLIP_OBS).sum()), int((np.abs(p) < CLIP_OBS).sum())
        print(f"{name}: width {p.shape[2]}, clipped {clipped}, inside {inside}")
        assert clipped and inside
    assert [out[n + "/priv"].shape[2] for n in sets] == [6, 2, 45, 18]
    # a recorded gravity for which the division and the multiply by the reciprocal differ in f32
    g = out["gravities"].astype(np.float32)
    scale, shift = np.float32(2.0 / (1.9 - -0.7)), np.float32((1.9 + -0.7) / 2.0)
    differ = int(((g - shift) / scale != (g - shift) * (np.float32(1.0) / scale)).sum())
    print("gravity values where / and * (1 / scale) differ:", differ, "of", g.size)
    assert differ
    # an env that resets while its base_lin_vel is nonzero
    assert (out["base_lin_vel"][out["reset"]] != 0).any()
    path = os.path.join(HERE, "priv_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
