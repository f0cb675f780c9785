"""Hip capsule contact (the reference's scene keeps the hip collision cylinders,
go1.urdf:106-111 / :229-234, as capsules, legged_robot_trajectory_tracking_config.py:214-215).

The native model carries each hip capsule as the two ends of its segment (model.py HIP_CAPSULE_*),
spheres of the capsule's radius on the hip link, in the f64 oracle (oracle/go1_oracle.c phys_substep
j == 0) and in the HIP integrator (csrc/go1_phys.h phys_substep, role 1).  Scenario: the trunk rolled 34-46
degrees to the left with the legs folded up, lowered until the left hips' outer capsule ends press
2-10 mm into the plane, so the hips are the only bodies in contact.

Effects stated and tested:
  * the left hips (FL, RL) report an upward contact force, every other body (right hips, legs,
    trunk) none;
  * collision_count does not move: the reference penalises contacts on thighs and calves only
    (train.py:80 penalize_contacts_on) and terminates on the base, the hips are in neither;
  * the static stance is unchanged (test_physics_invariants.py): standing, the hips are 0.2 m above
    the plane and report no force;
  * the HIP kernel's hip forces and the resulting state match the f64 oracle's (floor: 1.7e-5 relative,
    root 1e-5; ceiling, through the tunnel-tile terrain path: 7.8e-5, root 1.8e-5, measured on MI355X).
A second scenario presses the left hips into a flat tunnel ceiling (the trunk rolled the other way).
"""
import numpy as np
import pytest

from tests import physics_drive as D

N = 64
GZ = (0.0, 0.0, -9.81)
HIPS = [1, 5, 9, 13]  # FL, FR, RL, RR hip bodies in the 17-body contact_forces layout


def _rolled(n=N, seed=5):
    c, td, ter, st, scales = D.setup(n=n, seed=seed)
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-0.8, -0.6, n)  # roll: left side down
    st["root"][:, 3:7] = np.stack([np.sin(phi / 2), 0 * phi, 0 * phi, np.cos(phi / 2)], 1)
    st["root"][:, 7:13] = 0.0
    st["dof_pos"][:] = np.tile([0.0, 3.0, -1.0], 4)  # thighs up, calves folded: the feet clear the plane
    st["dof_vel"][:] = 0.0
    depth = rng.uniform(0.002, 0.01, n)
    outer = 0.04675 + 0.065  # hip joint y + the capsule segment's outer end (model.py)
    st["root"][:, 2] = -outer * np.sin(phi) + 0.046 - depth
    return c, td, ter, st, scales


def _check_contacts(cf, st):
    cf = cf.reshape(st.n, 17, 3)
    left, right = cf[:, [1, 9]], cf[:, [5, 13]]
    assert (left[..., 2] > 1.0).all(), left[..., 2].min()  # every left hip pushed up
    others = np.delete(cf, [1, 9], axis=1)
    assert np.abs(others).max() == 0.0, np.abs(others).max()
    assert np.abs(right).max() == 0.0
    assert (st["collision_count"] == 0).all()


def test_oracle_hip_capsule_contact():
    c, td, ter, st, scales = _rolled()
    s, cf, reset = next(D.oracle_roll(c, ter, st, scales, 1, GZ))
    assert not reset.any()
    _check_contacts(cf, s)


@pytest.mark.gpu
def test_hip_capsule_contact_matches_oracle():
    c, td, ter, st, scales = _rolled()
    ref = _rolled()[3]
    steps = 3
    hip = list(D.hip_roll(c, td, st, scales, steps, GZ))
    orc = []
    for s, cf, reset in D.oracle_roll(c, ter, ref, scales, steps, GZ):
        orc.append((s["root"].copy(), s["dof_vel"].copy(), cf.copy(), reset.copy()))
    for t, ((hs, hcf, hreset), (oroot, odv, ocf, oreset)) in enumerate(zip(hip, orc)):
        assert not hreset.any() and not oreset.any()
        if t == 0:
            _check_contacts(hcf, hs)
        h = hcf.reshape(N, 17, 3)[:, HIPS]
        o = ocf.reshape(N, 17, 3)[:, HIPS]
        scale = np.abs(o).max()
        err = np.abs(h - o).max() / scale
        root_err = np.abs(hs["root"] - oroot).max()
        print(f"\nstep {t}: hip force max {scale:.1f} N, rel err {err:.2e}, root err {root_err:.2e}")
        assert err < 2e-2, err
        assert root_err < 5e-3, root_err


def _ceiling(n=N, seed=7, height=0.6):
    """Trunk rolled 34-46 degrees right side down (left side up) under a flat ceiling `height` m above a flat floor (tunnel
    tiles, so the kernel's terrain path runs: LDS patch, bilinear heights), legs in the default stance, so
    the left hips' outer capsule ends press 2-10 mm into the ceiling and nothing else touches."""
    from legged_tracking_amd import config as CF, layout as L, terrain as T
    from oracle import oracle as O
    cfg = CF.readme_config(n_envs=n, terrain="single_path", rows=2, cols=2)
    cfg.domain_rand.randomize_motor_strength = False
    c = CF.build_abi_config(cfg)
    td = T.build(cfg, n, np.random.RandomState(11))
    td.tiles[:, 0] = height  # layer 0 ceiling
    td.tiles[:, 1] = 0.0     # layer 1 floor
    ter = O.NpTerrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    st = O.NpState(n, cfg=c)
    st["friction"][:, 0] = 1.0
    O.reset_envs(c, st, ter, np.ones(n, np.uint8), rng_seed=seed, rng_step=0)
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0.6, 0.8, n)  # roll: left side up
    st["root"][:, 3:7] = np.stack([np.sin(phi / 2), 0 * phi, 0 * phi, np.cos(phi / 2)], 1)
    st["root"][:, 7:13] = 0.0
    st["dof_pos"][:] = np.array(L.DEFAULT_DOF_POS, np.float32)
    st["dof_vel"][:] = 0.0
    st["motor_strength"][:] = 0.0
    st["payload"][:] = 0.0
    st["episode_length"][:, 0] = 1
    depth = rng.uniform(0.002, 0.01, n)
    outer = 0.04675 + 0.065
    ext = td.tiles.shape[2] * 0.05, td.tiles.shape[3] * 0.05  # tile extent (x, y), horizontal scale 0.05
    st["root"][:, 0] = td.env_terrain_origin[:, 0] + 0.5 * ext[0]  # mid-tile (world = terrain frame + origin)
    st["root"][:, 1] = td.env_terrain_origin[:, 1] + 0.5 * ext[1]
    st["root"][:, 2] = height + depth - 0.046 - outer * np.sin(phi)
    scales = CF.reward_scale_vector(CF.derived(cfg)["reward_scales"])
    return c, td, ter, st, scales


def _check_ceiling(cf, n):
    # every left hip in contact, nothing else; the reported force is the explicit part of the linearised
    # contact force, so over the 20 ms step the rebound can turn its sign: the
    # direction is checked where the hips still press (the median env)
    cf = cf.reshape(n, 17, 3)
    assert (np.linalg.norm(cf[:, [1, 9]], axis=2) > 0.1).all()
    assert np.median(cf[:, [1, 9], 2]) < -1.0, np.median(cf[:, [1, 9], 2])
    assert np.abs(np.delete(cf, [1, 9], axis=1)).max() == 0.0


G0 = (0.0, 0.0, 0.0)  # the ceiling scenario without gravity: the trunk stays pressed against the ceiling


def test_oracle_hip_capsule_ceiling_contact():
    c, td, ter, st, scales = _ceiling()
    s, cf, reset = next(D.oracle_roll(c, ter, st, scales, 1, G0))
    _check_ceiling(cf, st.n)


@pytest.mark.gpu
def test_hip_capsule_ceiling_contact_matches_oracle():
    c, td, ter, st, scales = _ceiling()
    ref = _ceiling()[3]
    hip = list(D.hip_roll(c, td, st, scales, 2, G0))
    orc = [(s["root"].copy(), cf.copy()) for s, cf, _ in D.oracle_roll(c, ter, ref, scales, 2, G0)]
    for t, ((hs, hcf, _), (oroot, ocf)) in enumerate(zip(hip, orc)):
        if t == 0:
            _check_ceiling(hcf, N)
        h = hcf.reshape(N, 17, 3)[:, HIPS]
        o = ocf.reshape(N, 17, 3)[:, HIPS]
        err = np.abs(h - o).max() / max(np.abs(o).max(), 1.0)  # the rebound separates them by step 1
        root_err = np.abs(hs["root"] - oroot).max()
        print(f"\nceiling step {t}: hip force max {np.abs(o).max():.1f} N, rel err {err:.2e}, root err {root_err:.2e}")
        assert err < 2e-2, err
        assert root_err < 5e-3, root_err
