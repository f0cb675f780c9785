"""Four control steps of the fused step kernel from poses that load every contact class, against a recording of the
build before the capsule search changed its lane layout (tests/golden/step_contact_classes/step_contact_classes.npz,
written by tests/golden/step_contact_classes/make_golden_step_contact_classes.py on the GPU).

tests/test_gpu_step_replay.py starts from standing robots: feet, and what a few N(0, 1) actions bring down.  Here
the 32 envs on single_path (the README configuration, the specialised kernel) start in four groups of eight:
  standing   the reset pose;
  side       rolled by +-90 degrees just above the floor: hips, thighs and calves of one side down;
  back       rolled by 180 degrees: the hip capsules and the trunk's corners and faces down;
  ceiling    crouched, raised into the lowest ceiling over the tile's path: trunk and hips against the upper layer.
The poses were chosen with the f64 oracle on the CPU (the first test below counts the classes there, without a
GPU); the GPU test counts them in the recording before it compares anything, so an empty recording cannot pass.
The change moves segments between lanes and drops candidates that cannot exist; no operation on a value changes, so
every output, every state plane, the contact forces of every step and aux are reproduced bit for bit."""
import os

import numpy as np
import pytest

from legged_tracking_amd import abi, config as CF, terrain as T
from oracle import oracle as O
from tests import golden_io as G

N = 32
STEPS = 4
FIXTURE = os.path.join(G.GOLDEN, "step_contact_classes", "step_contact_classes.npz")
DEV = "cuda:0"
PER_STEP = ("obs", "privileged_obs", "rew", "reset", "time_outs", "contact_forces")
# bodies: the trunk, then per leg hip, thigh, calf, foot
CLASSES = {"trunk": [0], "hip": [1, 5, 9, 13], "thigh": [2, 6, 10, 14], "calf": [3, 7, 11, 15],
           "foot": [4, 8, 12, 16]}
MIN_ENVS, MIN_CEILING = 4, 2  # envs with a force on each class; envs with one from the ceiling layer
CROUCH = (0.0, 1.4, -2.6)
SIDE_HIP = -0.5  # (the sign and size by trial in the oracle: calves down in 5 of the 8)


def _heights(tile, hs, x, y):
    """(floor, ceiling) vertex heights under (x, y) of the tile frame"""
    i = int(np.clip(np.floor(x / hs), 0, tile.shape[1] - 1))
    j = int(np.clip(np.floor(y / hs), 0, tile.shape[2] - 1))
    return float(tile[1, i, j]), float(tile[0, i, j])


def setup():
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=2, cols=4)
    c = CF.build_abi_config(cfg)
    td = T.build(cfg, N, np.random.RandomState(11))
    ter = O.NpTerrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    st = O.NpState(N, cfg=c)
    rng = np.random.default_rng(29)
    st["friction"][:, 0] = rng.uniform(0.1, 3.0, N)
    st["restitution"][:, 0] = rng.uniform(0.0, 0.4, N)
    st["payload"][:, 0] = rng.uniform(-1.0, 3.0, N)
    O.reset_envs(c, st, ter, np.ones(N, np.uint8), rng_seed=29, rng_step=0)
    hs = float(c.horizontal_scale)
    root = st["root"]
    for e in range(8, N):
        group = e // 8
        tile, org = td.tiles[td.env_tile[e]], td.env_terrain_origin[e]
        root[e, 7:13] = 0.0
        st["dof_vel"][e] = 0.0
        yaw = rng.uniform(-0.5, 0.5)
        cy, sy = np.cos(yaw / 2), np.sin(yaw / 2)
        if group == 1:    # on a side: roll +-90 degrees (then the yaw), the lower thighs about 1 cm into the floor
            s = 1.0 if e % 2 else -1.0
            q = (s * np.sqrt(0.5) * cy, s * np.sqrt(0.5) * sy, sy * np.sqrt(0.5), cy * np.sqrt(0.5))
            lift = 0.135 + 0.005 * (e % 3)
            st["dof_pos"][e, 0::3] = SIDE_HIP * s  # the lower legs swung towards the floor: knees and calves down
        elif group == 2:  # on the back: roll 180 degrees, the hips' capsules just above the floor
            q = (cy, sy, 0.0, 0.0)
            lift = 0.09 + 0.01 * (e % 4)
        else:             # under the lowest ceiling over the row of cells the env starts on, crouched
            j = int(np.clip(np.floor((root[e, 1] - org[1]) / hs), 0, tile.shape[2] - 1))
            i = int(tile[0, :, j].argmin())
            root[e, 0] = org[0] + (i + 0.5) * hs
            st["dof_pos"][e] = np.tile(CROUCH, 4) + rng.uniform(-0.1, 0.1, 12)
            q = (0.0, 0.0, sy, cy)
            lift = None
        f, cl = _heights(tile, hs, root[e, 0] - org[0], root[e, 1] - org[1])
        root[e, 2] = f + lift if lift is not None else cl - 0.05 - 0.01 * (e % 3)
        root[e, 3:7] = q
    actions = rng.normal(0.0, 1.0, (STEPS, N, 12)).astype(np.float32)
    scales = CF.reward_scale_vector(CF.derived(cfg)["reward_scales"])
    return cfg, c, td, ter, st, actions, scales


def class_counts(cf):
    """cf (STEPS, N, 17, 3) world forces -> {class: envs with a non-zero force on a body of it in some step}, and
    under "ceiling" the envs of the ceiling group whose trunk the first step pushes down by more than 100 N: it starts
    upright, more than 0.2 m above the floor, and the floor only pushes up (a self-contact reaction stays far below
    that force)"""
    hit = (np.abs(cf) > 0).any(axis=3).any(axis=0)  # (N, 17)
    out = {k: int(hit[:, b].any(axis=1).sum()) for k, b in CLASSES.items()}
    out["ceiling"] = int((cf[0, 24:32, 0, 2] < -100.0).sum())
    return out


def holds_every_class(counts):
    return all(counts[k] >= MIN_ENVS for k in CLASSES) and counts["ceiling"] >= MIN_CEILING


def replay():
    """{key: array} of the per-step outputs and, after the last step, the state planes and aux"""
    import torch
    from legged_tracking_amd import native
    cfg, c, td, _, st, actions, scales = setup()
    g = native.Go1Native(c, DEV)
    assert g.specialized
    g.set_terrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    g.state.load(st.arrays)
    grav, gvec = CF.gravity_state([0.0, 0.0, 0.0])
    aux = torch.zeros((N, abi.GO1_AUX), device=DEV)
    out = {}
    for t in range(STEPS):
        g.step(torch.from_numpy(actions[t]).to(DEV), gvec, grav, scales, rng_seed=31, rng_step=700 + t, aux=aux)
        torch.cuda.synchronize()
        for k, v in zip(PER_STEP, (g.obs, g.priv, g.rew, g.reset, g.time_out, g.contact_forces)):
            out[f"s{t}/{k}"] = v.cpu().numpy().copy()
    for k, v in g.state.numpy().items():
        out[f"state/{k}"] = np.ascontiguousarray(v)
    out["aux"] = aux.cpu().numpy()
    return out


def test_oracle_poses_load_every_contact_class():
    """the choice of poses, on the CPU: the f64 oracle's four steps from them load every class"""
    _, c, _, ter, st, actions, scales = setup()
    grav, gvec = CF.gravity_state([0.0, 0.0, 0.0])
    cf = np.stack([O.step(c, st, ter, actions[t], gvec, grav, scales, rng_seed=31, rng_step=700 + t,
                          debug=False)["contact_forces"] for t in range(STEPS)])
    counts = class_counts(cf)
    print(f"\noracle: {counts}")
    assert holds_every_class(counts), counts


@pytest.mark.gpu
def test_step_reproduces_the_recording_with_every_contact_class_bit_for_bit():
    ref = np.load(FIXTURE)
    counts = class_counts(np.stack([ref[f"s{t}/contact_forces"] for t in range(STEPS)]))
    print(f"\nrecording: {counts}")
    assert holds_every_class(counts), counts
    got = replay()
    keys = sorted(ref.files)
    assert keys == sorted(got)
    bad = []
    for k in keys:
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            bad.append((k, int((a != b).sum())))
    print(f"{len(keys)} arrays compared, {len(bad)} differ")
    assert not bad, bad
