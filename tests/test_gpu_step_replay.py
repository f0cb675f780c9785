"""Six control steps of the fused step kernel against a recording of the build before the step kernel's waits were
moved (tests/golden/step_replay/step_replay.npz, written by tests/golden/make_golden_step_replay.py on the GPU).

The changes that followed the recording move loads and keep values in registers: the loop-invariant config scalars
read once per launch, the capsule search's held parameter, the trunk faces' vertex addresses, the order of LDS reads.
None changes an operation or its order, so every output and every state plane is reproduced bit for bit:
  readme   the README configuration (decimation 4, n_internal 1): the specialised kernel;
  dec2x2   decimation 2, n_internal 2 on the generic kernel: other loop bounds, h = sim_dt / 2, and the values held
           over the control step carried across the inner integrator steps too.
32 envs on single_path from a seeded state, seeded N(0, 1) actions, and a few envs whose episode ends at the fourth
step, so that the held values and the terrain patch live through a reset inside the window.

(The fixture has a folder of its own: tests/test_gpu_parity.py and tests/test_oracle_golden.py replay every
tests/golden/step_*.npz as a reference fixture.)
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import abi, config as CF, native, terrain as T  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import golden_io as G  # noqa: E402

N = 32
STEPS = 6
VARIANTS = ("readme", "dec2x2")
TIMEOUT_ENVS = (1, 6, 18, 31)  # one per wave of two, alone and beside others; their episode ends at step 3
FIXTURE = os.path.join(G.GOLDEN, "step_replay", "step_replay.npz")
DEV = "cuda:0"
PER_STEP = ("obs", "privileged_obs", "rew", "reset", "time_outs")


def setup(variant):
    cfg = CF.readme_config(n_envs=N, terrain="single_path", rows=2, cols=4)
    physics = None
    if variant == "dec2x2":
        cfg.control.decimation = 2
        physics = {"n_internal": 2}
    c = CF.build_abi_config(cfg, physics=physics)
    td = T.build(cfg, N, np.random.RandomState(11))
    ter = O.NpTerrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    st = O.NpState(N, cfg=c)
    rng = np.random.default_rng(17)
    st["friction"][:, 0] = rng.uniform(0.1, 3.0, N)
    st["restitution"][:, 0] = rng.uniform(0.0, 0.4, N)
    st["payload"][:, 0] = rng.uniform(-1.0, 3.0, N)
    O.reset_envs(c, st, ter, np.ones(N, np.uint8), rng_seed=17, rng_step=0)
    st["episode_length"][:, 0] = rng.integers(0, 200, N)
    # time_out = episode_length + 1 > max_episode_length, first true at step 3 (the fourth)
    st["episode_length"][list(TIMEOUT_ENVS), 0] = int(np.floor(float(c.max_episode_length))) - 3
    actions = rng.normal(0.0, 1.0, (STEPS, N, 12)).astype(np.float32)
    scales = CF.reward_scale_vector(CF.derived(cfg)["reward_scales"])
    return cfg, c, td, st, actions, scales


def replay(variant):
    """{key: array} of the per-step outputs and, after the last step, the state planes, contact forces and aux."""
    cfg, c, td, st, actions, scales = setup(variant)
    g = native.Go1Native(c, DEV)
    if variant == "dec2x2":
        assert not g.specialized
    else:
        assert g.specialized
    g.set_terrain(td.tiles, td.env_tile, td.env_terrain_origin, td.env_origins)
    g.state.load(st.arrays)
    grav, gvec = CF.gravity_state([0.2, -0.1, 0.3])
    aux = torch.zeros((N, abi.GO1_AUX), device=DEV)
    out = {}
    for t in range(STEPS):
        g.step(torch.from_numpy(actions[t]).to(DEV), gvec, grav, scales, rng_seed=23, rng_step=500 + t, aux=aux)
        torch.cuda.synchronize()
        for k, v in zip(PER_STEP, (g.obs, g.priv, g.rew, g.reset, g.time_out)):
            out[f"{variant}/s{t}/{k}"] = v.cpu().numpy().copy()
    for k, v in g.state.numpy().items():
        out[f"{variant}/state/{k}"] = np.ascontiguousarray(v)
    out[f"{variant}/contact_forces"] = g.contact_forces.cpu().numpy()
    out[f"{variant}/aux"] = aux.cpu().numpy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_step_replays_recording_bit_for_bit(variant):
    ref = np.load(FIXTURE)
    got = replay(variant)
    keys = sorted(k for k in ref.files if k.startswith(variant + "/"))
    assert keys == sorted(got)
    # the window holds what it is meant to: the chosen envs time out at step 3 and nowhere before, contacts act
    to = np.stack([ref[f"{variant}/s{t}/time_outs"] for t in range(STEPS)]).astype(bool)
    assert to[3, list(TIMEOUT_ENVS)].all() and not to[:3].any()
    assert ref[f"{variant}/s3/reset"].astype(bool)[list(TIMEOUT_ENVS)].all()
    assert (np.abs(ref[f"{variant}/contact_forces"]).max(axis=(1, 2)) > 0).sum() >= N // 2
    bad = []
    for k in keys:
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.tobytes() != b.tobytes():
            bad.append((k, int((a != b).sum())))
    print(f"{variant}: {len(keys)} arrays compared, {len(bad)} differ")
    assert not bad, bad
