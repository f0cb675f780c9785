"""The streamed height scan (go1_step_kernel<INJ, 0, false>: any measured_points grid) on the GPU.

  * the two non-README fixtures recorded from the reference (tests/golden/make_golden_scan.py: 31 x 15 front
    half, 5 x 3 full scan with uneven spacing and points off the tile) replay in injected-state parity mode:
    height samples, masks and counters bit-equal, obs / rewards / torques within the project's bounds against the
    reference (tests/test_gpu_parity.py);
  * on the 21 x 11 grid the streamed kernel (Go1Native.scan_mode) is bit-identical to the register-resident
    kernels the oracle pins, front half and full scan;
  * the 31 x 15 grid through TrajectoryTrackingEnv + HistoryWrapper with the native integrator, and one learning
    iteration on it.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from legged_tracking_amd import abi, config as CF, native  # noqa: E402
from tests import golden_io as G  # noqa: E402

DEV = "cuda:0"
FINE_X, FINE_Y = np.linspace(-1, 1, 31), np.linspace(-0.5, 0.5, 15)


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def _replay(d, c, streamed=None):
    """Every step of fixture `d` from its recorded pre-state with the injected post-physics state; per step the
    outputs, the debug buffers and the state planes as numpy."""
    n = c.n_envs
    ter = G.terrain_of(d)
    g = native.Go1Native(c, DEV)
    if streamed is not None:
        g.scan_mode(streamed)
    g.set_terrain(ter.tiles, ter.env_tile, ter.eto, ter.eo)
    dbg = native.debug_buffers(n, c.decimation, DEV, grid=(c.scan_nx, c.scan_ny))
    steps = []
    for t in range(int(d["meta/n_steps"])):
        g.state.load(G.state_at(d, t, "pre", c).arrays)
        inp = G.step_inputs(d, t)
        inj = {k: _dev(v, torch.float32) for k, v in inp["inj"].items()}
        u = _dev(np.nan_to_num(inp["uniforms"], nan=0.5), torch.float32)
        g.step(_dev(inp["actions"]), inp["gravity_vec"], inp["sim_gravity"], inp["reward_scales"], uniforms=u,
               inj=inj, debug=dbg)
        torch.cuda.synchronize()
        out = {k: getattr(g, k).cpu().numpy() for k in native.OUT_KEYS}
        out.update({"dbg_" + k: v.cpu().numpy() for k, v in dbg.items()})
        out["state"] = g.state.numpy()
        steps.append(out)
    streamed_ran = g.streamed
    g.close()
    return steps, streamed_ran


@pytest.mark.parametrize("name", ["scan_fine.npz", "scan_tiny.npz"])
def test_streamed_step_replays_reference_fixture(name):
    d = G.load(name)
    _, c = G.fixture_config(d)
    steps, streamed = _replay(d, c)
    assert streamed  # go1_create selects the streamed kernel for any grid but 21 x 11
    assert any(d[f"s{t}/reset"].any() for t in range(len(steps)))  # the post-reset z of the height columns runs
    for t, o in enumerate(steps):
        np.testing.assert_array_equal(o["dbg_heights"], d[f"s{t}/measured_heights"])
        np.testing.assert_array_equal(o["reset"], d[f"s{t}/reset"])
        np.testing.assert_array_equal(o["time_out"], d[f"s{t}/time_out"])
        np.testing.assert_array_equal(o["dbg_reached"].astype(bool), d[f"s{t}/reached"])
        for k in ("episode_length", "curr_pose_index", "collision_count"):
            np.testing.assert_array_equal(o["state"][k].ravel(), d[f"s{t}/post/{k}"].ravel(), err_msg=k)
        assert o["obs"].shape == d[f"s{t}/obs"].shape == (c.n_envs, c.num_obs)
        err = np.abs(o["obs"] - d[f"s{t}/obs"])
        print(name, "step", t, "obs max abs error", err.max(), "height columns", err[:, 41:].max(),
              "rew", np.abs(o["rew"] - d[f"s{t}/rew"]).max(), "torques",
              np.abs(o["dbg_torques"] - d[f"s{t}/torques"]).max())
        np.testing.assert_allclose(o["obs"], d[f"s{t}/obs"], rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(o["rew"], d[f"s{t}/rew"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(o["dbg_torques"], d[f"s{t}/torques"], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("name", ["step_single_path.npz", "step_v_full_scan.npz"])
def test_streamed_kernel_is_bit_identical_on_the_readme_grid(name):
    """Front half (110 points, 7 per lane in registers) and full scan (231, 15 per lane) of the 21 x 11 grid:
    the streamed kernel forced on the same handle configuration computes the same bits."""
    d = G.load(name)
    _, c = G.fixture_config(d)
    assert (c.scan_nx, c.scan_ny) == (abi.GO1_GRID_X, abi.GO1_GRID_Y)
    built, s0 = _replay(d, c)
    forced, s1 = _replay(d, c, streamed=True)
    assert (s0, s1) == (False, True)
    assert len(built) == len(forced) == int(d["meta/n_steps"])
    for t, (a, b) in enumerate(zip(built, forced)):
        for k in ("obs", "rew", "reset", "dbg_heights"):
            assert a[k].tobytes() == b[k].tobytes(), (t, k)
        for k in G.STATE_KEYS:
            assert a["state"][k].tobytes() == b["state"][k].tobytes(), (t, k)
        assert np.abs(a["obs"][:, 41:]).max() > 0  # the scan is in the row


def test_scan_mode_selects_the_kernels():
    c = CF.build_abi_config(CF.readme_config(n_envs=16, terrain="single_path", rows=2, cols=2))
    g = native.Go1Native(c, DEV)
    assert g.specialized and not g.streamed
    g.scan_mode(True)
    assert g.streamed and not g.specialized
    with pytest.raises(native.NativeError, match="streamed"):
        g.specialize(True)
    g.scan_mode(False)
    assert g.specialized and not g.streamed
    with pytest.raises(native.NativeError, match="debug heights"):
        g.step(torch.zeros((16, 12), device=DEV), (0, 0, -1), (0, 0, -9.81), np.zeros(c.n_terms, np.float32),
               debug=dict(heights=torch.zeros((16, 2, 31, 15), device=DEV)))
    g.close()
    d = G.load("scan_tiny.npz")
    g = native.Go1Native(G.fixture_config(d)[1], DEV)
    assert g.streamed
    with pytest.raises(native.NativeError, match="21 x 11"):
        g.scan_mode(False)
    g.close()


def _fine_cfg(n, rows=2, cols=2):
    cfg = CF.readme_config(n_envs=n, terrain="single_path", rows=rows, cols=cols)
    cfg.terrain.measured_points_x, cfg.terrain.measured_points_y = FINE_X, FINE_Y
    cfg.env.num_observations = cfg.env.num_scalar_observations = 41 + 2 * 15 * 15
    return cfg


def test_fine_grid_learning_iteration(tmp_path):
    """One Runner.learn(1) at 64 envs on the 31 x 15 grid: finite losses (a 491-wide history row)."""
    from legged_tracking_amd import env as E, rollout as R
    torch.manual_seed(0)
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=DEV, cfg=_fine_cfg(64), seed=4))
    runner = R.Runner(env, device=DEV, save_dir=str(tmp_path))
    alg = runner.alg
    losses, update = [], alg.update

    def capture():
        losses.append(update())
        return losses[-1]

    alg.update = capture
    runner.learn(1)
    torch.cuda.synchronize()
    print("policy path:", "fused policy kernel" if alg.fused is not None else "torch", "losses", losses)
    assert len(losses) == 1 and np.isfinite(np.array([float(x) for x in losses[0]])).all(), losses
    assert alg.storage.observation_histories.shape[-1] == 491 * env.obs_history_length
    assert torch.isfinite(alg.storage.observation_histories).all()
    env.close()


def _env_steps(n, rows=2, cols=2):
    """31 x 15 front half through TrajectoryTrackingEnv + HistoryWrapper, native integrator, 3 steps: shapes,
    finiteness, and every height column within clip 0.3 x scale 0.1 (:404, :411)."""
    from legged_tracking_amd import env as E
    env = E.HistoryWrapper(E.TrajectoryTrackingEnv(sim_device=DEV, cfg=_fine_cfg(n, rows, cols), seed=4))
    assert env.num_obs == 491
    env.reset()
    for _ in range(3):
        ob, rew, done, _ = env.step(torch.zeros((n, 12), device=DEV))
        torch.cuda.synchronize()
        obs, hist = ob["obs"], ob["obs_history"]
        assert obs.shape == (n, 491) and hist.shape == (n, 491 * env.obs_history_length) and rew.shape == (n,)
        assert torch.isfinite(obs).all() and torch.isfinite(hist).all() and torch.isfinite(rew).all()
        assert float(obs[:, 41:].abs().max()) <= 0.03 + 1e-7
        assert float(obs[:, 41:].abs().max()) > 0
    env.close()


def test_fine_grid_through_the_env_full_wave():
    """16 envs: four full blocks of 4 envs."""
    _env_steps(16)


def test_fine_grid_through_the_env():
    """7 envs: not a multiple of the 4 envs per wave.  The streamed kernel's last wave is partial (its spare lanes
    mirror env 6); the 21 x 11 kernels keep go1_create's multiple of 16."""
    _env_steps(7, rows=1, cols=7)  # one env per sub-terrain (the env count is a multiple of the sub-terrains)
    c = CF.build_abi_config(CF.readme_config(n_envs=7, terrain="single_path", rows=2, cols=2))
    with pytest.raises(native.NativeError, match="multiple of 16"):
        native.Go1Native(c, DEV)


def test_partial_wave_matches_the_full_one():
    """The first 7 envs of a 16-env handle and a 7-env handle, same global env ids, same actions, 3 steps of the
    native integrator with Philox draws: bit-identical outputs and state (the mirror lanes change nothing, and
    the divergence counter and the compact episode log count every env once)."""
    from legged_tracking_amd import terrain as T
    outs = []
    for n in (16, 7):
        cfg = _fine_cfg(n)
        c = CF.build_abi_config(cfg)
        td = T.build(_fine_cfg(16), 16, np.random.RandomState(11))
        g = native.Go1Native(c, DEV)
        g.set_terrain(td.tiles, td.env_tile[:n], td.env_terrain_origin[:n], td.env_origins[:n])
        g.reset_envs(torch.ones(n, dtype=torch.bool, device=DEV), rng_seed=5, rng_step=0)
        g.state["episode_length"][:3] = 500  # time-outs: the reset path and the compact log run
        grav, gvec = CF.gravity_state([0.0, 0.0, 0.0])
        scales = CF.reward_scale_vector(CF.derived(cfg)["reward_scales"])
        gen = torch.Generator(device=DEV).manual_seed(0)
        w = abi.episode_log_width(c.n_terms)
        elog, count = torch.zeros((64, w + 2), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        args = g.prepare(None, episode_log=elog, log_count=count)
        for k in range(3):
            act = torch.randn((16, 12), device=DEV, generator=gen)[:n].contiguous()
            g.step_prepared(args, act, gvec, grav, scales, k, 5, 1 + k, log_tag=k)
        torch.cuda.synchronize()
        rows = elog[:int(count.item())].cpu().numpy()
        rows = rows[np.lexsort((rows[:, -1], rows[:, -2]))]
        outs.append(dict(obs=g.obs.cpu().numpy(), rew=g.rew.cpu().numpy(), reset=g.reset.cpu().numpy(),
                         state=g.state.numpy(), rows=rows))
        g.close()
    full, part = outs
    for k in ("obs", "rew", "reset"):
        assert full[k][:7].tobytes() == part[k].tobytes(), k
    for k in G.STATE_KEYS:
        assert full["state"][k][:7].tobytes() == part["state"][k].tobytes(), k
    sel = full["rows"][full["rows"][:, -1] < 7]
    assert len(part["rows"]) == len(sel) >= 3 and sel.tobytes() == part["rows"].tobytes()
