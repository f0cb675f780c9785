"""The height scan takes any Cfg.terrain.measured_points_x / _y grid (host side, no GPU): the observation
layout and the C ABI's scan fields follow the Cfg's counts, what the step does not take raises before a
handle is built with the cause named, the two non-README fixtures build a config, and the streamed step
kernel (go1_step_kernel<INJ, 0, false>) neither spills nor loses an address space."""
import ctypes as C
import os

import numpy as np
import pytest

from legged_tracking_amd import abi, config as CF
from tests import golden_io as G
from tests import test_kernel_isa as ISA


def _cfg(x=None, y=None, front_half=True, num_obs=None, n=32, **over):
    cfg = CF.readme_config(n_envs=n, terrain="single_path", rows=4, cols=4)
    if x is not None:
        cfg.terrain.measured_points_x = x
    if y is not None:
        cfg.terrain.measured_points_y = y
    cfg.terrain.measure_front_half = front_half
    if num_obs is not None:
        cfg.env.num_observations = num_obs
    for path, v in over.items():
        obj = cfg
        parts = path.split(".")
        for p in parts[:-1]:
            obj = getattr(obj, p)
        setattr(obj, parts[-1], v)
    return cfg


def _abi(*a, **k):
    cfg = _cfg(*a, **k)
    return CF.build_abi_config(cfg, n_envs=int(cfg.env.num_envs))


def test_fine_front_half_grid_layout():
    x, y = np.linspace(-1, 1, 31), np.linspace(-0.5, 0.5, 15)
    c = _abi(x, y, True, 491)
    assert (c.num_obs, c.u_per_env, c.scan_nx, c.scan_ny) == (491, 47 + 491, 31, 15)
    np.testing.assert_array_equal(np.array(c.scan_x[:31], np.float32), x.astype(np.float32))
    np.testing.assert_array_equal(np.array(c.scan_y[:15], np.float32), y.astype(np.float32))
    ol = CF.obs_layout(_cfg(x, y, True, 491))
    assert (ol["n_points"], ol["height_offset"], ol["width"]) == (15 * 15, 41, 491)


def test_tiny_full_grid_layout():
    c = _abi([-0.3, 0.0, 0.25, 0.6, 2.5], [-1.5, 0.0, 0.2], False, 71)
    assert (c.num_obs, c.u_per_env, c.scan_nx, c.scan_ny) == (71, 47 + 71, 5, 3)
    assert c.scan_x[4] == 2.5 and c.scan_y[0] == -1.5


def test_largest_grid_is_the_cnn_encoder_map():
    """61 x 31 (the reference's ppo_cse_cnn map) is inside the caps."""
    c = _abi(np.linspace(-1, 2, 61), np.linspace(-0.75, 0.75, 31), False, 41 + 2 * 61 * 31)
    assert (c.scan_nx, c.scan_ny, c.num_obs) == (61, 31, 3823)
    c = _abi(np.linspace(-1, 2, 64), np.linspace(-0.75, 0.75, 32), False, 41 + 2 * 64 * 32)
    assert (c.scan_nx, c.scan_ny) == (abi.GO1_MAX_SCAN_X, abi.GO1_MAX_SCAN_Y)


def test_readme_config_is_unchanged():
    c = _abi()
    assert (c.num_obs, c.u_per_env, c.scan_nx, c.scan_ny) == (261, 308, 21, 11)
    assert list(c.scan_x[:21]) == list(c.height_grid_x) and list(c.scan_y[:11]) == list(c.height_grid_y)
    np.testing.assert_array_equal(np.array(c.height_grid_x[:], np.float32), np.linspace(-1, 1, 21).astype(np.float32))
    c = _abi(front_half=False, num_obs=503)
    assert (c.num_obs, c.u_per_env) == (503, 47 + 503)


@pytest.mark.parametrize("kw, exc, text", [
    (dict(x=np.linspace(-1, 1, 65), front_half=False, num_obs=41 + 2 * 65 * 11), NotImplementedError,
     "measured_points_x"),
    (dict(y=np.linspace(-1, 1, 33), num_obs=41 + 2 * 10 * 33), NotImplementedError, "measured_points_y"),
    (dict(x=[], num_obs=41), ValueError, "measured_points_x is empty"),
    (dict(y=[], num_obs=41), ValueError, "measured_points_y is empty"),
    # the reference fails here itself: its noise vector covers nx // 2 rows (:1123-1125), the observation
    # nx - (nx // 2 + 1) (:395-399)
    (dict(x=np.linspace(-1, 1, 12), y=np.linspace(-0.5, 0.5, 7), num_obs=41 + 2 * 5 * 7), RuntimeError,
     "even count.*measure_front_half.*add_noise"),
    (dict(x=[0.0, 0.5], num_obs=41), ValueError, "measure_front_half keeps"),
    (dict(x=[0.0], num_obs=41), ValueError, "measure_front_half keeps"),
    # a grid whose width differs from num_observations: the message names the grid
    (dict(x=np.linspace(-1, 1, 31), y=np.linspace(-0.5, 0.5, 15)), AssertionError,
     "num_observations 261.*31 x 15 measured_points"),
])
def test_unsupported_grids_raise_with_the_cause(kw, exc, text):
    with pytest.raises(exc, match=text):
        _abi(**kw)


def test_even_count_is_fine_without_noise_or_with_the_full_scan():
    x, y = np.linspace(-1, 1, 12), np.linspace(-0.5, 0.5, 7)
    assert _abi(x, y, True, 41 + 2 * 5 * 7, **{"noise.add_noise": False}).num_obs == 111
    assert _abi(x, y, False, 41 + 2 * 12 * 7).num_obs == 209
    assert _abi([0.0, 0.5], front_half=False, num_obs=41 + 2 * 2 * 11).scan_nx == 2


@pytest.mark.parametrize("name, shape", [("scan_fine.npz", (31, 15, 491)), ("scan_tiny.npz", (5, 3, 71))])
def test_fixture_config_builds_for_the_scan_fixtures(name, shape):
    d = G.load(name)
    cfg, c = G.fixture_config(d)
    assert (c.scan_nx, c.scan_ny, c.num_obs) == shape
    n = c.n_envs
    assert d["s0/obs"].shape == (n, c.num_obs) and d["s0/measured_heights"].shape == (n, 2, c.scan_nx, c.scan_ny)
    assert d["s0/uniforms"].shape == (n, c.u_per_env)
    assert not G.spec_match(c)


def test_library_checks_the_scan_fields():
    """go1_create repeats the guards for a foreign binding (no device work before them)."""
    from legged_tracking_amd import native
    lib = native.lib()
    h = C.c_void_p()
    for edit, text in ((lambda c: setattr(c, "scan_nx", 65), b"scan_nx"), (lambda c: setattr(c, "scan_ny", 0), b"scan_nx"),
                       (lambda c: c.scan_x.__setitem__(3, 0.123), b"height_grid_x"),
                       (lambda c: setattr(c, "scan_nx", 23), b"num_obs")):
        c = _abi(n=16)
        edit(c)
        assert lib.go1_create(C.byref(c), C.byref(h)) == -1
        assert text in lib.go1_last_error(), lib.go1_last_error()
    assert lib.go1_scan_mode(None, 1) == -1 and lib.go1_is_streamed(None) == 0
    # the env count: a multiple of 16 for the 21 x 11 kernels (no partial wave), any for the streamed one
    c = _abi(n=7)
    assert lib.go1_create(C.byref(c), C.byref(h)) == -1 and b"multiple of 16" in lib.go1_last_error()


@pytest.mark.skipif(not os.path.exists(os.path.join(ISA.LLVM, "llvm-objdump")), reason="ROCm LLVM tools not available")
@pytest.mark.parametrize("kernel", ["_Z15go1_step_kernelILb0ELi0ELb0EEvPK10go1_config",
                                    "_Z15go1_step_kernelILb1ELi0ELb0EEvPK10go1_config"])
def test_streamed_kernel_has_no_flat_or_scratch_access(kernel):
    """The streamed instantiations (native integrator / injected state), as tests/test_kernel_isa.py checks
    the specialised one: no register spill, and the scan coordinates read from the config stay global loads."""
    path = os.path.join(ISA.BUILD, "libgo1_mi355x.so")
    if not os.path.exists(path):
        pytest.skip("libgo1_mi355x.so not built (python -c 'import __graft_entry__ as g; g.build()')")
    ins = ISA._kernel_body(ISA._disasm(path), kernel)
    assert len(ins) > 1000, f"kernel {kernel} not found"
    flat = [i for i in ins if i.startswith("flat_")]
    scratch = [i for i in ins if i.startswith("scratch_")]
    assert not flat, f"{len(flat)} flat memory instructions (an LDS or global access lost its address space)"
    assert not scratch, f"{len(scratch)} scratch instructions (register spills)"
    assert sum(i.startswith("v_mfma") for i in ins) >= 60
