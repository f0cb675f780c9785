"""The privileged-observation assembler without a GPU: the numpy restatement (tests/priv_ref.py) against the reference's
own output (tests/golden/priv_cases.npz, written by tests/golden/make_golden_priv.py), the column table and the two
errors of the reference, the library's ABI and argument refusals, and what the library is built from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from legged_tracking_amd import build as B, config as CF, env as E, privileged as PV, velocity as VEL, \
    velocity_config as V
from tests import priv_ref as PR
from tests.cpu_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "go1_priv.h")
needs_lib = pytest.mark.skipif(not os.path.exists(PV.LIB_PATH), reason="libgo1_priv.so not built")
FULL = (("friction", 1), ("restitution", 1), ("base_mass", 1), ("com_displacement", 3), ("motor_strength", 12),
        ("motor_offset", 12), ("body_height", 1), ("body_velocity", 3), ("gravity", 3), ("clock_inputs", 4),
        ("desired_contact_states", 4))  # compute_observations' order (:482-587)


@pytest.fixture(scope="module")
def fixture():
    return PR.load()


@pytest.mark.parametrize("name", PR.SETS)
def test_restatement_matches_the_reference(fixture, name):
    d = fixture
    cfg = PR.cfg_of(d, name)
    cols = PV.columns(cfg)
    want = d[name + "/priv"]
    steps, n, w = want.shape
    assert (steps, n, w) == (10, 32, PR.WIDTHS[name]) == (10, 32, len(cols))
    PV.check(cfg)
    for s in range(steps):
        got = PR.assemble(cols, cfg.normalization.clip_observations, n, d["gravities"][s], **PR.planes_of(d, s))
        assert got.dtype == np.float32
        np.testing.assert_array_equal(PR.bits(got), PR.bits(want[s]), err_msg=f"{name} step {s}")
    clip = np.float32(d["clip_obs"])
    assert (np.abs(want) == clip).any() and (np.abs(want) < clip).any()


def test_fixture_holds_what_it_is_for(fixture):
    d = fixture
    # a gravity value whose division differs from the multiply by the reciprocal, in f32
    scale, shift = (np.float32(x) for x in PV.scale_shift([-0.7, 1.9]))
    assert list(d["norm"][list(d["norm_names"]).index("gravity_range")]) == [-0.7, 1.9]
    g = d["gravities"].astype(np.float32)
    assert ((g - shift) / scale != (g - shift) * (np.float32(1.0) / scale)).any()
    # envs that reset with a nonzero base_lin_vel, which the recorded vector shows unchanged (pre-reset)
    assert (d["base_lin_vel"][d["reset"]] != 0).any()
    cols = PV.columns(PR.cfg_of(d, "sparse"))
    k = [c[0] for c in cols].index(("body_velocity", 0))
    s, e = np.argwhere(d["reset"])[0]
    got = PR.assemble(cols, d["clip_obs"], 32, d["gravities"][s], **PR.planes_of(d, s))
    assert PR.bits(got)[e, k] == PR.bits(d["sparse/priv"][s])[e, k]
    # the scales are no powers of two
    for lo, hi in d["norm"]:
        assert np.log2(2.0 / (hi - lo)) % 1 != 0


def _cfg(**flags):
    cfg = CF.readme_config(n_envs=32, terrain="single_path", rows=4, cols=4)
    for k in [k for k in dir(cfg.env) if k.startswith("priv_observe_")]:
        setattr(cfg.env, k, False)
    for k, v in flags.items():
        setattr(cfg.env, "priv_observe_" + k, v)
    cfg.env.num_privileged_obs = len(PV.columns(cfg))
    return cfg


def test_columns_follow_the_reference_order():
    cfg = _cfg(**{k: True for k, _ in FULL})
    assert PV.names(cfg) == [(k, i) for k, n in FULL for i in range(n)] and len(PV.names(cfg)) == 45
    cols = PV.columns(cfg)
    by = {c[0]: c for c in cols}
    assert by[("gravity", 2)][1:3] == (PV.SRC_GRAVITY, 2) and by[("gravity", 2)][5] == PV.OP_DIV
    assert by[("body_height", 0)][1:3] == (PV.SRC_ROOT, 2) and by[("body_velocity", 1)][1:3] == (PV.SRC_AUX, 1)
    assert by[("base_mass", 0)][1] == PV.SRC_PAYLOADS and by[("com_displacement", 1)][1] == PV.SRC_ZERO
    assert by[("clock_inputs", 3)][5] == PV.OP_RAW and by[("motor_offset", 11)][1:3] == (PV.SRC_MOTOR_OFFSET, 11)
    assert sum(c[5] == PV.OP_DIV for c in cols) == 3
    # scale and shift: get_scale_shift in Python floats, rounded to f32 once -- the two existing columns' values
    a = CF.build_abi_config(_cfg(friction=True, restitution=True), n_envs=32)
    assert (by[("friction", 0)][3], by[("friction", 0)][4]) == (a.priv_friction_shift, a.priv_friction_scale)
    assert (by[("restitution", 0)][3], by[("restitution", 0)][4]) == (a.priv_rest_shift, a.priv_rest_scale)
    lo, hi = cfg.normalization.body_velocity_range
    assert by[("body_velocity", 0)][3:5] == (float(np.float32((hi + lo) / 2.0)), float(np.float32(2.0 / (hi - lo))))


def test_widths_of_the_four_sets_and_the_ignored_flags(fixture):
    for name in PR.SETS:
        cfg = PR.cfg_of(fixture, name)
        assert len(PV.columns(cfg)) == PR.WIDTHS[name]
        assert PV.wanted(cfg) == (name != "train")
    # the class defaults set friction_indep, joint_friction, Kp_factor and Kd_factor, which compute_observations never
    # reads: exactly six columns
    d = CF.Cfg.env
    assert d.priv_observe_friction_indep and d.priv_observe_joint_friction and d.priv_observe_Kp_factor and \
        d.priv_observe_Kd_factor and d.num_privileged_obs == 6
    cfg = _cfg()
    for k in [k for k in dir(d) if k.startswith("priv_observe_")]:
        setattr(cfg.env, k, getattr(d, k))
    assert [n[0] for n in PV.names(cfg)] == ["friction", "restitution", "base_mass"] + ["com_displacement"] * 3
    base = _cfg(friction=True, restitution=True)
    for k in ("friction_indep", "joint_friction", "Kp_factor", "Kd_factor", "contact_forces", "contact_states",
              "foot_height"):
        setattr(base.env, "priv_observe_" + k, True)
    assert len(PV.columns(base)) == 2 and not PV.wanted(base)
    PV.check(base)
    # one flag, or the two in another company, is a set of its own
    assert PV.wanted(_cfg(friction=True)) and PV.wanted(_cfg(friction=True, restitution=True, gravity=True))


def _build(cfg):
    made = []

    def backend(c):
        made.append(c)
        return OracleBackend(c)

    return E.LeggedRobot(cfg, seed=1, backend=backend), made


def test_the_references_two_errors_come_before_any_handle():
    cfg = _cfg(friction=True, restitution=True, base_mass=True)
    cfg.env.num_privileged_obs = 2
    made = []
    with pytest.raises(AssertionError, match=re.escape(
            "num_privileged_obs (2) != the number of privileged observations (3), you will discard data from the "
            "student!")):
        E.LeggedRobot(cfg, seed=1, backend=lambda c: made.append(c) or OracleBackend(c))
    cfg = _cfg(friction=True, restitution=True, ground_friction=True)
    with pytest.raises(AttributeError, match="'LeggedRobot' object has no attribute '_get_ground_frictions'"):
        E.LeggedRobot(cfg, seed=1, backend=lambda c: made.append(c) or OracleBackend(c))
    assert not made
    with pytest.raises(AssertionError, match="num_privileged_obs"):
        CF.build_abi_config(_with_width(_cfg(friction=True), 2), n_envs=32)


def _with_width(cfg, w):
    cfg.env.num_privileged_obs = w
    return cfg


def test_env_on_the_cpu_backend_builds_and_only_the_launch_raises():
    env, made = _build(_cfg(friction=True, restitution=True))
    assert len(made) == 1 and env.privileged is None and env._kout is env._out
    env.step(np.zeros((32, 12), np.float32))
    assert env.privileged_obs_buf.shape == (32, 2)
    wide, _ = _build(_cfg(friction=True, restitution=True, base_mass=True, body_velocity=True))
    p = wide.privileged
    assert p is not None and p.width == 6 and p.needs_aux and p.names[2] == ("base_mass", 0)
    assert wide._priv.shape == (E.OUT_RING, 32, 6) and all(o["priv"].shape == (32, 2) for o in wide._kout)
    assert wide._kout[0]["priv"] is wide._kout[3]["priv"] and wide._out[1]["priv"].shape == (32, 6)
    wide.set_output_demand(aux=False)
    assert wide._stores_aux()
    with pytest.raises(RuntimeError, match="aux"):
        wide.base_lin_vel
    with pytest.raises(PV.NativeError, match="no GPU|no CPU fallback"):
        wide.step(np.zeros((32, 12), np.float32))
    narrow, _ = _build(_cfg(friction=True, restitution=True, base_mass=True))
    narrow.set_output_demand(aux=False)
    assert not narrow.privileged.needs_aux and not narrow._stores_aux()


def test_priv_buffers_on_a_cpu_device():
    cfg = _cfg(**{k: True for k, _ in FULL})
    b = PV.PrivBuffers(4, "cpu", PV.columns(cfg), 100.0)
    assert b.width == 45 and b._cfg.n_envs == 4 and b._cfg.cols[44].op == PV.OP_RAW and b._table is None
    assert b.reads == set(PV.PLANES)
    with pytest.raises(PV.NativeError, match="no GPU|no CPU fallback"):
        b.launch(None, (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="columns"):
        PV.PrivBuffers(4, "cpu", [], 100.0)
    with pytest.raises(ValueError, match="columns"):
        PV.PrivBuffers(4, "cpu", PV.columns(cfg) * 2, 100.0)


def test_velocity_env_still_refuses_a_third_flag():
    cfg = V.train_velocity_config(n_envs=32)
    VEL.build_configs(cfg, n_envs=32)
    cfg.env.priv_observe_base_mass, cfg.env.num_privileged_obs = True, 3
    with pytest.raises(NotImplementedError, match="privileged observations"):
        VEL.build_configs(cfg, n_envs=32)


def _struct_fields(txt, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.sub(r"\[.*?\]|\W", "", first.split()[-1])] + [re.sub(r"\[.*?\]|\W", "", r) for r in rest]
    return names


def test_header_constants_and_fields_match_the_binding_and_the_restatement():
    txt = open(HEADER).read()
    d = {k: int(v) for k, v in re.findall(r"#define (GO1_PRIV_\w+) (\d+)", txt)}
    assert d["GO1_PRIV_ABI_VERSION"] == PV.GO1_PRIV_ABI_VERSION and d["GO1_PRIV_MAX_COLS"] == PV.MAX_COLS == 48
    srcs = ("ZERO", "FRICTION", "RESTITUTION", "PAYLOADS", "MOTOR_STRENGTH", "MOTOR_OFFSET", "ROOT", "AUX", "GRAVITY")
    assert [d["GO1_PRIV_SRC_" + s] for s in srcs] == [getattr(PV, "SRC_" + s) for s in srcs] == list(range(9))
    assert d["GO1_PRIV_NUM_SRC"] == 9
    assert tuple(s.lower() for s in srcs[1:8]) == PV.PLANES == PR.PLANES
    assert (PR.SRC_ZERO, PR.SRC_GRAVITY) == (PV.SRC_ZERO, PV.SRC_GRAVITY)
    assert [d["GO1_PRIV_OP_" + s] for s in ("MUL", "DIV", "RAW")] == [PV.OP_MUL, PV.OP_DIV, PV.OP_RAW] == \
        [PR.OP_MUL, PR.OP_DIV, PR.OP_RAW]
    for struct, mirror in (("go1_priv_col", PV.Go1PrivCol), ("go1_priv_config", PV.Go1PrivConfig),
                           ("go1_priv_args", PV.Go1PrivArgs)):
        assert _struct_fields(txt, struct) == [f for f, _ in mirror._fields_], struct


@needs_lib
def test_library_exports_and_struct_sizes():
    lib = PV.lib()  # loads without a GPU
    names = sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(go1_\w+)\s*\(", open(HEADER).read(), re.M)))
    assert names == ["go1_priv_abi_sizes", "go1_priv_abi_version", "go1_priv_last_error", "go1_priv_step"]
    assert lib.go1_priv_abi_version() == PV.GO1_PRIV_ABI_VERSION
    out = (C.c_int64 * 4)()
    lib.go1_priv_abi_sizes(out)
    assert list(out) == PV.abi_sizes() == [20, 16 + 48 * 20, C.sizeof(PV.Go1PrivArgs), 48]
    nm = subprocess.run(["nm", "-D", "--defined-only", PV.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "go1_" in l)
    assert exported == names


@needs_lib
def test_argument_errors_are_reported_not_thrown():
    lib = PV.lib()
    cfg = _cfg(friction=True, motor_offset=True, gravity=True)
    b = PV.PrivBuffers(0, "cpu", PV.columns(cfg), 5.0)
    c, a = b._cfg, PV.Go1PrivArgs()

    def call():
        return lib.go1_priv_step(C.byref(c), C.byref(a), None)

    assert lib.go1_priv_step(None, None, None) == -1 and b"null" in lib.last_error()
    # a null plane that a column reads: -1 with its name, before anything else about the arguments
    assert call() == -1 and b"friction" in lib.last_error() and b"NULL" in lib.last_error()
    a.friction, a.friction_stride = 16, 1  # never dereferenced: n_envs is 0
    assert call() == -1 and b"motor_offset" in lib.last_error()
    a.motor_offset, a.motor_offset_stride = 16, 8
    assert call() == -1 and b"component 8" in lib.last_error()  # a row of 8 has no columns 8 .. 11
    a.motor_offset_stride = 12
    assert call() == -1 and b"table and out" in lib.last_error()
    a.table = a.out = 16
    # restitution, payloads, motor_strength, root and aux stay null: no column reads them
    assert call() == 0
    c.n_envs = -1
    assert call() == -1 and b"n_envs" in lib.last_error()
    c.n_envs, c.width = 0, 49
    assert call() == -1 and b"width" in lib.last_error()
    c.width, c.n_envs = 14, 1 << 28
    assert call() == -1 and b"2^31" in lib.last_error()
    c.n_envs, c.clip_obs = 0, -1.0
    assert call() == -1 and b"clip_obs" in lib.last_error()
    c.clip_obs = 5.0
    c.cols[3].src = 9
    assert call() == -1 and b"column 3: unknown source" in lib.last_error()
    c.cols[3].src, c.cols[3].op = PV.SRC_MOTOR_OFFSET, 3
    assert call() == -1 and b"unknown operation" in lib.last_error()
    c.cols[3].op = PV.OP_MUL
    c.cols[13].scale = 0.0  # a gravity column: a division
    assert call() == -1 and b"zero scale" in lib.last_error()


def test_the_library_is_made_of_its_own_two_files_only():
    srcs, flags = B.LIBS["libgo1_priv.so"]
    assert srcs == ["go1_priv.hip"] and flags == B.STEP_FLAGS and "-ffp-contract=off" in B.FLAGS
    mine = {os.path.basename(x) for x in B.lib_files("libgo1_priv.so")}
    assert mine == {"go1_priv.hip", "go1_priv.h"}
    assert not any(f == "go1_host.h" or f.startswith(("go1_dr.", "go1_plan.")) for f in mine)
    for name in B.LIBS:  # disjoint from every other library, the ray caster's and the tracer's among them
        if name != "libgo1_priv.so":
            assert not mine & {os.path.basename(x) for x in B.lib_files(name)}, name
    # the step library's row is what it was
    assert B.LIBS["libgo1_mi355x.so"] == (["go1_step.hip", "go1_terrain.hip"], B.STEP_FLAGS)
