"""The after-start domain randomiser without a GPU: the numpy restatement (tests/dr_ref.py) against the reference's own
output (tests/golden/dr_cases.npz, written by tests/golden/make_golden_dr.py), the Cfg guards of both envs, play's
DR_OFF, and the library's ABI and argument refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from legged_tracking_amd import build as B, config as CF, play as PL, randomize as RZ, velocity as VEL, \
    velocity_config as V
from tests import dr_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "go1_dr.h")
needs_lib = pytest.mark.skipif(not os.path.exists(RZ.LIB_PATH), reason="libgo1_dr.so not built")
FLAG_NAMES, ref_of = DR.FLAG_NAMES, DR.ref_of


@pytest.mark.parametrize("name", ["all", "partial"])
def test_restatement_matches_the_reference(name):
    d = DR.load_set(name)
    steps, n = d["reset"].shape
    assert (steps, n) == (12, 32) and int(d["rand_interval"]) == 4 and int(d["push_interval"]) == 3
    ref, flags, _, priv = ref_of(d)
    # the restatement's priv constants are the reference's get_scale_shift values (shift, scale), rounded to f32
    np.testing.assert_array_equal(np.array(priv[:4]), d["priv_consts"].astype(np.float32))
    for s in range(steps):
        ref.load(d["root_before"][s], d["friction_before"][s], d["restitution_before"][s], d["payloads_before"][s])
        pv = d["priv_before"][s].copy()
        rig, push = ref.step(d["reset"][s], d["episode_length"][s], d["uniforms"][s], pv)
        np.testing.assert_array_equal(rig, d["rigids"][s])
        np.testing.assert_array_equal(push, d["pushed"][s])
        for k, got in (("root", ref.root), ("friction", ref.friction), ("restitution", ref.restitution),
                       ("payloads", ref.payloads), ("priv", pv)):
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got.view(np.uint32), d[k + "_after"][s].view(np.uint32), err_msg=f"{k} {s}")
        # only the velocity columns of the root change, and the plane the integrator reads never does
        other = [c for c in range(13) if c not in (7, 8)]
        np.testing.assert_array_equal(d["root_after"][s][:, other], d["root_before"][s][:, other])
        np.testing.assert_array_equal(d["payload_plane"][s], d["payload_plane"][0])
        if s + 1 < steps:  # the fixture's steps are consecutive
            for k in ("friction", "restitution", "payloads"):
                np.testing.assert_array_equal(d[k + "_after"][s], d[k + "_before"][s + 1])
    # every branch is in the fixture: due by interval, by reset, by both; pushed; pushed and reset
    assert d["twice"].any() and (d["rigids"] & ~d["reset"]).any() and (d["reset"] & ~d["twice"]).any()
    assert (np.abs(d["priv_after"]) == d["clip_obs"]).any() and (np.abs(d["priv_after"]) < d["clip_obs"]).any()
    if flags["push_robots"]:
        assert d["pushed"].any() and (d["reset"] & (d["uniforms"][..., DR.U_PUSH_X] != 0)).any()
        assert (d["root_after"][..., 7:9] != d["root_before"][..., 7:9]).any()
    else:
        np.testing.assert_array_equal(d["root_after"], d["root_before"])
    if not flags["friction"]:
        np.testing.assert_array_equal(d["friction_after"], d["friction_before"])
        assert (d["payloads_after"] != d["payloads_before"]).any()


@pytest.mark.parametrize("name", ["all", "partial"])
def test_restatement_matches_the_reference_on_a_host_reset(name):
    d = DR.load_set(name)
    ref, _, _, _ = ref_of(d)
    ref.load(np.zeros((32, 13)), d["host_friction_before"], d["host_restitution_before"], d["host_payloads_before"])
    ref.reset(d["host_ids"], d["host_uniforms"])
    for k, got in (("friction", ref.friction), ("restitution", ref.restitution), ("payloads", ref.payloads)):
        np.testing.assert_array_equal(got.view(np.uint32), d[f"host_{k}_after"].view(np.uint32))
    assert (d["host_payloads_after"] != d["host_payloads_before"]).sum() == len(d["host_ids"])


def test_philox_restatement_known_answer():
    """Philox4x32-10 known-answer vectors (Random123's kat_vectors): the restatement is the generator the header
    names, so the GPU tests' `dbg_uniforms` comparison pins the kernel's counter layout to it."""
    assert DR.philox4x32([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert DR.philox4x32([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert DR.philox4x32([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    u = DR.philox_uniforms(11, (1 << 62) + 5, 3, 1)
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))


def test_header_constants_match_the_binding_and_the_restatement():
    txt = open(HEADER).read()
    d = {k: int(v, 0) for k, v in re.findall(r"#define (GO1_DR_\w+) (0x[0-9A-Fa-f]+|\d+)", txt)}
    assert d["GO1_DR_ABI_VERSION"] == RZ.GO1_DR_ABI_VERSION
    assert d["GO1_DR_U"] == RZ.DR_U == DR.DR_U and d["GO1_DR_TAG"] == RZ.DR_TAG == DR.DR_TAG
    slots = (d["GO1_DR_U_PAYLOAD"], d["GO1_DR_U_FRICTION"], d["GO1_DR_U_RESTITUTION"], d["GO1_DR_U_PUSH_X"],
             d["GO1_DR_U_PUSH_Y"])
    assert slots == (RZ.U_PAYLOAD, RZ.U_FRICTION, RZ.U_RESTITUTION, RZ.U_PUSH_X, RZ.U_PUSH_Y) == \
        (DR.U_PAYLOAD, DR.U_FRICTION, DR.U_RESTITUTION, DR.U_PUSH_X, DR.U_PUSH_Y)
    # the rigid props share one Philox block, the push another; the tag clears every block index of the step kernels
    assert {s // 4 for s in slots[:3]} == {0} and {s // 4 for s in slots[3:]} == {1} and RZ.DR_TAG >= 1 << 16
    # every struct field of the header, in order, is a field of its mirror
    for struct, mirror in (("go1_dr_config", RZ.Go1DrConfig), ("go1_dr_state", RZ.Go1DrState),
                           ("go1_dr_args", RZ.Go1DrArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                names += [re.sub(r"\W", "", first.split()[-1])] + [re.sub(r"\W", "", r) for r in rest]
        assert names == [f for f, _ in mirror._fields_], struct


@needs_lib
def test_library_exports_and_struct_sizes():
    lib = RZ.lib()  # loads without a GPU
    names = sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(go1_\w+)\s*\(", open(HEADER).read(), re.M)))
    assert names == ["go1_dr_abi_sizes", "go1_dr_abi_version", "go1_dr_last_error", "go1_dr_reset", "go1_dr_step"]
    for n in names:
        assert hasattr(lib, n), n
    assert lib.go1_dr_abi_version() == RZ.GO1_DR_ABI_VERSION
    out = (C.c_int64 * 4)()
    lib.go1_dr_abi_sizes(out)
    assert list(out) == RZ.abi_sizes()
    # exactly the declared symbols are exported
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", RZ.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "go1_" in l)
    assert exported == names


@needs_lib
def test_argument_errors_are_reported_not_thrown():
    lib = RZ.lib()
    c, s, a = RZ.Go1DrConfig(), RZ.Go1DrState(), RZ.Go1DrArgs()

    def call():
        return lib.go1_dr_step(C.byref(c), C.byref(s), C.byref(a), None)

    assert lib.go1_dr_step(None, None, None, None) == -1 and b"null" in lib.last_error()
    assert call() == -1 and b"n_envs" in lib.last_error()
    c.n_envs = 4
    assert call() == -1 and b"rand_interval" in lib.last_error()
    c.rand_interval = 4
    assert call() == -1 and b"push_interval" in lib.last_error()
    c.push_interval = 3
    c.friction_range = -1.0
    assert call() == -1 and b"range" in lib.last_error()
    c.friction_range = 1.0
    assert call() == -1 and b"state" in lib.last_error()
    s.root = s.friction = s.restitution = 16  # never dereferenced: refused first
    assert call() == -1 and b"args" in lib.last_error()
    a.reset = a.episode_length = 16
    a.priv, a.priv_stride = 16, 1
    assert call() == -1 and b"priv_stride" in lib.last_error()
    a.priv_stride = 2
    assert call() == 0  # both flags off: accepted, nothing launched
    assert lib.go1_dr_reset(C.byref(c), C.byref(s), None, -1, 0, None, None) == -1 and b"n_ids" in lib.last_error()
    assert lib.go1_dr_reset(C.byref(c), C.byref(s), None, 2, 0, None, None) == -1 and b"ids" in lib.last_error()
    assert lib.go1_dr_reset(C.byref(c), C.byref(s), None, 0, 0, None, None) == 0


def _traj_cfg():
    return CF.readme_config(n_envs=32, terrain="single_path", rows=4, cols=4)


def test_trajectory_config_guard():
    for flag in ("push_robots", "randomize_rigids_after_start"):
        cfg = _traj_cfg()
        setattr(cfg.domain_rand, flag, True)
        with pytest.raises(NotImplementedError, match=flag):  # the step alone does neither
            CF.build_abi_config(cfg, n_envs=32)
        a = CF.build_abi_config(cfg, n_envs=32, randomizer=True)
        setattr(cfg.domain_rand, flag, False)
        assert bytes(a) == bytes(CF.build_abi_config(cfg, n_envs=32))  # the step's config does not change
    cfg = _traj_cfg()
    cfg.domain_rand.randomize_com_displacement = True  # on its own it stays refused, randomiser or not
    with pytest.raises(NotImplementedError, match="randomize_com_displacement"):
        CF.build_abi_config(cfg, n_envs=32, randomizer=True)
    cfg = _traj_cfg()
    cfg.domain_rand.push_robots, cfg.domain_rand.push_interval_s = True, 0.0
    with pytest.raises(ValueError, match="push_interval"):
        CF.build_abi_config(cfg, n_envs=32, randomizer=True)


def test_velocity_config_guard():
    for flag in ("push_robots", "randomize_rigids_after_start"):
        cfg = V.train_velocity_config(n_envs=32)
        setattr(cfg.domain_rand, flag, True)
        with pytest.raises(NotImplementedError, match=flag):
            VEL.build_configs(cfg, n_envs=32)
        c, v = VEL.build_configs(cfg, n_envs=32, randomizer=True)[:2]
        setattr(cfg.domain_rand, flag, False)
        c0, v0 = VEL.build_configs(cfg, n_envs=32)[:2]
        assert bytes(c) == bytes(c0) and bytes(v) == bytes(v0)
    cfg = V.train_velocity_config(n_envs=32)
    cfg.domain_rand.randomize_rigids_after_start, cfg.domain_rand.rand_interval_s = True, -1.0
    with pytest.raises(ValueError, match="rand_interval"):
        VEL.build_configs(cfg, n_envs=32, randomizer=True)


def test_check_randomizer_refusals():
    def cfg_with(**kw):
        cfg = _traj_cfg()
        cfg.domain_rand.push_robots = cfg.domain_rand.randomize_rigids_after_start = True
        for k, v in kw.items():
            setattr(cfg.domain_rand, k, v)
        return cfg

    RZ.check_randomizer(cfg_with())
    assert RZ.wanted(cfg_with()) and not RZ.wanted(_traj_cfg())
    with pytest.raises(ValueError, match="rand_interval of 0 steps"):
        RZ.check_randomizer(cfg_with(rand_interval_s=0.0))
    with pytest.raises(ValueError, match="push_interval of 0 steps"):
        RZ.check_randomizer(cfg_with(push_interval_s=0.0))
    for name, flag in (("added_mass_range", "randomize_base_mass"), ("friction_range", "randomize_friction"),
                       ("restitution_range", "randomize_restitution")):
        with pytest.raises(ValueError, match=name + ".*hi < lo"):
            RZ.check_randomizer(cfg_with(**{name: [1.0, 0.5], flag: True}))
        RZ.check_randomizer(cfg_with(**{name: [1.0, 0.5], flag: False}))  # a range nothing draws from
    with pytest.raises(ValueError, match="max_push_vel_xy"):
        RZ.check_randomizer(cfg_with(max_push_vel_xy=-0.1))
    with pytest.raises(NotImplementedError, match="randomize_com_displacement with randomize_rigids_after_start"):
        RZ.check_randomizer(cfg_with(randomize_com_displacement=True))
    # the intervals are the reference's ceil(seconds / dt)
    cfg = cfg_with(rand_interval_s=0.15, push_interval_s=0.05)
    dt = cfg.control.decimation * cfg.sim.dt
    assert RZ.intervals(cfg) == (int(np.ceil(0.15 / dt)), int(np.ceil(0.05 / dt)))


def test_binding_refuses_before_any_device_work():
    ranges = dict(payload=(-1.0, 3.0), friction=(0.1, 3.0), restitution=(0.0, 0.4), push=0.5)
    flags = dict.fromkeys(FLAG_NAMES, True)
    priv = DR.priv_consts((0.0, 1.0), (0.0, 1.0), 100.0)
    with pytest.raises(ValueError, match="push_interval"):
        RZ.DrBuffers(4, "cpu", ranges, flags, 4, 0, priv)
    with pytest.raises(ValueError, match="friction range"):
        RZ.DrBuffers(4, "cpu", dict(ranges, friction=(3.0, 0.1)), flags, 4, 3, priv)
    b = RZ.DrBuffers(4, "cpu", ranges, flags, 4, 3, priv, env_id_offset=8, seed=5, payloads=[1.0, 2.0, 3.0, 4.0])
    assert b.payloads.shape == (4, 1) and b.payloads[:, 0].tolist() == [1.0, 2.0, 3.0, 4.0]
    c = b._cfg
    assert (c.n_envs, c.env_id_offset, c.rand_interval, c.push_interval, c.rng_seed) == (4, 8, 4, 3, 5)
    assert np.float32(c.friction_range) == np.float32(3.0 - 0.1) and np.float32(c.push_range) == np.float32(1.0)
    assert np.float32(c.push_lo) == np.float32(-0.5)
    with pytest.raises(RZ.NativeError, match="no GPU|no CPU fallback"):
        b.launch(*([None] * 6))


def test_play_switches_the_randomiser_off(tmp_path):
    assert {"push_robots", "randomize_rigids_after_start"} <= set(PL.DR_OFF)
    import pickle
    with open(tmp_path / "parameters.pkl", "wb") as f:  # a run trained with both on
        pickle.dump({"domain_rand": {"push_robots": True, "randomize_rigids_after_start": True}}, f)
    assert RZ.wanted(PL.checkpoint_cfg(str(tmp_path), 16, 4, 4, dr_off=False))
    assert not RZ.wanted(PL.checkpoint_cfg(str(tmp_path), 16, 4, 4))
    assert not RZ.wanted(PL.load_cfg(str(tmp_path), 16, 64, 48))


def test_dr_library_is_built_with_the_planners_flags():
    srcs, flags = B.LIBS["libgo1_dr.so"]
    assert srcs == ["go1_dr.hip"] and flags == B.LIBS["libgo1_plan.so"][1] and "-ffp-contract=off" in B.FLAGS
    files = {os.path.basename(x) for x in B.lib_files("libgo1_dr.so")}
    assert {"go1_dr.hip", "go1_dr.h", "go1_lanes.h", "go1_torch_math.h"} <= files
    for name in B.LIBS:  # its own source and header belong to no other library
        if name != "libgo1_dr.so":
            assert not {"go1_dr.hip", "go1_dr.h"} & {os.path.basename(x) for x in B.lib_files(name)}
