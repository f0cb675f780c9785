"""The local target planner without a GPU: the numpy restatement (tests/plan_ref.py) against the reference's own
output (tests/golden/plan_cases.npz, written by tests/golden/make_golden_plan.py), the host tables, the Cfg guard,
and the library's ABI and argument refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from legged_tracking_amd import build as B, config as CF, plan as P
from tests import plan_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "go1_plan.h")
TOL = dict(rtol=2e-5, atol=2e-5)  # the project's reference tolerance (tests/test_gpu_parity.py)
load_set, angle_close = PR.load_set, PR.angle_close
needs_lib = pytest.mark.skipif(not os.path.exists(P.LIB_PATH), reason="libgo1_plan.so not built")


def ref_of(d, n=None, **kw):
    n = d["root"].shape[1] if n is None else n
    return PR.PlanRef(n, d["cand"], d["grid_x"], d["grid_y"], int(d["traj_length"]), int(d["plan_interval"]),
                      float(d["switch_dist"]), float(d["switch_yaw"]), **kw)


@pytest.mark.parametrize("name", ["default", "small"])
def test_restatement_matches_the_reference(name):
    d = load_set(name)
    steps, n = d["root"].shape[:2]
    assert (steps, n) == (8, 32) and d["redraws"][0] <= 0.02 * d["redraws"][1]
    ref = ref_of(d)
    seen = set()
    for s in range(steps):
        ref.step(d["root"][s], d["trajectory"][s], d["curr_pose_index"][s], d["episode_length"][s], d["reset"][s],
                 d["heights"][s])
        live = ~d["reset"][s]
        np.testing.assert_array_equal(ref.chosen, d["chosen"][s])
        np.testing.assert_array_equal(ref.plan_buf, d["plan_buf"][s])
        np.testing.assert_array_equal(ref.replan, d["replan"][s])
        np.testing.assert_array_equal(ref.plan_length, d["plan_length"][s])  # reset envs too
        np.testing.assert_allclose(ref.local_target[live][:, :3], d["local_target"][s][live][:, :3], **TOL)
        assert angle_close(ref.local_target[live][:, 3:], d["local_target"][s][live][:, 3:])
        np.testing.assert_allclose(ref.local_rel_lin, d["local_rel_lin"][s], **TOL)
        assert angle_close(ref.local_rel_rot, d["local_rel_rot"][s])
        seen |= set(np.unique(d["chosen"][s]).tolist())
    # every branch of the plan decision is in the fixture
    assert {PR.CLOSE, PR.NOT_PLANNED} <= seen and any(c >= 0 for c in seen)
    assert (d["replan"] & d["planned"]).any() and (d["replan"] & ~d["planned"]).any()
    if name == "default":
        assert PR.NONE_VALID in seen
        assert ref.no_valid == int((d["chosen"] == PR.NONE_VALID).sum())
    else:
        assert d["cand"].shape[0] % 64 and (d["curr_pose_index"].max(0) != d["curr_pose_index"].min(0)).any()


def test_unstable_argsort_picks_an_equal_key_valid_candidate():
    """The reference as it is (torch.argsort is not stable): its pick may differ from the stable one, but only among
    valid candidates of the same key."""
    d = load_set("default")
    cand = d["cand"].astype(np.float32)
    differ = 0
    for s in range(d["root"].shape[0]):
        prev_idx = np.zeros(32, np.int64) if s == 0 else np.where(d["reset"][s - 1], 0, d["curr_pose_index"][s - 1])
        for e in np.nonzero(d["chosen"][s] >= 0)[0]:
            root, lt = d["root"][s][e], d["unstable_local_target"][s][e]
            rpy = PR.quat_to_rpy(root[None, 3:7])[0]
            xy = PR.quat_apply(PR.yaw_quat(root[3:7])[None], cand[:, :3])[:, :2] + root[:2]
            pose = np.concatenate([xy, cand[:, 2:3], PR.wrap_to_pi(cand[:, 3:] + rpy)], 1)
            dist = np.maximum(np.abs(pose[:, :3] - lt[:3]).max(1), np.abs(PR.wrap_to_pi(pose[:, 3:] - lt[3:])).max(1))
            u, c = int(np.argmin(dist)), int(d["chosen"][s][e])
            assert dist[u] < 1e-5
            target = d["trajectory"][s][e].reshape(-1, 6)[prev_idx[e]]
            k = PR.keys(cand, target[:2] - root[:2])
            assert k[u] == k[c]
            assert PR.metrics(cand[u:u + 1], d["grid_x"], d["grid_y"], d["heights"][s][e])[0] > 1.0
            differ += u != c
    assert differ > 0  # the indeterminacy is real on this torch build too, or the tie rule would be untested


def test_prepare_tables_default_set():
    cand = CF.Cfg.commands.candidate_target_poses
    np.testing.assert_array_equal(cand, PR.default_candidates())
    t = P.prepare_tables(cand, np.linspace(-1, 1, 21), np.linspace(-0.5, 0.5, 11))
    assert t["cand"].shape == (1575, 6) and t["cand"].dtype == np.float32
    # 175 unique (x, y, z, yaw) rows; but quat_apply_yaw_inverse (:897) tests a candidate with roll and pitch both
    # nonzero at yaw -+ 2 atan(tan(7.5 deg)^2), so the reference's ellipsoid test has 3 x 175 distinct footprints
    assert len(np.unique(t["cand"][:, [0, 1, 2, 5]], axis=0)) == 175
    assert t["foot"].shape == (525, P.FOOT) and not t["foot"][:, 5:].any()
    np.testing.assert_array_equal(t["foot"][t["cand_foot"], :5], P.footprint_rows(t["cand"]))
    zero = (t["cand"][:, 3] == 0) | (t["cand"][:, 4] == 0)
    yaw_eff = 2 * np.arctan2(t["foot"][t["cand_foot"], 3], t["foot"][t["cand_foot"], 4])
    np.testing.assert_allclose(yaw_eff[zero], t["cand"][zero, 5], atol=1e-6)
    assert np.all(np.abs(np.abs(yaw_eff[~zero] - t["cand"][~zero, 5]) - 2 * np.arctan(np.tan(np.pi / 24) ** 2)) < 1e-6)
    # the restatement's f32 yaw quaternion (the reference's own formula) agrees with the table's
    q = PR.yaw_quat(PR.quat_from_euler_xyz(t["cand"][:, 3], t["cand"][:, 4], t["cand"][:, 5]))
    np.testing.assert_allclose(q[:, 2:], t["foot"][t["cand_foot"], 3:5], atol=2e-7)
    tc = torch.from_numpy(np.asarray(cand)).float()
    np.testing.assert_array_equal(t["key_rot"], (torch.linalg.norm(tc[:, 3:], dim=1) * 0.1).numpy())
    assert t["key_rot"].dtype == np.float32 and len(np.unique(t["key_rot"])) <= 63
    assert t["scan_x"].dtype == np.float32 and t["scan_x"].shape == (21,) and t["scan_y"].shape == (11,)


def test_prepare_tables_refusals():
    gx, gy = np.linspace(-1, 1, 21), np.linspace(-0.5, 0.5, 11)
    for bad in (np.zeros((0, 6)), np.zeros((4, 5)), np.zeros(6)):
        with pytest.raises(ValueError, match="candidate_target_poses"):
            P.prepare_tables(bad, gx, gy)
    with pytest.raises(NotImplementedError, match="GO1_PLAN_MAX_CAND"):
        P.prepare_tables(np.zeros((P.MAX_CAND + 1, 6)), gx, gy)
    with pytest.raises(NotImplementedError, match="scan"):
        P.prepare_tables(np.zeros((2, 6)), np.zeros(P.MAX_X + 1), gy)
    assert P.prepare_tables(np.zeros((P.MAX_CAND, 6)), gx, gy)["foot"].shape[0] == 1


def planning_cfg():
    cfg = CF.readme_config(n_envs=32, terrain="random_pyramid", rows=4, cols=4)
    cfg.commands.sampling_based_planning = True
    cfg.commands.plan_interval = 5
    return cfg


def test_config_guard():
    cfg = planning_cfg()
    with pytest.raises(NotImplementedError, match="sampling_based_planning"):  # the step alone does not plan
        CF.build_abi_config(cfg, n_envs=32)
    lay = __import__("legged_tracking_amd.terrain", fromlist=["x"]).tunnel_layout(cfg.terrain)
    kw = dict(n_envs=32, hf_shape=(lay.tile_x, lay.tile_y), planner=True)
    a = CF.build_abi_config(cfg, **kw)
    cfg.commands.sampling_based_planning = False
    b = CF.build_abi_config(cfg, **kw)
    assert bytes(a) == bytes(b)  # the step's config does not change: the planner is a launch of its own
    cfg.commands.sampling_based_planning = True
    for interval in (0, -3):
        cfg.commands.plan_interval = interval
        with pytest.raises(NameError, match="ep_start"):
            CF.build_abi_config(cfg, **kw)
    cfg.commands.plan_interval = 5
    good = cfg.commands.candidate_target_poses
    for bad in (np.zeros((0, 6)), np.zeros((7, 3))):
        cfg.commands.candidate_target_poses = bad
        with pytest.raises(ValueError, match="candidate_target_poses"):
            CF.build_abi_config(cfg, **kw)
    cfg.commands.candidate_target_poses = np.zeros((P.MAX_CAND + 1, 6))
    with pytest.raises(NotImplementedError, match="GO1_PLAN_MAX_CAND"):
        CF.build_abi_config(cfg, **kw)
    cfg.commands.candidate_target_poses = good
    CF.build_abi_config(cfg, **kw)
    # reaching_local_goal stays refused, planner or not
    cfg.rewards.reward_container_name = "TrajectoryTrackingRewards"
    cfg.reward_scales.reaching_local_goal = 1.0
    try:
        with pytest.raises(NotImplementedError, match="reaching_local_goal"):
            CF.build_abi_config(cfg, **kw)
    finally:
        cfg.reward_scales.reaching_local_goal = 0.0
        cfg.rewards.reward_container_name = "RewardsCrawling"


def test_header_constants_match_the_binding_and_the_restatement():
    txt = open(HEADER).read()
    d = {k: int(v.strip("()")) for k, v in re.findall(r"#define (GO1_PLAN_\w+) (\(?-?\d+\)?)", txt)}
    assert d["GO1_PLAN_ABI_VERSION"] == P.GO1_PLAN_ABI_VERSION
    assert (d["GO1_PLAN_MAX_CAND"], d["GO1_PLAN_MAX_X"], d["GO1_PLAN_MAX_Y"], d["GO1_PLAN_FOOT"]) == \
        (P.MAX_CAND, P.MAX_X, P.MAX_Y, P.FOOT)
    assert (d["GO1_PLAN_CLOSE"], d["GO1_PLAN_NONE_VALID"], d["GO1_PLAN_NOT_PLANNED"]) == \
        (P.CLOSE, P.NONE_VALID, P.NOT_PLANNED) == (PR.CLOSE, PR.NONE_VALID, PR.NOT_PLANNED)
    assert P.MAX_CAND >= 4096 and (P.MAX_X, P.MAX_Y) == (64, 32) and P.ROBOT_SIZE == PR.ROBOT_SIZE


@needs_lib
def test_library_exports_and_struct_sizes():
    lib = P.lib()
    names = sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(go1_\w+)\s*\(", open(HEADER).read(), re.M)))
    assert names == ["go1_plan_abi_sizes", "go1_plan_abi_version", "go1_plan_last_error", "go1_plan_step"]
    for n in names:
        assert hasattr(lib, n), n
    assert lib.go1_plan_abi_version() == P.GO1_PLAN_ABI_VERSION
    out = (C.c_int64 * 6)()
    lib.go1_plan_abi_sizes(out)
    assert list(out) == P.abi_sizes()


@needs_lib
def test_argument_errors_are_reported_not_thrown():
    lib = P.lib()
    c, t, s, a = P.Go1PlanConfig(), P.Go1PlanTables(), P.Go1PlanState(), P.Go1PlanArgs()

    def call():
        return lib.go1_plan_step(C.byref(c), C.byref(t), C.byref(s), C.byref(a), None)

    assert lib.go1_plan_step(None, None, None, None, None) == -1 and b"null" in lib.last_error()
    assert call() == -1 and b"n_envs" in lib.last_error()
    c.n_envs = 4
    assert call() == -1 and b"traj_length" in lib.last_error()
    c.traj_length = 1
    assert call() == -1 and b"plan_interval" in lib.last_error() and b"ep_start" in lib.last_error()
    c.plan_interval = 5
    assert call() == -1 and b"scan_nx" in lib.last_error()
    c.scan_nx, c.scan_ny = 65, 11
    assert call() == -1 and b"scan_nx" in lib.last_error()
    c.scan_nx = 21
    assert call() == -1 and b"n_cand" in lib.last_error()
    c.n_cand = P.MAX_CAND + 1
    assert call() == -1 and b"n_cand" in lib.last_error()
    c.n_cand, c.n_foot = 70, 71
    assert call() == -1 and b"n_foot" in lib.last_error()
    c.n_foot = 35
    assert call() == -1 and b"robot_size" in lib.last_error()
    c.robot_size[:] = list(P.ROBOT_SIZE)
    assert call() == -1 and b"tables" in lib.last_error()
    t.cand = t.cand_foot = t.key_rot = t.foot = 16  # never dereferenced: refused first
    assert call() == -1 and b"state" in lib.last_error()
    for f, _ in P.Go1PlanState._fields_:
        setattr(s, f, 16)
    assert call() == -1 and b"args" in lib.last_error()
    for f in ("root", "trajectory", "curr_pose_index", "episode_length", "reset", "heights", "obs"):
        setattr(a, f, 16)
    a.obs_stride = 4
    assert call() == -1 and b"obs_stride" in lib.last_error()
    a.obs_stride, a.commands, a.commands_stride = 42, 16, 1
    assert call() == -1 and b"commands_stride" in lib.last_error()


def test_binding_refuses_before_any_device_work():
    with pytest.raises(NameError, match="ep_start"):
        P.PlanBuffers(4, "cpu", PR.default_candidates(), np.zeros(21), np.zeros(11), 1, 0, 0.3, 0.5, 100.0)
    pb = P.PlanBuffers(4, "cpu", PR.default_candidates()[:70], np.zeros(5), np.zeros(3), 1, 3, 0.3, 0.5, 100.0)
    assert int(pb.chosen[0]) == P.NOT_PLANNED and not pb.plan_buf.any()
    pb.mark_reset([1, 3])
    assert pb.plan_buf.tolist() == [False, True, False, True]
    with pytest.raises(P.NativeError, match="no GPU|no CPU fallback"):
        pb.launch(*([None] * 7))


def test_plan_library_is_built_as_the_step_kernels_and_shares_nothing_with_render_and_trace():
    srcs, flags = B.LIBS["libgo1_plan.so"]
    assert srcs == ["go1_plan.hip"] and flags == B.STEP_FLAGS
    files = {os.path.basename(x) for x in B.lib_files("libgo1_plan.so")}
    assert {"go1_plan.hip", "go1_plan.h", "go1_torch_math.h", "pmath.h"} <= files
    for other in ("libgo1_render.so", "libgo1_trace.so"):  # nothing but the add-ons' host-side header
        assert files & {os.path.basename(x) for x in B.lib_files(other)} == {"go1_host.h"}
    for other in ("libgo1_mi355x.so", "libgo1_velocity.so", "libgo1_rollout.so", "libgo1_ppo.so"):
        assert "go1_host.h" not in {os.path.basename(x) for x in B.lib_files(other)}
    # its own source and header belong to no other library
    for name in B.LIBS:
        if name != "libgo1_plan.so":
            assert not {"go1_plan.hip", "go1_plan.h"} & {os.path.basename(x) for x in B.lib_files(name)}
