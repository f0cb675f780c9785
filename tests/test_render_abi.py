"""The render library loads without a GPU, exports every entry point of include/go1_render.h, its struct layouts
match the ctypes mirrors of legged_tracking_amd/render.py, and argument errors are reported, not thrown (no launch)."""
import ctypes as C
import os
import re

from legged_tracking_amd import build as B, model as M, render as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "go1_render.h")


def test_library_exports_every_declared_symbol():
    lib = R.lib()
    txt = open(HEADER).read()
    names = sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(go1_\w+)\s*\(", txt, re.M)))
    assert names == ["go1_render", "go1_render_abi_sizes", "go1_render_abi_version", "go1_render_last_error",
                     "go1_render_record"]
    for n in names:
        assert hasattr(lib, n), n
    assert lib.go1_render_abi_version() == R.GO1_RENDER_ABI_VERSION


def test_struct_layouts_match_ctypes_mirror():
    out = (C.c_int64 * 4)()
    R.lib().go1_render_abi_sizes(out)
    assert list(out) == [C.sizeof(R.Go1RenderModel), C.sizeof(R.Go1RenderView), C.sizeof(R.Go1RenderArgs),
                         C.sizeof(R.Go1RecordArgs)]


def test_header_constants_match_the_binding():
    txt = open(HEADER).read()
    d = {k: v for k, v in re.findall(r"#define (GO1_\w+) (\(?-?\d+\)?)", txt)}
    val = lambda k: int(d[k].strip("()"))  # noqa: E731
    assert val("GO1_PRIM_TRUNK") == R.PRIM_TRUNK and val("GO1_PRIM_FLOOR") == R.PRIM_FLOOR
    assert val("GO1_PRIM_CEILING") == R.PRIM_CEILING and val("GO1_PRIM_MARKER") == R.PRIM_MARKER
    assert val("GO1_PRIM_BACKGROUND") == R.PRIM_BACKGROUND and val("GO1_RENDER_MAX_MARKERS") == R.MAX_MARKERS
    assert val("GO1_VIEW_NO_CEILING") == R.VIEW_NO_CEILING and val("GO1_RENDER_ABI_VERSION") == R.GO1_RENDER_ABI_VERSION
    states = re.search(r"enum go1_record_state \{([^}]*)\}", txt).group(1)
    assert [s.split("=")[0].strip() for s in states.split(",")] == ["GO1_REC_IDLE", "GO1_REC_ARMED",
                                                                    "GO1_REC_RECORDING", "GO1_REC_COMPLETE"]
    assert (R.REC_IDLE, R.REC_ARMED, R.REC_RECORDING, R.REC_COMPLETE) == (0, 1, 2, 3)


def test_model_struct_comes_from_model_py():
    m = R.model_struct()
    assert tuple(m.trunk_half) == tuple(C.c_float(x / 2).value for x in M.TRUNK_BOX)
    assert m.foot_radius == C.c_float(M.FOOT_RADIUS).value and m.hip_radius == C.c_float(M.HIP_CAPSULE_RADIUS).value
    assert m.hip_origin[1][1] == -m.hip_origin[0][1] and m.hip_origin[2][0] == -m.hip_origin[0][0]   # FR, RL mirror FL
    assert m.hip_capsule_y[1][0] == -m.hip_capsule_y[0][0]
    # the bounding sphere holds every primitive of random poses (tests/self_geom.py's kinematics)
    import numpy as np
    from tests import self_geom as SG
    q = np.random.default_rng(0).uniform(-3.2, 3.2, (2000, 12))
    P, r = SG.capsules(q)
    assert (np.linalg.norm(P, axis=-1) + r[None, :, None]).max() < m.bound_radius
    assert np.linalg.norm(np.array(M.TRUNK_BOX) / 2) < m.bound_radius


def test_argument_errors_are_reported_not_thrown():
    lib = R.lib()
    assert lib.go1_render(None, None) == -1 and b"null" in lib.last_error()
    a = R.Go1RenderArgs()
    assert lib.go1_render(C.byref(a), None) == -1 and b"must be set" in lib.last_error()
    a.root = a.dof_pos = a.views = a.rgba = 16      # never dereferenced: refused first
    a.n_envs, a.n_views, a.width, a.height, a.horizontal_scale = 1, 1, 0, 8, 0.1
    assert lib.go1_render(C.byref(a), None) == -1 and b"width" in lib.last_error()
    a.width, a.tiles, a.hf_nx, a.hf_ny = 8, 16, 1, 4
    assert lib.go1_render(C.byref(a), None) == -1 and b"tiles" in lib.last_error()
    r = R.Go1RecordArgs()
    assert lib.go1_render_record(C.byref(r), None) == -1
    assert lib.go1_render_record(None, None) == -1 and b"null" in lib.last_error()


def test_render_library_keeps_the_step_libraries_build_as_it_was():
    """The ray caster is a library of its own with the plain flags; it shares no source or dependency with the
    step libraries, and with the other add-on libraries only their host-side header (go1_host.h: the error message
    and the launch check, no device code)."""
    srcs, flags = B.LIBS["libgo1_render.so"]
    assert srcs == ["go1_render.hip"] and flags == []
    addons = ("libgo1_render.so", "libgo1_trace.so", "libgo1_plan.so", "libgo1_dr.so")
    mine = {os.path.basename(x) for x in B.lib_files("libgo1_render.so")}
    for name in B.LIBS:
        if name != "libgo1_render.so":
            shared = mine & {os.path.basename(x) for x in B.lib_files(name)}
            assert shared == ({"go1_host.h"} if name in addons else set()), (name, shared)
    host = open(os.path.join(B.HERE, "csrc", "go1_host.h")).read()
    assert "__global__" not in host and "__device__" not in host and '#include "' not in host
    assert "go1_model_consts.h" not in open(os.path.join(B.HERE, "csrc", "go1_render.hip")).read()
