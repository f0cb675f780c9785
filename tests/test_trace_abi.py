"""The trace library loads without a GPU, exports every entry point of include/go1_trace.h, its struct layout matches
the ctypes mirror of legged_tracking_amd/trace.py, and argument errors are reported, not thrown (no launch)."""
import ctypes as C
import os
import re

import pytest

from legged_tracking_amd import build as B, trace as T
from tests import trace_ref as TR

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "go1_trace.h")
needs_lib = pytest.mark.skipif(not os.path.exists(T.LIB_PATH), reason="libgo1_trace.so not built")


@needs_lib
def test_library_exports_every_declared_symbol():
    lib = T.lib()
    names = sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(go1_\w+)\s*\(", open(HEADER).read(), re.M)))
    assert names == ["go1_trace_abi_sizes", "go1_trace_abi_version", "go1_trace_last_error", "go1_trace_push"]
    for n in names:
        assert hasattr(lib, n), n
    assert lib.go1_trace_abi_version() == T.GO1_TRACE_ABI_VERSION


@needs_lib
def test_struct_layout_matches_ctypes_mirror():
    out = (C.c_int64 * 3)()
    T.lib().go1_trace_abi_sizes(out)
    assert list(out) == [C.sizeof(T.Go1TraceArgs), T.ROW, T.META]


def test_header_constants_match_the_binding_and_the_reference():
    txt = open(HEADER).read()
    d = {k: int(v) for k, v in re.findall(r"#define (GO1_\w+) (\d+)", txt)}
    assert d["GO1_TRACE_ABI_VERSION"] == T.GO1_TRACE_ABI_VERSION
    assert d["GO1_TRACE_ROW"] == T.ROW == TR.ROW == 13 + 12 + 1 and d["GO1_TRACE_META"] == T.META == TR.META
    assert d["GO1_TRACE_TERMINATED"] == T.TERMINATED == TR.TERMINATED
    assert d["GO1_TRACE_TIMEOUT"] == T.TIMEOUT == TR.TIMEOUT
    words = re.search(r"enum go1_trace_meta \{([^}]*)\}", txt).group(1)
    assert [w.split("=")[0].strip() for w in words.split(",")][:6] == [
        "GO1_TM_ENV", "GO1_TM_ORDINAL", "GO1_TM_END_PUSH", "GO1_TM_KEPT", "GO1_TM_LENGTH", "GO1_TM_CAUSE"]
    assert (T.TM_ENV, T.TM_ORDINAL, T.TM_END_PUSH, T.TM_KEPT, T.TM_LENGTH, T.TM_CAUSE) == (0, 1, 2, 3, 4, 5)
    assert T.want_bits(("terminated", "timeout")) == 3 and T.want_bits(("timeout",)) == 2 and T.want_bits(1) == 1
    with pytest.raises(ValueError):
        T.want_bits(("fall",))


@needs_lib
def test_argument_errors_are_reported_not_thrown():
    lib = T.lib()
    assert lib.go1_trace_push(None, None) == -1 and b"null" in lib.last_error()
    a = T.Go1TraceArgs()
    assert lib.go1_trace_push(C.byref(a), None) == -1 and b"must be set" in lib.last_error()
    a.root = a.dof_pos = a.reset = a.time_out = 16      # never dereferenced: refused first
    assert lib.go1_trace_push(C.byref(a), None) == -1 and b"ring" in lib.last_error()
    a.ring = a.ep_start = a.ep_ordinal = a.cap_rows = a.cap_meta = a.cap_count = 16
    a.n_envs, a.depth, a.capacity = 4, 0, 1
    assert lib.go1_trace_push(C.byref(a), None) == -1 and b"depth" in lib.last_error()
    a.depth, a.want = 3, 4
    assert lib.go1_trace_push(C.byref(a), None) == -1 and b"want" in lib.last_error()
    a.want, a.wp_trajectory = 3, 16
    assert lib.go1_trace_push(C.byref(a), None) == -1 and b"wp_trajectory" in lib.last_error()


def test_trace_library_is_a_library_of_its_own():
    srcs, flags = B.LIBS["libgo1_trace.so"]
    assert srcs == ["go1_trace.hip"] and flags == []
    # it shares one file, and only with the other add-on libraries: their host-side header
    addons = ("libgo1_render.so", "libgo1_trace.so", "libgo1_plan.so", "libgo1_dr.so")
    mine = {os.path.basename(x) for x in B.lib_files("libgo1_trace.so")}
    for name in B.LIBS:
        if name != "libgo1_trace.so":
            shared = mine & {os.path.basename(x) for x in B.lib_files(name)}
            assert shared == ({"go1_host.h"} if name in addons else set()), (name, shared)
