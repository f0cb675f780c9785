"""ctypes binding of go1dc_lanes_n (legged_tracking_amd/csrc/go1_devcheck.hip): the role-sum helpers of go1_lanes.h at
the sizes the step kernels instantiate them with, one full wave per value set.  The library, its loading and the
tensor plumbing are tests/devcheck.py's."""
import ctypes as C

import torch

from tests import devcheck as D

NVAL = 27  # DC_LANEN_VALS: values per set
# (helper, N) in the kernel's output order; pairsum_rows_n<N> writes its N lo values, then its N hi values
CALLS = (("rowsum4", 1), ("rowsum4", 2), ("rowsum4", 6), ("rowsum4", 15),
         ("pairsum", 1), ("pairsum", 2), ("pairsum", 27),
         ("row1", 1), ("row1", 2), ("row1", 27),
         ("odd", 1), ("odd", 2), ("odd", 21))
OUTS = sum(n * (2 if h == "pairsum" else 1) for h, n in CALLS)  # DC_LANEN_OUTS
assert OUTS == 138


def lanes_n(v):
    """(nsets, NVAL, 64) f32 -> (nsets, OUTS, 64) f32: every call of CALLS on the set's first N values"""
    l = D.lib()
    l.go1dc_lanes_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    v = D._dev(v)
    assert v.shape[1:] == (NVAL, 64)
    o = torch.empty((len(v), OUTS, 64), device="cuda")
    D._run(l.go1dc_lanes_n, v.data_ptr(), o.data_ptr(), len(v))
    return o.cpu().numpy()
