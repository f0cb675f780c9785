"""The HIP rollout library (libgo1_rollout.so: csrc/rollout.hip with its parts rollout_record.h, policy_full.h,
policy_split.h and rollout_colsum.h, policy_actor.hip, encoder.hip; C ABI include/go1_rollout.h), loaded once.  The
learner's leaf module: it imports learn_abi and native only."""
import os

import torch

from . import learn_abi as LA, native

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GO1_ROLLOUT_LIB_OVERRIDE") or os.path.join(HERE, "_build", "libgo1_rollout.so")

_lib = None


def lib():
    """The HIP rollout library (libgo1_rollout.so), loaded once; NativeError when it is missing or another ABI."""
    global _lib
    if _lib is None:
        _lib = native.load_library(LIB_PATH, "go1_rollout_abi_version", LA.GO1_ROLLOUT_ABI_VERSION,
                                   "go1_rollout_last_error", LA.ROLLOUT_ARGTYPES)
    return _lib


def _colsum(g):
    """Column sums of a (rows, cols) gradient (the bias gradient) with the deterministic HIP kernel
    (go1_colsum); torch's sum(0) off the GPU and for what the kernel does not take."""
    if not g.is_cuda or g.dim() != 2 or not g.is_contiguous() or g.dtype != torch.float32 or g.shape[0] < 64:
        return g.sum(0)
    rows, cols = g.shape
    parts = max(1, min(512 // ((cols + 63) // 64), rows // 256, 64))
    part = torch.empty((parts, cols), dtype=torch.float32, device=g.device)
    out = torch.empty(cols, dtype=torch.float32, device=g.device)
    native.check(lib(), lib().go1_colsum(g.data_ptr(), rows, cols, part.data_ptr(), parts, out.data_ptr(),
                                         native.raw_stream(g.device)))
    return out
