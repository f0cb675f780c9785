"""ctypes binding of the test-only device-function library (legged_tracking_amd/csrc/go1_devcheck.hip,
libgo1_devcheck.so): torch tensors in and out, one function per launcher.  GO1_DEVCHECK_LIB, when set, names the
library to load instead of the built one (a devcheck build of a deliberately altered copy of csrc/, to show that the
tests notice: DESIGN.md, "device-function checks")."""
import ctypes as C
import os

import numpy as np
import torch

from legged_tracking_amd import build as B

NAME = "libgo1_devcheck.so"
LANE_OUTS = 22  # DC_LANE_OUTS
PSZX, PSZY = 20, 16  # go1_contact.h
_lib = None
P, I, F = C.c_void_p, C.c_int, C.c_float


def lib_path():
    return os.environ.get("GO1_DEVCHECK_LIB") or os.path.join(B.BUILD, NAME)


def lib():
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"device-check library missing: {path} (run python -c 'import __graft_entry__ as g; "
                               "g.build()')")
        l = C.CDLL(path)
        l.go1dc_pm1.argtypes = [I, P, P, P, I, P]
        l.go1dc_pm2.argtypes = [I, P, P, P, I, P]
        l.go1dc_softsign2.argtypes = [P, P, I, P]
        l.go1dc_quat.argtypes = [I, P, P, P, I, P]
        l.go1dc_solve6.argtypes = [P, P, P, P, I, P]
        l.go1dc_lanes.argtypes = [P, P, I, P]
        l.go1dc_seg_closest.argtypes = [P] * 5 + [I, P]
        l.go1dc_seg_box_t.argtypes = [P] * 6 + [I, P]
        l.go1dc_terrain.argtypes = [I, P, P, P, F, I, I] + [P] * 8 + [P]
        _lib = l
    return _lib


def _dev(x, dtype=torch.float32):
    """a contiguous cuda tensor of the numpy array / tensor x"""
    if isinstance(x, np.ndarray) and not x.flags.writeable:
        x = x.copy()  # (the shared cases are read-only; torch wants a writable array to wrap)
    return torch.as_tensor(x).to(device="cuda", dtype=dtype).contiguous()


def _run(fn, *args):
    rc = fn(*args, None)  # the null stream
    assert rc == 0, rc
    torch.cuda.synchronize()


def _pm1(fn, x, two=False):
    x = _dev(x).reshape(-1)
    o0, o1 = torch.empty_like(x), torch.empty_like(x) if two else None
    _run(lib().go1dc_pm1, fn, x.data_ptr(), o0.data_ptr(), o1.data_ptr() if two else None, x.numel())
    return (o0.cpu().numpy(), o1.cpu().numpy()) if two else o0.cpu().numpy()


def pm_sincos(x):
    return _pm1(0, x, True)


def pm_asin(x):
    return _pm1(1, x)


def pm_atan(x):
    return _pm1(2, x)


def pm_softsign(x):
    return _pm1(3, x)


def wrap_to_pi(x):
    return _pm1(4, x)


def hw_sincos(x):
    return _pm1(5, x, True)


def _pm2(fn, a, b):
    a, b = _dev(a).reshape(-1), _dev(b).reshape(-1)
    assert a.numel() == b.numel()
    o = torch.empty_like(a)
    _run(lib().go1dc_pm2, fn, a.data_ptr(), b.data_ptr(), o.data_ptr(), a.numel())
    return o.cpu().numpy()


def pm_atan2(y, x):
    return _pm2(0, y, x)


def remainder(a, b):
    return _pm2(1, a, b)


def pm_softsign2(x):
    """pm_softsign2 on the pairs (x[2 i], x[2 i + 1]) of an even-sized array"""
    x = _dev(x).reshape(-1)
    assert x.numel() % 2 == 0
    o = torch.empty_like(x)
    _run(lib().go1dc_softsign2, x.data_ptr(), o.data_ptr(), x.numel() // 2)
    return o.cpu().numpy()


def quat_rotate_inverse(q, v):
    q, v = _dev(q).reshape(-1, 4), _dev(v).reshape(-1, 3)
    o = torch.empty_like(v)
    _run(lib().go1dc_quat, 0, q.data_ptr(), v.data_ptr(), o.data_ptr(), len(q))
    return o.cpu().numpy()


def quat_to_rpy(q):
    q = _dev(q).reshape(-1, 4)
    o = torch.empty((len(q), 3), device="cuda")
    _run(lib().go1dc_quat, 1, q.data_ptr(), None, o.data_ptr(), len(q))
    return o.cpu().numpy()


def solve6(A, b):
    """x of solve6p for (n, 6, 6) symmetric A packed as the kernel packs a spatial inertia, and what sip_get reads
    back from that packing (n, 6, 6)"""
    A, b = _dev(A).reshape(-1, 36), _dev(b).reshape(-1, 6)
    assert len(A) == len(b)
    x, G = torch.empty_like(b), torch.empty_like(A)
    _run(lib().go1dc_solve6, A.data_ptr(), b.data_ptr(), x.data_ptr(), G.data_ptr(), len(A))
    return x.cpu().numpy(), G.cpu().numpy().reshape(-1, 6, 6)


def lanes(v):
    """(nsets, 3, 64) f32 -> (nsets, LANE_OUTS, 64) f32 (see dc_lanes for the order)"""
    v = _dev(v)
    assert v.shape[1:] == (3, 64)
    o = torch.empty((len(v), LANE_OUTS, 64), device="cuda")
    _run(lib().go1dc_lanes, v.data_ptr(), o.data_ptr(), len(v))
    return o.cpu().numpy()


def seg_closest(P0, P1, Q0, Q1):
    a = [_dev(x).reshape(-1, 3) for x in (P0, P1, Q0, Q1)]
    st = torch.empty((len(a[0]), 2), device="cuda")
    _run(lib().go1dc_seg_closest, *(x.data_ptr() for x in a), st.data_ptr(), len(st))
    return st.cpu().numpy()


def seg_box_t(P0, P1, R, pos, th):
    p0, p1, ps = (_dev(x).reshape(-1, 3) for x in (P0, P1, pos))
    r, h = _dev(R).reshape(-1, 9), _dev(th).reshape(3)
    assert len(r) == len(p0) == len(p1) == len(ps)
    t = torch.empty(len(p0), device="cuda")
    _run(lib().go1dc_seg_box_t, p0.data_ptr(), p1.data_ptr(), r.data_ptr(), ps.data_ptr(), h.data_ptr(), t.data_ptr(),
         len(t))
    return t.cpu().numpy()


def terrain(mode, tiles, env_i, hs, pt, A, B, r, stage=None):
    """The terrain queries of nenv waves (see dc_terrain).  tiles: flat f32 array holding every env's (2, nx, ny)
    tile; env_i: (nenv, 5) ints (offset, nx, ny, pi0, pj0); pt (N, 2), A, B (N, 3), r (N,) with N = nenv * 64 * nq,
    lane l of env e running queries (e * nq + k) * 64 + l.  mode 0: patch and tile, 1: tile only, 2: plane.
    stage: the array the patches are staged from (default: tiles).  Returns dict(hq (N, 9), t (N,), cell (N,),
    hqc (N, 6))."""
    tiles = _dev(tiles).reshape(-1)
    stage = tiles if stage is None else _dev(stage).reshape(-1)
    assert stage.numel() == tiles.numel()
    env_np = np.ascontiguousarray(env_i, np.int32).reshape(-1, 5)
    for off, nx, ny, _, _ in env_np:  # every env's tile lies inside the array
        assert off >= 0 and nx >= 1 and ny >= 1 and off + 2 * nx * ny <= tiles.numel()
    env = _dev(env_np, torch.int32)
    pt, A, B, r = _dev(pt).reshape(-1, 2), _dev(A).reshape(-1, 3), _dev(B).reshape(-1, 3), _dev(r).reshape(-1)
    N = len(pt)
    assert N % (64 * len(env)) == 0 and len(A) == len(B) == len(r) == N
    nq = N // (64 * len(env))
    hq = torch.empty((N, 9), device="cuda")
    t = torch.empty(N, device="cuda")
    cell = torch.empty(N, device="cuda", dtype=torch.int32)
    hqc = torch.empty((N, 6), device="cuda")
    _run(lib().go1dc_terrain, mode, tiles.data_ptr(), stage.data_ptr(), env.data_ptr(), float(hs), len(env), nq,
         pt.data_ptr(), A.data_ptr(), B.data_ptr(), r.data_ptr(), hq.data_ptr(), t.data_ptr(), cell.data_ptr(),
         hqc.data_ptr())
    return dict(hq=hq.cpu().numpy(), t=t.cpu().numpy(), cell=cell.cpu().numpy(), hqc=hqc.cpu().numpy())
