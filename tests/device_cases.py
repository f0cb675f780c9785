"""Inputs of the portable-math checks, shared by tests/test_portable_math.py (the oracle copy against float64, on the
CPU) and tests/test_gpu_device_math.py (the HIP copy against the oracle copy, bit for bit).  Every function is cached
and returns read-only f32 arrays."""
import functools

import numpy as np

N_DRAWS = 2_000_000
TWO_PI_F = np.float32(2.0 * np.pi)  # go1_device.h TWO_PI_F, torch's f32 scalar
ATAN2_GRID = np.array([s * v for v in (0.0, 1.0, 1e-30, 1e30, 1e-45, 3e38) for s in (1.0, -1.0)]
                      + [0.41421357, 2.4142137], np.float32)


def _ro(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


def _around(x):
    """x and its two f32 neighbours"""
    x = np.asarray(x, np.float32)
    return np.concatenate([x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))])


@functools.lru_cache(None)
def sincos_uniform(lim):
    return _ro(np.random.default_rng(int(lim)).uniform(-lim, lim, N_DRAWS))


@functools.lru_cache(None)
def sincos_near_quadrants():
    """every f32 within one step of k pi / 2, |x| <= 1e4"""
    k = np.arange(-6366, 6367)
    return _ro(_around((k * (np.pi / 2)).astype(np.float32)))


@functools.lru_cache(None)
def asin_inputs():
    """(uniform draws on [-1, 1], the edges: +-1, +-0.5 and their neighbours, +-0, 1e-20, 1e-40 (subnormal))"""
    u = np.random.default_rng(11).uniform(-1.0, 1.0, N_DRAWS)
    e = np.concatenate([_around([1.0, -1.0, 0.5, -0.5]), np.array([0.0, -0.0, 1e-20, -1e-20, 1e-40, -1e-40])])
    e = e[np.abs(e) <= 1.0]
    return _ro(u), _ro(e)


@functools.lru_cache(None)
def atan_inputs():
    """atan alone: log-uniform magnitudes and the two thresholds with their neighbours, +-0, subnormals, inf"""
    rng = np.random.default_rng(12)
    u = rng.choice([-1.0, 1.0], N_DRAWS) * 10.0 ** rng.uniform(-6, 6, N_DRAWS)
    e = np.concatenate([_around([0.41421357, -0.41421357, 2.4142137, -2.4142137, 1.0]),
                        np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, 3e38])])
    return _ro(u), _ro(e)


@functools.lru_cache(None)
def atan2_uniform():
    """(y, x): signs at random, magnitudes log-uniform in [1e-6, 1e6]"""
    rng = np.random.default_rng(13)
    y, x = (rng.choice([-1.0, 1.0], N_DRAWS) * 10.0 ** rng.uniform(-6, 6, N_DRAWS) for _ in range(2))
    return _ro(y), _ro(x)


@functools.lru_cache(None)
def atan2_grid():
    """(y, x): the full grid of ATAN2_GRID in both arguments"""
    y, x = np.meshgrid(ATAN2_GRID, ATAN2_GRID, indexing="ij")
    return _ro(y.ravel()), _ro(x.ravel())


@functools.lru_cache(None)
def remainder_inputs():
    """(a, b): a in +-20 uniform, exact multiples of the divisor, +-0, +-1e10; b = TWO_PI_F and 1.0"""
    u = np.random.default_rng(14).uniform(-20.0, 20.0, 200_000).astype(np.float32)
    out_a, out_b = [], []
    for b in (TWO_PI_F, np.float32(1.0)):
        k = np.arange(-4, 5).astype(np.float32)
        a = np.concatenate([u, k * b, _around(k * b), np.array([0.0, -0.0, 1e10, -1e10], np.float32)])
        out_a.append(a)
        out_b.append(np.full(a.shape, b, np.float32))
    return _ro(np.concatenate(out_a)), _ro(np.concatenate(out_b))


def ulp32(x):
    """the f32 ulp at |x| (float64 array)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
