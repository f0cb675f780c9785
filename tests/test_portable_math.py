"""The oracle's copy of the portable f32 math (oracle/portable_math.h, and go1_oracle.c's remainder / wrap / rpy)
against float64 on its own -- no step, no fixture.  The HIP copy (csrc/pmath.h) is held to this copy bit for bit on
the same inputs by tests/test_gpu_device_math.py, so the two files together bound the kernels' functions.

Measured maxima of the oracle copy against float64 on the inputs of tests/device_cases.py (CPU), and the asserted
bounds (1.5 x):

  function              maximum                     bound
  sin / cos, |x| <= 1e4 abs 9.3e-8                  1.395e-7
  asin                  abs 1.66e-7 (2.3 ulp)       2.49e-7
  atan2                 abs 2.61e-7 (3.06 ulp)      3.915e-7

(This file's seeds give 9.2e-8, 1.65e-7 and 2.66e-7; each test prints its figure.)

The bounds are absolute: near a multiple of pi the reduced argument carries the rounding of x - j pi / 2 (three
Cody-Waite terms), so the relative error of sin / cos is unbounded in ulps (5.8 ulp for |x| <= 10, ~600 ulp near
multiples of pi at |x| ~ 1e3) while the absolute error stays at the level above."""
import numpy as np
import torch

from oracle import oracle as O
from tests import device_cases as DC

SINCOS_ABS = 1.5 * 9.3e-8
ASIN_ABS = 1.5 * 1.66e-7
ATAN2_ABS = 1.5 * 2.61e-7


def _err(got, want):
    return np.abs(got.astype(np.float64) - want)


def test_sincos_against_float64():
    worst = {}
    for name, x in [("|x|<=10", DC.sincos_uniform(10.0)), ("|x|<=1e3", DC.sincos_uniform(1e3)),
                    ("|x|<=1e4", DC.sincos_uniform(1e4)), ("near k pi/2", DC.sincos_near_quadrants())]:
        s, c = O.pm_sincos(x)
        x64 = x.astype(np.float64)
        es, ec = _err(s, np.sin(x64)), _err(c, np.cos(x64))
        worst[name] = max(es.max(), ec.max())
        print(f"\nsin/cos {name}: max abs error {worst[name]:.3e}", end="")
        assert not np.isnan(s).any() and not np.isnan(c).any()
        assert worst[name] <= SINCOS_ABS, (name, worst[name])
    # sin(+-0) is a zero (+0 for both: the reduction's fma(-j, hi, x) adds +0 to -0), cos(0) is exactly 1
    s, c = O.pm_sincos(np.array([0.0, -0.0], np.float32))
    assert (s == 0.0).all() and (c == 1.0).all()


def test_asin_against_float64():
    u, e = DC.asin_inputs()
    for name, x in (("uniform", u), ("edges", e)):
        got = O.pm_asin(x)
        want = np.arcsin(x.astype(np.float64))
        err = _err(got, want)
        print(f"\nasin {name}: max abs error {err.max():.3e} ({(err / DC.ulp32(want)).max():.2f} ulp)", end="")
        assert not np.isnan(got).any()
        assert err.max() <= ASIN_ABS, (name, err.max())
        assert (np.signbit(got) == np.signbit(x)).all()  # asin's sign is its argument's, zeros included
    z = O.pm_asin(np.array([0.0, -0.0, 1e-40, -1e-40, 1e-20], np.float32))
    assert z[0] == 0 and z[1] == 0 and (z[2:] == np.array([1e-40, -1e-40, 1e-20], np.float32)).all()
    one = O.pm_asin(np.array([1.0, -1.0], np.float32))
    assert abs(float(one[0]) - np.pi / 2) <= ASIN_ABS and one[1] == -one[0]


def test_atan_thresholds_against_float64():
    """atan alone, with the two range thresholds (0.414..., 2.414...) and their neighbours; the atan2 bound holds"""
    u, e = DC.atan_inputs()
    for x in (u, e):
        got = O.pm_atan(x)
        assert not np.isnan(got).any()
        assert _err(got, np.arctan(x.astype(np.float64))).max() <= ATAN2_ABS
        assert (np.signbit(got) == np.signbit(x)).all()


def test_atan2_against_float64():
    for name, (y, x) in (("magnitudes 1e-6..1e6", DC.atan2_uniform()), ("grid", DC.atan2_grid())):
        got = O.pm_atan2(y, x)
        want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
        err = _err(got, want)
        print(f"\natan2 {name}: max abs error {err.max():.3e}", end="")
        assert not np.isnan(got).any(), name
        assert err.max() <= ATAN2_ABS, (name, err.max(), y[err.argmax()], x[err.argmax()])
        # the sign of the result is y's wherever the exact result is not 0 (a +-0 result has y's sign too:
        # atan2(+-0, x > 0) = +-0), as IEEE atan2 has it
        assert (np.signbit(got) == np.signbit(y)).all(), name
        zero = want == 0.0
        assert (got[zero] == 0.0).all() and (np.signbit(got[zero]) == np.signbit(want[zero])).all()


def test_remainder_restatement_equals_torch_remainder():
    """go1_oracle.c remainder_f (fmodf and the sign fix) against torch.remainder on CPU f32, as values, for the
    divisors TWO_PI_F and 1.0; wrap_to_pi_f against the reference's wrap_to_pi restated in torch f32."""
    a, b = DC.remainder_inputs()
    got = O.remainder(a, b)
    want = torch.remainder(torch.from_numpy(a.copy()), torch.from_numpy(b.copy())).numpy()
    assert got.dtype == want.dtype == np.float32
    assert not np.isnan(got).any() and not np.isnan(want).any()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (a[bad[:5]], b[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert ((got >= 0) & (got <= b)).all()  # (= b: a tiny negative a plus b rounds to b, in torch too)
    sel = b == DC.TWO_PI_F
    w = torch.remainder(torch.from_numpy(a[sel].copy()), float(DC.TWO_PI_F))
    w = torch.where(w > np.pi, w - float(DC.TWO_PI_F), w).numpy()
    gw = O.wrap_to_pi(a[sel])
    assert (gw == w).all()
    assert (np.abs(gw) <= np.float32(np.pi)).all()


def rpy_reference():
    """test_oracle_math.euler_inputs()' quaternions as f32, the planner's float64 angles recorded in planner_math.npz
    (3, n), and the error (mod 2 pi) of the f32 torch stub (refstubs isaacgym.torch_utils.get_euler_xyz on the CPU)
    against them per row and angle (n, 3): the yardstick of the rpy checks, here and in test_gpu_device_math.py"""
    from tests.test_oracle_math import _planner_outputs, _stub, euler_inputs
    q = euler_inputs()[0]
    want = _planner_outputs()["get_euler_xyz"]
    q = q.astype(np.float32)
    stub = np.stack([x.numpy().astype(np.float64) for x in _stub().get_euler_xyz(torch.from_numpy(q))], 1)
    return q, want, ang_err(stub, want)


def ang_err(got, want):
    """|got (n, 3) - want (3, n)| as angles mod 2 pi"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want).T) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def test_quat_to_rpy_export_against_float64():
    """The oracle's quat_to_rpy_f against the planner's float64 copy (angles mod 2 pi): each row's error is at most
    4 x the error of the f32 torch stub on that row, plus 1e-6 (the bound tests/test_gpu_device_math.py holds the
    HIP function to; the two are bit-identical there)."""
    q, want, stub_err = rpy_reference()
    got = O.quat_to_rpy(q)
    assert not np.isnan(got).any() and np.abs(got).max() <= np.float32(np.pi)
    err = ang_err(got, want)
    print(f"\nrpy: worst error {err.max():.3e}, the stub's {stub_err.max():.3e}; worst excess over 4 x stub "
          f"{(err - 4 * stub_err).max():.3e}")
    assert (err <= 4 * stub_err + 1e-6).all()
