"""The step kernels' math device functions on their own (csrc/pmath.h, go1_torch_math.h, go1_spatial.h's hw_sincosf
and solve6p), through the test-only library of csrc/go1_devcheck.hip (tests/devcheck.py).

Contract-off functions (pmath.h, go1_torch_math.h) are compared BIT FOR BIT with the oracle's copies on the inputs
on which tests/test_portable_math.py bounds those copies against float64; the integrator's functions (contract on;
the fusion in the check kernel may differ from the step kernel's) within bounds against float64:

  hw_sincosf, |x| <= 8     measured max abs error 7.26e-7 (MI355X); asserted 2 x = HW_SINCOS_ABS
  hw_sincosf, |x| <= 1e4   HW_SINCOS_ABS + 2^-22 |x| (the rounding of x / 2 pi in f32, which fract cannot recover)
  solve6p                  relative forward error <= 64 x 2^-24 x cond(M) (Cholesky's backward stability, n = 6)
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import device_cases as DC
from tests import devcheck as D

pytestmark = pytest.mark.gpu

HW_SINCOS_MEASURED = 7.26e-7  # max abs error on |x| <= 8, MI355X
HW_SINCOS_ABS = 2 * HW_SINCOS_MEASURED


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, what):
    """equal as uint32; NaN results only have to be NaN on both sides"""
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), what
    bad = np.nonzero((_bits(got) != _bits(want)) & ~nan)[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


SPECIAL = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-45, -1e-45, 0.0, -0.0], np.float32)


def test_pm_sincos_bit_for_bit():
    for x in (DC.sincos_uniform(10.0), DC.sincos_uniform(1e3), DC.sincos_uniform(1e4), DC.sincos_near_quadrants(),
              SPECIAL):
        s, c = D.pm_sincos(x)
        so, co = O.pm_sincos(x)
        _same_bits(s, so, "sin")
        _same_bits(c, co, "cos")


def test_pm_asin_atan_bit_for_bit():
    u, e = DC.asin_inputs()
    for x in (u, e, SPECIAL, np.array([1.5, -1.5], np.float32)):
        _same_bits(D.pm_asin(x), O.pm_asin(x), "asin")
    u, e = DC.atan_inputs()
    for x in (u, e, SPECIAL):
        _same_bits(D.pm_atan(x), O.pm_atan(x), "atan")


def test_pm_atan2_bit_for_bit():
    sy, sx = np.meshgrid(SPECIAL, SPECIAL, indexing="ij")
    for y, x in (DC.atan2_uniform(), DC.atan2_grid(), (sy.ravel(), sx.ravel())):
        _same_bits(D.pm_atan2(y, x), O.pm_atan2(y, x), "atan2")


def _softsign_ref(x):
    with np.errstate(all="ignore"):
        return (x / (np.abs(x) + np.float32(1.0))).astype(np.float32)


def test_softsign_equals_the_ieee_quotient():
    """pm_softsign and pm_softsign2 against numpy's f32 x / (|x| + 1) on 16 M random bit patterns (four arrays of
    4 M) and the edges.  (The exhaustive run over all 2^32 inputs lives only in tools/probes/softsign_div.hip,
    outside the suite.)"""
    p2 = 2.0 ** np.arange(24, 32)
    edges = np.concatenate([p2, -p2, np.nextafter(p2.astype(np.float32), np.float32(0)), p2 + 2.0, p2 * 1.5,
                            [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38,
                             3.4028235e38, -3.4028235e38, 1.0, -1.0, 16777215.0, 16777217.0, 33554430.0]])
    edges = edges.astype(np.float32)
    edges = np.concatenate([edges, edges[:1]]) if edges.size % 2 else edges
    rng = np.random.default_rng(21)
    for k in range(5):
        x = edges if k == 4 else rng.integers(0, 2 ** 32, 4_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
        want = _softsign_ref(x)
        _same_bits(D.pm_softsign(x), want, "softsign")
        _same_bits(D.pm_softsign2(x), want, "softsign2")
        if k == 4:  # the signs of zero quotients and the saturated ends
            assert np.signbit(want[x == 0]).tolist() == np.signbit(x[x == 0]).tolist()


def test_remainder_and_wrap_equal_the_cpu_torch_values():
    """remainder_f (the two cheap cases and the fmodf path: 1e10) and wrap_to_pi_f on the inputs of
    tests/test_portable_math.py, against torch.remainder on CPU f32 as values and the oracle bit for bit."""
    a, b = DC.remainder_inputs()
    got = D.remainder(a, b)
    want = torch.remainder(torch.from_numpy(a.copy()), torch.from_numpy(b.copy())).numpy()
    assert not np.isnan(got).any()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (a[bad[:5]], b[bad[:5]], got[bad[:5]], want[bad[:5]])
    _same_bits(got, O.remainder(a, b), "remainder")
    sel = b == DC.TWO_PI_F
    w = torch.remainder(torch.from_numpy(a[sel].copy()), float(DC.TWO_PI_F))
    w = torch.where(w > np.pi, w - float(DC.TWO_PI_F), w).numpy()
    gw = D.wrap_to_pi(a[sel])
    assert (gw == w).all()
    _same_bits(gw, O.wrap_to_pi(a[sel]), "wrap_to_pi")
    # NaN / inf arguments take the fmodf path and give NaN, as torch does
    sp = np.array([np.nan, np.inf, -np.inf], np.float32)
    assert np.isnan(D.remainder(sp, np.full(3, DC.TWO_PI_F))).all()


def test_quat_rotate_inverse_against_the_planner_copy():
    """quat_rotate_inverse_f against the planner's float64 quat_apply_inverse (planner_math.npz): each row within
    4 x the f32 torch stub's own error on that row (its largest component), plus 1e-6; and the oracle's bits."""
    from tests.test_oracle_math import _planner_outputs, _stub, apply_inputs
    q, v = (x.astype(np.float32) for x in apply_inputs())
    want = _planner_outputs()["quat_apply_inverse"]
    stub = _stub().quat_rotate_inverse(torch.from_numpy(q), torch.from_numpy(v)).numpy().astype(np.float64)
    stub_err = np.abs(stub - want).max(1)
    got = D.quat_rotate_inverse(q, v)
    err = np.abs(got.astype(np.float64) - want).max(1)
    print(f"\nquat_rotate_inverse: worst error {err.max():.3e}, the stub's {stub_err.max():.3e}")
    assert (err <= 4 * stub_err + 1e-6).all(), (err - 4 * stub_err).max()
    _same_bits(got, O.quat_rotate_inverse(q, v), "quat_rotate_inverse")


def test_quat_to_rpy_bit_for_bit_and_against_float64():
    from tests.test_portable_math import ang_err, rpy_reference
    q, want, stub_err = rpy_reference()
    got = D.quat_to_rpy(q)
    _same_bits(got, O.quat_to_rpy(q), "quat_to_rpy")  # gimbal rows (q[4:7]) included
    err = ang_err(got, want)
    print(f"\nquat_to_rpy: worst error {err.max():.3e}, the stub's {stub_err.max():.3e}")
    assert (err <= 4 * stub_err + 1e-6).all(), (err - 4 * stub_err).max()


def test_hw_sincos_against_float64():
    rng = np.random.default_rng(31)
    x8 = np.concatenate([rng.uniform(-8, 8, 2_000_000), [0.0, -0.0, np.pi, -np.pi, np.pi / 2, 8.0, -8.0]])
    x8 = x8.astype(np.float32)
    s, c = D.hw_sincos(x8)
    x64 = x8.astype(np.float64)
    e8 = max(np.abs(s - np.sin(x64)).max(), np.abs(c - np.cos(x64)).max())
    print(f"\nhw_sincosf |x| <= 8: max abs error {e8:.3e} (asserted {HW_SINCOS_ABS:.2e})")
    assert e8 <= HW_SINCOS_ABS
    x = rng.uniform(-1e4, 1e4, 2_000_000).astype(np.float32)
    s, c = D.hw_sincos(x)
    x64 = x.astype(np.float64)
    e = np.maximum(np.abs(s - np.sin(x64)), np.abs(c - np.cos(x64)))
    bound = HW_SINCOS_ABS + 2.0 ** -22 * np.abs(x64)
    print(f"hw_sincosf |x| <= 1e4: max abs error {e.max():.3e}, worst share of its bound {(e / bound).max():.2f}")
    assert (e <= bound).all()


def _spd_systems(n, rng):
    """n SPD 6 x 6 systems Q diag(lam) Q^T, lam log-uniform in [1e-3, 10], as the f32 matrices the kernel reads"""
    Q = np.linalg.qr(rng.normal(size=(n, 6, 6)))[0]
    lam = 10.0 ** rng.uniform(-3, 1, (n, 6))
    A = np.einsum("nik,nk,njk->nij", Q, lam, Q)
    A = (0.5 * (A + A.transpose(0, 2, 1))).astype(np.float32)
    return A, rng.normal(size=(n, 6)).astype(np.float32)


def test_solve6p_against_float64():
    rng = np.random.default_rng(41)
    A, b = _spd_systems(20_000, rng)
    x, G = D.solve6(A, b)
    assert (G == A).all()  # the check kernel's packing, read back through sip_get
    A64, b64 = A.astype(np.float64), b.astype(np.float64)
    ref = np.linalg.solve(A64, b64[..., None])[..., 0]
    kappa = np.linalg.cond(A64)
    rel = np.linalg.norm(x - ref, axis=1) / np.linalg.norm(ref, axis=1)
    bound = 64 * 2.0 ** -24 * kappa
    print(f"\nsolve6p: worst relative error {rel.max():.3e}; worst share of 64 x 2^-24 x cond: "
          f"{(rel / bound).max():.3f} (cond up to {kappa.max():.2e})")
    assert np.isfinite(x).all()
    assert (rel <= bound).all()
    # rank-deficient: one eigenvalue 0 (and the zero matrix): finite values, by the fmaxf(s, 1e-30f) guard
    Q = np.linalg.qr(rng.normal(size=(6, 6)))[0]
    S = (Q * np.array([0.0, 1.0, 2.0, 0.5, 3.0, 1.5])) @ Q.T
    S = np.stack([0.5 * (S + S.T), np.zeros((6, 6))]).astype(np.float32)
    xs, _ = D.solve6(S, np.ones((2, 6), np.float32))
    assert np.isfinite(xs).all()
