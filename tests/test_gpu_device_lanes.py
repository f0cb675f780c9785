"""The cross-lane helpers of csrc/go1_lanes.h (DPP quad moves, v_permlane16/32_swap), one full wave per value set,
against a numpy f32 restatement in the order each function's comment documents -- bit for bit, since no arithmetic
there can contract.  Lane l sits in quad l // 4 and row l // 16 (column l % 16).

  qsum               (l0 + l1) + (l2 + l3) of the quad, on its four lanes
  rowsum4, _n<3>     (r0 + r1) + (r2 + r3) of the column, on its four lanes
  pairsum_rows_n<3>  lo = r0 + r1, hi = r2 + r3, both on every lane of the column
  row1_bcast_n<2>    row 1's value, on every lane of the column
  oddrows_sum_n<3>   r1 + r3 (no zeros added: -0 + -0 stays -0, and a lone -0 ... + -0 too)
  quad_min / max     fminf / fmaxf over the quad (a NaN loses to a number)
  quad_xor<D>        the value of lane l ^ D;  quad_or: the OR over the quad
"""
import numpy as np
import pytest

from tests import devcheck as D

pytestmark = pytest.mark.gpu

NSETS = 256


def _value_sets():
    """(NSETS, 3, 64) f32: normals across 1e-8 .. 1e8 with random signs, and in classes of sets +-0 only, zeros among
    normals, inf, NaN, and cancelling sets (big, small, -big, small) whose sum depends on the order"""
    rng = np.random.default_rng(51)
    v = (rng.choice([-1.0, 1.0], (NSETS, 3, 64)) * 10.0 ** rng.uniform(-8, 8, (NSETS, 3, 64))).astype(np.float32)
    for s in range(NSETS):
        kind = s % 8
        if kind == 1:  # only zeros of either sign
            v[s] = np.where(rng.random((3, 64)) < 0.5, 0.0, -0.0)
        elif kind == 2:  # zeros of either sign among normals
            m = rng.random((3, 64))
            v[s] = np.where(m < 0.3, 0.0, np.where(m < 0.6, -0.0, v[s]))
        elif kind == 3:  # infinities (inf - inf = NaN among them)
            m = rng.random((3, 64))
            v[s] = np.where(m < 0.1, np.inf, np.where(m < 0.15, -np.inf, v[s]))
        elif kind == 4:  # NaNs
            v[s] = np.where(rng.random((3, 64)) < 0.15, np.nan, v[s])
        elif kind == 5:  # cancellation within quads and columns: the order decides the f32 result
            big = (10.0 ** rng.uniform(3, 8, (3, 64))).astype(np.float32)
            small = rng.uniform(0.1, 10.0, (3, 64)).astype(np.float32)
            lane = np.arange(64)
            pat_q = np.where(lane % 4 == 0, 1.0, np.where(lane % 4 == 2, -1.0, 0.0))  # quad: big s -big s
            bq = np.repeat(big[:, ::4], 4, axis=1)
            v[s, 0] = np.where(pat_q != 0, pat_q * bq[0], small[0])
            pat_r = np.where(lane // 16 == 0, 1.0, np.where(lane // 16 == 2, -1.0, 0.0))  # column: big s -big s
            br = np.tile(big[:, :16], (1, 4))
            v[s, 1] = np.where(pat_r != 0, pat_r * br[1], small[1])
            v[s, 2] = np.where(pat_r != 0, -pat_r * br[2], small[2])
    return v


def _same(got, want, what, zero_sign=True):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), what
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    diff = (gb != wb) & ~nan
    if not zero_sign:
        diff &= ~((got == 0) & (want == 0))
    bad = np.argwhere(diff)
    assert bad.size == 0, (what, len(bad), bad[:4], got[diff][:4], want[diff][:4])


def test_lane_helpers_bit_for_bit():
    v = _value_sets()
    out = D.lanes(v)
    assert out.shape == (NSETS, D.LANE_OUTS, 64)
    with np.errstate(all="ignore"):
        q = v.reshape(NSETS, 3, 16, 4)  # [..., quad, lane in quad]
        r = v.reshape(NSETS, 3, 4, 16)  # [..., row, column]
        qs = np.repeat(((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))[..., None], 4, -1).reshape(NSETS, 3, 64)
        lo, hi = r[:, :, 0] + r[:, :, 1], r[:, :, 2] + r[:, :, 3]
        col = lambda a: np.tile(a, (1, 1, 4))  # noqa: E731  (a column's value on its four lanes)
        rows, odd = col(lo + hi), col(r[:, :, 1] + r[:, :, 3])
        assert lo.dtype == np.float32
    k = 0
    _same(out[:, k], qs[:, 0], "qsum"); k += 1
    _same(out[:, k], rows[:, 0], "rowsum4"); k += 1
    for i in range(3):
        _same(out[:, k], rows[:, i], f"rowsum4_n[{i}]"); k += 1
    for i in range(3):
        _same(out[:, k], col(lo)[:, i], f"pairsum lo[{i}]"); k += 1
    for i in range(3):
        _same(out[:, k], col(hi)[:, i], f"pairsum hi[{i}]"); k += 1
    for i in range(2):
        _same(out[:, k], col(r[:, :, 1])[:, i], f"row1_bcast[{i}]"); k += 1
    for i in range(3):
        _same(out[:, k], odd[:, i], f"oddrows_sum[{i}]"); k += 1
    q0 = q[:, 0]
    rep = lambda a: np.repeat(a[..., None], 4, -1).reshape(NSETS, 64)  # noqa: E731
    # (min / max of +0 and -0: either zero is a correct fminf / fmaxf, so zero results are compared as values)
    for name, f in (("quad_min", np.fmin), ("quad_max", np.fmax)):
        _same(out[:, k], rep(f(f(q0[..., 0], q0[..., 1]), f(q0[..., 2], q0[..., 3]))), name, False); k += 1
    lane = np.arange(64)
    for d in (1, 2, 3):
        got, want = out[:, k].view(np.uint32), v[:, 0][:, lane ^ d].view(np.uint32)
        assert (got == want).all(), f"quad_xor<{d}>"  # a move: NaN payloads too
        k += 1
    b = v[:, 0].view(np.uint32).reshape(NSETS, 16, 4)
    want = np.repeat((b[..., 0] | b[..., 1] | b[..., 2] | b[..., 3])[..., None], 4, -1).reshape(NSETS, 64)
    assert (out[:, k].view(np.uint32) == want).all(), "quad_or"
    k += 1
    assert k == D.LANE_OUTS
    # the inputs can tell the documented orders from others: another association gives other bits in many sets
    with np.errstate(all="ignore"):
        alt_q = np.repeat((((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])[..., None], 4, -1).reshape(NSETS, 3, 64)
        alt_r = col((r[:, :, 0] + r[:, :, 2]) + (r[:, :, 1] + r[:, :, 3]))
    fin = np.isfinite(qs) & np.isfinite(alt_q)
    assert ((qs != alt_q) & fin).any(axis=(1, 2)).sum() >= NSETS // 4
    fin = np.isfinite(rows) & np.isfinite(alt_r)
    assert ((rows != alt_r) & fin).any(axis=(1, 2)).sum() >= NSETS // 4
    # and the -0 remark: sets of zeros only hold -0 sums (every term -0) as well as +0 sums
    z = odd[1::8]
    assert (z == 0).all() and np.signbit(z).any() and (~np.signbit(z)).any()
