"""The role sums of csrc/go1_lanes.h at the sizes the step kernels use, which take their values two per lane swap:
rowsum4_n<1, 2, 6, 15>, pairsum_rows_n<1, 2, 27>, row1_bcast_n<1, 2, 27>, oddrows_sum_n<1, 2, 21> -- a lone value, one
pair, and the kernels' even and odd counts -- one full wave per value set, bit for bit against a numpy f32
restatement in the documented orders (lane l sits in row l // 16, column l % 16):

  rowsum4_n        (r0 + r1) + (r2 + r3) of the column, on its four lanes
  pairsum_rows_n   lo = r0 + r1, hi = r2 + r3, both on every lane of the column
  row1_bcast_n     row 1's value on every lane of the column; rows 0, 2 and 3 never reach it
  oddrows_sum_n    r1 + r3 with no zero added; rows 0 and 2 never reach it

Every value and lane of the normal sets is distinct, so a pair whose members came back exchanged, or a result taken
from the other member's rows, shows.
"""
import numpy as np
import pytest

from tests import devcheck_lanes as L
from tests.test_gpu_device_lanes import _same

pytestmark = pytest.mark.gpu

NSETS = 64
NV = L.NVAL


def _value_sets():
    """(NSETS, 27, 64) f32 in the classes of test_gpu_device_lanes._value_sets -- normals across 1e-8 .. 1e8 with
    random signs, +-0 only, zeros among normals, inf, NaN, cancelling columns (big, small, -big, small) -- and two
    classes that put inf and NaN on the rows that must not contribute: 6 on rows 0 and 2 (oddrows_sum_n), 7 on rows 0,
    2 and 3 (row1_bcast_n)"""
    rng = np.random.default_rng(1151)
    shp = (NV, 64)
    v = (rng.choice([-1.0, 1.0], (NSETS, *shp)) * 10.0 ** rng.uniform(-8, 8, (NSETS, *shp))).astype(np.float32)
    row = np.arange(64) // 16
    for s in range(NSETS):
        kind = s % 8
        if kind == 1:
            v[s] = np.where(rng.random(shp) < 0.5, 0.0, -0.0)
        elif kind == 2:
            m = rng.random(shp)
            v[s] = np.where(m < 0.3, 0.0, np.where(m < 0.6, -0.0, v[s]))
        elif kind == 3:
            m = rng.random(shp)
            v[s] = np.where(m < 0.1, np.inf, np.where(m < 0.15, -np.inf, v[s]))
        elif kind == 4:
            v[s] = np.where(rng.random(shp) < 0.15, np.nan, v[s])
        elif kind == 5:  # the order of the column's additions decides the f32 result
            big = np.tile((10.0 ** rng.uniform(3, 8, (NV, 16))).astype(np.float32), (1, 4))
            small = rng.uniform(0.1, 10.0, shp).astype(np.float32)
            sgn = np.where(np.arange(NV) % 2 == 0, 1.0, -1.0)[:, None]
            pat = np.where(row == 0, 1.0, np.where(row == 2, -1.0, 0.0))[None, :]
            v[s] = np.where(pat != 0, sgn * pat * big, small)
        elif kind >= 6:
            bad = np.isin(row, (0, 2) if kind == 6 else (0, 2, 3))[None, :]
            poison = rng.choice(np.array([np.inf, -np.inf, np.nan], np.float32), shp)
            v[s] = np.where(bad, poison, v[s])
    return v


def test_role_sums_at_kernel_sizes_bit_for_bit():
    v = _value_sets()
    nrm = v[0::8]  # the normal sets: every value and lane distinct
    assert len(np.unique(nrm.view(np.uint32))) == nrm.size
    out = L.lanes_n(v)
    assert out.shape == (NSETS, L.OUTS, 64)
    with np.errstate(all="ignore"):
        r = v.reshape(NSETS, NV, 4, 16)  # [..., row, column]
        col = lambda a: np.tile(a, (1, 1, 4))  # noqa: E731  (a column's value on its four lanes)
        lo, hi = r[:, :, 0] + r[:, :, 1], r[:, :, 2] + r[:, :, 3]
        want = {"rowsum4": col(lo + hi), "lo": col(lo), "hi": col(hi), "row1": col(r[:, :, 1]),
                "odd": col(r[:, :, 1] + r[:, :, 3])}
        assert all(w.dtype == np.float32 for w in want.values())
    k = 0
    for helper, n in L.CALLS:
        for part in (("lo", "hi") if helper == "pairsum" else (helper,)):
            for i in range(n):
                _same(out[:, k], want[part][:, i], f"{part}_n<{n}>[{i}]")
                k += 1
    assert k == L.OUTS
    # the rows that must not contribute held inf / NaN, and the expected (hence the computed) results are finite
    assert not np.isfinite(v[6::8].reshape(-1, NV, 4, 16)[:, :, (0, 2)]).any()
    assert not np.isfinite(v[7::8].reshape(-1, NV, 4, 16)[:, :, (0, 2, 3)]).any()
    assert np.isfinite(want["odd"][6::8]).all() and np.isfinite(want["row1"][6::8]).all()
    assert np.isfinite(want["row1"][7::8]).all()
    # the inputs tell the documented order from another association, and the members of every pair apart
    with np.errstate(all="ignore"):
        alt = col((r[:, :, 0] + r[:, :, 2]) + (r[:, :, 1] + r[:, :, 3]))
    fin = np.isfinite(want["rowsum4"]) & np.isfinite(alt)
    assert ((want["rowsum4"] != alt) & fin).any(axis=(1, 2)).sum() >= NSETS // 4
    for w in want.values():
        assert (w[0::8, 0:NV - 1:2] != w[0::8, 1:NV:2]).all()
    # sets of zeros only hold -0 sums (every term -0) as well as +0 sums
    z = want["odd"][1::8]
    assert (z == 0).all() and np.signbit(z).any() and (~np.signbit(z)).any()
