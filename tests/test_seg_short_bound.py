"""The bound the capsule search's short pass rests on (csrc/go1_contact.h seg_deepest<1, 1, 2>; its static_asserts
state the same from the model constants): a segment of the compiled hip-capsule length on the finest grid go1_create
accepts (hs = 0.0499) never crosses more than 1 line u = k, 1 line v = k and 2 cell diagonals, and each of these
maxima is reached -- by the laid-out segments of tests/seg_cases.py, which tests/test_gpu_seg_layout.py runs through
the kernel, so that the last candidate slot of every kind is exercised there.  Pure numpy, no GPU."""
import numpy as np

from tests import seg_cases as S

N = 200_000


def _counts(A, B, hs):
    A, B = (np.asarray(x, np.float32).astype(np.float64) / hs for x in (A, B))  # the f32 ends the kernel reads
    return S.crossings(A[:, 0], A[:, 1], B[:, 0], B[:, 1])


def _inputs(length):
    rng = np.random.default_rng(12)
    Ar, Br = S.random_xy(N, length, S.HS_MIN, rng)
    Aw, Bw = S.worst_xy(length, S.HS_MIN, cell=(3, 5))
    return np.concatenate([Aw, Ar]), np.concatenate([Bw, Br])


def test_compiled_length_is_the_models():
    assert abs(S.short_len() - 0.04) < 1e-6
    assert S.short_len() / S.HS_MIN < 1 and S.short_len() / S.HS_MIN * np.sqrt(2) < 2  # the header's static_asserts


def test_hip_capsule_crosses_at_most_1_1_2_edges_and_reaches_each():
    A, B = _inputs(S.short_len())
    nu, nv, nd = _counts(A, B, S.HS_MIN)
    print(f"\n{len(A)} segments of {S.short_len():.6f} m at hs {S.HS_MIN}: maxima {nu.max()} / {nv.max()} / {nd.max()}")
    assert nu.max() == 1 and nv.max() == 1 and nd.max() == 2
    # the laid-out cases alone reach every maximum, one of them all three at once
    wu, wv, wd = (c[:6] for c in (nu, nv, nd))
    assert wu.max() == 1 and wv.max() == 1 and wd.max() == 2
    assert ((wu == 1) & (wv == 1) & (wd == 2)).any()


def test_half_link_needs_the_full_set():
    """the counting sees more than 1 / 1 / 2 where there is more: a half link reaches 3 / 3 / 4 and no more"""
    A, B = _inputs(S.HALF_LINK)
    nu, nv, nd = _counts(A, B, S.HS_MIN)
    assert nu.max() == 3 and nv.max() == 3 and nd.max() == 4
    assert nu[:6].max() == 3 and nv[:6].max() == 3 and nd[:6].max() == 4
