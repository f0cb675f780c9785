"""The self-collision work list is conservative (CPU; go1_selfcol.h self_broad / self_narrow restated in numpy).

The step kernel evaluates a primitive pair only if it is on the lane's work list:
  * cross-leg pairs: the two legs' trunk-frame boxes overlap (self_broad: the thigh joint, the knee .. foot span grown
    by the largest link radius, the hip capsule grown by its radius) AND the two primitives' world-axis boxes overlap
    (self_narrow: the segment's ends grown by its radius);
  * same-leg pairs (hip - calf, hip - foot, thigh - foot): the leg has a joint more than 0.1 rad past its URDF range
    AND the primitives' world-axis boxes overlap.
A pair that is not on the list gets no force, so every pair closer than the sum of its radii must be on it.  Checked
over random joint states within the limits and up to 1.2 rad past them, the trunk at a random pose (the primitive
boxes are world-axis boxes), in f32 as the kernel computes them; the distances come from tests/self_geom.py in f64.
"""
import numpy as np

from legged_tracking_amd import layout as L
from tests.self_geom import SAME, capsules, seg_dist

BAND = 0.1  # rad past the URDF range before the same-leg pairs are tested (self_broad `wild`)


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def leg_boxes(P, r):
    """self_broad: (n, 4, 3) lower and upper corners of the legs' boxes in the trunk frame (f32)."""
    P = P.astype(np.float32)
    r = r.astype(np.float32)
    rmax = max(r[0], r[2], r[3])
    lo, hi = [], []
    for l in range(4):
        th, kn, ft = P[:, 4 * l, 0], P[:, 4 * l, 1], P[:, 4 * l + 3, 0]
        h0, h1 = P[:, 4 * l + 1, 0], P[:, 4 * l + 1, 1]
        clo, chi = np.minimum(kn, ft) - rmax, np.maximum(kn, ft) + rmax
        tlo, thi = np.minimum(th, clo), np.maximum(th, chi)
        hlo, hhi = np.minimum(h0, h1) - r[1], np.maximum(h0, h1) + r[1]
        lo.append(np.minimum(tlo, hlo))
        hi.append(np.maximum(thi, hhi))
    return np.stack(lo, 1), np.stack(hi, 1)


def prim_boxes(Pw, r):
    """self_narrow: (n, 16, 3) corners of the primitives' world-axis boxes (f32)."""
    Pw = Pw.astype(np.float32)
    rr = r.astype(np.float32)[None, :, None]
    return np.minimum(Pw[:, :, 0], Pw[:, :, 1]) - rr, np.maximum(Pw[:, :, 0], Pw[:, :, 1]) + rr


def overlap(alo, ahi, blo, bhi):
    return ((alo <= bhi) & (blo <= ahi)).all(-1)


def wild_legs(q):
    """self_broad: (n, 4) the leg has a joint more than BAND past its range."""
    lim = np.array(L.JOINT_LIMITS)
    q3 = q.reshape(-1, 4, 3).astype(np.float32)
    lo, hi = (lim[:, 0] - BAND).astype(np.float32), (lim[:, 1] + BAND).astype(np.float32)
    return ((q3 < lo) | (q3 > hi)).any(-1)


def work_list(q, R, pos):
    """(n, 16, 16) symmetric: pair (i, j) is on the work list of the lanes of primitives i and j."""
    P, r = capsules(q)
    Pw = np.einsum("nij,npej->npei", R, P) + pos[:, None, None, :]
    llo, lhi = leg_boxes(P, r)
    plo, phi = prim_boxes(Pw, r)
    wild = wild_legs(q)
    n = len(q)
    on = np.zeros((n, 16, 16), bool)
    for i in range(16):
        for j in range(16):
            la, lb = i // 4, j // 4
            box = overlap(plo[:, i], phi[:, i], plo[:, j], phi[:, j])
            if la != lb:
                on[:, i, j] = overlap(llo[:, la], lhi[:, la], llo[:, lb], lhi[:, lb]) & box
            elif (i % 4, j % 4) in SAME or (j % 4, i % 4) in SAME:
                on[:, i, j] = wild[:, la] & box
    return on, P, r


def test_every_touching_pair_is_on_the_work_list():
    rng = np.random.default_rng(7)
    lim = np.array([L.JOINT_LIMITS[j % 3] for j in range(12)])
    n = 8000
    inside = rng.uniform(lim[:, 0], lim[:, 1], (n, 12))
    inward = rng.uniform(lim[:, 0], lim[:, 1], (n, 12))  # hips turned toward the body: knees and feet under the trunk
    sgn = np.array([-1.0, 1.0, -1.0, 1.0])
    for l in range(4):
        inward[:, 3 * l] = sgn[l] * rng.uniform(0.2, 0.8, n)
    past = rng.uniform(lim[:, 0] - 1.2, lim[:, 1] + 1.2, (n, 12))
    q = np.concatenate([inside, inward, past])
    assert len(q) >= 20000
    R = _rotations(rng, len(q))
    pos = rng.uniform(-50.0, 50.0, (len(q), 3))
    on, P, r = work_list(q, R, pos)
    assert (on == on.transpose(0, 2, 1)).all()  # both lanes of a pair list it (equal and opposite forces)
    touching = listed = 0
    for i in range(16):
        for j in range(i + 1, 16):
            la, lb = i // 4, j // 4
            if la == lb and (i % 4, j % 4) not in SAME:
                continue  # adjacent links never collide
            t = seg_dist(P[:, i, 0], P[:, i, 1], P[:, j, 0], P[:, j, 1]) < r[i] + r[j]
            miss = t & ~on[:, i, j]
            assert not miss.any(), (i, j, int(miss.sum()), q[np.nonzero(miss)[0][0]])
            touching += int(t.sum())
            listed += int(on[:, i, j].sum())
    print(f"\n{len(q)} states: {touching} touching pairs, {listed} listed pairs")
    assert touching > 2000  # the property was exercised
    assert listed < 20 * touching  # and the list is a cull, not everything
