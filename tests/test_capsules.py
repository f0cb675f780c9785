"""Capsule collision geometry of the legs (round 6, VERDICT r05 missing #1): the thigh and calf collide as capsules over
their full 0.213 m (thigh r = 12.25 mm, calf r = 8 mm: the narrow half widths of the URDF boxes, go1.urdf:148-153,
176-181), the hip as its capsule (go1.urdf:106-111 per replace_cylinder_with_capsule), the foot as its sphere --
against each other (self-collision, go1_crawling.py:44), the trunk box, and the floor / ceiling heightfields.
Rounds 3-5 carried the thigh and calf as sphere chains (3 x r 12.25 mm and 2 x r 8 mm) that left 46-55 mm holes
between their spheres; a foot or a terrain ridge could pass through a link.

Properties checked here in the f64 oracle (oracle/go1_oracle.c seg_deepest / seg_seg_closest, phys_substep), each
one a case the sphere chains failed (asserted alongside as documentation):
  * the deepest point of a segment against the floor / ceiling triangle meshes is the maximum over the whole segment
    (dense sampling agrees to the comparison quantum);
  * a floor vertex raised under any point of the thigh or calf -- the middle of the calf between the old spheres
    included -- meets a force on that link (the sphere chain missed the vertex under the middle of the calf);
  * a foot overlapping another leg's thigh or calf capsule anywhere meets a force on both bodies.
The GPU kernel (go1_contact.h seg_deepest / go1_selfcol.h self_narrow) is checked against the same oracle in
tests/test_gpu_self_collision.py and tests/test_gpu_parity.py.
"""
import numpy as np
import pytest

from legged_tracking_amd import config as CF, layout as L, model as M
from oracle import oracle as O
from tests.mesh_ref import HS, _gap, _mesh
from tests.self_geom import capsules, leg_capsules, seg_dist

G0 = np.zeros(3)
STAND = np.array([0.1, 0.8, -1.5, -0.1, 0.8, -1.5, 0.1, 1.0, -1.5, -0.1, 1.0, -1.5])


def test_seg_deepest_is_the_mesh_maximum():
    """Random rough tiles (floor and ceiling), random segments up to 0.25 m in every direction: the gap at the chosen
    point equals the densely sampled maximum along the segment (over the triangle meshes) to within the comparison
    quantum (1e-5 m)."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for k in range(400):
        tile = np.empty((2, 16, 16), np.float32)
        tile[1] = rng.uniform(0.0, 0.08, (16, 16))
        tile[0] = rng.uniform(0.22, 0.30, (16, 16))
        A = np.array([rng.uniform(0.2, 0.55), rng.uniform(0.2, 0.55), rng.uniform(0.05, 0.25)])
        d = rng.normal(size=3)
        B = A + d / np.linalg.norm(d) * rng.uniform(0.0, 0.25)
        if k % 10 == 0:
            B[:2] = A[:2]  # vertical segment
        r = 0.01
        t = O.seg_deepest(tile, HS, A, B, r)
        ts = np.linspace(0.0, 1.0, 4001)
        dense = _gap(tile, A + ts[:, None] * (B - A), r).max()
        got = _gap(tile, A + t * (B - A), r)
        worst = max(worst, dense - got)
        assert got >= dense - 1.2e-5, (k, got, dense)
    print(f"\nworst shortfall against 4001 samples: {worst:.2e} m")


def test_seg_deepest_ties_and_plane_cases():
    """A segment level over a flat floor ties everywhere: the first end (t = 0; the halves of the thigh and calf are
    walked from their outer ends, so a link lying flat is carried at both ends); tilted, the lower end."""
    tile = np.empty((2, 16, 16), np.float32)
    tile[1], tile[0] = 0.0, 1.0
    A, B = np.array([0.31, 0.42, 0.05]), np.array([0.47, 0.33, 0.05])
    assert O.seg_deepest(tile, HS, A, B, 0.01) == 0.0
    assert O.seg_deepest(tile, HS, A, B + [0, 0, -0.01], 0.01) == 1.0
    # a ceiling lower than the floor is close: the ceiling's deepest point wins
    tile[0] = 0.06
    assert O.seg_deepest(tile, HS, A + [0, 0, 0.02], B, 0.01) == 0.0


def _cfg():
    cfg = CF.readme_config(n_envs=16, terrain="single_path", rows=2, cols=4)
    cfg.env.camera_zero = False
    return CF.build_abi_config(cfg)


def _flat_tile(c, floor=-1.0, ceil=2.0):
    t = np.empty((2, c.hf_nx, c.hf_ny), np.float32)
    t[1], t[0] = floor, ceil
    return t


def _link_point(leg, kind, t, q=STAND):
    """trunk-frame point at parameter t of leg's thigh (kind 0) or calf (kind 2) capsule axis"""
    P, r = leg_capsules(*(np.array([q[3 * leg + j]]) for j in range(3)), l=leg)
    return P[0, kind, 0] + t * (P[0, kind, 1] - P[0, kind, 0]), r[kind]


def _old_chain_gap(tile, pos, leg, kind, q):
    """largest floor gap of the round-3..5 sphere chain of the link (thigh 71/142/213 mm, calf 71/142 mm)"""
    zs = (0.071, 0.142, 0.213) if kind == 0 else (0.071, 0.142)
    r = M.THIGH_BOX_HALF_WIDTH if kind == 0 else M.CALF_BOX_HALF_WIDTH
    g = []
    for z in zs:
        p, _ = _link_point(leg, kind, z / 0.213, q)
        w = pos + p
        g.append(_mesh(tile, 1, w[0], w[1]) + r - w[2])
    return max(g)


@pytest.mark.parametrize("kind", [0, 2], ids=["thigh", "calf"])
def test_floor_vertex_under_any_point_of_a_link_meets_a_force(kind):
    """The link held level (FL thigh horizontal with the calf hanging from the knee, or the thigh down and the calf
    horizontal), a floor vertex raised 3 cm above its neighbours and 2 mm into the capsule right under the link's axis
    at t (15 points from the joint to the link's end): the link reports an upward contact force every time.  The
    sphere chain of rounds 3-5 missed the vertex between its spheres (asserted as documentation)."""
    c = _cfg()
    body_idx = 1 + 4 * 0 + (1 if kind == 0 else 2)  # FL thigh / calf in the 17-body layout
    q = STAND.copy()
    q[0:3] = [0.0, np.pi / 2, -np.pi / 2] if kind == 0 else [0.0, 0.0, -np.pi / 2]
    i0, j0 = 40, 20
    missed_by_chain = 0
    for t in np.linspace(0.03, 0.97, 15):
        p, r = _link_point(0, kind, t, q)
        pos = np.array([i0 * HS, j0 * HS, 0.0]) - np.array([p[0], p[1], 0.0]) + [0.0, 0.0, 0.6]
        tile = _flat_tile(c)
        zc = pos[2] + p[2]
        tile[1, i0 - 1:i0 + 2, j0 - 1:j0 + 2] = zc - r + 0.002 - 0.03  # a 3 cm vertex on a one-cell plateau
        tile[1, i0, j0] = zc - r + 0.002
        b = dict(pos=pos, quat=[0.0, 0.0, 0.0, 1.0], v=[0.0] * 3, w=[0.0] * 3, q=q.copy(), qd=np.zeros(12))
        cf = O.physics(c, b, np.zeros(12), 1, 0.005, G0, 1.0, 0.0, 0.0, tile=tile)
        assert cf[body_idx, 2] > 10.0, (t, cf[body_idx])
        missed_by_chain += _old_chain_gap(tile, pos, 0, kind, q) <= 0.0
    print(f"\nvertex positions the sphere chain would have missed: {missed_by_chain} of 15")
    assert missed_by_chain >= 5


def _old_spheres(q):
    """the round-3..5 sphere chains: (n, 4, 6, 3) thigh x3, calf x2, foot per leg, radii (6,)"""
    out = []
    for l in range(4):
        P, _ = leg_capsules(q[:, 3 * l], q[:, 3 * l + 1], q[:, 3 * l + 2], l)
        th, ca = P[:, 0], P[:, 2]
        pts = [th[:, 0] + f * (th[:, 1] - th[:, 0]) for f in (1 / 3, 2 / 3, 1.0)]
        pts += [ca[:, 0] + f * (ca[:, 1] - ca[:, 0]) for f in (1 / 3, 2 / 3)]
        pts.append(ca[:, 1])
        out.append(np.stack(pts, 1))
    r = np.array([M.THIGH_BOX_HALF_WIDTH] * 3 + [M.CALF_BOX_HALF_WIDTH] * 2 + [M.FOOT_RADIUS])
    return np.stack(out, 1), r


def test_foot_overlapping_another_legs_thigh_or_calf_meets_a_force():
    """Poses with the hips turned inward (feet and knees under the trunk): wherever a foot overlaps another leg's
    thigh or calf capsule by more than 1 mm, both bodies report a contact force.  Among these poses, some overlap
    only where the sphere chains had holes (asserted as documentation)."""
    c = CF.build_abi_config(_plane_cfg())
    rng = np.random.default_rng(17)
    lim = np.array([L.JOINT_LIMITS[j % 3] for j in range(12)])
    n = 40000
    q = rng.uniform(lim[:, 0], lim[:, 1], (n, 12))
    sgn = np.array([-1.0, 1.0, -1.0, 1.0])
    for l in range(4):
        q[:, 3 * l] = sgn[l] * rng.uniform(0.2, 0.8, n)
    P, r = capsules(q)
    S, rs = _old_spheres(q)
    cases = []
    for la in range(4):
        for lb in range(4):
            if la == lb:
                continue
            for kind in (0, 2):
                F, A = P[:, 4 * la + 3], P[:, 4 * lb + kind]
                depth = r[3] + r[kind] - seg_dist(F[:, 0], F[:, 1], A[:, 0], A[:, 1])
                chain = [S[:, la, 5] - S[:, lb, s] for s in ((0, 1, 2) if kind == 0 else (3, 4))]
                chain_hit = np.any([np.linalg.norm(d, axis=1) < rs[5] + rs[3 if kind == 2 else 0] for d in chain], 0)
                for i in np.nonzero(depth > 1e-3)[0][:6]:
                    cases.append((i, la, lb, kind, bool(chain_hit[i])))
    assert len(cases) >= 20, len(cases)
    for i, la, lb, kind, _ in cases:
        b = dict(pos=[0.0, 0.0, 2.0], quat=[0.0, 0.0, 0.0, 1.0], v=[0.0] * 3, w=[0.0] * 3, q=q[i].copy(),
                 qd=np.zeros(12))
        cf = O.physics(c, b, np.zeros(12), 1, 0.005, G0, 1.0, 0.0, 0.0)
        foot, link = 1 + 4 * la + 3, 1 + 4 * lb + (1 if kind == 0 else 2)
        assert np.linalg.norm(cf[foot]) > 0.1, (i, la, lb, kind)
        assert np.linalg.norm(cf[link]) > 0.1, (i, la, lb, kind)
        np.testing.assert_allclose(cf.sum(0), 0.0, atol=1e-8)
    holes = sum(not h for *_, h in cases)
    print(f"\nfoot-link overlaps checked: {len(cases)}; in a sphere-chain hole: {holes}")
    assert holes >= 3


def _plane_cfg():
    cfg = CF.readme_config(n_envs=16, terrain="plane", rows=2, cols=4)
    cfg.env.camera_zero = False
    return cfg


def test_segment_closest_points():
    """seg_seg_closest against a dense search on random segment pairs (points and parallel pairs included)."""
    rng = np.random.default_rng(5)
    ts = np.linspace(0, 1, 401)
    for k in range(300):
        P0, P1, Q0, Q1 = (rng.normal(size=3) for _ in range(4))
        if k % 7 == 0:
            P1 = P0.copy()
        if k % 11 == 0:
            Q1 = Q0 + (P1 - P0) * 0.5
        s, t = O.seg_closest(P0, P1, Q0, Q1)
        d = np.linalg.norm((P0 + s * (P1 - P0)) - (Q0 + t * (Q1 - Q0)))
        A = P0 + ts[:, None] * (P1 - P0)
        B = Q0 + ts[:, None] * (Q1 - Q0)
        dense = np.sqrt(((A[:, None] - B[None]) ** 2).sum(-1)).min()
        assert d <= dense + 1e-9 and d >= dense - 0.01, (k, d, dense)
