"""seg_deepest's candidate edges across the border of the LDS patch (csrc/go1_contact.h).

Every line and diagonal candidate of the capsule search reads the two vertices of a mesh edge -- (k, j) - (k, j + 1) on
a line u = k, (i, k) - (i + 1, k) on a line v = k, (i, j) - (i + 1, j + 1) on a diagonal.  Where exactly one of the two
lies inside the patch, one read is served by the patch and the other by the tile (verts_fetch tests every vertex; a
fetch that tests an edge as a pair would read both from the tile).  Either way the patch is a pure cache of the tile:
seg_deepest's t and cell with the patch (mode 0) are, bit for bit, those of the tile-only run (mode 1), which is the
reference.  The segments here are laid over the patch's last and first rows and columns so that candidate edges
straddle each of the four borders, and some lie wholly outside; which ones straddle is computed from the geometry in
float64 and asserted, not assumed.
"""
import numpy as np
import pytest

from tests import devcheck as D

pytestmark = pytest.mark.gpu

HS = float(np.float32(0.05))
PSZX, PSZY = D.PSZX, D.PSZY
NX, NY = 64, 48
# (pi0, pj0): three patches inside the tile, one overhanging two of its edges
ENVS = [(10, 8), (30, 20), (40, 30), (-3, 35)]
NQ = 2  # 4 envs x 2 rounds x 64 lanes = 512 queries
KINDS = ("last row", "last column", "first row", "first column", "outside")


def _segments():
    rng = np.random.default_rng(1152)
    N = len(ENVS) * NQ * 64
    env = np.repeat(np.arange(len(ENVS)), NQ * 64)
    pi0, pj0 = np.array(ENVS)[env, 0], np.array(ENVS)[env, 1]
    kind = rng.integers(0, len(KINDS), N)
    along_u, along_v = pi0 + rng.uniform(0, PSZX, N), pj0 + rng.uniform(0, PSZY, N)
    # the middle of the segment: in the border's row / column of cells, half a cell either side; or 3 .. 5 cells off
    band = rng.uniform(-1.0, 1.0, N)
    u = np.select([kind == 0, kind == 2, kind == 4], [pi0 + PSZX - 0.5 + band, pi0 - 0.5 + band,
                                                      pi0 + PSZX + rng.uniform(3, 5, N)], along_u)
    v = np.select([kind == 1, kind == 3], [pj0 + PSZY - 0.5 + band, pj0 - 0.5 + band], along_v)
    ang = rng.uniform(0, 2 * np.pi, N)
    half = rng.uniform(0.4, 1.05, N)  # cells; a link half spans at most 2.13 (0.1065 m at 0.05 m cells)
    du, dv = half * np.cos(ang), half * np.sin(ang)
    z = rng.uniform(0.05, 0.25, (N, 2))
    A = np.stack([(u - du) * HS, (v - dv) * HS, z[:, 0]], 1).astype(np.float32).astype(np.float64)
    B = np.stack([(u + du) * HS, (v + dv) * HS, z[:, 1]], 1).astype(np.float32).astype(np.float64)
    return env, pi0, pj0, kind, A, B


def _straddling(pi0, pj0, A, B):
    """per query, which borders (last row, last column, first row, first column) a valid candidate edge straddles:
    exactly one of its two vertices lies in the patch.  The candidates are seg_deepest's: the crossings of u = k,
    v = k and u - v = k strictly inside the segment"""
    n = len(A)
    uA, vA, uB, vB = A[:, 0] / HS, A[:, 1] / HS, B[:, 0] / HS, B[:, 1] / HS
    hit = np.zeros((n, 4), bool)
    inside = lambda i, j: (i >= pi0) & (i < pi0 + PSZX) & (j >= pj0) & (j < pj0 + PSZY)  # noqa: E731

    def edges(wA, wB, di, dj, vertex):
        k0 = np.floor(np.minimum(wA, wB)).astype(int) + 1
        for m in range(4):
            k = k0 + m
            valid = k < np.maximum(wA, wB)
            t = np.where(valid, (k - wA) / np.where(wB != wA, wB - wA, 1.0), 0.0)
            i, j = vertex(k, uA + (uB - uA) * t, vA + (vB - vA) * t)
            a, b = inside(i, j), inside(i + di, j + dj)
            one = valid & (a != b)
            far_i, far_j = np.where(a, i + di, i), np.where(a, j + dj, j)  # the vertex outside
            hit[:, 0] |= one & (far_i >= pi0 + PSZX)
            hit[:, 1] |= one & (far_j >= pj0 + PSZY)
            hit[:, 2] |= one & (far_i < pi0)
            hit[:, 3] |= one & (far_j < pj0)

    edges(uA, uB, 0, 1, lambda k, u, v: (k, np.floor(v).astype(int)))
    edges(vA, vB, 1, 0, lambda k, u, v: (np.floor(u).astype(int), k))
    edges(uA - vA, uB - vB, 1, 1, lambda k, u, v: (np.floor(u).astype(int), np.floor(u).astype(int) - k))
    return hit


def test_edge_pairs_across_the_patch_border_equal_the_tile_only_run():
    rng = np.random.default_rng(1153)
    tile = np.empty((2, NX, NY), np.float32)
    tile[1] = rng.uniform(0.0, 0.08, (NX, NY))
    tile[0] = rng.uniform(0.22, 0.30, (NX, NY))
    env, pi0, pj0, kind, A, B = _segments()
    env_i = np.array([[0, NX, NY, p, q] for p, q in ENVS], np.int32)
    r = np.full(len(A), np.float32(0.01))
    out = {m: D.terrain(m, tile.ravel(), env_i, HS, A[:, :2], A, B, r) for m in (0, 1)}
    for key in ("t", "cell", "hqc"):
        x, y = out[0][key], out[1][key]
        assert np.isfinite(x.astype(np.float64)).all()
        bad = np.nonzero((x.view(np.uint32) if x.dtype == np.float32 else x) !=
                         (y.view(np.uint32) if y.dtype == np.float32 else y))[0]
        assert bad.size == 0, (key, bad.size, bad[:5], kind[bad[:5]], env[bad[:5]])
    # the inputs did what they are for: edges with one vertex in the patch, at each of its four borders
    hit = _straddling(pi0, pj0, A, B)
    print("\nstraddling queries:", int(hit.any(1).sum()), "per border:", dict(zip(KINDS, hit.sum(0).tolist())))
    assert hit.any(1).sum() >= 64
    assert (hit.sum(0) >= 16).all(), hit.sum(0)
    # segments wholly outside the patch, with candidates of their own; and the search moved off the segments' ends
    uv = np.stack([A[:, :2], B[:, :2]], 1) / HS
    outside = (uv[:, :, 0] >= (pi0 + PSZX + 1)[:, None]).all(1)
    assert (outside & (kind == 4)).sum() >= 32
    t = out[1]["t"]
    assert ((t > 0) & (t < 1) & hit.any(1)).sum() >= 16
