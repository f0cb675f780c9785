"""f64 numpy ray caster of the collision scene: the checker of the HIP ray caster (include/go1_render.h).

TEST INFRASTRUCTURE ONLY; shares no code with the kernel.  The robot's primitives come from tests/self_geom.capsules
(the geometry the self-collision tests use) and the root transform; the terrain is traced as world-space triangles
(Moeller-Trumbore) over the cells of the ray's footprint, marched along the ray's major axis; the camera and the
shading restate the header.

A *stable pixel* is one whose five traces -- through the pixel centre and through the four points (+-0.05, +-0.05) px
from it -- agree: same prim id, depths within 1e-3 (1 + t), colours within 2 LSB.  Silhouettes, grazing hits,
grid-line edges and triangle seams, where an f32 and an f64 tracer may legitimately differ, fall out by themselves."""
import numpy as np

from legged_tracking_amd import model as M
from tests import self_geom as SG

PRIM_TRUNK, PRIM_FLOOR, PRIM_CEILING, PRIM_MARKER, PRIM_BACKGROUND = 16, 17, 18, 19, -1
# trunk, hip, thigh, calf, foot, floor, ceiling, marker, background
COLOURS = np.array([[200, 60, 60], [240, 160, 40], [60, 160, 220], [80, 200, 120], [240, 240, 80], [170, 170, 170],
                    [110, 110, 140], [230, 50, 230], [135, 180, 235]], np.float64)
CLASS_OF_K = (2, 1, 3, 4)  # primitive k of a leg: thigh, hip, calf, foot
OFFSETS = ((0.0, 0.0), (0.05, 0.05), (0.05, -0.05), (-0.05, 0.05), (-0.05, -0.05))
EPS = 1e-9


def quat_R(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def robot(root, q):
    """World-frame segment ends (16, 2, 3), radii (16,), and the trunk box (centre, R, half extents)."""
    root, q = np.asarray(root, np.float64), np.asarray(q, np.float64)
    P, r = SG.capsules(q[None])
    R = quat_R(root[3:7])
    return root[:3] + P[0] @ R.T, r, (root[:3], R, np.array(M.TRUNK_BOX) / 2)


def camera(mode, root=None, pos=None, look_at=None):
    """(pos, f, right, up') of a view."""
    if mode == 0:
        pos, look_at = (root[0] - 0.495, root[1], 0.35), (root[0], root[1], 0.25)
    elif mode == 1:
        pos, look_at = (root[0], root[1] - 1.0, root[2] + 1.0), (root[0], root[1], root[2])
    pos, look_at = np.asarray(pos, np.float64), np.asarray(look_at, np.float64)
    f = look_at - pos
    f = f / np.linalg.norm(f)
    up = np.array([1.0, 0, 0]) if abs(f[0]) < 1e-6 and abs(f[1]) < 1e-6 else np.array([0, 0, 1.0])
    right = np.cross(f, up)
    right /= np.linalg.norm(right)
    return pos, f, right, np.cross(right, f)


def rays(cam, W, H, off=(0.0, 0.0)):
    """Unit directions (H * W, 3) through (col + 0.5 + off[0], row + 0.5 + off[1])."""
    _, f, right, up = cam
    col, row = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    sx = 2 * (col + 0.5 + off[0]) / W - 1
    sy = (1 - 2 * (row + 0.5 + off[1]) / H) * (H / W)
    d = f + sx[..., None] * right + sy[..., None] * up
    d = d.reshape(-1, 3)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _first(lo, hi):
    """First positive end of the interval [lo, hi] of a two-sided convex solid (inf: none)."""
    ok = lo <= hi
    t = np.where(lo > 0, lo, hi)
    return np.where(ok & (t > 0), t, np.inf)


def _sphere_span(o, d, c, r):
    oc = o - c
    b = d @ oc
    disc = b * b - (oc @ oc - r * r)
    s = np.sqrt(np.maximum(disc, 0))
    return np.where(disc >= 0, -b - s, np.inf), np.where(disc >= 0, -b + s, -np.inf)


def sphere_hit(o, d, c, r):
    """t (inf: none) and |n . d| of rays o + t d (d (N, 3)) with a sphere."""
    t = _first(*_sphere_span(o, d, c, r))
    tt = np.where(np.isfinite(t), t, 0.0)
    n = (o + tt[:, None] * d - c) / r
    return t, np.abs((n * d).sum(1))


def seg_point_dist(P, a, b):
    ab = b - a
    L2 = ab @ ab
    s = np.clip(((P - a) @ ab) / L2, 0, 1) if L2 > 0 else np.zeros(P.shape[0])
    Q = a + s[:, None] * ab
    return np.linalg.norm(P - Q, axis=1), Q


def capsule_hit(o, d, a, b, r):
    """t and |n . d| with the capsule a -> b (a == b: a sphere).  A capsule is convex: the ray meets it in the
    interval spanned by its end spheres and the cylinder between the end planes."""
    L = np.linalg.norm(b - a)
    lo, hi = _sphere_span(o, d, a, r)
    if L > 0:
        l2, h2 = _sphere_span(o, d, b, r)
        lo, hi = np.minimum(lo, l2), np.maximum(hi, h2)
        u = (b - a) / L
        oc = o - a
        ocu, du = oc @ u, d @ u
        op, dp = oc - ocu * u, d - du[:, None] * u
        A, B, Cc = (dp * dp).sum(1), dp @ op, op @ op - r * r
        with np.errstate(divide="ignore", invalid="ignore"):
            disc = B * B - A * Cc
            s = np.sqrt(np.maximum(disc, 0))
            par = A < 1e-24
            c0 = np.where(par, -np.inf, (-B - s) / np.where(par, 1, A))
            c1 = np.where(par, np.inf, (-B + s) / np.where(par, 1, A))
            ok = np.where(par, Cc <= 0, disc >= 0)
            flat = np.abs(du) < 1e-24
            s0, s1 = (0 - ocu) / np.where(flat, 1, du), (L - ocu) / np.where(flat, 1, du)
            smin = np.where(flat, -np.inf, np.minimum(s0, s1))
            smax = np.where(flat, np.inf, np.maximum(s0, s1))
            ok &= ~(flat & ((ocu < 0) | (ocu > L)))
        c0, c1 = np.maximum(c0, smin), np.minimum(c1, smax)
        ok &= c0 <= c1
        lo, hi = np.where(ok, np.minimum(lo, c0), lo), np.where(ok, np.maximum(hi, c1), hi)
    t = _first(lo, hi)
    tt = np.where(np.isfinite(t), t, 0.0)
    P = o + tt[:, None] * d
    _, Q = seg_point_dist(P, a, b)
    n = (P - Q) / r
    return t, np.abs((n * d).sum(1))


def box_hit(o, d, centre, R, half):
    """t and |n . d| with the box (two-sided): slabs in the box frame."""
    ob, db = (o - centre) @ R, d @ R
    lo, hi = np.full(d.shape[0], -np.inf), np.full(d.shape[0], np.inf)
    nlo, nhi = np.zeros(d.shape[0]), np.zeros(d.shape[0])
    miss = np.zeros(d.shape[0], bool)
    for i in range(3):
        flat = np.abs(db[:, i]) < 1e-24
        den = np.where(flat, 1, db[:, i])
        t1, t2 = (-half[i] - ob[i]) / den, (half[i] - ob[i]) / den
        tn = np.where(flat, -np.inf, np.minimum(t1, t2))
        tf = np.where(flat, np.inf, np.maximum(t1, t2))
        miss |= flat & (abs(ob[i]) > half[i])
        nlo = np.where(tn > lo, np.abs(db[:, i]), nlo)
        lo = np.maximum(lo, tn)
        nhi = np.where(tf < hi, np.abs(db[:, i]), nhi)
        hi = np.minimum(hi, tf)
    t = np.where(miss, np.inf, _first(lo, hi))
    return t, np.where(lo > 0, nlo, nhi)


def _tri(o, d, V0, V1, V2):
    """Moeller-Trumbore, two-sided: t (inf: none) and |n . d| of ray k with triangle k."""
    e1, e2 = V1 - V0, V2 - V0
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = o - V0
        bu = (tv * pv).sum(1) * inv
        qv = np.cross(tv, e1)
        bv = (d * qv).sum(1) * inv
        t = (e2 * qv).sum(1) * inv
    ok = (np.abs(det) > 1e-300) & (bu >= -EPS) & (bv >= -EPS) & (bu + bv <= 1 + EPS) & (t > 0)
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ok, t, np.inf), np.abs((n * d).sum(1))


def _cells(o, d, tile, ox, oy, hs, ci, cj, layers):
    """Nearest hit of ray k in cell (ci[k], cj[k]): t, |n . d|, layer."""
    N = d.shape[0]
    bt, bs, bl = np.full(N, np.inf), np.zeros(N), np.full(N, -1)
    x0, y0 = ox + ci * hs, oy + cj * hs
    for layer in layers:
        h = tile[layer]

        def vert(di, dj):
            return np.stack([x0 + di * hs, y0 + dj * hs, h[ci + di, cj + dj].astype(np.float64)], 1)
        v00, v10, v01, v11 = vert(0, 0), vert(1, 0), vert(0, 1), vert(1, 1)
        for tri in ((v00, v10, v11), (v00, v11, v01)):
            t, s = _tri(o, d, *tri)
            c = t < bt
            bt, bs, bl = np.where(c, t, bt), np.where(c, s, bs), np.where(c, layer, bl)
    return bt, bs, bl


def terrain_hit(o, d, tile, ox, oy, hs, ceiling=True):
    """t, |n . d| and layer (-1: none) of the rays' first hit with the tile's two triangle meshes.  The rays are
    marched along their major axis: column by column (row by row), every cell the ray's footprint touches in that
    column is tested; a hit in a column ends the ray, since the columns are visited in the order of t."""
    N = d.shape[0]
    bt, bs, bl = np.full(N, np.inf), np.zeros(N), np.full(N, -1)
    n = (tile.shape[1], tile.shape[2])
    layers = (1, 0) if ceiling else (1,)
    o2, org = np.array([o[0], o[1]]), np.array([ox, oy])
    g0 = (o2 - org) / hs                      # ray origin in grid units
    gd = d[:, :2] / hs
    # the part of the ray over the vertex grid
    t0, t1 = np.zeros(N), np.full(N, np.inf)
    miss = np.zeros(N, bool)
    for ax in range(2):
        flat = np.abs(gd[:, ax]) < 1e-15
        den = np.where(flat, 1, gd[:, ax])
        ta, tb = (0 - g0[ax]) / den, (n[ax] - 1 - g0[ax]) / den
        t0 = np.where(flat, t0, np.maximum(t0, np.minimum(ta, tb)))
        t1 = np.where(flat, t1, np.minimum(t1, np.maximum(ta, tb)))
        miss |= flat & ((g0[ax] < 0) | (g0[ax] > n[ax] - 1))
    live = ~miss & (t0 <= t1)
    # a cell's triangles lie between the lowest and the highest of its four vertices: cells whose height range
    # the ray's z range over the column does not touch are skipped (exact; it only saves triangle tests)
    hh = np.asarray(tile, np.float64)
    quad = np.stack([hh[:, :-1, :-1], hh[:, 1:, :-1], hh[:, :-1, 1:], hh[:, 1:, 1:]])
    cmin, cmax = quad.min(0)[list(layers)].min(0) - 1e-9, quad.max(0)[list(layers)].max(0) + 1e-9
    if len(layers) == 2:  # between the floor's top and the ceiling's bottom there is nothing either
        gap_lo, gap_hi = quad.max(0)[1] + 1e-9, quad.min(0)[0] - 1e-9
    else:
        gap_lo = gap_hi = None
    major =(np.abs(gd[:, 1]) > np.abs(gd[:, 0])).astype(int)
    for ma in range(2):
        mi = 1 - ma
        idx = np.nonzero(live & (major == ma))[0]
        if idx.size == 0:
            continue
        dm, dn = gd[idx, ma], gd[idx, mi]
        still = np.abs(dm) < 1e-15             # straight down / up: one cell
        sgn = np.where(dm >= 0, 1, -1)
        start = np.clip(np.floor(g0[ma] + t0[idx] * dm), 0, n[ma] - 2).astype(int)
        T1 = np.where(np.isfinite(t1[idx]), t1[idx], t0[idx] + 1e6)
        for k in range(n[ma] - 1):
            c = start + k * sgn
            act = (c >= 0) & (c <= n[ma] - 2) & ~np.isfinite(bt[idx]) & ((k == 0) | ~still)
            if not act.any():
                break
            # a ray that is not active now never is again (it has its hit or has left the grid): drop it
            idx, dm, dn, still, sgn, start, T1, c = (x[act] for x in (idx, dm, dn, still, sgn, start, T1, c))
            a_i, ca, dma, dna, st = idx, c, dm, dn, still
            den = np.where(st, 1, dma)
            ta = np.where(st, t0[a_i], np.clip(np.minimum((ca - g0[ma]) / den, (ca + 1 - g0[ma]) / den), t0[a_i], T1))
            tb = np.where(st, T1, np.clip(np.maximum((ca - g0[ma]) / den, (ca + 1 - g0[ma]) / den), t0[a_i], T1))
            va, vb = g0[mi] + ta * dna, g0[mi] + tb * dna
            jlo = np.clip(np.floor(np.minimum(va, vb) - 1e-7), 0, n[mi] - 2).astype(int)
            jhi = np.clip(np.floor(np.maximum(va, vb) + 1e-7), 0, n[mi] - 2).astype(int)
            za, zb = o[2] + ta * d[a_i, 2], o[2] + tb * d[a_i, 2]
            zlo, zhi = np.minimum(za, zb) - 1e-6, np.maximum(za, zb) + 1e-6
            for jj in range(int((jhi - jlo).max()) + 1):
                cm = np.minimum(jlo + jj, jhi)
                ci, cj = (ca, cm) if ma == 0 else (cm, ca)
                use = (jlo + jj <= jhi) & (zhi >= cmin[ci, cj]) & (zlo <= cmax[ci, cj])
                if gap_lo is not None:
                    use &= ~((zlo > gap_lo[ci, cj]) & (zhi < gap_hi[ci, cj]))
                if not use.any():
                    continue
                u_i = a_i[use]
                ci, cj = ci[use], cj[use]
                t, s, l = _cells(o, d[u_i], tile, ox, oy, hs, ci, cj, layers)
                better = t < bt[u_i]
                bt[u_i] = np.where(better, t, bt[u_i])
                bs[u_i] = np.where(better, s, bs[u_i])
                bl[u_i] = np.where(better, l, bl[u_i])
    return bt, bs, bl


def trace(scene, o, d):
    """First hit of the rays o + t d: depth (inf: background), prim id, rgb (N, 3) float (before rounding).
    scene: dict(root, q, tile=None or (2, nx, ny), origin=(ox, oy), hs, ceiling=True, markers=[(x, y, z, r)])."""
    N = d.shape[0]
    bt, bs, bp = np.full(N, np.inf), np.ones(N), np.full(N, PRIM_BACKGROUND)

    def take(t, s, prim):
        nonlocal bt, bs, bp
        c = t < bt
        bt, bs, bp = np.where(c, t, bt), np.where(c, s, bs), np.where(c, prim, bp)

    seg, rad, (bc, bR, bh) = robot(scene["root"], scene["q"])
    for k in range(16):
        if k % 4 == 3:
            take(*sphere_hit(o, d, seg[k, 0], rad[k]), k)
        else:
            take(*capsule_hit(o, d, seg[k, 0], seg[k, 1], rad[k]), k)
    take(*box_hit(o, d, bc, bR, bh), PRIM_TRUNK)
    for m in scene.get("markers", ()):
        take(*sphere_hit(o, d, np.asarray(m[:3], np.float64), float(m[3])), PRIM_MARKER)
    hs = float(scene["hs"])
    tile = scene.get("tile")
    if tile is None:
        with np.errstate(divide="ignore"):
            t = -o[2] / d[:, 2]
        t = np.where(t > 0, t, np.inf)
        take(t, np.abs(d[:, 2]), PRIM_FLOOR)
        ox = oy = 0.0
    else:
        ox, oy = (float(v) for v in scene["origin"][:2])
        t, s, l = terrain_hit(o, d, np.asarray(tile), ox, oy, hs, scene.get("ceiling", True))
        take(t, s, np.where(l == 1, PRIM_FLOOR, PRIM_CEILING))
    cls = np.full(N, 8)
    leg = (bp >= 0) & (bp < 16)
    cls[leg] = np.array(CLASS_OF_K)[bp[leg] % 4]
    for prim, c in ((PRIM_TRUNK, 0), (PRIM_FLOOR, 5), (PRIM_CEILING, 6), (PRIM_MARKER, 7)):
        cls[bp == prim] = c
    shade = np.where(bp < 0, 1.0, 0.25 + 0.75 * np.minimum(bs, 1.0))
    ter = (bp == PRIM_FLOOR) | (bp == PRIM_CEILING)
    tt = np.where(np.isfinite(bt), bt, 0.0)
    P = o + tt[:, None] * d
    u, v = (P[:, 0] - ox) / hs, (P[:, 1] - oy) / hs
    line = ter & (((u - np.floor(u)) < 0.04) | ((v - np.floor(v)) < 0.04))
    shade = np.where(line, shade * 0.8, shade)
    return bt, bp, COLOURS[cls] * shade[:, None]


def to_u8(rgb):
    return np.minimum(np.floor(rgb + 0.5), 255).astype(np.int64)


def view_camera(scene, view):
    """camera() of a view record (mode, pos, look_at) on the scene's root."""
    mode = view[0]
    return camera(mode, np.asarray(scene["root"], np.float64), *(view[1:3] if mode == 2 else ()))


def render(scene, view, W, H):
    """The checker's picture of one view: dict(depth (H, W), prim (H, W), rgb (H, W, 3) int, stable (H, W) bool,
    cam, dirs (H, W, 3))."""
    cam = view_camera(scene, view)
    o = cam[0]
    n = W * H
    t, p, c = trace(scene, o, np.concatenate([rays(cam, W, H, off) for off in OFFSETS]))  # one batch of 5 n rays
    res = [(t[i * n:(i + 1) * n], p[i * n:(i + 1) * n], c[i * n:(i + 1) * n]) for i in range(len(OFFSETS))]
    t0, p0, c0 = res[0]
    c0 = to_u8(c0)
    stable = np.ones(W * H, bool)
    for t, p, c in res[1:]:
        same_t = np.where(np.isfinite(t0) | np.isfinite(t), np.abs(np.where(np.isfinite(t), t, 1e300) -
                                                                   np.where(np.isfinite(t0), t0, 1e300))
                          <= 1e-3 * (1 + np.where(np.isfinite(t0), t0, 0.0)), True)
        stable &= (p == p0) & same_t & (np.abs(to_u8(c) - c0).max(1) <= 2)
    return dict(depth=t0.reshape(H, W), prim=p0.reshape(H, W), rgb=c0.reshape(H, W, 3), stable=stable.reshape(H, W),
                cam=cam, dirs=rays(cam, W, H).reshape(H, W, 3))
