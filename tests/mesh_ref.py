"""float64 reference of the heightfield's triangle mesh, shared by tests/test_capsules.py and
tests/test_gpu_device_geometry.py."""
import numpy as np

HS = 0.05


def _mesh(tile, layer, x, y, hs=HS):
    """height of the heightfield's triangle mesh (cells split along the (i, j) - (i + 1, j + 1) diagonal, as isaacgym
    terrain_utils.convert_heightfield_to_trimesh builds the reference's terrain) at world (x, y)"""
    nx, ny = tile.shape[1:]
    u = np.clip(x / hs, -4.0, nx + 4.0)
    v = np.clip(y / hs, -4.0, ny + 4.0)
    i, j = np.floor(u).astype(int), np.floor(v).astype(int)
    a, b = u - i, v - j
    at = lambda ii, jj: tile[layer, np.clip(ii, 0, nx - 1), np.clip(jj, 0, ny - 1)].astype(np.float64)  # noqa: E731
    lower = at(i, j) + a * (at(i + 1, j) - at(i, j)) + b * (at(i + 1, j + 1) - at(i + 1, j))
    upper = at(i, j) + b * (at(i, j + 1) - at(i, j)) + a * (at(i + 1, j + 1) - at(i, j + 1))
    return np.where(a >= b, lower, upper)


def _gap(tile, P, r):
    """max over the layers of the vertical gap at points P (..., 3): floor h + r - z, ceiling z + r - h"""
    f = _mesh(tile, 1, P[..., 0], P[..., 1]) + r - P[..., 2]
    c = P[..., 2] + r - _mesh(tile, 0, P[..., 0], P[..., 1])
    return np.maximum(f, c)
