"""Segments for the capsule search's short pass (csrc/go1_contact.h seg_deepest<1, 1, 2>, seg_deepest2), shared by
tests/test_seg_short_bound.py and tests/test_gpu_seg_layout.py: the compiled hip-capsule length, the mesh edges a
segment's (x, y) projection crosses as the search counts them, and the laid-out segments that reach each maximum."""
import numpy as np

from legged_tracking_amd import model as M

HS_MIN = float(np.float32(0.0499))  # go1_contact.h SEG_MIN_HS: go1_create refuses finer grids
HALF_LINK = 0.1065                  # a thigh or calf half: the full candidate set's length


def short_len():
    """the hip capsule's length as compiled (go1_contact.h SEG_SHORT_MAX: the f32 model block's difference)"""
    mb = M.model_block().astype(np.float32)
    return float(np.float32(mb[177] - mb[176]))


def crossings(uA, vA, uB, vB):
    """(n_u, n_v, n_d): the lines u = k, v = k and the diagonals u - v = k strictly between the ends (cell units),
    as seg_deepest counts its valid candidates: the integers k with floor(min) + 1 <= k < max"""
    def n(a, b):
        return np.maximum(np.ceil(np.maximum(a, b)) - 1 - np.floor(np.minimum(a, b)), 0).astype(int)
    return n(uA, uB), n(vA, vB), n(uA - vA, uB - vB)


def worst_xy(length, hs, cell=(0, 0)):
    """(A, B), each (6, 2) metres: horizontal segments of `length` laid out to reach the crossing maxima of their
    length on cells of hs, from cell `cell` -- along u and along v from just before a line (the most lines of that
    direction), across the diagonals from just before one, placed so that it crosses the most diagonals and a line
    of either direction as well -- and each of the three reversed."""
    Lc = length / hs
    i0, j0 = cell
    d = Lc / np.sqrt(2.0)
    ew = (np.sqrt(2.0) * Lc - np.floor(np.sqrt(2.0) * Lc)) / 2  # u - v starts this far before a diagonal
    eu = (Lc - np.floor(Lc)) / 2
    uA = (1 - ew) / 2 if d < 1 else 1 - ew / 2
    S = [((1 - eu, 0.4), (1 - eu + Lc, 0.4)),
         ((0.4, 1 - eu), (0.4, 1 - eu + Lc)),
         ((uA, uA + ew), (uA + d, uA + ew - d))]
    S += [(b, a) for a, b in S]
    A = np.array([[a[0] + i0, a[1] + j0] for a, _ in S]) * hs
    B = np.array([[b[0] + i0, b[1] + j0] for _, b in S]) * hs
    return A, B


def random_xy(n, length, hs, rng, lo=0.0, hi=8.0):
    """(A, B), each (n, 2): horizontal segments of `length`, uniform in position and direction"""
    A = rng.uniform(lo, hi, (n, 2)) * hs
    th = rng.uniform(0, 2 * np.pi, n)
    return A, A + length * np.stack([np.cos(th), np.sin(th)], 1)
