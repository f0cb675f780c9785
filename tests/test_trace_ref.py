"""tests/trace_ref.py pinned on a hand-written case with literal expected arrays: n = 2, depth = 3, 7 pushes, with
one episode shorter than the ring, one longer than the ring (its rows wrap) and, at capacity 1, overflow."""
import numpy as np

from tests import trace_ref as TR


def _word(s, e):
    return np.float32(100 * s + 10 * e)


def _run(capacity, want=3):
    ref = TR.TraceRef(2, 3, capacity, traj_words=6, want=want)
    ref.traj_start[:] = TR.bits(np.array([[7.0] * 6, [8.0] * 6], np.float32))
    #          push:  0  1  2  3  4  5  6
    reset = np.array([[0, 0, 1, 0, 0, 0, 1],     # env 0: a 2-row episode (time-out), then a 4-row one (terminated)
                      [0, 0, 0, 0, 0, 1, 0]])    # env 1: a 5-row episode (terminated): pushes 2, 3, 4 are kept
    tout = np.array([[0, 0, 1, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0]])
    for s in range(7):
        root = np.stack([np.full(13, _word(s, e)) for e in range(2)])
        dof = root[:, :12] + np.float32(1)
        traj = np.full((2, 6), np.float32(s))    # the trajectory an episode starts with names its first push
        ref.push(root, dof, reset[:, s], tout[:, s], wp_index=np.array([s, s + 50], np.int32), traj=traj)
    return ref


def _row(s, e):
    w = _word(s, e)
    return TR.bits(np.array([w] * 13 + [w + 1] * 12, np.float32)).tolist() + [s + 50 * e]


def test_capacity_one_keeps_the_short_episode_and_counts_the_overflow():
    ref = _run(1)
    assert ref.counts() == (1, 2) and ref.claimed == 3
    np.testing.assert_array_equal(ref.cap_meta, [[0, 0, 2, 2, 2, TR.TIMEOUT, 0, 0]])
    np.testing.assert_array_equal(ref.cap_rows, [[_row(0, 0), _row(1, 0), [0] * 26]])
    np.testing.assert_array_equal(ref.cap_traj, TR.bits(np.array([[7.0] * 6], np.float32)))
    np.testing.assert_array_equal(ref.ep_start, [6, 5])
    np.testing.assert_array_equal(ref.ep_ordinal, [2, 1])
    np.testing.assert_array_equal(ref.traj_start, TR.bits(np.array([[6.0] * 6, [5.0] * 6], np.float32)))
    # the ring holds pushes 6, 4, 5 in slots 0, 1, 2
    np.testing.assert_array_equal(ref.ring, [[_row(6, 0), _row(6, 1)], [_row(4, 0), _row(4, 1)],
                                             [_row(5, 0), _row(5, 1)]])


def test_the_long_episode_wraps_and_comes_out_oldest_first():
    ref = _run(3)
    assert ref.counts() == (3, 0)
    np.testing.assert_array_equal(ref.cap_meta, [[0, 0, 2, 2, 2, TR.TIMEOUT, 0, 0],
                                                 [1, 0, 5, 3, 5, TR.TERMINATED, 0, 0],
                                                 [0, 1, 6, 3, 4, TR.TERMINATED, 0, 0]])
    np.testing.assert_array_equal(ref.cap_rows[1], [_row(2, 1), _row(3, 1), _row(4, 1)])  # ring slots 2, 0, 1
    np.testing.assert_array_equal(ref.cap_rows[2], [_row(3, 0), _row(4, 0), _row(5, 0)])
    np.testing.assert_array_equal(ref.cap_traj, TR.bits(np.array([[7.0] * 6, [8.0] * 6, [2.0] * 6], np.float32)))
    meta, rows, traj = ref.sorted_captures()
    np.testing.assert_array_equal(meta[:, 2], [2, 5, 6])


def test_want_and_eligible_filter_captures_but_not_the_bookkeeping():
    ref = _run(3, want=TR.TERMINATED)
    assert ref.counts() == (2, 0)
    np.testing.assert_array_equal(ref.cap_meta[:2, :3], [[1, 0, 5], [0, 1, 6]])
    np.testing.assert_array_equal(ref.ep_ordinal, [2, 1])
    masked = TR.TraceRef(2, 3, 3, eligible=[0, 1])
    z13, z12 = np.zeros((2, 13), np.float32), np.zeros((2, 12), np.float32)
    masked.push(z13, z12, [0, 0], [0, 0])
    masked.push(z13, z12, [1, 1], [0, 0])
    assert masked.counts() == (1, 0) and masked.cap_meta[0, 0] == 1
    masked.mark_reset([1])
    np.testing.assert_array_equal(masked.ep_ordinal, [1, 2])
    np.testing.assert_array_equal(masked.ep_start, [1, 2])


def test_bit_patterns_survive():
    odd = np.array([0x7fc00001, 0xffc12345, 0x7f800000, 0xff800000, 0x80000000, 0x7f800001], np.uint32)
    root = np.zeros((1, 13), np.float32)
    root.view(np.uint32)[0, :6] = odd
    ref = TR.TraceRef(1, 2, 1)
    ref.push(root, np.zeros((1, 12), np.float32), [0], [0])
    ref.push(root, np.zeros((1, 12), np.float32), [1], [0])
    np.testing.assert_array_equal(ref.cap_rows[0, 0, :6], odd)
