"""go1_trace_push on the MI355X against tests/trace_ref.py, on synthetic planes (no env): 40 pushes at depth 5 with a
scripted reset / time_out pattern whose episodes have 1, 3, 5, 6 and 13 rows (shorter than, equal to and longer than
the ring), 16 envs (one partial workgroup) and 48 (two workgroups, the second a partial wave), trajectories of 1 and
10 waypoints and none, every `want`, with and without an `eligible` mask.  The planes hold arbitrary bit patterns --
NaNs with payloads, infinities, -0.0 -- and everything is compared as 32-bit integers."""
import numpy as np
import pytest
import torch

from legged_tracking_amd import trace as T
from tests import trace_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEPTH, PUSHES = 5, 40
LENGTHS = (1, 3, 5, 6, 13)
SPECIAL = np.array([0x7fc00000, 0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0],
                   np.uint32)


def script(n):
    """reset / time_out (PUSHES, n): env e's episodes take LENGTHS in turn, starting at LENGTHS[e % 5], so the envs
    with equal e % 5 end in the same push."""
    reset = np.zeros((PUSHES, n), bool)
    for e in range(n):
        s, k = 0, e % 5
        while True:
            s += LENGTHS[k % 5]
            k += 1
            if s >= PUSHES:
                break
            reset[s, e] = True
    es = np.add.outer(np.arange(PUSHES), np.arange(n))
    time_out = (reset & (es % 2 == 0)) | (~reset & (es % 7 == 0))  # a time_out without a reset ends nothing
    return reset, time_out


def planes(n, tw, seed):
    """Per push: root (n, 13), dof_pos (n, 12), wp_index (n,), trajectory (n, tw) as arbitrary 32-bit words."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(PUSHES):
        words = [rng.integers(0, 2 ** 32, (n, w), dtype=np.uint64).astype(np.uint32) for w in (13, 12, 1, tw)]
        for w in words[:2] + words[3:]:
            hit = rng.random(w.shape) < 0.15
            w[hit] = rng.choice(SPECIAL, int(hit.sum()))
        out.append(words)
    return out


def run(n, wp_length, want, masked, capacity):
    tw = 6 * wp_length if wp_length else 0
    reset, time_out = script(n)
    data = planes(n, tw, seed=n + 7 * tw)
    eligible = (np.arange(n) % 3 != 1) if masked else None
    f32 = lambda w: torch.from_numpy(w.view(np.float32).copy()).to(DEV)  # noqa: E731
    root, dof = f32(data[0][0]), f32(data[0][1])
    wp = torch.from_numpy(data[0][2].view(np.int32).copy()).to(DEV) if wp_length else None
    traj = f32(data[0][3]) if wp_length else None
    buf = T.TraceBuffers(root, dof, DEPTH, capacity, want, None if eligible is None else torch.from_numpy(eligible),
                         trajectory=traj, wp_index=wp)
    refs = [TR.TraceRef(n, DEPTH, c, tw, want, eligible) for c in (capacity, 4096)]
    for ref in refs:
        ref.traj_start[:] = data[0][3]
    for s in range(PUSHES):
        r, d, w, t = data[s]
        root.copy_(f32(r))
        dof.copy_(f32(d))
        if wp_length:
            wp.copy_(torch.from_numpy(w.view(np.int32).copy()))
            traj.copy_(f32(t))
        buf.push(torch.from_numpy(reset[s]).to(DEV), torch.from_numpy(time_out[s]).to(DEV))
        for ref in refs:
            ref.push(r.view(np.float32), d.view(np.float32), reset[s], time_out[s],
                     wp_index=w.view(np.int32)[:, 0] if wp_length else None, traj=t.view(np.float32))
    torch.cuda.synchronize()
    return buf, refs[0], refs[1], reset


def check_state(buf, ref):
    np.testing.assert_array_equal(buf.ring.cpu().numpy().view(np.uint32), ref.ring)
    np.testing.assert_array_equal(buf.ep_start.cpu().numpy(), ref.ep_start)
    np.testing.assert_array_equal(buf.ep_ordinal.cpu().numpy(), ref.ep_ordinal)
    if ref.tw:
        np.testing.assert_array_equal(buf.traj_start.cpu().numpy().view(np.uint32), ref.traj_start)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("want", [1, 2, 3])
@pytest.mark.parametrize("wp_length", [1, 10, None])
@pytest.mark.parametrize("n", [16, 48])
def test_every_capture_equals_the_reference(n, wp_length, want, masked):
    buf, ref, _, reset = run(n, wp_length, want, masked, capacity=int(script(n)[0].sum()))
    assert ref.dropped == 0 and ref.counts()[0] > n // 2
    if want == 3 and not masked:
        assert ref.counts()[0] == reset.sum()
        assert {int(x) for x in ref.cap_meta[:ref.claimed, 3]} == {1, 3, 5}     # rows kept, at depth 5
        assert {int(x) for x in ref.cap_meta[:ref.claimed, 4]} == set(LENGTHS)  # full lengths
    assert buf.counts() == ref.counts()
    meta, rows, traj, _ = buf.captures()
    rmeta, rrows, rtraj = ref.sorted_captures()
    np.testing.assert_array_equal(meta, rmeta)
    np.testing.assert_array_equal(rows.view(np.uint32), rrows)
    np.testing.assert_array_equal(traj.view(np.uint32), rtraj)
    # the slots past the claimed ones are untouched
    assert not buf.cap_rows[ref.claimed:].any() and not buf.cap_meta[ref.claimed:].any()
    check_state(buf, ref)


@pytest.mark.parametrize("n", [16, 48])
def test_overflow_keeps_three_and_counts_the_rest(n):
    buf, ref, full, reset = run(n, 10, 3, False, capacity=3)
    first = reset[np.flatnonzero(reset.any(1))[0]]
    assert first.sum() > 3                                  # more than 3 candidates in the first ending push
    assert buf.counts() == (3, int(reset.sum()) - 3) == ref.counts()
    assert int(buf.cap_count[0]) == reset.sum()             # the raw counter counts past capacity
    meta, rows, traj, _ = buf.captures()
    by_key = {(int(m[0]), int(m[1])): i for i, m in enumerate(full.cap_meta[:full.claimed])}
    assert len({int(m[0]) for m in meta}) == 3 and all(first[int(m[0])] for m in meta)
    for m, r, t in zip(meta, rows, traj):
        i = by_key[int(m[0]), int(m[1])]
        np.testing.assert_array_equal(m, full.cap_meta[i])
        np.testing.assert_array_equal(r.view(np.uint32), full.cap_rows[i])
        np.testing.assert_array_equal(t.view(np.uint32), full.cap_traj[i])
    check_state(buf, ref)


def test_mark_reset_matches_the_reference_and_captures_nothing():
    n = 16
    root = torch.zeros(n, 13, device=DEV)
    dof = torch.zeros(n, 12, device=DEV)
    buf = T.TraceBuffers(root, dof, 4, 8)
    ref = TR.TraceRef(n, 4, 8)
    none = torch.zeros(n, dtype=torch.bool, device=DEV)
    for s in range(6):
        root.fill_(float(s))
        buf.push(none, none)
        ref.push(root.cpu().numpy(), dof.cpu().numpy(), np.zeros(n, bool), np.zeros(n, bool))
        if s == 2:
            buf.mark_reset([3, 7])
            ref.mark_reset([3, 7])
    ends = torch.ones(n, dtype=torch.bool, device=DEV)
    buf.push(ends, none)
    ref.push(root.cpu().numpy(), dof.cpu().numpy(), np.ones(n, bool), np.zeros(n, bool))
    assert buf.counts() == (8, 8)
    check_state(buf, ref)
    meta = buf.captures()[0]
    assert all(int(m[4]) == (3 if int(m[0]) in (3, 7) else 6) and int(m[1]) == (1 if int(m[0]) in (3, 7) else 0)
               for m in meta)
