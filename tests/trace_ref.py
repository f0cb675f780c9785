"""numpy restatement of go1_trace_push (include/go1_trace.h): sequential, ordered by env, so a push that overflows
the capture buffer drops the candidates with the highest env ids (the kernel's choice is unspecified; its count is
not).  Every array holds 32-bit words (rows, trajectories as uint32 bit patterns), so NaN payloads compare."""
import numpy as np

ROW, META = 26, 8
TERMINATED, TIMEOUT = 1, 2


def bits(a):
    """The 32-bit words of a float32 / int32 / uint32 array, as uint32."""
    return np.ascontiguousarray(a).view(np.uint32)


def make_row(root, dof_pos, wp_index=None):
    """(n, 26) uint32 rows of the (n, 13) / (n, 12) f32 planes and the optional (n,) int32 waypoint index."""
    n = root.shape[0]
    row = np.zeros((n, ROW), np.uint32)
    row[:, :13] = bits(np.asarray(root, np.float32))
    row[:, 13:25] = bits(np.asarray(dof_pos, np.float32))
    if wp_index is not None:
        row[:, 25] = bits(np.asarray(wp_index, np.int32).reshape(n))
    return row


class TraceRef:
    def __init__(self, n, depth, capacity, traj_words=0, want=TERMINATED | TIMEOUT, eligible=None):
        self.n, self.depth, self.capacity, self.tw, self.want = n, depth, capacity, traj_words, want
        self.eligible = None if eligible is None else np.asarray(eligible).astype(bool)
        self.ring = np.zeros((depth, n, ROW), np.uint32)
        self.ep_start = np.zeros(n, np.int64)
        self.ep_ordinal = np.zeros(n, np.int32)
        self.traj_start = np.zeros((n, traj_words), np.uint32)
        self.cap_rows = np.zeros((capacity, depth, ROW), np.uint32)
        self.cap_traj = np.zeros((capacity, traj_words), np.uint32)
        self.cap_meta = np.zeros((capacity, META), np.int32)
        self.claimed = 0   # counts past capacity, as cap_count[0]
        self.dropped = 0
        self.pushes = 0

    def _end(self, e, traj):
        self.ep_ordinal[e] += 1
        self.ep_start[e] = self.pushes
        if self.tw:
            self.traj_start[e] = bits(np.asarray(traj[e], np.float32))

    def push(self, root, dof_pos, reset, time_out, wp_index=None, traj=None):
        s, d = self.pushes, self.depth
        row = make_row(root, dof_pos, wp_index)
        for e in range(self.n):
            if not reset[e]:
                continue
            full = s - int(self.ep_start[e])
            kept = min(full, d)
            cause = TIMEOUT if time_out[e] else TERMINATED
            if cause & self.want and (self.eligible is None or self.eligible[e]):
                slot = self.claimed
                self.claimed += 1
                if slot < self.capacity:
                    for r in range(kept):
                        self.cap_rows[slot, r] = self.ring[(s - kept + r) % d, e]
                    self.cap_traj[slot] = self.traj_start[e]
                    self.cap_meta[slot] = [e, self.ep_ordinal[e], s, kept, full, cause, 0, 0]
                else:
                    self.dropped += 1
            self._end(e, traj)
        self.ring[s % d] = row
        self.pushes += 1

    def mark_reset(self, env_ids, traj=None):
        """A host-initiated reset: the bookkeeping of an ended episode without a capture."""
        for e in env_ids:
            self._end(int(e), traj)

    def counts(self):
        return min(self.claimed, self.capacity), self.dropped

    def sorted_captures(self):
        """(meta, rows, traj) of the claimed slots, sorted by (end push, env)."""
        return sort_captures(self.cap_meta, self.cap_rows, self.cap_traj, self.counts()[0])


def sort_captures(meta, rows, traj, k):
    meta, rows, traj = meta[:k], rows[:k], traj[:k]
    order = np.lexsort((meta[:, 0], meta[:, 2]))
    return meta[order], rows[order], traj[order]
