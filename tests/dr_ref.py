"""Numpy restatement of the after-start domain randomiser (include/go1_dr.h): what one go1_dr_step / go1_dr_reset
launch does to the planes, in f32 with a separate multiply and add, from given uniforms.  The fixture
tests/golden/dr_cases.npz (tests/golden/make_golden_dr.py: the reference's own _randomize_rigid_body_props and
_push_robots) pins it; the GPU tests compare the kernel with it."""
import os

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = os.path.join(HERE, "golden", "dr_cases.npz")
DR_U = 8
U_PAYLOAD, U_FRICTION, U_RESTITUTION, U_PUSH_X, U_PUSH_Y = 0, 1, 2, 4, 5
DR_TAG = 0x44520000


def load_set(name):
    """One case set ("all" / "partial") of the fixture as {array name: array}."""
    z = np.load(CASES)
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}


FLAG_NAMES = ("rigids_after_start", "push_robots", "payload", "friction", "restitution")


def ref_of(d, n=None):
    """(DrRef, flags, ranges, priv) configured as case set d was generated."""
    n = d["reset"].shape[1] if n is None else n
    flags = dict(zip(FLAG_NAMES, (bool(x) for x in d["flags"])))
    ranges = dict(payload=tuple(d["range_payload"]), friction=tuple(d["range_friction"]),
                  restitution=tuple(d["range_restitution"]), push=float(d["max_push"]))
    priv = priv_consts(d["norm_friction"], d["norm_restitution"], float(d["clip_obs"]))
    return DrRef(n, ranges, flags, int(d["rand_interval"]), int(d["push_interval"]), priv), flags, ranges, priv


def f32_range(rng):
    """(f32(hi - lo), f32(lo)): the Python-float difference, rounded once, as torch multiplies a f32 tensor by it."""
    lo, hi = rng
    return F(hi - lo), F(lo)


def priv_consts(friction_norm, restitution_norm, clip_obs):
    """(friction shift, friction scale, restitution shift, restitution scale, clip) of the privileged observation's
    normalisation ranges, as config.build_abi_config derives them."""
    fr, rr = friction_norm, restitution_norm
    return (F((fr[1] + fr[0]) / 2.0), F(2.0 / (fr[1] - fr[0])), F((rr[1] + rr[0]) / 2.0), F(2.0 / (rr[1] - rr[0])),
            F(clip_obs))


def priv_of(friction, restitution, pc):
    """The step kernels' privileged observation columns 0, 1 from the planes (go1_traj_step.h, go1_vel_step.h)."""
    fs, fk, rs, rk, clip = pc
    p0 = np.clip((np.asarray(friction, F).reshape(-1) - fs) * fk, -clip, clip)
    p1 = np.clip((np.asarray(restitution, F).reshape(-1) - rs) * rk, -clip, clip)
    return np.stack([p0, p1], 1).astype(F)


def philox4x32(ctr, key):
    """Philox4x32-10 of one counter (4 uint32) under one key (2 uint32), as go1_lanes.h has it."""
    c = [int(x) for x in ctr]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF,
             p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def philox_uniforms(seed, rng_step, gid, block):
    """The four uniforms of one block of global env gid, with the header's counter layout."""
    w = philox4x32([gid, DR_TAG + block, rng_step & 0xFFFFFFFF, rng_step >> 32], [seed & 0xFFFFFFFF, seed >> 32])
    return np.array([F(x >> 8) * F(1.0 / 16777216.0) for x in w], F)


class DrRef:
    """State and the two launches.  `ranges`, `flags`, `priv` as randomize.DrBuffers takes them."""

    def __init__(self, n, ranges, flags, rand_interval, push_interval, priv):
        self.n = n
        self.ranges, self.flags = dict(ranges), dict(flags)
        self.rand_interval, self.push_interval = int(rand_interval), int(push_interval)
        self.pc = tuple(F(x) for x in priv)
        self.root = np.zeros((n, 13), F)
        self.friction, self.restitution, self.payloads = (np.zeros(n, F) for _ in range(3))

    def load(self, root, friction, restitution, payloads):
        self.root = np.array(root, F).reshape(self.n, 13)
        self.friction, self.restitution, self.payloads = (np.array(x, F).reshape(self.n).copy()
                                                          for x in (friction, restitution, payloads))

    def due(self, reset, ep):
        """(rigids, push) masks of one go1_dr_step launch."""
        r, ep = np.asarray(reset).astype(bool).reshape(-1), np.asarray(ep).reshape(-1)
        rig = (r | (ep % self.rand_interval == 0)) if self.flags["rigids_after_start"] else np.zeros(self.n, bool)
        push = (~r & (ep % self.push_interval == 0)) if self.flags["push_robots"] else np.zeros(self.n, bool)
        return rig, push

    def _redraw(self, ids, u):
        for key, plane, slot in (("payload", self.payloads, U_PAYLOAD), ("friction", self.friction, U_FRICTION),
                                 ("restitution", self.restitution, U_RESTITUTION)):
            if self.flags[key]:
                rg, lo = f32_range(self.ranges[key])
                plane[ids] = F(u[ids, slot] * rg) + lo

    def step(self, reset, ep, uniforms, priv=None):
        """go1_dr_step; `priv` (n, >= 2) is rewritten in place for the redrawn envs.  Returns (rigids, push)."""
        u = np.asarray(uniforms, F).reshape(self.n, DR_U)
        rig, push = self.due(reset, ep)
        ids = np.nonzero(rig)[0]
        self._redraw(ids, u)
        if priv is not None and (self.flags["friction"] or self.flags["restitution"]) and ids.size:
            priv[ids, :2] = priv_of(self.friction[ids], self.restitution[ids], self.pc)
        mv = float(self.ranges["push"])
        rg, lo = F(mv - (-mv)), F(-mv)
        pid = np.nonzero(push)[0]
        self.root[pid, 7] = F(rg * u[pid, U_PUSH_X]) + lo
        self.root[pid, 8] = F(rg * u[pid, U_PUSH_Y]) + lo
        return rig, push

    def reset(self, env_ids, uniforms):
        """go1_dr_reset."""
        if self.flags["rigids_after_start"]:
            self._redraw(np.asarray(env_ids, np.int64), np.asarray(uniforms, F).reshape(self.n, DR_U))
