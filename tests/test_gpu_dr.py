"""The after-start domain randomiser's kernels against the reference's own output (tests/golden/dr_cases.npz) and the
restatement (tests/dr_ref.py): injected uniforms, Philox with the header's counter layout, absent optional pointers,
sharding by env_id_offset, more than one workgroup, and the host reset's redraw."""
import numpy as np
import pytest
import torch

from legged_tracking_amd import randomize as RZ
from tests import dr_ref as DR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x1234567890AB
GUARD = 7  # rows behind every plane that no launch may touch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Planes:
    """Device planes of n envs, each followed by GUARD rows of a sentinel; friction, restitution and the payload plane
    (which no launch is given) lie next to each other in one allocation."""

    def __init__(self, n, priv_width=2):
        self.n = n
        self.root = torch.full((n + GUARD, 13), -7.0, device=DEV)
        self.block = torch.full((3, n + GUARD, 1), -7.0, device=DEV)
        self.priv = torch.full((n + GUARD, priv_width), -7.0, device=DEV)
        self.dbg = torch.zeros((n + GUARD, RZ.DR_U), device=DEV)
        self.ep = torch.zeros((n, 1), dtype=torch.int32, device=DEV)
        self.reset = torch.zeros(n, dtype=torch.bool, device=DEV)

    friction = property(lambda s: s.block[0, :s.n])
    restitution = property(lambda s: s.block[1, :s.n])
    payload = property(lambda s: s.block[2, :s.n])

    def load(self, root, friction, restitution, payload, ep, reset, priv=None):
        n = self.n
        self.root[:n] = torch.from_numpy(np.asarray(root, np.float32)).to(DEV)
        for plane, v in ((self.friction, friction), (self.restitution, restitution), (self.payload, payload)):
            plane.copy_(torch.from_numpy(np.asarray(v, np.float32).reshape(n, 1)))
        self.ep.copy_(torch.from_numpy(np.asarray(ep, np.int32).reshape(n, 1)))
        self.reset.copy_(torch.from_numpy(np.asarray(reset).astype(bool)))
        if priv is not None:
            self.priv[:n, :2] = torch.from_numpy(np.asarray(priv, np.float32)).to(DEV)

    def launch(self, b, rng_step, uniforms=None, priv=True, dbg=False, payloads=True):
        n = self.n
        u = None if uniforms is None else torch.from_numpy(np.ascontiguousarray(uniforms, np.float32)).to(DEV)
        b.launch(self.root[:n], self.friction, self.restitution, self.ep, self.reset, rng_step,
                 self.priv[:n] if priv else None, u, self.dbg[:n] if dbg else None, payloads)
        torch.cuda.synchronize()

    def guards_intact(self):
        n = self.n
        return all(bool((t == -7.0).all()) for t in (self.root[n:], self.block[:, n:], self.priv[n:])) and \
            not bool(self.dbg[n:].any())

    def host(self, b):
        n = self.n
        return dict(root=self.root[:n].cpu().numpy(), friction=self.friction[:, 0].cpu().numpy(),
                    restitution=self.restitution[:, 0].cpu().numpy(), payloads=b.payloads[:, 0].cpu().numpy(),
                    priv=self.priv[:n, :2].cpu().numpy(), payload_plane=self.payload[:, 0].cpu().numpy())


def buffers(d, n=32, offset=0):
    _, flags, ranges, priv = DR.ref_of(d)
    return RZ.DrBuffers(n, DEV, ranges, flags, int(d["rand_interval"]), int(d["push_interval"]), priv,
                        env_id_offset=offset, seed=SEED)


@pytest.mark.parametrize("name", ["all", "partial"])
def test_kernel_matches_the_reference_with_injected_uniforms(name):
    d = DR.load_set(name)
    b, p = buffers(d), Planes(32, priv_width=3)  # a privileged observation wider than the two columns written
    for s in range(d["reset"].shape[0]):
        p.load(d["root_before"][s], d["friction_before"][s], d["restitution_before"][s], d["payload_plane"][s],
               d["episode_length"][s], d["reset"][s], d["priv_before"][s])
        b.payloads.copy_(torch.from_numpy(d["payloads_before"][s].reshape(32, 1)))
        p.launch(b, rng_step=s, uniforms=d["uniforms"][s])
        got = p.host(b)
        for k in ("root", "friction", "restitution", "payloads", "priv"):
            np.testing.assert_array_equal(bits(got[k]), bits(d[k + "_after"][s]), err_msg=f"{k}, step {s}")
        np.testing.assert_array_equal(bits(got["payload_plane"]), bits(d["payload_plane"][s]))
        assert p.guards_intact() and bool((p.priv[:32, 2] == -7.0).all())


@pytest.mark.parametrize("name", ["all", "partial"])
def test_kernel_philox_draws_feed_the_restatement_to_the_same_planes(name):
    d = DR.load_set(name)
    b, p = buffers(d, offset=64), Planes(32)
    ref, flags, _, _ = DR.ref_of(d)
    for s in (0, 3, 7):
        before = [d[k + "_before"][s] for k in ("root", "friction", "restitution")]
        p.load(*before, d["payload_plane"][s], d["episode_length"][s], d["reset"][s], d["priv_before"][s])
        b.payloads.copy_(torch.from_numpy(d["payloads_before"][s].reshape(32, 1)))
        p.dbg.zero_()
        step = (1 << 40) + s
        p.launch(b, rng_step=step, dbg=True)
        u = p.dbg[:32].cpu().numpy()
        ref.load(*before, d["payloads_before"][s])
        pv = d["priv_before"][s].copy()
        rig, push = ref.step(d["reset"][s], d["episode_length"][s], u, pv)
        got = p.host(b)
        for k, want in (("root", ref.root), ("friction", ref.friction), ("restitution", ref.restitution),
                        ("payloads", ref.payloads), ("priv", pv)):
            np.testing.assert_array_equal(bits(got[k]), bits(want), err_msg=f"{k}, step {s}")
        # the uniforms are the header's: Philox keyed by the seed, counter (global env, tag + block, step)
        assert np.all((u >= 0) & (u < 1)) and not u[~(rig | push)].any()
        for e in np.nonzero(rig)[0][:4]:
            w = DR.philox_uniforms(SEED, step, 64 + int(e), 0)
            for key, slot in (("payload", DR.U_PAYLOAD), ("friction", DR.U_FRICTION), ("restitution", DR.U_RESTITUTION)):
                assert u[e, slot] == (w[slot] if flags[key] else 0.0), (e, key)
        for e in np.nonzero(push)[0][:4]:
            w = DR.philox_uniforms(SEED, step, 64 + int(e), 1)
            assert u[e, DR.U_PUSH_X] == w[0] and u[e, DR.U_PUSH_Y] == w[1]
        assert p.guards_intact()


def test_optional_pointers_absent():
    d = DR.load_set("all")
    b, p = buffers(d), Planes(32)
    s = 3
    p.load(d["root_before"][s], d["friction_before"][s], d["restitution_before"][s], d["payload_plane"][s],
           d["episode_length"][s], d["reset"][s], d["priv_before"][s])
    b.payloads.fill_(-3.0)
    p.launch(b, rng_step=s, uniforms=d["uniforms"][s], priv=False, dbg=False, payloads=False)
    got = p.host(b)
    for k in ("root", "friction", "restitution"):
        np.testing.assert_array_equal(bits(got[k]), bits(d[k + "_after"][s]))
    np.testing.assert_array_equal(bits(got["priv"]), bits(d["priv_before"][s]))  # not given: not written
    assert bool((b.payloads == -3.0).all()) and not bool(p.dbg.any()) and p.guards_intact()


def test_two_shards_equal_one_buffer():
    d = DR.load_set("all")
    whole, pw = buffers(d), Planes(32)
    shards = [(buffers(d, 16, off), Planes(16), slice(off, off + 16)) for off in (0, 16)]
    s0 = 0
    pw.load(d["root_before"][s0], d["friction_before"][s0], d["restitution_before"][s0], d["payload_plane"][s0],
            d["episode_length"][s0], d["reset"][s0], d["priv_before"][s0])
    for _, p, sl in shards:
        p.load(d["root_before"][s0][sl], d["friction_before"][s0][sl], d["restitution_before"][s0][sl],
               d["payload_plane"][s0][sl], d["episode_length"][s0][sl], d["reset"][s0][sl], d["priv_before"][s0][sl])
    changed = 0
    for s in range(12):  # the planes carry over; the fixture supplies each step's resets and episode lengths
        for p, sl in [(pw, slice(0, 32))] + [(p, sl) for _, p, sl in shards]:
            p.ep.copy_(torch.from_numpy(d["episode_length"][s][sl].reshape(-1, 1)))
            p.reset.copy_(torch.from_numpy(d["reset"][s][sl]))
        pw.launch(whole, rng_step=100 + s)
        one = pw.host(whole)
        parts = []
        for b, p, _ in shards:
            p.launch(b, rng_step=100 + s)
            parts.append(p.host(b))
        for k in one:
            np.testing.assert_array_equal(bits(one[k]), bits(np.concatenate([x[k] for x in parts])), err_msg=f"{k} {s}")
        changed += int(d["rigids"][s].sum())
    assert changed > 32 and len(np.unique(bits(one["friction"]))) > 16  # draws differ between envs


def test_more_than_one_workgroup_against_the_restatement():
    n = 600  # three workgroups, the last one partly filled
    d = DR.load_set("all")
    _, flags, ranges, priv = DR.ref_of(d)
    b = RZ.DrBuffers(n, DEV, ranges, flags, 5, 7, priv, env_id_offset=1 << 20, seed=SEED)
    ref = DR.DrRef(n, ranges, flags, 5, 7, priv)
    rng = np.random.default_rng(3)
    root = rng.normal(0, 1, (n, 13)).astype(np.float32)
    fr, rs, pl = (rng.uniform(0.1, 1.0, n).astype(np.float32) for _ in range(3))
    ep = rng.integers(0, 40, n).astype(np.int32)
    reset = rng.random(n) < 0.05
    ep[reset] = 0
    ep[-1], reset[-1] = 35, False  # the last env is due for both
    pv = DR.priv_of(fr, rs, priv)
    p = Planes(n)
    p.load(root, fr, rs, pl, ep, reset, pv)
    b.payloads.copy_(torch.from_numpy(pl.reshape(n, 1)))
    step = (1 << 62) + 9
    p.launch(b, rng_step=step)
    u = np.zeros((n, DR.DR_U), np.float32)
    for e in range(n):
        u[e, :4] = DR.philox_uniforms(SEED, step, (1 << 20) + e, 0)
        u[e, 4:] = DR.philox_uniforms(SEED, step, (1 << 20) + e, 1)
    ref.load(root, fr, rs, pl)
    rig, push = ref.step(reset, ep, u, pv)
    assert rig[-1] and push[-1] and rig.sum() > 100 and push.sum() > 50 and (~(rig | push)).sum() > 100
    got = p.host(b)
    for k, want in (("root", ref.root), ("friction", ref.friction), ("restitution", ref.restitution),
                    ("payloads", ref.payloads), ("priv", pv)):
        np.testing.assert_array_equal(bits(got[k]), bits(want), err_msg=k)
    np.testing.assert_array_equal(bits(got["payload_plane"]), bits(pl))
    assert p.guards_intact()


@pytest.mark.parametrize("name", ["all", "partial"])
def test_host_reset_matches_the_reference(name):
    d = DR.load_set(name)
    b, p = buffers(d), Planes(32)
    root = d["root_before"][0]
    p.load(root, d["host_friction_before"], d["host_restitution_before"], d["payload_plane"][0], np.zeros(32), np.zeros(32))
    b.payloads.copy_(torch.from_numpy(d["host_payloads_before"].reshape(32, 1)))
    ids = torch.from_numpy(np.concatenate([d["host_ids"], [-1, 32, d["host_ids"][0]]]).astype(np.int64)).to(DEV)
    b.reset(p.root[:32], p.friction, p.restitution, ids, 5, torch.from_numpy(d["host_uniforms"]).to(DEV))
    torch.cuda.synchronize()
    got = p.host(b)
    for k in ("friction", "restitution", "payloads"):
        np.testing.assert_array_equal(bits(got[k]), bits(d[f"host_{k}_after"]), err_msg=k)
    np.testing.assert_array_equal(bits(got["root"]), bits(root))
    np.testing.assert_array_equal(bits(got["payload_plane"]), bits(d["payload_plane"][0]))
    assert p.guards_intact()
    # Philox: the reset's block 0 of the same counter layout
    b.reset(p.root[:32], p.friction, p.restitution, [3], (1 << 62) + 2)
    torch.cuda.synchronize()
    _, flags, ranges, _ = DR.ref_of(d)
    w = DR.philox_uniforms(SEED, (1 << 62) + 2, 3, 0)
    rg, lo = DR.f32_range(ranges["restitution"])
    assert float(p.restitution[3, 0]) == float(np.float32(w[DR.U_RESTITUTION] * rg) + lo)
