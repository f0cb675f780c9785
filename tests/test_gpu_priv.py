"""The privileged-observation kernel against the reference's own output (tests/golden/priv_cases.npz) and the
restatement (tests/priv_ref.py): every flag set and step of the fixture bit for bit, guard rows behind every plane and
the output, more than one ragged workgroup, planes passed as row views of wider allocations, absent planes."""
import numpy as np
import pytest
import torch

from legged_tracking_amd import privileged as PV
from tests import priv_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 5          # rows behind every plane and the output that no launch may touch
SENTINEL = -77.0   # outside every clip used here, so an unwritten output element shows


@pytest.fixture(scope="module")
def fixture():
    return PR.load()


class Planes:
    """Device planes of n envs, each followed by GUARD rows of the sentinel; `wide` allocates the motor planes and the
    root with extra columns and hands out row views."""

    def __init__(self, n, width, wide=False):
        self.n = n
        extra = 3 if wide else 0
        cols = dict(PV.PLANE_COLS, aux=32)
        self.store = {k: torch.full((n + GUARD, c + (extra if k in ("motor_strength", "motor_offset", "root") else 0)),
                                    SENTINEL, device=DEV) for k, c in cols.items()}
        self.cols = cols
        self.out = torch.full((n + GUARD, width), SENTINEL, device=DEV)

    def load(self, planes):
        for k, v in planes.items():
            v = np.asarray(v, np.float32).reshape(self.n, -1)
            self.store[k][:self.n, :v.shape[1]] = torch.from_numpy(v).to(DEV)

    def views(self, only=None):
        return {k: t[:self.n, :self.cols[k]] for k, t in self.store.items() if only is None or k in only}

    def launch(self, b, gravities, only=None):
        self.out.fill_(SENTINEL)
        b.launch(self.out[:self.n], gravities, **self.views(only))
        torch.cuda.synchronize()
        return self.out[:self.n].cpu().numpy()

    def guards_intact(self, planes):
        n = self.n
        ok = bool((self.out[n:] == SENTINEL).all())
        for k, t in self.store.items():
            ok &= bool((t[n:] == SENTINEL).all())
            if k in planes:  # the planes themselves are read only
                v = np.asarray(planes[k], np.float32).reshape(n, -1)
                ok &= bool((t[:n, :v.shape[1]].cpu().numpy() == v).all())
                ok &= bool((t[:n, v.shape[1]:] == SENTINEL).all())
        return ok


@pytest.mark.parametrize("name", PR.SETS)
def test_kernel_matches_the_reference(fixture, name):
    d = fixture
    cfg = PR.cfg_of(d, name)
    want = d[name + "/priv"]
    steps, n, w = want.shape
    b = PV.PrivBuffers(n, DEV, PV.columns(cfg), cfg.normalization.clip_observations)
    p = Planes(n, w)
    for s in range(steps):
        planes = PR.planes_of(d, s)
        p.load(planes)
        got = p.launch(b, d["gravities"][s])
        np.testing.assert_array_equal(PR.bits(got), PR.bits(want[s]), err_msg=f"{name} step {s}")
        assert p.guards_intact(planes)


def _random_planes(n, seed):
    rng = np.random.default_rng(seed)
    planes = dict(friction=rng.uniform(0.05, 5.5, (n, 1)), restitution=rng.uniform(0.0, 1.0, (n, 1)),
                  payloads=rng.uniform(-1.0, 3.0, (n, 1)), motor_strength=rng.uniform(0.9, 1.1, (n, 12)),
                  motor_offset=rng.uniform(-0.06, 0.06, (n, 12)), root=rng.normal(0.0, 2.0, (n, 13)),
                  aux=rng.normal(0.0, 3.0, (n, 32)))
    return {k: v.astype(np.float32) for k, v in planes.items()}, rng.uniform(-1.0, 1.0, 3).astype(np.float32)


@pytest.mark.parametrize("wide", [False, True])
def test_ragged_workgroups_and_row_views(fixture, wide):
    """70 envs x 45 columns = 3,150 elements: 13 workgroups, the last one ragged, no multiple of a wave.  wide: the
    motor planes and the root are row views of wider allocations (their row stride is not their width)."""
    n = 70
    cfg = PR.cfg_of(fixture, "all")
    cols = PV.columns(cfg)
    b = PV.PrivBuffers(n, DEV, cols, cfg.normalization.clip_observations)
    planes, g = _random_planes(n, 4300)
    p = Planes(n, 45, wide=wide)
    p.load(planes)
    if wide:
        assert not p.views()["root"].is_contiguous() and p.views()["motor_offset"].stride(0) == 15
    got = p.launch(b, g)
    want = PR.assemble(cols, cfg.normalization.clip_observations, n, g, **planes)
    np.testing.assert_array_equal(PR.bits(got), PR.bits(want))
    assert p.guards_intact(planes)
    clip = np.float32(cfg.normalization.clip_observations)
    assert (np.abs(got) == clip).any() and (np.abs(got) < clip).any()


def test_absent_planes(fixture):
    """A plane that no column reads may be left out; one that a column reads is refused by name before any launch."""
    d = fixture
    cfg = PR.cfg_of(d, "sparse")  # motor_offset, body_velocity (aux), gravity
    cols = PV.columns(cfg)
    b = PV.PrivBuffers(32, DEV, cols, cfg.normalization.clip_observations)
    p = Planes(32, 18)
    planes = PR.planes_of(d, 3)
    p.load(planes)
    got = p.launch(b, d["gravities"][3], only=("motor_offset", "aux"))
    np.testing.assert_array_equal(PR.bits(got), PR.bits(d["sparse/priv"][3]))
    with pytest.raises(PV.NativeError, match="aux plane"):
        p.launch(b, d["gravities"][3], only=("motor_offset",))
    assert bool((p.out == SENTINEL).all())  # refused before the launch
    with pytest.raises(PV.NativeError, match="out must be"):
        b.launch(p.out[:32, :17], d["gravities"][3], **p.views())
    with pytest.raises(PV.NativeError, match="motor_offset"):
        b.launch(p.out[:32], d["gravities"][3], **dict(p.views(), motor_offset=p.store["motor_offset"][:32, ::2]))
