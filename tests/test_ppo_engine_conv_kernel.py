"""conv_kernel of csrc/ppo_conv.h through its test entry go1_ppo_test_conv: the CNN height-map encoder's convolution
stack, forward and backward, against float64 autograd (tests/conv_ref.py).

Rows: screened random maps U(-5, 5) (tests/conv_ref.py: no pool winner and no ReLU sign decided within rounding)
followed by the three tie rows (a map constant per channel, two integer plateaus, all zeros under nonzero biases),
which fix the first-maximum rule and ReLU'(0) = 0.  d_feat is N(0, 1) scaled per row by 10^-4 .. 10^-9 (gradients of
a mean over 24,576 rows; the spread exercises the per-row scaling), every fifth row zero.  Row counts: 1 (+ 3 tie
rows), 3 (+ 3), and 257 in all: the smallest count at which a workgroup takes two rows (a launch has at most 256
workgroups) and the last strip is ragged (129 workgroups, the last with one row).

Bounds.  The features within 1.4e-6 of the output's scale (the rollout's enc_conv_kernel).  The four
gradient tensors within K x the yardstick on max and relative L2 error, with tests/ppo_cases._compare's floors; the
yardstick is torch's f32 autograd of the same stack on the GPU.  K by the project's rule: twice the worst measured
ratio rounded up to a power of two, at most 32.

Measured on an MI355X (worst kernel / yardstick ratio per case): one 3.37, three 3.53, ragged 2.10 (all
conv2.weight, L2: 4.6e-7 .. 6.1e-7 against 1.4e-7 .. 2.9e-7); the tie rows alone 4.29 (two plateaus, conv2.weight, L2:
4.38e-7 against 1.02e-7).  K = 16 (2 x 4.29 rounded up).  The features: 7.5e-7 of the scale (torch f32: 2.1e-7).  The
screen: 150 of 254 rows unsafe at first, none after 9 redraws.
"""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import ppo_engine as PE  # noqa: E402
from tests import conv_ref as CR  # noqa: E402
from tests.ppo_cases import _compare  # noqa: E402

DEV = "cuda:0"
K_GRAD = 16.0
FEAT_TOL = 1.4e-6
PART_BYTES = 4 * (32 * 144 + 32 + 16 * 18 + 16)
CASES = {"one": 1, "three": 3, "ragged": 254}  # random rows; the three tie rows follow


def _work_bytes(rows):
    return 41216 + PART_BYTES * min(rows, 256)


def _call(lib, maps, filters, d_feat, work=None, reps=1):
    rows = maps.shape[0]
    out = [torch.full(s, float("nan"), device=DEV) for s in
           ((rows, CR.N_FEAT), (16, 2, 3, 3), (16,), (32, 16, 3, 3), (32,))]
    nb = _work_bytes(rows)
    hold = torch.zeros(nb + 512, dtype=torch.uint8, device=DEV) if work is None else work
    base = (hold.data_ptr() + 255) // 256 * 256
    w1, b1, w2, b2 = filters
    rc = lib.go1_ppo_test_conv(maps.data_ptr(), rows, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                               d_feat.data_ptr(), *(t.data_ptr() for t in out), base, nb, reps,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.go1_ppo_last_error()
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def data():
    """Filters, the 257 rows of the largest case and their d_feat, screened once; the cases take leading random rows."""
    g = torch.Generator().manual_seed(20)
    filters = [t.to(DEV) for t in CR.make_filters(g)]
    n = max(CASES.values())
    maps, rounds, first = CR.screened_maps(g, n, filters)
    print(f"\n[conv-kernel] screen: {first} of {n} rows unsafe at first, none after {rounds} redraws")
    ties = CR.tie_maps()
    assert not bool(CR.unsafe_rows(ties.to(DEV), *filters).any())
    mag = 10.0 ** -(4.0 + 5.0 * torch.rand(n + 3, 1, generator=g))
    d_feat = torch.randn(n + 3, CR.N_FEAT, generator=g) * mag
    d_feat[::5] = 0.0
    d_feat[n:] = torch.randn(3, CR.N_FEAT, generator=g) * 1e-6  # the tie rows carry a gradient
    return filters, maps, ties, d_feat


def _rows(data, case):
    filters, maps, ties, d_feat = data
    n, nmax = CASES[case], max(CASES.values())
    sel = list(range(n)) + [nmax, nmax + 1, nmax + 2]
    if n == 1:
        sel[0] = 1  # row 0's d_feat is zero
    return filters, torch.cat([maps[sel[:n]], ties]).to(DEV).contiguous(), d_feat[sel].to(DEV).contiguous()


def test_entry_refuses_bad_arguments_before_it_reads_a_buffer():
    lib = PE.load_library()
    assert hasattr(lib, "go1_ppo_test_conv")
    one = C.c_void_p(256)  # never dereferenced: the checks come first
    args = lambda rows, work, nb: (one, rows) + (one,) * 10 + (work, nb, 1, None)  # noqa: E731
    # the last case: room for the filters' images alone, none for a partial
    for rows, work, nb, word in ((0, one, 1 << 30, b"rows"), (1, C.c_void_p(264), 1 << 30, b"aligned"),
                                 (1, None, 1 << 30, b"bad argument"), (300, one, 41216, b"too small")):
        assert lib.go1_ppo_test_conv(*args(rows, work, nb)) == -1
        assert word in lib.go1_ppo_last_error(), lib.go1_ppo_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_features_and_gradients_against_f64(data, case):
    lib = PE.load_library()
    filters, maps, d_feat = _rows(data, case)
    feat, *g = _call(lib, maps, filters, d_feat)
    f64, g64, terms = CR.grads(maps, filters, d_feat, torch.float64)
    f32, g32, _ = CR.grads(maps, filters, d_feat, torch.float32)
    scale = float(f64.abs().max())
    err, err32 = float((feat.double() - f64).abs().max()), float((f32.double() - f64).abs().max())
    print(f"\n[conv-kernel] {case}: feat max error {err / scale:.2e} of the scale (torch f32 {err32 / scale:.2e})")
    assert err <= FEAT_TOL * scale
    # the decisions: a feature is zero exactly where the reference's is
    assert torch.equal(feat > 0, f64 > 0)
    worst = [0.0, ""]
    bad = _compare(case, CR.NAMES, g, g32, g64, worst, terms, k_grad=K_GRAD, show="[conv-kernel]")
    print(f"[conv-kernel] {case}: worst kernel / yardstick error ratio {worst[0]:.2f} ({worst[1]})")
    assert not bad, bad


@pytest.mark.gpu
def test_tie_rows_alone(data):
    """The three tie rows without a random row beside them: every interior window of the constant map is a four-way
    tie and every window of the zero map too, so a rule other than the first maximum moves whole terms."""
    lib = PE.load_library()
    filters, _, ties, d_feat = data
    maps, d = ties.to(DEV).contiguous(), d_feat[-3:].to(DEV).contiguous()
    for rows in ([0], [1], [2], [0, 1, 2]):
        feat, *g = _call(lib, maps[rows].contiguous(), filters, d[rows].contiguous())
        f64, g64, terms = CR.grads(maps[rows], filters, d[rows], torch.float64)
        _, g32, _ = CR.grads(maps[rows], filters, d[rows], torch.float32)
        assert float((feat.double() - f64).abs().max()) <= FEAT_TOL * float(f64.abs().max())
        # the zero map alone has no conv1 weight gradient: exactly none from the kernel as well
        live = [i for i in range(4) if float(g64[i].abs().max()) > 0.0]
        assert live == ([1, 2, 3] if rows == [2] else [0, 1, 2, 3])
        assert all(not bool(g[i].any()) for i in range(4) if i not in live)
        pick = lambda seq: [seq[i] for i in live]  # noqa: E731
        worst = [0.0, ""]
        bad = _compare(f"ties{rows}", pick(CR.NAMES), pick(g), pick(g32), pick(g64), worst, terms, k_grad=K_GRAD,
                       show="[conv-kernel]")
        assert not bad, bad


@pytest.mark.gpu
def test_two_calls_agree_bitwise_and_a_dirty_workspace_does_not_matter(data):
    lib = PE.load_library()
    filters, maps, d_feat = _rows(data, "ragged")
    a = _call(lib, maps, filters, d_feat)
    dirty = torch.full((_work_bytes(maps.shape[0]) + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    b = _call(lib, maps, filters, d_feat, work=dirty, reps=2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # a row's features do not depend on the rows beside it or on its place in a strip
    c = _call(lib, maps[5:6].contiguous(), filters, d_feat[5:6].contiguous())
    assert torch.equal(c[0][0], a[0][5])
