"""The decision screen of tests/conv_ref.py on the CPU: it finds a constructed near-tie of a pool window and a
constructed ReLU sign within rounding, it passes rows whose only ties are exact ties of identical patches, and its
redraw loop converges on the random recipe.  Filters with one tap make the pre-activations readable: conv1's output
is the map's channel 0 plus the bias.
"""
import pytest

torch = pytest.importorskip("torch")

from tests import conv_ref as CR  # noqa: E402


def _tap_filters():
    """conv1: every channel the centre tap of map channel 0, bias 0.5; conv2: a small seeded random filter."""
    g = torch.Generator().manual_seed(11)
    w1 = torch.zeros(16, 2, 3, 3)
    w1[:, 0, 1, 1] = 1.0
    _, _, w2, b2 = CR.make_filters(g)
    return [w1, torch.full((16,), 0.5), w2, b2]


def _safe_rows(filters, n):
    maps, _, _ = CR.screened_maps(torch.Generator().manual_seed(3), n, filters)
    return maps


def test_near_tie_and_sign_flip_are_found_and_only_in_their_rows():
    f = _tap_filters()
    maps = _safe_rows(f, 4)
    assert not bool(CR.unsafe_rows(maps, *f).any())
    m = maps.clone().reshape(4, *CR.MAP)
    # row 1: two candidates of the pool window (5, 5) 1e-7 apart (the bound of either is 2^-21 x 3.5), the others low
    m[1, 0, 10:12, 10:12] = -4.0
    m[1, 0, 10, 11] = 3.0
    m[1, 0, 11, 10] = 3.0 + 1e-7
    # row 2: the winner of the window (7, 3) is 1e-7 above zero after the bias (bound 2^-21 x 1.0), the others negative
    m[2, 0, 14:16, 6:8] = -4.0
    m[2, 0, 15, 7] = -0.5 + 1e-7
    bad = CR.unsafe_rows(m.reshape(4, -1), *f)
    assert bad.tolist() == [False, True, True, False]
    # the same gap far from rounding is no finding: 1e-3 against a bound of 1.7e-6
    m[1, 0, 11, 10] = 3.0 + 1e-3
    m[2, 0, 15, 7] = -0.5 + 1e-3
    assert not bool(CR.unsafe_rows(m.reshape(4, -1), *f).any())


def test_a_near_tie_below_the_relu_is_no_decision():
    f = _tap_filters()
    m = _safe_rows(f, 1).reshape(1, *CR.MAP).clone()
    m[0, 0, 10:12, 10:12] = -4.0
    m[0, 0, 10, 11] = -3.0
    m[0, 0, 11, 10] = -3.0 + 1e-7  # both candidates are far below zero: whichever wins, the ReLU stops it
    assert not bool(CR.unsafe_rows(m.reshape(1, -1), *f).any())


def test_exact_ties_of_identical_patches_pass():
    g = torch.Generator().manual_seed(5)
    f = CR.make_filters(g)
    ties = CR.tie_maps()
    assert ties.shape == (3, CR.N_MAP)
    assert not bool(CR.unsafe_rows(ties, *f).any())
    # and the ties are there: a constant map's interior windows hold four equal candidates
    keep = {}
    CR.stack(ties[:1].double(), *(t.double() for t in f), keep=keep)
    z = keep["z1"][0, :, 2:4, 2:4]
    assert bool((z == z[:, :1, :1]).all())


def test_the_redraw_loop_converges_on_the_random_recipe():
    g = torch.Generator().manual_seed(5)
    f = CR.make_filters(g)
    maps, rounds, first = CR.screened_maps(g, 8, f)
    assert maps.shape == (8, CR.N_MAP) and rounds < 40
    assert not bool(CR.unsafe_rows(maps, *f).any())
    print(f"\n[conv-screen] 8 rows: {first} unsafe at first, none after {rounds} redraws")
