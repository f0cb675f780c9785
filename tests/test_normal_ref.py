"""tests/normal_ref.py (the numpy restatement of the policy kernels' Normal draw) against the published Philox
answers, the oracle's copy of the stream against the restatement, and the reference's own edge claims.  The seeds the
GPU tests draw with are chosen here, from the reference alone."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import normal_ref as NR

# Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

# the draws the GPU tests compare value by value (tests/test_gpu_policy_sampling.py)
DRAW_SEED, DRAW_STEPS, DRAW_N = 13, (7, 8, 9), 4096
# (global env, first action of the pair) whose u1 is exactly 1.0 at (DRAW_SEED, step 7): found by a sweep of the
# reference over 2^27 env ids
U1_ONE = ((5327885, 4), (6783923, 2))


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = NR.philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == want


def test_philox_known_answers_vectorised():
    """The three vectors as one batch: the array form computes what the scalar form does."""
    c = np.array([k[0] for k in KAT], dtype=np.uint64)
    k = np.array([k[1] for k in KAT], dtype=np.uint64)
    got = np.stack(NR.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]), axis=-1)
    np.testing.assert_array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint64))


def test_block_places_step_and_seed_words():
    """block(seed, step, gid, q) = philox(counter (gid, q, step lo, step hi), key (seed lo, seed hi)): the third
    known answer read as a 64-bit step and seed."""
    ctr, key, want = KAT[2]
    got = NR.block(key[0] | (key[1] << 32), ctr[2] | (ctr[3] << 32), ctr[0], ctr[1])
    assert tuple(int(v) for v in got) == want


def test_oracle_uniform_is_the_restated_stream():
    """oracle/go1_oracle.c go1o_uniform (the step kernels' stream, held bit for bit to go1_lanes.h by
    test_philox_streams_match_oracle) on 4,000 (seed, step, env, slot) tuples, high words of seed and step set."""
    lib = O.lib()
    g = np.random.default_rng(5)
    m = 4000
    seed = g.integers(0, 2 ** 64, m, dtype=np.uint64)
    step = g.integers(0, 2 ** 64, m, dtype=np.uint64)
    seed[:500] &= np.uint64(0xFFFFFFFF)  # and some with zero high words
    step[250:750] &= np.uint64(0xFFFFFFFF)
    env = g.integers(0, 2 ** 32, m, dtype=np.uint64)
    slot = g.integers(0, 64, m, dtype=np.uint64)
    assert (seed >> np.uint64(32)).any() and (step >> np.uint64(32)).any()
    got = np.array([lib.go1o_uniform(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(seed, step, env, slot)],
                   dtype=np.float32)
    x = np.stack(NR.block(seed, step, env, slot >> np.uint64(2)), axis=-1)
    want = NR.uniform_u2(x[np.arange(m), (slot & np.uint64(3)).astype(np.int64)])
    np.testing.assert_array_equal(got, want)


def test_u1_reaches_one_and_z_is_zero_there():
    """(f32(m) + 0.5f) is not representable for m >= 2^23 and rounds to even, so u1 = 1.0 for m = 2^24 - 1: the
    interval is (0, 1], r = sqrt(-2 ln 1) = 0 and z = +-0, never NaN.  u2 stays below 1."""
    x = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000100, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64)
    u1, u2 = NR.uniform_u1(x), NR.uniform_u2(x)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    assert u1[0] == np.float32(2.0 ** -25) and u1.min() > 0.0
    assert u1[-1] == 1.0 and u1[-2] == 1.0 and u1.max() == 1.0
    assert u1[4] == np.float32((2 ** 23 + 2) * 2.0 ** -24)  # m = 2^23 + 1, the tie goes to the even neighbour
    assert u2[0] == 0.0 and u2.max() == np.float32(1.0 - 2.0 ** -24) < 1.0
    # every u1 of a full sweep of the top mantissas, against every angle class
    m = np.arange(2 ** 24 - 4096, 2 ** 24, dtype=np.uint64) << np.uint64(8)
    zc, zs = NR.box_muller(NR.uniform_u1(m)[:, None], NR.uniform_u2(x)[None, :])
    assert np.isfinite(zc).all() and np.isfinite(zs).all()
    one = NR.uniform_u1(m) == 1.0
    assert one.any() and (zc[one] == 0.0).all() and (zs[one] == 0.0).all()
    # and the other end: the largest radius of the stream
    r = np.sqrt(-2.0 * np.log(np.float64(NR.uniform_u1(np.uint64(0)))))
    assert 5.887 < r < 5.8871  # sqrt(50 ln 2)


def test_action_layout():
    """normal(): element r of group q is action 4 q + r; pair p of the block gives (cos, sin) at 2 p, 2 p + 1."""
    n, seed, step, off = 5, 2 ** 40 + 3, 2 ** 32 + 5, 1000
    z = NR.normal(seed, step, n, off)
    assert z.shape == (n, 16)
    for e in (0, 4):
        for q in range(4):
            x = [int(v) for v in NR.block(seed, step, e + off, q)]
            for p in range(2):
                zc, zs = NR.box_muller(NR.uniform_u1(x[2 * p]), NR.uniform_u2(x[2 * p + 1]))
                assert z[e, 4 * q + 2 * p] == zc and z[e, 4 * q + 2 * p + 1] == zs
    # the offset shifts the env id: rows [1000, 1005) of an offset-0 batch
    np.testing.assert_array_equal(z, NR.normal(seed, step, off + n)[off:])


def test_chosen_seed_covers_the_edges():
    """The draws of tests/test_gpu_policy_sampling.py (4096 envs x 3 steps x 16 actions), from the reference alone:
    at least 5 values beyond 4 sigma, a u2 within 1e-3 of every quadrant boundary, a u1 above 1 - 2^-20."""
    big, near, top = NR.coverage(DRAW_SEED, DRAW_STEPS, DRAW_N)
    assert big >= 5, big
    assert (near < 1e-3).all(), near
    assert top > 1.0 - 2.0 ** -20, top


def test_chosen_envs_draw_u1_of_exactly_one():
    for gid, a in U1_ONE:
        u1, _ = NR.uniforms(DRAW_SEED, 7, 1, env_id_offset=gid)
        assert u1[0, a // 4, (a % 4) // 2] == 1.0
        z = NR.normal(DRAW_SEED, 7, 1, env_id_offset=gid)[0]
        assert z[a] == 0.0 and z[a + 1] == 0.0 and np.isfinite(z).all()


def test_reference_moments_and_log_prob():
    """Sanity of the reference itself: unit normal moments over 196,608 draws, and log_prob against the closed form."""
    z = np.concatenate([NR.normal(DRAW_SEED, s, DRAW_N) for s in DRAW_STEPS])
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    assert abs((z[:, 0::2] * z[:, 1::2]).mean()) < 0.01  # the cos and sin halves are uncorrelated
    std = np.linspace(0.3, 2.5, 13)
    lp = NR.log_prob(z[:8], std)
    want = sum(-0.5 * z[:8, a] ** 2 - np.log(std[a]) - 0.5 * np.log(2 * np.pi) for a in range(13))
    np.testing.assert_allclose(lp, want, rtol=1e-14)
