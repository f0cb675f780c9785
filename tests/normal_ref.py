"""numpy restatement of the policy kernels' in-kernel Normal draw (csrc/policy_tiles.h normal4) -- TEST REFERENCE ONLY.

Shares no code with the kernels or the oracle.  Philox4x32-10 is restated from Salmon, Moraes, Dror, Shaw,
"Parallel random numbers: as easy as 1, 2, 3" (SC'11) and held to the Random123 known answers
(tests/test_normal_ref.py); the uniforms are formed in float32 with the kernel's single IEEE operations, so they are
the kernel's bits; Box-Muller runs in float64 from those uniforms.

Stream layout (normal4): one Philox block per (global env, action group q of four actions, step),
counter = (gid, q, step lo, step hi), key = (seed lo, seed hi); output words (x0, x1) and (x2, x3) are the two
Box-Muller pairs, z[2 p] = r cos(2 pi u2), z[2 p + 1] = r sin(2 pi u2); element r of group q is action 4 q + r.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # the two multipliers (Salmon et al., table 2)
W0, W1 = 0x9E3779B9, 0xBB67AE85  # the Weyl key increments: golden ratio, sqrt(3) - 1
MASK = np.uint64(0xFFFFFFFF)
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on broadcastable arrays of 32-bit words; -> four uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) & MASK
                                                   for v in (c0, c1, c2, c3, k0, k1)))
    m0, m1, w0, w1, s32 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & MASK, (p0 >> s32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + w0) & MASK, (k1 + w1) & MASK
    return c0, c1, c2, c3


def block(seed, step, gid, q):
    """The four words of the block normal4 / go1o_uniform draw for (seed, step, global env, group)."""
    seed, step = np.asarray(seed, dtype=np.uint64), np.asarray(step, dtype=np.uint64)
    s32 = np.uint64(32)
    return philox4x32_10(gid, q, step & MASK, step >> s32, seed & MASK, seed >> s32)


def uniform_u1(x):
    """(f32(x >> 8) + 0.5f) * 2^-24 in float32: in (0, 1]; 1.0 where x >> 8 >= 2^23 is odd-rounded-up (the + 0.5f is
    not representable there and rounds to even)."""
    m = (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)
    return (m + np.float32(0.5)) * np.float32(2.0 ** -24)


def uniform_u2(x):
    """f32(x >> 8) * 2^-24 in float32: in [0, 1)."""
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def box_muller(u1, u2):
    """float64 Box-Muller of float32 uniforms -> (r cos, r sin)."""
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    a = 2.0 * np.pi * u2
    return r * np.cos(a), r * np.sin(a)


def uniforms(seed, step, n, env_id_offset=0, groups=4):
    """-> u1, u2 float32 (n, groups, 2): the uniforms of pair p of group q of env e (global id e + env_id_offset)."""
    gid = (np.arange(n, dtype=np.uint64) + np.uint64(env_id_offset))[:, None]
    x = block(seed, step, gid, np.arange(groups, dtype=np.uint64)[None, :])
    u1 = np.stack([uniform_u1(x[0]), uniform_u1(x[2])], axis=-1)
    u2 = np.stack([uniform_u2(x[1]), uniform_u2(x[3])], axis=-1)
    return u1, u2


def normal(seed, step, n, env_id_offset=0, groups=4):
    """-> z float64 (n, 4 * groups): the draws of the n envs' actions 0 .. 4 groups - 1."""
    u1, u2 = uniforms(seed, step, n, env_id_offset, groups)
    zc, zs = box_muller(u1, u2)
    return np.stack([zc, zs], axis=-1).reshape(n, 4 * groups)


def log_prob(z, std):
    """float64 sum over the real actions of log N(mean + std z; mean, std): z (n, >= len(std)), std (na,)."""
    std = np.asarray(std, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)[:, :len(std)]
    return (-0.5 * z * z - np.log(std) - LOG_SQRT_2PI).sum(-1)


def log_prob_f32_grouped(z32, std32, pairwise=True):
    """log_prob in float32 from the kernel's own float32 z, in the kernel's operation order: a partial sum per group
    of four actions in action order, then (lp0 + lp1) + (lp2 + lp3) (pairwise) or ((lp0 + lp1) + lp2) + lp3.  Every
    step is one f32 operation except the log of std (float64 log rounded to f32 here, the hardware's in the kernel):
    with std = 1 that term is exactly 0 on both sides and the result is the kernel's bits in the kernel's grouping."""
    f = np.float32
    z32 = np.asarray(z32, dtype=f)
    na = len(std32)
    ls = np.log(np.asarray(std32, dtype=np.float64)).astype(f)
    lp = np.zeros((z32.shape[0], 4), dtype=f)
    for a in range(na):
        t = (f(-0.5) * z32[:, a]) * z32[:, a] - ls[a] - f(0.91893853320467274)
        lp[:, a // 4] = lp[:, a // 4] + t
    if pairwise:
        return (lp[:, 0] + lp[:, 1]) + (lp[:, 2] + lp[:, 3])
    return ((lp[:, 0] + lp[:, 1]) + lp[:, 2]) + lp[:, 3]


def coverage(seed, steps, n, env_id_offset=0):
    """What the draws of `steps` contain, from the reference alone: (#|z| > 4, the smallest distance of a u2 to each
    of the quadrant boundaries 0, 1/4, 1/2, 3/4, the largest u1)."""
    big, near, top = 0, np.full(4, np.inf), 0.0
    for s in steps:
        u1, u2 = uniforms(seed, s, n, env_id_offset)
        big += int((np.abs(normal(seed, s, n, env_id_offset)) > 4.0).sum())
        for i, b in enumerate((0.0, 0.25, 0.5, 0.75)):
            near[i] = min(near[i], float(np.abs(u2.astype(np.float64) - b).min()))
        top = max(top, float(u1.max()))
    return big, near, top
