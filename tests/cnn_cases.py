"""The cases of the height-map encoder fixtures (tests/golden/ppo_cnn_<case>.npz) and the seeded generators of
everything large in them.

A state dict of the default head widths is 4 MB and a 40-row history of the 61 x 31 map 1.2 MB, more than a
committed file may hold, so the fixtures keep the reference's OUTPUTS (and every small array) while weights and
histories are drawn here from numpy's PCG64 streams, by the generator (tests/golden/make_golden_cnn.py, which
loads them into the reference's module) and by the tests alike.  The fixture records each tensor's key, shape
and |sum| so that a test notices a stream that no longer matches.  Updated weights of one PPO.update are kept
whole for tensors up to SAMPLE_ABOVE elements and at N_SAMPLE seeded positions for the larger ones.
"""
import numpy as np

NUM_SCALAR = 41   # 503 - 2 * 21 * 11: the scalar part of an observation frame (scripts/train.py:53)
NUM_PRIV, NUM_ACTIONS = 2, 12
CASES = {
    #            map shape     E    H   n  use_cnn
    "mlp":       ((2, 21, 11), 256, 2, 40, False),
    "mlp_small": ((2, 5, 3),   40,  1, 40, False),
    "cnn":       ((2, 61, 31), 32,  2, 40, True),
}
UPDATE_CASES = ("mlp", "cnn")
UPD_N, UPD_T, UPD_EPOCHS, UPD_MINI_BATCHES = 32, 4, 2, 4
SAMPLE_ABOVE, N_SAMPLE = 32768, 8192


def dims(case):
    shape, E, H, n, use_cnn = CASES[case]
    num_obs = NUM_SCALAR + int(np.prod(shape))
    return dict(shape=shape, E=E, H=H, n=n, use_cnn=use_cnn, num_obs=num_obs, num_hist=H * num_obs,
                policy_input=2 * NUM_SCALAR + E)


def _seed(case, what):
    return [list(CASES).index(case), what]


def make_hist(case, rows, what=0):
    """(rows, H * num_obs) f32 history: scalars N(0, 1), map columns U(-5, 5)."""
    d = dims(case)
    g = np.random.default_rng(_seed(case, 100 + what))
    x = g.normal(0, 1, (rows, d["H"], d["num_obs"]))
    x[:, :, NUM_SCALAR:] = g.uniform(-5, 5, (rows, d["H"], d["num_obs"] - NUM_SCALAR))
    return x.reshape(rows, -1).astype(np.float32)


def make_small_inputs(case):
    d = dims(case)
    g = np.random.default_rng(_seed(case, 200))
    return (g.normal(0, 1, (d["n"], NUM_PRIV)).astype(np.float32),
            g.normal(0, 1, (d["n"], NUM_ACTIONS)).astype(np.float32))


def make_state_dict(case, keys, shapes):
    """Weights U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), biases U(-0.1, 0.1), std 0.7, as numpy f32 by key."""
    sd = {}
    for i, (k, s) in enumerate(zip(keys, shapes)):
        g = np.random.default_rng(_seed(case, 1000 + i))
        s = tuple(int(v) for v in s)
        if k == "std":
            sd[k] = np.full(s, 0.7, np.float32)
        elif k.endswith(".weight"):
            b = 1.0 / np.sqrt(np.prod(s[1:]))
            sd[k] = g.uniform(-b, b, s).astype(np.float32)
        else:
            sd[k] = g.uniform(-0.1, 0.1, s).astype(np.float32)
    return sd


def sample_index(case, i, numel):
    """The positions of tensor i (of numel > SAMPLE_ABOVE elements) whose updated values a fixture keeps."""
    return np.sort(np.random.default_rng(_seed(case, 5000 + i)).choice(numel, N_SAMPLE, replace=False))


def ac_args(base, case):
    """A plain class with `base`'s (an AC_Args class's) public attributes and the case's encoder settings."""
    d = dims(case)
    attrs = {k: getattr(base, k) for k in dir(base) if not k.startswith("_")}
    attrs.update(use_cnn=d["use_cnn"], use_gru=False, height_map_shape=d["shape"], cnn_num_embedding=d["E"])
    return type("AC_Args_" + case, (), attrs)
