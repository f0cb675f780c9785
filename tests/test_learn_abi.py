"""The rollout and PPO-engine libraries' C ABIs (include/go1_rollout.h, include/go1_ppo.h) against their ctypes
mirrors (legged_tracking_amd/learn_abi.py): exported symbols, ABI versions, struct sizes, the loader's version
check and the argument errors.  No GPU, no compute calls."""
import ctypes as C
import os
import re

import pytest

from legged_tracking_amd import learn_abi as LA, native, ppo_engine as PE, rollout as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIBS = {
    "rollout": dict(lib=R.lib, path=R.LIB_PATH, header="go1_rollout.h", prefix="go1_rollout",
                    version=LA.GO1_ROLLOUT_ABI_VERSION, argtypes=LA.ROLLOUT_ARGTYPES,
                    mirrors=(LA.Transition, LA.PolicyLayer, LA.PolicyArgs), min_functions=8),
    "ppo": dict(lib=PE.load_library, path=PE.LIB_PATH, header="go1_ppo.h", prefix="go1_ppo",
                version=LA.GO1_PPO_ABI_VERSION, argtypes=LA.PPO_ARGTYPES,
                mirrors=(LA.PPODims, None, LA.PPOBufs), min_functions=10),
}


def _header(s):
    return open(os.path.join(REPO, "include", s["header"])).read()


@pytest.mark.parametrize("name", LIBS)
def test_every_declared_function_is_exported(name):
    s = LIBS[name]
    names = sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(go1_\w+)\s*\(", _header(s), re.M)))
    assert len(names) >= s["min_functions"] and set(s["argtypes"]) <= set(names)
    for n in (s["prefix"] + "_abi_version", s["prefix"] + "_abi_sizes", s["prefix"] + "_last_error"):
        assert n in names
    l = s["lib"]()
    for n in names:
        assert hasattr(l, n), n


@pytest.mark.parametrize("name", LIBS)
def test_abi_version_and_struct_sizes_match_the_mirrors(name):
    s = LIBS[name]
    l = s["lib"]()
    assert s["lib"]() is l  # one handle per process
    consts = dict(re.findall(r"#define (GO1_\w+) (\d+)", _header(s)))
    assert getattr(l, s["prefix"] + "_abi_version")() == s["version"]
    assert int(consts[s["prefix"].upper() + "_ABI_VERSION"]) == s["version"]
    out = (C.c_int64 * 3)()
    getattr(l, s["prefix"] + "_abi_sizes")(out)
    want = [C.sizeof(m) if m is not None else 4 * len(LA.HYPER_FIELDS) for m in s["mirrors"]]
    assert list(out) == want


def test_header_constants_match_the_mirror():
    r = dict(re.findall(r"#define (GO1_\w+) (\d+)", _header(LIBS["rollout"])))
    p = dict(re.findall(r"#define (GO1_\w+) (\d+)", _header(LIBS["ppo"])))
    assert int(r["GO1_POLICY_LAYERS"]) == LA.GO1_POLICY_LAYERS == len(LA.POLICY_LINEARS)
    assert int(p["GO1_PPO_AUX"]) == LA.GO1_PPO_AUX == PE.NAUX
    hyper = re.search(r"typedef struct go1_ppo_hyper \{(.*?)\} go1_ppo_hyper;", _header(LIBS["ppo"]), re.S).group(1)
    fields = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", hyper, flags=re.S))
    assert tuple(fields) == LA.HYPER_FIELDS
    # the shape table follows the header's hidden widths
    ha1, ha2, h1, h2, h3 = (int(p["GO1_PPO_" + k]) for k in ("HA1", "HA2", "H1", "H2", "H3"))
    assert LA.policy_shapes(261, 2, 12) == [(ha1, 261), (ha2, ha1), (2, ha2), (h1, 263), (h2, h1), (h3, h2), (12, h3),
                                            (h1, 263), (h2, h1), (h3, h2), (1, h3)]


def test_policy_description_matches_the_module():
    ac = R.ActorCritic(70, 2, 261, 12)
    lin = LA.policy_linears(ac)
    assert [tuple(m.weight.shape) for m in lin] == LA.policy_shapes(261, 2, 12)
    sd = list(ac.state_dict())
    assert PE.PARAM_NAMES == [k for k in sd if k != "std"] + ["std"] and sd[0] == "std"
    assert PE.PARAM_NAMES[:PE.N_ADAPT_TENSORS] == [k for k in sd if k.startswith("adaptation_module.")]
    assert R.FusedPolicy.supported(ac) and PE.supported(ac)
    assert not R.FusedPolicy.supported(R.ActorCritic(70, 9, 261, 12))  # latent wider than 8
    assert not PE.supported(R.ActorCritic(70, 2, 261, 17))  # more than 16 actions


@pytest.mark.parametrize("name", LIBS)
def test_loader_refuses_another_abi_version(name):
    s = LIBS[name]
    with pytest.raises(native.NativeError, match="ABI version mismatch"):
        native.load_library(s["path"], s["prefix"] + "_abi_version", s["version"] + 1, s["prefix"] + "_last_error",
                            s["argtypes"])
    with pytest.raises(native.NativeError, match="missing"):
        native.load_library(s["path"] + ".absent", s["prefix"] + "_abi_version", s["version"],
                            s["prefix"] + "_last_error", s["argtypes"])


def test_null_arguments_are_reported_not_thrown():
    l = R.lib()
    assert l.go1_policy_forward(None, None) == -1
    assert b"go1_policy_forward: bad argument" in l.go1_rollout_last_error()
    assert l.go1_record_transition(None, 16, 0.0, None) == -1
    assert b"go1_record_transition: bad argument" in l.go1_rollout_last_error()
    assert l.go1_gae(None, None, None, None, None, None, None, 24, 16, 0.99, 0.95, None) == -1
    assert l.go1_colsum(None, 64, 8, None, 1, None, None) == -1
    with pytest.raises(native.NativeError, match="go1_colsum: bad argument"):
        native.check(l, -1)
    p = PE.load_library()
    assert p.go1_ppo_param_count(None, None, None) == -1
    assert b"dims outside the supported architecture" in p.go1_ppo_last_error()
    d = LA.PPODims(hist=261, priv=2, actions=12, mb=384, rows=1536)
    for phase in (0, 1):
        assert p.go1_ppo_grad(C.byref(d), None, phase, None) == -1
        assert b"params, grads, hyper and work are required" in p.go1_ppo_last_error()
        assert p.go1_ppo_step(C.byref(d), None, phase, None) == -1
    assert p.go1_ppo_pack(None, None, None) == -1


def test_policy_forward_refuses_variant_1_outside_nine_k_groups():
    """go1_policy_forward's argument checks run before any HIP call: the single-workgroup policy kernel
    walks a compile-time nine packed 32-deep K groups, so a history narrower than 257 (fewer packed
    groups: its reads would leave the weight buffer) or wider than 288 inputs is refused."""
    lib = R.lib()
    a = LA.PolicyArgs(num_actions=12, num_priv=2, n_envs=16, variant=1)
    a.obs_history = a.privileged_obs = a.action_mean = a.value = 16  # never dereferenced: refused first
    for i in range(11):
        a.layers[i].w = a.layers[i].b = a.layers[i].wf = 16
    for hist, msg in ((210, b"257..286"), (256, b"257..286"), (287, b"257..286"), (300, b"got 300")):
        a.hist_dim, a.hist_ld = hist, hist
        assert lib.go1_policy_forward(C.byref(a), None) != 0
        assert msg in lib.go1_rollout_last_error(), hist
