"""The PPO update engine's encoder layout (go1_ppo_dims.enc_mode, ABI 2) and the host's support checks, without a GPU:
parameter counts and the phase-1 slice against rollout_cnn.ActorCritic, the workspace query, every refusal with its
message, the plain module's numbers unchanged, ppo_engine.encoder_supported and the switch PPO._engine_on consults."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from legged_tracking_amd import learn_abi as LA, ppo_engine as PE, rollout as R, rollout_cnn as RC
from tests import cnn_cases as CC
from tests.test_actor_critic_cnn import load_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (map shape, E, scalars per frame, frames)
ENC_CASES = [((2, 21, 11), 256, 41, 2), ((2, 5, 3), 128, 41, 1), ((2, 64, 32), 512, 3, 1)]
E_ARG = -1  # GO1_PPO_E_ARG
# (hist, priv, actions, mb, rows) -> (parameters, adaptation slice, workspace bytes) of ABI 1, recorded before the
# encoder fields existed
PLAIN = {
    (261, 2, 12, 384, 1536): (700699, 100226, 36771840),
    (2100, 2, 12, 16389, 20000): (3054619, 571010, 501934080),
    (70, 8, 16, 131, 200): (463657, 52104, 19620864),
    (1, 1, 1, 5, 5): (365316, 33537, 8980480),
    (1020, 6, 12, 24576, 98304): (1676831, 295046, 605826048),
}


def _module(shape, E, S, frames=1, priv=2, na=12, **kw):
    args = type("A", (RC.AC_Args,), dict(height_map_shape=shape, cnn_num_embedding=E, **kw))
    num_obs = S + int(np.prod(shape))
    return RC.ActorCritic(num_obs, priv, frames * num_obs, na, ac_args=args)


def _query(d):
    lib = PE.load_library()
    tot, ad, nb = C.c_int64(), C.c_int64(), C.c_int64()
    rc = (lib.go1_ppo_param_count(C.byref(d), C.byref(tot), C.byref(ad)),
          lib.go1_ppo_workspace_bytes(C.byref(d), C.byref(nb)))
    return rc, (tot.value, ad.value, nb.value)


@pytest.mark.parametrize("shape,E,S,frames", ENC_CASES)
def test_param_count_and_phase1_slice_match_the_module(shape, E, S, frames):
    ac = _module(shape, E, S, frames)
    assert PE.encoder_supported(ac) and not PE.supported(ac)
    d = LA.PPODims(hist=ac.num_obs_history, priv=2, actions=12, mb=37, rows=50, enc_mode=LA.GO1_PPO_ENC_MLP,
                   num_obs=ac.num_obs, n_map=ac.num_map, n_embed=E)
    rc, (tot, ad, nb) = _query(d)
    assert rc == (0, 0) and nb > 0
    sd = dict(ac.named_parameters())
    names = PE.ENC_PARAM_NAMES + PE.PARAM_NAMES
    assert sorted(names) == sorted(sd)
    assert tot == sum(p.numel() for p in ac.parameters()) == sum(sd[k].numel() for k in names)
    # the adaptation optimizer's slice: encoder + adaptation module, the leading tensors of the engine's order
    lead = names[:len(PE.ENC_PARAM_NAMES) + PE.N_ADAPT_TENSORS]
    assert all(k.startswith(("height_map_encoder.", "adaptation_module.")) for k in lead)
    assert ad == sum(sd[k].numel() for k in lead) == (sum(p.numel() for p in ac.height_map_encoder.parameters()) +
                                                      sum(p.numel() for p in ac.adaptation_module.parameters()))
    assert list(sd)[0] == "std" and names[-1] == "std"  # the engine's order is its own


def _enc_dims(**kw):
    base = dict(hist=503, priv=2, actions=12, mb=37, rows=50, enc_mode=1, num_obs=503, n_map=462, n_embed=256)
    base.update(kw)
    return LA.PPODims(**base)


@pytest.mark.parametrize("kw,msg", [
    (dict(enc_mode=2), b"enc_mode 2 is not implemented"),
    (dict(enc_mode=-1), b"enc_mode -1 is not implemented"),
    (dict(n_embed=200), b"n_embed 200 is not implemented"),
    (dict(n_embed=0), b"n_embed 0 is not implemented"),
    (dict(n_embed=640), b"n_embed 640 is not implemented"),
    (dict(n_map=0), b"n_map 0 is not implemented"),
    (dict(n_map=4097, num_obs=5000, hist=5000), b"n_map 4097 is not implemented"),
    (dict(n_map=504), b"n_map 504 is not implemented"),
    (dict(hist=504), b"hist 504 is not a multiple of num_obs 503"),
])
def test_refusals(kw, msg):
    lib = PE.load_library()
    d = _enc_dims(**kw)
    assert _query(_enc_dims())[0] == (0, 0)
    assert lib.go1_ppo_param_count(C.byref(d), None, None) == E_ARG
    assert msg in lib.go1_ppo_last_error(), lib.go1_ppo_last_error()
    assert lib.go1_ppo_workspace_bytes(C.byref(d), None) == E_ARG
    for phase in (0, 1):  # refused before any buffer is looked at
        bigger = _enc_dims(**kw)
        assert lib.go1_ppo_grad(C.byref(bigger), C.byref(LA.PPOBufs()), phase, None) == E_ARG
        assert msg in lib.go1_ppo_last_error()
        assert lib.go1_ppo_step(C.byref(bigger), C.byref(LA.PPOBufs()), phase, None) == E_ARG
    assert lib.go1_ppo_pack(C.byref(d), C.byref(LA.PPOBufs()), None) == E_ARG


def test_zero_encoder_fields_are_the_plain_module():
    for (hist, priv, na, mb, rows), want in PLAIN.items():
        d = LA.PPODims(hist=hist, priv=priv, actions=na, mb=mb, rows=rows)
        assert (d.enc_mode, d.num_obs, d.n_map, d.n_embed) == (0, 0, 0, 0)
        rc, got = _query(d)
        assert rc == (0, 0) and got == want
        # the encoder fields are read with enc_mode 1 only
        rc, got = _query(LA.PPODims(hist=hist, priv=priv, actions=na, mb=mb, rows=rows, num_obs=7, n_map=3, n_embed=5))
        assert rc == (0, 0) and got == want


def test_encoder_supported_and_the_plain_check():
    for case in CC.CASES:
        ac = load_case(case)[1]
        assert not PE.supported(ac) and ac.graph_capture is False
        assert PE.encoder_supported(ac) == (case == "mlp")  # cnn: convolutions; mlp_small: E = 40
    assert not PE.encoder_supported(_module((2, 21, 11), 256, 41, activation="tanh"))
    assert not PE.encoder_supported(_module((2, 21, 11), 528, 41))
    assert not PE.encoder_supported(R.ActorCritic(70, 2, 261, 12))
    assert PE.supported(R.ActorCritic(70, 2, 261, 12))
    for E in (128, 256, 384, 512):
        assert PE.encoder_supported(_module((2, 21, 11), E, 41, frames=5))
    assert not PE.encoder_supported(_module((2, 21, 11), 256, 41, priv=9))
    assert not PE.encoder_supported(_module((2, 21, 11), 256, 41, na=17))
    assert not PE.encoder_supported(_module((2, 21, 11), 256, 41, actor_hidden_dims=[256, 256, 128]))
    assert not PE.encoder_supported(_module((2, 70, 30), 256, 41))  # 4200 map values


def test_the_switch(monkeypatch):
    assert RC.ENGINE_DEFAULT == {"mlp": False, "cnn": False}
    ac = load_case("mlp")[1]
    monkeypatch.delenv("GO1_PPO_ENCODER_ENGINE", raising=False)
    assert not RC.encoder_engine_on(ac)
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    assert RC.encoder_engine_on(ac)
    monkeypatch.setitem(RC.ENGINE_DEFAULT, "mlp", True)
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "0")
    assert not RC.encoder_engine_on(ac)
    monkeypatch.delenv("GO1_PPO_ENCODER_ENGINE")
    assert RC.encoder_engine_on(ac)
    # no engine on the CPU, whatever the switch says
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    alg = R.PPO(ac, device="cpu")
    assert not alg._engine_on() and alg._engine is None


def test_abi_version_and_sizes_agree_with_the_mirrors():
    lib = PE.load_library()
    header = open(os.path.join(REPO, "include", "go1_ppo.h")).read()
    consts = dict(re.findall(r"#define (GO1_\w+) (\d+)", header))
    assert lib.go1_ppo_abi_version() == LA.GO1_PPO_ABI_VERSION == int(consts["GO1_PPO_ABI_VERSION"]) == 2
    out = (C.c_int64 * 3)()
    lib.go1_ppo_abi_sizes(out)
    assert list(out) == [C.sizeof(LA.PPODims), 4 * len(LA.HYPER_FIELDS), C.sizeof(LA.PPOBufs)]
    assert C.sizeof(LA.PPODims) == 40
    dims = re.search(r"typedef struct go1_ppo_dims \{(.*?)\} go1_ppo_dims;", header, re.S).group(1)
    fields = re.findall(r"int(?:32|64)_t\s+(\w+);", re.sub(r"/\*.*?\*/", "", dims, flags=re.S))
    assert fields == [f[0] for f in LA.PPODims._fields_]
    assert (int(consts["GO1_PPO_ENC_MLP"]), int(consts["GO1_PPO_ENC_HIDDEN"]), int(consts["GO1_PPO_ENC_MAX_MAP"])) == \
        (LA.GO1_PPO_ENC_MLP, LA.GO1_PPO_ENC_HIDDEN, LA.GO1_PPO_ENC_MAX_MAP)
    assert LA.GO1_PPO_ENC_HIDDEN == RC.ENC_HIDDEN and max(PE.ENC_EMBEDDINGS) == int(consts["GO1_PPO_ENC_MAX_EMBED"])
    assert PE.ENC_PARAM_NAMES == [f"height_map_encoder.model.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")]
