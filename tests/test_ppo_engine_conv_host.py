"""The PPO update engine's CNN encoder mode (go1_ppo_dims.enc_mode = GO1_PPO_ENC_CNN = 3) on the host, no GPU: the
flat parameter layout and the phase-1 slice against rollout_cnn.ActorCritic with use_cnn, the workspace query, every
new refusal, the plain module's and the MLP mode's numbers unchanged, the truth table of
ppo_engine.conv_encoder_supported, the switch, and the header's constants against their mirrors.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import learn_abi as LA, ppo_engine as PE, rollout as R, rollout_cnn as RC  # noqa: E402
from tests.test_ppo_engine_encoder_host import PLAIN  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1  # GO1_PPO_E_ARG
N_MAP, S = 3782, 41
# the MLP mode: (hist, priv, actions, mb, rows, num_obs, n_map, n_embed) -> (parameters, adaptation slice, workspace
# bytes), recorded from a build of the commit before the CNN mode
MLP = {
    (503, 2, 12, 37, 50, 503, 462, 256): (983579, 304258, 19453952),
    (1006, 2, 12, 384, 1536, 503, 462, 256): (983579, 304258, 47341568),
    (71, 8, 16, 131, 200, 71, 30, 128): (683689, 128776, 24356864),
    (4099, 2, 12, 130, 200, 4099, 4096, 512): (2210075, 1346434, 49067008),
    (2515, 2, 12, 24576, 98304, 503, 462, 256): (983579, 304258, 731583488),
}


def _module(E=256, frames=1, shape=(2, 61, 31), priv=2, na=12, use_cnn=True, **kw):
    args = type("A", (RC.AC_Args,), dict(height_map_shape=shape, cnn_num_embedding=E, use_cnn=use_cnn, **kw))
    num_obs = S + int(np.prod(shape))
    return RC.ActorCritic(num_obs, priv, frames * num_obs, na, ac_args=args)


def _dims(**kw):
    base = dict(hist=S + N_MAP, priv=2, actions=12, mb=37, rows=50, enc_mode=LA.GO1_PPO_ENC_CNN, num_obs=S + N_MAP,
                n_map=N_MAP, n_embed=256)
    base.update(kw)
    return LA.PPODims(**base)


def _query(d):
    lib = PE.load_library()
    tot, ad, nb = C.c_int64(), C.c_int64(), C.c_int64()
    rc = (lib.go1_ppo_param_count(C.byref(d), C.byref(tot), C.byref(ad)),
          lib.go1_ppo_workspace_bytes(C.byref(d), C.byref(nb)))
    return rc, (tot.value, ad.value, nb.value)


@pytest.mark.parametrize("E,frames", [(128, 1), (512, 1), (128, 2), (512, 2)])
def test_param_count_and_phase1_slice_match_the_module(E, frames):
    ac = _module(E, frames)
    assert PE.conv_encoder_supported(ac) and not PE.encoder_supported(ac) and not PE.supported(ac)
    rc, (tot, ad, nb) = _query(_dims(hist=ac.num_obs_history, n_embed=E))
    assert rc == (0, 0) and nb > 0
    sd = dict(ac.named_parameters())
    names = PE.CONV_PARAM_NAMES + PE.PARAM_NAMES
    assert sorted(names) == sorted(sd)
    assert tot == sum(p.numel() for p in ac.parameters()) == sum(sd[k].numel() for k in names)
    lead = names[:len(PE.CONV_PARAM_NAMES) + PE.N_ADAPT_TENSORS]
    assert all(k.startswith(("height_map_encoder.", "adaptation_module.")) for k in lead)
    assert ad == sum(sd[k].numel() for k in lead) == (sum(p.numel() for p in ac.height_map_encoder.parameters()) +
                                                      sum(p.numel() for p in ac.adaptation_module.parameters()))
    # the flat order is the module's: conv1, conv2, linear
    assert [tuple(sd[k].shape) for k in PE.CONV_PARAM_NAMES] == [(16, 2, 3, 3), (16,), (32, 16, 3, 3), (32,),
                                                                 (E, 3360), (E,)]


def test_workspace_grows_with_the_mini_batch():
    sizes = []
    for mb in (5, 37, 257, 4096, 24576):
        rc, (_, _, nb) = _query(_dims(mb=mb, rows=max(50, 4 * mb)))
        assert rc == (0, 0)
        sizes.append(nb)
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # the features and their gradient alone are 2 x 24576 rows x ~3400 floats
    assert sizes[-1] > 2 * 24576 * 3360 * 4


@pytest.mark.parametrize("kw,msg", [
    (dict(n_map=3781, num_obs=S + 3781, hist=S + 3781), b"n_map 3781 is not implemented"),
    (dict(n_embed=200), b"n_embed 200 is not implemented"),
    (dict(hist=S + N_MAP + 1), b"hist 3824 is not a multiple of num_obs 3823"),
    (dict(enc_mode=2), b"enc_mode 2 is not implemented"),
    (dict(enc_mode=4), b"enc_mode 4 is not implemented"),
])
def test_refusals(kw, msg):
    lib = PE.load_library()
    d = _dims(**kw)
    assert _query(_dims())[0] == (0, 0)
    assert lib.go1_ppo_param_count(C.byref(d), None, None) == E_ARG
    assert msg in lib.go1_ppo_last_error(), lib.go1_ppo_last_error()
    assert lib.go1_ppo_workspace_bytes(C.byref(d), None) == E_ARG
    for phase in (0, 1):  # refused before any buffer is looked at
        assert lib.go1_ppo_grad(C.byref(_dims(**kw)), C.byref(LA.PPOBufs()), phase, None) == E_ARG
        assert msg in lib.go1_ppo_last_error()
        assert lib.go1_ppo_step(C.byref(_dims(**kw)), C.byref(LA.PPOBufs()), phase, None) == E_ARG
    assert lib.go1_ppo_pack(C.byref(d), C.byref(LA.PPOBufs()), None) == E_ARG


def test_the_plain_module_and_the_mlp_mode_are_unchanged():
    for (hist, priv, na, mb, rows), want in PLAIN.items():
        rc, got = _query(LA.PPODims(hist=hist, priv=priv, actions=na, mb=mb, rows=rows))
        assert rc == (0, 0) and got == want
    for (hist, priv, na, mb, rows, num_obs, n_map, E), want in MLP.items():
        rc, got = _query(LA.PPODims(hist=hist, priv=priv, actions=na, mb=mb, rows=rows, enc_mode=LA.GO1_PPO_ENC_MLP,
                                    num_obs=num_obs, n_map=n_map, n_embed=E))
        assert rc == (0, 0) and got == want


def test_conv_encoder_supported_truth_table():
    assert PE.conv_encoder_supported(_module())  # the class defaults with use_cnn
    assert tuple(RC.AC_Args.height_map_shape) == (2, 61, 31) and RC.AC_Args.cnn_num_embedding == 256
    for E in (128, 256, 384, 512):
        assert PE.conv_encoder_supported(_module(E, frames=5))
    assert not PE.conv_encoder_supported(_module(32))
    assert not PE.conv_encoder_supported(_module(528))
    assert RC.cnn_feature_count((2, 60, 28)) == RC.CNN_FEATURES  # the module accepts it; the engine's dims cannot say it
    assert not PE.conv_encoder_supported(_module(shape=(2, 60, 28)))
    assert not PE.conv_encoder_supported(_module(na=17))
    assert not PE.conv_encoder_supported(_module(priv=9))
    assert not PE.conv_encoder_supported(_module(actor_hidden_dims=[256, 256, 128]))
    assert not PE.conv_encoder_supported(_module(activation="tanh"))
    mlp = _module(shape=(2, 21, 11), use_cnn=False)
    assert PE.encoder_supported(mlp) and not PE.conv_encoder_supported(mlp)
    plain = R.ActorCritic(70, 2, 261, 12)
    assert PE.supported(plain) and not PE.conv_encoder_supported(plain)
    assert not PE.encoder_supported(_module())  # the MLP check stays False for the CNN module


def test_the_switch(monkeypatch):
    assert RC.ENGINE_DEFAULT == {"mlp": False, "cnn": False}
    ac = _module(128)
    monkeypatch.delenv("GO1_PPO_ENCODER_ENGINE", raising=False)
    assert not RC.encoder_engine_on(ac)
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    assert RC.encoder_engine_on(ac)
    monkeypatch.setitem(RC.ENGINE_DEFAULT, "cnn", True)
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "0")
    assert not RC.encoder_engine_on(ac)
    monkeypatch.delenv("GO1_PPO_ENCODER_ENGINE")
    assert RC.encoder_engine_on(ac)
    # PPO._engine_on: no engine on the CPU whatever the switch says; on a GPU it follows the switch
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    alg = R.PPO(ac, device="cpu")
    assert not alg._engine_on() and alg._engine is None
    alg.device = "cuda:0"  # the device word alone: _engine_on builds nothing
    assert alg._engine_on()
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "0")
    assert not alg._engine_on()
    monkeypatch.setenv("GO1_PPO_ENCODER_ENGINE", "1")
    alg.actor_critic = _module(shape=(2, 60, 28))  # an unsupported shape keeps the torch path
    assert not alg._engine_on()


def test_header_constants_agree_with_the_mirrors():
    lib = PE.load_library()
    header = open(os.path.join(REPO, "include", "go1_ppo.h")).read()
    consts = dict(re.findall(r"#define (GO1_\w+) (\d+)", header))
    assert lib.go1_ppo_abi_version() == LA.GO1_PPO_ABI_VERSION == int(consts["GO1_PPO_ABI_VERSION"]) == 2
    assert C.sizeof(LA.PPODims) == 40
    assert int(consts["GO1_PPO_ENC_CNN"]) == LA.GO1_PPO_ENC_CNN == 3 and int(consts["GO1_PPO_ENC_MLP"]) == 1
    assert LA.CNN_FEATURES == RC.CNN_FEATURES == RC.cnn_feature_count(LA.CNN_MAP_SHAPE)
    assert int(np.prod(LA.CNN_MAP_SHAPE)) == N_MAP
    assert PE.CONV_PARAM_NAMES == [f"height_map_encoder.model.{i}.{k}" for i in (0, 3, 7) for k in ("weight", "bias")]
    assert PE.ENC_PARAM_NAMES == [f"height_map_encoder.model.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")]
