"""The PPO update engine's host code against a recording of the build before csrc/ppo_update.hip was split into
headers and its launch plumbing replaced by one layer table (tests/golden/ppo_replay/ppo_replay.json, written by
tests/golden/make_golden_ppo_replay.py on the GPU; the file names the commit it was recorded from).

That change moves no kernel (profiles/ppo_split/asm_diff.txt: the device code is identical), so what can differ is
what the host computes: the workspace layout and every launch's arguments.  Two parts:

  layout   no GPU: go1_ppo_param_count (total, adaptation slice) and go1_ppo_workspace_bytes of every case, at the
           case's mb / rows and at mb 24576 of 98304 rows.  The workspace total is a sum of independently rounded
           sizes: reordering buffers does not change it, another size does.
  update   on a fresh engine per case: start() (_bind, _write_hyper, pack, idx), then grad(0), step(0), grad(1),
           step(1) twice with the same idx; after each of the eight calls the sha256 of the raw bytes of grads,
           params, the four moment buffers, steps, lr and losses.  The second round runs on the max slots that
           finalize_kernel cleared and on the images of the phase-1 re-pack, both driven by the layer table.  The
           engine is deterministic from run to run (test_fresh_engines_agree_bitwise_*), so every digest is equal
           to the recorded one: there is no tolerance.

The inputs (the storage tensors, the initial parameters, idx) are digested too and compared first, under their own
message: they come from torch's generators and its f64 forward, so another torch can move them, and that is then
reported as input drift and not as an engine change.

Cases: the smallest shapes that reach every row of the layer table and its edges.  Plain module
(tests/test_ppo_engine_grad.SHAPES): smallest, widest_head_latent, checkpoint_latent_padded_ldg, velocity_window1
(hist_ld > hist).  Encoder module (tests/test_ppo_engine_encoder_grad.SHAPES): production, small_map, caps, window.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from legged_tracking_amd import learn_abi as LA, ppo_engine as PE  # noqa: E402
from tests import golden_io as G  # noqa: E402
from tests import test_ppo_engine_encoder_grad as ENC, test_ppo_engine_grad as PLAIN  # noqa: E402
from tests.ppo_cases import _Case, _args  # noqa: E402

FIXTURE = os.path.join(G.GOLDEN, "ppo_replay", "ppo_replay.json")
CASES = [("plain", n) for n in ("smallest", "widest_head_latent", "checkpoint_latent_padded_ldg", "velocity_window1")] \
    + [("encoder", n) for n in ("production", "small_map", "caps", "window")]
IDS = [f"{m}-{n}" for m, n in CASES]
BIG = (24576, 98304)  # the production mini-batch: mb, rows
ROUNDS = 2
CALLS = [f"round{r}/{fn}({ph})" for r in range(ROUNDS) for ph in (0, 1) for fn in ("grad", "step")]
BUFFERS = ("grads", "params", "exp_avg", "exp_avg_sq", "ad_exp_avg", "ad_exp_avg_sq", "steps", "lr", "losses")
STORAGE = ("observation_histories", "privileged_observations", "actions", "values", "advantages", "returns",
           "actions_log_prob", "mu", "sigma")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _rows(mb):
    return mb + max(3, mb // 7)  # _Case's storage


def dims(case, mb=None, rows=None):
    """go1_ppo_dims of a case (no module is built), at its own mini-batch or at (mb, rows)."""
    module, name = case
    if module == "plain":
        hist, priv, na, mb0 = PLAIN.SHAPES[name]
        enc = {}
    else:
        shape, E, S, frames, priv, na, mb0, _ = ENC.SHAPES[name]
        n_map = int(np.prod(shape))
        hist = frames * (S + n_map)
        enc = dict(enc_mode=LA.GO1_PPO_ENC_MLP, num_obs=S + n_map, n_map=n_map, n_embed=E)
    mb = mb0 if mb is None else mb
    return LA.PPODims(hist=hist, priv=priv, actions=na, mb=mb, rows=_rows(mb) if rows is None else rows, **enc)


def layout(case):
    """{param_count: [total, adaptation], workspace_bytes: [at the case's mb, at BIG]} from the library."""
    lib = PE.load_library()
    tot, ad, nb = C.c_int64(), C.c_int64(), C.c_int64()
    out = {"workspace_bytes": []}
    for d in (dims(case), dims(case, *BIG)):
        assert lib.go1_ppo_param_count(C.byref(d), C.byref(tot), C.byref(ad)) == 0
        assert lib.go1_ppo_workspace_bytes(C.byref(d), C.byref(nb)) == 0
        out["param_count"] = [tot.value, ad.value]
        out["workspace_bytes"].append(nb.value)
    return out


def build_case(case):
    module, name = case
    if module == "plain":
        hist, priv, na, mb = PLAIN.SHAPES[name]
        return _Case(hist, priv, na, mb, window=PLAIN.WINDOW.get(name, 0))
    return ENC._case(name)


def replay(case):
    """{inputs: {name: sha256}, calls: {call: {buffer: sha256}}} of one case on a fresh engine."""
    with _args():
        c = build_case(case)
        e = c.eng
        d = dims(case)
        assert (e.hist, e.priv, e.na, c.mb, c.rows) == (d.hist, d.priv, d.actions, d.mb, d.rows)
        inputs = {k: _sha(getattr(c.storage, k)) for k in STORAGE}
        inputs["params"] = _sha(e.params)
        inputs["idx"] = _sha(c.idx)
        c.start()
        assert (e.dims.enc_mode, e.dims.num_obs, e.dims.n_map, e.dims.n_embed) == (d.enc_mode, d.num_obs, d.n_map,
                                                                                   d.n_embed)
        calls = {}
        for r in range(ROUNDS):
            for ph in (0, 1):
                for fn in ("grad", "step"):
                    getattr(e, fn)(ph)
                    torch.cuda.synchronize()
                    calls[f"round{r}/{fn}({ph})"] = {k: _sha(getattr(e, k)) for k in BUFFERS}
        assert e.steps.tolist() == [float(ROUNDS), float(ROUNDS)]
    return {"inputs": inputs, "calls": calls}


def _recorded(case):
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert len(fx["recorded_from"]) == 40, "the fixture names the commit it was recorded from"
    return fx["cases"]["-".join(case)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_layout_is_the_recorded_one(case):
    assert layout(case) == _recorded(case)["layout"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_update_replays_recording_bit_for_bit(case):
    ref = _recorded(case)
    got = replay(case)
    drift = [k for k in ref["inputs"] if got["inputs"].get(k) != ref["inputs"][k]]
    assert sorted(got["inputs"]) == sorted(ref["inputs"]) and not drift, \
        f"input drift (the case's data is not the recorded one; nothing is said about the engine): {drift}"
    assert list(got["calls"]) == CALLS == list(ref["calls"])
    bad = [(call, k) for call in CALLS for k in BUFFERS if got["calls"][call][k] != ref["calls"][call][k]]
    # the window holds what it is meant to: every call moved something, the second round is not the first again
    for a, b in zip(CALLS, CALLS[1:]):
        assert ref["calls"][a] != ref["calls"][b], (a, b)
    print(f"{'-'.join(case)}: {len(CALLS) * len(BUFFERS)} digests compared, {len(bad)} differ")
    assert not bad, bad
