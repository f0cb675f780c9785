"""Checkpoints that describe themselves: what a Runner checkpoint directory holds besides the weights, and how a
state dict is turned back into the module that wrote it.

  parameters.pkl   the run's Cfg as {section: {key: value}} (nested sections as nested dicts), plain data only:
                   what the reference's Runner pickles at construction (ppo_cse/__init__.py:81-84, the same in
                   ppo_cse_cnn) and scripts/eval.py:70-80 / play.load_cfg read back.  Runner.save() writes it.
  ac_weights.pt    the ActorCritic state dict.  Which learner wrote it is read off its keys (describe):
                     no height_map_encoder.* key                    actor_critic.ActorCritic (ppo_cse)
                     a 4-D height_map_encoder.model.0.weight        ActorCriticCNN, CNN encoder (ppo_cse_cnn)
                     otherwise                                      ActorCriticCNN, MLP encoder

load_actor_critic builds the module for an env's dimensions, with an AC_Args copy (the class-level AC_Args and
AC_Args_CNN of actor_critic are not touched), and refuses a state dict that does not fit what the Cfg implies.
"""
import os
import pickle

import numpy as np
import torch

from . import actor_critic as AC, config as CF

_TYPE_DICT = type.__dict__["__dict__"]


def find(logdir, name):
    """LOGDIR/name or LOGDIR/checkpoints/name, whichever exists (else None)."""
    for p in (os.path.join(logdir, name), os.path.join(logdir, "checkpoints", name)):
        if os.path.exists(p):
            return p
    return None


# ----------------------------------------------------------------------------- parameters.pkl
def _plain(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    if isinstance(v, (list, tuple)):
        return type(v)(_plain(x) for x in v)
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return v


def _section(cls):
    out = {}
    for c in reversed(cls.__mro__):
        if c is object:
            continue
        for k, v in _TYPE_DICT.__get__(c).items():
            if k.startswith("_") or isinstance(v, (staticmethod, classmethod, property)):
                continue
            if isinstance(v, type):
                out[k] = _section(v)
            elif not callable(v):
                out[k] = _plain(v)
    return out


def cfg_to_dict(cfg):
    """A Cfg class tree as {section: {key: value}}; a nested section (terrain.top, sim.physx) is a nested dict.
    The inverse of play.load_cfg's overlay."""
    return {k: v for k, v in _section(cfg).items() if isinstance(v, dict)}


def save_parameters(cfg, save_path):
    """Write save_path/parameters.pkl; returns the file's path."""
    path = os.path.join(save_path, "parameters.pkl")
    with open(path, "wb") as f:
        pickle.dump(cfg_to_dict(cfg), f)
    return path


# ----------------------------------------------------------------------------- the learner of a state dict
ENC0 = "height_map_encoder.model.0.weight"


def _linear_keys(sd, prefix):
    """The weight keys of the Linear layers of Sequential `prefix`, in order."""
    idx = sorted(int(k[len(prefix) + 1:].split(".")[0]) for k in sd
                 if k.startswith(prefix + ".") and k.endswith(".weight"))
    return [f"{prefix}.{i}.weight" for i in idx]


def describe(sd):
    """{"kind": "old" | "mlp" | "cnn", "embedding": E or None, "encoder_in": in_features or None,
    "encoder_key": the key that carries encoder_in} of a state dict."""
    if not any(k.startswith("height_map_encoder.") for k in sd):
        return {"kind": "old", "embedding": None, "encoder_in": None, "encoder_key": None}
    if ENC0 not in sd:
        raise ValueError(f"{ENC0}: the state dict has height_map_encoder.* keys but not this one")
    last = _linear_keys(sd, "height_map_encoder.model")[-1]
    if sd[ENC0].dim() == 4:
        return {"kind": "cnn", "embedding": int(sd[last].shape[0]), "encoder_in": int(sd[last].shape[1]),
                "encoder_key": last}
    return {"kind": "mlp", "embedding": int(sd[last].shape[0]), "encoder_in": int(sd[ENC0].shape[1]),
            "encoder_key": ENC0}


def _mismatch(key, have, want, cfg_side, why):
    return ValueError(f"{key}: the checkpoint has shape {tuple(have)}, {cfg_side} implies {tuple(want)} ({why})")


def load_actor_critic(logdir, cfg, num_obs, num_privileged_obs, num_obs_history, num_actions, device="cpu"):
    """The ActorCritic of LOGDIR's ac_weights.pt, in eval mode on `device`, for an env of the given dimensions built
    from `cfg`.  The class and the encoder come from the state dict (describe); cnn_num_embedding is the last
    encoder layer's out_features, height_map_shape the (2, rows, ny) of config.scan_grid(cfg), the hidden widths
    those of the state dict.  ValueError, naming the key, both shapes and which side says what, when the state
    dict does not fit the Cfg: the encoder's input against the grid, the heads' widths against the frame and the
    history, num_privileged_obs, num_actions."""
    weights = find(logdir, "ac_weights.pt")
    if weights is None:
        raise FileNotFoundError(f"no ac_weights.pt under {logdir}")
    side = "parameters.pkl" if find(logdir, "parameters.pkl") else "the default Cfg (there is no parameters.pkl)"
    sd = torch.load(weights, map_location=device, weights_only=True)
    d = describe(sd)
    ad, actor, critic = (_linear_keys(sd, p) for p in ("adaptation_module", "actor_body", "critic_body"))
    for name, keys in (("adaptation_module", ad), ("actor_body", actor), ("critic_body", critic)):
        if len(keys) < 2:
            raise ValueError(f"{name}.0.weight: the state dict has no {name} layers")
    hidden = dict(adaptation_module_branch_hidden_dims=[int(sd[k].shape[0]) for k in ad[:-1]],
                  actor_hidden_dims=[int(sd[k].shape[0]) for k in actor[:-1]],
                  critic_hidden_dims=[int(sd[k].shape[0]) for k in critic[:-1]])
    npv, na = int(num_privileged_obs), int(num_actions)
    if d["kind"] == "old":
        width, why = int(num_obs_history), (f"num_obs_history = num_observation_history x num_observations = "
                                            f"{num_obs_history}, frames of {num_obs}")
        args = type("AC_Args", (AC.AC_Args,), hidden)
    else:
        g = CF.scan_grid(cfg)
        shape = (2, g["rows"], g["ny"])
        n_map = int(np.prod(shape))
        if d["kind"] == "cnn":
            want_in, what = AC.cnn_feature_count(shape), "features of the twice-pooled map"
        else:
            want_in, what = n_map, "map values"
        if d["encoder_in"] != want_in:
            k = d["encoder_key"]
            raise _mismatch(k, sd[k].shape, (sd[k].shape[0], want_in), side,
                            f"a {shape[1]} x {shape[2]} measured_points grid, height_map_shape {shape}: "
                            f"{want_in} {what}")
        if n_map > num_obs:
            raise _mismatch(d["encoder_key"], sd[d["encoder_key"]].shape, (sd[d["encoder_key"]].shape[0], want_in),
                            side, f"a frame of {num_obs} observations, fewer than the {n_map} values of "
                                  f"height_map_shape {shape}")
        width = 2 * (int(num_obs) - n_map) + d["embedding"]
        why = (f"policy input = 2 x {int(num_obs) - n_map} scalars of a {num_obs}-wide frame + the embedding of "
               f"{d['embedding']}")
        args = type("AC_Args", (AC.AC_Args_CNN,), dict(hidden, use_cnn=d["kind"] == "cnn", height_map_shape=shape,
                                                       cnn_num_embedding=d["embedding"]))
    checks = ((ad[0], (hidden["adaptation_module_branch_hidden_dims"][0], width), why),
              (ad[-1], (npv, sd[ad[-1]].shape[1]), f"num_privileged_obs = {npv}"),
              (actor[0], (hidden["actor_hidden_dims"][0], width + npv), f"{why}, + num_privileged_obs = {npv}"),
              (critic[0], (hidden["critic_hidden_dims"][0], width + npv), f"{why}, + num_privileged_obs = {npv}"),
              (actor[-1], (na, sd[actor[-1]].shape[1]), f"num_actions = {na}"))
    for key, want, reason in checks:
        if tuple(sd[key].shape) != tuple(want):
            raise _mismatch(key, sd[key].shape, want, side, reason)
    if d["kind"] == "old":
        ac = AC.ActorCritic(num_obs, npv, num_obs_history, na, ac_args=args)
    else:
        ac = AC.ActorCriticCNN(num_obs, npv, num_obs_history, na, ac_args=args)
    ac.load_state_dict(sd)
    return ac.to(device).eval()
