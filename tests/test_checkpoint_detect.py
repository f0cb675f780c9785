"""checkpoint.load_actor_critic: the learner is read off the state dict (ppo_cse module, ppo_cse_cnn with the MLP or
the CNN encoder), built with an AC_Args copy, and a state dict that does not fit the Cfg is refused by key."""
import copy

import numpy as np
import pytest
import torch

from legged_tracking_amd import checkpoint as CK, config as CF, rollout as R, rollout_cnn as RC

S = 41  # scalar observations of a frame


def _cfg(nx, ny, front_half, history=2):
    cfg = CF.readme_config(n_envs=16, terrain="single_path", rows=2, cols=2)
    cfg.terrain.measured_points_x, cfg.terrain.measured_points_y = np.linspace(-1, 1, nx), np.linspace(-0.5, 0.5, ny)
    cfg.terrain.measure_front_half = front_half
    cfg.env.num_observation_history = history
    cfg.env.num_observations = cfg.env.num_scalar_observations = CF.obs_layout(cfg)["width"]
    return cfg


def _dims(cfg, npriv=2):
    num_obs = cfg.env.num_observations
    return num_obs, npriv, num_obs * cfg.env.num_observation_history, 12


def _encoder_module(cfg, E, use_cnn, npriv=2):
    g = CF.scan_grid(cfg)
    args = type("A", (RC.AC_Args,), dict(use_cnn=use_cnn, height_map_shape=(2, g["rows"], g["ny"]),
                                         cnn_num_embedding=E))
    num_obs, _, hist, na = _dims(cfg, npriv)
    return RC.ActorCritic(num_obs, npriv, hist, na, ac_args=args)


def _save(tmp_path, ac, cfg=None):
    torch.save(ac.state_dict(), tmp_path / "ac_weights.pt")
    if cfg is not None:
        CK.save_parameters(cfg, str(tmp_path))
    return str(tmp_path)


def _class_args():
    return {c: copy.deepcopy({k: v for k, v in vars(c).items() if not k.startswith("_")})
            for c in (R.AC_Args, RC.AC_Args)}


CASES = {
    "old": lambda: (_cfg(21, 11, True), None),
    "mlp_21x11_E256": lambda: (_cfg(21, 11, False), (256, False)),
    "mlp_5x3_E128": lambda: (_cfg(5, 3, False), (128, False)),
    "cnn_61x31_E128": lambda: (_cfg(61, 31, False, history=1), (128, True)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_state_dicts_load_into_their_class(case, tmp_path):
    torch.manual_seed(0)
    cfg, enc = CASES[case]()
    dims = _dims(cfg)
    src = R.ActorCritic(*dims) if enc is None else _encoder_module(cfg, *enc)
    logdir = _save(tmp_path, src, cfg)
    before = _class_args()
    ac = CK.load_actor_critic(logdir, cfg, *dims, device="cpu")
    assert _class_args() == before  # the class-level AC_Args are untouched
    assert not ac.training
    if enc is None:
        assert type(ac) is R.ActorCritic and issubclass(ac.ac_args, R.AC_Args) and ac.ac_args is not R.AC_Args
        assert not hasattr(ac.ac_args, "use_cnn")
    else:
        E, use_cnn = enc
        g = CF.scan_grid(cfg)
        assert type(ac) is RC.ActorCritic and issubclass(ac.ac_args, RC.AC_Args) and ac.ac_args is not RC.AC_Args
        assert ac.ac_args.use_cnn is use_cnn and ac.use_cnn is use_cnn
        assert ac.ac_args.cnn_num_embedding == E and ac.cnn_num_embedding == E
        assert tuple(ac.ac_args.height_map_shape) == (2, g["rows"], g["ny"]) == ac.height_map_shape
    for a in (ac.ac_args.actor_hidden_dims, ac.ac_args.critic_hidden_dims):
        assert list(a) == [512, 256, 128]
    assert list(ac.ac_args.adaptation_module_branch_hidden_dims) == [256, 128]
    for k, v in src.state_dict().items():
        assert torch.equal(ac.state_dict()[k], v), k
    x = torch.randn(3, dims[2])
    with torch.no_grad():
        assert torch.equal(ac.act_student(x), src.eval().act_student(x))


def test_other_hidden_widths_come_from_the_state_dict(tmp_path):
    cfg = _cfg(21, 11, True)
    dims = _dims(cfg)
    args = type("A", (R.AC_Args,), dict(actor_hidden_dims=[64, 32], adaptation_module_branch_hidden_dims=[48]))
    src = R.ActorCritic(*dims, ac_args=args)
    ac = CK.load_actor_critic(_save(tmp_path, src, cfg), cfg, *dims, device="cpu")
    assert ac.ac_args.actor_hidden_dims == [64, 32] and ac.ac_args.adaptation_module_branch_hidden_dims == [48]
    assert R.AC_Args.actor_hidden_dims == [512, 256, 128]


def _raises(tmp_path, src, cfg, dims, key, with_pkl=True):
    logdir = _save(tmp_path, src, cfg if with_pkl else None)
    with pytest.raises(ValueError) as e:
        CK.load_actor_critic(logdir, cfg, *dims, device="cpu")
    msg = str(e.value)
    assert key in msg, msg
    assert str(tuple(src.state_dict()[key].shape)) in msg, msg  # the checkpoint's shape ...
    assert "the checkpoint has" in msg and ("parameters.pkl implies" in msg) == with_pkl, msg  # ... and who says what
    return msg


def test_grid_against_the_encoder_input(tmp_path):
    src = _encoder_module(_cfg(5, 3, False), 128, False)
    cfg = _cfg(21, 11, False)  # the Cfg scans 21 x 11, the encoder takes 2 x 5 x 3 values
    msg = _raises(tmp_path, src, cfg, _dims(cfg), "height_map_encoder.model.0.weight")
    assert "(256, 462)" in msg and "21 x 11" in msg


def test_num_privileged_obs(tmp_path):
    cfg = _cfg(21, 11, True)
    src = R.ActorCritic(*_dims(cfg, npriv=6))
    msg = _raises(tmp_path, src, cfg, _dims(cfg, npriv=2), "adaptation_module.4.weight")
    assert "(2, 128)" in msg and "num_privileged_obs = 2" in msg


def test_history_width(tmp_path):
    cfg = _cfg(21, 11, True, history=2)
    src = R.ActorCritic(*_dims(_cfg(21, 11, True, history=3)))
    msg = _raises(tmp_path, src, cfg, _dims(cfg), "adaptation_module.0.weight", with_pkl=False)
    assert f"(256, {2 * 261})" in msg and "there is no parameters.pkl" in msg


def test_cnn_on_a_21x11_grid(tmp_path):
    src = _encoder_module(_cfg(61, 31, False, history=1), 128, True)
    cfg = _cfg(21, 11, False)
    msg = _raises(tmp_path, src, cfg, _dims(cfg), "height_map_encoder.model.7.weight")
    assert "(128, 320)" in msg  # 32 x (21 // 4) x (11 // 4) pooled features, the Linear takes 3360


def test_old_learner_dict_with_a_503_wide_cfg(tmp_path):
    src = R.ActorCritic(*_dims(_cfg(21, 11, True)))
    cfg = _cfg(21, 11, False)
    assert cfg.env.num_observations == 503
    msg = _raises(tmp_path, src, cfg, _dims(cfg), "adaptation_module.0.weight")
    assert f"(256, {2 * 503})" in msg


def test_describe_reads_the_learner_off_the_keys():
    assert CK.describe(R.ActorCritic(261, 2, 261, 12).state_dict())["kind"] == "old"
    d = CK.describe(_encoder_module(_cfg(5, 3, False), 96, False).state_dict())
    assert (d["kind"], d["embedding"], d["encoder_in"]) == ("mlp", 96, 30)
    d = CK.describe(_encoder_module(_cfg(61, 31, False, history=1), 64, True).state_dict())
    assert (d["kind"], d["embedding"], d["encoder_in"]) == ("cnn", 64, 3360)
