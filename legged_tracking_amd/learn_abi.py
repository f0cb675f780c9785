"""ctypes mirrors of include/go1_rollout.h and include/go1_ppo.h (the rollout kernels' and the PPO update
engine's C ABIs), and the one description of the policy architecture both libraries compile in.  Pure host code.

Field for field as the headers; tests/test_learn_abi.py checks the sizes against go1_rollout_abi_sizes /
go1_ppo_abi_sizes of the compiled libraries.
"""
import ctypes as C

GO1_ROLLOUT_ABI_VERSION = 2
GO1_PPO_ABI_VERSION = 2
GO1_POLICY_LAYERS = 11
GO1_PPO_AUX = 8
GO1_ENCODER_LAYERS = 3
GO1_ENC_MLP, GO1_ENC_CNN = 0, 1
GO1_ENC_MAX_EMBED = 512
GO1_POLICY_FULL, GO1_POLICY_STUDENT, GO1_POLICY_TEACHER = 0, 1, 2  # go1_policy_args.mode
GO1_PPO_ENC_NONE, GO1_PPO_ENC_MLP = 0, 1  # go1_ppo_dims.enc_mode
GO1_PPO_ENC_CNN = 3  # 2 stays refused (go1_ppo.h)
CNN_MAP_SHAPE, CNN_FEATURES = (2, 61, 31), 3360  # the one map the engine's CNN mode takes, its twice-pooled size
GO1_PPO_ENC_HIDDEN = 256
GO1_PPO_ENC_MAX_MAP = 4096

P = C.c_void_p
I32 = C.c_int32
I64 = C.c_int64


class Transition(C.Structure):  # go1_transition
    _fields_ = [(k, P) for k in ("obs", "privileged_obs", "obs_history", "actions", "mu", "sigma",
                                 "actions_log_prob", "values", "rewards", "dones", "time_outs",
                                 "st_obs", "st_privileged_obs", "st_obs_history", "st_actions", "st_mu",
                                 "st_sigma", "st_actions_log_prob", "st_values", "st_rewards", "st_dones")] + [
        ("num_obs", I32), ("num_priv", I32), ("num_obs_history", I32), ("num_actions", I32),
        ("time_outs_flag", P), ("time_outs_pending", P), ("time_outs_dst", P), ("obs_history_ld", I64)]


class PolicyLayer(C.Structure):  # go1_policy_layer
    _fields_ = [("w", P), ("b", P), ("wf", P)]


class PolicyArgs(C.Structure):  # go1_policy_args
    _fields_ = [("obs_history", P), ("privileged_obs", P), ("action_mean", P), ("value", P), ("latent", P),
                ("std", P), ("actions", P), ("action_sigma", P), ("log_prob", P), ("rng_seed", C.c_uint64),
                ("rng_step", C.c_uint64), ("env_id_offset", I32), ("n_envs", I32), ("hist_dim", I32),
                ("num_actions", I32), ("num_priv", I32), ("variant", I32), ("overflow", P),
                ("layers", PolicyLayer * GO1_POLICY_LAYERS), ("hist_ld", I64), ("mode", I32)]


class EncoderArgs(C.Structure):  # go1_encoder_args
    _fields_ = [("obs_history", P), ("hist_ld", I64), ("frame_off", I64), ("num_obs", I32), ("n_scalar", I32),
                ("map_x", I32), ("map_y", I32), ("mode", I32), ("n_embed", I32), ("n_feat", I32), ("n_envs", I32),
                ("layers", PolicyLayer * GO1_ENCODER_LAYERS), ("scratch", P), ("policy_input", P), ("out_ld", I64),
                ("overflow", P)]


class PPODims(C.Structure):  # go1_ppo_dims
    _fields_ = [("hist", I32), ("priv", I32), ("actions", I32), ("mb", I32), ("rows", I64),
                # the height-map encoder in front of the heads (ABI 2); all zero: the plain module
                ("enc_mode", I32), ("num_obs", I32), ("n_map", I32), ("n_embed", I32)]


class PPOBufs(C.Structure):  # go1_ppo_bufs
    _fields_ = [("obs_history", P), ("hist_ld", I64)] + \
               [(k, P) for k in ("privileged_obs", "actions", "values", "advantages", "returns", "actions_log_prob",
                                 "mu", "sigma", "idx", "params", "grads", "exp_avg", "exp_avg_sq", "ad_exp_avg",
                                 "ad_exp_avg_sq", "steps", "lr", "hyper", "losses", "work")]


# go1_ppo_hyper: one float per field, written as a float32 tensor (ppo_engine.load_library checks the size)
HYPER_FIELDS = ("clip_param", "value_loss_coef", "entropy_coef", "max_grad_norm", "desired_kl",
                "use_clipped_value_loss", "selective", "beta1", "beta2", "eps", "world", "adaptation_lr")

_PP = C.POINTER
ROLLOUT_ARGTYPES = {
    "go1_rollout_abi_sizes": [_PP(I64)],
    "go1_policy_forward": [_PP(PolicyArgs), P],
    "go1_encoder_abi_sizes": [_PP(I64)],
    "go1_heightmap_encode": [_PP(EncoderArgs), P],
    "go1_record_transition": [_PP(Transition), I32, C.c_float, P],
    "go1_gae": [P] * 7 + [I32, I32, C.c_float, C.c_float, P],
    "go1_adv_normalize": [P, P, C.c_double, I64, P],
    "go1_colsum": [P, I64, I32, P, I32, P, P],
}
PPO_ARGTYPES = {
    "go1_ppo_abi_sizes": [_PP(I64)],
    "go1_ppo_param_count": [_PP(PPODims), _PP(I64), _PP(I64)],
    "go1_ppo_workspace_bytes": [_PP(PPODims), _PP(I64)],
    "go1_ppo_pack": [_PP(PPODims), _PP(PPOBufs), P],
    "go1_ppo_grad": [_PP(PPODims), _PP(PPOBufs), I32, P],
    "go1_ppo_step": [_PP(PPODims), _PP(PPOBufs), I32, P],
    "go1_ppo_test_linear": [P, I64, I32, P, P, I32, I32, P, P, I64, I32, P],
    "go1_ppo_test_wgrad": [P, P, I64, I32, I32, P, P, I64, I32, P],
    # maps, rows, w1, b1, w2, b2, d_feat | feat, dw1, db1, dw2, db2 | work, work_bytes, reps, stream
    "go1_ppo_test_conv": [P, I64] + [P] * 11 + [I64, I32, P],
}

# ----------------------------------------------------------------------------- the policy architecture
# The Linear layers of the supported ActorCritic in state_dict order: the order of go1_policy_args.layers
# (a1 a2 a3 p1 p2 p3 p4 c1 c2 c3 c4) and of the engine's flat parameter buffer (go1_ppo_bufs.params).
POLICY_LINEARS = tuple(("adaptation_module", i) for i in (0, 2, 4)) + \
                 tuple(("actor_body", i) for i in (0, 2, 4, 6)) + tuple(("critic_body", i) for i in (0, 2, 4, 6))
assert len(POLICY_LINEARS) == GO1_POLICY_LAYERS
N_ADAPT_LINEARS = 3
# the MLP height-map encoder's Linear layers (actor_critic.HeightMapEncoder.model), in front of the heads
ENCODER_LINEARS = (("height_map_encoder.model", 0), ("height_map_encoder.model", 2))
# the CNN height-map encoder's layers: Conv2d(2, 16, 3), Conv2d(16, 32, 3), Linear(3360, E)
CONV_ENCODER_LAYERS = (("height_map_encoder.model", 0), ("height_map_encoder.model", 3),
                       ("height_map_encoder.model", 7))


def policy_linears(ac):
    """The eleven Linear modules of an ActorCritic in state_dict order (IndexError / AttributeError when the
    module is laid out differently)."""
    return [getattr(ac, seq)[i] for seq, i in POLICY_LINEARS]


def policy_shapes(num_obs_history, num_privileged_obs, num_actions):
    """The (out, in) weight shapes of policy_linears(ac) for AC_Args' default widths (GO1_PPO_HA1.. / H1.. in
    go1_ppo.h, the compiled widths of rollout.hip)."""
    h, npv = num_obs_history, num_privileged_obs
    return [(256, h), (128, 256), (npv, 128),
            (512, h + npv), (256, 512), (128, 256), (num_actions, 128),
            (512, h + npv), (256, 512), (128, 256), (1, 128)]
