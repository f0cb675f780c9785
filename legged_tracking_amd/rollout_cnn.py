"""The height-map encoder actor-critic: the go1_gym_learn.ppo_cse_cnn API (scripts/train.py without --old_ppo).

Mirrors, with the same public names, constructor arguments and parameter names (so the reference's
`ac_weights.pt` state dicts load unchanged):

  AC_Args, HeightMapEncoder, ActorCritic  <- go1_gym_learn/ppo_cse_cnn/actor_critic.py:8-239
  Runner                                  <- go1_gym_learn/ppo_cse_cnn/__init__.py:66-357

PPO, RolloutStorage, PPO_Args and RunnerArgs are rollout.py's: ppo_cse_cnn/ppo.py differs from ppo_cse/ppo.py
in one line (:170-171, the adaptation step goes through process_obs_history), which PPO._minibatch_step takes
from the module (adaptation_pred_train).

What the module computes.  Every observation frame ends in the prod(height_map_shape) columns of the height
map; the encoder turns the map into an embedding of width E, and with the default nn.Identity recurrent layer
(use_gru = False) only the LAST frame of the history reaches the heads:

  policy_input = [scalars of the last frame | scalars of the last frame | embedding of the last frame]

of width 2 S + E, S = num_obs - prod(height_map_shape).  Adaptation module, actor and critic are rollout.py's
MLPs on policy_input in place of the history.

MI355X mapping: the rollout's forward is two HIP launches (FusedEncoderPolicy): go1_heightmap_encode
(csrc/encoder.hip) writes policy_input, go1_policy_forward (csrc/rollout.hip) runs the three heads on it.  The
PPO update of this module runs on torch autograd, eagerly, by default (ppo_engine.supported refuses its parameter
names, and that mini-batch step is not captured into a HIP graph).  With the MLP encoder it also runs on the HIP
update engine (csrc/ppo_update.hip, go1_ppo_dims.enc_mode 1: one encoder pass on the last frame, captured into a
HIP graph), switched by ENGINE_DEFAULT / GO1_PPO_ENCODER_ENGINE; with the CNN encoder on the (2, 61, 31) map
likewise (enc_mode 3, csrc/ppo_conv.h: the conv stack's forward and backward in one kernel per direction).
"""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Normal

from . import abi, learn_abi as LA, native, rollout as R
from .rollout import PPO, PPO_Args, RolloutStorage, RunnerArgs, get_activation, _mlp, _mlp_train  # noqa: F401

CNN_FEATURES = 3360  # the CNN's Linear(3360, E) (actor_critic.py:45): 32 channels x (61 // 4) x (31 // 4)
ENC_HIDDEN = 256     # the MLP encoder's hidden width (actor_critic.py:49)
# Which encoder modes take FusedEncoderPolicy in the rollout by default: those whose encode + policy launches
# beat the module's torch eager act + evaluate at 4096 envs (tools/encoder_kernel_time.py).
FUSED_DEFAULT = {"mlp": True, "cnn": True}
# Which encoder modes take the HIP update engine (ppo_engine.PPOEngine with go1_ppo_dims.enc_mode) in PPO.update
# by default.  The engine has the MLP encoder (ppo_engine.encoder_supported) and the CNN encoder on the (2, 61, 31)
# map (ppo_engine.conv_encoder_supported, csrc/ppo_conv.h); both stay off until their update-time tables
#  are weighed.
# GO1_PPO_ENCODER_ENGINE=1 / 0 overrides the default for a run; GO1_PPO_ENGINE=0 switches every engine off.
ENGINE_DEFAULT = {"mlp": False, "cnn": False}


def encoder_engine_on(ac):
    """The switch PPO._engine_on consults for this module (the architecture check is ppo_engine's)."""
    env = os.environ.get("GO1_PPO_ENCODER_ENGINE")
    if env in ("0", "1"):
        return env == "1"
    return ENGINE_DEFAULT["cnn" if ac.use_cnn else "mlp"]


class AC_Args(R.AC_Args):
    use_cnn = False
    use_gru = False
    height_map_shape = (2, 61, 31)
    cnn_num_embedding = 256
    lstm_num_embedding = 256


def cnn_feature_count(height_map_shape):
    """Flattened size after Conv3x3 / MaxPool2 twice (floor pooling), 32 channels."""
    _, x, y = height_map_shape
    return 32 * (x // 2 // 2) * (y // 2 // 2)


class HeightMapEncoder(nn.Module):
    """actor_critic.py:27-62: the map of one frame -> an embedding."""

    def __init__(self, height_map_shape, num_embedding=128, use_cnn=False, activation="elu"):
        super().__init__()
        self.height_map_shape = tuple(int(v) for v in height_map_shape)
        self.use_cnn = use_cnn
        self.num_embedding = num_embedding
        if use_cnn:
            self.model = nn.Sequential(
                nn.Conv2d(2, 16, kernel_size=3, stride=1, padding=1), nn.ReLU(), nn.MaxPool2d(kernel_size=2, stride=2),
                nn.Conv2d(16, 32, kernel_size=3, stride=1, padding=1), nn.ReLU(), nn.MaxPool2d(kernel_size=2, stride=2),
                nn.Flatten(), nn.Linear(CNN_FEATURES, num_embedding))
        else:
            act = get_activation(activation)
            self.model = nn.Sequential(nn.Linear(int(np.prod(self.height_map_shape)), ENC_HIDDEN), act,
                                       nn.Linear(ENC_HIDDEN, num_embedding), act)

    def _shape(self, x):
        return x.reshape(x.shape[0], *self.height_map_shape) if self.use_cnn else x.reshape(x.shape[0], -1)

    def forward(self, x):
        return self.model(self._shape(x))

    def forward_train(self, x):
        """forward for PPO.update's mini-batches (the Linear layers through rollout._LinearSplitK)."""
        return _mlp_train(self.model, self._shape(x))


class ActorCritic(nn.Module):
    """actor_critic.py:65-239 with use_gru = False."""

    is_recurrent = False
    graph_capture = False  # PPO runs this module's update eagerly (MIOpen convolutions are not captured)

    def __init__(self, num_obs, num_privileged_obs, num_obs_history, num_actions, ac_args=AC_Args, **kwargs):
        if kwargs:
            print("ActorCritic.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs)))
        super().__init__()
        shape = tuple(int(v) for v in ac_args.height_map_shape)
        n_map = int(np.prod(shape))
        if getattr(ac_args, "use_gru", False):
            raise NotImplementedError(
                "use_gru: the reference builds nn.GRU without batch_first (ppo_cse_cnn/actor_critic.py:103) and feeds "
                "it (env, frame, feature) (:191), so it recurs over the env dimension; this path does not "
                "reproduce that cross-env recurrence")
        if n_map > num_obs:
            raise ValueError(
                f"height_map_shape {shape} has {n_map} values but an observation frame only {num_obs} (the "
                f"--measure_front_half case; the reference fails in the reshape, ppo_cse_cnn/actor_critic.py:184)")
        if getattr(ac_args, "use_cnn", False) and (len(shape) != 3 or shape[0] != 2 or
                                                   cnn_feature_count(shape) != CNN_FEATURES):
            raise ValueError(
                f"use_cnn with height_map_shape {shape}: the twice-pooled map has "
                f"{cnn_feature_count(shape) if len(shape) == 3 else '?'} features, the encoder's Linear takes "
                f"{CNN_FEATURES} (ppo_cse_cnn/actor_critic.py:45; scripts/train.py:65 forces (2, 21, 11))")
        if getattr(ac_args, "normalize_obs", False):
            raise NotImplementedError("normalize_obs is off in the README configuration and not on this path")
        self.decoder = ac_args.use_decoder
        self.ac_args = ac_args
        self.num_obs = num_obs
        self.num_obs_history = num_obs_history
        self.num_privileged_obs = num_privileged_obs
        self.height_map_shape = shape
        self.num_map = n_map
        self.num_scalar = num_obs - n_map
        self.use_cnn = bool(ac_args.use_cnn)
        self.cnn_num_embedding = ac_args.cnn_num_embedding
        self.lstm_input_dim = int(num_obs - n_map + self.cnn_num_embedding)
        self.lstm_num_embedding = self.lstm_input_dim
        self.policy_input_dim = int(num_obs - n_map + self.lstm_num_embedding)
        act = get_activation(ac_args.activation)
        self.height_map_encoder = HeightMapEncoder(shape, self.cnn_num_embedding, use_cnn=self.use_cnn,
                                                   activation=ac_args.activation)
        self.recurrent_latent_embedding = nn.Identity()
        p, npv = self.policy_input_dim, num_privileged_obs
        self.adaptation_module = _mlp([p, *ac_args.adaptation_module_branch_hidden_dims, npv], act)
        self.actor_body = _mlp([npv + p, *ac_args.actor_hidden_dims, num_actions], act)
        self.critic_body = _mlp([npv + p, *ac_args.critic_hidden_dims, 1], act)
        self.std = nn.Parameter(ac_args.init_noise_std * torch.ones(num_actions))
        self.distribution = None
        self.normalize_obs = False

    def reset(self, dones=None):
        pass

    def forward(self):
        raise NotImplementedError

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    @property
    def entropy(self):
        return self.distribution.entropy().sum(dim=-1)

    def _policy_input(self, observation_history, encode):
        # actor_critic.py:180-198.  The reference encodes every frame and keeps recurrent_latent[:, -1]; with the
        # Identity layer that is the last frame's [scalars | embedding], so only the last frame is encoded here.
        last = observation_history.reshape(observation_history.shape[0], -1, self.num_obs)[:, -1]
        scalars = last[:, :self.num_scalar]
        return torch.cat([scalars, scalars, encode(last[:, self.num_scalar:])], dim=-1)

    def process_obs_history(self, observation_history):
        return self._policy_input(observation_history, self.height_map_encoder)

    def update_distribution(self, observation_history):
        x = self.process_obs_history(observation_history)
        latent = self.adaptation_module(x)
        mean = self.actor_body(torch.cat((x, latent), dim=-1))
        self.distribution = Normal(mean, mean * 0.0 + self.std, validate_args=False)

    def act(self, observation_history, **kwargs):
        self.update_distribution(observation_history)
        return self.distribution.sample()

    def get_actions_log_prob(self, actions):
        return self.distribution.log_prob(actions).sum(dim=-1)

    def act_expert(self, ob, policy_info={}):
        return self.act_teacher(ob["obs_history"], ob["privileged_obs"])

    def act_inference(self, ob, policy_info={}):
        return self.act_student(ob["obs_history"], policy_info=policy_info)

    def act_student(self, observation_history, policy_info={}):
        x = self.process_obs_history(observation_history)
        latent = self.adaptation_module(x)
        policy_info["latents"] = latent.detach().cpu().numpy()
        return self.actor_body(torch.cat((x, latent), dim=-1))

    def act_teacher(self, observation_history, privileged_info, policy_info={}):
        x = self.process_obs_history(observation_history)
        policy_info["latents"] = privileged_info
        return self.actor_body(torch.cat((x, privileged_info), dim=-1))

    def evaluate(self, observation_history, privileged_observations, **kwargs):
        x = self.process_obs_history(observation_history)
        return self.critic_body(torch.cat((x, privileged_observations), dim=-1))

    def get_student_latent(self, observation_history):
        return self.adaptation_module(self.process_obs_history(observation_history))

    # PPO.update's mini-batches (split-K weight gradients, rollout._LinearSplitK).  As in the reference, the
    # actor, the critic and the adaptation step each run the encoder (ppo.py:110-113, 170): its gradient is the
    # sum over the passes in the same order.
    def process_obs_history_train(self, observation_history):
        # every frame through the encoder, as the reference does (actor_critic.py:184-185): the earlier frames add
        # exact zeros to the weight gradients, but the update matches the reference's to 1e-6 only with its GEMM
        # shapes (Adam normalises the gradient, so a last-bit difference of a small component moves a weight)
        n = observation_history.shape[0]
        frames = observation_history.reshape(n, -1, self.num_obs)
        emb = self.height_map_encoder.forward_train(frames[:, :, self.num_scalar:].reshape(-1, self.num_map))
        scalars = frames[:, -1, :self.num_scalar]
        return torch.cat([scalars, scalars, emb.reshape(n, -1, self.cnn_num_embedding)[:, -1]], dim=-1)

    def update_distribution_train(self, observation_history):
        x = self.process_obs_history_train(observation_history)
        latent = _mlp_train(self.adaptation_module, x)
        mean = _mlp_train(self.actor_body, torch.cat((x, latent), dim=-1))
        self.distribution = Normal(mean, mean * 0.0 + self.std, validate_args=False)

    def evaluate_train(self, observation_history, privileged_observations):
        x = self.process_obs_history_train(observation_history)
        return _mlp_train(self.critic_body, torch.cat((x, privileged_observations), dim=-1))

    def adaptation_pred_train(self, observation_history):
        return _mlp_train(self.adaptation_module, self.process_obs_history_train(observation_history))


# ----------------------------------------------------------------------------- weight packers
def _pack_conv(conv):
    """nn.Conv2d (3x3) -> (split packed weights, padded bias) in _pack_linear's record order, the filter of output
    channel oc flattened to the row [oc][ic * 9 + ky * 3 + kx] (K = 9 ic padded to 32)."""
    return R._pack_matrix(conv.weight.detach().float().reshape(conv.out_channels, -1), conv.bias.detach().float())


def encoder_layers(ac):
    """The encoder's weight layers in go1_encoder_args.layers order: (Linear, Linear) or (Conv2d, Conv2d, Linear)."""
    m = ac.height_map_encoder.model
    return [m[0], m[3], m[7]] if ac.use_cnn else [m[0], m[2]]


class FusedEncoderPolicy:
    """ActorCritic forward for the rollout (act + evaluate) in two HIP launches: go1_heightmap_encode writes
    policy_input into a persistent (n, 2 S + E) buffer, go1_policy_forward runs the heads on it (FusedPolicy
    with the buffer as its history).  Re-pack after every optimiser step."""

    def __init__(self, ac):
        self.ac = ac
        self.lib = R.lib()
        self._encode = self.lib.go1_heightmap_encode
        self.heads = R.FusedPolicy(ac)
        self.overflow = self.heads.overflow  # one counter: encoder and head workgroups that fell back to f32
        dev = next(ac.parameters()).device
        self._stream = native.raw_stream_of(dev)
        self.packed = None
        self._bufs = {}

    @staticmethod
    def supported(ac):
        if not isinstance(ac, ActorCritic):
            return False
        try:
            shapes = [tuple(m.weight.shape) for m in LA.policy_linears(ac)]
        except (IndexError, AttributeError):
            return False
        p, npv, na = ac.policy_input_dim, ac.num_privileged_obs, shapes[6][0]
        kin, gl, GL = p + npv, p // 32, -(-(p + npv) // 32)
        g_last = 9 * (-(-GL // 9) - 1)
        heads = (shapes == LA.policy_shapes(p, npv, na) and 1 <= npv <= 8 and kin <= 16384 and gl >= g_last
                 and na <= 16 and isinstance(ac.adaptation_module[1], nn.ELU))
        c, x, y = ac.height_map_shape
        enc = (c == 2 and x <= abi.GO1_MAX_SCAN_X and y <= abi.GO1_MAX_SCAN_Y and ac.cnn_num_embedding <= 512
               and (ac.use_cnn or isinstance(ac.height_map_encoder.model[1], nn.ELU)))
        return heads and enc

    def pack(self):
        ac = self.ac
        mods = encoder_layers(ac)
        self.packed = [_pack_conv(m) if isinstance(m, nn.Conv2d) else R._pack_linear(m) for m in mods]
        self.wf = [m.weight.detach().float().contiguous() for m in mods]
        _, x, y = ac.height_map_shape
        self.n_feat = CNN_FEATURES if ac.use_cnn else ENC_HIDDEN
        self.args = LA.EncoderArgs(num_obs=ac.num_obs, n_scalar=ac.num_scalar, map_x=x, map_y=y,
                                   mode=LA.GO1_ENC_CNN if ac.use_cnn else LA.GO1_ENC_MLP,
                                   n_embed=ac.cnn_num_embedding, n_feat=self.n_feat,
                                   overflow=self.overflow.data_ptr())
        for i, (w, b) in enumerate(self.packed):
            L = self.args.layers[i]
            L.w, L.b, L.wf = w.data_ptr(), b.data_ptr(), self.wf[i].data_ptr()
        self.heads.pack()

    def _buffers(self, n, dev):
        b = self._bufs.get(n)
        if b is None:
            b = self._bufs[n] = (torch.empty(n, self.ac.policy_input_dim, device=dev),
                                 torch.empty(n, self.n_feat, device=dev))
        return b

    def encode(self, obs_history, out=None):
        """policy_input of obs_history (n, H * num_obs), rows any stride >= the width: into `out` (n, 2 S + E), rows
        any stride >= the width, or into the persistent buffer."""
        if self.packed is None:
            self.pack()
        h = obs_history.detach()
        if h.dim() != 2 or h.stride(1) != 1 or h.stride(0) < h.shape[1]:
            h = h.contiguous()
        n = h.shape[0]
        buf, scratch = self._buffers(n, h.device)
        if out is None:
            out = buf
        if out.shape != (n, self.ac.policy_input_dim) or out.stride(1) != 1 or out.dtype != torch.float32:
            raise ValueError("out must be (n, 2 S + E) f32 rows")
        a = self.args
        a.obs_history, a.hist_ld = h.data_ptr(), h.stride(0)
        a.frame_off = h.shape[1] - self.ac.num_obs
        a.scratch, a.policy_input, a.out_ld, a.n_envs = scratch.data_ptr(), out.data_ptr(), out.stride(0), n
        rc = self._encode(C.byref(a), self._stream())
        if rc:
            native.check(self.lib, rc)
        return out

    def forward(self, obs_history, privileged_obs, sample=None, mode=0):
        """FusedPolicy.forward's tuples for the encoder module (the encoder launch is the same in every mode)."""
        return self.heads.forward(self.encode(obs_history), privileged_obs, sample=sample, mode=mode)


def fused_policy(ac):
    """What rollout.HipRolloutKernels.policy returns for this module: the fused path where it is supported and
    the default for the module's mode (FUSED_DEFAULT), else None (the torch forward)."""
    if FusedEncoderPolicy.supported(ac) and FUSED_DEFAULT["cnn" if ac.use_cnn else "mlp"]:
        return FusedEncoderPolicy(ac)
    return None


class Runner(R.Runner):
    """ppo_cse_cnn/__init__.py:66-357: rollout.Runner around this module's ActorCritic."""
    actor_critic_class = ActorCritic
