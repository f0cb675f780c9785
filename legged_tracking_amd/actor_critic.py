"""The learner's torch modules: the history-MLP actor-critic (go1_gym_learn.ppo_cse) and its height-map encoder
subclass (go1_gym_learn.ppo_cse_cnn), with the reference's constructor arguments and parameter names, so that its
`ac_weights.pt` state dicts load unchanged.

The policy / value / adaptation MLPs are plain GEMM chains on hipBLASLt (through torch); PPO.update's mini-batches
take the split-K weight gradient (_LinearSplitK) and the HIP column sum (rollout_lib._colsum).  The rollout does not
run these forwards: policy_kernels.FusedPolicy / FusedEncoderPolicy do.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Normal

from .rollout_lib import _colsum


class _Args:
    """Plain mutable argument holder (scripts/train.py assigns attributes)."""


class AC_Args(_Args):
    """go1_gym_learn/ppo_cse/actor_critic.py:9-20."""
    init_noise_std = 1.0
    actor_hidden_dims = [512, 256, 128]
    critic_hidden_dims = [512, 256, 128]
    activation = "elu"
    adaptation_module_branch_hidden_dims = [256, 128]
    use_decoder = False
    normalize_obs = False


def get_activation(name):
    acts = dict(elu=nn.ELU, selu=nn.SELU, relu=nn.ReLU, crelu=nn.ReLU, lrelu=nn.LeakyReLU, tanh=nn.Tanh,
                sigmoid=nn.Sigmoid)
    if name not in acts:
        raise ValueError(f"invalid activation function {name!r}")
    return acts[name]()


class _LinearSplitK(torch.autograd.Function):
    """y = x W^T + b whose weight gradient is summed over K_SPLIT row chunks of the batch (one batched
    GEMM, then a sum over the chunks): the mini-batch weight gradient dW = dY^T X is a tall-skinny
    reduction (K = 24,576 samples, M x N <= 512 x 263), which one GEMM spreads over only a few dozen
    workgroups of the 256 CUs; the batched form gives each chunk its own tiles.  Same value as
    F.linear's backward up to the f32 summation order."""

    K_SPLIT = 16

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx = gy @ w if ctx.needs_input_grad[0] else None
        n, S = x.shape[0], _LinearSplitK.K_SPLIT
        if n % S == 0 and n // S >= 256:
            gw = torch.bmm(gy.view(S, n // S, -1).transpose(1, 2), x.view(S, n // S, -1)).sum(0)
        else:
            gw = gy.t() @ x
        return gx, gw, _colsum(gy)


def _mlp_train(seq, x):
    """nn.Sequential of Linear / activation layers evaluated with _LinearSplitK (training mini-batches)."""
    for m in seq:
        x = _LinearSplitK.apply(x, m.weight, m.bias) if isinstance(m, nn.Linear) else m(x)
    return x


def _mlp(sizes, act):
    layers = []
    for i in range(len(sizes) - 1):
        layers.append(nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            layers.append(act)
    return nn.Sequential(*layers)


class ActorCritic(nn.Module):
    """Student/teacher actor-critic (ppo_cse/actor_critic.py:21-156): adaptation module x -> latent (privileged
    estimate), actor (x, latent) -> action mean, critic (x, privileged_obs) -> value, state-independent std, where
    x = process_obs_history(obs_history) is the history itself.  ActorCriticCNN puts an encoder there.

    Parameters register, and draw their initial weights from torch's generator, in the order _build_input's
    modules, adaptation_module, actor_body, critic_body, std: the update engine's flat buffers, both Adam optimizers
    and the reference's state dicts depend on it."""

    is_recurrent = False

    def __init__(self, num_obs, num_privileged_obs, num_obs_history, num_actions, ac_args=None, **kwargs):
        super().__init__()
        A = self.ac_args = AC_Args if ac_args is None else ac_args  # a copy: checkpoint.load_actor_critic
        if getattr(A, "normalize_obs", False):
            raise NotImplementedError("normalize_obs is off in the README configuration and not on this path")
        self.decoder = A.use_decoder
        self.num_obs_history = num_obs_history
        self.num_privileged_obs = num_privileged_obs
        p, npv = self._build_input(num_obs), num_privileged_obs
        act = get_activation(A.activation)
        self.adaptation_module = _mlp([p, *A.adaptation_module_branch_hidden_dims, npv], act)
        self.actor_body = _mlp([npv + p, *A.actor_hidden_dims, num_actions], act)
        self.critic_body = _mlp([npv + p, *A.critic_hidden_dims, 1], act)
        self.std = nn.Parameter(A.init_noise_std * torch.ones(num_actions))
        self.distribution = None
        self.normalize_obs = False

    def _build_input(self, num_obs):
        """Registers what process_obs_history runs (nothing here) and returns the width of what it returns."""
        return self.num_obs_history

    def process_obs_history(self, observation_history):
        return observation_history

    def process_obs_history_train(self, observation_history):
        """process_obs_history for PPO.update's mini-batches."""
        return observation_history

    def reset(self, dones=None):
        pass

    @property
    def action_mean(self):
        return self.distribution.mean

    @property
    def action_std(self):
        return self.distribution.stddev

    @property
    def entropy(self):
        return self.distribution.entropy().sum(dim=-1)

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

    # PPO.update's mini-batches (split-K weight gradients, _LinearSplitK).  As in the reference, the actor, the
    # critic and the adaptation step each run process_obs_history_train (ppo.py:110-113, 170): an encoder's gradient
    # is the sum over the passes in the same order.
    def update_distribution_train(self, observation_history):
        x = self.process_obs_history_train(observation_history)
        latent = _mlp_train(self.adaptation_module, x)
        mean = _mlp_train(self.actor_body, torch.cat((x, latent), dim=-1))
        self.distribution = Normal(mean, mean * 0.0 + self.std, validate_args=False)

    def evaluate_train(self, observation_history, privileged_observations):
        x = self.process_obs_history_train(observation_history)
        return _mlp_train(self.critic_body, torch.cat((x, privileged_observations), dim=-1))

    def adaptation_pred_train(self, observation_history):
        """The adaptation step's prediction (ppo.py:170)."""
        return _mlp_train(self.adaptation_module, self.process_obs_history_train(observation_history))


# ----------------------------------------------------------------------------- the height-map encoder module
CNN_FEATURES = 3360  # the CNN's Linear(3360, E) (actor_critic.py:45): 32 channels x (61 // 4) x (31 // 4)
ENC_HIDDEN = 256     # the MLP encoder's hidden width (actor_critic.py:49)
# The classes that share a name with the plain learner's are public as rollout_cnn.AC_Args / ActorCritic / Runner and
# keep that qualified name (pickles and `type(ac).__module__` say which learner it is); only __name__ is new.
_PUBLIC_CNN = "legged_tracking_amd.rollout_cnn"


class AC_Args_CNN(AC_Args):
    """go1_gym_learn/ppo_cse_cnn/actor_critic.py:8-24 (rollout_cnn.AC_Args)."""
    __module__, __qualname__ = _PUBLIC_CNN, "AC_Args"
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
    """ppo_cse_cnn/actor_critic.py:27-62: the map of one frame -> an embedding."""

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
        """forward for PPO.update's mini-batches (the Linear layers through _LinearSplitK)."""
        return _mlp_train(self.model, self._shape(x))


class ActorCriticCNN(ActorCritic):
    """ppo_cse_cnn/actor_critic.py:65-239 with use_gru = False (rollout_cnn.ActorCritic).

    Every observation frame ends in the prod(height_map_shape) columns of the height map; the encoder turns the map
    into an embedding of width E, and with the default nn.Identity recurrent layer only the LAST frame of the history
    reaches the heads:

      policy_input = [scalars of the last frame | scalars of the last frame | embedding of the last frame]

    of width 2 S + E, S = num_obs - prod(height_map_shape).  The heads are ActorCritic's on policy_input in place of
    the history; height_map_encoder registers in front of them."""

    __module__, __qualname__ = _PUBLIC_CNN, "ActorCritic"
    graph_capture = False  # PPO runs this module's torch update eagerly (MIOpen convolutions are not captured)

    def __init__(self, num_obs, num_privileged_obs, num_obs_history, num_actions, ac_args=AC_Args_CNN, **kwargs):
        if kwargs:
            print("ActorCritic.__init__ got unexpected arguments, which will be ignored: " + str(list(kwargs)))
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
        super().__init__(num_obs, num_privileged_obs, num_obs_history, num_actions, ac_args)

    def _build_input(self, num_obs):
        A = self.ac_args
        self.num_obs = num_obs
        self.height_map_shape = tuple(int(v) for v in A.height_map_shape)
        self.num_map = int(np.prod(self.height_map_shape))
        self.num_scalar = num_obs - self.num_map
        self.use_cnn = bool(A.use_cnn)
        self.cnn_num_embedding = A.cnn_num_embedding
        self.lstm_input_dim = int(self.num_scalar + self.cnn_num_embedding)
        self.lstm_num_embedding = self.lstm_input_dim
        self.policy_input_dim = int(self.num_scalar + self.lstm_num_embedding)
        self.height_map_encoder = HeightMapEncoder(self.height_map_shape, self.cnn_num_embedding, use_cnn=self.use_cnn,
                                                   activation=A.activation)
        self.recurrent_latent_embedding = nn.Identity()
        return self.policy_input_dim

    def process_obs_history(self, observation_history):
        # actor_critic.py:180-198.  The reference encodes every frame and keeps recurrent_latent[:, -1]; with the
        # Identity layer that is the last frame's [scalars | embedding], so only the last frame is encoded here.
        last = observation_history.reshape(observation_history.shape[0], -1, self.num_obs)[:, -1]
        scalars = last[:, :self.num_scalar]
        return torch.cat([scalars, scalars, self.height_map_encoder(last[:, self.num_scalar:])], dim=-1)

    def process_obs_history_train(self, observation_history):
        # every frame through the encoder, as the reference does (actor_critic.py:184-185): the earlier frames add
        # exact zeros to the weight gradients, but the update matches the reference's to 1e-6 only with its GEMM
        # shapes (Adam normalises the gradient, so a last-bit difference of a small component moves a weight)
        n = observation_history.shape[0]
        frames = observation_history.reshape(n, -1, self.num_obs)
        emb = self.height_map_encoder.forward_train(frames[:, :, self.num_scalar:].reshape(-1, self.num_map))
        scalars = frames[:, -1, :self.num_scalar]
        return torch.cat([scalars, scalars, emb.reshape(n, -1, self.cnn_num_embedding)[:, -1]], dim=-1)
