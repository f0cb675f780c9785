"""PPO rollout over the HIP env step: the go1_gym_learn.ppo_cse API the training script uses, with the same public
names, constructor arguments and parameter names (so the reference's `ac_weights.pt` state dicts load unchanged).

An API module: it defines nothing.  The code lives in one module per concern, imported in this order --
rollout_lib (the HIP library), actor_critic (the torch modules), policy_kernels (packers, fused forwards, record /
GAE kernels, inference policies), storage, ppo, runner -- and every name this module ever held resolves here to the
same object.  rollout_cnn is the ppo_cse_cnn counterpart.
"""
from .actor_critic import (AC_Args, ActorCritic, _Args, _LinearSplitK, _mlp, _mlp_train,  # noqa: F401
                           get_activation)
from .policy_kernels import (FusedPolicy, HipRolloutKernels, InferencePolicy, _NO_INFO, _pack_linear,  # noqa: F401
                             _pack_matrix, fused_inference)
from .ppo import PPO, PPO_Args  # noqa: F401
from .rollout_lib import HERE, LIB_PATH, _colsum, lib  # noqa: F401
from .runner import Runner, RunnerArgs, _rollout_outputs  # noqa: F401
from .storage import RolloutStorage, _world  # noqa: F401
