"""The height-map encoder actor-critic: the go1_gym_learn.ppo_cse_cnn API (scripts/train.py without --old_ppo), with
the same public names, constructor arguments and parameter names as the reference.

An API module like rollout: it defines nothing.  ActorCritic, AC_Args and Runner are actor_critic.ActorCriticCNN,
actor_critic.AC_Args_CNN and runner.RunnerCNN; PPO, RolloutStorage, PPO_Args and RunnerArgs are the very objects
rollout has (ppo_cse_cnn/ppo.py differs from ppo_cse/ppo.py in one line, which PPO takes from the module).
"""
from .actor_critic import (AC_Args_CNN as AC_Args, ActorCriticCNN as ActorCritic, CNN_FEATURES,  # noqa: F401
                           ENC_HIDDEN, HeightMapEncoder, _mlp, _mlp_train, cnn_feature_count, get_activation)
from .policy_kernels import (FUSED_DEFAULT, FusedEncoderPolicy, _pack_conv, encoder_layers,  # noqa: F401
                             fused_policy)
from .ppo import ENGINE_DEFAULT, PPO, PPO_Args, encoder_engine_on  # noqa: F401
from .runner import RunnerArgs, RunnerCNN as Runner  # noqa: F401
from .storage import RolloutStorage  # noqa: F401
