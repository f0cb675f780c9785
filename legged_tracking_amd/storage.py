"""The rollout buffers: the per-step transition copy, the GAE scan and the advantage normalisation are HIP kernels
(policy_kernels.HipRolloutKernels).  With torch.distributed initialised (one process per GPU, RCCL) the advantage
statistics are all-reduced, so every rank normalises as one large-batch run would."""
import torch

from .policy_kernels import HipRolloutKernels


def _world():
    """The size of the process group, 1 without one: the learner's one test for 'are there other ranks'."""
    d = torch.distributed
    if d.is_available() and d.is_initialized():
        return d.get_world_size()
    return 1


class RolloutStorage:
    """Device-resident (T, n, ...) rollout buffers (go1_gym_learn/ppo_cse/rollout_storage.py:5-138)."""

    class Transition:
        def __init__(self):
            self.observations = None
            self.privileged_observations = None
            self.observation_histories = None
            self.critic_observations = None
            self.actions = None
            self.rewards = None
            self.dones = None
            self.values = None
            self.actions_log_prob = None
            self.action_mean = None
            self.action_sigma = None
            self.env_bins = None
            self.time_outs = None
            self.time_outs_deferred = None

        def clear(self):
            self.__init__()

    def __init__(self, num_envs, num_transitions_per_env, obs_shape, privileged_obs_shape, obs_history_shape,
                 actions_shape, device="cpu", kernels=None):
        self.device = device
        T, n = num_transitions_per_env, num_envs
        z = lambda *s: torch.zeros(T, n, *s, device=device)  # noqa: E731
        self.obs_shape, self.privileged_obs_shape = obs_shape, privileged_obs_shape
        self.obs_history_shape, self.actions_shape = obs_history_shape, actions_shape
        self.observations = z(*obs_shape)
        self.privileged_observations = z(*privileged_obs_shape)
        self.observation_histories = z(*obs_history_shape)
        self.rewards = z(1)
        self.actions = z(*actions_shape)
        self.dones = z(1).byte()
        self.actions_log_prob = z(1)
        self.values = z(1)
        self.returns = z(1)
        self.advantages = z(1)
        self.mu = z(*actions_shape)
        self.sigma = z(*actions_shape)
        self.env_bins = z(1)
        self.adv_stats = torch.zeros(2, dtype=torch.float64, device=device)
        self.num_transitions_per_env, self.num_envs = T, n
        self.step = 0
        self.kernels = kernels if kernels is not None else HipRolloutKernels()
        self._keep = None

    def add_transitions(self, transition, gamma=0.0):
        if self.step >= self.num_transitions_per_env:
            raise AssertionError("Rollout buffer overflow")
        tr = {k: getattr(transition, k) for k in ("observations", "privileged_observations", "observation_histories",
                                                  "actions", "action_mean", "action_sigma", "actions_log_prob",
                                                  "values", "rewards", "dones", "time_outs")}
        tr["time_outs_deferred"] = getattr(transition, "time_outs_deferred", None)
        self._keep = self.kernels.record(self, self.step, tr, gamma)
        self.step += 1

    def clear(self):
        self.step = 0

    def compute_returns(self, last_values, gamma, lam):
        """GAE (rollout_storage.py:76-90); global normalisation across ranks."""
        self.kernels.gae(self, last_values, gamma, lam)
        count = float(self.advantages.numel())
        if _world() > 1:
            torch.distributed.all_reduce(self.adv_stats)
            count *= _world()
        self.kernels.normalize(self, count)

    def get_statistics(self):
        done = self.dones.clone()
        done[-1] = 1
        flat_dones = done.permute(1, 0, 2).reshape(-1, 1)
        done_indices = torch.cat((flat_dones.new_tensor([-1], dtype=torch.int64),
                                  flat_dones.nonzero(as_tuple=False)[:, 0]))
        return (done_indices[1:] - done_indices[:-1]).float().mean(), self.rewards.mean()

    def flat_batch(self):
        """The (T n, ...) views a mini-batch is gathered from, in the order PPO._minibatch_step unpacks them: obs,
        critic obs (the same buffer), privileged obs, history, actions, values, advantages, returns, log-prob, mu,
        sigma (rollout_storage.py:118-136)."""
        return [x.flatten(0, 1) for x in (self.observations, self.observations, self.privileged_observations,
                                          self.observation_histories, self.actions, self.values, self.advantages,
                                          self.returns, self.actions_log_prob, self.mu, self.sigma)]

    def mini_batch_generator(self, num_mini_batches, num_epochs=8, generator=None):
        batch_size = self.num_envs * self.num_transitions_per_env
        mb = batch_size // num_mini_batches
        indices = torch.randperm(num_mini_batches * mb, device=self.device, generator=generator)
        flat = self.flat_batch()
        bins = self.env_bins.flatten(0, 1)
        for _ in range(num_epochs):
            for i in range(num_mini_batches):
                idx = indices[i * mb:(i + 1) * mb]
                b = [x[idx] for x in flat]
                yield (*b, None, bins[idx])
