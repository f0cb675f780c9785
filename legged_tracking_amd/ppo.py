"""PPO with the adaptation-module regression, for both actor-critic modules: go1_gym_learn/ppo_cse/ppo.py, and
ppo_cse_cnn/ppo.py, which differs in one line (:170-171, the adaptation step goes through process_obs_history), taken
from the module here (adaptation_pred_train).

MI355X mapping: the rollout's act + evaluate is the fused policy kernel (policy_kernels); the update is the
hand-written HIP engine (ppo_engine.PPOEngine, csrc/ppo_update.hip) where _engine_on says so, else torch autograd
with a fused Adam, captured into a HIP graph for the plain module.  With torch.distributed initialised the gradients
and the KL estimate are all-reduced, so that every rank follows the same optimisation trajectory as one large-batch
run.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ppo_engine
from .actor_critic import _Args
from .storage import RolloutStorage, _world


class PPO_Args(_Args):
    """go1_gym_learn/ppo_cse/ppo.py:13-30."""
    value_loss_coef = 1.0
    use_clipped_value_loss = True
    clip_param = 0.2
    entropy_coef = 0.01
    num_learning_epochs = 5
    num_mini_batches = 4
    learning_rate = 1.0e-3
    adaptation_module_learning_rate = 1.0e-3
    num_adaptation_module_substeps = 1
    schedule = "adaptive"
    gamma = 0.99
    lam = 0.95
    desired_kl = 0.01
    max_grad_norm = 1.0
    selective_adaptation_module_loss = False


# Which encoder modes take the HIP update engine (ppo_engine.PPOEngine with go1_ppo_dims.enc_mode) in PPO.update
# by default.  The engine has the MLP encoder (ppo_engine.encoder_supported) and the CNN encoder on the (2, 61, 31)
# map (ppo_engine.conv_encoder_supported, csrc/ppo_conv.h); both stay off until their update-time tables
#  are weighed.
# GO1_PPO_ENCODER_ENGINE=1 / 0 overrides the default for a run; GO1_PPO_ENGINE=0 switches every engine off.
ENGINE_DEFAULT = {"mlp": False, "cnn": False}


def encoder_engine_on(ac):
    """The switch PPO._engine_on consults for the encoder module (the architecture check is ppo_engine's)."""
    env = os.environ.get("GO1_PPO_ENCODER_ENGINE")
    if env in ("0", "1"):
        return env == "1"
    return ENGINE_DEFAULT["cnn" if ac.use_cnn else "mlp"]


class PPO:
    """PPO with the adaptation-module regression (ppo.py:33-206)."""

    def __init__(self, actor_critic, device="cpu", kernels=None):
        self.device = device
        self.actor_critic = actor_critic.to(device)
        self.storage = None
        self.kernels = kernels
        # On the GPU: fused Adam (one kernel per step instead of a foreach chain), its learning rate a device
        # tensor so that the adaptive schedule (ppo.py:124-136) runs on the device -- no host sync per
        # mini-batch; the rate is computed in f64 as the reference's Python floats are, and the f32 copy the
        # kernel reads is the value the foreach path would cast to.  On the CPU: the reference's path.
        self._dev_lr = torch.device(device).type == "cuda"
        params = list(self.actor_critic.parameters())
        # The mini-batch step (forward, backward, gradient clip, both Adam steps, the adaptive rate) is
        # captured once into a HIP graph and replayed for every later mini-batch (GO1_PPO_GRAPH=0: eager):
        # it is ~150 small launches whose host issue left the GPU idle between them.  One rank only (the
        # gradient all-reduce stays eager).
        # The engine's update is captured by GO1_PPO_GRAPH alone; `graph_capture` is the module's word on its torch
        # update (actor_critic.ActorCriticCNN: eager).
        self._engine_graph = self._dev_lr and os.environ.get("GO1_PPO_GRAPH", "1") != "0"
        self._graph_on = self._engine_graph and getattr(actor_critic, "graph_capture", True)
        self._graph = self._graph_key = None
        self._graph_warm = 0
        self._graph_idx = self._graph_acc = self._graph_draw = None  # static buffers of the captured step
        self._side = None  # the one stream of warm-up and capture
        self._engine = None  # ppo_engine.PPOEngine, created by the first update() that runs on it
        if self._dev_lr:
            self._lr64 = torch.tensor(PPO_Args.learning_rate, dtype=torch.float64, device=device)
            self._lr32 = torch.tensor(PPO_Args.learning_rate, dtype=torch.float32, device=device)
            cap = self._graph_on
            self.optimizer = torch.optim.Adam(params, lr=self._lr32, fused=True, capturable=cap)
            self.adaptation_module_optimizer = torch.optim.Adam(params, lr=PPO_Args.adaptation_module_learning_rate,
                                                                fused=True, capturable=cap)
        else:
            self.optimizer = torch.optim.Adam(params, lr=PPO_Args.learning_rate)
            self.adaptation_module_optimizer = torch.optim.Adam(params, lr=PPO_Args.adaptation_module_learning_rate)
        self.transition = RolloutStorage.Transition()
        self.learning_rate = PPO_Args.learning_rate
        self.fused = None  # FusedPolicy once the storage (and its kernels) exist
        self.sample_seed = 0x5EED
        self._sample_step = 0
        self.env_id_offset = 0
        if _world() > 1:  # every rank starts from rank 0's weights
            for p in self.actor_critic.parameters():
                torch.distributed.broadcast(p.data, 0)

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, privileged_obs_shape,
                     obs_history_shape, action_shape):
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape, privileged_obs_shape,
                                      obs_history_shape, action_shape, self.device, kernels=self.kernels)
        pol = getattr(self.storage.kernels, "policy", None)
        self.fused = pol(self.actor_critic) if pol is not None else None
        if _world() > 1:
            self.env_id_offset = torch.distributed.get_rank() * num_envs

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    def act(self, obs, privileged_obs, obs_history):
        ac = self.actor_critic
        t = self.transition
        if self.fused is not None and not torch.is_grad_enabled():
            # one kernel: adaptation module + actor + critic + Normal(mean, std) sample + log_prob
            self._sample_step += 1
            t.action_mean, t.values, _, t.actions, t.action_sigma, t.actions_log_prob = self.fused.forward(
                obs_history, privileged_obs, sample=(self.sample_seed, self._sample_step, self.env_id_offset))
        else:
            t.actions = ac.act(obs_history).detach()
            t.values = ac.evaluate(obs_history, privileged_obs).detach()
            t.actions_log_prob = ac.get_actions_log_prob(t.actions).detach()
            t.action_mean = ac.action_mean.detach()
            t.action_sigma = ac.action_std.detach()
        t.observations = obs
        t.critic_observations = obs
        t.privileged_observations = privileged_obs
        t.observation_histories = obs_history
        return t.actions

    def process_env_step(self, rewards, dones, infos):
        """Records the transition; the time-out bootstrap r += gamma * V * time_outs
        (ppo.py:85-87) is applied inside the record kernel."""
        t = self.transition
        t.rewards = rewards
        t.dones = dones
        t.time_outs_deferred = None
        deferred = getattr(infos, "deferred_time_outs", None)
        if deferred is not None and "time_outs" in infos:
            # the env's pending extras["time_outs"] rebinding is resolved by the record kernel
            # (no separate sync launch); the tensor it leaves current is the one read here
            t.time_outs, t.time_outs_deferred = deferred()
        else:
            t.time_outs = infos["time_outs"] if "time_outs" in infos else None
        self.storage.add_transitions(t, gamma=PPO_Args.gamma)
        t.clear()
        self.actor_critic.reset(dones)

    def compute_returns(self, last_critic_obs, last_critic_privileged_obs):
        if self.fused is not None and not torch.is_grad_enabled():
            last_values = self.fused.forward(last_critic_obs, last_critic_privileged_obs)[1]
        else:
            last_values = self.actor_critic.evaluate(last_critic_obs, last_critic_privileged_obs).detach()
        self.storage.compute_returns(last_values, PPO_Args.gamma, PPO_Args.lam)

    def _allreduce_grads(self):
        w = _world()
        if w == 1:
            return
        params = [p for p in self.actor_critic.parameters() if p.grad is not None]
        flat = torch.cat([p.grad.reshape(-1) for p in params])
        torch.distributed.all_reduce(flat)
        flat /= w
        off = 0
        for p in params:
            k = p.numel()
            p.grad.copy_(flat[off:off + k].view_as(p.grad))
            off += k

    def _minibatch_step(self, batch, acc, sample=True):
        """One mini-batch of PPO.update (ppo.py:107-201): the surrogate / value / entropy loss and its Adam step,
        the adaptive learning rate, then the adaptation-module regression step(s).  Loss values accumulate
        into `acc` on the device.  sample=False leaves out ac.act's unused sample (the graphed loop draws it
        outside the graph: torch's generator cannot be advanced inside a HIP capture here)."""
        A = PPO_Args
        ac = self.actor_critic
        (obs_b, critic_obs_b, priv_b, hist_b, act_b, target_v_b, adv_b, ret_b, old_logp_b, old_mu_b,
         old_sigma_b) = batch
        ac.update_distribution_train(hist_b)
        if sample:
            ac.distribution.sample()  # ac.act's (unused) sample: the reference's torch RNG consumption (ppo.py:110)
        logp_b = ac.get_actions_log_prob(act_b)
        value_b = ac.evaluate_train(hist_b, priv_b)
        mu_b, sigma_b, entropy_b = ac.action_mean, ac.action_std, ac.entropy
        if A.desired_kl is not None and A.schedule == "adaptive":
            with torch.inference_mode():
                kl = torch.sum(torch.log(sigma_b / old_sigma_b + 1.0e-5) +
                               (torch.square(old_sigma_b) + torch.square(old_mu_b - mu_b)) /
                               (2.0 * torch.square(sigma_b)) - 0.5, axis=-1)
                kl_mean = torch.mean(kl)
                if _world() > 1:
                    kl_mean = kl_mean.clone()
                    torch.distributed.all_reduce(kl_mean)
                    kl_mean /= _world()
            if self._dev_lr:
                with torch.no_grad():
                    k, lr = kl_mean.double(), self._lr64
                    new = torch.where(k > A.desired_kl * 2.0, torch.clamp(lr / 1.5, min=1e-5),
                                      torch.where((k < A.desired_kl / 2.0) & (k > 0.0),
                                                  torch.clamp(lr * 1.5, max=1e-2), lr))
                    self._lr64.copy_(new)
                    self._lr32.copy_(new)
            else:
                kl_mean, lr = float(kl_mean), self.learning_rate
                if kl_mean > A.desired_kl * 2.0:
                    lr = max(1e-5, lr / 1.5)
                elif A.desired_kl / 2.0 > kl_mean > 0.0:
                    lr = min(1e-2, lr * 1.5)
                self._set_lr(lr)
        ratio = torch.exp(logp_b - torch.squeeze(old_logp_b))
        surrogate = -torch.squeeze(adv_b) * ratio
        surrogate_clipped = -torch.squeeze(adv_b) * torch.clamp(ratio, 1.0 - A.clip_param, 1.0 + A.clip_param)
        surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
        if A.use_clipped_value_loss:
            value_clipped = target_v_b + (value_b - target_v_b).clamp(-A.clip_param, A.clip_param)
            value_loss = torch.max((value_b - ret_b).pow(2), (value_clipped - ret_b).pow(2)).mean()
        else:
            value_loss = (ret_b - value_b).pow(2).mean()
        loss = surrogate_loss + A.value_loss_coef * value_loss - A.entropy_coef * entropy_b.mean()
        self.optimizer.zero_grad()
        loss.backward()
        self._allreduce_grads()
        nn.utils.clip_grad_norm_(ac.parameters(), A.max_grad_norm)
        self.optimizer.step()
        acc[0] += value_loss.detach()
        acc[1] += surrogate_loss.detach()
        num_train = int(priv_b.shape[0] // 5 * 4)
        for _ in range(A.num_adaptation_module_substeps):
            pred = ac.adaptation_pred_train(hist_b)
            with torch.no_grad():
                target = priv_b
            # every column (ppo.py:193: linspace(0, w - 1, w) as an index), or column 0
            sel = 0 if A.selective_adaptation_module_loss else slice(None)
            adapt_loss = F.mse_loss(pred[:num_train, sel], target[:num_train, sel])
            adapt_test = F.mse_loss(pred[num_train:, sel], target[num_train:, sel])
            self.adaptation_module_optimizer.zero_grad()
            adapt_loss.backward()
            self._allreduce_grads()
            self.adaptation_module_optimizer.step()
            acc[2] += adapt_loss.detach()
            acc[3] += adapt_test.detach()

    GRAPH_WARMUP = 3  # eager mini-batches (on a side stream) before the capture: lazy handles and optimizer state

    _ARG_KEYS = ("clip_param", "value_loss_coef", "use_clipped_value_loss", "entropy_coef", "max_grad_norm",
                 "desired_kl", "schedule", "num_adaptation_module_substeps", "selective_adaptation_module_loss")

    def _torch_graph_key(self, mb, flat):
        """What a captured mini-batch step bakes in: the batch size, the storage it gathers from, the PPO_Args
        scalars of the loss / clip / schedule, and the optimizers' state tensors (load_state_dict replaces them)."""
        opt_state = tuple(id(t) for o in (self.optimizer, self.adaptation_module_optimizer)
                          for s in o.state.values() for t in s.values() if isinstance(t, torch.Tensor))
        return (mb, tuple(x.data_ptr() for x in flat), tuple(getattr(PPO_Args, k) for k in self._ARG_KEYS), opt_state)

    def _graphed_minibatches(self, acc):
        """The mini-batch loop of update() with the step replayed from a HIP graph: the batch is gathered inside the
        graph from the storage with a static index buffer, so a mini-batch costs one index copy and one replay."""
        A = PPO_Args
        st = self.storage
        batch = st.num_envs * st.num_transitions_per_env
        mb = batch // A.num_mini_batches
        indices = torch.randperm(A.num_mini_batches * mb, device=self.device)  # mini_batch_generator's draw
        flat = st.flat_batch()
        key = self._torch_graph_key(mb, flat)
        if self._graph is not None and self._graph_key != key:
            self._graph = None  # new storage, PPO_Args or optimizer state: capture again
            self._graph_warm = 0
        if self._graph is None and self._graph_warm == 0:
            self._graph_idx = torch.empty(mb, dtype=torch.int64, device=self.device)
            self._graph_acc = torch.zeros(4, dtype=torch.float32, device=self.device)
        idx, gacc = self._graph_idx, self._graph_acc
        # ac.act's unused sample per mini-batch, drawn before each step with the same shape: the same torch
        # generator advance as the eager loop's (the values are discarded there too)
        na = st.actions.shape[-1]
        if self._graph_draw is None or self._graph_draw[0].shape != (mb, na):
            self._graph_draw = (torch.zeros(mb, na, device=self.device), torch.ones(mb, na, device=self.device))

        def step():
            # the generator's obs and critic-obs batches (flat[0:2]) are never read by the step (the nets take the
            # history and the privileged obs): not gathered, two index kernels less per mini-batch
            self._minibatch_step([None, None] + [x[idx] for x in flat[2:]], gacc, sample=False)

        # warm-up and capture run on ONE persistent side stream: the parameters' AccumulateGrad nodes are created
        # there and every later backward (warm-up, capture) runs on the same stream (a fresh stream per warm-up
        # mini-batch made torch warn about a stream mismatch of the accumulation)
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        side = self._side
        for _ in range(A.num_learning_epochs):
            for i in range(A.num_mini_batches):
                idx.copy_(indices[i * mb:(i + 1) * mb])
                torch.normal(*self._graph_draw)
                if self._graph is not None:
                    self._graph.replay()
                    continue
                side.wait_stream(torch.cuda.current_stream(self.device))
                if self._graph_warm < self.GRAPH_WARMUP:
                    with torch.cuda.stream(side):
                        step()
                    self._graph_warm += 1
                else:
                    torch.cuda.synchronize(self.device)
                    for p in self.actor_critic.parameters():
                        p.grad = None
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=side):
                        step()
                    self._graph = g
                    self._graph_key = self._torch_graph_key(mb, flat)  # the optimizer state exists by now
                    with torch.cuda.stream(side):
                        g.replay()  # the capture recorded the step without running it
                torch.cuda.current_stream(self.device).wait_stream(side)
        acc += gacc
        gacc.zero_()

    def _engine_on(self):
        """The hand-written HIP update (ppo_engine.PPOEngine, csrc/ppo_update.hip) on the GPU for the default
        architecture; GO1_PPO_ENGINE=0 selects the torch autograd update (A/B).  The height-map encoder module
        runs on it where encoder_engine_on says so (ENGINE_DEFAULT, GO1_PPO_ENCODER_ENGINE)."""
        if torch.device(self.device).type != "cuda" or os.environ.get("GO1_PPO_ENGINE", "1") == "0":
            return False
        if ppo_engine.supported(self.actor_critic):
            return True
        if not (ppo_engine.encoder_supported(self.actor_critic) or
                ppo_engine.conv_encoder_supported(self.actor_critic)):
            return False
        return encoder_engine_on(self.actor_critic)

    def _set_lr(self, lr):
        """The learning rate of PPO.optimizer, everywhere it is kept: the attribute, the param groups (a device
        tensor with the fused Adam) and the device copies the adaptive schedule steps."""
        self.learning_rate = lr
        for g in self.optimizer.param_groups:
            if isinstance(g["lr"], torch.Tensor):
                g["lr"].fill_(lr)
            else:
                g["lr"] = lr
        if self._dev_lr:
            self._lr64.fill_(lr)
            self._lr32.fill_(lr)

    def update(self):
        A = PPO_Args
        n_up = A.num_learning_epochs * A.num_mini_batches
        n_ad = n_up * A.num_adaptation_module_substeps
        if self._engine_on() and A.num_adaptation_module_substeps == 1:
            if self._engine is None:
                self._engine = ppo_engine.PPOEngine(self)
            sums, lr = self._engine.update(A, A.num_mini_batches, A.num_learning_epochs, _world(),
                                           use_graph=self._engine_graph,
                                           split=os.environ.get("GO1_PPO_SPLIT", "0") == "1")
            self._set_lr(lr)
        else:
            if self._engine is not None:
                self._engine.release_optimizer_state()  # torch's Adam steps per-parameter state of its own
            # the loss means accumulate on the device (ppo.py:186-187, 200-201 call .item() per mini-batch:
            # a host sync each); one copy at the end.
            sums = torch.zeros(4, dtype=torch.float32, device=self.device)  # value, surrogate, adapt, adapt_test
            if self._graph_on and _world() == 1:
                self._graphed_minibatches(sums)
            else:
                gen = self.storage.mini_batch_generator(A.num_mini_batches, A.num_learning_epochs)
                for b in gen:
                    self._minibatch_step(b[:11], sums)
        self.storage.clear()
        if self.fused is not None:
            self.fused.pack()  # the rollout kernel reads the updated weights
        if isinstance(sums, torch.Tensor):  # the torch path's device sums, read once the pack is queued
            sums = sums.cpu().tolist()
            if self._dev_lr:
                self.learning_rate = float(self._lr64)
        return (sums[0] / n_up, sums[1] / n_up, sums[2] / n_ad, 0.0, 0.0, sums[3] / n_ad, 0.0, 0.0)
