"""The training loop of both learners: go1_gym_learn/ppo_cse/__init__.py and ppo_cse_cnn/__init__.py, which differ in
the actor-critic class alone."""
import contextlib
import copy
import os
import time

import numpy as np
import torch

from . import checkpoint
from .actor_critic import AC_Args, ActorCritic, ActorCriticCNN, _Args
from .ppo import PPO
from .storage import _world


class RunnerArgs(_Args):
    """go1_gym_learn/ppo_cse/__init__.py:47-63."""
    algorithm_class_name = "RMA"
    num_steps_per_env = 24
    max_iterations = 1500
    save_interval = 400
    save_video_interval = 100
    log_freq = 10
    resume = False
    load_run = -1
    checkpoint = -1
    resume_path = None
    resume_curriculum = True


@contextlib.contextmanager
def _rollout_outputs(env):
    """The rollout reads neither the contact forces nor the aux block (ppo_cse/__init__.py:164-214): the step leaves
    both stores out (LeggedRobot.set_output_demand) while it runs, and they are back on afterwards."""
    f = getattr(env, "set_output_demand", None)
    if f is None:
        yield
        return
    f(contact_forces=False, aux=False)
    try:
        yield
    finally:
        f(contact_forces=True, aux=True)


class Runner:
    """Runner (ppo_cse/__init__.py:66-357): rollout of num_steps_per_env env steps per
    iteration, GAE, PPO update, checkpoints (ac_weights.pt + TorchScript adaptation
    module and actor body, the formats scripts/eval.py and the deploy stack read)."""

    actor_critic_class = ActorCritic  # RunnerCNN: the height-map encoder module

    def __init__(self, env, device="cpu", runner_args=RunnerArgs, ac_args=AC_Args, log_wandb=False, kernels=None,
                 save_dir=None):
        self.device = device
        self.env = env
        self.runner_args = runner_args
        self.log_wandb = log_wandb
        self.save_dir = save_dir
        ac = self.actor_critic_class(env.num_obs, env.num_privileged_obs, env.num_obs_history,
                                     env.num_actions).to(device)
        if runner_args.resume:
            ac.load_state_dict(torch.load(runner_args.resume, map_location=device, weights_only=True))
        self.alg = PPO(ac, device=device, kernels=kernels)
        self.num_steps_per_env = runner_args.num_steps_per_env
        self.alg.init_storage(env.num_train_envs, self.num_steps_per_env, [env.num_obs], [env.num_privileged_obs],
                              [env.num_obs_history], [env.num_actions])
        self.tot_timesteps = 0
        self.tot_time = 0
        self.current_learning_iteration = 0
        self.last_recording_it = -1000
        self.env.reset()

    def rollout(self, obs, privileged_obs, obs_history, update_model=True, eval_expert=False):
        """One iteration's rollout (ppo_cse/__init__.py:164-214)."""
        n_train = self.env.num_train_envs
        rewards = dones = infos = None
        for _ in range(self.num_steps_per_env):
            actions = self.alg.act(obs[:n_train], privileged_obs[:n_train], obs_history[:n_train])
            if n_train < self.env.num_envs:
                ac = self.alg.actor_critic
                extra = ac.act_teacher(obs_history[n_train:], privileged_obs[n_train:]) if eval_expert else \
                    ac.act_student(obs_history[n_train:])
                actions = torch.cat((actions, extra), dim=0)
            obs_dict, rewards, dones, infos = self.env.step(actions)
            obs, privileged_obs, obs_history = obs_dict["obs"], obs_dict["privileged_obs"], obs_dict["obs_history"]
            if update_model:
                self.alg.process_env_step(rewards[:n_train], dones[:n_train], infos)
            if "train/episode" in infos and self.log_wandb:
                import wandb
                info = infos["train/episode"]
                wandb.log({"train": {k: np.mean(v) for k, v in info.items()}})
        return obs, privileged_obs, obs_history, infos

    def learn(self, num_learning_iterations, init_at_random_ep_len=False, eval_freq=100, curriculum_dump_freq=500,
              eval_expert=False, update_model=True):
        n_train = self.env.num_train_envs
        obs_dict = self.env.get_observations()
        obs, privileged_obs, obs_history = (obs_dict[k].to(self.device) for k in ("obs", "privileged_obs",
                                                                                  "obs_history"))
        self.alg.actor_critic.train()
        if init_at_random_ep_len:
            # as in the reference, this lands on the HistoryWrapper, not the env
            self.env.episode_length_buf = torch.randint_like(self.env.episode_length_buf,
                                                             high=int(self.env.max_episode_length))
        for it in range(num_learning_iterations):
            start = time.time()
            with torch.inference_mode(), _rollout_outputs(self.env):
                obs, privileged_obs, obs_history, infos = self.rollout(obs, privileged_obs, obs_history,
                                                                       update_model, eval_expert)
                if update_model:
                    self.alg.compute_returns(obs_history[:n_train], privileged_obs[:n_train])
            if update_model:
                losses = self.alg.update()
            else:
                losses = (0.0,) * 8
            if self.log_wandb:
                import wandb
                keys = ("mean_value_loss", "mean_surrogate_loss", "adaptation_loss", "mean_decoder_loss",
                        "mean_decoder_loss_student", "mean_adaptation_module_test_loss", "mean_decoder_test_loss",
                        "mean_decoder_test_loss_student")
                wandb.log({"metrics": dict(zip(keys, losses))})
            if self.runner_args.save_video_interval and self.log_wandb:
                self.log_video(it)
            self.tot_timesteps += self.num_steps_per_env * self.env.num_envs
            self.tot_time += time.time() - start
            self.current_learning_iteration = it
            if it % self.runner_args.save_interval == 0:
                self.save(self.checkpoint_dir())
        self.save(self.checkpoint_dir())

    def log_video(self, it):
        """log_video (ppo_cse/__init__.py:322-336): arm a recording every save_video_interval iterations and log
        the episode once it is complete; with save_dir set the episode is also written to videos/{it:05d}.gif."""
        if it - self.last_recording_it >= self.runner_args.save_video_interval:
            self.env.start_recording()
            self.last_recording_it = it
        frames = self.env.get_complete_frames()
        if len(frames) > 0:
            self.env.pause_recording()
            import wandb
            frames_np = np.stack(frames).transpose(0, 3, 1, 2)
            # no step=: this Runner's other wandb.log calls use wandb's own step counter
            wandb.log({"train": {"video": wandb.Video(frames_np, fps=1 / self.env.dt, format="mp4")}})
            if self.save_dir is not None:
                from . import video
                video.save_frames(frames, os.path.join(self.save_dir, "videos", f"{it:05d}.gif"), fps=1 / self.env.dt)

    def checkpoint_dir(self):
        """Where the reference's Runner writes checkpoints (ppo_cse/__init__.py:276-279):
        wandb.run.dir/checkpoints with wandb logging, last_run/checkpoints otherwise."""
        if self.save_dir is not None:
            return self.save_dir
        if self.log_wandb:
            import wandb
            return os.path.join(wandb.run.dir, "checkpoints")
        return "last_run/checkpoints"

    def save(self, save_path=None):
        """ac_weights.pt + adaptation_module_latest.jit + body_latest.jit (__init__.py:274-319) and parameters.pkl
        (the Cfg, which the reference pickles at construction, :81-84), uploaded with wandb.save when logging to
        wandb (:294-297)."""
        if _world() > 1 and torch.distributed.get_rank() != 0:
            return
        save_path = save_path or self.checkpoint_dir()
        os.makedirs(save_path, exist_ok=True)
        ac = self.alg.actor_critic
        paths = [os.path.join(save_path, "ac_weights.pt"), os.path.join(save_path, "adaptation_module_latest.jit"),
                 os.path.join(save_path, "body_latest.jit")]
        torch.save(ac.state_dict(), paths[0])
        torch.jit.script(copy.deepcopy(ac.adaptation_module).to("cpu")).save(paths[1])
        torch.jit.script(copy.deepcopy(ac.actor_body).to("cpu")).save(paths[2])
        cfg = getattr(self.env, "cfg", None)
        if cfg is not None:  # the run's Cfg, which play / evaluate rebuild the env from
            paths.append(checkpoint.save_parameters(cfg, save_path))
        if self.log_wandb:
            import wandb
            for path in paths:
                wandb.save(path)

    def get_inference_policy(self, device=None):
        self.alg.actor_critic.eval()
        if device is not None:
            self.alg.actor_critic.to(device)
        return self.alg.actor_critic.act_inference

    def get_expert_policy(self, device=None):
        self.alg.actor_critic.eval()
        if device is not None:
            self.alg.actor_critic.to(device)
        return self.alg.actor_critic.act_expert


class RunnerCNN(Runner):
    """ppo_cse_cnn/__init__.py:66-357 (rollout_cnn.Runner): Runner around the height-map encoder module."""
    __module__, __qualname__ = ActorCriticCNN.__module__, "Runner"
    actor_critic_class = ActorCriticCNN
