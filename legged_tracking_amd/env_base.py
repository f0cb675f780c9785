"""What the trajectory env (env.py) and the velocity env (velocity.py) keep on the host in the same way.

EnvBase owns the rank / world-size resolution, dims and seed, the OUT_RING output rings with their *_buf
views and per-slot dicts, the state views, the per-env Philox draws keyed by global env id (creation-time domain
randomisation), the global gravity schedule (_randomize_gravity, _tick_gravity_schedule), the action and
env-id normalisation, the twelve lazy numpy extras, the reference's recording / render surface (render.py) and the
one path of the add-on launches behind the step kernel and behind a host reset_idx (_after_step, _after_tick,
_after_reset_idx).

Each env keeps what differs: when its step ticks the gravity schedule (after the launch / before it, with
the pre- and post-tick vectors), the initial gravity draw (trajectory only), its aux column layout,
set_output_demand, its episode log and its obs-history mechanism.  step() is host-bound, so the helpers
here are leaf calls: no super().step() chain.
"""
from collections import deque

import numpy as np
import torch

from . import config as CF, layout as L

OUT_RING = 4
_LAZY = object()


def _dist_info():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size()
    except Exception:
        pass
    return 0, 1


class StepExtras(dict):
    """The env's `extras` dict: device-backed entries are materialised on read."""

    def __init__(self, env):
        super().__init__()
        self._env = env
        self._lazy = {}

    def set_lazy(self, key, fn):
        self._lazy[key] = fn
        dict.__setitem__(self, key, _LAZY)

    def __getitem__(self, key):
        if key in ("train/episode", "eval/episode", "timeouts"):
            self._env._flush_episode_log()
        v = dict.__getitem__(self, key)
        return self._lazy[key]() if v is _LAZY else v

    def get(self, key, default=None):
        return self[key] if key in self else default

    def deferred_time_outs(self):
        """extras["time_outs"] with its pending rebinding left to the consumer: returns
        (tensor, (flag, pending, dst) device pointers or None).  The PPO record kernel resolves
        it (ppo.py PPO.process_env_step), saving the sync launch a plain read costs."""
        return self._env._deferred_time_outs()

    def items(self):
        return [(k, self[k]) for k in list(self.keys())]

    def values(self):
        return [self[k] for k in list(self.keys())]


class EnvBase:
    """Host state shared by LeggedRobot and VelocityTrackingEasyEnv.  A subclass calls _init_dims, creates
    self._sim (a native handle or an injected backend) and self.device, then calls _init_host_state."""

    def _init_dims(self, cfg, derived, sim_device, headless, seed, rank, world_size):
        if rank is None or world_size is None:
            r, w = _dist_info()
            rank = r if rank is None else rank
            world_size = w if world_size is None else world_size
        self.rank, self.world_size = rank, world_size
        self.cfg = cfg
        self.eval_cfg = None
        self.sim_device = sim_device
        self.headless = headless
        self.num_obs = int(cfg.env.num_observations)
        self.num_privileged_obs = int(cfg.env.num_privileged_obs)
        self.num_actions = int(cfg.env.num_actions)
        self.num_envs = self.num_train_envs = int(cfg.env.num_envs)
        self.num_eval_envs = 0
        self._n_global = self.num_envs * world_size
        self.seed = int(seed)
        self.dt = derived["dt"]
        self.max_episode_length = derived["max_episode_length"]
        self.reward_scales = dict(derived["reward_scales"])
        self._gravity_interval = int(derived["gravity_rand_interval"])
        self._gravity_duration = int(derived["gravity_rand_duration"])

    def _init_host_state(self):
        n, dev, dr = self.num_envs, self.device, self.cfg.domain_rand
        # output rings: a tensor returned by step() stays valid for OUT_RING - 1 further steps
        self._obs = torch.zeros((OUT_RING, n, self.num_obs), device=dev)
        self._priv = torch.zeros((OUT_RING, n, self.num_privileged_obs), device=dev)
        self._rew = torch.zeros((OUT_RING, n), device=dev)
        self._reset = torch.zeros((OUT_RING, n), dtype=torch.bool, device=dev)
        self._time_out = torch.zeros((OUT_RING, n), dtype=torch.bool, device=dev)
        # the views of one slot, as a step hands them to the kernel, to the add-ons and to its caller
        self._out = [dict(obs=self._obs[s], priv=self._priv[s], rew=self._rew[s], reset=self._reset[s],
                          time_out=self._time_out[s]) for s in range(OUT_RING)]
        self._kout = self._out  # what the step kernel is handed; _init_privileged gives it a priv buffer of its own
        self._slot = 0
        self._last_hist = None
        # _randomize_rigid_body_props at creation: per-env draws keyed by GLOBAL env id (every rank draws the
        # global vector and keeps its slice), so an N-rank run starts from exactly the state one rank with
        # N x the envs does
        st = self._sim.state
        if dr.randomize_friction:
            st["friction"].copy_(self._global_uniform(1, *dr.friction_range))
        else:
            st["friction"].fill_(1.0)
        if dr.randomize_restitution:
            st["restitution"].copy_(self._global_uniform(2, *dr.restitution_range))
        if dr.randomize_base_mass:
            st["payload"].copy_(self._global_uniform(3, *dr.added_mass_range))
        st["motor_strength"].fill_(1.0)
        # gravity: Cfg.sim.gravity and the projection vector -z until the first draw; the draws come from
        # one host RNG that is identical on every rank
        self._host_rng = np.random.default_rng(self.seed)
        self.common_step_counter = 0
        self.gravities = np.zeros(3, np.float32)
        self._sim_gravity = np.asarray(self.cfg.sim.gravity, np.float32)
        self._gravity_vec = np.array([0.0, 0.0, -1.0], np.float32)
        self._grav_version = 0  # bumped by every _randomize_gravity
        self._rng_step = 0
        # measurement hook (bench.py): hipEvent_t pairs to record around the next steps' kernel
        self.kernel_events = deque()

    # ------------------------------------------------------------------ host draws
    def _global_rng(self, tag):
        """numpy Philox stream of (seed, tag): the same on every rank, indexed by global env id."""
        return np.random.Generator(np.random.Philox(key=[self.seed, tag]))

    def _global_uniform(self, tag, lo, hi):
        """(n, 1) f32 U(lo, hi) for this rank's envs, element i = global env rank * n + i."""
        u = self._global_rng(tag).random(self._n_global).astype(np.float32)
        u = u[self.rank * self.num_envs:(self.rank + 1) * self.num_envs, None]
        return torch.from_numpy(u * np.float32(hi - lo) + np.float32(lo)).to(self.device)

    def _randomize_gravity(self, external_force=None):
        """_randomize_gravity: one global draw shared by every env (and rank).  It replaces the
        _sim_gravity / _gravity_vec arrays, so references taken before it keep the old values."""
        if external_force is not None:
            self.gravities[:] = np.asarray(external_force, np.float32)
        elif self.cfg.domain_rand.randomize_gravity:
            lo, hi = self.cfg.domain_rand.gravity_range
            u = self._host_rng.random(3).astype(np.float32)
            self.gravities[:] = u * np.float32(hi - lo) + np.float32(lo)
        self._sim_gravity, self._gravity_vec = CF.gravity_state(self.gravities)
        self._grav_version += 1

    def _tick_gravity_schedule(self):
        """common_step_counter and the global schedule: a draw every gravity_rand_interval steps, zeroed
        gravity_rand_duration steps later."""
        self.common_step_counter += 1
        c, gi = self.common_step_counter, self._gravity_interval
        if c % gi == 0:
            self._randomize_gravity()
        if (c - self._gravity_duration) % gi == 0:
            self._randomize_gravity(np.zeros(3, np.float32))

    # ------------------------------------------------------------------ argument normalisation
    def _as_actions(self, actions):
        """The step's actions as a contiguous f32 (num_envs, num_actions) tensor on the env's device."""
        a = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(actions)
        if a.device != self.device or a.dtype != torch.float32:
            a = a.to(self.device, torch.float32)
        if a.requires_grad:
            a = a.detach()
        if not a.is_contiguous():
            a = a.contiguous()
        if a.shape != (self.num_envs, self.num_actions):
            raise ValueError(f"actions must be ({self.num_envs}, {self.num_actions}), got {tuple(a.shape)}")
        return a

    def _norm_env_ids(self, env_ids):
        """reset_idx's ids as a flat int64 tensor in [0, num_envs) (negative ids wrap, out-of-range ids raise
        as the reference's indexing does); None for an empty list."""
        env_ids = torch.as_tensor(env_ids, device=self.device).long().flatten()
        if env_ids.numel() == 0:
            return None
        if int(env_ids.min()) < -self.num_envs or int(env_ids.max()) >= self.num_envs:
            raise IndexError(f"env id out of range for {self.num_envs} envs")
        return torch.remainder(env_ids, self.num_envs)

    # ------------------------------------------------------------------ views
    @property
    def state(self):
        return self._sim.state

    @property
    def obs_buf(self):
        return self._obs[(self._slot - 1) % OUT_RING]

    @property
    def privileged_obs_buf(self):
        return self._priv[(self._slot - 1) % OUT_RING]

    @property
    def rew_buf(self):
        return self._rew[(self._slot - 1) % OUT_RING]

    @property
    def reset_buf(self):
        return self._reset[(self._slot - 1) % OUT_RING]

    @property
    def time_out_buf(self):
        return self._time_out[(self._slot - 1) % OUT_RING]

    @property
    def episode_length_buf(self):
        return self._sim.state["episode_length"][:, 0]

    @episode_length_buf.setter
    def episode_length_buf(self, v):
        self._sim.state["episode_length"][:, 0].copy_(torch.as_tensor(v, device=self.device))

    @property
    def root_states(self):
        return self._sim.state["root"]

    @property
    def dof_pos(self):
        return self._sim.state["dof_pos"]

    @property
    def dof_vel(self):
        return self._sim.state["dof_vel"]

    # ------------------------------------------------------------------ add-on launches
    _randomizer = None       # randomize.Randomizer, built by _init_randomizer when the Cfg sets one of its flags
    _planner = None          # plan.LocalPlanner, built by the trajectory env when its Cfg plans
    _privileged = None       # privileged.Privileged, built by the trajectory env for a priv_observe_* set of its own

    def _after_step(self, out, hist):
        """The add-ons' launches of one step, behind the step kernel on its stream, each only if present: `out` is
        the step's slot of the output ring, `hist` its copy of obs for the history tap or None.  The order is part of
        the behaviour: the randomiser rewrites priv before anything reads it, and the planner rewrites obs (and the
        commands of the trajectory env's aux block) before the recorder or the tracer run."""
        if self._randomizer is not None:
            # the step's own two columns; with the assembler behind it (_after_tick) nothing reads them
            self._randomizer.step(out["reset"], out["priv"] if self._kout is self._out else None, self._rng_step)
        if self._planner is not None:
            self._planner.step(out, self._planner.heights, hist, self._aux if self._demand[1] else None)
        if self._rec is not None:
            self._record_step(out["reset"])
        if self._tracer is not None:
            self._tracer.push(out["reset"], out["time_out"])

    def _after_tick(self, out):
        """The launch that reads what the step's tick of the gravity schedule changes, behind _after_step and the
        tick: the privileged observation of the step (compute_observations sees the schedule's draw, :826-830)."""
        if self._privileged is not None:
            self._privileged.step(out["priv"], self.gravities)

    def _after_reset_idx(self, env_ids, rng_step):
        """What the add-ons are told of a host reset_idx(env_ids), behind the env's own reset launch: the randomiser
        redraws with the `rng_step` that launch had, the planner and the tracer mark the ended episodes."""
        if self._randomizer is not None:
            self._randomizer.reset_idx(env_ids, rng_step)
        if self._planner is not None:
            self._planner.mark_reset(env_ids)
        if self._tracer is not None:
            self._tracer.mark_reset(env_ids)

    # ------------------------------------------------------------------ after-start randomiser (randomize.py)
    # With Cfg.domain_rand.push_robots or randomize_rigids_after_start, step() issues the randomiser's launch right
    # after the step kernel and reset_idx its redraw; with both off nothing is built and nothing is launched.

    def _init_randomizer(self):
        from . import randomize
        if randomize.wanted(self.cfg):
            self._randomizer = randomize.Randomizer(self)

    @property
    def randomizer(self):
        """The Randomizer behind this env, or None when the Cfg sets neither of its flags."""
        return self._randomizer

    # ------------------------------------------------------------------ privileged observations (privileged.py)
    # With a priv_observe_* set other than friction and restitution, the step kernel writes its two columns into an
    # (n, 2) buffer nothing reads and the assembler's launch fills the step's slot of the (OUT_RING, n, W) ring; with
    # exactly those two nothing is built and the kernel writes the ring itself, as before.

    def _init_privileged(self):
        from . import privileged
        if privileged.wanted(self.cfg):
            step_priv = torch.zeros((self.num_envs, 2), device=self.device)
            self._kout = [dict(o, priv=step_priv) for o in self._out]
            if self.num_privileged_obs > 0:  # no flag at all: an (n, 0) vector, nothing to assemble
                self._privileged = privileged.Privileged(self)

    @property
    def privileged(self):
        """The Privileged assembler behind this env (names, width), or None when the step kernel's own two columns
        are the whole vector."""
        return self._privileged

    @property
    def motor_strengths(self):
        return self._sim.state["motor_strength"]

    @property
    def motor_offsets(self):
        return self._sim.state["motor_offset"]

    @property
    def friction_coeffs(self):
        return self._sim.state["friction"]

    @property
    def restitutions(self):
        return self._sim.state["restitution"]

    @property
    def payloads(self):
        """The reference's tensor of that name: it follows the redraws after start, while the simulated mass (the
        payload plane) stays the creation-time one, as PhysX keeps it."""
        return self._randomizer.payloads if self._randomizer is not None else self._sim.state["payload"]

    def get_observations(self):
        return self.obs_buf

    def get_privileged_observations(self):
        return self.privileged_obs_buf

    # ------------------------------------------------------------------ extras
    def _install_step_extras(self, ex, body_linear_vel_cmd, body_angular_vel_cmd, body_pos):
        """The numpy extras the reference's step builds every time, computed on read (no device->host copy
        per step); the three arguments are the entries that differ between the tasks."""
        ex.set_lazy("joint_pos", lambda: self.dof_pos.cpu().numpy())
        ex.set_lazy("joint_vel", lambda: self.dof_vel.cpu().numpy())
        ex.set_lazy("joint_pos_target", lambda: self.joint_pos_target.cpu().numpy())
        dict.__setitem__(ex, "joint_vel_target", torch.zeros(12))
        ex.set_lazy("body_linear_vel", lambda: self.base_lin_vel.cpu().numpy())
        ex.set_lazy("body_angular_vel", lambda: self.base_ang_vel.cpu().numpy())
        ex.set_lazy("body_linear_vel_cmd", body_linear_vel_cmd)
        ex.set_lazy("body_angular_vel_cmd", body_angular_vel_cmd)
        ex.set_lazy("contact_states",
                    lambda: (self.contact_forces[:, list(L.FEET_INDICES), 2] > 1.0).cpu().numpy().copy())
        ex.set_lazy("foot_positions", lambda: self.foot_positions.cpu().numpy().copy())
        ex.set_lazy("body_pos", body_pos)
        ex.set_lazy("torques", lambda: self.torques.cpu().numpy())

    # ------------------------------------------------------------------ misc API
    # ------------------------------------------------------------------ recording and rendering (render.py)
    # legged_robot_trajectory_tracking.py:1690-1711, :1775-1806.  Nothing is allocated or launched until the first
    # start_recording / render call; while a recording is armed, _after_step issues one recording launch
    # (_record_step), which reads the state planes and the step's reset output only.
    renderer_factory = None  # tests inject a test double; None: render.Renderer
    _renderer = None         # created on first use
    _rec = None              # the renderer while record_now is set (:1777), else None

    def _get_renderer(self):
        if self._renderer is None:
            factory = self.renderer_factory
            if factory is None:
                from . import render
                factory = render.Renderer
            self._renderer = factory(self)
        return self._renderer

    def _records(self):
        """Only the rank that owns global env 0 records; the others keep the surface's empty answers."""
        return self.rank == 0

    def _record_step(self, reset):
        self._rec.record_step(reset)

    def start_recording(self):
        if self._records():
            self._rec = self._get_renderer()
            self._rec.start()

    def pause_recording(self):
        if self._renderer is not None:
            self._renderer.pause()
        self._rec = None

    def start_recording_eval(self):
        pass

    def pause_recording_eval(self):
        pass

    def get_complete_frames(self):
        """[] until the recorded episode of env 0 is complete, then its (240, 360, 4) uint8 frames."""
        return self._renderer.complete_frames() if self._renderer is not None else []

    def get_complete_frames_eval(self):
        return []

    # ------------------------------------------------------------------ episode tracer (trace.py)
    # While a tracer is attached, _after_step issues its push launch last: it reads the state planes and the step's
    # reset / time_out outputs only.  With none attached nothing changes.
    _tracer = None

    def attach_tracer(self, tracer):
        if self._tracer is not None and self._tracer is not tracer:
            raise RuntimeError("the env already has a tracer attached (detach_tracer first)")
        self._tracer = tracer

    def detach_tracer(self):
        self._tracer = None

    def render(self, mode="rgb_array"):
        """render (:1690-1699): env 0 from the follow camera, (240, 360, 4) uint8; None on the ranks that do not own
        global env 0."""
        assert mode == "rgb_array"
        if not self._records():
            return None
        from . import render as R
        r = self._get_renderer()
        return r.render((0,), r.width, r.height, R.MODE_FOLLOW, R.VIEW_NO_CEILING)[0]

    def render_all_envs(self):
        """render_all_envs (:1701-1711): one (recording_height_px, recording_width_px, 4) frame per env with the
        video camera's mode, or None unless cfg.env.record_all_envs."""
        e = self.cfg.env
        if not getattr(e, "record_all_envs", False):
            return None
        frames = self._get_renderer().render(tuple(range(self.num_envs)), e.recording_width_px, e.recording_height_px)
        return list(frames)

    def close(self):
        self._sim.close()
