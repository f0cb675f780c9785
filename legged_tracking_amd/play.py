"""python -m legged_tracking_amd.play LOGDIR --out DIR [--steps 500] [--envs 16] [--width 640] [--height 480]
                                      [--terrain single_path|narrow_path|random_pyramid]
                                      [--deterministic] [--seed 11]

What the reference's scripts/eval.py:68-173 does, without the plots: load a Runner checkpoint (LOGDIR/ac_weights.pt
or LOGDIR/checkpoints/ac_weights.pt; the Cfg of LOGDIR/parameters.pkl when it is there), build a 4 x 4 tunnel grid
with the domain randomisation switched off and record_all_envs on, run the policy and write one GIF per env
(env_{i}.gif; .npy without PIL) from render_all_envs().  The tunnel is the checkpoint's own terrain_type
(single_path without a parameters.pkl) unless --terrain names another producer.

Either learner's checkpoint plays: the module is rebuilt from the state dict (checkpoint.load_actor_critic: the
ppo_cse module, or ppo_cse_cnn's with the MLP or the CNN encoder) and driven through policy_kernels.fused_inference, i.e.
go1_policy_forward in student mode (behind go1_heightmap_encode for the encoder module).  As eval.py:49,64 calls
act(), the actions are Normal(mean, std) draws, here in-kernel and keyed by --seed; --deterministic plays the mean.
Without a parameters.pkl a ppo_cse or MLP-encoder checkpoint plays on readme_config when its widths fit, a CNN
checkpoint on the 61 x 31 scan over the README extents with one frame of history; anything else asks for the file."""
import argparse
import os
import pickle

import numpy as np
import torch

from . import checkpoint as CK, config as CF, policy_kernels as PK, video
from .env import HistoryWrapper, TrajectoryTrackingEnv

# scripts/eval.py:89-101, and randomize_rigids_after_start: eval.py leaves it on, where it redraws nothing once every
# randomize_* flag below is off; here it would still cost the randomiser's launch behind every step
DR_OFF = ("push_robots", "randomize_rigids_after_start", "randomize_friction", "randomize_gravity",
          "randomize_restitution", "randomize_motor_offset", "randomize_motor_strength",
          "randomize_friction_indep", "randomize_ground_friction", "randomize_base_mass",
          "randomize_Kd_factor", "randomize_Kp_factor", "randomize_joint_friction", "randomize_com_displacement")


_find = CK.find


def _apply(section, values):
    """Saved {key: value} onto a Cfg section; a nested dict goes into the sub-section of that name
    (terrain.top / terrain.bottom, sim.physx)."""
    for k, v in values.items():
        if isinstance(v, dict) and isinstance(getattr(section, k, None), type):
            _apply(getattr(section, k), v)
        else:
            setattr(section, k, v)


CNN_GRID = (61, 31)  # the map of the reference's CNN encoder (actor_critic.py:45), over the README scan's extents


def checkpoint_cfg(logdir, n_envs, rows, cols, terrain=None, dr_off=True):
    """The Cfg a checkpoint is replayed on: readme_config on a rows x cols grid, overridden by parameters.pkl
    ({section: {key: value}}); without that file, a CNN checkpoint gets the 61 x 31 full scan with one frame of
    history (the heads see the last frame only).  `terrain` replaces the terrain_type (the checkpoint's, or
    single_path); dr_off switches the domain randomisation off as eval.py:89-101 does."""
    cfg = CF.readme_config(n_envs=n_envs, terrain="single_path", rows=rows, cols=cols)
    pkl = _find(logdir, "parameters.pkl")
    if pkl is not None:
        with open(pkl, "rb") as f:
            saved = pickle.load(f)
        for section, values in saved.items():
            if hasattr(cfg, section) and isinstance(values, dict):
                _apply(getattr(cfg, section), values)
    else:
        weights = _find(logdir, "ac_weights.pt")
        if weights is not None and CK.describe(torch.load(weights, map_location="cpu",
                                                          weights_only=True))["kind"] == "cnn":
            x, y = cfg.terrain.measured_points_x, cfg.terrain.measured_points_y
            cfg.terrain.measured_points_x = np.linspace(np.min(x), np.max(x), CNN_GRID[0])
            cfg.terrain.measured_points_y = np.linspace(np.min(y), np.max(y), CNN_GRID[1])
            cfg.terrain.measure_front_half = False
            cfg.env.num_observation_history = 1
            cfg.env.num_observations = cfg.env.num_scalar_observations = CF.obs_layout(cfg)["width"]
    if terrain is not None:
        cfg.terrain.terrain_type = terrain
    cfg.env.num_envs = int(n_envs)
    cfg.terrain.num_rows, cfg.terrain.num_cols = int(rows), int(cols)
    if dr_off:
        for k in DR_OFF:
            setattr(cfg.domain_rand, k, False)
    return cfg


def load_policy_module(logdir, cfg, env):
    """checkpoint.load_actor_critic for a built env; without a parameters.pkl a checkpoint that does not fit the
    default Cfg asks for the file."""
    try:
        return CK.load_actor_critic(logdir, cfg, env.num_obs, env.num_privileged_obs, env.num_obs_history,
                                    env.num_actions, env.device)
    except ValueError as e:
        if _find(logdir, "parameters.pkl") is not None:
            raise
        raise ValueError(f"{e}.  {logdir} has no parameters.pkl: put the run's parameters.pkl (Runner.save() writes "
                         f"it next to ac_weights.pt) there, so that the env is rebuilt as it was trained") from e


def load_cfg(logdir, n_envs, width, height, terrain=None):
    """readme_config on a 4 x 4 grid, overridden by parameters.pkl ({section: {key: value}}) and then by
    eval.py's play settings (:82-101).  `terrain` replaces the terrain_type (the checkpoint's, or single_path)."""
    # a 4 x 4 grid (:87-88); fewer than 16 envs get the largest square grid that their number fills evenly
    g = max(k for k in (1, 2, 3, 4) if n_envs % (k * k) == 0)
    cfg = checkpoint_cfg(logdir, n_envs, g, g, terrain)
    e = cfg.env
    e.recording_width_px, e.recording_height_px = int(width), int(height)
    e.num_envs, e.look_from_back, e.record_all_envs = int(n_envs), True, True
    cfg.terrain.num_rows = cfg.terrain.num_cols = g
    for k in DR_OFF:
        setattr(cfg.domain_rand, k, False)
    return cfg


def play(logdir, out, steps=500, envs=16, width=640, height=480, device="cuda:0", seed=11, terrain=None,
         deterministic=False):
    """Returns the files written, one per env."""
    if _find(logdir, "ac_weights.pt") is None:
        raise FileNotFoundError(f"no ac_weights.pt under {logdir}")
    envs = int(envs)
    n_built = -(-envs // 16) * 16  # the HIP step takes multiples of 16 envs; the first `envs` are written
    cfg = load_cfg(logdir, n_built, width, height, terrain)
    env = HistoryWrapper(TrajectoryTrackingEnv(sim_device=device, headless=True, cfg=cfg, seed=seed))
    ac = load_policy_module(logdir, cfg, env)
    policy = PK.fused_inference(ac, sample=None if deterministic else seed)
    obs = env.reset()
    frames = []
    with torch.no_grad():
        for _ in range(int(steps)):
            obs, _, _, _ = env.step(policy(obs))
            frames.append(np.stack(env.render_all_envs()[:envs]))
    env.close()
    per_env = np.stack(frames).transpose(1, 0, 2, 3, 4)  # (env, step, H, W, 4)
    return [video.save_frames(f, os.path.join(out, f"env_{i}.gif"), fps=1 / env.dt) for i, f in enumerate(per_env)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("logdir")
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--terrain", default=None, choices=list(CF.TUNNEL_TYPES),
                    help="tunnel producer (default: the checkpoint's terrain_type, single_path without one)")
    ap.add_argument("--deterministic", action="store_true", help="play the action mean instead of sampling")
    ap.add_argument("--seed", type=int, default=11, help="env seed and key of the in-kernel action sampling")
    a = ap.parse_args(argv)
    for p in play(a.logdir, a.out, a.steps, a.envs, a.width, a.height, a.device, seed=a.seed, terrain=a.terrain,
                  deterministic=a.deterministic):
        print(p)


if __name__ == "__main__":
    main()
