"""Buffer layouts of the velocity-tracking step (BASELINE configs[1]), shared by the host code, the
C ABI (include/go1_velocity.h) and the tests.  Pure data -- no torch, no GPU.

Reference: go1_gym/envs/base/legged_robot_velocity_tracking.py (bare :N below), CoRLRewards
(go1_gym/envs/rewards/corl_rewards.py), RewardThresholdCurriculum (go1_gym/envs/base/curriculum.py).
"""

NUM_COMMANDS = 15          # x vel, y vel, yaw vel, body height, gait freq, phase, offset, bound, duration,
                           # footswing height, body pitch, body roll, stance width, stance length, aux coef
NUM_OBS = 70               # gravity 3, commands 15, dof pos 12, dof vel 12, actions 12, last actions 12, clock 4
NUM_PRIV = 2
N_CATEGORIES = 4           # pronk, trot, pace, bound (gaitwise_curricula, :1319-1321)
N_COMMAND_SUM_EXTRA = 5    # lin_vel_raw, ang_vel_raw, lin_vel_residual, ang_vel_residual, ep_timesteps (:1446)
MAX_TERMS = 24             # CoRLRewards terms with a nonzero scale (19 in train_velocity_tracking.py)

# ---- per-env f32 uniform draws (torch.rand / rand_like of one step), parity mode; Philox otherwise
VU_CAT_A = 0               # _resample_commands category draw, periodic resample (:760, via :704)
VU_CAT_B = 1               # the same, resample inside reset_idx (:182)
VU_DR_STRENGTH = 2         # _randomize_dof_props every rand_interval (:715-717): strength (1), offsets (12)
VU_RESET_STRENGTH = 15     # _randomize_dof_props in reset_idx (:183): strength (1), offsets (12)
VU_RESET_DOF = 28          # _reset_dofs (:974): 12
VU_RESET_YAW = 40          # _reset_root_states yaw (:1007-1009)
VU_RESET_VEL = 41          # _reset_root_states base velocities (:1014): 6
VU_NOISE = 47              # compute_observations noise (:394): NUM_OBS
VU_PER_ENV = VU_NOISE + NUM_OBS  # 117

# ---- per-env f64 draws of the curriculum's numpy RandomState (Curriculum.sample, curriculum.py:67-89)
VD_CHOICE_A = 0            # rng.choice uniform (periodic resample), then 15 rng.uniform cell draws
VD_CHOICE_B = 16           # the same for the resample in reset_idx
VD_PER_ENV = 32

# The state planes and the reward-term ids are tabulated once, in vel_abi.VEL_STATE_SPEC / vel_abi.VTERM_IDS.
