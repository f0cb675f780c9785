"""The reference's unchanged scripts/train.py with its DEFAULT learner (no --old_ppo: go1_gym_learn.ppo_cse_cnn) runs
on this package (legged_tracking_amd.compat -> rollout_cnn).

Container-only (marker `reference`, as tests/test_compat.py): the step and the rollout kernels are replaced by
their CPU test doubles; without --measure_front_half the frame has 503 observations and the encoder takes the
2 x 21 x 11 map.  One learning iteration, the three checkpoint files, and ac_weights.pt loads into a fresh module.
"""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

REF_TRAIN = "/root/reference/scripts/train.py"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.reference,
              pytest.mark.skipif(not os.path.exists(REF_TRAIN), reason="reference checkout not present")]


def test_reference_train_script_default_learner_runs_through_compat(tmp_path):
    script = tmp_path / "run.py"
    script.write_text(textwrap.dedent(f"""
        import sys
        sys.dont_write_bytecode = True
        sys.path.insert(0, {REPO!r})
        from legged_tracking_amd import compat, env as E, rollout as R, rollout_cnn as RC
        from tests.cpu_backend import OracleBackend
        from tests.rollout_ref import TorchRolloutKernels
        init = E.LeggedRobot.__init__
        def env_init(self, cfg, *a, **k):
            k["backend"] = OracleBackend
            return init(self, cfg, *a, **k)
        E.LeggedRobot.__init__ = env_init
        st_init = R.RolloutStorage.__init__
        def storage_init(self, *a, **k):
            k["kernels"] = TorchRolloutKernels()
            return st_init(self, *a, **k)
        R.RolloutStorage.__init__ = storage_init
        run_init = R.Runner.__init__
        def runner_init(self, env, device="cpu", *a, **k):
            run_init(self, env, "cpu", *a, **k)
            print("MODULE", type(self.alg.actor_critic).__module__, self.alg.actor_critic.height_map_shape,
                  env.num_obs, self.alg.actor_critic.policy_input_dim)
        R.Runner.__init__ = runner_init
        R.RunnerArgs.num_steps_per_env = 4
        R.PPO_Args.num_learning_epochs = 1
        compat.main([{REF_TRAIN!r}, "--headless", "--terrain", "single_path", "--camera_zero",
                     "--penalty_scaler", "1.0", "--strategy", "e2e", "--terminal_body_height", "0.0",
                     "--device", "0", "--logdir", {str(tmp_path / "logs")!r}])
        print("RAN", R.RunnerArgs.save_video_interval, RC.AC_Args.height_map_shape)
    """))
    env = dict(os.environ, GO1_NUM_ENVS="1024", GO1_MAX_ITERATIONS="1", GO1_GYM_ROOT=str(tmp_path),
               PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg")
    r = subprocess.run([sys.executable, str(script)], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "MODULE legged_tracking_amd.rollout_cnn (2, 21, 11) 503 338" in r.stdout
    assert "RAN 500 (2, 21, 11)" in r.stdout  # train.py:65, :243 mutated the classes we exported
    ck = tmp_path / "last_run" / "checkpoints"
    for f in ("ac_weights.pt", "body_latest.jit", "adaptation_module_latest.jit"):
        assert (ck / f).exists(), f
    sys.path.insert(0, REPO)
    from legged_tracking_amd import rollout_cnn as RC
    args = type("A", (RC.AC_Args,), dict(height_map_shape=(2, 21, 11)))
    ac = RC.ActorCritic(503, 2, 5 * 503, 12, ac_args=args)
    sd = torch.load(ck / "ac_weights.pt", weights_only=True, map_location="cpu")
    assert sd["adaptation_module.0.weight"].shape[1] == 338  # policy_input, not the history
    ac.load_state_dict(sd)
