"""The learner's module layout: one module per concern with no import cycle, the two API modules (rollout,
rollout_cnn) holding every name they held when they held the code, and the actor-critic modules' parameter and
initialisation order.  tests/golden/learner_split/api_names.json was recorded before the split: the names rollout.py
and rollout_cnn.py defined (classes and functions of their own, upper-case constants) and named_parameters() of
three modules."""
import ast
import json
import os
import pickle
import subprocess
import sys

import pytest
import torch

from legged_tracking_amd import actor_critic as AC, rollout as R, rollout_cnn as RC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "legged_tracking_amd")
CONCERNS = ("rollout_lib", "actor_critic", "policy_kernels", "storage", "ppo", "runner")
# no import below module level among these, except the heavy leaf `video` (and third parties: wandb)
ACYCLIC = CONCERNS + ("rollout", "rollout_cnn", "ppo_engine", "checkpoint", "play", "evaluate")
ALLOWED_LATE = {"video"}
with open(os.path.join(REPO, "tests", "golden", "learner_split", "api_names.json")) as f:
    RECORDED = json.load(f)
SIBLINGS = {f[:-3] for f in os.listdir(PKG) if f.endswith(".py")}


def _package_imports(node):
    """The package's own modules an Import / ImportFrom node names."""
    if isinstance(node, ast.ImportFrom) and node.level == 1:
        return {node.module.split(".")[0]} if node.module else {a.name for a in node.names}
    names = [node.module or ""] if isinstance(node, ast.ImportFrom) else [a.name for a in node.names]
    return {n.split(".")[1] for n in names if n.startswith("legged_tracking_amd.")}


@pytest.mark.parametrize("name", ACYCLIC)
def test_no_import_below_module_level(name):
    with open(os.path.join(PKG, name + ".py")) as f:
        tree = ast.parse(f.read())
    top = {id(n) for n in tree.body}
    late = set()
    for node in ast.walk(tree):
        if isinstance(node, (ast.Import, ast.ImportFrom)) and id(node) not in top:
            late |= _package_imports(node) & SIBLINGS
    assert late <= ALLOWED_LATE, (name, late)
    if name == "rollout_lib":  # the leaf
        used = set().union(*(_package_imports(n) for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))))
        assert used == {"learn_abi", "native"}
    if name in ("rollout", "rollout_cnn"):  # a docstring and imports, nothing else
        assert all(isinstance(n, (ast.Import, ast.ImportFrom)) for n in tree.body[1:]) and ast.get_docstring(tree)


@pytest.mark.parametrize("name", CONCERNS)
def test_concern_module_imports_alone(name):
    r = subprocess.run([sys.executable, "-c", f"import legged_tracking_amd.{name}"], cwd=REPO, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr


def test_api_modules_hold_the_recorded_names():
    for mod, key in ((R, "rollout"), (RC, "rollout_cnn")):
        missing = [n for n in RECORDED[key] if not hasattr(mod, n)]
        assert not missing, (key, missing)
    assert RC.PPO is R.PPO and RC.RolloutStorage is R.RolloutStorage
    assert RC.PPO_Args is R.PPO_Args and RC.RunnerArgs is R.RunnerArgs
    assert RC._mlp is R._mlp and RC._mlp_train is R._mlp_train and RC.get_activation is R.get_activation
    from legged_tracking_amd import policy_kernels as PK, ppo as P, rollout_lib as RL
    assert RC.FUSED_DEFAULT is PK.FUSED_DEFAULT and RC.ENGINE_DEFAULT is P.ENGINE_DEFAULT
    assert R.lib is RL.lib and R.LIB_PATH is RL.LIB_PATH and R._colsum is RL._colsum
    assert R._pack_linear is PK._pack_linear and RC._pack_conv is PK._pack_conv
    assert issubclass(RC.ActorCritic, R.ActorCritic) and issubclass(RC.AC_Args, R.AC_Args)
    for cls in (RC.ActorCritic, RC.AC_Args, RC.Runner):  # public under the name they had: pickled by it
        assert cls.__module__ == RC.__name__ and pickle.loads(pickle.dumps(cls)) is cls
    for cls in (R.ActorCritic, R.AC_Args, R.Runner, R.PPO, R.RolloutStorage):
        assert pickle.loads(pickle.dumps(cls)) is cls


def _modules():
    """The three modules of the fixture, in its order, each built at the generator's current state."""
    mlp = type("A", (RC.AC_Args,), dict(use_cnn=False, height_map_shape=(2, 21, 11)))
    cnn = type("A", (RC.AC_Args,), dict(use_cnn=True, height_map_shape=(2, 61, 31)))
    return (("plain", lambda: R.ActorCritic(70, 2, 261, 12), None, 261),
            ("mlp", lambda: RC.ActorCritic(503, 2, 503, 12, ac_args=mlp), mlp, 2 * 41 + 256),
            ("cnn", lambda: RC.ActorCritic(41 + 3782, 2, 41 + 3782, 12, ac_args=cnn), cnn, 2 * 41 + 256))


def test_parameter_order_is_the_recorded_one():
    for key, make, _, _ in _modules():
        got = [[k, list(v.shape)] for k, v in make().named_parameters()]
        assert got == RECORDED["parameters"][key], key
        assert list(make().state_dict()) == [k for k, _ in got], key


def test_layers_draw_their_weights_in_the_documented_order():
    """height_map_encoder (the encoder module), adaptation_module, actor_body, critic_body, std."""
    for key, make, args, p in _modules():
        torch.manual_seed(0)
        ac = make()
        after = torch.get_rng_state()
        torch.manual_seed(0)
        A, act = args or R.AC_Args, AC.get_activation("elu")
        want = {}
        if args is not None:
            enc = AC.HeightMapEncoder(A.height_map_shape, A.cnn_num_embedding, use_cnn=A.use_cnn, activation="elu")
            want.update({f"height_map_encoder.{k}": v for k, v in enc.state_dict().items()})
        for name, sizes in (("adaptation_module", [p, *A.adaptation_module_branch_hidden_dims, 2]),
                            ("actor_body", [2 + p, *A.actor_hidden_dims, 12]),
                            ("critic_body", [2 + p, *A.critic_hidden_dims, 1])):
            want.update({f"{name}.{k}": v for k, v in AC._mlp(sizes, act).state_dict().items()})
        want["std"] = A.init_noise_std * torch.ones(12)
        assert torch.equal(torch.get_rng_state(), after), key
        got = ac.state_dict()
        assert sorted(got) == sorted(want), key
        for k, v in got.items():
            assert torch.equal(v, want[k]), (key, k)


def test_the_plain_module_passes_its_history_through():
    ac = R.ActorCritic(70, 2, 261, 12)
    h = torch.randn(4, 261)
    assert ac.process_obs_history(h) is h and ac.process_obs_history_train(h) is h
