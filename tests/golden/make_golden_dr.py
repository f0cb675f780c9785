"""Fixture of the reference's after-start domain randomisation (container-only test infrastructure).

Imports the reference behind the offline stand-ins of tests/golden/refstubs, as make_golden_plan.py does, and calls its
own LeggedRobot._randomize_rigid_body_props (legged_robot_trajectory_tracking.py:710-732) and _push_robots
(:1074-1084) through its own _call_train_eval on a stub namespace that holds just what they read: cfg, device,
num_actor, num_train_envs, payloads, com_displacements, friction_coeffs, restitutions, root_states,
episode_length_buf and a gym whose set_actor_root_state_tensor does nothing.  refresh_actor_rigid_shape_props (the
hand-over to PhysX) is a no-op.  32 envs run for 12 consecutive steps per flag set; between steps this generator moves
the roots, increments episode_length_buf, restates the call sites (:819, :822-823 and :831-833, reset_idx :233-235 with
the root and episode-length reset) and the two privileged-observation lines (:482-487, :504-509, clipped as step
:107-108 does), and resets a few envs per step.

torch.rand is wrapped to record every draw.  Recorded per step are the planes a go1_dr_step launch sees after the env
step (root, friction, restitution, payloads, episode_length, reset, priv: everything as the step would leave it
WITHOUT the randomisation), the same planes after it, and the draws in the launch's slot order (`uniforms`
(steps, n, 8): an env that is due and resets in one step draws twice in the reference; the slot holds the reset's
draw, which is the one that survives).  A second block records a host reset_idx(env_ids) (:233-235) alone.

Usage: python tests/golden/make_golden_dr.py [reference root]   (writes tests/golden/dr_cases.npz)
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GO1_REFERENCE_ROOT", "")  # the reference checkout

sys.dont_write_bytecode = True  # the reference tree is read-only
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, os.path.join(HERE, "refstubs"))
sys.path.insert(1, REF)
sys.path.insert(2, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import dr_ref as DR  # noqa: E402

N, STEPS = 32, 12
RAND_INTERVAL, PUSH_INTERVAL = 4, 3
CLIP_OBS = 4.0  # small enough that the largest frictions clip
RANGES = dict(payload=(-1.0, 3.0), friction=(0.1, 3.0), restitution=(0.0, 0.4), push=0.5)
NORM = dict(friction=(0.0, 1.0), restitution=(0.0, 1.0))
SETS = {
    "all": dict(rigids_after_start=True, push_robots=True, payload=True, friction=True, restitution=True),
    "partial": dict(rigids_after_start=True, push_robots=False, payload=True, friction=False, restitution=True),
}


def coarse(rng, span, shape):
    """Multiples of 1 / 64 in +-span / 64 (exact in f32; the root planes stay small in the compressed fixture)."""
    return torch.from_numpy((rng.integers(-span, span + 1, shape) / 64.0).astype(np.float32))


def make_cfg(flags):
    dr = types.SimpleNamespace(
        randomize_rigids_after_start=flags["rigids_after_start"], push_robots=flags["push_robots"],
        randomize_base_mass=flags["payload"], added_mass_range=list(RANGES["payload"]),
        randomize_com_displacement=False, com_displacement_range=[-0.15, 0.15],
        randomize_friction=flags["friction"], friction_range=list(RANGES["friction"]),
        randomize_restitution=flags["restitution"], restitution_range=list(RANGES["restitution"]),
        rand_interval=RAND_INTERVAL, push_interval=np.ceil(PUSH_INTERVAL - 0.5), max_push_vel_xy=RANGES["push"])
    norm = types.SimpleNamespace(friction_range=list(NORM["friction"]), restitution_range=list(NORM["restitution"]),
                                 clip_observations=CLIP_OBS)
    return types.SimpleNamespace(domain_rand=dr, normalization=norm)


def run_set(name, flags, LR, get_scale_shift, seed):
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    ns = types.SimpleNamespace()
    ns.device, ns.num_actor, ns.num_envs, ns.num_train_envs, ns.num_dof = "cpu", 1, N, N, 12
    ns.cfg = make_cfg(flags)
    ns.eval_cfg = None
    ns.sim = None
    ns.gym = types.SimpleNamespace(set_actor_root_state_tensor=lambda sim, t: None)
    ns.payloads = torch.from_numpy(rng.uniform(*RANGES["payload"], N).astype(np.float32))
    ns.com_displacements = torch.zeros(N, 3)
    ns.friction_coeffs = torch.from_numpy(rng.uniform(*RANGES["friction"], (N, 1)).astype(np.float32))
    ns.restitutions = torch.from_numpy(rng.uniform(*RANGES["restitution"], (N, 1)).astype(np.float32))
    ns.root_states = coarse(rng, 256, (N, 13))
    ns.episode_length_buf = torch.from_numpy(rng.integers(0, 7, N)).long()
    ns._call_train_eval = types.MethodType(LR._call_train_eval, ns)
    ns._randomize_rigid_body_props = types.MethodType(LR._randomize_rigid_body_props, ns)
    ns._push_robots = types.MethodType(LR._push_robots, ns)
    ns.refresh_actor_rigid_shape_props = lambda env_ids, cfg: None
    payload_plane = ns.payloads.numpy().copy()  # the simulated mass: fixed at creation (:1593)

    draws = []
    real_rand = torch.rand

    def recording_rand(*a, **k):
        t = real_rand(*a, **k)
        draws.append(t.clone())
        return t

    def take():
        out = list(draws)
        draws.clear()
        return out

    def rigid_slots(u, ids, got):
        """The draws of one _randomize_rigid_body_props(ids) call, in its order, into the launch's slots."""
        got = list(got)
        for key, slot in (("payload", DR.U_PAYLOAD), ("friction", DR.U_FRICTION), ("restitution", DR.U_RESTITUTION)):
            if flags[key]:
                u[ids, slot] = got.pop(0).numpy().reshape(-1)
        assert not got

    def priv_lines():
        fs, fsh = get_scale_shift(ns.cfg.normalization.friction_range)
        rs, rsh = get_scale_shift(ns.cfg.normalization.restitution_range)
        p = torch.cat(((ns.friction_coeffs[:, 0].unsqueeze(1) - fsh) * fs,
                       (ns.restitutions[:, 0].unsqueeze(1) - rsh) * rs), dim=1)
        return torch.clip(p, -CLIP_OBS, CLIP_OBS).numpy().copy()

    keys = ("root", "friction", "restitution", "payloads", "priv")
    rec = {k: [] for k in ("episode_length", "reset", "uniforms", "rigids", "pushed", "twice", "payload_plane") +
           tuple(f"{k}_{w}" for k in keys for w in ("before", "after"))}
    torch.rand = recording_rand
    try:
        for step in range(STEPS):
            # the "physics": every root moves, episode lengths count (:126)
            ns.root_states = ns.root_states + coarse(rng, 8, (N, 13))
            ns.episode_length_buf += 1
            reset = np.zeros(N, bool)
            reset[rng.choice(N, 3, replace=False)] = True
            if step % 4 == 3:  # an env that is due by its interval and resets in the same step
                due = np.nonzero((ns.episode_length_buf.numpy() % RAND_INTERVAL) == 0)[0]
                if due.size:
                    reset[due[0]] = True
            if step % 4 == 1:  # an env that is pushed and resets in the same step: the reset's root survives
                due = np.nonzero((ns.episode_length_buf.numpy() % PUSH_INTERVAL) == 0)[0]
                if due.size:
                    reset[due[-1]] = True
            rid = torch.from_numpy(np.nonzero(reset)[0])
            reset_roots = coarse(rng, 256, (len(rid), 13))
            # what the step leaves without the randomisation: reset envs at their reset root with episode length 0
            before_root = ns.root_states.clone()
            before_root[rid] = reset_roots
            before = dict(root=before_root.numpy().copy(), friction=ns.friction_coeffs[:, 0].numpy().copy(),
                          restitution=ns.restitutions[:, 0].numpy().copy(), payloads=ns.payloads.numpy().copy(),
                          priv=priv_lines())
            u = np.zeros((N, DR.DR_U), np.float32)
            all_ids = torch.arange(N)
            # :819
            take()
            pushed = (ns.episode_length_buf % int(ns.cfg.domain_rand.push_interval) == 0).numpy() & flags["push_robots"]
            ns._call_train_eval(ns._push_robots, all_ids)
            got = take()
            if flags["push_robots"]:
                assert len(got) == 1 and got[0].shape == (int(pushed.sum()), 2)
                u[np.nonzero(pushed)[0], DR.U_PUSH_X:DR.U_PUSH_Y + 1] = got[0].numpy()
            else:
                assert not got
            # :822-823, :831-833
            env_ids = (ns.episode_length_buf % int(ns.cfg.domain_rand.rand_interval) == 0).nonzero(
                as_tuple=False).flatten()
            if ns.cfg.domain_rand.randomize_rigids_after_start:
                ns._call_train_eval(ns._randomize_rigid_body_props, env_ids)
                ns._call_train_eval(ns.refresh_actor_rigid_shape_props, env_ids)
            if len(env_ids):
                rigid_slots(u, env_ids.numpy(), take())
            interval_ids = set(env_ids.tolist())
            # reset_idx (:228-238): the redraw, then the root and the episode length of the reset
            if len(rid):
                if ns.cfg.domain_rand.randomize_rigids_after_start:
                    ns._call_train_eval(ns._randomize_rigid_body_props, rid)
                    ns._call_train_eval(ns.refresh_actor_rigid_shape_props, rid)
                rigid_slots(u, rid.numpy(), take())
                ns.root_states[rid] = reset_roots
                ns.episode_length_buf[rid] = 0
            rigids = np.zeros(N, bool)
            rigids[list(interval_ids | set(rid.tolist()))] = flags["rigids_after_start"]
            twice = np.zeros(N, bool)
            twice[list(interval_ids & set(rid.tolist()))] = True
            after = dict(root=ns.root_states.numpy().copy(), friction=ns.friction_coeffs[:, 0].numpy().copy(),
                         restitution=ns.restitutions[:, 0].numpy().copy(), payloads=ns.payloads.numpy().copy(),
                         priv=priv_lines())
            for k in keys:
                rec[f"{k}_before"].append(before[k])
                rec[f"{k}_after"].append(after[k])
            rec["episode_length"].append(ns.episode_length_buf.numpy().astype(np.int32))
            rec["reset"].append(reset)
            rec["uniforms"].append(u)
            rec["rigids"].append(rigids)
            rec["pushed"].append(pushed & ~reset)
            rec["twice"].append(twice)
            rec["payload_plane"].append(payload_plane.copy())
        # a host reset_idx(env_ids) alone (:233-235)
        ids = np.array([1, 7, 8, 30])
        hb = dict(friction=ns.friction_coeffs[:, 0].numpy().copy(), restitution=ns.restitutions[:, 0].numpy().copy(),
                  payloads=ns.payloads.numpy().copy())
        take()
        ns._call_train_eval(ns._randomize_rigid_body_props, torch.from_numpy(ids))
        hu = np.zeros((N, DR.DR_U), np.float32)
        rigid_slots(hu, ids, take())
        ha = dict(friction=ns.friction_coeffs[:, 0].numpy().copy(), restitution=ns.restitutions[:, 0].numpy().copy(),
                  payloads=ns.payloads.numpy().copy())
    finally:
        torch.rand = real_rand
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update({f"host_{k}_before": v for k, v in hb.items()})
    out.update({f"host_{k}_after": v for k, v in ha.items()})
    out.update(host_ids=ids.astype(np.int32), host_uniforms=hu)
    fs, fsh = get_scale_shift(NORM["friction"])
    rs, rsh = get_scale_shift(NORM["restitution"])
    out.update(rand_interval=np.int32(RAND_INTERVAL), push_interval=np.int32(int(ns.cfg.domain_rand.push_interval)),
               clip_obs=np.float32(CLIP_OBS), norm_friction=np.array(NORM["friction"], np.float64),
               norm_restitution=np.array(NORM["restitution"], np.float64),
               priv_consts=np.array([fsh, fs, rsh, rs], np.float64),
               range_payload=np.array(RANGES["payload"], np.float64),
               range_friction=np.array(RANGES["friction"], np.float64),
               range_restitution=np.array(RANGES["restitution"], np.float64), max_push=np.float64(RANGES["push"]),
               flags=np.array([flags[k] for k in ("rigids_after_start", "push_robots", "payload", "friction",
                                                  "restitution")], bool))
    print(f"{name}: rigids {int(out['rigids'].sum())}, pushed {int(out['pushed'].sum())}, resets "
          f"{int(out['reset'].sum())}, drawn twice {int(out['twice'].sum())}, priv clipped "
          f"{int((np.abs(out['priv_after']) == CLIP_OBS).sum())}")
    assert out["twice"].any() and out["rigids"].any() and (out["reset"] & ~out["twice"]).any()
    assert not flags["push_robots"] or out["pushed"].any()
    # a pushed env that also resets keeps the root of its reset
    assert not flags["push_robots"] or (out["reset"] & (out["uniforms"][..., DR.U_PUSH_X] != 0)).any()
    return out


def main():
    from go1_gym.envs.base.legged_robot_trajectory_tracking import LeggedRobot as LR
    from go1_gym.utils.math_utils import get_scale_shift
    out = {}
    for i, (name, flags) in enumerate(SETS.items()):
        for k, v in run_set(name, flags, LR, get_scale_shift, 4100 + i).items():
            out[f"{name}/{k}"] = v
    path = os.path.join(HERE, "dr_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
