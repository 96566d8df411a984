"""The bits of the readout queries' outputs: dynamics, dynamics_solve, forward_dynamics, push, contact_solve, contact_space and
inverse_dynamics over two small batches -- 130 envs on the plane and 67 on the random-terrain pool (130 = 4 * 32 + 2 and 67 = 2 * 32 + 3:
the last workgroup of 32 rows repeats its last row), after 8 steps with fixed seeds and per-env mass and friction scales -- once over
every env and once over 37 distinct envs in shuffled order, and the sha256 of every output tensor written to one JSON file.  Two builds of
the library compute the same thing exactly when their files are equal:

    REX_LIB_PATH=<one build> python tools/readout_bits.py a.json;  REX_LIB_PATH=<another> python tools/readout_bits.py b.json;  cmp a.json b.json

(one process per build: a process loads the library once).  Every kernel sum runs in a fixed order, so a build's file does not change from run
to run."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUNDS = (("plane", 130, {}), ("random_terrain", 67, dict(terrain_type="random", terrain_pool=8)))
STEPS, PICKED, SWEEPS = 8, 37, 60


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make_env(n, kw):
    """the batch after STEPS steps; the same call gives the same state"""
    import torch
    from rex_gym_amd import RexBatchEnv
    rng = np.random.RandomState(n)
    env = RexBatchEnv(n, task="walk", signal_type="ik", seed=3, auto_reset=True, check_actions=False, **kw)
    env.set_body_params(base_mass_scale=rng.uniform(0.8, 1.2, n).astype(np.float32), leg_mass_scale=rng.uniform(0.8, 1.2, n).astype(np.float32),
                        foot_friction=rng.uniform(0.3, 0.9, n).astype(np.float32))
    env.reset()
    for _ in range(STEPS):
        env.step(torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device))
    return env


def queries(env, ids, rec):
    """every read-only query over the rows `ids` (None: every env) -> rec[name] = digest"""
    import torch
    from rex_gym_amd import contact, contact_space, dynamics
    k = env.num_envs if ids is None else len(ids)
    rng = np.random.RandomState(1000 + k)

    def dev(*shape, scale=1.0):
        return torch.as_tensor((scale * rng.standard_normal(shape)).astype(np.float32), device=env.device)

    def put(name, result, fields):
        rec.update({"%s.%s" % (name, f): digest(getattr(result, f)) for f in fields})

    tau, toe, wrench, vdot = dev(k, 12, scale=3.0), dev(k, 4, 2, 3, scale=20.0), dev(k, 6, scale=10.0), dev(k, 18, scale=5.0)
    put("dynamics", env.dynamics(env_ids=ids), dynamics.FIELDS)
    for f in dynamics.FIELDS:                                      # mass_matrix and toe_jacobian are staged in LDS: other barrier paths
        put("dynamics[%s]" % f, env.dynamics(env_ids=ids, fields=(f,)), (f,))
    for K in (1, 6):
        rhs = dev(k, K, 18, scale=4.0)
        rec["dynamics_solve.K%d" % K] = digest(env.dynamics_solve(rhs, env_ids=ids))
        env.dynamics_solve(rhs, env_ids=ids, out=rhs)
        rec["dynamics_solve.K%d.in_place" % K] = digest(rhs)
    for name, kw in (("tau", dict(tau=tau)), ("toe", dict(toe_forces=toe)), ("wrench", dict(base_wrench=wrench)),
                     ("all", dict(tau=tau, toe_forces=toe, base_wrench=wrench))):
        rec["forward_dynamics.%s" % name] = digest(env.forward_dynamics(env_ids=ids, **kw))
    for name, kw in (("damped_60", dict(iterations=SWEEPS, residual_threshold=0.0)), ("undamped_60", dict(iterations=SWEEPS, residual_threshold=0.0, damping=False)),
                     ("damped_exit", dict(iterations=SWEEPS))):            # the config's threshold: the envs leave the loop at different sweeps
        put("contact_solve.%s" % name, env.contact_solve(tau=tau, env_ids=ids, **kw), contact.FIELDS)
    put("contact_space", env.contact_space(tau=tau, base_wrench=wrench, env_ids=ids), contact_space.FIELDS)
    for f in contact_space.FIELDS:                                 # each alone: the early returns
        put("contact_space[%s]" % f, env.contact_space(tau=tau, base_wrench=wrench, env_ids=ids, fields=(f,)), (f,))
    for name, kw in (("h", {}), ("vdot", dict(vdot=vdot)), ("toe", dict(toe_forces=toe)), ("vdot_all", dict(vdot=vdot, tau=tau, toe_forces=toe, base_wrench=wrench))):
        rec["inverse_dynamics.%s" % name] = digest(env.inverse_dynamics(env_ids=ids, **kw))


def push(env, ids, rec):
    import torch
    k = env.num_envs if ids is None else len(ids)
    rng = np.random.RandomState(2000 + k)
    imp = {name: torch.as_tensor((s * rng.standard_normal((k,) + shape)).astype(np.float32), device=env.device)
           for name, shape, s in (("base_impulse", (6,), 2.0), ("toe_impulses", (4, 2, 3), 0.5), ("joint_impulses", (12,), 0.1))}
    rec["push.dv"] = digest(env.push(env_ids=ids, **imp))
    rec["push.state"] = digest(env.state)


def main(out_path):
    out = {}
    for ground, n, kw in GROUNDS:
        picked = [int(i) for i in np.random.RandomState(7).permutation(n)[:PICKED]]
        for rows, ids in (("all", None), ("picked", picked)):
            rec = out["%s/%s" % (ground, rows)] = {}
            env = make_env(n, kw)
            rec["state"] = digest(env.state)
            queries(env, ids, rec)
            env.close()
            env = make_env(n, kw)                                  # a fresh env: the push writes to the state
            push(env, ids, rec)
            env.close()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("%d runs, %d tensors -> %s" % (len(out), sum(len(r) for r in out.values()), out_path))


if __name__ == "__main__":
    main(sys.argv[1])
