#!/usr/bin/env python3
"""Golden rollouts and torques of the reference's ACTUATOR knobs (MotorModel.set_strength_ratios / set_voltage /
set_viscous_damping, model/motor.py:40-74, and the PD gains of Rex.ApplyAction, rex.py:568-600).

The harness is make_rollout_golden.py's, imported as it is: the reference's unmodified env / Rex / MotorModel classes over the
oracle's rigid-body substep.  A randomizer object (tests/motor_randomizer.py) goes in through the reference's own
`env_randomizer=` keyword and turns the knobs in `randomize_env`.  The motor model survives the reference's soft reset, so the
nominal values are restored before every env.reset(): the reset motion is then the nominal robot's -- this project's documented
deviation, the same as for the masses.

Families (60 control steps, one episode, one action tape per family): walk_ik, gallop_ol, walk_ik_arm; each holds the nominal
scenario and the variations of VARIATIONS below.  Every non-nominal scenario must separate from its family's nominal run by at
least 1e-2 rad in some joint angle inside the window (asserted here, stored as `separation`): a fixture that could pass without
the feature is not written.  A controller block follows: MotorModel.convert_to_torque with the setters applied, for random
(cmd, q, qd, qd_true, kp, kd, voltage, damping, strength).

Run in the build container:  PYTHONPATH=/root/reference python tests/golden/make_motor_golden.py
Writes tests/golden/motor_rollout_golden.npz (arrays; the scenario table is the JSON string `meta`).
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_rollout_golden as mrg                                  # noqa: E402  (its main() is guarded)
from motor_randomizer import MotorRandomizer                       # noqa: E402  (tests/ is on the path through mrg)
from rex_gym.model import motor                                    # noqa: E402

STEPS = 60
MIN_SEPARATION = 1e-2
V0 = motor.MOTOR_VOLTAGE


def per_motor(nm, seed=5):
    return np.random.RandomState(seed).uniform(0.6, 1.2, nm).round(4).tolist()


def variations(nm, family):
    v = [("nominal", {})]
    v.append(("strength_0.7", dict(strength=[0.7] * nm)))
    v.append(("strength_per_motor", dict(strength=per_motor(nm))))
    v.append(("voltage_0.8", dict(voltage=0.8 * V0)))
    if family == "gallop_ol":          # (too weak on walk-IK for the replay tolerances: 7e-3 rad)
        v.append(("damping_0.1", dict(damping=0.1)))
    v.append(("gains", dict(kp=0.7, kd=0.03)))
    v.append(("all", dict(strength=per_motor(nm), voltage=0.85 * V0, damping=0.008, kp=1.2, kd=0.015)))
    return v


FAMILIES = [
    # name, env class, constructor kwargs, seed of the action tape
    ("walk_ik", mrg.walk_env.RexWalkEnv, dict(target_position=1.0, backwards=False, signal_type="ik"), 311),
    ("gallop_ol", mrg.gallop_env.RexReactiveEnv, dict(target_position=2.0, signal_type="ol"), 312),
    ("walk_ik_arm", mrg.walk_env.RexWalkEnv, dict(target_position=1.0, backwards=False, signal_type="ik", mark="arm"), 313),
]


def run(cls, kwargs, params, seed):
    mrg.gp.time.time = mrg.planner_clock
    random.seed(seed)
    rnd = MotorRandomizer(**params)
    env, inner = mrg.build_env(cls, dict(kwargs, env_randomizer=rnd))
    rex = inner.rex
    nm = rex.num_motors
    # the constructor's reset has already run the randomizer: back to the nominal motor before the recorded reset
    rex._motor_model.set_strength_ratios([1.0] * nm); rex._motor_model.set_voltage(V0)
    rex._motor_model.set_viscous_damping(motor.MOTOR_VISCOUS_DAMPING); rex._kp, rex._kd = 1.0, 0.02
    rng = np.random.RandomState(seed)
    lo, hi = mrg.action_space(inner)
    client = inner._pybullet_client
    obs = env.reset()                  # nominal reset motion, then randomize_env (rex_gym_env.py:341-346)
    mrg.restart_phase(inner)
    in_effect = dict(strength=np.asarray(rex._motor_model._strength_ratios, float).tolist(), voltage=float(rex._motor_model.get_voltage()),
                     damping=float(rex._motor_model.get_viscous_dampling()), kp=float(rex._kp), kd=float(rex._kd))
    rec = dict(reset_obs=np.asarray(obs, float), reset_body=np.asarray(client.st, float), action=[], obs=[], reward=[], done=[], cmd=[], body=[])
    for _ in range(STEPS):
        a = rng.uniform(lo, hi)
        obs, reward, done, info = env.step(a)
        assert not done, "the scenarios run their 60 steps without a done"
        rec["action"].append(a); rec["obs"].append(np.asarray(obs, float)); rec["reward"].append(float(reward))
        rec["done"].append(bool(done)); rec["cmd"].append(np.asarray(info["action"], float)); rec["body"].append(np.asarray(client.st, float))
    return {k: np.asarray(v) for k, v in rec.items()}, in_effect


def controller_block(n=1000, seed=9):
    """MotorModel.convert_to_torque with the setters applied, one model per problem."""
    rng = np.random.RandomState(seed)
    cmd, q = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n)
    near = rng.rand(n) < 0.5                               # half of the problems inside the unsaturated band of the PD loop
    q[near] = cmd[near] + rng.uniform(-0.6, 0.6, near.sum())
    qd, qd_true = rng.uniform(-20, 20, n), rng.uniform(-20, 20, n)
    par = np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(0.0, 0.05, n), rng.uniform(20.0, 36.0, n), rng.uniform(0.0, 0.1, n),
                    rng.uniform(0.5, 1.3, n)], axis=1)      # kp, kd, voltage, damping, strength
    actual, observed = np.zeros(n), np.zeros(n)
    for i in range(n):
        m = motor.MotorModel(motors_num=1, kp=par[i, 0], kd=par[i, 1])
        m.set_voltage(par[i, 2]); m.set_viscous_damping(par[i, 3]); m.set_strength_ratios([par[i, 4]])
        a, o = m.convert_to_torque(np.array([cmd[i]]), np.array([q[i]]), np.array([qd[i]]), np.array([qd_true[i]]),
                                   np.array([par[i, 0]]), np.array([par[i, 1]]))
        actual[i], observed[i] = a[0], o[0]
    return dict(ctl_cmd=cmd, ctl_q=q, ctl_qd=qd, ctl_qd_true=qd_true, ctl_par=par, ctl_actual=actual, ctl_observed=observed)


def main():
    arrays, meta = {}, dict(description=__doc__.split("\n\n")[0], steps=STEPS, min_separation=MIN_SEPARATION, families=[])
    for fname, cls, kwargs, seed in FAMILIES:
        nm = 18 if kwargs.get("mark") == "arm" else 12
        vs = variations(nm, fname)
        if fname == "walk_ik_arm":     # nominal + the all-at-once variation with a stronger damping
            vs = [vs[0], ("all", dict(vs[-1][1], damping=0.05))]
        fam = dict(name=fname, env_class=cls.__name__, env_kwargs=kwargs, num_motors=nm, scenarios=[])
        nominal = None
        for vname, params in vs:
            rec, in_effect = run(cls, kwargs, params, seed)
            q = rec["body"][:, 13:13 + nm]
            if nominal is None:
                nominal, sep = q, 0.0
                assert np.array_equal(in_effect["strength"], [1.0] * nm) and in_effect["voltage"] == V0 and in_effect["damping"] == 0.0
            else:
                sep = float(np.abs(q - nominal).max())
                assert sep >= MIN_SEPARATION, (fname, vname, sep)
            key = f"{fname}/{vname}"
            for k, v in rec.items():
                arrays[f"{key}/{k}"] = v
            fam["scenarios"].append(dict(name=vname, key=key, nominal=vname == "nominal", separation=sep, params=in_effect))
            print(f"{key}: separation from nominal {sep:.3e} rad")
        meta["families"].append(fam)
    arrays.update(controller_block())
    path = os.path.join(HERE, "motor_rollout_golden.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
