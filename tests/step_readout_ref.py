"""What tests/test_step_readout_host.py (CPU) and tests/test_gpu_step_readout.py (MI355X) share: ONE substep of the step from the synthetic
states of contact_solve_ref's scenes, held to the numpy references.

The env of both sides: walk, ik signal, action_repeat 1, control time step 0.001 s, 60 sweeps, no latency, auto-reset off, no episode
limit -- one step() is one physics substep with the sweep cap of the readout tests, under the torque the motor model draws from the
step's own motor command.  The scenes are the six mark-base scenes of dynamics_ref.SCENES with dynamics_ref.scene_scales and the friction
of contact_solve_ref.scene_params; the actions are seeded and inside the walk env's box.

    v_next      contact_solve_ref.reference(S0, ..., tau)["v_next"] with tau = the motor model on (cmd, q0, qd0, qd0)   <-> velocity words of S1
    integrator  kinematics_ref.advance(S0 with S1's velocities, dt)                                                   <-> pos, quat, q of S1
"""
import numpy as np

import contact_solve_ref as cr
import dynamics_ref as dr
import kinematics_ref as kr
import orclib

SCENES = [(n, ground) for _, n, ground in dr.SCENES]
THRESHOLDS = (0.0, cr.THRESHOLD)
STEP_KW = dict(action_repeat=1, control_time_step=cr.DT, solver_iterations=cr.ITERATIONS)      # on top of test_gpu_kinematics.make_env's keywords
ENV_KW = dict(task="walk", signal_type="ik", seed=5, **STEP_KW)
VEL_WORDS = list(range(7, 13)) + list(range(25, 37))        # REX_S_LINVEL, REX_S_ANGVEL, REX_S_QD: the order of v
ACTION_BOUND = 0.4                                          # the walk env's box (ik signal)
ALL_MOTORS = (1 << 12) - 1


def actions(n, seed=77):
    """[n, 2] float32, inside the box"""
    return np.random.RandomState(seed + n).uniform(-ACTION_BOUND, ACTION_BOUND, (n, 2)).astype(np.float32)


def threshold32(thr):
    """the residual threshold as RexConfig carries it (a float32), widened"""
    return float(np.float32(thr))


def body_params(n):
    """[3, n] float32: the scene's base and leg mass scales and foot friction"""
    bs, ls = dr.scene_scales(n)
    return np.stack([bs, ls, cr.scene_params(n)[1]]).astype(np.float32)


def oracle_env(n, ground, thr, dtype=np.float64, params=True):
    """An OracleEnv of the scene after reset(): the config of ENV_KW, the scene's terrain and (params=True) body parameters"""
    cfg = orclib.default_config("walk", "ik", n, seed=ENV_KW["seed"], action_repeat=1, solver_iterations=cr.ITERATIONS, sim_time_step=cr.DT,
                                solver_residual_threshold=thr)
    if ground == "custom":
        cfg.init_height = 0.6
    orc = orclib.OracleEnv(cfg, dtype)
    if ground == "random":
        from rex_gym_amd.terrain import random_terrain_pool
        orc.set_terrain(*random_terrain_pool(kr.POOL))
    elif ground == "custom":
        fields = kr.custom_fields()
        orc.set_heightfield(fields, kr.custom_mids(fields), kr.CUSTOM_CELL, kr.CUSTOM_ORIGIN[:2])
    if params:
        orc.set_body_params(body_params(n))
    orc.reset()
    return orc


def oracle_substep(orc, S, keep, action):
    """Writes the columns keep.. of S (words 0 .. 36 and the episode word; float64, the quaternion as given) over the oracle's state, takes
    one step.  -> (the state before [54, n], after [54, n], the motor command [n, 12], done [n])"""
    ew = kr.episode_word(False)
    st = orc.get_state()
    st[0:37, keep:] = S[0:37, keep:]
    st[ew, keep:] = np.asarray(S[ew, keep:], np.float32).view(np.int32)
    orc.set_state(st)
    before = orc.get_state()
    _, _, done, cmd = orc.step(action)
    return before, orc.get_state(), np.asarray(cmd, np.float64), done


def real_family(n, ground, count):
    """The family of the GPU test's leading `real` columns, made on the CPU: a float32 OracleEnv of the scene with unit body parameters,
    reset, 8 steps with test_gpu_render._steps' actions (seed 2) -- the robot stands on all eight toe points, the solve of its redundant
    contact rows is not converged after 60 sweeps -- then one step with actions(n).
    -> (state float32 [37, count], episode [count], the motor command of that step [count, 12])"""
    orc = oracle_env(n, ground, 0.0, np.float32, params=False)
    rng = np.random.RandomState(2)
    for _ in range(8):
        orc.step(rng.uniform(-ACTION_BOUND, ACTION_BOUND, (n, 2)).astype(np.float32))
    st = orc.get_state()
    cmd = np.asarray(orc.step(actions(n))[3], np.float64)
    orc.close()
    return st[0:37, :count].astype(np.float32), st[orclib.S_EPISODE, :count].astype(np.int64), cmd[:count]


def motor_tau(cmd, state, g, kp=1.0, kd=0.02, q_obs=None, qd_obs=None, observed=False):
    """The torque the substep applies to env g (float64): the motor model on (cmd, q, qd, qd) -- with no latency the PD loop sees the
    substep's own joint angles and rates (csrc/rex_kernels.h rex_substep) -- for enabled motors.  q_obs, qd_obs [12]: what the PD loop
    sees under the latency model (the true rate stays the state's); observed: the torque the sensor reports instead (motor.py:127-129)"""
    s = np.asarray(state[:, g], np.float64)
    q = s[13:25] if q_obs is None else np.asarray(q_obs, np.float64)
    qd = s[25:37] if qd_obs is None else np.asarray(qd_obs, np.float64)
    return _motor().motor_torque(cmd, q, qd, s[25:37], kp, kd)[1 if observed else 0]


def motor_tau_params(cmd, state, g, voltage, damping, kp, kd, strength, q_obs=None, qd_obs=None, observed=False):
    """motor_tau for an actuator with its own parameters (float64; strength [12]): the motor model of the reference's model/motor.py as
    include/rexsim.h states it for rex_motor_torque_params -- pwm = clip(kp (cmd - q) - kd qd, +-1), net voltage clip(pwm V - (Kt + damping)
    qd, +-50), current = that / R, torque = strength x sign x interp(|current|, the table) -- R 0.186 ohm, Kt 0.0954; the observed
    torque clip(Kt pwm V / R, +-5.7) carries no strength ratio (motor.py:127-129)"""
    s = np.asarray(state[:, g], np.float64)
    q = s[13:25] if q_obs is None else q_obs
    qd = s[25:37] if qd_obs is None else qd_obs
    return motor_model(cmd, q, qd, s[25:37], voltage, damping, kp, kd, strength)[1 if observed else 0]


def motor_model(cmd, q, qd, qd_true, voltage=32.0, damping=0.0, kp=1.0, kd=0.02, strength=1.0):
    """-> (actual, observed) torque, float64, elementwise over arrays of any one shape: motor_tau_params' model on the angles and rates
    the PD loop sees (q, qd) and the true rates (qd_true)"""
    cmd, q, qd, qd_true = (np.asarray(x, np.float64) for x in (cmd, q, qd, qd_true))
    pwm = np.clip(-1.0 * kp * (q - cmd) - kd * qd, -1.0, 1.0)
    observed = np.clip(0.0954 * (pwm * voltage / 0.186), -5.7, 5.7)
    cur = np.clip(pwm * voltage - (0.0954 + damping) * qd_true, -50.0, 50.0) / 0.186
    actual = np.asarray(strength, np.float64) * np.sign(cur) * np.interp(np.abs(cur), [0, 10, 20, 30, 40, 50, 60], [0, 1, 1.9, 2.45, 3.0, 3.25, 3.5])
    return actual, observed


def motor_params(n, seed=91):
    """heterogeneous actuators of a scene: dict(voltage [n], damping [n], kp [n], kd [n], strength [12, n]) float32"""
    rng = np.random.RandomState(seed + n)
    f = np.float32
    return dict(voltage=rng.uniform(24.0, 34.0, n).astype(f), damping=rng.uniform(0.0, 0.05, n).astype(f), kp=rng.uniform(0.7, 1.3, n).astype(f),
                kd=rng.uniform(0.01, 0.04, n).astype(f), strength=rng.uniform(0.7, 1.2, (12, n)).astype(f))


_MOTOR = []


def _motor():
    if not _MOTOR:
        _MOTOR.append(orclib.Oracle(np.float64))
    return _MOTOR[0]


def vel_error(got, want):
    """largest component of the difference of two velocity vectors [18], relative to max(1, largest |component| of `want`)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def advanced(before, after, g, dt=cr.DT):
    """kinematics_ref.advance of env g's pre-step state along its post-step velocities (symplectic Euler), the quaternion normalised:
    -> (pos [3], quat [4], q [12]) float64"""
    A = np.array(before[0:37], np.float64)
    A[VEL_WORDS, g] = np.asarray(after, np.float64)[VEL_WORDS, g]
    s = kr.advance(A, g, False, dt)
    return s[0:3], s[3:7] / np.linalg.norm(s[3:7]), s[13:25]


def integrator_errors(before, after, g, dt=cr.DT):
    """-> (pos, quat, q): largest absolute component of env g's post-step words from advanced(); the quaternion up to its sign"""
    pos, quat, q = advanced(before, after, g, dt)
    a = np.asarray(after, np.float64)[:, g]
    dq = min(np.abs(a[3:7] - quat).max(), np.abs(a[3:7] + quat).max())
    return float(np.abs(a[0:3] - pos).max()), float(dq), float(np.abs(a[13:25] - q).max())


def kept(state, g, field, ref, motor_en, toe_dist_bound, position_shift):
    """whether env g enters the comparison of a step with the reference: contact_solve_ref.compared, no component of the reference's
    v_next at the +-100 clamp (a clamped component carries no information about the solve), every motor enabled (a disabled one draws no
    torque: another problem than the one tau states)"""
    if int(motor_en) != ALL_MOTORS or np.any(np.abs(ref["v_next"]) >= cr.MAX_VEL):
        return False
    return cr.compared(state, g, field, ref, toe_dist_bound, position_shift)
