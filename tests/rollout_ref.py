"""The float64 reference of rex_rollout, composed of parts that exist (tests/test_rollout_host.py on the CPU, tests/test_gpu_rollout.py on
the MI355X):

    torque      step_readout_ref.motor_model on (command, q, qd, qd) of the state -- with an actuator's parameters where given -- times the
                motor enable bits; or the command itself (tau mode)
    v_next      contact_solve_ref.reference(state, ..., tau)["v_next"], damping on
    integrator  kinematics_ref.advance of the state with its velocity words replaced by v_next, the quaternion normalised

transition() is one substep from a given state (float32 as the kernel emits it, or float64) in float64 or float32 arithmetic; rollout() the
trajectory of one (env, candidate): T control steps of `repeat` substeps, the command of a control step held over its substeps and the torque
drawn anew in each.  No trajectory of the kernel is compared with a trajectory of the reference: round-off is amplified through contact
events.  Every transition the kernel emits is held to ONE substep of the reference from the kernel's own emitted state, at single-substep
bounds.

The module also holds the cases of both test files (CASES), their commands (targets) and the walk that measures the float32 floor
(walk): along the float64 reference's trajectory with each state rounded to float32, per transition the deviation of the float32
evaluation's v_next from the float64 one."""
import numpy as np

import contact_solve_ref as cr
import kinematics_ref as kr
import step_readout_ref as sr

WORDS = 37
DT = float(np.float32(cr.DT))                      # the time step the config carries: a float32
# (envs, ground, K, T): 15, 134, 134, 134 and 130 rows, none a multiple of the kernel's 32 rows per workgroup
CASES = [(5, "plane", 3, 4), (67, "plane", 2, 3), (67, "random", 2, 3), (67, "custom", 2, 3), (130, "plane", 1, 2)]
CASE_IDS = ["%d-%s-K%d-T%d" % c for c in CASES]
SPREAD = 0.3                                       # rad: the commands lie within +-SPREAD of the row's initial joint angles
FAMILIES = ("synthetic", "real")


def torque(command, s, mode="targets", motor=None, motor_en=sr.ALL_MOTORS, kp=1.0, kd=0.02):
    """the joint torque [12] of one substep, float64: the motor model on (command, q, qd, qd) of state s [37] -- motor: dict(voltage,
    damping, kp, kd, strength [12]) of the env, None: the nominal actuator with the config's gains -- times the enable bits; mode "tau":
    the command as given"""
    if mode == "tau":
        return np.asarray(command, np.float64)
    s = np.asarray(s, np.float64)
    q, qd = s[13:25], s[25:37]
    if motor is None:
        act = sr.motor_model(command, q, qd, qd, kp=kp, kd=kd)[0]
    else:
        act = sr.motor_model(command, q, qd, qd, float(motor["voltage"]), float(motor["damping"]), float(motor["kp"]), float(motor["kd"]),
                             np.asarray(motor["strength"], np.float64))[0]
    return act * np.array([(int(motor_en) >> j) & 1 for j in range(12)], np.float64)


def transition(s, command, field=None, scales=(1.0, 1.0), mu=0.5, mode="targets", motor=None, motor_en=sr.ALL_MOTORS, dt=DT, iterations=cr.ITERATIONS,
               residual_threshold=0.0, dtype=np.float64, tau=None):
    """One substep from state s [37] (its dtype is kept: float32 as emitted, or float64) in `dtype` arithmetic (the torque and the
    integrator always float64).  tau: the torque to apply instead of the one `command` draws (the wrong references of the teeth).
    -> dict(state [37] float64, v_next [18], foot_contact [4] bool, tau [12], ref: contact_solve_ref.reference's result)"""
    col = np.asarray(s).reshape(WORDS, 1)
    tau = torque(command, col[:, 0], mode, motor, motor_en) if tau is None else np.asarray(tau, np.float64)
    ref = cr.reference(col, 0, field, scales, mu, tau, dt=dt, iterations=iterations, residual_threshold=residual_threshold, dtype=dtype)
    A = np.array(col, np.float64)
    A[sr.VEL_WORDS, 0] = np.asarray(ref["v_next"], np.float64)
    nxt = kr.advance(A, 0, False, dt)
    nxt[3:7] /= np.linalg.norm(nxt[3:7])
    contact = (np.asarray(ref["toe_lambda"])[:, 0] > 0).reshape(4, 2).any(1)
    return dict(state=nxt, v_next=np.asarray(ref["v_next"]), foot_contact=contact, tau=tau, ref=ref)


def rollout(s0, commands, repeat=1, round32=False, **kw):
    """The trajectory of one (env, candidate) from state s0 [37] under commands [T, 12]; round32: every state rounded to float32 before
    the next substep (the walk of the floor; else float64 throughout).  kw: transition's.
    -> dict(state [37], trajectory [T, 37], foot_contact [T, 4] bool, sweeps, transitions: per substep (t, h, the state before, transition()))"""
    commands = np.asarray(commands)
    s = np.asarray(s0, np.float32 if round32 else np.float64)
    traj, contact, steps, sweeps = [], [], [], 0
    for t in range(len(commands)):
        for h in range(repeat):
            tr = transition(s, commands[t], **kw)
            steps.append((t, h, s, tr))
            sweeps += tr["ref"]["sweeps"]
            s = tr["state"].astype(np.float32) if round32 else tr["state"]
        traj.append(np.asarray(s, np.float64))
        contact.append(tr["foot_contact"])
    return dict(state=traj[-1], trajectory=np.array(traj), foot_contact=np.array(contact), sweeps=sweeps, transitions=steps)


def kept(s, field, ref, toe_dist_bound, position_shift):
    """the reference's own part of the kept rule: contact_solve_ref.compared on the state before, and no component of v_next at the clamp"""
    if np.any(np.abs(np.asarray(ref["v_next"], np.float64)) >= cr.MAX_VEL):
        return False
    return cr.compared(np.asarray(s).reshape(WORDS, 1), 0, field, ref, toe_dist_bound, position_shift)


# ---------------------------------------------------------------- the cases
def targets(q0, K, T, seed=123):
    """[n, K, T, 12] float32: the row's initial joint angles q0 [n, 12] + uniform(-SPREAD, SPREAD)"""
    q0 = np.asarray(q0, np.float32)
    n = q0.shape[0]
    u = np.random.RandomState(seed + 1000 * K + 10 * T + n).uniform(-SPREAD, SPREAD, (n, K, T, 12))
    return (q0[:, None, None, :].astype(np.float64) + u).astype(np.float32)


def case_params(n, ground, heights=None, mids=None):
    """-> (fields, body parameters [3, n]: base and leg mass scale, friction) of a case's scene"""
    return kr.scene_fields(ground, heights, mids), sr.body_params(n)


def host_states(n, ground):
    """The states of a case as the CPU has them: contact_solve_ref.scene_states with the leading real columns from
    step_readout_ref.real_family.  -> (S float32 [37, n], episode [n], kinds [n])"""
    S, kinds = cr.scene_states(n, ground)
    keep = kr.scene_keep(n)
    ep = S[kr.episode_word(False)].view(np.int32).astype(np.int64)
    S = S[0:WORDS].copy()
    real, rep, _ = sr.real_family(n, ground, keep)
    S[:, :keep], ep[:keep] = real, rep
    return S, ep, kinds


def family(kind):
    return "real" if kind == "real" else "synthetic"


def walk(n, ground, K, T, toe_dist_bound, position_shift, v_bound, repeat=1, envs=None):
    """The float32 floor's walk over a case (envs: a subset of its envs): per (env, candidate) the float64 reference's trajectory with each
    state rounded to float32, per transition the float32 evaluation of the same substep.
    -> list of dict(env, cand, t, h, kind, family, state, command, field, scales, mu, ref, dev: vel_error of the float32 v_next from the
    float64 one, kept: kept() and dev <= v_bound)"""
    S, ep, kinds = host_states(n, ground)
    fields, bp = case_params(n, ground)
    cmds = targets(S[13:25].T, K, T)
    out = []
    for g in (range(n) if envs is None else envs):
        fld = kr.field_of(fields, g, ep[g])
        kw = dict(field=fld, scales=(bp[0, g], bp[1, g]), mu=float(bp[2, g]))
        for c in range(K):
            for t, h, s, tr in rollout(S[:, g], cmds[g, c], repeat, round32=True, **kw)["transitions"]:
                v32 = transition(s, cmds[g, c, t], dtype=np.float32, **kw)["v_next"]
                dev = sr.vel_error(v32, tr["v_next"])
                ok = kept(s, fld, tr["ref"], toe_dist_bound, position_shift) and dev <= v_bound
                out.append(dict(env=g, cand=c, t=t, h=h, kind=kinds[g], family=family(kinds[g]), state=s, command=cmds[g, c, t], ref=tr["ref"],
                                tau=tr["tau"], dev=dev, kept=bool(ok), **kw))
    return out

