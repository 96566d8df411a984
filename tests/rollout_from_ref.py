"""The float64 reference of rex_rollout_from, composed of parts that exist (tests/test_rollout_from_host.py on the CPU,
tests/test_gpu_rollout_from.py on the MI355X): rollout_ref.transition with

    body      the row's (base mass scale, leg mass scale, toe friction) in place of the env's `scales` and `mu`
    wrench    a world force at the base origin and a world moment, rows 0..5 of the equation of motion (rex_forward_dynamics'
              base_wrench), held over the control step's substeps.  It enters the free velocity, v* = v + dt M^-1 (S^T tau + w - h - d):
              contact_solve_ref.reference forms b = S^T tau - bias, so it is handed dynamics_ref.reference's result with `bias` reduced
              by (w, 0 .. 0) -- no solver code is restated
    init      the state the row starts from is the caller's: transition() and rollout() take the state as an argument already

The module also holds the cases of both test files (CASES: two of rollout_ref.CASES, one on the plane and one on the random pool), the
draws of the per-row inputs (draws) and the walk that measures the float32 floor (walk: rollout_ref.walk with the wrench and the
overrides)."""
import numpy as np

import contact_solve_ref as cr
import dynamics_ref as dr
import kinematics_ref as kr
import rollout_ref as rr
import step_readout_ref as sr

WORDS = rr.WORDS
CASES = [c for c in rr.CASES if c in ((5, "plane", 3, 4), (67, "random", 2, 3))]
CASE_IDS = ["%d-%s-K%d-T%d" % c for c in CASES]
assert len(CASES) == 2
G = dr.G                                           # 10 m/s^2 in this sim
# the draws: force uniform within +-FORCE x the nominal robot's weight per axis, moment within +-that x ARM, mass scales and friction
FORCE, ARM, SCALE_RANGE, MU_RANGE = 0.5, 0.1, (0.8, 1.2), (0.3, 1.0)


def nominal_weight():
    """mass x g of the robot with unit scales, N"""
    return float(sum(dr.MASS[:13])) * G


def draws(n, K, T, seed=321):
    """-> (wrench [n, K, T, 6] float32, body [n, K, 3] float32) of a case: one draw per row and control step"""
    rng = np.random.RandomState(seed + 1000 * K + 10 * T + n)
    f = FORCE * nominal_weight()
    w = rng.uniform(-1.0, 1.0, (n, K, T, 6)) * np.array([f, f, f, f * ARM, f * ARM, f * ARM])
    body = np.stack([rng.uniform(*SCALE_RANGE, (n, K)), rng.uniform(*SCALE_RANGE, (n, K)), rng.uniform(*MU_RANGE, (n, K))], -1)
    return w.astype(np.float32), body.astype(np.float32)


def transition(s, command, wrench=None, body=None, field=None, scales=(1.0, 1.0), mu=0.5, mode="targets", motor=None, motor_en=sr.ALL_MOTORS, dt=rr.DT,
               iterations=cr.ITERATIONS, residual_threshold=0.0, dtype=np.float64, tau=None):
    """rollout_ref.transition from state s [37] under the row's body [3] (None: scales, mu as given) and wrench [6] (None: none, and the
    call IS rollout_ref.transition).  -> its dict"""
    if body is not None:
        scales, mu = (body[0], body[1]), float(body[2])
    if wrench is None:
        return rr.transition(s, command, field, scales, mu, mode, motor, motor_en, dt, iterations, residual_threshold, dtype, tau)
    col = np.asarray(s).reshape(WORDS, 1)
    tau = rr.torque(command, col[:, 0], mode, motor, motor_en) if tau is None else np.asarray(tau, np.float64)
    d = dict(dr.reference(col, 0, field, scales, dtype))
    bias = np.array(d["bias"], dtype)
    bias[0:6] = (bias[0:6] - np.asarray(wrench, dtype)).astype(dtype)
    d["bias"] = bias
    ref = cr.reference(col, 0, field, scales, mu, tau, dt=dt, iterations=iterations, residual_threshold=residual_threshold, dtype=dtype, dyn=d)
    A = np.array(col, np.float64)
    A[sr.VEL_WORDS, 0] = np.asarray(ref["v_next"], np.float64)
    nxt = kr.advance(A, 0, False, dt)
    nxt[3:7] /= np.linalg.norm(nxt[3:7])
    contact = (np.asarray(ref["toe_lambda"])[:, 0] > 0).reshape(4, 2).any(1)
    return dict(state=nxt, v_next=np.asarray(ref["v_next"]), foot_contact=contact, tau=tau, ref=ref)


def rollout(s0, commands, wrenches=None, body=None, repeat=1, round32=False, **kw):
    """rollout_ref.rollout from state s0 [37] under commands [T, 12], wrenches [T, 6] (None: none) and the row's body [3] (None: kw's)"""
    commands = np.asarray(commands)
    s = np.asarray(s0, np.float32 if round32 else np.float64)
    traj, contact, steps, sweeps = [], [], [], 0
    for t in range(len(commands)):
        for h in range(repeat):
            tr = transition(s, commands[t], None if wrenches is None else wrenches[t], body, **kw)
            steps.append((t, h, s, tr))
            sweeps += tr["ref"]["sweeps"]
            s = tr["state"].astype(np.float32) if round32 else tr["state"]
        traj.append(np.asarray(s, np.float64))
        contact.append(tr["foot_contact"])
    return dict(state=traj[-1], trajectory=np.array(traj), foot_contact=np.array(contact), sweeps=sweeps, transitions=steps)


def walk(n, ground, K, T, toe_dist_bound, position_shift, v_bound, repeat=1, envs=None):
    """rollout_ref.walk with the case's draws: per (env, candidate) the float64 reference's trajectory under the row's wrenches and body
    with each state rounded to float32, per transition the float32 evaluation of the same substep.
    -> list of dict(env, cand, t, h, kind, family, state, command, wrench, body, field, ref, tau, dev, kept)"""
    S, ep, kinds = rr.host_states(n, ground)
    fields, _ = rr.case_params(n, ground)
    cmds = rr.targets(S[13:25].T, K, T)
    wr, body = draws(n, K, T)
    out = []
    for g in (range(n) if envs is None else envs):
        fld = kr.field_of(fields, g, ep[g])
        for c in range(K):
            for t, h, s, tr in rollout(S[:, g], cmds[g, c], wr[g, c], body[g, c], repeat, round32=True, field=fld)["transitions"]:
                v32 = transition(s, cmds[g, c, t], wr[g, c, t], body[g, c], field=fld, dtype=np.float32)["v_next"]
                dev = sr.vel_error(v32, tr["v_next"])
                ok = rr.kept(s, fld, tr["ref"], toe_dist_bound, position_shift) and dev <= v_bound
                out.append(dict(env=g, cand=c, t=t, h=h, kind=kinds[g], family=rr.family(kinds[g]), state=s, command=cmds[g, c, t], wrench=wr[g, c, t],
                                body=body[g, c], field=fld, ref=tr["ref"], tau=tr["tau"], dev=dev, kept=bool(ok)))
    return out
