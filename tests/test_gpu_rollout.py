"""Candidate rollouts on the GPU (rex_rollout, csrc/rex_rollout.hip; RexBatchEnv.rollout) against the float64 reference of
tests/rollout_ref.py -- step_readout_ref.motor_model, contact_solve_ref.reference and kinematics_ref.advance composed -- and against the
step kernels and rex_contact_solve on one state.

No trajectory is compared with a trajectory: round-off is amplified through contact events.  Every transition the kernel emits is held to ONE
substep of the reference evaluated in float64 from the kernel's own emitted float32 state, at single-substep bounds.

Envs: walk, ik, action_repeat 1, control time step 0.001 s, 60 sweeps, no latency (step_readout_ref.STEP_KW on top of
test_gpu_kinematics.make_env), contact_solve_ref's synthetic columns behind the leading real ones, the scene's mass scales and friction.
Cases (rollout_ref.CASES): 5 envs on the plane with K = 3, T = 4; 67 on the plane, the random pool and the custom field with K = 2, T = 3; 130
on the plane with K = 1, T = 2 -- 15, 134, 134, 134 and 130 rows, none a multiple of the kernel's 32 rows per workgroup.  Commands: the row's
initial joint angles + uniform(-0.3, 0.3) (rollout_ref.targets).

Bounds on the velocities, relative to max(1, largest |component| of the reference's v_next) (step_readout_ref.vel_error): FACTOR (4) x the
float32 floor of one transition, the project's margin for a float32 kernel with a different, equally valid order of operations.  The floor is
measured without a GPU (tests/test_rollout_host.py, which holds BOUNDS to it): along the float64 reference's trajectories of these cases with
each state rounded to float32, the deviation of the float32 evaluation's v_next from the float64 one, largest over the kept transitions, one
per family of columns:

    family      floor       bound
    synthetic   1.497e-04   5.988e-04     (67 envs on the custom field)
    real        2.173e-04   8.692e-04     (67 envs on the random pool)

A transition is kept when contact_solve_ref.compared holds on the state before it, no component of the reference's v_next is at the +-100
clamp, and float32 numpy itself reproduces the float64 v_next to test_gpu_contact_solve.BOUNDS["v_next"] (a transition that float32 numpy
cannot reproduce to the bound the single-substep readout is held to says nothing about a kernel); all three are the reference's alone.  At
least 90 % of every case are kept (asserted).  Positions, joint angles and the quaternion are held to the integrator tolerances of
tests/test_gpu_step_readout.py (c.), which are derived there for the same arithmetic."""
import numpy as np
import pytest

import contact_solve_ref as cr
import kinematics_ref as kr
import rollout_ref as rr
import step_readout_ref as sr
import test_gpu_contact_solve as tc
import test_gpu_kinematics as tk
import test_gpu_step_readout as tg

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOORS = {"synthetic": 1.497e-04, "real": 2.173e-04}
BOUNDS = {"synthetic": 5.988e-04, "real": 8.692e-04}
KW = dict(repeat=1, iterations=cr.ITERATIONS, residual_threshold=0.0)
FIELDS = ("state", "trajectory", "foot_contact", "sweeps")


def same(a, b):
    import torch
    return torch.equal(tc.bits(a) if a.dtype == torch.float32 else a, tc.bits(b) if b.dtype == torch.float32 else b)


class Case:
    """a case's env, its state S0 (numpy and device), the commands and the full result of one rollout call"""

    def __init__(self, n, ground, K, T, motor=False):
        import torch
        self.n, self.ground, self.K, self.T = n, ground, K, T
        self.env = env = tk.make_env("base", n, ground, solver_residual_threshold=0.0, check_actions=False, **sr.STEP_KW)
        self.kinds = tc.write_states(env, n, ground)
        self.bp = bp = sr.body_params(n)
        env.set_body_params(base_mass_scale=bp[0], leg_mass_scale=bp[1], foot_friction=bp[2])
        self.params = sr.motor_params(n) if motor else None
        if motor:
            env.set_motor_params(**self.params)
        torch.cuda.synchronize()
        self.S0 = env.state.clone()
        self.s0 = self.S0.cpu().numpy()
        assert np.all(self.s0[tg.S_MOTOR_EN].view(np.int32) == sr.ALL_MOTORS)
        self.cmd_np = rr.targets(self.s0[13:25].T, K, T)
        self.cmd = tc.dev(env, self.cmd_np)
        self.out = env.rollout(targets=self.cmd, **KW)
        torch.cuda.synchronize()
        heights = env.terrain_heights.cpu().numpy() if ground != "plane" else None
        mids = env.terrain_mids.cpu().numpy() if ground != "plane" else None
        self.fields = kr.scene_fields(ground, heights, mids)
        self.ep = self.s0[tg.S_EPISODE].view(np.int32)

    def kw(self, g):
        """rollout_ref.transition's keywords of env g"""
        p = self.params
        motor = None if p is None else dict(voltage=p["voltage"][g], damping=p["damping"][g], kp=p["kp"][g], kd=p["kd"][g], strength=p["strength"][:, g])
        return dict(field=kr.field_of(self.fields, g, self.ep[g]), scales=(self.bp[0, g], self.bp[1, g]), mu=float(self.bp[2, g]), motor=motor)

    def unchanged(self):
        import torch
        return torch.equal(tc.bits(self.env.state), tc.bits(self.S0))


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n, ground, K, T, motor=False):
        key = (n, ground, K, T, motor)
        if key not in made:
            made[key] = Case(*key)
        return made[key]
    yield get
    for c in made.values():
        c.env.close()


# ---------------------------------------------------------------- A. every emitted transition is one substep of the physics
@pytest.mark.parametrize("n,ground,K,T", rr.CASES, ids=rr.CASE_IDS)
def test_every_emitted_transition_is_one_substep_of_the_reference(cases, n, ground, K, T):
    import torch
    c = cases(n, ground, K, T)
    out = c.out
    assert out.fields == FIELDS and tuple(out) == (out.state, out.trajectory, out.foot_contact, out.sweeps) and len(out) == 4
    assert out.state.shape == (n, K, 37) and out.trajectory.shape == (n, K, T, 37) and out.foot_contact.shape == (n, K, T, 4) and out.sweeps.shape == (n, K)
    assert out.state.dtype == out.trajectory.dtype == torch.float32 and out.foot_contact.dtype == torch.uint8 and out.sweeps.dtype == torch.int32
    assert all(t.device == c.env.device and t.is_contiguous() for t in out)
    assert c.unchanged()
    traj, contact = out.trajectory.cpu().numpy(), out.foot_contact.cpu().numpy()
    assert same(out.state, out.trajectory[:, :, T - 1]) and same(out.base_pos, out.state[..., 0:3]) and same(out.joint_rates, out.state[..., 25:37])
    assert bool((out.sweeps == T * cr.ITERATIONS).all()) and np.isin(contact, (0, 1)).all() and np.isfinite(traj).all()
    dt = rr.DT
    worst = {f: 0.0 for f in rr.FAMILIES}
    integ = np.zeros(3)
    total = kept = touching = 0
    failures = []
    for g in range(n):
        kw, fam = c.kw(g), rr.family(c.kinds[g])
        for k in range(K):
            s = c.s0[0:37, g]
            for t in range(T):
                after = traj[g, k, t]
                tr = rr.transition(s, c.cmd_np[g, k, t], **kw)
                ok = rr.kept(s, kw["field"], tr["ref"], tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"])
                ok = ok and sr.vel_error(rr.transition(s, c.cmd_np[g, k, t], dtype=np.float32, **kw)["v_next"], tr["v_next"]) <= tc.BOUNDS["v_next"]
                total += 1
                # the integrator, every transition: from the emitted state along the emitted velocities
                s64, a64 = s.astype(np.float64), after.astype(np.float64)
                move = dt * a64[sr.VEL_WORDS]
                e_pos = np.abs(a64[0:3] - (s64[0:3] + move[0:3])) / (tg.ULP * (np.abs(s64[0:3]) + np.abs(move[0:3])) + 1e-300)
                e_q = np.abs(a64[13:25] - (s64[13:25] + move[6:18])) / (tg.ULP * (np.abs(s64[13:25]) + np.abs(move[6:18])) + 1e-300)
                e_quat = sr.integrator_errors(s.reshape(37, 1), after.reshape(37, 1), 0, dt)[1] / tg.QUAT_TOL
                integ = np.maximum(integ, [e_pos.max(), e_q.max(), e_quat])
                assert abs(np.linalg.norm(a64[3:7]) - 1.0) <= 5 * 2.0 ** -24
                if ok:
                    kept += 1
                    e = sr.vel_error(after[sr.VEL_WORDS], tr["v_next"])
                    worst[fam] = max(worst[fam], e)
                    touching += int(tr["foot_contact"].any())
                    if not e <= BOUNDS[fam] or not np.array_equal(contact[g, k, t].astype(bool), tr["foot_contact"]):
                        failures.append((g, k, t, c.kinds[g], e, contact[g, k, t].tolist(), tr["foot_contact"].tolist()))
                s = after
    print((n, ground, K, T), "kept %d of %d transitions, %d with a foot on the ground;" % (kept, total, touching),
          "velocities worst / bound:", {f: "%.3e / %.3e" % (worst[f], BOUNDS[f]) for f in rr.FAMILIES},
          "; integrator in units of the tolerance: pos %.3f, q %.3f, quat %.3f" % tuple(integ))
    assert kept >= 0.9 * total, (kept, total)
    assert not failures, (failures[:6], len(failures))
    assert np.all(integ <= 1.0), integ
    assert touching > 0


# ---------------------------------------------------------------- B. the first substep against the step
@pytest.mark.parametrize("n,ground,K,T,motor", [(67, "plane", 2, 3, False), (67, "custom", 2, 3, False), (67, "plane", 2, 3, True)],
                         ids=["67-plane", "67-custom", "67-plane-actuators"])
def test_first_substep_against_the_step(cases, n, ground, K, T, motor):
    """S0, one env.step (one substep: action_repeat 1) -> S1 and the motor command; S0 written back (bits asserted); rollout(targets = the
    command, K = T = repeat = 1).  Both sides lie within their bounds of the common float64 reference (the step: test_gpu_step_readout's a.),
    so they lie within the sum of each other, relative to max(1, largest |component| of the reference's v_next); over the envs
    step_readout_ref.kept keeps."""
    import torch
    c = cases(n, ground, K, T, motor)
    env = c.env
    _, _, _, info = env.step(tc.dev(env, sr.actions(n)))
    torch.cuda.synchronize()
    s1, cmd = env.state.cpu().numpy(), info["action"].clone()
    env.state.copy_(c.S0)
    torch.cuda.synchronize()
    assert c.unchanged()
    out = env.rollout(targets=cmd.reshape(n, 1, 1, 12).contiguous(), **KW)
    torch.cuda.synchronize()
    got, cmd_np = out.state.cpu().numpy()[:, 0], cmd.cpu().numpy()
    worst, kept, failures = {f: 0.0 for f in rr.FAMILIES}, 0, []
    for g in range(n):
        kw, fam = c.kw(g), rr.family(c.kinds[g])
        ref = rr.transition(c.s0[0:37, g], cmd_np[g], **kw)["ref"]
        if not sr.kept(c.s0, g, kw["field"], ref, c.s0[tg.S_MOTOR_EN, g].view(np.int32), tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"]):
            continue
        kept += 1
        e = float(np.abs(got[g][sr.VEL_WORDS].astype(np.float64) - s1[sr.VEL_WORDS, g]).max() / max(1.0, np.abs(ref["v_next"]).max()))
        worst[fam] = max(worst[fam], e)
        if not e <= tg.STEP_BOUNDS[0.0] + BOUNDS[fam]:
            failures.append((g, c.kinds[g], e))
    print((n, ground, "actuators" if motor else ""), "kept %d of %d; rollout against the step, worst / bound:" % (kept, n),
          {f: "%.3e / %.3e" % (worst[f], tg.STEP_BOUNDS[0.0] + BOUNDS[f]) for f in rr.FAMILIES})
    assert kept >= 0.9 * n and not failures, (kept, failures[:6], len(failures))
    if motor:                                                 # the actuator's parameters do enter: the same state and commands in the nominal env
        nominal = cases(67, "plane", 2, 3)
        assert torch.equal(tc.bits(nominal.S0), tc.bits(c.S0))
        assert not same(nominal.env.rollout(targets=cmd.reshape(n, 1, 1, 12).contiguous(), **KW).state, out.state)
    assert c.unchanged()


# ---------------------------------------------------------------- C. bit for bit
def test_tau_mode_is_contact_solve_and_the_candidates_are_independent(cases):
    import torch
    c = cases(67, "custom", 2, 3)
    env, n = c.env, 67
    tau = tc.dev(env, cr.scene_params(n)[0])
    con = env.contact_solve(tau=tau, iterations=cr.ITERATIONS, residual_threshold=0.0)
    one = env.rollout(tau=tau.reshape(n, 1, 1, 12).contiguous(), **KW)
    torch.cuda.synchronize()
    vel = torch.as_tensor(sr.VEL_WORDS, device=env.device)
    assert same(one.state[:, 0][:, vel], con.v_next) and same(one.sweeps[:, 0], con.sweeps)
    assert torch.equal(one.foot_contact[:, 0, 0].bool(), con.foot_contact)
    # candidates: K = 3 against K = 1; a permutation of the candidates permutes the rows
    K, T = 3, 4
    cmd = tc.dev(env, rr.targets(c.s0[13:25].T, K, T))
    full = env.rollout(targets=cmd, **KW)
    single = env.rollout(targets=cmd[:, 1:2].contiguous(), **KW)
    perm = [2, 0, 1]
    moved = env.rollout(targets=cmd[:, perm].contiguous(), **KW)
    torch.cuda.synchronize()
    for name in FIELDS:
        assert same(getattr(full, name)[:, 1:2], getattr(single, name)), name
        assert same(getattr(full, name)[:, perm], getattr(moved, name)), name
    assert not same(full.state[:, 0], full.state[:, 1])
    # env_ids rows
    ids = list(range(66, -1, -3))
    part = env.rollout(targets=cmd[ids].contiguous(), env_ids=ids, **KW)
    torch.cuda.synchronize()
    for name in FIELDS:
        assert same(getattr(part, name), getattr(full, name)[ids]), name
    # prefixes: trajectory[:, :, t] of the T = 4 call is `state` of the T = t + 1 call
    for t in range(T):
        pre = env.rollout(targets=cmd[:, :, :t + 1].contiguous(), fields=("state", "foot_contact"), **KW)
        assert same(pre.state, full.trajectory[:, :, t]) and same(pre.foot_contact, full.foot_contact[:, :, :t + 1]), t
    # repeat = 2 is repeat = 1 with every command doubled, at every second entry
    two = env.rollout(targets=cmd, repeat=2, iterations=cr.ITERATIONS, residual_threshold=0.0)
    doubled = env.rollout(targets=cmd.repeat_interleave(2, dim=2).contiguous(), **KW)
    torch.cuda.synchronize()
    assert same(two.trajectory, doubled.trajectory[:, :, 1::2]) and same(two.state, doubled.state) and same(two.sweeps, doubled.sweeps)
    assert same(two.foot_contact, doubled.foot_contact[:, :, 1::2]) and bool((two.sweeps == 2 * T * cr.ITERATIONS).all())
    assert not same(two.trajectory, full.trajectory)
    # the config's defaults: repeat None is action_repeat (1 here), iterations and threshold the config's (60, 0)
    default = env.rollout(targets=cmd)
    assert all(same(getattr(default, name), getattr(full, name)) for name in FIELDS)
    # fields and out=
    small = env.rollout(targets=cmd, fields=("sweeps", "state"), **KW)
    assert small.fields == ("state", "sweeps") and small.trajectory is None and small.foot_contact is None and tuple(small)[1] is None
    assert same(small.state, full.state) and same(small.sweeps, full.sweeps)
    ptr = small.state.data_ptr()
    small.state.fill_(-7.0)
    again = env.rollout(targets=cmd, fields=("sweeps", "state"), out=small, **KW)
    torch.cuda.synchronize()
    assert again is small and small.state.data_ptr() == ptr and same(small.state, full.state)
    with pytest.raises(ValueError):
        env.rollout(targets=cmd, fields=("state",), out=small, **KW)
    with pytest.raises(ValueError):
        env.rollout(targets=cmd[:, :2].contiguous(), fields=("sweeps", "state"), out=small, **KW)
    assert c.unchanged()


def test_early_exit_counts_each_rows_own_sweeps(cases):
    """the config-style threshold: every substep leaves the sweep loop on its own residual, the counts are summed per row"""
    import torch
    c = cases(130, "plane", 1, 2)
    out = c.env.rollout(targets=c.cmd, repeat=1, iterations=cr.ITERATIONS, residual_threshold=cr.THRESHOLD)
    torch.cuda.synchronize()
    sweeps = out.sweeps.cpu().numpy()
    assert np.all((sweeps >= c.T) & (sweeps <= c.T * cr.ITERATIONS)) and len(set(sweeps.reshape(-1).tolist())) >= 3
    assert not same(out.state, c.out.state) and c.unchanged()


# ---------------------------------------------------------------- D. nothing else is touched
def test_guard_words_around_the_outputs(cases):
    """Every output 16 elements into a larger buffer, then one element further: the sentinels in front of and behind it survive and both
    placements hold the bits of the plain call."""
    import ctypes
    import torch
    from rex_gym_amd import _lib
    c = cases(67, "plane", 2, 3)
    env, n, K, T = c.env, 67, 2, 3
    inp = _lib.RexRolloutIn(c.cmd.data_ptr(), None, K, T, 1, 0.0, cr.ITERATIONS, 0.0)
    sizes = {k: int(getattr(c.out, k).numel()) for k in FIELDS}
    for first in (16, 17):
        bufs = {k: torch.full((sizes[k] + 64,), 249 if k == "foot_contact" else -7, dtype=getattr(c.out, k).dtype, device=env.device) for k in sizes}
        out = _lib.RexRolloutOut(**{k: b[first:].data_ptr() for k, b in bufs.items()})
        _lib.check(env._L.rex_rollout(env._h, None, n, ctypes.byref(inp), ctypes.byref(out), env._stream_ptr()), "rex_rollout")
        torch.cuda.synchronize()
        for k, b in bufs.items():
            guard = 249 if k == "foot_contact" else -7
            assert bool((b[:first] == guard).all()) and bool((b[first + sizes[k]:] == guard).all()), (k, first)
            assert same(b[first:first + sizes[k]], getattr(c.out, k).reshape(-1)), (k, first)
    assert c.unchanged()


# ---------------------------------------------------------------- E. refusals
def test_bad_arguments_and_unsupported_envs_raise(cases):
    import ctypes
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    c = cases(67, "plane", 2, 3)
    env, n, cmd = c.env, 67, c.cmd
    for bad in (torch.zeros((n, 2, 3, 11), device=env.device), torch.zeros((n - 1, 2, 3, 12), device=env.device), torch.zeros((n, 2, 3, 12)),
                torch.zeros((n, 2, 3, 12), dtype=torch.float64, device=env.device), torch.zeros((n, 2, 3, 24), device=env.device)[..., ::2],
                torch.zeros((n, 3, 12), device=env.device), torch.zeros((n, 0, 3, 12), device=env.device), np.zeros((n, 2, 3, 12), np.float32)):
        with pytest.raises(ValueError):
            env.rollout(targets=bad)
        with pytest.raises(ValueError):
            env.rollout(tau=bad)
    with pytest.raises(ValueError):
        env.rollout()
    with pytest.raises(ValueError):
        env.rollout(targets=cmd, tau=cmd)
    for ids in ([67], [-1], []):
        with pytest.raises(IndexError):
            env.rollout(targets=cmd, env_ids=ids)
    for kw in (dict(fields=("nope",)), dict(iterations=1001), dict(iterations=0), dict(dt=0.0), dict(residual_threshold=-1.0), dict(out=object()),
               dict(repeat=0), dict(repeat=1366), dict(repeat=1.5)):
        with pytest.raises(ValueError):
            env.rollout(targets=cmd, **kw)
    L, sp = env._L, env._stream_ptr()
    buf = torch.zeros(n * 2 * 37, device=env.device)
    out, empty, p = _lib.RexRolloutOut(state=buf.data_ptr()), _lib.RexRolloutOut(), cmd.data_ptr()
    In = _lib.RexRolloutIn
    calls = ((In(p, None, 2, 3, 1, 0.0, 0, -1.0), empty, n, b"every output pointer is null"), (In(p, p, 2, 3, 1, 0.0, 0, -1.0), out, n, b"exactly one of"),
             (In(None, None, 2, 3, 1, 0.0, 0, -1.0), out, n, b"exactly one of"), (In(p, None, 0, 3, 1, 0.0, 0, -1.0), out, n, b"candidates"),
             (In(p, None, 2, 0, 1, 0.0, 0, -1.0), out, n, b"steps"), (In(p, None, 2, 3, 1366, 0.0, 0, -1.0), out, n, b"substeps"),
             (In(p, None, 2, 3, 1, 0.0, 1001, -1.0), out, n, b"iterations"), (In(p, None, 2, 3, 1, float("inf"), 0, -1.0), out, n, b"finite"),
             (In(p, None, 2, 3, 1, 0.0, 0, float("nan")), out, n, b"finite"), (In(p, None, 2, 3, 1, 0.0, 0, -1.0), out, 0, b"at least one env"),
             (In(p, None, 2, 3, 1, 0.0, 0, -1.0), out, 68, b"without env ids"), (In(p, None, 2 ** 26, 3, 1, 0.0, 0, -1.0), out, n, b"below 2^31"))
    for inp, o, rows, msg in calls:
        assert L.rex_rollout(env._h, None, rows, ctypes.byref(inp), ctypes.byref(o), sp) == -1 and msg in L.rex_last_error(), (msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and c.unchanged()
    inp = In(p, None, 1, 1, 1, 0.0, 0, -1.0)
    for kw, error, msg in ((dict(mark="arm"), NotImplementedError, b"mark arm"), (dict(on_rack=True), ValueError, b"on_rack"),
                           (dict(task="poses"), ValueError, b"body_contacts"), (dict(pd_latency=0.002), ValueError, b"latency"),
                           (dict(control_latency=0.003), ValueError, b"latency")):
        other = RexBatchEnv(5, **{"task": "walk", "signal_type": "ik", "seed": 5, **kw})
        other.reset()
        state = other.state.clone()
        t5 = torch.zeros((5, 1, 1, 12), device=other.device)
        with pytest.raises(error):
            other.rollout(targets=t5)
        buf5 = torch.zeros(5 * 37, device=other.device)
        o5 = _lib.RexRolloutOut(state=buf5.data_ptr())
        inp5 = In(t5.data_ptr(), None, 1, 1, 1, 0.0, 0, -1.0)
        assert other._L.rex_rollout(other._h, None, 5, ctypes.byref(inp5), ctypes.byref(o5), other._stream_ptr()) == -1 and msg in other._L.rex_last_error()
        torch.cuda.synchronize()
        assert bool((buf5 == 0).all()) and torch.equal(tc.bits(other.state), tc.bits(state))
        other.close()
