"""Rollouts from given states, under base pushes and per-candidate bodies on the GPU (rex_rollout_from, the second instantiation of
rex_rollout_kernel in csrc/rex_rollout.hip; RexBatchEnv.rollout(init_state=, base_wrench=, body=)) against rex_rollout itself, bit for bit,
and against the float64 reference of tests/rollout_from_ref.py.

Envs, states and commands are those of tests/test_gpu_rollout.py (its Case), the cases the two of rollout_ref.CASES that
rollout_from_ref.CASES names: 5 envs on the plane with K = 3, T = 4 and 67 on the random pool with K = 2, T = 3 -- 15 and 134 rows, neither a
multiple of the kernel's 32 rows per workgroup -- and one env_ids subset in reversed order.  Every state handed in is finite and stands on
the env's terrain; bad input is not tried on the device (the kernel was read for it: the header comment of rex_rollout_from).

A. - C. hold no tolerance: the kernel holds W as float32 in LDS and emits it as it is, the two instantiations are one source, and the
build fixes arithmetic by source (-ffp-contract=on).  The wrench is taken off the bias wrench as x - w, and x - (+0) is x: a wrench of
zeros changes no bit.

D. Every emitted transition at repeat = 1 under a wrench and a body drawn per row (rollout_from_ref.draws: force uniform within +- half
the nominal robot's weight per axis, 22.6 N; moment within +- that x 0.1 m; mass scales 0.8 .. 1.2; friction 0.3 .. 1.0) is held to ONE
substep of the reference from the kernel's own emitted state, as in tests/test_gpu_rollout.py: velocities relative to max(1, largest
|component| of the reference's v_next) (step_readout_ref.vel_error), FACTOR (4) x the float32 floor of one transition per family of
columns; positions, joint angles and the quaternion at the integrator tolerances of tests/test_gpu_step_readout.py.  The floor is measured
without a GPU (tests/test_rollout_from_host.py, which holds BOUNDS to it): rollout_from_ref.walk over the two cases, the deviation of the
float32 evaluation's v_next from the float64 one along the float64 trajectory, largest over the kept transitions:

    family      floor       bound
    synthetic   5.185e-05   2.074e-04     (67 envs on the random pool)
    real        9.221e-05   3.688e-04     (5 envs on the plane)

Kept: rollout_ref.kept, unchanged, and float32 numpy within test_gpu_contact_solve.BOUNDS["v_next"] of float64 (as in
tests/test_gpu_rollout.py).  At least 95 % of each case's transitions are kept (asserted; the CPU walk keeps 60 of 60 and 402 of 402)."""
import ctypes

import numpy as np
import pytest

import contact_solve_ref as cr
import rollout_from_ref as rf
import rollout_ref as rr
import step_readout_ref as sr
import test_gpu_contact_solve as tc
import test_gpu_kinematics as tk
import test_gpu_rollout as tro
import test_gpu_step_readout as tg
from rex_gym_amd._lib import RexRolloutFrom          # (a tree without the call fails here: no test of this file passes on it)

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOORS = {"synthetic": 5.185e-05, "real": 9.221e-05}
BOUNDS = {"synthetic": 2.074e-04, "real": 3.688e-04}
KW = tro.KW
FIELDS = tro.FIELDS
same = tro.same


class FromCase(tro.Case):
    """test_gpu_rollout.Case with the case's per-row draws on the device and what the bit tests share: the env's own words 0..36 and body
    parameters repeated over K, a T = 4 command block"""

    def __init__(self, n, ground, K, T):
        super().__init__(n, ground, K, T)
        env = self.env
        self.wr_np, self.body_np = rf.draws(n, K, T)
        self.wr, self.body = tc.dev(env, self.wr_np), tc.dev(env, self.body_np)
        self.own_state = self.S0[0:37].t().contiguous()                                      # [n, 37]
        self.own_body = tc.dev(env, np.repeat(self.bp.T[:, None, :], K, axis=1))              # [n, K, 3]
        self.cmd4 = tc.dev(env, rr.targets(self.s0[13:25].T, K, 4))
        self.wr4 = tc.dev(env, rf.draws(n, K, 4, seed=99)[0])


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(n, ground, K, T):
        key = (n, ground, K, T)
        if key not in made:
            made[key] = FromCase(*key)
        return made[key]
    yield get
    for c in made.values():
        c.env.close()


def equal(a, b, names=FIELDS):
    return [n for n in names if not same(getattr(a, n), getattr(b, n))]


# ---------------------------------------------------------------- A. the env's own inputs handed in change no bit
@pytest.mark.parametrize("n,ground,K,T", rf.CASES, ids=rf.CASE_IDS)
def test_the_envs_own_state_body_and_a_zero_wrench_change_no_bit(cases, n, ground, K, T):
    import torch
    c = cases(n, ground, K, T)
    env, plain = c.env, c.out
    init = c.own_state[:, None, :].expand(n, K, 37).contiguous()
    zero = torch.zeros((n, K, T, 6), device=env.device)
    for kw in (dict(init_state=init), dict(init_state=c.own_state), dict(body=c.own_body), dict(base_wrench=zero),
               dict(init_state=init, body=c.own_body, base_wrench=zero)):
        got = env.rollout(targets=c.cmd, **kw, **KW)
        torch.cuda.synchronize()
        assert got.fields == FIELDS and not equal(got, plain), (sorted(kw), equal(got, plain))
    # ... and each of the three does enter
    for kw in (dict(init_state=init.roll(1, 0).contiguous()), dict(body=c.body), dict(base_wrench=c.wr)):
        got = env.rollout(targets=c.cmd, **kw, **KW)
        torch.cuda.synchronize()
        assert not same(got.state, plain.state) and bool(torch.isfinite(got.trajectory).all()), sorted(kw)
    assert c.unchanged()


# ---------------------------------------------------------------- B. chaining
@pytest.mark.parametrize("n,ground,K,T", rf.CASES, ids=rf.CASE_IDS)
def test_a_rollout_continued_from_its_state_is_the_unsplit_rollout(cases, n, ground, K, T):
    """repeat = 2: T = 4 against T = 2 followed by T = 2 from its `state` under the last two commands, plain and under a wrench and a body"""
    import torch
    c = cases(n, ground, K, T)
    env, kw = c.env, dict(repeat=2, iterations=cr.ITERATIONS, residual_threshold=0.0)
    for extra in ({}, dict(body=c.body, base_wrench=c.wr4)):
        part = lambda lo, hi: {k: (v[:, :, lo:hi].contiguous() if k == "base_wrench" else v) for k, v in extra.items()}
        whole = env.rollout(targets=c.cmd4, **extra, **kw)
        head = env.rollout(targets=c.cmd4[:, :, :2].contiguous(), **part(0, 2), **kw)
        tail = env.rollout(targets=c.cmd4[:, :, 2:].contiguous(), init_state=head.state, **part(2, 4), **kw)
        torch.cuda.synchronize()
        assert same(head.trajectory, whole.trajectory[:, :, :2]) and same(tail.trajectory, whole.trajectory[:, :, 2:]), sorted(extra)
        assert same(head.foot_contact, whole.foot_contact[:, :, :2]) and same(tail.foot_contact, whole.foot_contact[:, :, 2:]), sorted(extra)
        assert same(tail.state, whole.state) and same(head.sweeps + tail.sweeps, whole.sweeps), sorted(extra)
        assert bool((whole.sweeps == 8 * cr.ITERATIONS).all()) and not same(head.state, whole.state)
    assert c.unchanged()


# ---------------------------------------------------------------- C. rows are independent
@pytest.mark.parametrize("n,ground,K,T", rf.CASES, ids=rf.CASE_IDS)
def test_every_row_is_the_single_candidate_call_with_its_inputs(cases, n, ground, K, T):
    """candidate k of env g starts from the state of env (g + k + 1) mod n, in its own body and under its own wrenches; the env_ids subset
    in reversed order picks the same rows"""
    import torch
    c = cases(n, ground, K, T)
    env = c.env
    init = torch.stack([c.own_state.roll(-(k + 1), 0) for k in range(K)], 1).contiguous()
    full = env.rollout(targets=c.cmd, init_state=init, body=c.body, base_wrench=c.wr, **KW)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(full.trajectory).all())
    for k in range(K):
        one = env.rollout(targets=c.cmd[:, k:k + 1].contiguous(), init_state=init[:, k:k + 1].contiguous(), body=c.body[:, k:k + 1].contiguous(),
                          base_wrench=c.wr[:, k:k + 1].contiguous(), **KW)
        torch.cuda.synchronize()
        assert all(same(getattr(one, f), getattr(full, f)[:, k:k + 1]) for f in FIELDS), k
        assert k == 0 or not same(full.state[:, k], full.state[:, 0])
    ids = list(range(n - 1, -1, -3))
    pick = lambda t: t[ids].contiguous()
    part = env.rollout(targets=pick(c.cmd), env_ids=ids, init_state=pick(init), body=pick(c.body), base_wrench=pick(c.wr), **KW)
    torch.cuda.synchronize()
    assert part.state.shape == (len(ids), K, 37) and all(same(getattr(part, f), getattr(full, f)[ids]) for f in FIELDS)
    # fields and out=
    small = env.rollout(targets=c.cmd, init_state=init, body=c.body, base_wrench=c.wr, fields=("state",), **KW)
    small.state.fill_(-7.0)
    again = env.rollout(targets=c.cmd, init_state=init, body=c.body, base_wrench=c.wr, fields=("state",), out=small, **KW)
    torch.cuda.synchronize()
    assert again is small and small.trajectory is None and same(small.state, full.state)
    assert c.unchanged()


# ---------------------------------------------------------------- D. every emitted transition is one substep of the physics
@pytest.mark.parametrize("n,ground,K,T", rf.CASES, ids=rf.CASE_IDS)
def test_every_transition_under_a_wrench_and_a_body_is_one_substep_of_the_reference(cases, n, ground, K, T):
    import torch
    c = cases(n, ground, K, T)
    out = c.env.rollout(targets=c.cmd, base_wrench=c.wr, body=c.body, **KW)
    torch.cuda.synchronize()
    assert c.unchanged()
    traj, contact = out.trajectory.cpu().numpy(), out.foot_contact.cpu().numpy()
    assert same(out.state, out.trajectory[:, :, T - 1]) and bool((out.sweeps == T * cr.ITERATIONS).all()) and np.isfinite(traj).all()
    dt = rr.DT
    worst = {f: 0.0 for f in rr.FAMILIES}
    integ = np.zeros(3)
    total = kept = touching = 0
    failures = []
    for g in range(n):
        fld, fam = c.kw(g)["field"], rr.family(c.kinds[g])
        for k in range(K):
            s = c.s0[0:37, g]
            for t in range(T):
                after = traj[g, k, t]
                args = (s, c.cmd_np[g, k, t], c.wr_np[g, k, t], c.body_np[g, k])
                tr = rf.transition(*args, field=fld)
                ok = rr.kept(s, fld, tr["ref"], tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"])
                ok = ok and sr.vel_error(rf.transition(*args, field=fld, dtype=np.float32)["v_next"], tr["v_next"]) <= tc.BOUNDS["v_next"]
                total += 1
                s64, a64 = s.astype(np.float64), after.astype(np.float64)
                move = dt * a64[sr.VEL_WORDS]
                e_pos = np.abs(a64[0:3] - (s64[0:3] + move[0:3])) / (tg.ULP * (np.abs(s64[0:3]) + np.abs(move[0:3])) + 1e-300)
                e_q = np.abs(a64[13:25] - (s64[13:25] + move[6:18])) / (tg.ULP * (np.abs(s64[13:25]) + np.abs(move[6:18])) + 1e-300)
                e_quat = sr.integrator_errors(s.reshape(37, 1), after.reshape(37, 1), 0, dt)[1] / tg.QUAT_TOL
                integ = np.maximum(integ, [e_pos.max(), e_q.max(), e_quat])
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
    assert kept >= 0.95 * total, (kept, total)
    assert not failures, (failures[:6], len(failures))
    assert np.all(integ <= 1.0), integ
    assert touching > 0


# ---------------------------------------------------------------- E. refusals
def test_bad_inputs_raise_before_any_launch(cases):
    import torch
    from rex_gym_amd import _lib
    n, ground, K, T = rf.CASES[0]
    c = cases(n, ground, K, T)
    env, z = c.env, lambda *shape, **kw: torch.zeros(shape, device=c.env.device, **kw)
    bad = dict(init_state=(z(n, K, 36), z(n - 1, K, 37), z(n, K + 1, 37), z(n, 37, dtype=torch.float64), z(n, K, 74)[..., ::2], torch.zeros((n, K, 37)),
                           np.zeros((n, K, 37), np.float32), z(n, K, 1, 37)),
               base_wrench=(z(n, K, T, 5), z(n, K, T + 1, 6), z(n, K, 6), z(n, K, T, 6, dtype=torch.float16), z(n, K, T, 12)[..., ::2], torch.zeros((n, K, T, 6))),
               body=(z(n, K, 2), z(n, 3), z(n, K, 3, dtype=torch.float64), z(n, K, 6)[..., ::2], torch.zeros((n, K, 3)), [1.0, 1.0, 0.5]))
    for name, tensors in bad.items():
        for t in tensors:
            with pytest.raises(ValueError) as e:
                env.rollout(targets=c.cmd, **{name: t})
            assert str(e.value).startswith("rollout: " + name), (name, str(e.value))
    with pytest.raises(IndexError):
        env.rollout(targets=c.cmd, env_ids=[n], init_state=c.own_state)
    L, sp = env._L, env._stream_ptr()
    buf = z(n * K * 37)
    out, empty, p = _lib.RexRolloutOut(state=buf.data_ptr()), _lib.RexRolloutOut(), c.cmd.data_ptr()
    src, In = RexRolloutFrom(None, None, c.own_body.data_ptr()), _lib.RexRolloutIn
    good = In(p, None, K, T, 1, 0.0, 0, -1.0)
    calls = ((good, None, out, n, b"null pointer"), (good, src, None, n, b"null pointer"), (None, src, out, n, b"null pointer"),
             (good, src, empty, n, b"every output pointer is null"), (In(p, p, K, T, 1, 0.0, 0, -1.0), src, out, n, b"exactly one of"),
             (In(p, None, 0, T, 1, 0.0, 0, -1.0), src, out, n, b"candidates"), (In(p, None, K, 0, 1, 0.0, 0, -1.0), src, out, n, b"steps"),
             (In(p, None, K, T, 1366, 0.0, 0, -1.0), src, out, n, b"substeps"), (In(p, None, K, T, 1, 0.0, 1001, -1.0), src, out, n, b"iterations"),
             (In(p, None, K, T, 1, float("nan"), 0, -1.0), src, out, n, b"finite"), (good, src, out, 0, b"at least one env"),
             (good, src, out, n + 1, b"without env ids"), (In(p, None, 2 ** 26, T, 1, 0.0, 0, -1.0), src, out, n, b"below 2^31"))
    ref = lambda x: ctypes.byref(x) if x is not None else None
    for inp, s, o, rows, msg in calls:
        assert L.rex_rollout_from(env._h, None, rows, ref(inp), ref(s), ref(o), sp) == -1
        assert L.rex_last_error().startswith(b"rex_rollout_from: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and c.unchanged()
    # all three null: the call computes rex_rollout's result
    none = RexRolloutFrom()
    _lib.check(L.rex_rollout_from(env._h, None, n, ctypes.byref(In(p, None, K, T, 1, 0.0, cr.ITERATIONS, 0.0)), ctypes.byref(none), ctypes.byref(out), sp),
               "rex_rollout_from")
    torch.cuda.synchronize()
    assert same(buf.reshape(n, K, 37), c.out.state) and c.unchanged()
