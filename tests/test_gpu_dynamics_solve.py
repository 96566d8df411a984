"""Solves with the mass matrix on the GPU (rex_dynamics_solve, rex_forward_dynamics, rex_apply_impulse; csrc/rex_dynamics_solve.hip) against
the float64 numpy reference of tests/dynamics_solve_ref.py: x_ref = np.linalg.solve(M_ref, b) with M, h and J of dynamics_ref.reference.

States: the scenes of tests/test_gpu_dynamics.py, set up the same way (reset, 8 random steps, synthetic columns over all but the first few
envs, per-env mass scales): 1, 5, 67 and 130 envs on the plane (a lone row, a partial wave, a partial last workgroup), 67 on the random
terrain pool, 67 on the [2, 9, 13] custom field.

Bounds: FACTOR (4) x the larger error of the reference's two float32 routes (a dense Cholesky of the float32 M; the block elimination in
float32) against the float64 reference over the synthetic states of all scenes -- tests/test_dynamics_solve_host.py measures them without a
GPU and holds BOUNDS to them.  The measure is dynamics_solve_ref.errors: |D^1/2 (x - x_ref)| / (kappa |D^1/2 x_ref|) per right-hand side,
D = diag(M_ref), kappa = cond_2(D^-1/2 M_ref D^-1/2) of the env (19.0 .. 52.6 over the scenes' synthetic states):

    kind      floor       bound       right-hand sides
    solve     2.651e-07   1.060e-06   per env six: 3 x sqrt(M_ii) N(0, 1), J_p^T of a unit force at a toe point, h, a unit foot-joint vector
    forward   2.057e-07   8.228e-07   S^T tau + sum J_p^T f_p + w - h from dynamics_solve_ref.loads: each input alone, all together
    impulse   2.053e-07   8.212e-07   the same without h

Toe forces are set to zero at the points dynamics_ref.stable_points rejects (a facet that flips under round-off changes the point, not the
solve); at least 90 % of a scene's points carry a force (asserted; the reference alone rejects none)."""
import numpy as np
import pytest

import dynamics_ref as dr
import dynamics_solve_ref as sr
import kinematics_ref as kr
import test_gpu_dynamics as td
import test_gpu_kinematics as tk
import test_gpu_render as col

pytestmark = pytest.mark.gpu

FACTOR = 4.0
BOUNDS = {"solve": 1.060e-06, "forward": 8.228e-07, "impulse": 8.212e-07}
VEL_WORDS = list(range(7, 13)) + list(range(25, 37))        # REX_S_LINVEL, REX_S_ANGVEL, REX_S_QD: the order of v


def dev(env, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=env.device)


class Scene:
    """a scene's env, its state as numpy, the reference rows (dynamics_ref.reference per env, the kept toe points), its loads with the toe
    forces zeroed at the points left out, and the right-hand sides of the solve"""

    def __init__(self, n, ground):
        self.n, self.ground = n, ground
        self.env = td.make_env(n, ground)
        self.state = self.env.state.cpu().numpy()
        heights = self.env.terrain_heights.cpu().numpy() if ground != "plane" else None
        mids = self.env.terrain_mids.cpu().numpy() if ground != "plane" else None
        self.rows = td.scene_reference(n, ground, self.state, heights, mids)
        self.ok = np.array([row["ok"] for row in self.rows])
        self.load = sr.loads(n)
        self.load["toe"][~self.ok] = 0.0
        self.rhs = np.array([sr.rhs_set(row["ref"], sr.rhs_seed(n, g)) for g, row in enumerate(self.rows)])        # [n, 6, 18] float32
        self.M = [row["ref"]["mass_matrix"] for row in self.rows]

    def inputs(self, combo):
        """(tau, toe [n, 4, 2, 3], wrench) device tensors of the members in combo, None for the others"""
        pick = lambda k, shape: dev(self.env, self.load[k].reshape(shape)) if k in combo else None
        return pick("tau", (self.n, 12)), pick("toe", (self.n, 4, 2, 3)), pick("wrench", (self.n, 6))

    def load_reference(self, combo, with_bias, ids=None):
        out = []
        for g in (range(self.n) if ids is None else ids):
            r = self.rows[g]["ref"]
            b = sr.load_rhs(r["toe_jacobian"], r["bias"] if with_bias else None, **sr.pick(self.load, g, combo))
            out.append(sr.solve_ref(r["mass_matrix"], b)[0])
        return np.array(out)

    def check(self, x, want, kind, what, ids=None):
        """x, want [k, 18] or [k, K, 18] of the envs ids against BOUNDS[kind]"""
        ids = list(range(self.n)) if ids is None else ids
        worst, failures = 0.0, []
        for k, g in enumerate(ids):
            e = sr.errors(x[k], want[k], self.M[g])
            worst = max(worst, float(e.max()))
            if not np.all(e <= BOUNDS[kind]):
                failures.append((g, self.rows[g]["kind"], float(e.max())))
        print(what, kind, "worst / bound: %.2e / %.2e" % (worst, BOUNDS[kind]))
        assert not failures, (what, kind, failures[:8], len(failures))


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(n, ground):
        if (n, ground) not in made:
            made[(n, ground)] = Scene(n, ground)
        return made[(n, ground)]
    yield get
    for s in made.values():
        s.env.close()


def bits(t):
    import torch
    return t.view(torch.int32)


# ---------------------------------------------------------------- a. dynamics_solve against the reference
@pytest.mark.parametrize("mark,n,ground", dr.SCENES)
def test_solve_against_the_reference(scenes, mark, n, ground):
    import torch
    s = scenes(n, ground)
    env = s.env
    want = np.array([sr.solve_ref(s.M[g], s.rhs[g]) for g in range(n)])            # [n, 6, 18]
    one = dev(env, s.rhs[:, 0])
    x1 = env.dynamics_solve(one)
    many = dev(env, s.rhs)
    x6 = env.dynamics_solve(many)
    torch.cuda.synchronize()
    assert x1.shape == (n, 18) and x6.shape == (n, sr.K_SET, 18) and x1.dtype == x6.dtype == torch.float32 and x6.device == env.device
    s.check(x1.cpu().numpy(), want[:, 0], "solve", (n, ground, "K = 1"))
    s.check(x6.cpu().numpy(), want, "solve", (n, ground, "K = 6"))
    assert torch.equal(bits(x6[:, 0]), bits(x1))                                  # a right-hand side's solution does not depend on K
    for rhs, x in ((one, x1), (many, x6)):                                           # in place: bit for bit the out-of-place solution
        work = rhs.clone()
        assert env.dynamics_solve(work, out=work) is work
        torch.cuda.synchronize()
        assert torch.equal(bits(work), bits(x))
    assert torch.equal(many, dev(env, s.rhs))                                        # out of place leaves rhs alone
    assert np.array_equal(env.state.cpu().numpy().view(np.uint32), s.state.view(np.uint32))


def test_solve_of_the_toe_jacobians_gives_the_delassus_matrix(scenes):
    """K = 24: the rows of the GPU's own toe_jacobian as right-hand sides, against the float64 solve of those float32 rows; J M^-1 J^T is then
    symmetric positive semidefinite to round-off."""
    import torch
    s = scenes(67, "custom")
    env = s.env
    J = env.dynamics(fields=("toe_jacobian",)).toe_jacobian.view(s.n, 24, 18)
    X = env.dynamics_solve(J)
    torch.cuda.synchronize()
    Jn = J.cpu().numpy()
    s.check(X.cpu().numpy(), np.array([sr.solve_ref(s.M[g], Jn[g]) for g in range(s.n)]), "solve", "K = 24")
    assert torch.einsum("kpd,kqd->kpq", J, X).shape == (s.n, 24, 24)                   # the README's line
    Xn = X.cpu().numpy().astype(np.float64)
    for g in range(s.n):
        # W = J x^T with |D^1/2 dx_q| <= B kappa |D^1/2 x_q| <= B kappa |D^-1/2 J_q| / lambda_min(D^-1/2 M D^-1/2):  |dW_pq| <= that times |D^-1/2 J_p|
        sd, kappa = sr.conditioning(s.M[g])
        a = np.linalg.norm(Jn[g] / sd, axis=-1)
        dW = BOUNDS["solve"] * kappa / np.linalg.eigvalsh(s.M[g] / np.outer(sd, sd)).min() * np.outer(a, a)
        W = Jn[g].astype(np.float64) @ Xn[g].T
        assert np.all(np.abs(W - W.T) <= 2 * dW), g
        assert np.linalg.eigvalsh(0.5 * (W + W.T)).min() >= -np.linalg.norm(dW), g


# ---------------------------------------------------------------- b. forward_dynamics against the reference
@pytest.mark.parametrize("mark,n,ground", dr.SCENES)
def test_forward_dynamics_against_the_reference(scenes, mark, n, ground):
    import torch
    s = scenes(n, ground)
    env = s.env
    assert s.ok.sum() >= 0.9 * s.ok.size, (int(s.ok.sum()), s.ok.size)
    for combo in sr.COMBOS:
        tau, toe, wrench = s.inputs(combo)
        vdot = env.forward_dynamics(tau=tau, toe_forces=toe, base_wrench=wrench)
        torch.cuda.synchronize()
        assert vdot.shape == (n, 18) and vdot.dtype == torch.float32
        s.check(vdot.cpu().numpy(), s.load_reference(combo, True), "forward", (n, ground, combo))
    with pytest.raises(ValueError):
        env.forward_dynamics()
    assert np.array_equal(env.state.cpu().numpy().view(np.uint32), s.state.view(np.uint32))


def test_a_load_without_the_row_dimension_holds_for_every_row(scenes):
    import torch
    s = scenes(67, "random")
    env = s.env
    tau, toe, wrench = (dev(env, s.load[k][3].reshape(shape)) for k, shape in (("tau", (12,)), ("toe", (4, 2, 3)), ("wrench", (6,))))
    a = env.forward_dynamics(tau=tau, toe_forces=toe, base_wrench=wrench)
    b = env.forward_dynamics(tau=tau.expand(67, 12).contiguous(), toe_forces=toe.expand(67, 4, 2, 3).contiguous(), base_wrench=wrench.expand(67, 6).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(bits(a), bits(b))
    free = env.forward_dynamics(base_wrench=torch.zeros(6, device=env.device)).cpu().numpy()          # no load: M vdot = -h
    s.check(free, np.array([sr.solve_ref(s.M[g], -s.rows[g]["ref"]["bias"])[0] for g in range(67)]), "forward", "free")


# ---------------------------------------------------------------- c. push: dv against the reference, and what it does to the state
@pytest.mark.parametrize("mark,n,ground", dr.SCENES)
def test_push_against_the_reference_and_the_state_words_it_touches(scenes, mark, n, ground):
    import torch
    s = scenes(n, ground)
    env = s.env
    ids = None if n < 67 else [g for g in range(n - 1, -1, -1) if g % 3 != 1]          # the large scenes: a reversed subset
    rows = list(range(n)) if ids is None else ids
    others = [g for g in range(n) if g not in rows]
    saved = env.state.clone()
    try:
        for combo in sr.COMBOS:
            tau, toe, wrench = (t if t is None else t[rows].contiguous() for t in s.inputs(combo))
            before = env.state.cpu().numpy()
            dv = env.push(base_impulse=wrench, toe_impulses=toe, joint_impulses=tau, env_ids=ids)
            torch.cuda.synchronize()
            dvn, after = dv.cpu().numpy(), env.state.cpu().numpy()
            assert dv.shape == (len(rows), 18)
            s.check(dvn, s.load_reference(combo, False, rows), "impulse", (n, ground, combo), rows)
            want = before.copy()
            want[np.ix_(VEL_WORDS, rows)] = (before[np.ix_(VEL_WORDS, rows)] + dvn.T).astype(np.float32)      # one float32 add per word
            assert np.array_equal(after.view(np.uint32), want.view(np.uint32)), combo       # ... and every other word, every other env: as before
            assert np.abs(dvn).max() > 1e-3 and (not others or np.array_equal(after[:, others].view(np.uint32), before[:, others].view(np.uint32)))
            env.state.copy_(saved)
    finally:
        env.state.copy_(saved)
        torch.cuda.synchronize()


# ---------------------------------------------------------------- d. identities between the GPU's own outputs
@pytest.mark.parametrize("n,ground", [(130, "plane"), (67, "custom")])
def test_a_push_changes_the_momentum_by_the_impulse(scenes, n, ground):
    """After a push with the base impulse (p, m) and toe impulses p_k: the linear momentum changes by p + sum p_k, the angular momentum about
    the centre of mass by m + (o_0 - com) x p + sum (P_k - com) x p_k, com_pos does not move, toe_vel changes by J_p dv.
    Slack, from the bounds of the fields involved: a momentum readout is off by BOUNDS[momentum] x its scale (twice: before and after); dv is
    off by at most e = BOUNDS[impulse] kappa |D^1/2 dv| in the D^1/2 norm and the float32 add by 2^-24 |v + dv| per word, which moves row i of
    M dv by at most sqrt(M_ii) lambda_max(D^-1/2 M D^-1/2) times that norm; com and toe_pos enter the lever arms with their bounds."""
    import torch
    s = scenes(n, ground)
    env = s.env
    saved = env.state.clone()
    try:
        _, toe, wrench = s.inputs(("toe", "wrench"))
        d0 = td.to_numpy(env.dynamics(fields=("com", "momentum", "mass", "toe_jacobian")))
        k0 = env.kinematics(fields=("toe_vel", "toe_pos"))
        tv0, P = k0.toe_vel.cpu().numpy().reshape(n, 8, 3).astype(np.float64), k0.toe_pos.cpu().numpy().reshape(n, 8, 3).astype(np.float64)
        dv = env.push(base_impulse=wrench, toe_impulses=toe).cpu().numpy().astype(np.float64)
        d1 = td.to_numpy(env.dynamics(fields=("com", "momentum")))
        tv1 = env.kinematics(fields=("toe_vel",)).toe_vel.cpu().numpy().reshape(n, 8, 3).astype(np.float64)
        torch.cuda.synchronize()
        after = env.state.cpu().numpy().astype(np.float64)
        for g in range(n):
            M = s.M[g]
            sd, kappa = sr.conditioning(M)
            lam = float(np.linalg.eigvalsh(M / np.outer(sd, sd)).max())
            v1 = after[VEL_WORDS, g]
            e = 1.001 * BOUNDS["impulse"] * kappa * np.linalg.norm(sd * dv[g]) + 2.0 ** -24 * np.linalg.norm(sd * v1)
            row = sd * lam * e                                                        # how far row i of M (v + dv) may be off
            mass, com = float(d0["mass"][g]), d0["com"][g, 0:3].astype(np.float64)
            p, m, pk = s.load["wrench"][g, 0:3].astype(np.float64), s.load["wrench"][g, 3:6].astype(np.float64), s.load["toe"][g].astype(np.float64)
            mom0, mom1 = d0["momentum"][g].astype(np.float64), d1["momentum"][g].astype(np.float64)
            lin_read = 1.001 * td.BOUNDS["momentum"] * (max(mass, np.linalg.norm(mom0[0:3])) + max(mass, np.linalg.norm(mom1[0:3])))
            want_lin = p + pk.sum(0)
            assert np.linalg.norm(mom1[0:3] - mom0[0:3] - want_lin) <= lin_read + np.linalg.norm(row[0:3]), (g, s.rows[g]["kind"])
            o0 = s.state[0:3, g].astype(np.float64)
            want_ang = m + np.cross(o0 - com, p) + np.cross(P[g] - com, pk).sum(0)
            rot = np.sqrt(np.trace(M[3:6, 3:6]))
            ang_read = 1.001 * td.BOUNDS["momentum"] * (max(rot, np.linalg.norm(mom0[3:6])) + max(rot, np.linalg.norm(mom1[3:6])))
            levers = np.sqrt(3.0) * (td.BOUNDS["com"] * (np.linalg.norm(p) + np.linalg.norm(pk, axis=-1).sum()) + tk.BOUNDS["toe_pos"] * np.linalg.norm(pk[s.ok[g]], axis=-1).sum())
            ang_slack = ang_read + np.linalg.norm(row[3:6]) + np.linalg.norm(com - o0) * np.linalg.norm(row[0:3]) + levers
            assert np.linalg.norm(mom1[3:6] - mom0[3:6] - want_ang) <= ang_slack, (g, s.rows[g]["kind"])
            assert np.abs(d1["com"][g, 0:3] - d0["com"][g, 0:3]).max() <= 2 * td.BOUNDS["com"]
            J = d0["toe_jacobian"][g].astype(np.float64)
            tv_slack = (tk.BOUNDS["toe_vel"] * (np.maximum(1.0, np.linalg.norm(tv0[g], axis=-1)) + np.maximum(1.0, np.linalg.norm(tv1[g], axis=-1)))
                        + np.sqrt(3.0) * np.abs(dv[g]).sum() * td.BOUNDS["toe_jacobian"] + np.sqrt(3.0) * np.abs(J).max() * 2.0 ** -24 * np.abs(v1).sum())
            assert np.all(np.linalg.norm(tv1[g] - tv0[g] - J @ dv[g], axis=-1) <= tv_slack), (g, s.rows[g]["kind"])
    finally:
        env.state.copy_(saved)
        torch.cuda.synchronize()


# ---------------------------------------------------------------- e. plumbing
@pytest.mark.parametrize("ids", [list(range(66, -1, -1)), [64], [5, 66, 0, 31]], ids=["reversed", "one", "subset"])
@pytest.mark.parametrize("ground", ["plane", "custom"])
def test_env_ids(scenes, ids, ground):
    import torch
    s = scenes(67, ground)
    env = s.env
    rhs = dev(env, s.rhs)
    tau, toe, wrench = s.inputs(("tau", "toe", "wrench"))
    full_x, full_v = env.dynamics_solve(rhs), env.forward_dynamics(tau, toe, wrench)
    part_x = env.dynamics_solve(rhs[ids].contiguous(), env_ids=ids)
    part_v = env.forward_dynamics(tau[ids].contiguous(), toe[ids].contiguous(), wrench[ids].contiguous(), env_ids=ids)
    torch.cuda.synchronize()
    assert part_x.shape == (len(ids), sr.K_SET, 18) and part_v.shape == (len(ids), 18)
    assert torch.equal(bits(part_x), bits(full_x[ids])) and torch.equal(bits(part_v), bits(full_v[ids]))      # bit for bit the full call's rows
    assert not torch.equal(full_v[0], full_v[5])


def test_guard_words_around_out(scenes):
    """Each output 16 floats into a larger buffer, then one float further (off every wider alignment): the sentinels in front of and behind it
    survive and both placements hold the same bits."""
    import torch
    s = scenes(67, "plane")
    env, n = s.env, 67
    rhs = dev(env, s.rhs)
    _, toe, wrench = s.inputs(("toe", "wrench"))
    saved = env.state.clone()
    calls = {"solve": (n * sr.K_SET * 18, (n, sr.K_SET, 18), lambda out: env.dynamics_solve(rhs, out=out)),
             "forward": (n * 18, (n, 18), lambda out: env.forward_dynamics(toe_forces=toe, base_wrench=wrench, out=out)),
             "push": (n * 18, (n, 18), lambda out: env.push(base_impulse=wrench, toe_impulses=toe, out=out))}
    try:
        for name, (size, shape, call) in calls.items():
            got = []
            for first in (16, 17):
                buf = torch.full((size + 64,), -7.0, dtype=torch.float32, device=env.device)
                out = buf[first:first + size].view(shape)
                assert call(out) is out
                torch.cuda.synchronize()
                env.state.copy_(saved)
                b = buf.cpu().numpy()
                assert np.all(b[:first] == -7.0) and np.all(b[first + size:] == -7.0), (name, first)
                got.append(b[first:first + size])
            assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)) and not np.any(got[0] == -7.0), name
    finally:
        env.state.copy_(saved)
        torch.cuda.synchronize()


def test_on_a_stream_of_its_own():
    import torch
    from rex_gym_amd import RexBatchEnv
    stream = torch.cuda.Stream()
    kw = dict(task="walk", signal_type="ik", seed=5)
    env, twin = RexBatchEnv(37, stream=stream, **kw), RexBatchEnv(37, **kw)
    for e in (env, twin):
        e.reset()
        col._steps(e, 3, seed=2)
    ids = [36, 0, 7]
    rng = np.random.RandomState(3)
    rhs, imp = rng.standard_normal((3, 2, 18)).astype(np.float32), rng.standard_normal((3, 6)).astype(np.float32)
    got = []
    for e in (env, twin):
        r, w = dev(e, rhs), dev(e, imp)
        torch.cuda.synchronize()
        got.append((e.dynamics_solve(r, env_ids=ids), e.forward_dynamics(base_wrench=w, env_ids=ids), e.push(base_impulse=w, env_ids=ids)))
        stream.synchronize()
        torch.cuda.synchronize()
    for a, b in zip(*got):
        assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(env.state), bits(twin.state))
    env.close(); twin.close()


# ---------------------------------------------------------------- f. the step after it
def test_steps_after_the_solves_and_after_a_push():
    """A zero impulse leaves the state bit-identical; a step after it, and after the read-only dynamics_solve / forward_dynamics, matches a
    twin that made none of these calls, bit for bit.  A second twin pushed with the base impulse (1 N s, 0, 0) is ahead of the first in
    REX_S_POS x after one step."""
    import torch
    from rex_gym_amd import RexBatchEnv
    kw = dict(task="walk", signal_type="ik", seed=7, terrain_type="random", terrain_pool=kr.POOL)
    env, twin, pushed = RexBatchEnv(67, **kw), RexBatchEnv(67, **kw), RexBatchEnv(67, **kw)
    for e in (env, twin, pushed):
        e.reset()
        col._steps(e, 4, seed=6)
    before = env.state.clone()
    env.dynamics_solve(torch.ones((67, 18), device=env.device))
    env.forward_dynamics(tau=torch.ones(12, device=env.device))
    dv = env.push(base_impulse=torch.zeros(6, device=env.device))
    torch.cuda.synchronize()
    assert not dv.any() and torch.equal(bits(env.state), bits(before))
    dv = pushed.push(base_impulse=torch.tensor([1.0, 0, 0, 0, 0, 0], device=pushed.device))
    torch.cuda.synchronize()
    assert bool((dv[:, 0] > 0).all()) and torch.equal(bits(pushed.state[0:7]), bits(before[0:7]))
    for e in (env, twin, pushed):
        col._steps(e, 1, seed=8)
    torch.cuda.synchronize()
    assert torch.equal(bits(env.state), bits(twin.state))
    assert bool((pushed.state[0] > twin.state[0]).all())
    for e in (env, twin, pushed):
        e.close()


# ---------------------------------------------------------------- g. refusals, all before any launch
def test_bad_arguments_raise_before_any_launch(scenes):
    import ctypes
    import torch
    from rex_gym_amd import _lib
    s = scenes(67, "plane")
    env, n = s.env, 67
    good = torch.zeros((n, 18), device=env.device)
    w = torch.ones((n, 6), device=env.device)
    cpu = torch.device("cpu")
    for ids in ([67], [-1], []):
        for call in (lambda: env.dynamics_solve(good, env_ids=ids), lambda: env.forward_dynamics(base_wrench=w, env_ids=ids), lambda: env.push(base_impulse=w, env_ids=ids)):
            with pytest.raises(IndexError):
                call()
    bad_rhs = [torch.zeros((n, 17), device=env.device), torch.zeros((n - 1, 18), device=env.device), torch.zeros((n, 0, 18), device=env.device),
               torch.zeros((n, 18), dtype=torch.float64, device=env.device), torch.zeros((n, 18), device=cpu), torch.zeros((n, 36), device=env.device)[:, ::2],
               torch.zeros((n * 18,), device=env.device), np.zeros((n, 18), np.float32)]
    for rhs in bad_rhs:
        with pytest.raises(ValueError):
            env.dynamics_solve(rhs)
    for out in (torch.zeros((n, 17), device=env.device), torch.zeros((n, 18), device=cpu), torch.zeros((n, 18), dtype=torch.float64, device=env.device),
                torch.zeros((n, 36), device=env.device)[:, ::2]):
        with pytest.raises(ValueError):
            env.dynamics_solve(good, out=out)
        with pytest.raises(ValueError):
            env.forward_dynamics(base_wrench=w, out=out)
        with pytest.raises(ValueError):
            env.push(base_impulse=w, out=out)
    both = torch.zeros((n * 18 + 18,), device=env.device)
    with pytest.raises(ValueError):
        env.dynamics_solve(both[:n * 18].view(n, 18), out=both[18:].view(n, 18))          # overlapping in part
    for kw in (dict(tau=torch.zeros((n, 11), device=env.device)), dict(toe_forces=torch.zeros((n, 8, 3), device=env.device)),
               dict(base_wrench=torch.zeros((n, 6), device=cpu)), dict(base_wrench=torch.zeros((n, 6), dtype=torch.float64, device=env.device)),
               dict(base_wrench=torch.zeros((n, 12), device=env.device)[:, ::2]), dict(tau=torch.zeros((n - 1, 12), device=env.device)), dict()):
        with pytest.raises(ValueError):
            env.forward_dynamics(**kw)
        with pytest.raises(ValueError):
            env.push(**{{"tau": "joint_impulses", "toe_forces": "toe_impulses", "base_wrench": "base_impulse"}[k]: v for k, v in kw.items()})
    with pytest.raises(ValueError):
        env.push(base_impulse=w[:4].contiguous(), env_ids=[5, 66, 5, 0])                      # duplicate ids
    L, buf = env._L, torch.zeros(n * 18, dtype=torch.float32, device=env.device)
    p, sp = buf.data_ptr(), env._stream_ptr()
    load, empty = _lib.RexDynamicsLoad(base=w.data_ptr()), _lib.RexDynamicsLoad()
    one_id = torch.zeros(1, dtype=torch.int32, device=env.device).data_ptr()
    calls = ((lambda: L.rex_dynamics_solve(env._h, None, 0, 1, p, p, sp), b"at least one env"), (lambda: L.rex_dynamics_solve(env._h, None, 68, 1, p, p, sp), b"without env ids"),
             (lambda: L.rex_dynamics_solve(env._h, None, n, 0, p, p, sp), b"at least one right-hand side"),
             (lambda: L.rex_dynamics_solve(env._h, one_id, 2 ** 20, 2 ** 7, p, p, sp), b"2^31"), (lambda: L.rex_dynamics_solve(env._h, None, n, 1, p, p + 72, sp), b"overlap"),
             (lambda: L.rex_dynamics_solve(env._h, None, n, 1, None, p, sp), b"null pointer"), (lambda: L.rex_forward_dynamics(env._h, None, n, None, p, sp), b"null pointer"),
             (lambda: L.rex_forward_dynamics(env._h, None, -2, ctypes.byref(load), p, sp), b"at least one env"),
             (lambda: L.rex_apply_impulse(env._h, None, n, ctypes.byref(empty), p, sp), b"every impulse pointer is null"),
             (lambda: L.rex_apply_impulse(env._h, None, n, None, p, sp), b"null pointer"), (lambda: L.rex_apply_impulse(env._h, None, 68, ctypes.byref(load), None, sp), b"without env ids"))
    for call, msg in calls:
        assert call() == -1 and msg in L.rex_last_error(), (msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and bool((good == 0).all())
    assert np.array_equal(env.state.cpu().numpy().view(np.uint32), s.state.view(np.uint32))


def test_mark_arm_on_rack_and_a_push_before_reset_are_refused():
    import ctypes
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    arm = RexBatchEnv(5, task="walk", signal_type="ik", mark="arm", seed=5)
    arm.reset()
    w = torch.ones((5, 6), device=arm.device)
    buf = torch.zeros((5, 18), device=arm.device)
    for call in (lambda: arm.dynamics_solve(buf), lambda: arm.forward_dynamics(base_wrench=w), lambda: arm.push(base_impulse=w)):
        with pytest.raises(NotImplementedError):
            call()
    load = _lib.RexDynamicsLoad(base=w.data_ptr())
    state = arm.state.clone()
    for rc in (arm._L.rex_dynamics_solve(arm._h, None, 5, 1, w.data_ptr(), buf.data_ptr(), arm._stream_ptr()),
               arm._L.rex_forward_dynamics(arm._h, None, 5, ctypes.byref(load), buf.data_ptr(), arm._stream_ptr()),
               arm._L.rex_apply_impulse(arm._h, None, 5, ctypes.byref(load), buf.data_ptr(), arm._stream_ptr())):
        assert rc == -1 and b"mark arm" in arm._L.rex_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and torch.equal(bits(arm.state), bits(state))
    arm.close()
    rack = RexBatchEnv(5, task="walk", signal_type="ik", on_rack=True, seed=5)
    w = torch.ones((5, 6), device=rack.device)
    buf = torch.zeros((5, 18), device=rack.device)
    rack.reset()
    state = rack.state.clone()
    with pytest.raises(ValueError):
        rack.push(base_impulse=w)
    load = _lib.RexDynamicsLoad(base=w.data_ptr())
    assert rack._L.rex_apply_impulse(rack._h, None, 5, ctypes.byref(load), buf.data_ptr(), rack._stream_ptr()) == -1 and b"on_rack" in rack._L.rex_last_error()
    assert rack.forward_dynamics(base_wrench=w).shape == (5, 18)                     # the read-only calls work on a rack (the anchor is left out)
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and torch.equal(bits(rack.state), bits(state))
    rack.close()
    fresh = RexBatchEnv(5, task="walk", signal_type="ik", seed=5)
    state = fresh.state.clone()
    with pytest.raises(RuntimeError):
        fresh.push(base_impulse=torch.ones((5, 6), device=fresh.device))
    torch.cuda.synchronize()
    assert torch.equal(bits(fresh.state), bits(state))
    fresh.close()
