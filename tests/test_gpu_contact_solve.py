"""The contact solve on the GPU (rex_contact_solve, csrc/rex_contact_solve.hip) against the float64 numpy reference of
tests/contact_solve_ref.py (dense M, h and toe Jacobians of dynamics_ref, the toe points of kinematics_ref, a restated damping force and a
dense projected Gauss-Seidel) and, for one scene, against the C oracle directly.

States: the scenes of contact_solve_ref -- sizes and grounds of tests/test_gpu_dynamics.py (1, 5, 67, 130 envs on the plane: a lone row, a
partial wave, a partial last workgroup; 67 on the random terrain pool; 67 on the custom field), the leading columns real (reset, 8 random
steps), the others half kinematics_ref's synthetic states (every third with two joints beyond a bound) and half the "stance" family
that stands on two to eight toe points; per-env mass scales (dynamics_ref.scene_scales), friction 0.3 .. 0.9 and torques in +-3 N m
(contact_solve_ref.scene_params).

Bounds: FACTOR (4) x the deviation of the reference evaluated in float32 from float64 over the compared synthetic states of all scenes, 60
sweeps, residual threshold 0 (tests/test_contact_solve_host.py measures them without a GPU and holds BOUNDS to them); the measures are
contact_solve_ref.errors', one number per env and field, each relative to a scale of that env:

    field         floor       bound       relative to
    toe_force     1.832e-04   7.329e-04   max(largest |component| of the env's reference forces, mass x 10 N)
    toe_lambda    1.913e-04   7.652e-04   max(largest |lambda| of the env's reference, mass x 10 x dt N s)
    limit_torque  5.675e-06   2.270e-05   max(largest |torque| of the env's reference, mass x 10 x 0.1 N m)
    v_next        1.001e-04   4.005e-04   max(1, largest |component| of the reference)

(Re-measured with the custom field's grid constants held as the float32 values the product holds, kinematics_ref.grid_constants: before, the
floors were 3.470e-04, 2.782e-04 and 1.585e-04, the largest deviations those of a reference standing 1e-8 m beside the kernel's grid.  Sixty Gauss-Seidel sweeps over rows that clamp are not a smooth function of the data: the floors are those of the problem, two to three
orders over a single solve's.)  An env is left out of the numerical comparison only where a discrete decision sits within round-off of its
threshold (contact_solve_ref.compared); at least 90 % of every scene's envs are compared (asserted)."""
import numpy as np
import pytest

import contact_solve_ref as cr
import dynamics_ref as dr
import kinematics_ref as kr
import test_gpu_dynamics as td
import test_gpu_dynamics_solve as ts
import test_gpu_kinematics as tk

pytestmark = pytest.mark.gpu

FACTOR = 4.0
BOUNDS = {"toe_force": 7.329e-04, "toe_lambda": 7.652e-04, "limit_torque": 2.270e-05, "v_next": 4.005e-04}
ULP = 2.0 ** -23


def dev(env, a, dtype=np.float32):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=env.device)


def bits(t):
    import torch
    return t if t.dtype == torch.int32 else t.view(torch.int32)


def write_states(env, n, ground):
    """contact_solve_ref's synthetic columns over all but the first few envs (the episode word is kinematics_ref's, already there)"""
    import torch
    S, kinds = cr.scene_states(n, ground)
    keep = kr.scene_keep(n)
    env.state[0:37, keep:] = torch.as_tensor(S, device=env.device)[0:37, keep:]
    torch.cuda.synchronize()
    return kinds


def to_numpy(con):
    return {k: getattr(con, k).cpu().numpy().reshape((-1,) + {"toe_force": (8, 3), "toe_lambda": (8, 3)}.get(k, getattr(con, k).shape[1:])) for k in con.fields}


class Scene:
    """a scene's env, its state as numpy, the reference rows (60 sweeps, threshold 0), which envs are compared, and the full GPU result"""

    def __init__(self, n, ground, unit=False):
        import torch
        self.n, self.ground = n, ground
        self.env = env = tk.make_env("base", n, ground) if unit else td.make_env(n, ground)
        self.kinds = write_states(env, n, ground)
        tau, mu = cr.scene_params(n)
        if not unit:
            env.set_body_params(foot_friction=mu)
        self.mu = np.full(n, 0.5, np.float32) if unit else mu
        self.tau_np, self.tau = tau, dev(env, tau)
        self.state = env.state.cpu().numpy()
        heights = env.terrain_heights.cpu().numpy() if ground != "plane" else None
        mids = env.terrain_mids.cpu().numpy() if ground != "plane" else None
        self.rows = cr.scene_reference(n, ground, self.state, heights, mids, unit=unit)
        self.ok = np.array([cr.compared(self.state, g, r["field"], r, tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"]) for g, r in enumerate(self.rows)])
        self.con = env.contact_solve(tau=self.tau, iterations=cr.ITERATIONS, residual_threshold=0.0)
        torch.cuda.synchronize()
        self.gpu = to_numpy(self.con)

    def unchanged(self):
        return np.array_equal(self.env.state.cpu().numpy().view(np.uint32), self.state.view(np.uint32))


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(n, ground, unit=False):
        if (n, ground, unit) not in made:
            made[(n, ground, unit)] = Scene(n, ground, unit)
        return made[(n, ground, unit)]
    yield get
    for s in made.values():
        s.env.close()


# ---------------------------------------------------------------- a. every scene against the reference
@pytest.mark.parametrize("mark,n,ground", dr.SCENES)
def test_scene_against_the_reference(scenes, mark, n, ground):
    import torch
    s = scenes(n, ground)
    env, con, gpu = s.env, s.con, s.gpu
    assert con.fields == tuple(cr.FIELDS) + ("sweeps",)
    assert con.toe_force.shape == con.toe_lambda.shape == (n, 4, 2, 3) and con.limit_torque.shape == (n, 12) and con.v_next.shape == (n, 18)
    assert con.sweeps.shape == (n,) and con.sweeps.dtype == torch.int32
    assert all(getattr(con, k).dtype == torch.float32 for k in cr.FIELDS) and all(getattr(con, k).device == env.device for k in con.fields)
    assert con.foot_force.shape == (n, 4, 3) and con.foot_contact.shape == (n, 4) and con.foot_contact.dtype == torch.bool
    assert s.unchanged()
    assert np.all(gpu["sweeps"] == cr.ITERATIONS)
    worst, failures = {k: 0.0 for k in cr.FIELDS}, []
    for g in np.nonzero(s.ok)[0]:
        for k, e in cr.errors({k: gpu[k][g] for k in cr.FIELDS}, s.rows[g]).items():
            worst[k] = max(worst[k], e)
            if not e <= BOUNDS[k]:
                failures.append((k, int(g), s.kinds[g], e))
    print((n, ground), "worst / bound:", {k: "%.2e / %.2e" % (worst[k], BOUNDS[k]) for k in cr.FIELDS}, "compared %d of %d" % (s.ok.sum(), n))
    assert not failures, (failures[:8], len(failures))
    assert s.ok.sum() >= 0.9 * n
    # identities of the GPU's own outputs, every env
    kin = env.kinematics(fields=("toe_normal", "toe_in_reach"))
    reach = kin.toe_in_reach.cpu().numpy().reshape(n, 8).astype(bool)
    nrm = kin.toe_normal.cpu().numpy().reshape(n, 8, 3)
    lam, force = gpu["toe_lambda"].astype(np.float64), gpu["toe_force"].astype(np.float64)
    assert np.all(gpu["toe_lambda"][~reach] == 0) and np.all(gpu["toe_force"][~reach] == 0)
    assert np.all(lam[..., 0] >= 0)
    assert np.all(np.abs(lam[..., 1:]) <= s.mu.astype(np.float64)[:, None, None] * lam[..., 0:1] * (1 + 2 * ULP))
    assert np.array_equal(con.foot_contact.cpu().numpy(), (gpu["toe_lambda"][..., 0] > 0).reshape(n, 4, 2).any(-1))
    assert np.array_equal(con.foot_force.cpu().numpy(), con.toe_force.sum(dim=2).cpu().numpy())
    for g in range(n):
        for p in np.nonzero(reach[g])[0]:
            t1, t2 = cr.plane_space(nrm[g, p])
            want = (lam[g, p, 0] * nrm[g, p] + lam[g, p, 1] * t1 + lam[g, p, 2] * t2) / cr.DT
            assert np.all(np.abs(force[g, p] - want) <= 16 * ULP * np.abs(lam[g, p]).sum() / cr.DT), (g, p)
    assert (lam[..., 0] > 0).any() or n == 1


# ---------------------------------------------------------------- b. against the C oracle directly
def test_plane_scene_with_default_scales_against_the_oracle(scenes):
    """67 envs on the plane, mass scales 1, mu 0.5: v_next against Oracle(np.float64).physics_substep on the env's own state words, one
    substep per env, 60 sweeps, at the v_next bound."""
    import orclib
    s = scenes(67, "plane", True)
    oracle = orclib.Oracle(np.float64)
    worst, failures = 0.0, []
    for g in np.nonzero(s.ok)[0]:
        want = oracle.physics_substep(s.state[:, g].astype(np.float64), s.tau_np[g], dt=cr.DT, iterations=cr.ITERATIONS, residual_threshold=0.0)[ts.VEL_WORDS]
        e = float(np.abs(s.gpu["v_next"][g] - want).max() / max(1.0, np.abs(want).max()))
        worst = max(worst, e)
        if not e <= BOUNDS["v_next"]:
            failures.append((int(g), s.kinds[g], e))
    print("against the oracle: worst / bound %.2e / %.2e, compared %d of 67" % (worst, BOUNDS["v_next"], s.ok.sum()))
    assert not failures and s.ok.sum() >= 60, (failures[:8], len(failures))
    assert s.unchanged()


# ---------------------------------------------------------------- c. consistency with rex_forward_dynamics
@pytest.mark.parametrize("n,ground", [(130, "plane"), (67, "custom")])
def test_without_damping_v_next_is_the_forward_dynamics_of_its_own_forces(scenes, n, ground):
    """damping=False: v_next = v + dt forward_dynamics(tau + limit_torque, toe_force) wherever no component meets the +-100 clamp; both
    sides are the GPU's, the bound is the sum of the forward and the v_next bounds, relative to max(1, largest |component| of v_next)."""
    import torch
    s = scenes(n, ground)
    env = s.env
    con = env.contact_solve(tau=s.tau, iterations=cr.ITERATIONS, residual_threshold=0.0, damping=False)
    vdot = env.forward_dynamics(tau=s.tau + con.limit_torque, toe_forces=con.toe_force)
    torch.cuda.synchronize()
    v = s.state[ts.VEL_WORDS].T.astype(np.float64)
    got, want = con.v_next.cpu().numpy().astype(np.float64), v + cr.DT * vdot.cpu().numpy().astype(np.float64)
    free = np.abs(got).max(-1) < cr.MAX_VEL
    e = np.abs(got - want).max(-1) / np.maximum(1.0, np.abs(got).max(-1))
    print((n, ground), "worst %.2e, bound %.2e, %d of %d unclamped" % (e[free].max(), ts.BOUNDS["forward"] + BOUNDS["v_next"], free.sum(), n))
    assert free.sum() >= 0.9 * n and np.all(e[free] <= ts.BOUNDS["forward"] + BOUNDS["v_next"])
    assert not torch.equal(con.v_next, s.con.v_next) and s.unchanged()               # the damping forces do enter the default call


# ---------------------------------------------------------------- d. early exit
def test_early_exit_is_each_envs_own(scenes):
    import torch
    s = scenes(130, "plane")
    env = s.env
    con = env.contact_solve(tau=s.tau)                                            # the config's 60 sweeps and threshold
    torch.cuda.synchronize()
    sweeps = con.sweeps.cpu().numpy()
    assert np.all((sweeps >= 1) & (sweeps <= cr.ITERATIONS)) and len(set(sweeps.tolist())) >= 3, sorted(set(sweeps.tolist()))
    explicit = env.contact_solve(tau=s.tau, dt=cr.DT, iterations=cr.ITERATIONS, residual_threshold=cr.THRESHOLD)
    assert all(torch.equal(bits(getattr(con, k)), bits(getattr(explicit, k))) for k in con.fields)
    values = sorted(set(sweeps.tolist()))
    for v in values[:2] + values[len(values) // 2:len(values) // 2 + 1] + values[-2:]:
        cut = env.contact_solve(tau=s.tau, iterations=int(v), residual_threshold=0.0)
        torch.cuda.synchronize()
        rows = torch.as_tensor(np.nonzero(sweeps == v)[0], device=env.device)
        assert bool((cut.sweeps == int(v)).all())
        for k in cr.FIELDS:
            assert torch.equal(bits(getattr(cut, k)[rows]), bits(getattr(con, k)[rows])), (v, k)
    one = env.contact_solve(tau=s.tau, iterations=1, residual_threshold=0.0)
    assert not torch.equal(one.v_next, s.con.v_next) and bool((one.sweeps == 1).all())
    assert s.unchanged()


# ---------------------------------------------------------------- e. plumbing
@pytest.mark.parametrize("ground", ["plane", "custom"])
def test_env_ids_tau_forms_fields_and_out(scenes, ground):
    import torch
    s = scenes(67, ground)
    env, full = s.env, s.con
    kw = dict(iterations=cr.ITERATIONS, residual_threshold=0.0)
    ids = list(range(66, -1, -3))
    part = env.contact_solve(tau=s.tau[ids].contiguous(), env_ids=ids, **kw)
    torch.cuda.synchronize()
    assert part.v_next.shape == (len(ids), 18) and part.sweeps.shape == (len(ids),)
    for k in full.fields:
        assert torch.equal(bits(getattr(part, k)), bits(getattr(full, k)[ids])), k
    one = env.contact_solve(tau=s.tau[5].contiguous(), **kw)                      # a [12] tau holds for every row
    assert torch.equal(bits(one.v_next), bits(env.contact_solve(tau=s.tau[5].expand(67, 12).contiguous(), **kw).v_next))
    assert torch.equal(bits(one.v_next[5]), bits(full.v_next[5])) and not torch.equal(one.v_next[6], full.v_next[6])
    none, zero = env.contact_solve(**kw), env.contact_solve(tau=torch.zeros((67, 12), device=env.device), **kw)
    assert all(torch.equal(bits(getattr(none, k)), bits(getattr(zero, k))) for k in full.fields)
    small = env.contact_solve(tau=s.tau, fields=("sweeps", "toe_force"), **kw)
    assert small.fields == ("toe_force", "sweeps") and small.v_next is None and small.toe_lambda is None
    assert torch.equal(bits(small.toe_force), bits(full.toe_force)) and torch.equal(small.sweeps, full.sweeps)
    with pytest.raises(AttributeError):
        small.foot_contact
    ptr = small.toe_force.data_ptr()
    small.toe_force.fill_(-7.0)
    again = env.contact_solve(tau=s.tau, fields=("sweeps", "toe_force"), out=small, **kw)
    torch.cuda.synchronize()
    assert again is small and small.toe_force.data_ptr() == ptr and torch.equal(bits(small.toe_force), bits(full.toe_force))
    with pytest.raises(ValueError):
        env.contact_solve(tau=s.tau, fields=("toe_force",), out=small, **kw)
    assert s.unchanged()


def test_guard_words_around_the_outputs(scenes):
    """Every output 16 elements into a larger buffer, then one element further: the sentinels in front of and behind it survive and both
    placements hold the bits of the plain call."""
    import ctypes
    import torch
    from rex_gym_amd import _lib
    s = scenes(67, "plane")
    env, n = s.env, 67
    inp = _lib.RexContactSolveIn(s.tau.data_ptr(), 0.0, cr.ITERATIONS, 0.0, 1)
    sizes = {k: int(getattr(s.con, k).numel()) for k in s.con.fields}
    for first in (16, 17):
        bufs = {k: torch.full((sizes[k] + 64,), -7, dtype=getattr(s.con, k).dtype, device=env.device) for k in sizes}
        out = _lib.RexContactSolveOut(**{k: b[first:].data_ptr() for k, b in bufs.items()})
        _lib.check(env._L.rex_contact_solve(env._h, None, n, ctypes.byref(inp), ctypes.byref(out), env._stream_ptr()), "rex_contact_solve")
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert bool((b[:first] == -7).all()) and bool((b[first + sizes[k]:] == -7).all()), (k, first)
            assert torch.equal(bits(b[first:first + sizes[k]]), bits(getattr(s.con, k).reshape(-1))), (k, first)
    assert s.unchanged()


def test_bad_arguments_and_unsupported_envs_raise(scenes):
    import ctypes
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    s = scenes(67, "plane")
    env, n = s.env, 67
    cpu = torch.device("cpu")
    for tau in (torch.zeros((n, 11), device=env.device), torch.zeros((n - 1, 12), device=env.device), torch.zeros((n, 12), device=cpu),
                torch.zeros((n, 12), dtype=torch.float64, device=env.device), torch.zeros((n, 24), device=env.device)[:, ::2], np.zeros((n, 12), np.float32)):
        with pytest.raises(ValueError):
            env.contact_solve(tau=tau)
    for ids in ([67], [-1], []):
        with pytest.raises(IndexError):
            env.contact_solve(env_ids=ids)
    for kw in (dict(fields=("nope",)), dict(iterations=1001), dict(iterations=0), dict(dt=0.0), dict(residual_threshold=-1.0), dict(out=object())):
        with pytest.raises(ValueError):
            env.contact_solve(**kw)
    L, sp = env._L, env._stream_ptr()
    buf = torch.zeros(n * 24, device=env.device)
    out, empty = _lib.RexContactSolveOut(toe_force=buf.data_ptr()), _lib.RexContactSolveOut()
    calls = ((_lib.RexContactSolveIn(None, 0.0, 0, -1.0, 1), empty, n, b"every output pointer is null"), (_lib.RexContactSolveIn(None, 0.0, 1001, -1.0, 1), out, n, b"iterations"),
             (_lib.RexContactSolveIn(None, float("inf"), 0, -1.0, 1), out, n, b"finite"), (_lib.RexContactSolveIn(None, 0.0, 0, float("nan"), 1), out, n, b"finite"),
             (_lib.RexContactSolveIn(None, 0.0, 0, -1.0, 1), out, 0, b"at least one env"), (_lib.RexContactSolveIn(None, 0.0, 0, -1.0, 1), out, 68, b"without env ids"))
    for inp, o, rows, msg in calls:
        assert L.rex_contact_solve(env._h, None, rows, ctypes.byref(inp), ctypes.byref(o), sp) == -1 and msg in L.rex_last_error(), (msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and s.unchanged()
    inp = _lib.RexContactSolveIn(None, 0.0, 0, -1.0, 1)
    for kw, error, msg in ((dict(mark="arm"), NotImplementedError, b"mark arm"), (dict(on_rack=True), ValueError, b"on_rack"), (dict(task="poses"), ValueError, b"body_contacts")):
        other = RexBatchEnv(5, **{"task": "walk", "signal_type": "ik", "seed": 5, **kw})
        other.reset()
        state = other.state.clone()
        with pytest.raises(error):
            other.contact_solve()
        buf5 = torch.zeros(5 * 18, device=other.device)
        o5 = _lib.RexContactSolveOut(v_next=buf5.data_ptr())
        assert other._L.rex_contact_solve(other._h, None, 5, ctypes.byref(inp), ctypes.byref(o5), other._stream_ptr()) == -1 and msg in other._L.rex_last_error()
        torch.cuda.synchronize()
        assert bool((buf5 == 0).all()) and torch.equal(bits(other.state), bits(state))
        other.close()
