"""The contact-space readout and inverse dynamics on the GPU (rex_contact_space, rex_inverse_dynamics; csrc/rex_contact_space.hip) against
the float64 numpy reference of tests/contact_space_ref.py: delassus = J solve(M, J^T), toe_acc_free = J solve(M, S^T tau + w - h) + drift,
force = M vdot + h - load, with M, h and J of dynamics_ref.reference and the drift recursion on kinematics_ref's link data.

States: the scenes of tests/test_gpu_dynamics.py, set up the same way (reset, 8 random steps, synthetic columns over all but the first few
envs, per-env mass scales): 1, 5, 67 and 130 envs on the plane (a lone row, a partial wave, a partial last workgroup), 67 on the random
terrain pool, 67 on the [2, 9, 13] custom field.  Loads: dynamics_solve_ref.loads; accelerations: contact_space_ref.accelerations.

Bounds: FACTOR (4) x the larger error of the reference's two float32 routes (the Jacobian-route M with a dense Cholesky; the composite-route
M with the block elimination) against the float64 reference over the synthetic states of all scenes -- tests/test_contact_space_host.py
measures them without a GPU and holds BOUNDS to them.  The measures are contact_space_ref.errors' and force_errors':

    kind          floor       bound       kernel's worst   measure
    delassus      6.298e-07   2.519e-06   6.34e-07         |dL_rs| / (kappa sqrt(L_rr L_ss)), kappa = cond_2(D^-1/2 M D^-1/2) of the env
    toe_drift     3.123e-06   1.249e-05   3.10e-06         per point, largest component / max(10 m/s^2, the env's largest reference component)
    toe_acc_free  1.006e-05   4.023e-05   7.83e-06         as toe_drift; with (tau, w) and with neither
    force         4.298e-05   1.719e-04   4.15e-05         per block |d| / max(scale, |ref|): 10 mass; 10 mass 0.1 m; 10 (carried mass) 0.1 m per joint

(kernel's worst: over all scenes on an MI355X, profiles/contact_space.md.)  Toe points that dynamics_ref.stable_points rejects are left out
of the point-wise comparisons -- an entry of delassus is compared when both its points are kept -- and toe forces there are zero; at least
90 % of a scene's points are compared (asserted; the reference alone rejects none).  The identities between the GPU's own outputs hold for
every point: they do not depend on which facet a point found."""
import ctypes

import numpy as np
import pytest

import contact_space_ref as cs
import dynamics_ref as dr
import dynamics_solve_ref as sr
import test_gpu_dynamics as td
import test_gpu_dynamics_solve as ts

pytestmark = pytest.mark.gpu

FACTOR = 4.0
BOUNDS = {"delassus": 2.519e-06, "toe_drift": 1.249e-05, "toe_acc_free": 4.023e-05, "force": 1.719e-04}

dev, bits = ts.dev, ts.bits


class Scene:
    """a scene's env, its state as numpy, the reference rows (dynamics_ref.reference per env, the kept toe points), its inputs with the toe
    forces zeroed at the points left out, the float64 reference of the full call and the GPU's full call"""

    def __init__(self, n, ground):
        import torch
        self.n, self.ground = n, ground
        self.env = td.make_env(n, ground)
        self.state = self.env.state.cpu().numpy()
        heights = self.env.terrain_heights.cpu().numpy() if ground != "plane" else None
        mids = self.env.terrain_mids.cpu().numpy() if ground != "plane" else None
        self.rows = td.scene_reference(n, ground, self.state, heights, mids)
        self.ok = np.array([row["ok"] for row in self.rows])
        self.inp = cs.scene_inputs(n)
        self.inp["toe"][~self.ok] = 0.0
        self.dyn = [row["ref"] for row in self.rows]
        self.ref = [cs.reference(None, g, dyn=self.dyn[g], tau=self.inp["tau"][g], wrench=self.inp["wrench"][g]) for g in range(n)]
        self.tau, self.wrench = dev(self.env, self.inp["tau"]), dev(self.env, self.inp["wrench"])
        self.toe, self.vdot = dev(self.env, self.inp["toe"].reshape(n, 4, 2, 3)), dev(self.env, self.inp["vdot"])
        self.full = self.env.contact_space(tau=self.tau, base_wrench=self.wrench)
        torch.cuda.synchronize()

    def numpy(self, res):
        return {k: getattr(res, k).cpu().numpy() for k in res.fields}

    def check(self, got, refs, what, ids=None):
        """got: numpy fields of the envs ids in order, against refs[g] at BOUNDS over the kept points"""
        ids = list(range(self.n)) if ids is None else ids
        worst, failures = {k: 0.0 for k in got}, []
        for k, g in enumerate(ids):
            ok = self.ok[g]
            e = cs.errors({name: got[name][k] for name in got}, refs[g])
            for name, v in e.items():
                v = v[cs.point_mask(ok)] if name == "delassus" else v[ok]
                if v.size:
                    worst[name] = max(worst[name], float(v.max()))
                    if not np.all(v <= BOUNDS[name]):
                        failures.append((name, g, self.rows[g]["kind"], float(v.max())))
        print(what, "worst / bound:", {k: "%.2e / %.2e" % (worst[k], BOUNDS[k]) for k in got})
        assert not failures, (what, failures[:8], len(failures))

    def check_force(self, force, want, what, ids=None):
        ids = list(range(self.n)) if ids is None else ids
        worst, failures = 0.0, []
        for k, g in enumerate(ids):
            e = float(cs.force_errors(force[k], want[k], self.dyn[g]).max())
            worst = max(worst, e)
            if not e <= BOUNDS["force"]:
                failures.append((g, self.rows[g]["kind"], e))
        print(what, "force worst / bound: %.2e / %.2e" % (worst, BOUNDS["force"]))
        assert not failures, (what, failures[:8], len(failures))

    def pick(self, combo):
        """(device keyword arguments of inverse_dynamics, per-env numpy keyword arguments of contact_space_ref.inverse) of the members in combo"""
        names = {"vdot": "vdot", "tau": "tau", "toe": "toe_forces", "wrench": "base_wrench"}
        tensors = {"vdot": self.vdot, "tau": self.tau, "toe": self.toe, "wrench": self.wrench}
        return ({names[k]: tensors[k] for k in combo}, [{k: self.inp[k][g] for k in combo} for g in range(self.n)])


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


def state_unchanged(s):
    return np.array_equal(s.env.state.cpu().numpy().view(np.uint32), s.state.view(np.uint32))


# ---------------------------------------------------------------- a. every scene against the reference
@pytest.mark.parametrize("mark,n,ground", dr.SCENES)
def test_contact_space_against_the_reference(scenes, mark, n, ground):
    import torch
    s = scenes(n, ground)
    env, full = s.env, s.full
    assert s.ok.sum() >= 0.9 * s.ok.size, (int(s.ok.sum()), s.ok.size)
    assert full.fields == cs.FIELDS and full.delassus.shape == (n, 24, 24) and full.toe_drift.shape == full.toe_acc_free.shape == (n, 4, 2, 3)
    assert all(getattr(full, k).dtype == torch.float32 and getattr(full, k).device == env.device for k in cs.FIELDS)
    s.check(s.numpy(full), s.ref, (n, ground, "tau, wrench"))
    bare = env.contact_space(fields=("toe_acc_free",))                      # neither tau nor a wrench: the acceleration of the free robot
    torch.cuda.synchronize()
    s.check(s.numpy(bare), [cs.reference(None, g, dyn=s.dyn[g]) for g in range(n)], (n, ground, "no load"))
    assert state_unchanged(s)


@pytest.mark.parametrize("mark,n,ground", dr.SCENES)
def test_inverse_dynamics_against_the_reference(scenes, mark, n, ground):
    import torch
    s = scenes(n, ground)
    env = s.env
    for combo in cs.COMBOS:
        kw, per_env = s.pick(combo)
        need = env.inverse_dynamics(**kw)
        torch.cuda.synchronize()
        assert need.shape == (n, 18) and need.dtype == torch.float32 and need.device == env.device
        want = [cs.inverse(s.dyn[g]["mass_matrix"], s.dyn[g]["bias"], s.dyn[g]["toe_jacobian"], **per_env[g]) for g in range(n)]
        s.check_force(need.cpu().numpy(), want, (n, ground, combo))
    assert state_unchanged(s)


# ---------------------------------------------------------------- b. identities between the GPU's own outputs
IDENTITY_SCENES = [(130, "plane"), (67, "custom")]


@pytest.mark.parametrize("n,ground", IDENTITY_SCENES)
def test_delassus_equals_its_transpose_bit_for_bit_and_is_positive_semidefinite(scenes, n, ground):
    """Both triangles carry the same bits.  Every entry is within BOUNDS kappa sqrt(W_rr W_ss) of an exactly positive semidefinite matrix, so
    the smallest eigenvalue is no lower than minus the Frobenius norm of that slack, BOUNDS kappa trace(W)."""
    import torch
    s = scenes(n, ground)
    W = s.full.delassus
    assert torch.equal(bits(W), bits(W.transpose(1, 2).contiguous()))
    Wn = W.cpu().numpy().astype(np.float64)
    for g in range(n):
        _, kappa = sr.conditioning(s.dyn[g]["mass_matrix"])
        assert np.all(np.diag(Wn[g]) > 0)
        assert np.linalg.eigvalsh(Wn[g]).min() >= -BOUNDS["delassus"] * kappa * np.trace(Wn[g]), g


@pytest.mark.parametrize("n,ground", IDENTITY_SCENES)
def test_delassus_agrees_with_the_three_call_route(scenes, n, ground):
    """J M^-1 J^T from env.dynamics' toe_jacobian and env.dynamics_solve with K = 24 (the product taken in float64 on the host), within the sum
    of both bounds: this call's, BOUNDS kappa sqrt(W_pp W_qq), and the solve's as tests/test_gpu_dynamics_solve.py derives it for this
    product, ts.BOUNDS[solve] kappa / lambda_min(D^-1/2 M D^-1/2) |D^-1/2 J_p| |D^-1/2 J_q|."""
    import torch
    s = scenes(n, ground)
    env = s.env
    J = env.dynamics(fields=("toe_jacobian",)).toe_jacobian.view(n, 24, 18)
    X = env.dynamics_solve(J)
    torch.cuda.synchronize()
    Jn, Xn, Wn = J.cpu().numpy().astype(np.float64), X.cpu().numpy().astype(np.float64), s.full.delassus.cpu().numpy().astype(np.float64)
    for g in range(n):
        M = s.dyn[g]["mass_matrix"]
        sd, kappa = sr.conditioning(M)
        a = np.linalg.norm(Jn[g] / sd, axis=-1)
        d = np.sqrt(np.diag(Wn[g]))
        slack = 1.001 * (BOUNDS["delassus"] * kappa * np.outer(d, d) + ts.BOUNDS["solve"] * kappa / np.linalg.eigvalsh(M / np.outer(sd, sd)).min() * np.outer(a, a))
        assert np.all(np.abs(Wn[g] - Jn[g] @ Xn[g].T) <= slack), (g, s.rows[g]["kind"])


@pytest.mark.parametrize("n,ground", IDENTITY_SCENES)
def test_the_acceleration_under_ground_forces_is_the_free_one_plus_delassus_times_the_forces(scenes, n, ground):
    """J forward_dynamics(tau, f, w) + toe_drift = toe_acc_free(tau, w) + delassus f, the products in float64 on the host.  Slack per row r:
    forward_dynamics is off by at most e = ts.BOUNDS[forward] kappa |D^1/2 vdot| in the D^1/2 norm, which moves J_r vdot by |D^-1/2 J_r| e;
    delassus f by sum_s BOUNDS[delassus] kappa sqrt(W_rr W_ss) |f_s|; toe_acc_free by BOUNDS[toe_acc_free] times its scale, twice (the
    reference it is held to sits between); toe_drift is the same bits on both sides up to one rounding of the sum."""
    import torch
    s = scenes(n, ground)
    env = s.env
    J = env.dynamics(fields=("toe_jacobian",)).toe_jacobian.view(n, 24, 18).cpu().numpy().astype(np.float64)
    vdot = env.forward_dynamics(tau=s.tau, toe_forces=s.toe, base_wrench=s.wrench).cpu().numpy().astype(np.float64)
    torch.cuda.synchronize()
    full = {k: v.astype(np.float64) for k, v in s.numpy(s.full).items()}
    f = s.inp["toe"].reshape(n, 24).astype(np.float64)
    for g in range(n):
        W, free, drift = full["delassus"][g], full["toe_acc_free"][g].reshape(24), full["toe_drift"][g].reshape(24)
        sd, kappa = sr.conditioning(s.dyn[g]["mass_matrix"])
        e = 1.001 * ts.BOUNDS["forward"] * kappa * np.linalg.norm(sd * vdot[g])
        d = np.sqrt(np.diag(W))
        acc_scale = max(cs.ACC_SCALE, np.abs(free).max())
        slack = np.linalg.norm(J[g] / sd, axis=-1) * e + BOUNDS["delassus"] * kappa * d * (d @ np.abs(f[g])) + 2.002 * BOUNDS["toe_acc_free"] * acc_scale
        assert np.all(np.abs(J[g] @ vdot[g] + drift - free - W @ f[g]) <= slack), (g, s.rows[g]["kind"])


@pytest.mark.parametrize("n,ground", IDENTITY_SCENES)
def test_inverse_dynamics_of_the_forward_acceleration_returns_the_torques(scenes, n, ground):
    """inverse_dynamics(forward_dynamics(tau, f, w), toe_forces=f, base_wrench=w) = (0, tau).  Slack per block b, in newtons and newton
    metres: vdot is off by at most e = ts.BOUNDS[forward] kappa |D^1/2 vdot| in the D^1/2 norm, which moves row i of M vdot by at most
    sqrt(M_ii) lambda_max(D^-1/2 M D^-1/2) e; the inverse call's own round-off is BOUNDS[force] times the block's scale or the magnitude of
    the terms it sums, (|M| |vdot|)_b + |h_b| + |load_b|, whichever is larger -- here they cancel to (0, tau), and round-off follows the
    terms, not their sum."""
    import torch
    s = scenes(n, ground)
    env = s.env
    vdot = env.forward_dynamics(tau=s.tau, toe_forces=s.toe, base_wrench=s.wrench)
    need = env.inverse_dynamics(vdot=vdot, toe_forces=s.toe, base_wrench=s.wrench).cpu().numpy().astype(np.float64)
    torch.cuda.synchronize()
    vd = vdot.cpu().numpy().astype(np.float64)
    blocks = lambda x: np.concatenate([[np.linalg.norm(x[0:3]), np.linalg.norm(x[3:6])], np.abs(x[6:])])
    for g in range(n):
        r = s.dyn[g]
        M = r["mass_matrix"]
        sd, kappa = sr.conditioning(M)
        lam = float(np.linalg.eigvalsh(M / np.outer(sd, sd)).max())
        e = 1.001 * ts.BOUNDS["forward"] * kappa * np.linalg.norm(sd * vd[g])
        load = sr.load_rhs(r["toe_jacobian"], None, tau=None, toe=s.inp["toe"][g], wrench=s.inp["wrench"][g])
        terms = np.abs(M) @ np.abs(vd[g]) + np.abs(r["bias"]) + np.abs(load)
        mass = float(r["mass"])
        scales = np.concatenate([[dr.G * mass, dr.G * mass * dr.LEVER], dr.G * dr.LEVER * np.asarray(r["carried"], np.float64)])
        slack = blocks(sd * lam * e) + 1.001 * BOUNDS["force"] * np.maximum(scales, blocks(terms))
        want = np.concatenate([np.zeros(6), s.inp["tau"][g].astype(np.float64)])
        assert np.all(blocks(need[g] - want) <= slack), (g, s.rows[g]["kind"], blocks(need[g] - want) / slack)


@pytest.mark.parametrize("n,ground", IDENTITY_SCENES)
def test_inverse_dynamics_of_nothing_is_the_bias(scenes, n, ground):
    import torch
    s = scenes(n, ground)
    env = s.env
    need = env.inverse_dynamics().cpu().numpy()
    bias = env.dynamics(fields=("bias",)).bias.cpu().numpy()
    torch.cuda.synchronize()
    for g in range(n):
        assert cs.force_errors(need[g], bias[g], s.dyn[g]).max() <= td.BOUNDS["bias"], g
    s.check_force(need, [s.dyn[g]["bias"] for g in range(n)], (n, ground, "nothing given"))


# ---------------------------------------------------------------- c. plumbing
def test_field_subsets_match_the_full_call_bit_for_bit(scenes):
    import torch
    s = scenes(67, "custom")
    env = s.env
    for names in (("delassus",), ("toe_drift",), ("toe_acc_free",), ("toe_acc_free", "delassus"), "toe_drift", ("toe_drift", "toe_acc_free")):
        part = env.contact_space(tau=s.tau, base_wrench=s.wrench, fields=names)
        torch.cuda.synchronize()
        want = tuple(k for k in cs.FIELDS if k in ((names,) if isinstance(names, str) else names))
        assert part.fields == want and all(getattr(part, k) is None for k in cs.FIELDS if k not in want)
        for k in want:
            assert torch.equal(bits(getattr(part, k)), bits(getattr(s.full, k))), (names, k)
    only_tau = env.contact_space(tau=s.tau, fields=("toe_acc_free", "toe_drift"))
    zero_w = env.contact_space(tau=s.tau, base_wrench=torch.zeros(6, device=env.device), fields=("toe_acc_free",))
    torch.cuda.synchronize()
    assert torch.equal(bits(only_tau.toe_acc_free), bits(zero_w.toe_acc_free)) and not torch.equal(only_tau.toe_acc_free, s.full.toe_acc_free)
    assert torch.equal(bits(only_tau.toe_drift), bits(s.full.toe_drift))
    for bad in ((), ("delassus", "toe_vel"), "mass_matrix"):
        with pytest.raises(ValueError):
            env.contact_space(fields=bad)
    assert state_unchanged(s)


@pytest.mark.parametrize("ids", [list(range(66, -1, -1)), [64], [5, 66, 0, 31]], ids=["reversed", "one", "subset"])
@pytest.mark.parametrize("ground", ["plane", "custom"])
def test_env_ids(scenes, ids, ground):
    import torch
    s = scenes(67, ground)
    env = s.env
    part = env.contact_space(tau=s.tau[ids].contiguous(), base_wrench=s.wrench[ids].contiguous(), env_ids=ids)
    full_need = env.inverse_dynamics(vdot=s.vdot, tau=s.tau, toe_forces=s.toe, base_wrench=s.wrench)
    part_need = env.inverse_dynamics(vdot=s.vdot[ids].contiguous(), tau=s.tau[ids].contiguous(), toe_forces=s.toe[ids].contiguous(),
                                     base_wrench=s.wrench[ids].contiguous(), env_ids=ids)
    torch.cuda.synchronize()
    assert part.delassus.shape == (len(ids), 24, 24) and part_need.shape == (len(ids), 18)
    for k in cs.FIELDS:
        assert torch.equal(bits(getattr(part, k)), bits(getattr(s.full, k)[ids])), k                  # bit for bit the full call's rows
    assert torch.equal(bits(part_need), bits(full_need[ids])) and not torch.equal(full_need[0], full_need[5])


def test_out_is_refilled_in_place_and_loads_without_the_row_dimension_hold_for_every_row(scenes):
    import torch
    s = scenes(67, "random")
    env, n = s.env, 67
    small = env.contact_space(tau=s.tau, fields=("delassus", "toe_acc_free"))
    ptrs = [small.delassus.data_ptr(), small.toe_acc_free.data_ptr()]
    keep = small.toe_acc_free.clone()
    small.delassus.fill_(-7.0)
    again = env.contact_space(tau=s.tau, base_wrench=s.wrench, fields=("delassus", "toe_acc_free"), out=small)
    torch.cuda.synchronize()
    assert again is small and [small.delassus.data_ptr(), small.toe_acc_free.data_ptr()] == ptrs
    assert torch.equal(bits(small.delassus), bits(s.full.delassus)) and torch.equal(bits(small.toe_acc_free), bits(s.full.toe_acc_free))
    assert not torch.equal(small.toe_acc_free, keep)
    with pytest.raises(ValueError):
        env.contact_space(fields=("delassus",), out=small)                     # other fields than the result was made with
    with pytest.raises(ValueError):
        env.contact_space(fields=("delassus", "toe_acc_free"), out=small, env_ids=[1, 2])
    one = env.contact_space(tau=s.tau[3].contiguous(), base_wrench=s.wrench[3].contiguous(), fields=("toe_acc_free",))
    rows = env.contact_space(tau=s.tau[3].expand(n, 12).contiguous(), base_wrench=s.wrench[3].expand(n, 6).contiguous(), fields=("toe_acc_free",))
    buf = torch.full((n * 18 + 64,), -7.0, device=env.device)
    need = env.inverse_dynamics(vdot=s.vdot[3].contiguous(), toe_forces=s.toe[3].contiguous(), out=buf[17:17 + n * 18].view(n, 18))     # off every wider alignment
    want = env.inverse_dynamics(vdot=s.vdot[3].expand(n, 18).contiguous(), toe_forces=s.toe[3].expand(n, 4, 2, 3).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(bits(one.toe_acc_free), bits(rows.toe_acc_free)) and torch.equal(bits(need), bits(want))
    assert need.data_ptr() == buf.data_ptr() + 17 * 4 and bool((buf[:17] == -7.0).all()) and bool((buf[17 + n * 18:] == -7.0).all())
    assert state_unchanged(s)


# ---------------------------------------------------------------- d. refusals, all before any launch
def test_bad_arguments_raise_before_any_launch(scenes):
    import torch
    from rex_gym_amd import _lib
    s = scenes(67, "plane")
    env, n = s.env, 67
    cpu = torch.device("cpu")
    for ids in ([67], [-1], []):
        for call in (lambda: env.contact_space(env_ids=ids), lambda: env.inverse_dynamics(env_ids=ids)):
            with pytest.raises(IndexError):
                call()
    bad = (dict(tau=torch.zeros((n, 11), device=env.device)), dict(base_wrench=torch.zeros((n, 6), device=cpu)),
           dict(base_wrench=torch.zeros((n, 6), dtype=torch.float64, device=env.device)), dict(base_wrench=torch.zeros((n, 12), device=env.device)[:, ::2]),
           dict(tau=torch.zeros((n - 1, 12), device=env.device)), dict(tau=np.zeros((n, 12), np.float32)))
    for kw in bad:
        with pytest.raises(ValueError):
            env.contact_space(**kw)
        with pytest.raises(ValueError):
            env.inverse_dynamics(**kw)
    for kw in (dict(vdot=torch.zeros((n, 17), device=env.device)), dict(toe_forces=torch.zeros((n, 8, 3), device=env.device)),
               dict(out=torch.zeros((n, 17), device=env.device)), dict(out=torch.zeros((n, 18), device=cpu)), dict(out=torch.zeros((n, 36), device=env.device)[:, ::2])):
        with pytest.raises(ValueError):
            env.inverse_dynamics(**kw)
    L, sp = env._L, env._stream_ptr()
    buf = torch.zeros(n * 576 + 8, dtype=torch.float32, device=env.device)
    p = buf.data_ptr()
    whole, empty, skew = _lib.RexContactSpaceOut(delassus=p, toe_drift=p, toe_acc_free=p), _lib.RexContactSpaceOut(), _lib.RexContactSpaceOut(delassus=p + 4)
    one_id = torch.zeros(1, dtype=torch.int32, device=env.device).data_ptr()
    calls = ((lambda: L.rex_contact_space(env._h, None, n, None, None, None, sp), b"null pointer"),
             (lambda: L.rex_contact_space(env._h, None, 0, None, None, ctypes.byref(whole), sp), b"at least one env"),
             (lambda: L.rex_contact_space(env._h, None, 68, None, None, ctypes.byref(whole), sp), b"without env ids"),
             (lambda: L.rex_contact_space(env._h, one_id, 2 ** 22, None, None, ctypes.byref(whole), sp), b"n * 24 * 24 must stay below 2^31"),
             (lambda: L.rex_contact_space(env._h, one_id, 2 ** 27, None, None, ctypes.byref(whole), sp), b"n * 18 must stay below 2^31"),
             (lambda: L.rex_contact_space(env._h, None, n, None, None, ctypes.byref(empty), sp), b"every output pointer is null"),
             (lambda: L.rex_contact_space(env._h, None, n, None, None, ctypes.byref(skew), sp), b"16-byte aligned"),
             (lambda: L.rex_inverse_dynamics(env._h, None, n, None, None, None, sp), b"null pointer"),
             (lambda: L.rex_inverse_dynamics(env._h, None, -3, None, None, p, sp), b"at least one env"),
             (lambda: L.rex_inverse_dynamics(env._h, None, 68, None, None, p, sp), b"without env ids"),
             (lambda: L.rex_inverse_dynamics(env._h, one_id, 2 ** 27, None, None, p, sp), b"n * 18 must stay below 2^31"))
    for call, msg in calls:
        assert call() == -1 and msg in L.rex_last_error(), (msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and state_unchanged(s)


def test_mark_arm_is_refused():
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    arm = RexBatchEnv(5, task="walk", signal_type="ik", mark="arm", seed=5)
    arm.reset()
    for call in (lambda: arm.contact_space(), lambda: arm.inverse_dynamics()):
        with pytest.raises(NotImplementedError):
            call()
    buf = torch.zeros((5, 576), device=arm.device)
    out = _lib.RexContactSpaceOut(delassus=buf.data_ptr())
    state = arm.state.clone()
    for rc in (arm._L.rex_contact_space(arm._h, None, 5, None, None, ctypes.byref(out), arm._stream_ptr()),
               arm._L.rex_inverse_dynamics(arm._h, None, 5, None, None, buf.data_ptr(), arm._stream_ptr())):
        assert rc == -1 and b"mark arm" in arm._L.rex_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and torch.equal(bits(arm.state), bits(state))
    arm.close()
