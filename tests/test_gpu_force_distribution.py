"""Force distribution on the GPU (rex_force_distribution; csrc/rex_force_distribution.hip) against the float64 numpy reference of
tests/force_distribution_ref.py, which restates the iteration step for step: at the same step count the two differ by round-off only, so no
assertion here depends on how far the iteration has converged.  ITERATIONS (300) steps, except where the default is what is tested.

States: the scenes of tests/test_gpu_contact_space.py, set up the same way (reset, 8 random steps, synthetic columns over all but the first few
envs, per-env mass scales) plus a per-env foot friction of 0.3 .. 0.9 (force_distribution_ref.scene_friction): 1, 5, 67 and 130 envs on the
plane, 67 on the random terrain pool, 67 on the [2, 9, 13] custom field.  Inputs: force_distribution_ref.scene_inputs.  Stance sets:
force_distribution_ref.STANCES -- all four legs, both trot diagonals, three legs, one leg, none, a per-env random mix, and None (the kernel's
own in-reach flags against the reference's).

Bounds: FACTOR (4) x the larger error of the reference's two float32 routes against the float64 reference at the same step count, over the
synthetic states of all scenes, every stance set, with (vdot, wrench) and with neither -- tests/test_force_distribution_host.py measures
them without a GPU and holds BOUNDS to them.  The measures are force_distribution_ref.errors':

    kind           floor       bound       kernel's worst   measure
    toe_force      1.467e-04   5.867e-04   2.12e-04         per point, largest component / (10 mass)
    tau            8.565e-05   3.426e-04   1.31e-04         per joint / (10 mass 0.1 m)
    base_residual  3.312e-05   1.325e-04   3.81e-05         per component / (10 mass), the moment / (10 mass 0.1 m)
    residual       7.123e-05   2.849e-04   9.79e-05         absolute / (10 mass)

(kernel's worst: over all scenes on an MI355X, profiles/force_distribution.md.)  The solve couples all points of an env, so an env is compared
only when dynamics_ref.stable_points keeps all eight of its toe points; at least 90 % of a scene's envs are compared (asserted; the reference
alone keeps every env).  The identities between the GPU's own outputs hold for every env."""
import ctypes

import numpy as np
import pytest

import dynamics_ref as dr
import force_distribution_ref as fr
import test_gpu_contact_space as tc
import test_gpu_dynamics as td
import test_gpu_dynamics_solve as ts

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ITERATIONS = fr.GPU_ITERATIONS
BOUNDS = {"toe_force": 5.867e-04, "tau": 3.426e-04, "base_residual": 1.325e-04, "residual": 2.849e-04}
# residual / (10 mass) at the default step count, stance "all", on the plane: the float64 reference's own residual there plus FACTOR x the
# float32 routes' deviation from it (tests/test_force_distribution_host.py derives both)
DEFAULT_RESIDUAL_BOUND = 7.866e-05

dev, bits = ts.dev, ts.bits


class Scene:
    """a scene's env, its state as numpy, dynamics_ref.reference per env, the envs whose eight toe points are all kept, its inputs and the
    GPU's full call for the stance set "mix" """

    def __init__(self, n, ground):
        import torch
        self.n, self.ground = n, ground
        self.env = td.make_env(n, ground)
        self.mu = fr.scene_friction(n)
        self.env.set_body_params(foot_friction=self.mu)
        self.state = self.env.state.cpu().numpy()
        heights = self.env.terrain_heights.cpu().numpy() if ground != "plane" else None
        mids = self.env.terrain_mids.cpu().numpy() if ground != "plane" else None
        self.rows = td.scene_reference(n, ground, self.state, heights, mids)
        self.ok = np.array([row["ok"].all() for row in self.rows])
        self.dyn = [row["ref"] for row in self.rows]
        self.inp = fr.scene_inputs(n)
        self.vdot, self.wrench = dev(self.env, self.inp["vdot"]), dev(self.env, self.inp["wrench"])
        self.mix = self.stance("mix")
        self.full = self.env.force_distribution(vdot=self.vdot, base_wrench=self.wrench, stance=self.mix, iterations=ITERATIONS)
        torch.cuda.synchronize()

    def stance(self, name):
        import torch
        st = fr.stance_of(name, self.n)
        return None if st is None else torch.as_tensor(st, device=self.env.device)

    def reference(self, name, given, iterations=ITERATIONS, ids=None):
        ids = list(range(self.n)) if ids is None else ids
        st = fr.stance_of(name, self.n)
        P = fr.problem([self.dyn[g] for g in ids], self.mu[ids], stance=None if st is None else st[ids],
                       vdot=self.inp["vdot"][ids] if given else None, wrench=self.inp["wrench"][ids] if given else None)
        return P, fr.solve(P, iterations)

    def numpy(self, res):
        return {k: getattr(res, k).cpu().numpy() for k in res.fields}

    def check(self, got, want, mass, what):
        """got: numpy fields of every env, against the reference at BOUNDS over the kept envs"""
        e = fr.errors(got, want, mass)
        worst = {k: float(v[self.ok].max()) if self.ok.any() else 0.0 for k, v in e.items()}
        print(what, "worst / bound:", {k: "%.2e / %.2e" % (worst[k], BOUNDS[k]) for k in got})
        failures = [(k, int(g), self.rows[g]["kind"], float(e[k][g].max())) for k in got for g in np.nonzero(self.ok)[0] if not np.all(e[k][g] <= BOUNDS[k])]
        assert not failures, (what, failures[:8], len(failures))


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


# ---------------------------------------------------------------- 1, 2. every scene and stance set against the reference
@pytest.mark.parametrize("stance", fr.STANCES)
@pytest.mark.parametrize("mark,n,ground", dr.SCENES)
def test_force_distribution_against_the_reference(scenes, mark, n, ground, stance):
    import torch
    s = scenes(n, ground)
    env = s.env
    assert s.ok.sum() >= 0.9 * s.n, (int(s.ok.sum()), s.n)
    assert np.array_equal(env.body_params[2].cpu().numpy(), s.mu)
    for given in (True, False):
        kw = dict(vdot=s.vdot, base_wrench=s.wrench) if given else {}
        res = env.force_distribution(stance=s.stance(stance), iterations=ITERATIONS, **kw)
        torch.cuda.synchronize()
        assert res.fields == fr.FIELDS and res.toe_force.shape == (n, 4, 2, 3) and res.tau.shape == (n, 12)
        assert res.base_residual.shape == (n, 6) and res.residual.shape == (n,)
        assert all(getattr(res, k).dtype == torch.float32 and getattr(res, k).device == env.device for k in fr.FIELDS)
        got = s.numpy(res)
        assert all(np.isfinite(v).all() for v in got.values())
        P, want = s.reference(stance, given)
        if stance == "reach":                                   # the kernel's own flags are rex_kinematics'
            reach = env.kinematics(fields=("toe_in_reach",)).toe_in_reach.cpu().numpy().reshape(n, 8) != 0
            assert np.array_equal(reach[s.ok], P["inS"][s.ok])
        if stance == "none":
            assert not got["toe_force"].any() and not got["residual"].any()
        s.check(got, want, P["mass"], (n, ground, stance, "vdot, wrench" if given else "hold still"))
    assert state_unchanged(s)


# ---------------------------------------------------------------- 3. identities between the GPU's own outputs, on every env
IDENTITY_SCENES = [(130, "plane"), (67, "custom")]


@pytest.mark.parametrize("n,ground", IDENTITY_SCENES)
def test_inverse_dynamics_of_the_returned_forces_gives_the_base_residual_and_the_torques(scenes, n, ground):
    import torch
    s = scenes(n, ground)
    env, full = s.env, s.full
    need = env.inverse_dynamics(vdot=s.vdot, toe_forces=full.toe_force, base_wrench=s.wrench).cpu().numpy()
    hold = env.force_distribution(iterations=ITERATIONS)
    need_hold = env.inverse_dynamics(toe_forces=hold.toe_force).cpu().numpy()
    torch.cuda.synchronize()
    for res, got in ((full, need), (hold, need_hold)):
        want = np.concatenate([res.base_residual.cpu().numpy(), res.tau.cpu().numpy()], -1)
        worst = max(float(tc.cs.force_errors(got[g], want[g], s.dyn[g]).max()) for g in range(n))
        print((n, ground), "inverse dynamics worst / bound: %.2e / %.2e" % (worst, tc.BOUNDS["force"]))
        assert worst <= tc.BOUNDS["force"]


@pytest.mark.parametrize("n,ground", IDENTITY_SCENES)
def test_forces_lie_in_their_cones_and_vanish_outside_the_stance_set(scenes, n, ground):
    """|t| <= mu s up to the rounding of a float32 force: 4 ulp of its magnitude.  Normals: rex_kinematics' toe_normal."""
    import torch
    s = scenes(n, ground)
    env = s.env
    nrm = env.kinematics(fields=("toe_normal",)).toe_normal.cpu().numpy().reshape(n, 8, 3).astype(np.float64)
    for name in ("mix", "all", "one", "reach"):
        res = env.force_distribution(vdot=s.vdot, base_wrench=s.wrench, stance=s.stance(name), iterations=ITERATIONS, fields=("toe_force",))
        torch.cuda.synchronize()
        f = res.toe_force.cpu().numpy().reshape(n, 8, 3).astype(np.float64)
        st = fr.stance_of(name, n)
        inS = env.kinematics(fields=("toe_in_reach",)).toe_in_reach.cpu().numpy().reshape(n, 8) != 0 if st is None else np.repeat(st != 0, 2, axis=1)
        assert not f[~inS].any(), name
        sn = (nrm * f).sum(-1)
        t = np.linalg.norm(f - sn[..., None] * nrm, axis=-1)
        assert np.all(t <= s.mu.astype(np.float64)[:, None] * sn + 4 * 2.0 ** -23 * np.linalg.norm(f, axis=-1)), name
        assert inS.any() and f.any()


def test_field_subsets_match_the_full_call_bit_for_bit(scenes):
    import torch
    s = scenes(67, "custom")
    env = s.env
    for names in (("toe_force",), ("tau",), ("base_residual",), ("residual",), "tau", ("residual", "toe_force"), ("tau", "base_residual")):
        part = env.force_distribution(vdot=s.vdot, base_wrench=s.wrench, stance=s.mix, iterations=ITERATIONS, fields=names)
        torch.cuda.synchronize()
        want = tuple(k for k in fr.FIELDS if k in ((names,) if isinstance(names, str) else names))
        assert part.fields == want and all(getattr(part, k) is None for k in fr.FIELDS if k not in want)
        for k in want:
            assert torch.equal(bits(getattr(part, k)), bits(getattr(s.full, k))), (names, k)
    for bad in ((), ("tau", "toe_vel"), "delassus"):
        with pytest.raises(ValueError):
            env.force_distribution(fields=bad)
    assert state_unchanged(s)


@pytest.mark.parametrize("ids", [list(range(66, -1, -1)), [64], [5, 66, 0, 31]], ids=["reversed", "one", "subset"])
@pytest.mark.parametrize("ground", ["plane", "custom"])
def test_env_ids(scenes, ids, ground):
    import torch
    s = scenes(67, ground)
    part = s.env.force_distribution(vdot=s.vdot[ids].contiguous(), base_wrench=s.wrench[ids].contiguous(), stance=s.mix[ids].contiguous(),
                                    iterations=ITERATIONS, env_ids=ids)
    torch.cuda.synchronize()
    assert part.toe_force.shape == (len(ids), 4, 2, 3) and part.residual.shape == (len(ids),)
    for k in fr.FIELDS:
        assert torch.equal(bits(getattr(part, k)), bits(getattr(s.full, k)[ids])), k                   # bit for bit the full call's rows
    assert not torch.equal(s.full.tau[0], s.full.tau[5])


def test_out_is_refilled_without_allocating_and_two_calls_give_the_same_bits(scenes):
    import torch
    s = scenes(67, "random")
    env = s.env
    kw = dict(vdot=s.vdot, base_wrench=s.wrench, stance=s.mix, iterations=ITERATIONS)
    small = env.force_distribution(fields=("toe_force", "residual"), **kw)
    ptrs = [small.toe_force.data_ptr(), small.residual.data_ptr()]
    small.toe_force.fill_(-7.0)
    small.residual.fill_(-7.0)
    env.force_distribution(fields=("toe_force", "residual"), out=small, **kw)          # (the first call with out= checks the result)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(env.device)
    again = env.force_distribution(fields=("toe_force", "residual"), out=small, **kw)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(env.device) == before
    assert again is small and [small.toe_force.data_ptr(), small.residual.data_ptr()] == ptrs
    assert torch.equal(bits(small.toe_force), bits(s.full.toe_force)) and torch.equal(bits(small.residual), bits(s.full.residual))
    twice = env.force_distribution(**kw)
    torch.cuda.synchronize()
    for k in fr.FIELDS:
        assert torch.equal(bits(getattr(twice, k)), bits(getattr(s.full, k))), k
    as_bool = env.force_distribution(vdot=s.vdot, base_wrench=s.wrench, stance=s.mix != 0, iterations=ITERATIONS, fields=("tau",))
    torch.cuda.synchronize()
    assert torch.equal(bits(as_bool.tau), bits(s.full.tau))
    with pytest.raises(ValueError):
        env.force_distribution(fields=("toe_force",), out=small)                      # other fields than the result was made with
    with pytest.raises(ValueError):
        env.force_distribution(fields=("toe_force", "residual"), out=small, env_ids=[1, 2])
    assert state_unchanged(s)


# ---------------------------------------------------------------- 4. the default step count
def test_the_default_step_count_brings_the_residual_below_the_derived_bound(scenes):
    import torch
    from rex_gym_amd import force_distribution
    s = scenes(130, "plane")
    for kw in (dict(vdot=s.vdot, base_wrench=s.wrench), {}):
        res = s.env.force_distribution(stance=s.stance("all"), fields=("residual",), **kw)
        torch.cuda.synchronize()
        mass = np.array([float(r["mass"]) for r in s.dyn])
        measure = res.residual.cpu().numpy().astype(np.float64) / (10.0 * mass)
        print("default %d steps: residual / (10 mass) worst %.2e, bound %.2e" % (force_distribution.ITERATIONS, measure.max(), DEFAULT_RESIDUAL_BOUND))
        assert np.all(measure <= DEFAULT_RESIDUAL_BOUND)


# ---------------------------------------------------------------- 5. refusals, all before any launch
def test_bad_arguments_raise_before_any_launch(scenes):
    import torch
    from rex_gym_amd import _lib
    s = scenes(67, "plane")
    env, n = s.env, 67
    for ids in ([67], [-1], []):
        with pytest.raises(IndexError):
            env.force_distribution(env_ids=ids)
    bad = (dict(vdot=torch.zeros((n, 17), device=env.device)), dict(base_wrench=torch.zeros((n, 6), device=torch.device("cpu"))),
           dict(stance=torch.zeros((n, 4), device=env.device)), dict(stance=torch.zeros((n, 8), dtype=torch.uint8, device=env.device)),
           dict(stance=np.zeros((n, 4), np.uint8)), dict(weights=(1, 1, 1, 1, 1, 0)), dict(weights=(1, 1, 1)), dict(eps=0.0), dict(eps=-1.0),
           dict(eps=float("nan")), dict(friction_scale=-0.5), dict(iterations=0), dict(iterations=10001), dict(iterations=2.5))
    for kw in bad:
        with pytest.raises(ValueError):
            env.force_distribution(**kw)
    L, sp = env._L, env._stream_ptr()
    buf = torch.zeros(n * 24 + 8, dtype=torch.float32, device=env.device)
    p = buf.data_ptr()
    whole, empty = _lib.RexForceDistributionOut(toe_force=p, tau=p, base_residual=p, residual=p), _lib.RexForceDistributionOut()
    par = lambda **kw: _lib.RexForceDistributionParams(**{**dict(weights=(ctypes.c_float * 6)(*fr.WEIGHTS), eps=fr.EPS, friction_scale=1.0, iterations=10), **kw})
    good = par()
    call = lambda n_, params, out: L.rex_force_distribution(env._h, None, n_, None, None, None, params, out, sp)
    calls = ((lambda: call(n, None, ctypes.byref(whole)), b"null pointer"), (lambda: call(n, ctypes.byref(good), None), b"null pointer"),
             (lambda: call(0, ctypes.byref(good), ctypes.byref(whole)), b"at least one env"),
             (lambda: call(68, ctypes.byref(good), ctypes.byref(whole)), b"without env ids"),
             (lambda: call(n, ctypes.byref(good), ctypes.byref(empty)), b"every output pointer is null"),
             (lambda: call(n, ctypes.byref(par(weights=(ctypes.c_float * 6)(1, 1, 0, 1, 1, 1))), ctypes.byref(whole)), b"weights[2]"),
             (lambda: call(n, ctypes.byref(par(eps=0.0)), ctypes.byref(whole)), b"eps 0"),
             (lambda: call(n, ctypes.byref(par(friction_scale=-1.0)), ctypes.byref(whole)), b"friction_scale"),
             (lambda: call(n, ctypes.byref(par(iterations=0)), ctypes.byref(whole)), b"iterations 0: 1 .. 10000"),
             (lambda: call(n, ctypes.byref(par(iterations=10001)), ctypes.byref(whole)), b"iterations 10001: 1 .. 10000"))
    for c, msg in calls:
        assert c() == -1 and msg in L.rex_last_error(), (msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and state_unchanged(s)


def test_mark_arm_is_refused():
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    arm = RexBatchEnv(5, task="walk", signal_type="ik", mark="arm", seed=5)
    arm.reset()
    with pytest.raises(NotImplementedError):
        arm.force_distribution()
    buf = torch.zeros((5, 24), device=arm.device)
    out = _lib.RexForceDistributionOut(toe_force=buf.data_ptr())
    par = _lib.RexForceDistributionParams((ctypes.c_float * 6)(*fr.WEIGHTS), fr.EPS, 1.0, 10)
    state = arm.state.clone()
    rc = arm._L.rex_force_distribution(arm._h, None, 5, None, None, None, ctypes.byref(par), ctypes.byref(out), arm._stream_ptr())
    assert rc == -1 and b"mark arm" in arm._L.rex_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and torch.equal(bits(arm.state), bits(state))
    arm.close()
