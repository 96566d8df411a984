"""Rigid-body dynamics readout on the GPU (rex_dynamics, csrc/rex_dynamics.hip) against the float64 numpy reference of
tests/dynamics_ref.py (per-link Jacobian sums over kinematics_ref's poses and velocities; masses REX_MASS times the env's scales,
rotational inertias unscaled).

States: the mark-base scenes of kinematics_ref.SCENES, set up as tests/test_gpu_kinematics.py does (reset, 8 random steps, then the
synthetic columns written over all but the first few envs, corner cases included): 1, 5, 67 and 130 envs on the plane (a lone row, a
partial wave, a partial last workgroup), 67 on the random terrain pool, 67 on the [2, 9, 13] custom field; every env with its own
base (0.8 .. 1.2) and leg (0.7 .. 1.3) mass scale through env.set_body_params (dynamics_ref.scene_scales).

Bounds: FACTOR (4) x the larger deviation of the reference's two routes evaluated in float32 from the float64 reference, per field,
over the synthetic states of all scenes (tests/test_dynamics_host.py measures them without a GPU and holds BOUNDS to them); the
measures are dynamics_ref.errors':

    field         floor       bound      measure
    mass_matrix   8.361e-06   3.344e-05  |dM_ij| / sqrt(M_ii M_jj)
    bias          2.539e-06   1.016e-05  per block |d| / max(scale, |ref|): 10 mass; 10 mass 0.1 m; 10 (carried mass) 0.1 m per joint
    gravity       2.582e-06   1.033e-05  as bias
    toe_jacobian  6.842e-07   2.737e-06  largest component (m for the angular and joint columns)
    com           8.291e-07   3.316e-06  position m; velocity |dv| / max(1, |v|)
    momentum      1.041e-05   4.164e-05  linear / max(mass 1 m/s, |p|); angular / max(sqrt(trace M[3:6, 3:6]), |L|)
    mass          2.693e-07   1.077e-06  relative

toe_jacobian rows are compared only for the points kinematics_ref.stable_points keeps (both ground facets unchanged under a shift by
the kinematics test's toe_pos bound); at most 10 % of a scene's points may be left out (asserted; the reference alone leaves out 0).

One identity the readout is NOT held to:  v . (bias - gravity) = 0  does not hold in these coordinates -- it is the rate of the kinetic
energy at zero generalized acceleration, v^T Mdot v / 2 (tests/test_dynamics_host.py checks that against a finite difference) -- so
the GPU's value is compared with the reference's value of the same product, within exactly what the per-block bounds of bias and
gravity imply (it checks that the outputs pair with the order of v, not the reference again), and  v . gravity = 10 mass com_vel_z  is
held between the GPU's own outputs."""
import ctypes

import numpy as np
import pytest

import dynamics_ref as dr
import kinematics_ref as kr
import test_gpu_kinematics as tk
import test_gpu_render as col

pytestmark = pytest.mark.gpu

FACTOR = {"mass_matrix": 4.0, "bias": 4.0, "gravity": 4.0, "toe_jacobian": 4.0, "com": 4.0, "momentum": 4.0, "mass": 4.0}
BOUNDS = {"mass_matrix": 3.344e-05, "bias": 1.016e-05, "gravity": 1.033e-05, "toe_jacobian": 2.737e-06, "com": 3.316e-06, "momentum": 4.164e-05, "mass": 1.077e-06}
TOTAL_MASS = float(dr.MASS.sum())


def velocity_of(state, g):
    return np.concatenate([state[7:13, g], state[25:37, g]]).astype(np.float64)


def make_env(n, ground):
    env = tk.make_env("base", n, ground)
    bs, ls = dr.scene_scales(n)
    env.set_body_params(base_mass_scale=bs, leg_mass_scale=ls)
    return env


def to_numpy(dyn):
    """a Dynamics -> a dict of numpy arrays shaped as the reference's (toe_jacobian [k, 8, 3, 18])"""
    out = {}
    for name in dyn.fields:
        a = getattr(dyn, name).cpu().numpy()
        out[name] = a.reshape(a.shape[0], 8, 3, 18) if name == "toe_jacobian" else a
    return out


def scene_reference(n, ground, state, heights, mids):
    fields = kr.scene_fields(ground, heights, mids)
    episode = state[kr.episode_word(False)].view(np.int32)
    bs, ls = dr.scene_scales(n)
    _, kinds = kr.scene_states(False, n, ground, kr.scene_keep(n))
    rows = []
    for g in range(n):
        f = kr.field_of(fields, g, episode[g])
        r = dr.reference(state, g, f, (bs[g], ls[g]))
        rows.append(dict(env=g, ref=r, ok=dr.stable_points(state, g, f, r["kin"], tk.BOUNDS["toe_pos"]), kind=kinds[g], field=f))
    return rows


def check_rows(gpu, rows, what):
    """gpu: to_numpy() of rows' envs in order.  Every field against the reference at BOUNDS"""
    worst = {k: 0.0 for k in dr.FIELDS}
    points = left_out = 0
    failures = []
    for k, row in enumerate(rows):
        r, ok = row["ref"], row["ok"]
        e = dr.errors({name: gpu[name][k] for name in gpu}, r)
        for name, v in e.items():
            v = v[ok] if name == "toe_jacobian" else v
            if v.size:
                worst[name] = max(worst[name], float(np.max(v)))
                if not np.all(v <= BOUNDS[name]):
                    failures.append((name, row["env"], row["kind"], float(np.max(v))))
        points, left_out = points + 8, left_out + int((~ok).sum())
    print(what, "worst / bound:", {k: "%.2e / %.2e" % (worst[k], BOUNDS[k]) for k in gpu}, "left out %d of %d" % (left_out, points))
    assert not failures, (what, failures[:8], len(failures))
    assert left_out <= 0.1 * points, (what, left_out, points)
    return worst


@pytest.fixture(scope="module")
def scenes():
    """(n, ground) -> (env, state numpy, reference rows, full readout as numpy, the Dynamics), built once per scene"""
    import torch
    made = {}

    def get(n, ground):
        key = (n, ground)
        if key not in made:
            env = make_env(n, ground)
            state = env.state.cpu().numpy()
            heights = env.terrain_heights.cpu().numpy() if ground != "plane" else None
            mids = env.terrain_mids.cpu().numpy() if ground != "plane" else None
            rows = scene_reference(n, ground, state, heights, mids)
            dyn = env.dynamics()
            torch.cuda.synchronize()
            made[key] = (env, state, rows, to_numpy(dyn), dyn)
        return made[key]
    yield get
    for env, *_ in made.values():
        env.close()


# ---------------------------------------------------------------- a. every scene against the reference
@pytest.mark.parametrize("mark,n,ground", dr.SCENES)
def test_scene_against_the_reference(scenes, mark, n, ground):
    env, state, rows, gpu, dyn = scenes(n, ground)
    assert dyn.fields == dr.FIELDS and len(env.dof_names) == 18
    assert dyn.mass_matrix.shape == (n, 18, 18) and dyn.bias.shape == (n, 18) and dyn.gravity.shape == (n, 18) and dyn.toe_jacobian.shape == (n, 4, 2, 3, 18)
    assert dyn.com.shape == (n, 6) and dyn.momentum.shape == (n, 6) and dyn.mass.shape == (n,) and dyn.com_pos.shape == (n, 3) and dyn.com_vel.shape == (n, 3)
    assert all(str(getattr(dyn, k).dtype) == "torch.float32" and getattr(dyn, k).device == env.device for k in dr.FIELDS)
    check_rows(gpu, rows, (n, ground))
    # the scales arrived: every env's mass is its own
    bs, ls = dr.scene_scales(n)
    want = dr.MASS[0] * bs.astype(np.float64) + dr.MASS[1:].sum() * ls.astype(np.float64)
    assert np.abs(gpu["mass"] - want).max() <= BOUNDS["mass"] * want.max() and (n == 1 or gpu["mass"].std() > 0.05)


# ---------------------------------------------------------------- b. GPU against GPU on the same state
def power_slack(v, r, name):
    """how far v . x may be off for x = the GPU's bias or gravity, each of whose blocks (base force, base torque, each joint) lies within
    BOUNDS[name] max(block scale, |reference block|) of the reference r: sum over blocks of |v block| times that"""
    ref, mass = np.asarray(r[name], np.float64), float(r["mass"])
    scales = np.concatenate([[10 * mass, 10 * mass * dr.LEVER], 10 * dr.LEVER * np.asarray(r["carried"], np.float64)])
    vb = np.concatenate([[np.linalg.norm(v[0:3]), np.linalg.norm(v[3:6])], np.abs(v[6:])])
    mags = np.concatenate([[np.linalg.norm(ref[0:3]), np.linalg.norm(ref[3:6])], np.abs(ref[6:])])
    return BOUNDS[name] * float((vb * np.maximum(scales, mags)).sum())


@pytest.mark.parametrize("n,ground", [(130, "plane"), (67, "random"), (67, "custom")])
def test_structure_of_the_mass_matrix_and_the_jacobians(scenes, n, ground):
    """Bit for bit: M is symmetric (written from one value per pair), its blocks between two legs and the other legs' columns of each toe
    Jacobian are exact zeros, M[0,0] = M[1,1] = M[2,2] = mass, and the translation block of J is the identity."""
    _, _, _, gpu, _ = scenes(n, ground)
    M, J = gpu["mass_matrix"], gpu["toe_jacobian"]
    assert np.array_equal(M.view(np.uint32), M.transpose(0, 2, 1).copy().view(np.uint32))
    for a in range(4):
        for b in range(4):
            if a != b:
                assert not M[:, 6 + 3 * a:9 + 3 * a, 6 + 3 * b:9 + 3 * b].view(np.uint32).any(), (a, b)
        for p in (2 * a, 2 * a + 1):
            other = [6 + 3 * b + i for b in range(4) if b != a for i in range(3)]
            assert not J[:, p][:, :, other].copy().view(np.uint32).any(), p
            assert np.abs(J[:, p][:, :, 6 + 3 * a:9 + 3 * a]).max() > 0.01
    assert np.array_equal(J[:, :, :, 0:3], np.broadcast_to(np.eye(3, dtype=np.float32), (n, 8, 3, 3)))
    for k in range(3):
        assert np.array_equal(M[:, k, k].view(np.uint32), gpu["mass"].view(np.uint32))
    assert not M[:, 0, 1].any() and not M[:, 0, 2].any() and not M[:, 1, 2].any() and not M[:, 0, 3].any() and not M[:, 1, 4].any() and not M[:, 2, 5].any()


@pytest.mark.parametrize("n,ground", [(130, "plane"), (67, "custom")])
def test_identities_between_the_outputs_and_the_kinematics_readout(scenes, n, ground):
    """J_p v is rex_kinematics' toe_vel (both bounds); M v is the momentum: (M v)[0:3] = p, (M v)[3:6] - (com - o_0) x p = L; v . gravity =
    10 mass com_vel_z; and v . (bias - gravity) is the reference's value of that product (the module docstring says why it is not 0).
    Each within the bounds of the fields involved, the products formed in float64 from the float32 outputs."""
    import torch
    env, state, rows, gpu, _ = scenes(n, ground)
    kin = env.kinematics(fields=("toe_vel",))
    torch.cuda.synchronize()
    toe_vel = kin.toe_vel.cpu().numpy().reshape(n, 8, 3).astype(np.float64)
    for g in range(n):
        v = velocity_of(state, g)
        M, J = gpu["mass_matrix"][g].astype(np.float64), gpu["toe_jacobian"][g].astype(np.float64)
        jv = J @ v
        slack = tk.BOUNDS["toe_vel"] * np.maximum(1.0, np.linalg.norm(toe_vel[g], axis=-1)) + np.sqrt(3.0) * np.abs(v).sum() * BOUNDS["toe_jacobian"]
        assert np.all(np.linalg.norm(jv - toe_vel[g], axis=-1) <= slack), (g, rows[g]["kind"])
        # M v against the momentum: an entry of M is off by at most BOUNDS sqrt(M_ii M_jj)
        mass, com, mom = float(gpu["mass"][g]), gpu["com"][g].astype(np.float64), gpu["momentum"][g].astype(np.float64)
        sd = np.sqrt(np.diag(M))
        dmv = BOUNDS["mass_matrix"] * sd * (sd @ np.abs(v))
        p = M @ v
        lin_slack = BOUNDS["momentum"] * max(mass, np.linalg.norm(mom[0:3]))
        assert np.linalg.norm(p[0:3] - mom[0:3]) <= np.linalg.norm(dmv[0:3]) + lin_slack, (g, rows[g]["kind"])
        rc = com[0:3] - state[0:3, g].astype(np.float64)
        ang = p[3:6] - np.cross(rc, p[0:3])
        ang_slack = (np.linalg.norm(dmv[3:6]) + np.linalg.norm(rc) * (np.linalg.norm(dmv[0:3]) + lin_slack) + np.sqrt(3.0) * BOUNDS["com"] * np.linalg.norm(p[0:3])
                     + BOUNDS["momentum"] * max(np.sqrt(np.trace(M[3:6, 3:6])), np.linalg.norm(mom[3:6])))
        assert np.linalg.norm(ang - mom[3:6]) <= ang_slack, (g, rows[g]["kind"])
        # the powers: a block of bias / gravity is off by at most BOUNDS max(block scale, |ref block|) (dynamics_ref.errors), so its
        # product with that block of v by at most |v block| times that -- the bound the scene comparison implies, and no looser
        r = rows[g]["ref"]
        bias, grav = gpu["bias"][g].astype(np.float64), gpu["gravity"][g].astype(np.float64)
        grav_slack = power_slack(v, r, "gravity")
        com_slack = 10 * mass * (BOUNDS["com"] * max(1.0, np.linalg.norm(r["com"][3:6])) + BOUNDS["mass"] * abs(com[5]))
        assert abs(v @ grav - 10 * mass * com[5]) <= grav_slack + com_slack, (g, rows[g]["kind"])
        assert abs(v @ (bias - grav) - v @ (r["bias"] - r["gravity"])) <= power_slack(v, r, "bias") + grav_slack, (g, rows[g]["kind"])
        if rows[g]["kind"] == "origin":
            assert not mom.any() and not com[3:6].any()                      # every velocity 0: exact zeros


# ---------------------------------------------------------------- c. plumbing
@pytest.mark.parametrize("ids", [list(range(66, -1, -1)), [5, 66, 5, 0], [64]], ids=["reversed", "duplicate", "one"])
@pytest.mark.parametrize("ground", ["plane", "custom"])
def test_env_ids(scenes, ids, ground):
    import torch
    env, _, rows, full, _ = scenes(67, ground)
    part = env.dynamics(env_ids=ids)
    torch.cuda.synchronize()
    part = to_numpy(part)
    for name in full:
        assert part[name].shape[0] == len(ids)
        assert np.array_equal(part[name].view(np.uint32), full[name][ids].view(np.uint32)), name          # bit for bit the full call's rows
    assert not np.array_equal(full["mass_matrix"][0], full["mass_matrix"][5])


@pytest.mark.parametrize("n,ground", [(67, "custom"), (5, "plane")])
def test_field_subsets_are_the_full_calls_and_the_state_is_untouched(scenes, n, ground):
    import torch
    env, state, _, full, _ = scenes(n, ground)
    for names in [(k,) for k in dr.FIELDS] + [("gravity", "mass_matrix"), ("bias", "gravity", "com", "momentum", "mass"), ("toe_jacobian", "mass")]:
        sub = env.dynamics(fields=names)
        torch.cuda.synchronize()
        assert set(sub.fields) == set(names) and all(getattr(sub, other) is None for other in dr.FIELDS if other not in names)
        got = to_numpy(sub)
        for k in names:
            assert np.array_equal(got[k].view(np.uint32), full[k].view(np.uint32)), (names, k)
    again = env.dynamics()
    torch.cuda.synchronize()
    assert all(np.array_equal(a.view(np.uint32), full[k].view(np.uint32)) for k, a in to_numpy(again).items())
    assert np.array_equal(env.state.cpu().numpy().view(np.uint32), state.view(np.uint32))
    with pytest.raises(AttributeError):
        env.dynamics(fields=("bias",)).com_pos


def test_guard_words_and_unaligned_outputs(scenes):
    """Every output 16 floats into a larger buffer, then one float further (off every wider alignment; mass_matrix and toe_jacobian, which
    the kernel writes in 16-byte chunks, four floats further): the sentinels in front of and behind each survive, and both placements hold
    the bits of the env's own readout.  A mass_matrix or toe_jacobian off its 16 bytes is refused before any launch."""
    import torch
    from rex_gym_amd import _lib, dynamics
    n = 67
    env, _, _, full, _ = scenes(n, "plane")
    wide = ("mass_matrix", "toe_jacobian")
    for offset in (0, 1):
        bufs, ptrs, sizes, first = {}, {}, {}, {}
        for name in dynamics.FIELDS:
            size = int(np.prod(dynamics.field_shape(name, n)))
            bufs[name] = torch.full((size + 64,), -7.0, dtype=torch.float32, device=env.device)
            assert bufs[name].data_ptr() % 16 == 0
            first[name] = 16 + offset * (4 if name in wide else 1)
            ptrs[name], sizes[name] = bufs[name].data_ptr() + first[name] * 4, size
        assert env._L.rex_dynamics(env._h, None, n, ctypes.byref(_lib.RexDynamicsOut(**ptrs)), env._stream_ptr()) == 0, env._L.rex_last_error()
        torch.cuda.synchronize()
        for name in dynamics.FIELDS:
            b, lo = bufs[name].cpu().numpy(), first[name]
            assert np.all(b[:lo] == -7.0) and np.all(b[lo + sizes[name]:] == -7.0), (name, offset)
            assert np.array_equal(b[lo:lo + sizes[name]].view(np.uint32), full[name].reshape(-1).view(np.uint32)), (name, offset)
        for name in wide:
            for shift in (4, 8):
                off = dict(ptrs)
                off[name] = ptrs[name] + shift
                bufs[name].fill_(-7.0)
                assert env._L.rex_dynamics(env._h, None, n, ctypes.byref(_lib.RexDynamicsOut(**off)), env._stream_ptr()) == -1
                assert b"16-byte aligned" in env._L.rex_last_error()
                torch.cuda.synchronize()
                assert bool((bufs[name] == -7.0).all()), (name, shift)


def test_out_is_reused_refreshed_after_a_step_and_checked():
    import torch
    env = make_env(67, "plane")
    names = ("bias", "com", "mass_matrix")
    first = env.dynamics(fields=names)
    tensors = (first.mass_matrix, first.bias, first.com)
    ptrs = [t.data_ptr() for t in tensors]
    torch.cuda.synchronize()
    before = first.bias.clone()
    col._steps(env, 1, seed=3)
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated(env.device)
    for _ in range(2):
        again = env.dynamics(fields=names, out=first)
        assert again is first and (again.mass_matrix, again.bias, again.com) == tensors and [t.data_ptr() for t in tensors] == ptrs
    assert torch.cuda.memory_allocated(env.device) == allocated
    torch.cuda.synchronize()
    fresh = env.dynamics(fields=names)
    torch.cuda.synchronize()
    assert not torch.equal(first.bias, before) and all(torch.equal(getattr(first, k), getattr(fresh, k)) for k in names)
    with pytest.raises(ValueError):
        env.dynamics(out=first)                                        # other fields
    with pytest.raises(ValueError):
        env.dynamics(fields=names, env_ids=[1, 2], out=first)          # another row count
    with pytest.raises(ValueError):
        env.dynamics(out=first.bias)                                   # not a result
    part = env.dynamics(fields=names, env_ids=[1, 2])
    assert env.dynamics(fields=names, env_ids=[2, 1], out=part) is part
    env.close()


def test_bad_arguments_raise_before_any_launch(scenes):
    import torch
    from rex_gym_amd import _lib
    env, state, _, _, _ = scenes(67, "plane")
    for ids in ([67], [-1], []):
        with pytest.raises(IndexError):
            env.dynamics(env_ids=ids)
    for fields in (["toe_force"], ["bias", "nope"], []):
        with pytest.raises(ValueError):
            env.dynamics(fields=fields)
    L, buf = env._L, torch.zeros(67 * 18, dtype=torch.float32, device=env.device)
    good, empty = _lib.RexDynamicsOut(bias=buf.data_ptr()), _lib.RexDynamicsOut()
    for sim, n, out, msg in ((env._h, 0, good, b"at least one env"), (env._h, -3, good, b"at least one env"), (env._h, 68, good, b"without env ids"),
                             (env._h, 67, None, b"null pointer"), (env._h, 67, empty, b"every output pointer is null"), (None, 67, good, b"null sim"),
                             (env._h, 2 ** 31 // 432 + 1, good, b"2^31")):
        ids = torch.zeros(1, dtype=torch.int32, device=env.device) if n > 68 else None
        rc = L.rex_dynamics(sim, ids.data_ptr() if ids is not None else None, n, ctypes.byref(out) if out is not None else None, env._stream_ptr())
        assert rc == -1 and msg in L.rex_last_error(), (n, msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
    assert np.array_equal(env.state.cpu().numpy().view(np.uint32), state.view(np.uint32))


def test_mark_arm_is_refused():
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    env = RexBatchEnv(5, task="walk", signal_type="ik", mark="arm", seed=5)
    env.reset()
    with pytest.raises(NotImplementedError):
        env.dynamics()
    buf = torch.zeros(5 * 18, dtype=torch.float32, device=env.device)
    rc = env._L.rex_dynamics(env._h, None, 5, ctypes.byref(_lib.RexDynamicsOut(bias=buf.data_ptr())), env._stream_ptr())
    assert rc == -1 and b"mark arm" in env._L.rex_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 0).all())
    env.close()


def test_on_a_stream_of_its_own():
    import torch
    from rex_gym_amd import RexBatchEnv
    stream = torch.cuda.Stream()
    kw = dict(task="walk", signal_type="ik", seed=5)
    env, twin = RexBatchEnv(37, stream=stream, **kw), RexBatchEnv(37, **kw)
    for e in (env, twin):
        e.reset()
        col._steps(e, 3, seed=2)
    dyn = env.dynamics(env_ids=[36, 0, 7])
    stream.synchronize()
    want = twin.dynamics(env_ids=[36, 0, 7])
    torch.cuda.synchronize()
    for k in dr.FIELDS:
        assert torch.equal(getattr(dyn, k), getattr(want, k)), k
    env.close(); twin.close()


def test_mass_follows_the_per_reset_draws():
    """mass_scale_range with auto_reset: every env's mass lies in [0.8, 1.2] x the model's, differs between envs, and changes for an env
    that starts another episode."""
    import torch
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(37, task="walk", signal_type="ik", seed=9, auto_reset=True, mass_scale_range=(0.8, 1.2))
    env.reset()
    col._steps(env, 2, seed=1)
    mass = env.dynamics(fields=("mass",)).mass.cpu().numpy().astype(np.float64)
    assert np.all(mass >= 0.8 * TOTAL_MASS * (1 - 1e-6)) and np.all(mass <= 1.2 * TOTAL_MASS * (1 + 1e-6)) and len(set(mass.tolist())) > 30
    env.reset([3])
    after = env.dynamics(fields=("mass", "mass_matrix"))
    torch.cuda.synchronize()
    now = after.mass.cpu().numpy().astype(np.float64)
    assert now[3] != mass[3] and np.array_equal(np.delete(now, 3), np.delete(mass, 3)) and 0.8 * TOTAL_MASS * (1 - 1e-6) <= now[3] <= 1.2 * TOTAL_MASS * (1 + 1e-6)
    assert torch.equal(after.mass_matrix[:, 0, 0], after.mass)
    env.close()


def test_a_step_after_the_readout_matches_a_twin_that_never_read():
    import torch
    from rex_gym_amd import RexBatchEnv
    kw = dict(task="walk", signal_type="ik", seed=7, terrain_type="random", terrain_pool=kr.POOL)
    env, twin = RexBatchEnv(67, **kw), RexBatchEnv(67, **kw)
    for e in (env, twin):
        e.reset()
        col._steps(e, 4, seed=6)
    before = env.state.clone()
    env.dynamics()
    torch.cuda.synchronize()
    assert torch.equal(env.state.view(torch.int32), before.view(torch.int32))
    for e in (env, twin):
        col._steps(e, 2, seed=8)
    torch.cuda.synchronize()
    assert torch.equal(env.state.view(torch.int32), twin.state.view(torch.int32))
    env.close(); twin.close()
