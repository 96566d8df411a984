"""Per-env actuator parameters on the GPU (rex_set_motor_params / rex_set_motor_randomization / rex_get_motor_params /
rex_motor_torque_params): pinned to the reference's own MotorModel and Rex classes through tests/golden/motor_rollout_golden.npz
(tests/golden/make_motor_golden.py), plus the bit identities and the purity of the per-reset draws.
Run on the MI355X box: python -m pytest tests/test_gpu_motor_params.py -m gpu -s"""
import ctypes
import json
import os

import numpy as np
import pytest

import orclib
from helpers import product_state_to_numeric
from motor_randomizer import MotorRandomizer

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPLAY_WINDOW = 60      # as tests/test_gpu_parity.py::test_hip_path_reproduces_reference_rollouts


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need an MI355X"
    return t


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(HERE, "golden", "motor_rollout_golden.npz"))
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def parent_fx():
    return np.load(os.path.join(HERE, "golden", "motor_parent_commit_rollout.npz"))


_REPORT = []


def _say(line):
    """Measured values: printed, and collected for the report the module writes when REX_MOTOR_REPORT names a file -- the parity
    section of profiles/motor_params.md is that file (REX_MOTOR_REPORT=... python -m pytest tests/test_gpu_motor_params.py -m gpu)."""
    print(line)
    _REPORT.append(line)


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("REX_MOTOR_REPORT")
    if path and _REPORT:
        with open(path, "w") as f:
            f.write("\n".join(_REPORT) + "\n")


def _dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _family(meta, name):
    return next(f for f in meta["families"] if f["name"] == name)


def _env_kwargs(fam):
    kw = dict(fam["env_kwargs"])
    signal = kw.pop("signal_type")
    task = {"RexWalkEnv": "walk", "RexReactiveEnv": "gallop"}[fam["env_class"]]
    return task, signal, kw


def _install(env, scenarios):
    """column k of the parameter table = scenario k's actuator"""
    p = env.set_motor_params()
    host = np.zeros((4 + env.num_motors, len(scenarios)), np.float32)
    for k, sc in enumerate(scenarios):
        q = sc["params"]
        host[0, k], host[1, k], host[2, k], host[3, k] = q["voltage"], q["damping"], q["kp"], q["kd"]
        host[4:, k] = q["strength"]
    p.copy_(env._torch.as_tensor(host, device=env.device))
    return host


# ------------------------------------------------------------------ controller
def test_motor_torque_params_kernel_vs_reference(torch, fx):
    """rex_motor_torque_params against MotorModel.convert_to_torque with the setters applied (voltage 20-36 V, damping 0-0.1,
    strength 0.5-1.3, kp 0.5-1.5, kd 0-0.05).  The bound is test_motor_kernel_vs_reference_golden's (atol 2e-5, rtol 1e-5: fp32
    against fp64 on a 3.5 / 5.7 N m full scale) times the largest strength ratio of the block -- the ratio multiplies the torque
    and its rounding error alike."""
    from rex_gym_amd import _lib
    z, _ = fx
    cmd, q, qd, qdt = (_dev(torch, z[k]) for k in ("ctl_cmd", "ctl_q", "ctl_qd", "ctl_qd_true"))
    par = _dev(torch, z["ctl_par"])
    n = cmd.numel()
    assert n >= 1000 and par.shape == (n, 5)
    act, obs = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    _lib.check(_lib.lib().rex_motor_torque_params(n, cmd.data_ptr(), q.data_ptr(), qd.data_ptr(), qdt.data_ptr(), par.data_ptr(),
                                                  act.data_ptr(), obs.data_ptr(), None), "rex_motor_torque_params")
    torch.cuda.synchronize()
    smax = float(z["ctl_par"][:, 4].max())
    assert 1.0 < smax <= 1.3
    ea, eo = np.abs(act.cpu().numpy() - z["ctl_actual"]), np.abs(obs.cpu().numpy() - z["ctl_observed"])
    _say("controller (%d problems): max |actual torque error| %.2e N m, max |observed torque error| %.2e N m, largest strength ratio %.3f "
         "(bound 2e-5 x %.3f)\n" % (n, ea.max(), eo.max(), smax, smax))
    # the block exercises the knobs: saturated and unsaturated PWM, both clips of the net voltage side
    assert (np.abs(z["ctl_actual"]) > 3.0).any() and (np.abs(z["ctl_actual"]) < 0.5).any()
    np.testing.assert_allclose(act.cpu().numpy(), z["ctl_actual"], atol=2e-5 * smax, rtol=1e-5 * smax)
    np.testing.assert_allclose(obs.cpu().numpy(), z["ctl_observed"], atol=2e-5 * smax, rtol=1e-5 * smax)


# ------------------------------------------------------------------ rollouts against the reference's classes
def _replay(torch, env, z, scenarios, nm, step, reset):
    """Replays env k against scenario k; returns per scenario the worst errors over the window, done compared exactly."""
    n = len(scenarios)
    ref = {k: np.stack([z[f"{sc['key']}/{k}"] for sc in scenarios]) for k in ("reset_obs", "action", "obs", "reward", "done", "cmd", "body")}
    assert all(np.array_equal(ref["action"][0], ref["action"][k]) for k in range(n)), "one action tape per family"
    worst = {k: np.zeros(n) for k in ("obs", "rate", "reward", "cmd", "q")}
    obs0 = reset()
    e = np.abs(obs0 - ref["reset_obs"])
    worst["obs"] = np.maximum(worst["obs"], np.delete(e, [2, 3], axis=1).max(axis=1)); worst["rate"] = np.maximum(worst["rate"], e[:, 2:4].max(axis=1))
    steps = min(ref["action"].shape[1], REPLAY_WINDOW)
    for t in range(steps):
        o, r, d, cmd, q = step(ref["action"][:, t].astype(np.float32))
        assert np.array_equal(d.astype(bool), ref["done"][:, t].astype(bool)), f"step {t}: done"
        e = np.abs(o - ref["obs"][:, t])
        worst["obs"] = np.maximum(worst["obs"], np.delete(e, [2, 3], axis=1).max(axis=1))
        worst["rate"] = np.maximum(worst["rate"], e[:, 2:4].max(axis=1))
        worst["reward"] = np.maximum(worst["reward"], np.abs(r - ref["reward"][:, t]))
        worst["cmd"] = np.maximum(worst["cmd"], np.abs(cmd - ref["cmd"][:, t]).max(axis=1))
        worst["q"] = np.maximum(worst["q"], np.abs(q - ref["body"][:, t, 13:13 + nm]).max(axis=1))
    return worst


def _check_bounds(label, scenarios, worst, arm):
    """Bounds of test_hip_path_reproduces_reference_rollouts: cmd 2e-5, obs and joint angles 2e-3, rates 5e-2 (0.25 for the arm),
    reward 2e-3.  A randomised scenario's angle bounds (obs, q) may instead be 2 x the worst error of the NOMINAL scenario of the
    same family in the same run (the same fp32 round-off mechanism), capped at one fifth of the separation stored in the fixture."""
    base = dict(cmd=2e-5, obs=2e-3, q=2e-3, rate=0.25 if arm else 5e-2, reward=2e-3)
    nom = next(k for k, sc in enumerate(scenarios) if sc["nominal"])
    failures = []
    _say(f"{label}\n\n| scenario | cmd | obs (angles) | joint angles | rates | reward | separation from nominal [rad] |\n|---|---|---|---|---|---|---|")
    for k, sc in enumerate(scenarios):
        bound = dict(base)
        if not sc["nominal"]:
            for key in ("obs", "q"):
                bound[key] = max(base[key], min(2.0 * worst[key][nom], sc["separation"] / 5.0))
        _say("| %s | %s | %.2e |" % (sc["name"], " | ".join("%.2e (< %.0e)" % (worst[key][k], bound[key]) for key in ("cmd", "obs", "q", "rate", "reward")),
                                 sc["separation"]))
        failures += [(sc["name"], key, worst[key][k], bound[key]) for key in bound if not worst[key][k] < bound[key]]
    _say("")
    assert not failures, failures


@pytest.mark.parametrize("family,epw", [("walk_ik", 4), ("walk_ik", 16), ("walk_ik", 64), ("gallop_ol", 4), ("gallop_ol", 16), ("gallop_ol", 64),
                                        ("walk_ik_arm", 4), ("walk_ik_arm", 16)])
def test_heterogeneous_batch_reproduces_reference_rollouts(torch, fx, monkeypatch, family, epw):
    """ONE batch per family whose env k carries scenario k's actuator through set_motor_params (the nominal scenario included:
    n = 6, 7 and 2, ragged on purpose), replayed against what the reference's own env / Rex / MotorModel classes produced for
    that scenario (tests/golden/make_motor_golden.py), at every envs-per-wave variant."""
    from rex_gym_amd import RexBatchEnv
    z, meta = fx
    fam = _family(meta, family)
    scs, nm = fam["scenarios"], fam["num_motors"]
    task, signal, kw = _env_kwargs(fam)
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    env = RexBatchEnv(len(scs), task=task, signal_type=signal, **kw)
    assert env._L.rex_envs_per_wave(env._h) == epw and env.num_motors == nm
    host = _install(env, scs)
    np.testing.assert_array_equal(env.motor_params().cpu().numpy(), host)

    def step(a):
        o, r, d, info = env.step(torch.as_tensor(a, device="cuda"))
        ps = product_state_to_numeric(env.state)
        return o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), info["action"].cpu().numpy(), ps[orclib.S_Q:orclib.S_Q + nm].T   # (Q = 13 for both marks: 13 + num_motors words)

    worst = _replay(torch, env, z, scs, nm, step, lambda: env.reset().cpu().numpy())
    _check_bounds(f"{family} epw {epw}", scs, worst, arm=nm == 18)
    env.close()


def test_reference_style_randomizer_through_the_motor_model(torch, fx):
    """The randomizer class that drove the reference's RexWalkEnv in the fixture's generator (tests/motor_randomizer.py: it acts
    through env.rex._motor_model and env.rex._kp / _kd), passed unchanged as env_randomizer= to this project's RexWalkEnv,
    reproduces the walk_ik all-at-once scenario."""
    from rex_gym_amd.envs.gym.walk_env import RexWalkEnv
    z, meta = fx
    fam = _family(meta, "walk_ik")
    sc = next(s for s in fam["scenarios"] if s["name"] == "all")
    nominal = next(s for s in fam["scenarios"] if s["nominal"])
    p = sc["params"]
    rnd = MotorRandomizer(strength=p["strength"], voltage=p["voltage"], damping=p["damping"], kp=p["kp"], kd=p["kd"])
    env = RexWalkEnv(env_randomizer=rnd, **fam["env_kwargs"])
    assert env.rex._motor_model.get_voltage() == pytest.approx(32.0) and env.rex._motor_model.get_viscous_dampling() == 0.0

    def step(a):
        o, r, d, info = env.step(a[0])
        ps = product_state_to_numeric(env._batch.state)
        return o[None], np.array([r]), np.array([d]), info["action"][None], ps[orclib.S_Q:orclib.S_Q + 12].T

    worst = _replay(torch, env, z, [sc], 12, step, lambda: env.reset()[None])
    assert env.rex._motor_model.get_voltage() == pytest.approx(p["voltage"]) and env.rex._kp == pytest.approx(p["kp"])
    # (no nominal env in this run: the base bounds alone)
    base = dict(cmd=2e-5, obs=2e-3, q=2e-3, rate=5e-2, reward=2e-3)
    _say("randomizer surface (tests/motor_randomizer.py through env.rex._motor_model on RexWalkEnv, walk_ik all-at-once): "
         + ", ".join("%s %.2e" % (k, float(worst[k][0])) for k in ("cmd", "obs", "q", "rate", "reward")) + "; separation %.2e rad\n" % sc["separation"])
    assert nominal["nominal"]
    assert all(worst[k][0] < base[k] for k in base), worst
    env.close()


# ------------------------------------------------------------------ bit identities
def _run(torch, env, acts, prepare=None):
    """reset + single steps: (reset obs, obs [T, N, O], reward [T, N], done [T, N], final state)"""
    obs0 = env.reset().cpu().numpy().copy()
    if prepare is not None:
        prepare(env)
    o_, r_, d_ = [], [], []
    for a in acts:
        o, r, d, _ = env.step(a)
        o_.append(o.cpu().numpy().copy()); r_.append(r.cpu().numpy().copy()); d_.append(d.cpu().numpy().copy())
    return obs0, np.stack(o_), np.stack(r_), np.stack(d_), env.state.cpu().numpy().copy()


def _acts(torch, env, steps, seed=3):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    lo, hi = float(np.abs(env.action_space.low).min()), float(np.abs(env.action_space.high).min())
    b = min(lo, hi)
    return [(torch.rand((env.num_envs, env.action_dim), device="cuda", generator=g) * 2 - 1) * b for _ in range(steps)]


def _random_params(n, nm, seed=11):
    rng = np.random.RandomState(seed)
    return np.concatenate([rng.uniform(24, 34, (1, n)), rng.uniform(0, 0.05, (1, n)), rng.uniform(0.7, 1.3, (1, n)), rng.uniform(0.01, 0.04, (1, n)),
                           rng.uniform(0.6, 1.2, (nm, n))]).astype(np.float32)


N_ID, T_ID = 24, 10
KW_ID = dict(task="walk", signal_type="ik", seed=5)


def test_nominal_explicit_parameters_are_no_parameters(torch):
    from rex_gym_amd import RexBatchEnv
    a = RexBatchEnv(N_ID, **KW_ID)
    acts = _acts(torch, a, T_ID)
    ra = _run(torch, a, acts)
    b = RexBatchEnv(N_ID, **KW_ID)
    p = b.set_motor_params()
    assert p.shape == (16, N_ID) and p[:4, 0].tolist() == [32.0, 0.0, 1.0, pytest.approx(0.02)] and bool((p[4:] == 1).all())
    rb = _run(torch, b, acts)
    for x, y in zip(ra, rb):
        assert x.tobytes() == y.tobytes()
    # ... and the parameters are not ignored: a weaker battery changes the rollout; NULL restores the nominal motor
    b.set_motor_params(voltage=24.0)
    rc = _run(torch, b, acts)
    assert rc[1].tobytes() != ra[1].tobytes()
    from rex_gym_amd import _lib
    _lib.check(b._L.rex_set_motor_params(b._h, None), "rex_set_motor_params")
    b.state.zero_()
    a2 = RexBatchEnv(N_ID, **KW_ID)
    rd, re_ = _run(torch, b, acts), _run(torch, a2, acts)
    for x, y in zip(rd[:4], re_[:4]):
        assert x.tobytes() == y.tobytes()
    for e in (a, b, a2):
        e.close()


def test_gain_rows_equal_a_sim_built_with_those_gains(torch):
    """kp / kd rows (0.8, 0.03) on a default sim against a sim built with motor_kp=0.8, motor_kd=0.03 and no parameters.  The reset
    motion is the config's (the nominal robot's), so both start the steps from the second sim's reset state."""
    from rex_gym_amd import RexBatchEnv
    b = RexBatchEnv(N_ID, motor_kp=0.8, motor_kd=0.03, **KW_ID)
    acts = _acts(torch, b, T_ID)
    start = []
    rb = _run(torch, b, acts, prepare=lambda env: start.append(env.state.clone()))
    a = RexBatchEnv(N_ID, **KW_ID)
    a.set_motor_params(kp=0.8, kd=0.03)
    ra = _run(torch, a, acts, prepare=lambda env: env.state.copy_(start[0]))
    assert ra[0].tobytes() != rb[0].tobytes()       # (the two reset motions differ: the gains of the config drive them)
    for x, y in zip(ra[1:], rb[1:]):
        assert x.tobytes() == y.tobytes()
    a.close(); b.close()


def test_heterogeneous_env_equals_uniform_batch_and_segment_equals_steps(torch):
    from rex_gym_amd import RexBatchEnv
    par = _random_params(N_ID, 12)
    het = RexBatchEnv(N_ID, **KW_ID)
    het.set_motor_params().copy_(torch.as_tensor(par, device="cuda"))
    acts = _acts(torch, het, T_ID)
    rh = _run(torch, het, acts)
    assert np.isfinite(rh[1]).all()
    for i in (0, 7, 23):
        uni = RexBatchEnv(N_ID, **KW_ID)
        uni.set_motor_params().copy_(torch.as_tensor(np.repeat(par[:, i:i + 1], N_ID, axis=1), device="cuda"))
        ru = _run(torch, uni, acts)
        assert ru[0][i].tobytes() == rh[0][i].tobytes()
        for x, y in zip(ru[1:4], rh[1:4]):
            assert np.ascontiguousarray(x[:, i]).tobytes() == np.ascontiguousarray(y[:, i]).tobytes(), i
        assert np.ascontiguousarray(ru[4][:, i]).tobytes() == np.ascontiguousarray(rh[4][:, i]).tobytes(), i
        uni.close()
    # step_segment with parameters == single steps
    seg = RexBatchEnv(N_ID, **KW_ID)
    seg.set_motor_params().copy_(torch.as_tensor(par, device="cuda"))
    seg.reset()
    o, r, d, _ = seg.step_segment(torch.stack(acts))
    assert o.cpu().numpy().tobytes() == rh[1].tobytes() and r.cpu().numpy().tobytes() == rh[2].tobytes()
    assert d.cpu().numpy().tobytes() == rh[3].tobytes() and seg.state.cpu().numpy().tobytes() == rh[4].tobytes()
    het.close(); seg.close()


def test_walk_and_gallop_inside_a_mixed_batch_equal_the_single_task_sims(torch):
    from rex_gym_amd import RexBatchEnv, RexMixedBatchEnv
    par = _random_params(N_ID, 12, seed=12)
    mix = RexMixedBatchEnv(N_ID, tasks=(("walk", "ik"), ("gallop", "ik")), seed=5)
    mix.set_motor_params().copy_(torch.as_tensor(par, device="cuda"))
    ids = mix.task_ids().cpu().numpy()
    assert set(ids) == {0, 1}
    acts = _acts(torch, mix, T_ID)
    rm = _run(torch, mix, acts)
    for tid, name in ((0, "walk"), (1, "gallop")):
        one = RexBatchEnv(N_ID, task=name, signal_type="ik", seed=5)
        one.set_motor_params().copy_(torch.as_tensor(par, device="cuda"))
        ro = _run(torch, one, acts)
        sel = ids == tid
        w = one.obs_dim
        assert np.ascontiguousarray(ro[0][sel]).tobytes() == np.ascontiguousarray(rm[0][sel][:, :w]).tobytes()
        assert np.ascontiguousarray(ro[1][:, sel]).tobytes() == np.ascontiguousarray(rm[1][:, sel][:, :, :w]).tobytes(), name
        assert np.ascontiguousarray(ro[2][:, sel]).tobytes() == np.ascontiguousarray(rm[2][:, sel]).tobytes(), name
        assert np.ascontiguousarray(ro[3][:, sel]).tobytes() == np.ascontiguousarray(rm[3][:, sel]).tobytes(), name
        one.close()
    mix.close()


@pytest.mark.parametrize("mark,epw", [("base", 4), ("base", 8), ("arm", 4)])
def test_body_contact_variant_reads_the_parameters(torch, monkeypatch, mark, epw):
    """The link-box contact kernels (body_contacts): nominal explicit parameters == no parameters bit for bit, env i of a heterogeneous
    batch == env i of a uniform batch, and a segment == single steps."""
    from rex_gym_amd import RexBatchEnv
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    n, nm = 12, 18 if mark == "arm" else 12
    kw = dict(task="walk", signal_type="ik", seed=5, body_contacts=True, mark=mark)
    a = RexBatchEnv(n, **kw)
    assert a._L.rex_envs_per_wave(a._h) == epw
    acts = _acts(torch, a, 6)
    ra = _run(torch, a, acts)
    b = RexBatchEnv(n, **kw)
    b.set_motor_params()
    rb = _run(torch, b, acts)
    for x, y in zip(ra, rb):
        assert x.tobytes() == y.tobytes()
    par = _random_params(n, nm, seed=14)
    b.set_motor_params().copy_(torch.as_tensor(par, device="cuda"))
    b.state.zero_()
    rh = _run(torch, b, acts)
    assert rh[1].tobytes() != ra[1].tobytes()
    uni = RexBatchEnv(n, **kw)
    uni.set_motor_params().copy_(torch.as_tensor(np.repeat(par[:, 5:6], n, axis=1), device="cuda"))
    ru = _run(torch, uni, acts)
    for x, y in zip(ru[1:4], rh[1:4]):
        assert np.ascontiguousarray(x[:, 5]).tobytes() == np.ascontiguousarray(y[:, 5]).tobytes()
    uni.set_motor_params().copy_(torch.as_tensor(par, device="cuda"))
    uni.state.zero_(); uni.reset()
    o, r, d, _ = uni.step_segment(torch.stack(acts))
    assert o.cpu().numpy().tobytes() == rh[1].tobytes() and r.cpu().numpy().tobytes() == rh[2].tobytes() and uni.state.cpu().numpy().tobytes() == rh[4].tobytes()
    for e in (a, b, uni):
        e.close()


@pytest.mark.parametrize("kind,mark,epw", [("forward", "base", 4), ("forward", "arm", 16), ("recurrent", "base", 8), ("recurrent", "arm", 4)])
def test_fused_actor_launches_carry_the_parameters(torch, monkeypatch, kind, mark, epw):
    """The closed-loop launches (rex_step_segment_policy with the forward and with the recurrent actor) read the same parameters as
    the open-loop ones: a twin env with the same table and per-reset ranges, fed the actions the policy took through plain step(),
    returns the same bits -- through in-launch resets --, and the parameters are not ignored (a twin without them differs)."""
    import test_gpu_policy as tp
    import test_gpu_policy_recurrent as tr
    from rex_gym_amd import RexBatchEnv
    n, T = 40, 14
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    nm = 18 if mark == "arm" else 12
    par = _random_params(n, nm, seed=13)
    mk = lambda **kw: RexBatchEnv(n, task="walk", signal_type="ik", mark=mark, seed=17, auto_reset=True, max_episode_steps=6, check_actions=False,
                                  range_normalize=True, **kw)
    envs = [mk(battery_voltage_range=(24.0, 34.0)), mk(battery_voltage_range=(24.0, 34.0)), mk()]
    pol, twin, plain = envs
    assert pol._L.rex_envs_per_wave(pol._h) == epw
    for e in (pol, twin):
        e.set_motor_params().copy_(torch.as_tensor(par, device="cuda"))
    actor = (tp._actor(torch, pol, big=True) if kind == "forward" else tr._actor(torch, pol))
    obs = pol.reset(); twin.reset(); plain.reset()
    o, r, d, info = pol.step_segment_policy(T, obs)
    differs = False
    for t in range(T):
        to, tr_, td, _ = twin.step(info["policy_action"][t])
        assert torch.equal(to, o[t]) and torch.equal(tr_, r[t]) and torch.equal(td, d[t]), (kind, mark, epw, t)
        po, _, _, _ = plain.step(info["policy_action"][t])
        differs |= not torch.equal(po, o[t])
    assert torch.equal(pol.state, twin.state) and differs and int(d.sum()) >= 2 * n
    del actor
    for e in envs:
        e.close()


def test_parameters_toggled_after_a_policy_launch(torch):
    """One sim launches the plain AND the parameter-reading instantiation of the forward fused actor (whose weights sit in dynamic LDS:
    the limit is raised per kernel function): policy launch without parameters, then with a table, then with the table removed again.
    Every phase equals a twin that is fed the recorded actions through plain step()."""
    import test_gpu_policy as tp
    from rex_gym_amd import RexBatchEnv, _lib
    n, T = 40, 5
    par = _random_params(n, 12, seed=15)
    mk = lambda: RexBatchEnv(n, task="walk", signal_type="ik", seed=17, auto_reset=True, max_episode_steps=6, check_actions=False, range_normalize=True)
    pol, twin = mk(), mk()
    actor = tp._actor(torch, pol, big=True)
    assert pol._L.rex_envs_per_wave(pol._h) <= 8         # (the four-wave workgroups with the weights in LDS)
    obs = pol.reset(); twin.reset()
    for phase in ("off", "table", "off again", "table again"):
        for e in (pol, twin):
            if phase.startswith("table"):
                e.set_motor_params().copy_(torch.as_tensor(par, device="cuda"))
                _lib.check(e._L.rex_set_motor_params(e._h, e.motor_params_tensor.data_ptr()), "rex_set_motor_params")
            else:
                _lib.check(e._L.rex_set_motor_params(e._h, None), "rex_set_motor_params")
        o, r, d, info = pol.step_segment_policy(T, obs)
        torch.cuda.synchronize()
        for t in range(T):
            to, tr_, td, _ = twin.step(info["policy_action"][t])
            assert torch.equal(to, o[t]) and torch.equal(tr_, r[t]) and torch.equal(td, d[t]), (phase, t)
        obs = o[-1].clone()
    assert torch.equal(pol.state, twin.state)
    del actor
    pol.close(); twin.close()


def test_event_trace_and_parameters_refuse_each_other_when_set(torch):
    from rex_gym_amd import RexBatchEnv, _lib
    env = RexBatchEnv(4, task="walk", signal_type="ik")
    env.set_event_trace(True)
    with pytest.raises(_lib.RexSimError, match="event trace"):
        env.set_motor_params()
    assert env.motor_params_tensor is None
    r = _lib.RexMotorRandom(); r.strength_lo, r.strength_hi, r.strength_per_motor = 0.6, 1.2, 1
    assert env._L.rex_set_motor_randomization(env._h, ctypes.byref(r)) == -1 and b"event trace" in env._L.rex_last_error()
    env.set_event_trace(False)
    env.set_motor_params()
    with pytest.raises(_lib.RexSimError, match="event trace"):
        env.set_event_trace(True)
    env.reset(); env.step(torch.zeros((4, 2), device="cuda"))
    env.close()


# ------------------------------------------------------------------ per-reset draws
RANGES = dict(motor_strength_range=(0.6, 1.2), battery_voltage_range=(24.0, 34.0), motor_kp_range=(0.7, 1.3))   # damping and kd: not drawn
KW_DRAW = dict(task="walk", signal_type="ik", seed=9, auto_reset=True, max_episode_steps=5)
N_DRAW, T_DRAW = 16, 12


def _draw_run(torch, env, acts, rows=slice(None)):
    """reset + steps; per step (obs, reward, done, motor_params(), episode words)"""
    out = [(env.reset().cpu().numpy().copy(), None, None, env.motor_params().cpu().numpy().copy(),
            product_state_to_numeric(env.state)[orclib.S_EPISODE].copy())]
    for a in acts:
        o, r, d, _ = env.step(a[rows])
        out.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), d.cpu().numpy().copy(), env.motor_params().cpu().numpy().copy(),
                    product_state_to_numeric(env.state)[orclib.S_EPISODE].copy()))
    return out


def test_per_reset_draws_inside_the_launch(torch):
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(N_DRAW, **KW_DRAW, **RANGES)
    acts = _acts(torch, env, T_DRAW)
    run = _draw_run(torch, env, acts)
    changes = 0
    for k in range(1, len(run)):
        (p0, e0), (p1, e1) = run[k - 1][3:], run[k][3:]
        moved = (p0 != p1).any(axis=0)
        np.testing.assert_array_equal(moved, e0 != e1)       # the parameters change exactly when the episode word does
        changes += int(moved.sum())
    assert changes >= 2 * N_DRAW                              # the episode cap of 5 ended every env's episode twice in 12 steps
    for o, r, d, p, e in run:
        assert ((p[4:] >= 0.6) & (p[4:] <= 1.2)).all() and ((p[0] >= 24.0) & (p[0] <= 34.0)).all() and ((p[2] >= 0.7) & (p[2] <= 1.3)).all()
        assert (p[1] == 0.0).all() and (p[3] == np.float32(0.02)).all()          # undrawn rows stay nominal
        assert (np.ptp(p[4:], axis=0) > 0.05).all()                               # one draw per motor
    spread = np.concatenate([p[4:].ravel() for *_, p, e in run])
    assert spread.min() < 0.65 and spread.max() > 1.15                            # ... over the whole range
    # two shards reproduce the batch bit for bit
    for base in (0, 8):
        sh = RexBatchEnv(8, env_index_base=base, **KW_DRAW, **RANGES)
        rs = _draw_run(torch, sh, acts, rows=slice(base, base + 8))
        for full, part in zip(run, rs):
            for x, y in zip(full, part):
                if x is not None:
                    assert np.ascontiguousarray(x[..., base:base + 8] if x.shape[-1] == N_DRAW else x[base:base + 8]).tobytes() == y.tobytes()
        sh.close()
    # strength_per_motor = 0: one draw per env
    one = RexBatchEnv(N_DRAW, motor_strength_per_motor=False, **KW_DRAW, **RANGES)
    one.reset()
    p = one.motor_params().cpu().numpy()
    assert (p[4:] == p[4:5]).all() and np.ptp(p[4]) > 0.1
    one.close()
    # the drawn values installed explicitly, without randomisation, reproduce the first episode bit for bit
    ex = RexBatchEnv(N_DRAW, **KW_DRAW)
    ex.set_motor_params().copy_(torch.as_tensor(run[0][3], device="cuda"))
    re_ = _draw_run(torch, ex, acts[:4])
    for full, part in zip(run[:5], re_):
        for x, y in zip(full[:3], part[:3]):
            if x is not None:
                assert x.tobytes() == y.tobytes()
    ex.close(); env.close()


def test_mass_and_friction_draws_are_what_the_parent_commit_drew(torch, parent_fx):
    """A run with mass / friction ranges alone (no motor ranges) is bit-identical to the values recorded from the commit before this
    feature (tests/golden/motor_parent_commit_rollout.npz, recorded on an MI355X by tests/golden/make_motor_parent_golden.py -- the recipe is
    in that file -- with the same constructor arguments and actions):
    the code path of the motor draws, present but not asked for, leaves the body draws and the step's arithmetic alone."""
    from rex_gym_amd import RexBatchEnv
    kw = dict(task="walk", signal_type="ik", seed=9, auto_reset=True, max_episode_steps=5, mass_scale_range=(0.8, 1.2), friction_range=(0.25, 0.625))
    env = RexBatchEnv(N_DRAW, **kw)
    acts = [torch.as_tensor(a, device="cuda") for a in parent_fx["actions"]]
    obs0 = env.reset().cpu().numpy()
    assert obs0.tobytes() == parent_fx["reset_obs"].tobytes()
    for k, a in enumerate(acts):
        o, r, d, _ = env.step(a)
        assert o.cpu().numpy().tobytes() == parent_fx["obs"][k].tobytes(), k
        assert r.cpu().numpy().tobytes() == parent_fx["reward"][k].tobytes(), k
        assert d.cpu().numpy().astype(np.uint8).tobytes() == parent_fx["done"][k].astype(np.uint8).tobytes(), k
    assert env.state.cpu().numpy().tobytes() == parent_fx["state"].tobytes()
    env.close()


# ------------------------------------------------------------------ overheat protection sees the torque after the strength ratio
def test_overheat_after_strength(torch):
    """The on-rack overheat setup of test_overheat_shutdown_on_the_gpu (fixture walk_ol_on_rack_overheat: the front-left foot joint
    commanded 3 rad below its bound saturates its motor at 3.5 N m).  Env 1 carries strength 0.4 on that motor: 3.5 x 0.4 = 1.4 N m
    stays below the 2.45 N m threshold (rex.py:603 tests the torque after the strength ratio), so its motor is never switched off
    within the fixture's first episode, while the nominal env 0 of the same batch switches off on the recorded step."""
    from rex_gym_amd import RexBatchEnv
    with open(os.path.join(HERE, "golden", "rollout_golden.json")) as f:
        sc = next(s for s in json.load(f)["scenarios"] if s["name"] == "walk_ol_on_rack_overheat")
    kw = dict(sc["env_kwargs"]); kw.pop("action_bias"); signal = kw.pop("signal_type")
    env = RexBatchEnv(2, task="walk", signal_type=signal, check_actions=False, **kw)
    strength = np.ones((12, 2), np.float32); strength[2, 1] = 0.4
    env.set_motor_params(strength=strength)
    seen_off, resets = False, 0
    for k, ev in enumerate(sc["events"]):
        if ev["kind"] == "reset":
            resets += 1
            if resets == 2:
                break
            env.reset()
        else:
            env.step(torch.as_tensor(np.tile(np.asarray(ev["action"], np.float32), (2, 1)), device="cuda"))
        ps = product_state_to_numeric(env.state)
        mask = ps[orclib.S_MOTOR_EN].astype(np.int64)
        assert [bool((mask[0] >> j) & 1) for j in range(12)] == ev["motor_enabled"], (k, bin(mask[0]))    # the nominal env: the recorded step
        assert (mask[1] >> 2) & 1, k                                                                  # the weak motor: never off
        packed = ps[orclib.S_OVERHEAT:orclib.S_OVERHEAT + 6].astype(np.int64)
        if ev["kind"] == "step":                           # ... and its counter (motor 2: low half of word 1) does not run: what the nominal
            assert (int(packed[1, 1]) & 0xFFFF) == 0, k    # reset motion left in it is cleared by the first substep below the threshold
            assert (int(packed[1, 0]) & 0xFFFF) == ev["overheat"][2], k
        seen_off |= not ev["motor_enabled"][2]
    assert seen_off
    env.close()


# ------------------------------------------------------------------ argument checks
def test_argument_checks(torch):
    from rex_gym_amd import RexBatchEnv, _lib
    L = _lib.lib()
    assert L.rex_set_motor_params(None, None) == -1          # REX_EINVAL
    assert b"null sim" in L.rex_last_error()
    assert L.rex_set_motor_randomization(None, None) != 0 and b"null sim" in L.rex_last_error()
    assert L.rex_get_motor_params(None, None, None) != 0 and b"null" in L.rex_last_error()
    assert L.rex_motor_torque_params(0, None, None, None, None, None, None, None, None) != 0 and b"bad arguments" in L.rex_last_error()
    env = RexBatchEnv(4, task="walk", signal_type="ik")
    assert L.rex_get_motor_params(env._h, None, None) != 0 and b"output buffer" in L.rex_last_error()
    nan = float("nan")
    for field, lo, hi, word in (("strength", 1.2, 0.6, b"strength"), ("voltage", -1.0, 32.0, b"voltage"), ("voltage", 24.0, 0.0, b"voltage"),
                                ("damping", nan, 0.1, b"damping"), ("kp", 0.5, nan, b"kp"), ("kd", 0.0, float("inf"), b"kd")):
        r = _lib.RexMotorRandom()
        setattr(r, field + "_lo", lo); setattr(r, field + "_hi", hi)
        assert L.rex_set_motor_randomization(env._h, ctypes.byref(r)) == -1, (field, lo, hi)
        assert word in L.rex_last_error()
    r = _lib.RexMotorRandom(); r.strength_per_motor = 2
    assert L.rex_set_motor_randomization(env._h, ctypes.byref(r)) != 0 and b"strength_per_motor" in L.rex_last_error()
    ok = _lib.RexMotorRandom(); ok.strength_lo, ok.strength_hi, ok.strength_per_motor = 0.6, 1.2, 1
    assert L.rex_set_motor_randomization(env._h, ctypes.byref(ok)) == 0 and L.rex_set_motor_randomization(env._h, None) == 0
    env.close()
    for bad in (dict(motor_strength_range=(1.2, 0.6)), dict(battery_voltage_range=(-1, 32)), dict(motor_damping_range=(nan, 0.1)),
                dict(motor_kp_range=(0.5,)), dict(motor_kd_range=(0.0, float("inf")))):
        with pytest.raises(ValueError):
            RexBatchEnv(4, task="walk", signal_type="ik", **bad)
    # the keywords are allowed with auto_reset (host hooks are not)
    RexBatchEnv(4, task="walk", signal_type="ik", auto_reset=True, motor_strength_range=(0.6, 1.2)).close()
