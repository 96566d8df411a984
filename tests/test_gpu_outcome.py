"""The step's epilogue as a readout on the GPU (rex_outcome, rex_rollout_actions_outcome; RexBatchEnv.outcome and the reward, done, obs,
motor_torque fields of RexBatchEnv.rollout_actions).

1. Against env.step: 40 envs (a full workgroup of 32 rows and a partial one), action_repeat = 1, auto_reset off, states written into
   env.state before the step so that the batch holds all four forward-reward branches (and a negative x), tilts either side of r22 = 0.85
   and of the gallop roll / pitch / y limits, a turn env whose goal delay runs out in this very step beside one a step short of it, and
   steps = max_episode_steps - 1.  tau = rex_motor_torque_params' observed torque on the pre-step state and info['action'] (one substep:
   the step's last substep starts from the pre-step state).  env.outcome is fed the post-step words 0..36, the words 37..44 and that tau:
   done and obs bit for bit (the same device functions on the same inputs), reward bit for bit for turn and standup, and for walk and
   gallop |reward - step's| <= 16 x 2^-24 x (|w_dist fwd| + w_energy dt sum |tau_j qd_j| + |w_drift drift| + |w_shake shake|) -- float32
   summation in another order -- and the same bound against tests/outcome_ref.py in float64.
2. rollout_actions with the new fields, 5 envs x 7 candidates, T = 3, repeat = 2: the seven old fields are bit for bit those of the call
   without the new ones; reward[t], done[t], obs[t] are bit for bit env.outcome(trajectory[t], ctrl_trajectory[t], motor_torque[t]); at
   repeat = 1 motor_torque[t] is bit for bit rex_motor_torque_params on the pre-step row and targets[t], a row of an env with a disabled
   motor included (the observed torque is not masked).
3. Chaining: head (2 steps) then tail (1 step) through (state, ctrl) is the unsplit call in the new fields.
4. env.state is bit-identical before and after every call (asserted inside 1. - 3. and 6.).
5. The first step against the env: T = 1 at the env's own repeat from the env's state, then env.step with the same actions on the plane.
   The two kernels' physics differ at the float32 floor, so only `done` is held, for the envs whose r22 is farther than 1e-3 from 0.85
   (outcome_ref on the step's own post-state); the share left out is printed and must stay at or below 10 %.  |reward difference| is
   printed (profiles/rollout_outcome.md records it); it is not gated.
6. Refusals before any launch."""
import ctypes
import math

import numpy as np
import pytest

import contact_solve_ref as cr
import outcome_ref as oref
import test_gpu_contact_solve as tc
import test_gpu_rollout_actions as tra
from rex_gym_amd._lib import RexOutcomeOut, RexRolloutActionsOutcome            # (a tree without the calls fails here: no test of this file passes on it)

pytestmark = pytest.mark.gpu

S_PHI, S_TARGET, S_ENDTIME, S_FLAGS, S_STEPS, S_MOTOR_EN = 37, 40, 41, 43, 44, 46
N = 40
ULP = 2.0 ** -24
OLD = tra.FIELDS
NEW = ("reward", "done", "obs", "motor_torque")
bits, same = tra.bits, tra.same
# (task, signal, further keywords of RexBatchEnv)
STEP_CASES = [("walk", "ik", {}), ("walk", "ol", {}), ("gallop", "ik", {}), ("turn", "ik", {}), ("standup", "ol", {}),
              ("walk", "ik", dict(range_normalize=True)), ("walk", "ik", dict(max_episode_steps=50)), ("walk", "ik", dict(backwards=True))]
STEP_IDS = ["-".join((t, s) + tuple(sorted(kw))) for t, s, kw in STEP_CASES]
TARGET = 0.375


def quat_of(roll, pitch, yaw):
    sr, cr, sp, cp, sy, cy = (f(0.5 * a) for a in (roll, pitch, yaw) for f in (math.sin, math.cos))
    return [sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy]


def written_states(env, task, max_steps):
    """the pre-step words written over the reset state: per env a place on the forward reward's branches, a tilt, a sideways offset"""
    import torch
    n, st = env.num_envs, env.state
    xs = [0.6, 0.45, 0.02, -0.1, 0.2]                        # past the stop space, inside it, standing, behind the start, on the way (target 0.375)
    rolls = [0.0, 0.1, 0.29, 0.31, -0.31, 0.5, 0.56, 0.0]    # r22 = cos(roll) cos(pitch) = 0.85 at roll 0.5548 (pitch 0); the gallop limit 0.3
    pitches = [0.0, 0.0, 0.0, 0.2, 0.0, 0.0, 0.0, 0.49, 0.51, 0.56, 0.54]        # the gallop limit 0.5
    ys = [0.0, 0.29, 0.31, -0.1, 0.05, 0.0, 0.12]
    S = st[0:13].t().cpu().numpy().copy()
    for i in range(n):
        sign = 1.0 if (task == "walk" and env.config.backwards > 0) else -1.0
        S[i, 0] = sign * xs[i % len(xs)] if task != "turn" else 0.01 * (i % 5) - 0.02
        S[i, 1] = ys[i % len(ys)]
        roll, pitch = rolls[i % len(rolls)], pitches[i % len(pitches)]
        S[i, 2] = 0.19 + 0.12 * (abs(roll) + abs(pitch))     # clear of the plane when tilted
        S[i, 3:7] = quat_of(roll, pitch, 0.3 * (i % 3))
        S[i, 7:13] = 0.05 * np.sin(np.arange(6) + i)
    st[0:13] = tc.dev(env, S).t()
    words = st.view(torch.int32)
    words[S_FLAGS] &= ~16
    if task in ("walk", "gallop"):
        st[S_TARGET] = torch.where(torch.arange(n, device=env.device) % 2 == 0, TARGET, -TARGET)      # the step takes |target|
    if task == "turn":                                       # stay_still since step 0: the delay of 1 s = n1 steps runs out in the step from n1, not in the one from n1 - 1
        words[S_FLAGS, 0:12] |= 7
        words[S_ENDTIME, 0:12] = 0
        n1 = int(round(1.0 / (env.config.action_repeat * float(np.format_float_positional(np.float32(env.config.sim_time_step))))))
        words[S_STEPS, 0:12] = torch.as_tensor([n1, n1 - 1] * 6, device=env.device, dtype=torch.int32)
    if max_steps:
        words[S_STEPS, 0:n:4] = max_steps - 1
    torch.cuda.synchronize()


def observed_torque(env, cmd, q, qd):
    """rex_motor_torque_params' observed torque with the config's gains and the nominal motor, [rows, 12] each"""
    import torch
    from rex_gym_amd import _lib
    rows = cmd.shape[0]
    par = np.zeros((rows, 12, 5), np.float32)                # kp, kd, voltage, damping, strength per problem
    par[..., 0], par[..., 1], par[..., 2], par[..., 4] = env.config.motor_kp, env.config.motor_kd, 32.0, 1.0
    par, cmd, q, qd = tc.dev(env, par), cmd.contiguous(), q.contiguous(), qd.contiguous()
    act, obs = torch.zeros_like(cmd), torch.zeros_like(cmd)
    _lib.check(env._L.rex_motor_torque_params(12 * rows, cmd.data_ptr(), q.data_ptr(), qd.data_ptr(), qd.data_ptr(), par.data_ptr(), act.data_ptr(),
                                              obs.data_ptr(), env._stream_ptr()), "rex_motor_torque_params")
    torch.cuda.synchronize()
    return obs


# ---------------------------------------------------------------- 1. against env.step
@pytest.mark.parametrize("task,signal,kw", STEP_CASES, ids=STEP_IDS)
def test_outcome_of_the_post_step_state_is_what_the_step_returned(task, signal, kw):
    import torch
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(N, task=task, signal_type=signal, seed=3, action_repeat=1, auto_reset=False, check_actions=False, body_contacts=False,
                      **{"target_position": TARGET, "backwards": False, **kw})
    env.reset()
    written_states(env, task, kw.get("max_episode_steps", 0))
    S0 = env.state.clone()
    rng = np.random.RandomState(5)
    lo, hi = np.minimum(env.action_space.low, env.action_space.high), np.maximum(env.action_space.low, env.action_space.high)
    a = tc.dev(env, rng.uniform(lo, hi, (N, env.action_dim)))
    obs, reward, done, info = env.step(a)
    torch.cuda.synchronize()
    obs, reward, done = obs.clone(), reward.clone(), done.clone()
    S1 = env.state.clone()
    tau = observed_torque(env, info["action"], S0[13:25].t(), S0[25:37].t())
    post, ctrl = S1[0:37].t().contiguous(), S1[S_PHI:S_PHI + 8].t().contiguous()
    oc = env.outcome(post, ctrl, tau)
    torch.cuda.synchronize()
    assert torch.equal(bits(env.state), bits(S1))                                         # 4. nothing written
    assert oc.fields == ("reward", "done", "obs") and oc.reward.shape == (N,) and oc.done.dtype == torch.uint8 and oc.obs.shape == (N, env.obs_dim)
    assert bool(torch.isfinite(reward).all()) and bool(torch.isfinite(obs).all())
    # the env's own words are the default inputs; a candidate axis on the inputs comes back on the outputs
    own = env.outcome(motor_torque=tau)
    wide = env.outcome(post[:, None, :].expand(N, 2, 37).contiguous(), ctrl, tau)
    assert all(same(getattr(own, f), getattr(oc, f)) for f in oc.fields) and wide.reward.shape == (N, 2) and same(wide.obs[:, 1], oc.obs) and same(wide.done[:, 0], oc.done)
    part = env.outcome(post[[37, 3]].contiguous(), ctrl[[37, 3]].contiguous(), tau[[37, 3]].contiguous(), env_ids=[37, 3], fields=("reward",))
    assert part.fields == ("reward",) and part.done is None and same(part.reward, oc.reward[[37, 3]])
    done_b = done.view(torch.uint8) if done.dtype == torch.bool else done.to(torch.uint8)
    assert torch.equal(oc.done, done_b), (task, (oc.done != done_b).nonzero().flatten().tolist())
    assert same(oc.obs, obs), (task, float((oc.obs - obs).abs().max()))
    cfg = oref.config(env.config, task, env.obs_dim)
    P, C, Tq = post.cpu().numpy().astype(np.float64), ctrl.cpu().numpy(), tau.cpu().numpy().astype(np.float64)
    flags, steps = C.view(np.int32)[:, 6], C.view(np.int32)[:, 7]
    got, want = oc.reward.cpu().numpy().astype(np.float64), reward.cpu().numpy().astype(np.float64)
    ref_done = [oref.done(cfg, P[i], bool(flags[i] & 32), int(steps[i])) for i in range(N)]
    assert ref_done == [bool(d) for d in done_b.cpu().numpy()]
    assert 0 < sum(ref_done) < N, sum(ref_done)                                           # both sides of the thresholds are in the batch
    if task in ("turn", "standup"):
        assert same(oc.reward, reward), task
        ref = np.array([oref.reward(cfg, P[i], float(C[i, 3])) for i in range(N)])
        print(task, "largest |reward - float64 reference| %.3e" % np.abs(got - ref).max())
    else:
        scale = np.array([oref.reward_scale(cfg, P[i], float(C[i, 3]), Tq[i]) for i in range(N)])
        ref = np.array([oref.reward(cfg, P[i], float(C[i, 3]), Tq[i]) for i in range(N)])
        bound = 16 * ULP * scale
        print(task, signal, sorted(kw), "largest |reward - step's| / bound %.3f, |reward - float64 reference| / bound %.3f; energy share of the scale up to %.3f" % (
            (np.abs(got - want) / bound).max(), (np.abs(got - ref) / bound).max(), (cfg["w_energy"] * cfg["dt"] * np.abs(Tq * P[:, 25:37]).sum(1) / scale).max()))
        assert (np.abs(got - want) <= bound).all(), (task, np.abs(got - want).max())
        assert (np.abs(got - ref) <= bound).all(), (task, (np.abs(got - ref) / bound).max())
        # the four forward-reward branches were in the batch (post-step x against the target, as the reward reads them)
        x = (P[:, 0] if cfg["backwards"] else -P[:, 0])
        T = np.abs(C[:, 3].astype(np.float64))
        assert (x > T + 0.15).any() and ((T <= x) & (x <= T + 0.15)).any() and (x <= 0.05).any() and ((x > 0.05) & (x < T)).any() and (x < 0).any()
    if task == "turn":
        assert bool(flags[0] & 32) and not bool(flags[1] & 32)                             # the goal delay ran out in this step / is a step short
    if kw.get("max_episode_steps"):
        assert (steps[0:N:4] == kw["max_episode_steps"]).all() and all(ref_done[0:N:4])
    env.close()


# ---------------------------------------------------------------- the case of 2. - 4.
@pytest.fixture(scope="module")
def case():
    import torch
    c = tra.Case(5, "plane", 7, 3)
    c.env.state.view(torch.int32)[S_MOTOR_EN, 2] &= ~(1 << 4)                               # env 2 runs with motor 4 switched off
    torch.cuda.synchronize()
    c.S0 = c.env.state.clone()
    yield c
    c.env.close()


def inputs(c, given):
    return dict(init_state=c.init, ctrl=c.ctrl, base_wrench=c.wr, body=c.body) if given else {}


@pytest.mark.parametrize("given", [True, False], ids=["inputs-given", "env-state"])
def test_rollout_actions_with_the_outcome_fields(case, given):
    import torch
    c, env = case, case.env
    ids = [3, 0, 4, 1, 2] if given else None
    kw = dict(inputs(c, given), env_ids=ids, **tra.KW)
    old = env.rollout_actions(c.actions, **kw)
    new = env.rollout_actions(c.actions, fields=OLD + NEW, **kw)
    torch.cuda.synchronize()
    assert old.fields == OLD and len(old) == 7 and new.fields == OLD + NEW and len(new) == 7 and isinstance(new, type(old))
    assert not tra.differing(old, new)
    T, k, K = c.T, c.n, c.K
    assert new.reward.shape == (T, k, K) and new.done.shape == (T, k, K) and new.done.dtype == torch.uint8 and new.obs.shape == (T, k, K, env.obs_dim)
    assert new.motor_torque.shape == (T, k, K, 12) and bool(torch.isfinite(new.reward).all()) and bool((new.motor_torque.abs() <= 5.7).all())
    for t in range(T):
        oc = env.outcome(new.trajectory[t], new.ctrl_trajectory[t], new.motor_torque[t], env_ids=ids)
        torch.cuda.synchronize()
        assert same(oc.reward, new.reward[t]) and same(oc.done, new.done[t]) and same(oc.obs, new.obs[t]), t
    # a subset of the new fields alone, in tensors handed back
    few = env.rollout_actions(c.actions, fields=("reward", "done"), **kw)
    few.reward.fill_(-7.0)
    again = env.rollout_actions(c.actions, fields=("reward", "done"), out=few, **kw)
    torch.cuda.synchronize()
    assert again is few and few.fields == ("reward", "done") and few.state is None and same(few.reward, new.reward) and same(few.done, new.done)
    assert c.unchanged()


def test_motor_torque_is_the_observed_torque_of_the_last_substep(case):
    import torch
    c, env = case, case.env
    kw = dict(tra.KW, repeat=1)
    ro = env.rollout_actions(c.actions, init_state=c.init, fields=("trajectory", "targets", "motor_torque"), **kw)
    torch.cuda.synchronize()
    for t in range(c.T):
        pre = (c.init if t == 0 else ro.trajectory[t - 1]).reshape(-1, 37)
        tau = observed_torque(env, ro.targets[t].reshape(-1, 12), pre[:, 13:25], pre[:, 25:37])
        assert same(tau.reshape(c.n, c.K, 12), ro.motor_torque[t]), t
    assert bool((ro.motor_torque[:, 2, :, 4] != 0).any())                                  # the disabled motor's observed torque is not masked
    assert c.unchanged()


# ---------------------------------------------------------------- 3. chaining
def test_a_rollout_continued_from_its_state_and_ctrl_is_the_unsplit_rollout_in_the_new_fields(case):
    import torch
    c, env = case, case.env
    fields = ("state", "ctrl") + NEW
    for given in (False, True):
        extra = inputs(c, given)
        part = lambda lo, hi, **over: {**{k: (v[lo:hi].contiguous() if k == "base_wrench" else v) for k, v in extra.items()}, **over}
        whole = env.rollout_actions(c.actions, fields=fields, **extra, **tra.KW)
        head = env.rollout_actions(c.actions[:2].contiguous(), fields=fields, **part(0, 2), **tra.KW)
        tail = env.rollout_actions(c.actions[2:].contiguous(), fields=fields, **part(2, c.T, init_state=head.state, ctrl=head.ctrl), **tra.KW)
        torch.cuda.synchronize()
        for f in NEW:
            assert same(getattr(head, f), getattr(whole, f)[:2]) and same(getattr(tail, f), getattr(whole, f)[2:]), (given, f)
        assert same(tail.state, whole.state) and same(tail.ctrl, whole.ctrl)
    assert c.unchanged()


# ---------------------------------------------------------------- 5. the first step against the env
def test_first_step_against_the_env():
    import torch
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(N, task="walk", signal_type="ik", seed=3, auto_reset=False, check_actions=False, target_position=TARGET, backwards=False)
    env.reset()
    written_states(env, "walk", 0)
    st = env.state                                           # tilts well away from r22 = 0.85 for all but the two rolls next to it
    S0 = st.clone()
    a = tc.dev(env, np.random.RandomState(9).uniform(-0.4, 0.4, (1, N, 1, 2)))
    ro = env.rollout_actions(a, fields=("state", "reward", "done"))
    torch.cuda.synchronize()
    assert torch.equal(bits(env.state), bits(S0))
    _, reward, done, _ = env.step(a[0, :, 0].contiguous())
    torch.cuda.synchronize()
    cfg = oref.config(env.config, "walk", env.obs_dim)
    post = env.state[0:37].t().cpu().numpy().astype(np.float64)
    far = np.array([oref.fall_margin(cfg, post[i]) > 1e-3 for i in range(N)])
    left_out = 1.0 - far.mean()
    d_step, d_roll = done.cpu().numpy().astype(bool), ro.done[0, :, 0].cpu().numpy().astype(bool)
    diff = np.abs(ro.reward[0, :, 0].cpu().numpy().astype(np.float64) - reward.cpu().numpy().astype(np.float64))
    print("first step against env.step, %d envs at the env's repeat %d: %.1f %% within 1e-3 of r22 = 0.85 left out; done differs on %d of the others; "
          "|reward difference| median %.3e, largest %.3e; %d done" % (N, env.config.action_repeat, 100 * left_out, int((d_step != d_roll)[far].sum()),
                                                                       np.median(diff), diff.max(), int(d_step.sum())))
    assert left_out <= 0.10
    assert (d_step == d_roll)[far].all()
    assert 0 < d_step.sum() < N
    env.close()


# ---------------------------------------------------------------- 6. refusals
def test_bad_arguments_and_unsupported_envs_raise_before_any_launch(case):
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    c, env = case, case.env
    n, K, T = c.n, c.K, c.T
    z = lambda *shape, **kw: torch.zeros(shape, device=env.device, **kw)
    bad = dict(state=(z(n, K, 36), z(n - 1, K, 37), z(n, K, 37, dtype=torch.float64), z(n, K, 74)[..., ::2], torch.zeros((n, K, 37)), np.zeros((n, K, 37), np.float32)),
               ctrl=(z(n, K, 7), z(n, K + 1, 8), z(n, K, 8, dtype=torch.int32), torch.zeros((n, K, 8))),
               motor_torque=(z(n, K, 11), z(n, K, 12, dtype=torch.float16), z(n, 13), torch.zeros((n, K, 12))))
    full = dict(state=z(n, K, 37), ctrl=z(n, K, 8), motor_torque=z(n, K, 12))
    for name, tensors in bad.items():
        for t in tensors:
            with pytest.raises(ValueError) as e:
                env.outcome(**{**full, name: t})
            assert str(e.value).startswith("outcome: " + name), (name, str(e.value))
    for kw in (dict(fields=()), dict(fields=("reward", "nope")), dict(out=object()), dict(env_ids=[1, 1])):
        with pytest.raises(ValueError):
            env.outcome(**kw)
    with pytest.raises(IndexError):
        env.outcome(env_ids=[0, n])
    for kw in (dict(fields=("reward", "nope")), dict(fields=("reward",), out=env.rollout_actions(c.actions, fields=("state",), **tra.KW)), dict(fields=NEW, repeat=0)):
        with pytest.raises(ValueError):
            env.rollout_actions(c.actions, **kw)
    assert c.unchanged()
    # the library's own refusals, with a sim
    L, sp = env._L, env._stream_ptr()
    buf, ws = z(T * n * K * 37), z(n * K * 102)
    p, some, empty = buf.data_ptr(), RexOutcomeOut(reward=buf.data_ptr()), RexOutcomeOut()
    for args, msg in (((n, K, None, None, None, None), b"null pointer"), ((n, K, None, None, None, ctypes.byref(empty)), b"every output pointer is null"),
                      ((n, 0, None, None, None, ctypes.byref(some)), b"candidates"), ((0, K, None, None, None, ctypes.byref(some)), b"at least one env"),
                      ((n + 1, K, None, None, None, ctypes.byref(some)), b"without env ids")):
        assert L.rex_outcome(env._h, None, *args, sp) == -1
        assert L.rex_last_error().startswith(b"rex_outcome: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    In, src, out = _lib.RexRolloutActionsIn, _lib.RexRolloutFrom(), _lib.RexRolloutActionsOut()
    good, wsb = In(c.actions.data_ptr(), None, K, T, 1, 0.0, 0, -1.0), ws.numel() * 4
    ref = lambda x: ctypes.byref(x) if x is not None else None
    for inp, o, oc, wb, msg in ((good, out, None, wsb, b"null pointer"), (good, out, RexRolloutActionsOutcome(), wsb, b"every output pointer is null"),
                                (good, out, RexRolloutActionsOutcome(reward=p), wsb - 1, b"workspace"),
                                (In(c.actions.data_ptr(), None, K, T, 4096, 0.0, 0, -1.0), out, RexRolloutActionsOutcome(reward=p), wsb, b"substeps")):
        assert L.rex_rollout_actions_outcome(env._h, None, n, ref(inp), ref(src), ref(o), ref(oc), ws.data_ptr(), wb, sp) == -1
        assert L.rex_last_error().startswith(b"rex_rollout_actions_outcome: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0).all()) and c.unchanged()
    # envs the calls do not cover: Python first, then the library itself, each naming the cause
    for kw, exc, word, both in ((dict(task="mixed"), ValueError, "mixed", True), (dict(mark="arm"), NotImplementedError, "arm", True),
                                (dict(pd_latency=0.003, control_latency=0.02), ValueError, "latency", True),
                                (dict(body_contacts=True), ValueError, "body_contacts", False), (dict(on_rack=True), ValueError, "on_rack", False)):
        e = RexBatchEnv(4, **{"task": "walk", "signal_type": "ik", **kw})
        e.reset()
        torch.cuda.synchronize()
        s0 = e.state.clone()
        acts = torch.zeros((2, 4, 1, e.action_dim), device=e.device)
        with pytest.raises(exc) as err:
            e.rollout_actions(acts, fields=("reward",))
        assert word in str(err.value)
        o4, w4 = z(4 * 37), z(4 * 102)
        assert e._L.rex_rollout_actions_outcome(e._h, None, 4, ref(In(acts.data_ptr(), None, 1, 2, 1, 0.0, 0, -1.0)), ref(src), ref(out),
                                                ref(RexRolloutActionsOutcome(reward=o4.data_ptr())), w4.data_ptr(), w4.numel() * 4, e._stream_ptr()) == -1, kw
        assert e._L.rex_last_error().startswith(b"rex_rollout_actions_outcome: ") and word.encode() in e._L.rex_last_error().lower(), e._L.rex_last_error()
        if both:
            with pytest.raises(exc) as err:
                e.outcome()
            assert word in str(err.value)
            assert e._L.rex_outcome(e._h, None, 4, 1, None, None, None, ref(RexOutcomeOut(reward=o4.data_ptr())), e._stream_ptr()) == -1, kw
            assert e._L.rex_last_error().startswith(b"rex_outcome: ")
        torch.cuda.synchronize()
        assert bool((o4 == 0).all()) and torch.equal(bits(e.state), bits(s0))
        e.close()
