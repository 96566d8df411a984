"""The step's epilogue as a readout, the parts that need no GPU: tests/outcome_ref.py (the float64 reference of
tests/test_gpu_outcome.py) held to tests/golden/rollout_golden.json, which the reference's own env code produced; the C ABI's declarations
and their ctypes mirror; struct field order; the refusals the arguments alone decide and the Python argument checks.

The golden scenarios used are those of mark base without the latency model, from each step event's `body` (the words 0..36 after the
step); none is skipped -- every one of them records body, obs, reward and done.  The record holds no motor torques, so a walk or gallop
reward is held from both sides: minus the reference's non-energy terms it is <= 0 and at least -w_energy dt 5.7 sum |qd| (5.7 N m: the
motor model's clip of the observed torque, motor.py:116-119).  The record holds no controller words either: a turn env's
env_goal_reached is taken as False, which `done` equal on every event confirms.  The three scenarios recorded behind the reference's
wrapper chain (`wrap` in env_kwargs) end in ConvertTo32Bit: there the float64 value is rounded to float32 as that wrapper does before it
is compared, under the same 1e-12."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import outcome_ref as oref
from rex_gym_amd import _lib, build, outcome, rollout_actions as ra
from rex_gym_amd._lib import RexOutcomeOut, RexRolloutActionsOutcome            # (a tree without the calls fails here: no test of this file passes on it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
CSRC = os.path.join(ROOT, "rex_gym_amd", "csrc")
CALLS = ("rex_outcome", "rex_rollout_actions_outcome")
EPS = 1e-12


def strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ---------------------------------------------------------------- the reference against the reference's own record
def scenario_config(sc):
    oc = sc["oracle_config"]
    cfg = _lib.RexConfig()
    assert _lib.lib().rex_default_config(_lib.TASKS[oc["task"]], _lib.SIGNALS[oc["signal"]], 1, ctypes.byref(cfg)) == 0
    for k, v in oc.items():
        if k not in ("task", "signal"):
            setattr(cfg, k, v)
    return oref.config(cfg, oc["task"], _lib.lib().rex_obs_dim(ctypes.byref(cfg))), cfg


@pytest.fixture(scope="module")
def scenarios():
    assert os.path.exists(build.LIB_PATH), "the library is missing: build it first (rex_default_config fills the weights)"
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "rollout_golden.json")))
    picked = [sc for sc in golden["scenarios"] if not sc["oracle_config"].get("mark") and not sc["oracle_config"].get("control_latency")
              and not sc["oracle_config"].get("pd_latency")]
    assert len(picked) >= 12 and {sc["oracle_config"]["task"] for sc in picked} == {"walk", "gallop", "turn", "poses", "standup"}
    return picked


def rows(sc):
    """(body, obs, reward, done, the episode's step count after the step) of every env of every step event"""
    steps = None
    for ev in sc["events"]:
        batch = np.ndim(ev["body"]) == 2
        n = len(ev["body"]) if batch else 1
        if steps is None:
            steps = np.zeros(n, int)
        if ev["kind"] == "reset":
            idx = ev.get("indices")
            steps[list(range(n)) if idx is None else idx] = 0
            continue
        steps += 1
        for k in range(n):
            pick = (lambda v: v[k]) if batch else (lambda v: v)
            yield np.asarray(pick(ev["body"]), np.float64), np.asarray(pick(ev["obs"]), np.float64), float(pick(ev["reward"])), bool(pick(ev["done"])), int(steps[k])


def test_observation_against_the_record(scenarios):
    worst, angles = 0.0, 0
    for sc in scenarios:
        cfg, _ = scenario_config(sc)
        for body, obs, _, _, _ in rows(sc):
            got = oref.obs(cfg, body)
            if "wrap" in sc["env_kwargs"]:                                # the recorder's wrapper chain ends in ConvertTo32Bit (playground/trainer.py:47-52)
                got = got.astype(np.float32).astype(np.float64)
            assert got.shape == obs.shape == (cfg["obs_dim"],), sc["name"]
            err = float(np.abs(got - obs).max())
            worst = max(worst, err)
            angles += obs.size - 4
            assert err <= EPS, (sc["name"], err)
    print("largest |obs - record| %.3e over the scenarios; %d gallop motor angles compared" % (worst, angles))
    assert angles > 0                                                     # the gallop rows carry their MapToMinusPiToPi motor angles


def test_done_equal_on_every_event(scenarios):
    seen = {}
    for sc in scenarios:
        cfg, _ = scenario_config(sc)
        for body, _, _, done, steps in rows(sc):
            assert oref.done(cfg, body, False, steps) == done, (sc["name"], steps)
            seen[sc["name"]] = seen.get(sc["name"], 0) + int(done)
    assert seen["walk_ik_until_fallen"] == 2 and seen["walk_ik_wrapped"] >= 1 and seen["gallop_ol_wrapped"] >= 1 and seen["turn_ik_batch"] >= 1, seen


def test_rewards_against_the_record(scenarios):
    exact, bounded, widest = 0.0, 0, 0.0
    for sc in scenarios:
        cfg, c = scenario_config(sc)
        for body, _, reward, _, _ in rows(sc):
            if cfg["task"] in ("turn", "poses", "standup"):
                got = oref.reward(cfg, body, c.target_position)
                err = abs((float(np.float32(got)) if "wrap" in sc["env_kwargs"] else got) - reward)          # (ConvertTo32Bit, as for obs)
                exact = max(exact, err)
                assert err <= EPS, (sc["name"], err)
            else:
                rest = reward - oref.reward(cfg, body, c.target_position, None)         # w_energy x the energy term, which the record's torques made
                room = cfg["w_energy"] * cfg["dt"] * oref.TORQUE_CLIP * float(np.abs(body[25:37]).sum())
                assert -room - EPS <= rest <= EPS, (sc["name"], rest, room)
                bounded += 1
                widest = max(widest, -rest / room if room > 0 else 0.0)
    print("turn / poses / standup: largest |reward - record| %.3e; %d walk and gallop rewards inside the energy bound, at most %.3f of it" % (exact, bounded, widest))
    assert bounded > 0


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_two_calls_and_the_two_structs_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert set(CALLS) <= declared and declared == set(_lib.EXPORTED_SYMBOLS)
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    for name, cls in (("RexOutcomeOut", RexOutcomeOut), ("RexRolloutActionsOutcome", RexRolloutActionsOutcome)):
        body = strip(re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1))
        assert re.findall(r"(\w+)\s*;", body) == [f[0] for f in cls._fields_], name
    flat = re.sub(r"\s+", " ", strip(HEADER))
    assert ("REX_API int rex_outcome(RexSim* sim, const int32_t* d_env_ids, int n, int candidates, const float* d_state, const float* d_ctrl, "
            "const float* d_motor_torque, const RexOutcomeOut* out, void* stream);") in flat
    assert ("REX_API int rex_rollout_actions_outcome(RexSim* sim, const int32_t* d_env_ids, int n, const RexRolloutActionsIn* in, const RexRolloutFrom* from, "
            "const RexRolloutActionsOut* out, const RexRolloutActionsOutcome* outcome, void* d_workspace, long long workspace_bytes, void* stream);") in flat
    assert len(_lib._SIGS["rex_outcome"][0]) == 9 and len(_lib._SIGS["rex_rollout_actions_outcome"][0]) == 10
    low = re.sub(r"[\s*]+", " ", HEADER).lower()                            # the comments' text, their line breaks and margins taken out
    assert "no address is formed from a state or controller word" in low and "sensor noise is not drawn; there is no reset" in low
    assert "running or of done" in low and "cumsum" in low and "terminal one" in low


def test_struct_layouts_and_the_units_the_kernels_live_in():
    src = open(os.path.join(CSRC, "rexsim.hip")).read()
    sizes = re.search(r"static_assert\(sizeof\(RexOutcomeOut\) == (\d+) && sizeof\(RexRolloutActionsOutcome\) == (\d+)", src)
    assert sizes and ctypes.sizeof(RexOutcomeOut) == int(sizes.group(1)) == 24 and ctypes.sizeof(RexRolloutActionsOutcome) == int(sizes.group(2)) == 32
    assert [f[0] for f in RexOutcomeOut._fields_] == ["reward", "done", "obs"] == [f[0] for f in RexRolloutActionsOutcome._fields_][:3]
    assert [getattr(RexOutcomeOut, f[0]).offset for f in RexOutcomeOut._fields_] == [0, 8, 16]
    assert [getattr(RexRolloutActionsOutcome, f[0]).offset for f in RexRolloutActionsOutcome._fields_] == [0, 8, 16, 24]
    assert list(outcome.FIELDS) == ["reward", "done", "obs"] and list(ra.OUTCOME_FIELDS) == ["reward", "done", "obs", "motor_torque"]
    assert list(ra.ALL_FIELDS)[:7] == list(ra.FIELDS) and ra.ActionRollout.STRUCT is _lib.RexRolloutActionsOut and len(ra.ActionRollout._fields) == 7
    # built into the readout object, no object of its own; one device function, two callers, the step's helpers called and not restated
    assert build.INCLUDED_IN["rex_outcome.hip"] == "rex_render.hip" and "rex_outcome.hip" in build.SOURCES and "rex_outcome.h" in build.HEADERS
    assert len(build.variant_jobs()) == 34
    fn = open(os.path.join(CSRC, "rex_outcome.h")).read()
    for call in ("quat_to_euler(", "euler_to_row2(", "env_observation<NM>(", "normalize_obs1(", "group_sum<4>("):
        assert call in fn, call
    assert "__global__" not in fn and "atan2" not in fn and "sincos" not in fn
    assert open(os.path.join(CSRC, "rex_outcome.hip")).read().count("__global__") == 1
    roll = open(os.path.join(CSRC, "rex_rollout.hip")).read()
    assert roll.count("__global__") == 1 and roll.count("outcome_row(") == 2 - 1 and "RexRolloutOutcomeLaunch : RexRolloutFromLaunch" in roll
    assert "if constexpr (OUTCOME) tobs[i] = obs;" in roll


def test_every_refusal_the_arguments_alone_decide_comes_without_a_device():
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    buf = (ctypes.c_float * 512)()
    p = ctypes.addressof(buf)
    some, empty = RexOutcomeOut(reward=p), RexOutcomeOut()
    for args, msg in (((1, 1, p, p, p, None), b"null pointer"), ((1, 1, p, p, p, ctypes.byref(empty)), b"every output pointer is null"),
                      ((1, 0, p, p, p, ctypes.byref(some)), b"candidates 0"), ((1, 1, None, None, None, ctypes.byref(some)), b"null sim"),
                      ((1, 3, p, p, p, ctypes.byref(RexOutcomeOut(done=p))), b"null sim")):
        rc = L.rex_outcome(None, None, *args, None)
        assert rc == -1 and L.rex_last_error().startswith(b"rex_outcome: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    In, out, none, src = _lib.RexRolloutActionsIn, _lib.RexRolloutActionsOut(ctrl=p), _lib.RexRolloutActionsOut(), _lib.RexRolloutFrom(p, p, p)
    good, oc, big = In(p, None, 1, 1, 1, 0.0, 0, -1.0), RexRolloutActionsOutcome(reward=p), 1 << 40
    ref = lambda x: ctypes.byref(x) if x is not None else None
    for inp, s, o, c, w, wb, msg in ((None, src, out, oc, p, big, b"null pointer"), (good, src, out, None, p, big, b"null pointer"), (good, src, None, oc, p, big, b"null pointer"),
                                     (In(None, p, 1, 1, 1, 0.0, 0, -1.0), src, out, oc, p, big, b"null actions"),
                                     (good, src, out, RexRolloutActionsOutcome(), p, big, b"every output pointer is null"),
                                     (good, src, none, oc, None, big, b"workspace"), (good, src, out, oc, p, 407, b"workspace"),
                                     (In(p, None, 0, 1, 1, 0.0, 0, -1.0), src, out, oc, p, big, b"candidates 0"),
                                     (In(p, None, 1, 4097, 0, 0.0, 0, -1.0), src, out, oc, p, big, b"at most 4096 substeps"),
                                     (good, src, none, RexRolloutActionsOutcome(motor_torque=p), p, 408, b"null sim")):      # (`out` may be all null here)
        rc = L.rex_rollout_actions_outcome(None, None, 1, ref(inp), ref(s), ref(o), ref(c), w, wb, None)
        assert rc == -1 and L.rex_last_error().startswith(b"rex_rollout_actions_outcome: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    assert all(v == 0.0 for v in buf)


def stub_env(**kw):
    import torch
    cfg = _lib.RexConfig()
    cfg.action_repeat = 5
    env = type("StubEnv", (), dict(_torch=torch, device=torch.device("cpu"), action_dim=2, obs_dim=4, num_envs=5, mark="base", task="walk", config=cfg))()
    env._row_ids = lambda ids, who: (ids, 5 if ids is None else len(ids))
    for k, v in kw.items():
        setattr(env, k, v)
    return env


def test_python_checks_of_the_arguments():
    import torch
    k, K, T = 5, 3, 4
    # the envs the call does not cover, before anything else is looked at
    lat = _lib.RexConfig(); lat.control_latency = 0.01
    with pytest.raises(NotImplementedError):
        outcome.run(stub_env(mark="arm"))
    for env_kw, word in ((dict(task="mixed"), "mixed"), (dict(config=lat), "latency")):
        with pytest.raises(ValueError) as e:
            outcome.run(stub_env(**env_kw))
        assert str(e.value).startswith("outcome: ") and word in str(e.value)
    rack = _lib.RexConfig(); rack.on_rack = 1
    boxes = _lib.RexConfig(); boxes.body_contacts = 1
    for c, word in ((rack, "on_rack"), (boxes, "body_contacts")):
        with pytest.raises(ValueError) as e:
            ra.run(stub_env(config=c), None, fields=("reward",))
        assert word in str(e.value)
    # fields, then shapes, dtypes and devices (the stub has no library handle: a check that let one through would fail on env._L)
    env = stub_env()
    for bad in ((), ("rewards",), ("reward", "state")):
        with pytest.raises(ValueError) as e:
            outcome.run(env, fields=bad)
        assert "fields must be a non-empty subset" in str(e.value)
    with pytest.raises(ValueError) as e:
        ra.run(env, None, fields=("reward", "dones"))
    assert "motor_torque" in str(e.value)                                 # the message lists what can be named
    env._on_stream = lambda: __import__("contextlib").nullcontext()
    full = dict(state=torch.zeros((k, K, 37)), ctrl=torch.zeros((k, K, 8)), motor_torque=torch.zeros((k, K, 12)))
    for name, t in (("state", torch.zeros((k, K, 36))), ("state", torch.zeros((k, K, 37)).double()), ("state", torch.zeros((k + 1, K, 37))),
                    ("ctrl", torch.zeros((k, K + 1, 8))), ("ctrl", torch.zeros((k, 7))), ("ctrl", torch.zeros((k, K, 8)).numpy()),
                    ("motor_torque", torch.zeros((k, K, 24))[..., ::2]), ("motor_torque", torch.zeros((k, K, 12), device="meta")), ("motor_torque", torch.zeros((k, 11)))):
        with pytest.raises(ValueError) as e:
            outcome.run(env, **{**full, name: t})
        assert str(e.value).startswith("outcome: " + name), (name, str(e.value))
    with pytest.raises(ValueError) as e:
        outcome.run(env, env_ids=[1, 2, 1])
    assert "twice" in str(e.value)
    with pytest.raises(ValueError) as e:
        outcome.run(env, **full, out=object())
    assert "out must be a result of outcome()" in str(e.value)
    assert outcome.candidates_of(env, (None, torch.zeros((k, 8)), None)) is None and outcome.candidates_of(env, (torch.zeros((k, 37)), torch.zeros((k, K, 8)), None)) == K
    # shapes of the results, the public signatures
    assert ra.field_shape("reward", k, K, T) == (T, k, K) == ra.field_shape("done", k, K, T) and ra.field_shape("obs", k, K, T, 16) == (T, k, K, 16)
    assert ra.field_shape("motor_torque", k, K, T) == (T, k, K, 12) and ra.field_shape("state", k, K, T) == (k, K, 37)
    names = ("state", "reward", "done")
    ro = ra.ActionOutcomeRollout({n: torch.zeros(ra.field_shape(n, k, K, T, 4), dtype=getattr(torch, ra.ALL_FIELDS[n][2])) for n in names}, k, K, T)
    assert ro.fields == names and len(ro) == 7 and ro[0] is ro.state and ro[1] is None and ro.obs is None and ro.done.dtype == torch.uint8
    assert isinstance(ro, ra.ActionRollout) and isinstance(ro.struct, _lib.RexRolloutActionsOut) and ro.struct.state == ro.state.data_ptr() and not ro.struct.ctrl
    assert ro.outcome_struct.reward == ro.reward.data_ptr() and ro.outcome_struct.done == ro.done.data_ptr() and not ro.outcome_struct.obs
    oc = outcome.Outcome({"reward": torch.zeros(k), "obs": torch.zeros((k, 4))})
    assert oc.fields == ("reward", "obs") and oc.done is None and oc.rows == k and oc.candidates is None and oc.struct.obs == oc.obs.data_ptr()
    from rex_gym_amd.envs import batch_env
    assert list(inspect.signature(batch_env.RexBatchEnv.outcome).parameters)[1:] == ["state", "ctrl", "motor_torque", "env_ids", "fields", "out"]
