"""Rollouts from given states, under base pushes and per-candidate bodies, the parts that need no GPU: the C ABI's declaration
(include/rexsim.h) and its ctypes mirror (rex_gym_amd/_lib.py), the refusals the arguments alone decide, the Python checks, the float64
reference of tests/rollout_from_ref.py held to its own properties, the float32 floor behind the bounds of tests/test_gpu_rollout_from.py,
and the teeth of that bound.

The floor (test 3): per case of rollout_from_ref.CASES, repeat = 1, the commands of rollout_ref.targets, per row and control step a wrench
-- force uniform within +- half the nominal robot's weight per axis (0.5 x 4.52 kg x 10 m/s^2 = 22.6 N), moment within +- that x 0.1 m --
and per row a body -- mass scales 0.8 .. 1.2, friction 0.3 .. 1.0 (rollout_from_ref.draws; as first chosen, not shrunk to reach the kept share).  Walk the
float64 reference's trajectory with each state rounded to float32; per transition the deviation of the float32 evaluation's v_next from the
float64 one (step_readout_ref.vel_error).  Kept: rollout_ref.kept, and that deviation at most test_gpu_contact_solve.BOUNDS["v_next"].
Measured here (kept of all transitions, floor per family of columns):

    case                  kept          synthetic    real
    5   plane   K3 T4     60 / 60       3.314e-06    9.221e-05
    67  random  K2 T3     402 / 402     5.185e-05    8.913e-05

Teeth (test 4), the 5-env plane case, its 60 kept transitions: a reference that ignores the wrench misses the family's bound on 60, one
that takes the env's body parameters instead of the row's on 60."""
import ctypes
import os
import re

import numpy as np
import pytest

import contact_solve_ref as cr
import kinematics_ref as kr
import rollout_from_ref as rf
import rollout_ref as rr
import step_readout_ref as sr
from rex_gym_amd import _lib, build, rollout
from rex_gym_amd._lib import RexRolloutFrom          # (a tree without the call fails here: no test of this file passes on it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
CSRC = os.path.join(ROOT, "rex_gym_amd", "csrc")
CALL = "rex_rollout_from"


# ---------------------------------------------------------------- 1. ABI
def test_header_declares_the_call_and_the_struct_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert CALL in declared and declared == set(_lib.EXPORTED_SYMBOLS)
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    strip = lambda body: re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = strip(re.search(r"typedef struct RexRolloutFrom \{(.*?)\} RexRolloutFrom;", HEADER, re.S).group(1))
    members = re.findall(r"const float\s*\*\s*(\w+)\s*;", body)
    assert members == ["init_state", "base_wrench", "body"] == [f[0] for f in _lib.RexRolloutFrom._fields_]
    assert all(f[1] is ctypes.c_void_p for f in _lib.RexRolloutFrom._fields_)
    flat = re.sub(r"\s+", " ", strip(HEADER))
    assert re.search(r"REX_API int rex_rollout_from\(RexSim\* sim, const int32_t\* d_env_ids, int n, const RexRolloutIn\* in, const RexRolloutFrom\* from, "
                     r"const RexRolloutOut\* out, void\* stream\)", flat)
    assert "a bad row" in HEADER.lower() and "garbage in that row only" in HEADER


def test_struct_layout_and_the_kernel_is_one_source_with_rex_rollouts():
    src = open(os.path.join(CSRC, "rexsim.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(RexRolloutFrom\) == (\d+)", src)
    assert asserted and ctypes.sizeof(_lib.RexRolloutFrom) == int(asserted.group(1)) == 24
    assert [getattr(_lib.RexRolloutFrom, f[0]).offset for f in _lib.RexRolloutFrom._fields_] == [0, 8, 16]
    assert ctypes.sizeof(_lib.RexRolloutIn) == 40 and ctypes.sizeof(_lib.RexRolloutOut) == 32          # pinned: the new call takes them as they are
    assert CALL in _lib.EXPORTED_SYMBOLS and len(_lib._SIGS[CALL][0]) == 7
    kernel = open(os.path.join(CSRC, "rex_rollout.hip")).read()
    assert kernel.count("__global__") == 1 and "rex_rollout_kernel<rex::RexRolloutLaunch>" in kernel and "rex_rollout_kernel<rex::RexRolloutFromLaunch>" in kernel
    assert 'asm volatile("" : "+v"(el), "+v"(leg))' in kernel                                           # the opaque copies stay in the substep loop
    rows = open(os.path.join(CSRC, "rex_contact_rows.h")).read()
    assert "template <bool WRENCH = false>" in rows and "con_free_velocity<true>(" in kernel


def test_every_refusal_the_arguments_alone_decide_comes_without_a_device():
    """what rex_rollout refuses in front of everything the sim decides, through the new entry point, and a null `from`; then the null sim"""
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    In, out, empty = _lib.RexRolloutIn, _lib.RexRolloutOut(state=p), _lib.RexRolloutOut()
    src, none = RexRolloutFrom(p, p, p), RexRolloutFrom()
    good = In(p, None, 1, 1, 1, 0.0, 0, -1.0)
    nan, inf = float("nan"), float("inf")
    calls = [(None, src, out, b"null pointer"), (good, None, out, b"null pointer"), (good, src, None, b"null pointer"),
             (In(p, p, 1, 1, 1, 0.0, 0, -1.0), src, out, b"exactly one of targets and tau"), (In(None, None, 1, 1, 1, 0.0, 0, -1.0), src, out, b"exactly one of targets and tau"),
             (good, src, empty, b"every output pointer is null"), (In(p, None, 0, 1, 1, 0.0, 0, -1.0), src, out, b"candidates 0"),
             (In(None, p, -3, 1, 1, 0.0, 0, -1.0), none, out, b"candidates -3"), (In(p, None, 1, 0, 1, 0.0, 0, -1.0), src, out, b"steps 0"),
             (In(p, None, 1, 4097, 0, 0.0, 0, -1.0), src, out, b"at most 4096 substeps"), (In(p, None, 1, 1025, 4, 0.0, 0, -1.0), src, out, b"at most 4096 substeps"),
             (In(p, None, 1, 2 ** 30, 2 ** 30, 0.0, 0, -1.0), src, out, b"at most 4096 substeps"), (In(p, None, 1, 1, 1, 0.0, 1001, -1.0), src, out, b"iterations 1001"),
             (In(p, None, 1, 1, 1, inf, 0, -1.0), src, out, b"finite"), (In(p, None, 1, 1, 1, nan, 0, -1.0), src, out, b"finite"),
             (In(p, None, 1, 1, 1, 0.0, 0, nan), src, out, b"finite"), (In(p, None, 1, 1, 1, 0.0, 0, inf), src, out, b"finite"),
             (good, src, out, b"null sim"), (good, none, out, b"null sim"), (In(None, p, 3, 1024, 4, 0.001, 1000, 0.0), src, out, b"null sim")]
    ref = lambda x: ctypes.byref(x) if x is not None else None
    for inp, s, o, msg in calls:
        rc = L.rex_rollout_from(None, None, 1, ref(inp), ref(s), ref(o), None)
        assert rc == -1 and L.rex_last_error().startswith(b"rex_rollout_from: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    assert all(v == 0.0 for v in buf)


def test_python_checks_of_the_three_inputs():
    import torch
    env = type("StubEnv", (), dict(_torch=torch, device=torch.device("cpu")))()
    k, K, T = 5, 3, 4
    init, wr, body = torch.zeros((k, K, 37)), torch.zeros((k, K, T, 6)), torch.zeros((k, K, 3))
    assert rollout.check_from(env, None, None, None, k, K, T) == (None, None, None)
    a, b, c = rollout.check_from(env, init, wr, body, k, K, T)
    assert a is init and b is wr and c is body
    one = torch.arange(k * 37, dtype=torch.float32).reshape(k, 37)
    spread = rollout.check_from(env, one, None, None, k, K, T)[0]
    assert spread.shape == (k, K, 37) and spread.is_contiguous() and all(torch.equal(spread[:, j], one) for j in range(K))
    bad = dict(init_state=(init[:4], init[:, :2], init[..., :36], init.double(), init.numpy(), torch.zeros((k, K, 74))[..., ::2], one[:, :36], torch.zeros((k, 1, 37))),
               base_wrench=(wr[:, :, :3], wr[..., :5], wr.half(), torch.zeros((k, K, T, 12))[..., ::2], torch.zeros((k, K, 6))),
               body=(body[:, :2], body[..., :2], body.double(), torch.zeros((k, 3)), [1.0, 1.0, 0.5]))
    for name, tensors in bad.items():
        for t in tensors:
            with pytest.raises(ValueError) as e:
                rollout.check_from(env, **{"init_state": None, "base_wrench": None, "body": None, name: t}, k=k, K=K, T=T)
            assert str(e.value).startswith("rollout: " + name)
    import inspect
    from rex_gym_amd.envs import batch_env
    names = list(inspect.signature(batch_env.RexBatchEnv.rollout).parameters)
    assert names[-3:] == ["init_state", "base_wrench", "body"] == list(inspect.signature(rollout.run).parameters)[-3:]
    assert names[1:-3] == list(inspect.signature(rollout.run).parameters)[1:-3]                          # the keywords from before, in their order


# ---------------------------------------------------------------- 2. the reference's own properties, float64
@pytest.fixture(scope="module")
def small():
    """the 5-env plane case: states, fields, the scene's body parameters, commands [5, 3, 4, 12], the draws"""
    n, ground, K, T = rf.CASES[0]
    S, ep, kinds = rr.host_states(n, ground)
    fields, bp = rr.case_params(n, ground)
    wr, body = rf.draws(n, K, T)
    return S, [kr.field_of(fields, g, ep[g]) for g in range(n)], bp, rr.targets(S[13:25].T, K, T), wr, body


def test_the_reference_is_rollout_refs_with_the_wrench_in_the_free_velocity_and_the_rows_body(small):
    S, flds, bp, cmds, wr, body = small
    assert abs(rf.nominal_weight() - 45.2) < 0.05 and np.abs(wr[..., :3]).max() <= 0.5 * rf.nominal_weight() and np.abs(wr[..., :3]).max() > 20.0
    assert np.abs(wr[..., 3:]).max() <= 0.05 * rf.nominal_weight() and 0.8 <= body[..., :2].min() and body[..., :2].max() <= 1.2 and 0.3 <= body[..., 2].min()
    for g in (0, 4):
        s, kw = S[:, g], dict(field=flds[g], scales=(bp[0, g], bp[1, g]), mu=float(bp[2, g]))
        plain = rr.transition(s, cmds[g, 0, 0], **kw)
        # no wrench, the env's body: rollout_ref's transition; a wrench of zeros: the same numbers (b - 0)
        for tr in (rf.transition(s, cmds[g, 0, 0], **kw), rf.transition(s, cmds[g, 0, 0], np.zeros(6), bp[:, g], field=flds[g]), rf.transition(s, cmds[g, 0, 0], np.zeros(6), **kw)):
            assert np.array_equal(tr["state"], plain["state"]) and np.array_equal(tr["v_next"], plain["v_next"])
        # v* moves by dt M^-1 (w, 0): the free velocity of the contact reference, tau and the damping as they were
        w = wr[g, 0, 0].astype(np.float64)
        pushed = rf.transition(s, cmds[g, 0, 0], w, **kw)
        M = np.asarray(plain["ref"]["dyn"]["mass_matrix"], np.float64)
        want = plain["ref"]["v_star"] + rr.DT * np.linalg.solve(M, np.concatenate([w, np.zeros(12)]))
        assert np.abs(pushed["ref"]["v_star"] - want).max() <= 1e-12 and np.abs(pushed["ref"]["v_star"] - plain["ref"]["v_star"]).max() > 1e-3
        assert np.array_equal(pushed["tau"], plain["tau"]) and np.array_equal(pushed["ref"]["dyn"]["bias"][6:], plain["ref"]["dyn"]["bias"][6:])
        assert np.abs(plain["ref"]["dyn"]["bias"][:6] - pushed["ref"]["dyn"]["bias"][:6] - w).max() <= 1e-12
        # the body: scales and mu of the row
        other = rf.transition(s, cmds[g, 0, 0], None, body[g, 1], field=flds[g])
        assert np.array_equal(other["v_next"], rr.transition(s, cmds[g, 0, 0], field=flds[g], scales=(body[g, 1, 0], body[g, 1, 1]), mu=float(body[g, 1, 2]))["v_next"])
        assert not np.array_equal(other["v_next"], plain["v_next"]) and other["ref"]["mu"] == float(body[g, 1, 2])


def test_a_rollout_continued_from_its_state_is_the_unsplit_one(small):
    S, flds, bp, cmds, wr, body = small
    for g in (1, 3):
        kw = dict(body=body[g, 1], field=flds[g])
        whole = rf.rollout(S[:, g], cmds[g, 1], wr[g, 1], repeat=2, **kw)
        head = rf.rollout(S[:, g], cmds[g, 1, :2], wr[g, 1, :2], repeat=2, **kw)
        tail = rf.rollout(head["state"], cmds[g, 1, 2:], wr[g, 1, 2:], repeat=2, **kw)
        assert np.array_equal(head["trajectory"], whole["trajectory"][:2]) and np.array_equal(tail["trajectory"], whole["trajectory"][2:])
        assert np.array_equal(tail["state"], whole["state"]) and head["sweeps"] + tail["sweeps"] == whole["sweeps"] == 8 * cr.ITERATIONS
        assert [(t, h) for t, h, _, _ in whole["transitions"]] == [(t, h) for t in range(4) for h in range(2)]


# ---------------------------------------------------------------- 3. the floor
@pytest.fixture(scope="module")
def walks():
    import test_gpu_contact_solve as tc
    import test_gpu_kinematics as tk
    return {case: rf.walk(*case, tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"], tc.BOUNDS["v_next"]) for case in rf.CASES}


def test_bounds_of_the_gpu_test_are_the_stated_multiple_of_the_float32_floor(walks):
    """At least 95 % of every case's transitions are kept by the reference walk alone; per family the largest deviation over the kept
    transitions of both cases is the floor; the GPU test's bound is FACTOR (4) x that, with 2 % of slack for another libm; the profile holds
    the same numbers."""
    import test_gpu_rollout_from as tg
    assert rf.CASES == [(5, "plane", 3, 4), (67, "random", 2, 3)]
    floors = {f: 0.0 for f in rr.FAMILIES}
    for case, rows in walks.items():
        assert len(rows) == case[0] * case[2] * case[3] and all(r["h"] == 0 for r in rows)
        kept = [r for r in rows if r["kept"]]
        own = {f: max([r["dev"] for r in kept if r["family"] == f] or [0.0]) for f in rr.FAMILIES}
        print(case, "kept %d of %d (%.1f %%), floors" % (len(kept), len(rows), 100.0 * len(kept) / len(rows)), {f: "%.3e" % v for f, v in own.items()},
              "largest deviation left out %.2e" % max([r["dev"] for r in rows if not r["kept"]] or [0.0]))
        assert len(kept) >= 0.95 * len(rows), (case, len(kept), len(rows))
        assert all(any(r["family"] == f for r in kept) for f in rr.FAMILIES)
        assert any(np.asarray(r["ref"]["toe_lambda"])[:, 0].max() > 0 for r in kept) and any(np.abs(r["wrench"][:3]).max() > 0.4 * rf.nominal_weight() for r in kept)
        floors = {f: max(floors[f], own[f]) for f in rr.FAMILIES}
    print("floors", {f: "%.3e" % v for f, v in floors.items()}, "written", tg.FLOORS, "bounds", tg.BOUNDS)
    assert tg.FACTOR == 4.0 and set(tg.BOUNDS) == set(tg.FLOORS) == set(rr.FAMILIES)
    profile = open(os.path.join(ROOT, "profiles", "rollout_from.md")).read()
    for f in rr.FAMILIES:
        assert tg.BOUNDS[f] <= tg.FACTOR * tg.FLOORS[f] * (1 + 1e-3)
        assert tg.FACTOR * floors[f] * 0.98 <= tg.BOUNDS[f] <= tg.FACTOR * floors[f] * 1.02, (f, tg.BOUNDS[f], floors[f])
        assert "%.3e" % tg.BOUNDS[f] in profile and "%.3e" % tg.FLOORS[f] in profile and "%.3e" % tg.BOUNDS[f] in tg.__doc__


# ---------------------------------------------------------------- 4. teeth
def test_a_reference_without_the_wrench_and_one_with_the_envs_body_miss_the_bound(walks):
    """The 5-env plane case.  From every kept transition of the walk: the reference that leaves the wrench out, and the one that takes the
    env's body parameters (the scene's) instead of the row's, each against the right one -- both miss the family's bound on most of them."""
    import test_gpu_rollout_from as tg
    n, ground, K, T = rf.CASES[0]
    _, bp = rr.case_params(n, ground)
    kept = [r for r in walks[rf.CASES[0]] if r["kept"]]
    no_wrench, env_body = [], []
    for r in kept:
        right, g = r["ref"]["v_next"], r["env"]
        a = rf.transition(r["state"], r["command"], None, r["body"], field=r["field"])["v_next"]
        b = rf.transition(r["state"], r["command"], r["wrench"], bp[:, g], field=r["field"])["v_next"]
        no_wrench.append(sr.vel_error(a, right) > tg.BOUNDS[r["family"]])
        env_body.append(sr.vel_error(b, right) > tg.BOUNDS[r["family"]])
    print("kept transitions: %d of %d; over the bound: without the wrench %d, with the env's body %d" % (len(kept), n * K * T, sum(no_wrench), sum(env_body)))
    assert len(kept) >= 0.95 * n * K * T
    assert np.mean(no_wrench) > 0.5 and np.mean(env_body) > 0.5, (np.mean(no_wrench), np.mean(env_body))
