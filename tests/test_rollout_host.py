"""Candidate rollouts, the parts that need no GPU: the build lists, the C ABI's declarations (include/rexsim.h) and their ctypes mirror
(rex_gym_amd/_lib.py), the refusals the arguments alone decide, the float64 reference of tests/rollout_ref.py held to its own properties, the
float32 floor behind the bounds of tests/test_gpu_rollout.py, and the teeth of that bound.

The floor (test 3): per case of rollout_ref.CASES, repeat = 1, targets = the row's initial joint angles + uniform(-0.3, 0.3), the scene's mass
scales and friction, the leading real columns from step_readout_ref.real_family.  Walk the float64 reference's trajectory with each state
rounded to float32; per transition the deviation of the float32 evaluation's v_next from the float64 one (step_readout_ref.vel_error).  A
transition is kept when contact_solve_ref.compared holds, no component of v_next is at the +-100 clamp and that deviation is at most
test_gpu_contact_solve.BOUNDS["v_next"].  Measured here (kept of all transitions, floor per family of columns):

    case                  kept          synthetic    real
    5   plane   K3 T4     60 / 60       4.042e-06    3.442e-05
    67  plane   K2 T3     399 / 402     4.888e-05    7.318e-05
    67  random  K2 T3     398 / 402     8.737e-05    2.173e-04
    67  custom  K2 T3     397 / 402     1.497e-04    2.942e-05
    130 plane   K1 T2     260 / 260     2.213e-05    1.462e-05

The transitions left out are float32 numpy's own misses (deviations up to 1.2: two nearly dependent toe rows under a fast-spinning foot
joint, unresolved after 60 sweeps)."""
import ctypes
import os
import re

import numpy as np
import pytest

import contact_solve_ref as cr
import kinematics_ref as kr
import rollout_ref as rr
import step_readout_ref as sr
from rex_gym_amd import _lib, build, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
CSRC = os.path.join(ROOT, "rex_gym_amd", "csrc")
CALL = "rex_rollout"


# ---------------------------------------------------------------- 1. build and ABI
def test_build_lists_hold_the_unit_and_its_headers():
    assert "rex_rollout.hip" in build.SOURCES and build.INCLUDED_IN["rex_rollout.hip"] == "rex_render.hip"
    assert '#include "rex_rollout.hip"' in open(os.path.join(CSRC, "rex_render.hip")).read()
    assert {"rex_rollout.h", "rex_rollout_leg.h", "rex_contact_rows.h", "rex_contact_solve.h", "rex_dynamics_leg.h"} <= set(build.HEADERS)
    assert all(job[0] != "rex_rollout.hip" for job in build.variant_jobs())           # no object of its own
    kernel, solve = open(os.path.join(CSRC, "rex_rollout.hip")).read(), open(os.path.join(CSRC, "rex_contact_solve.hip")).read()
    for shared in ("con_free_velocity(", "con_build_rows(", "con_sweeps(", "con_velocity_change("):       # both kernels call the lifted sections
        assert shared in kernel and shared in solve, shared
    assert "atomic" not in kernel.split("namespace rex {")[1] and kernel.count("__syncthreads()") == 2 and "rollout_integrate(" in kernel


def test_header_declares_the_call_and_both_structs_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert CALL in declared and declared == set(_lib.EXPORTED_SYMBOLS)
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    strip = lambda body: re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = strip(re.search(r"typedef struct RexRolloutIn \{(.*?)\} RexRolloutIn;", HEADER, re.S).group(1))
    members = [(t.replace(" ", ""), n) for t, n in re.findall(r"(const float\s*\*|float|int32_t)\s*(\w+)(?=\s*[;,])", body)]
    want = [("constfloat*", "targets"), ("constfloat*", "tau"), ("int32_t", "candidates"), ("int32_t", "steps"), ("int32_t", "repeat"), ("float", "dt"),
            ("int32_t", "iterations"), ("float", "residual_threshold")]
    assert members == want and [f[0] for f in _lib.RexRolloutIn._fields_] == [m[1] for m in want]
    ctype = {"constfloat*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [f[1] for f in _lib.RexRolloutIn._fields_] == [ctype[m[0]] for m in want]
    body = strip(re.search(r"typedef struct RexRolloutOut \{(.*?)\} RexRolloutOut;", HEADER, re.S).group(1))
    outs = re.findall(r"(float|uint8_t|int32_t)\s*\*\s*(\w+)\s*;", body)
    assert outs == [("float", "state"), ("float", "trajectory"), ("uint8_t", "foot_contact"), ("int32_t", "sweeps")]
    assert [m[1] for m in outs] == [f[0] for f in _lib.RexRolloutOut._fields_] == list(rollout.FIELDS)
    assert [rollout.FIELDS[m[1]][1] for m in outs] == ["float32", "float32", "uint8", "int32"]
    flat = re.sub(r"\s+", " ", strip(HEADER))
    assert re.search(r"REX_API int rex_rollout\(RexSim\* sim, const int32_t\* d_env_ids, int n, const RexRolloutIn\* in, const RexRolloutOut\* out, void\* stream\)", flat)


def test_struct_layouts_and_the_limits_the_host_code_asserts():
    src = open(os.path.join(CSRC, "rexsim.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(RexRolloutIn\) == (\d+) && sizeof\(RexRolloutOut\) == (\d+)", src)
    assert asserted and ctypes.sizeof(_lib.RexRolloutIn) == int(asserted.group(1)) == 40
    assert ctypes.sizeof(_lib.RexRolloutOut) == int(asserted.group(2)) == 32 == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert [getattr(_lib.RexRolloutIn, f[0]).offset for f in _lib.RexRolloutIn._fields_] == [0, 8, 16, 20, 24, 28, 32, 36]
    hdr = open(os.path.join(CSRC, "rex_rollout.h")).read()
    assert re.search(r"kRolloutMaxSubsteps = (\d+)", hdr).group(1) == "4096" == str(rollout.MAX_SUBSTEPS)
    assert re.search(r"kRolloutWords = (\d+)", hdr).group(1) == "37" == str(rollout.WORDS) == str(rr.WORDS)
    assert CALL in _lib.EXPORTED_SYMBOLS and len(_lib._SIGS[CALL][0]) == 6


def test_every_refusal_the_arguments_alone_decide_comes_without_a_device():
    """in front of everything the sim decides, so with a null sim: null in / out, both or neither command, no output, K < 1, T < 1, more than
    4096 substeps, more than 1000 sweeps, a non-finite dt or threshold; then the null sim itself.  (n < 1, n > num_envs, the 2^31 limit and
    the sims that are refused need a sim: tests/test_gpu_rollout.py.)"""
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    In, out, empty = _lib.RexRolloutIn, _lib.RexRolloutOut(state=p), _lib.RexRolloutOut()
    good = In(p, None, 1, 1, 1, 0.0, 0, -1.0)
    nan, inf = float("nan"), float("inf")
    calls = [(None, out, b"null pointer"), (good, None, b"null pointer"), (In(p, p, 1, 1, 1, 0.0, 0, -1.0), out, b"exactly one of targets and tau"),
             (In(None, None, 1, 1, 1, 0.0, 0, -1.0), out, b"exactly one of targets and tau"), (good, empty, b"every output pointer is null"),
             (In(p, None, 0, 1, 1, 0.0, 0, -1.0), out, b"candidates 0"), (In(None, p, -3, 1, 1, 0.0, 0, -1.0), out, b"candidates -3"),
             (In(p, None, 1, 0, 1, 0.0, 0, -1.0), out, b"steps 0"), (In(p, None, 1, 4097, 0, 0.0, 0, -1.0), out, b"at most 4096 substeps"),
             (In(p, None, 1, 1025, 4, 0.0, 0, -1.0), out, b"at most 4096 substeps"), (In(p, None, 1, 2 ** 30, 2 ** 30, 0.0, 0, -1.0), out, b"at most 4096 substeps"),
             (In(p, None, 1, 1, 1, 0.0, 1001, -1.0), out, b"iterations 1001"), (In(p, None, 1, 1, 1, inf, 0, -1.0), out, b"finite"),
             (In(p, None, 1, 1, 1, nan, 0, -1.0), out, b"finite"), (In(p, None, 1, 1, 1, 0.0, 0, nan), out, b"finite"), (In(p, None, 1, 1, 1, 0.0, 0, inf), out, b"finite"),
             (good, out, b"null sim"), (In(None, p, 3, 1024, 4, 0.001, 1000, 0.0), out, b"null sim")]
    for inp, o, msg in calls:
        rc = L.rex_rollout(None, None, 1, ctypes.byref(inp) if inp is not None else None, ctypes.byref(o) if o is not None else None, None)
        assert rc == -1 and L.rex_last_error().startswith(b"rex_rollout: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    assert all(v == 0.0 for v in buf)


def test_python_checks_refuse_before_any_launch():
    import torch
    env = type("StubEnv", (), dict(_torch=torch, device=torch.device("cpu")))()
    names = tuple(rollout.FIELDS)
    assert rollout.check_fields(None) == names and rollout.check_fields("sweeps") == ("sweeps",) and rollout.check_fields(("sweeps", "state")) == ("state", "sweeps")
    for bad in (("nope",), ()):
        with pytest.raises(ValueError) as e:
            rollout.check_fields(bad)
        assert str(e.value) == f"rollout: fields must be a non-empty subset of {names}, got {bad}"
    assert {n: rollout.field_shape(n, 5, 3, 4) for n in names} == {"state": (5, 3, 37), "trajectory": (5, 3, 4, 37), "foot_contact": (5, 3, 4, 4), "sweeps": (5, 3)}
    assert rollout.check_repeat(None, 4, 5) == 0 and rollout.check_repeat(7, 4, 5) == 7 and rollout.check_repeat(4, 1024, 5) == 4
    for bad, T in ((0, 1), (-1, 1), (1.0, 1), (True, 1), ("2", 1), (5, 820), (None, 820)):
        with pytest.raises(ValueError):
            rollout.check_repeat(bad, T, 5)
    assert rollout.check_settings(None, None, None) == (0.0, 0, -1.0) and rollout.check_settings(0.002, 10, 0) == (0.002, 10, 0.0)
    for kw in (dict(dt=0.0), dict(dt=float("nan")), dict(iterations=1001), dict(iterations=0), dict(residual_threshold=-1.0)):
        with pytest.raises(ValueError) as e:
            rollout.check_settings(**{**dict(dt=None, iterations=None, residual_threshold=None), **kw})
        assert str(e.value).startswith("rollout: ")
    cmd = torch.zeros((5, 3, 4, 12))
    assert rollout.check_commands(env, cmd, None, 5) == (cmd, 3, 4) and rollout.check_commands(env, None, cmd, 5) == (cmd, 3, 4)
    for targets, tau in ((None, None), (cmd, cmd), (cmd[:4], None), (cmd[..., :11], None), (cmd.double(), None), (cmd[:, :, 0], None), (cmd.numpy(), None),
                         (torch.zeros((5, 3, 4, 24))[..., ::2], None), (None, torch.zeros((5, 0, 4, 12))), (torch.zeros((5, 3, 0, 12)), None)):
        with pytest.raises(ValueError) as e:
            rollout.check_commands(env, targets, tau, 5)
        assert str(e.value).startswith("rollout: ")
    shapes = {n: rollout.field_shape(n, 5, 3, 4) for n in names}
    out = rollout.Rollout({n: torch.zeros(shapes[n], dtype=getattr(torch, rollout.FIELDS[n][1])) for n in names}, 3, 4)
    assert out.fields == names and (out.rows, out.candidates, out.steps) == (5, 3, 4) and rollout.check_result(out, names, 5, 3, 4, env) is None
    state, trajectory, foot_contact, sweeps = out
    assert state is out.state and trajectory is out.trajectory and foot_contact is out.foot_contact and sweeps is out.sweeps and out[3] is sweeps
    assert out.joint_angles.shape == (5, 3, 12) and out.base_quat.shape == (5, 3, 4)
    for wrong, want, shape in ((None, names, (5, 3, 4)), (out, names[:1], (5, 3, 4)), (out, names, (6, 3, 4)), (out, names, (5, 2, 4)), (out, names, (5, 3, 5))):
        with pytest.raises(ValueError) as e:
            rollout.check_result(wrong, want, *shape, env)
        assert str(e.value).startswith("rollout: out")


# ---------------------------------------------------------------- 2. the reference's own properties, float64
@pytest.fixture(scope="module")
def small():
    """the 5-env plane case: states, per-env keywords of rollout_ref.transition, commands [5, 3, 4, 12]"""
    n, ground, K, T = rr.CASES[0]
    S, ep, kinds = rr.host_states(n, ground)
    fields, bp = rr.case_params(n, ground)
    kw = [dict(field=kr.field_of(fields, g, ep[g]), scales=(bp[0, g], bp[1, g]), mu=float(bp[2, g])) for g in range(n)]
    return S, kw, rr.targets(S[13:25].T, K, T), kinds


def test_one_step_of_the_reference_is_the_motor_model_the_contact_reference_and_advance(small):
    S, kw, cmds, kinds = small
    assert kinds[0] == "real" and kinds[4] != "real"
    for g in (0, 4):
        s = S[:, g]
        out = rr.rollout(s, cmds[g, 0, :1], **kw[g])
        tau = sr.motor_model(cmds[g, 0, 0], s[13:25], s[25:37], s[25:37])[0]
        # (the oracle's motor model in C is another implementation of the same formula: float64 round-off apart)
        assert np.abs(tau - sr.motor_tau(cmds[g, 0, 0], S, g)).max() <= 1e-12 and np.abs(tau).max() > 0.5
        ref = cr.reference(S, g, kw[g]["field"], kw[g]["scales"], kw[g]["mu"], tau, dt=rr.DT)
        A = S.astype(np.float64)
        A[sr.VEL_WORDS, g] = ref["v_next"]
        want = kr.advance(A, g, False, rr.DT)
        want[3:7] /= np.linalg.norm(want[3:7])
        assert np.array_equal(out["state"], want[0:37]) and np.array_equal(out["trajectory"][0], want[0:37]) and out["sweeps"] == cr.ITERATIONS
        assert np.array_equal(out["foot_contact"][0], (ref["toe_lambda"][:, 0] > 0).reshape(4, 2).any(1))
        # tau mode applies the command itself; a disabled motor draws nothing
        assert np.array_equal(rr.rollout(s, tau[None], mode="tau", **kw[g])["state"], out["state"])
        off = rr.torque(cmds[g, 0, 0], s, motor_en=sr.ALL_MOTORS & ~(1 << 4))
        assert off[4] == 0.0 and np.array_equal(np.delete(off, 4), np.delete(tau, 4))
        p = dict(voltage=28.0, damping=0.03, kp=1.2, kd=0.03, strength=np.linspace(0.7, 1.2, 12))
        assert np.array_equal(rr.torque(cmds[g, 0, 0], s, motor=p), sr.motor_tau_params(cmds[g, 0, 0], S, g, 28.0, 0.03, 1.2, 0.03, p["strength"]))


def test_a_rollout_split_at_any_control_step_equals_the_unsplit_one(small):
    S, kw, cmds, _ = small
    for g in (1, 3):
        whole = rr.rollout(S[:, g], cmds[g, 1], **kw[g])
        for cut in (1, 2, 3):
            head = rr.rollout(S[:, g], cmds[g, 1, :cut], **kw[g])
            tail = rr.rollout(head["state"], cmds[g, 1, cut:], **kw[g])
            assert np.array_equal(head["trajectory"], whole["trajectory"][:cut]) and np.array_equal(tail["trajectory"], whole["trajectory"][cut:])
            assert np.array_equal(tail["state"], whole["state"]) and np.array_equal(tail["foot_contact"], whole["foot_contact"][cut:])
            assert head["sweeps"] + tail["sweeps"] == whole["sweeps"]
        assert not np.array_equal(whole["trajectory"][0], whole["trajectory"][1])


def test_repeat_two_is_repeat_one_with_every_command_doubled(small):
    S, kw, cmds, _ = small
    for g in (0, 2):
        two = rr.rollout(S[:, g], cmds[g, 2, :2], repeat=2, **kw[g])
        doubled = rr.rollout(S[:, g], np.repeat(cmds[g, 2, :2], 2, axis=0), **kw[g])
        assert np.array_equal(two["trajectory"], doubled["trajectory"][1::2]) and np.array_equal(two["state"], doubled["state"])
        assert np.array_equal(two["foot_contact"], doubled["foot_contact"][1::2]) and two["sweeps"] == doubled["sweeps"] == 4 * cr.ITERATIONS
        assert [(t, h) for t, h, _, _ in two["transitions"]] == [(0, 0), (0, 1), (1, 0), (1, 1)]


# ---------------------------------------------------------------- 3. the floor
@pytest.fixture(scope="module")
def walks():
    import test_gpu_contact_solve as tc
    import test_gpu_kinematics as tk
    return {case: rr.walk(*case, tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"], tc.BOUNDS["v_next"]) for case in rr.CASES}


def test_bounds_of_the_gpu_test_are_the_stated_multiple_of_the_float32_floor(walks):
    """At least 90 % of every case's transitions are kept; per family the largest deviation over the kept transitions of all cases is the
    floor; the GPU test's bound is FACTOR (4) x that, with 2 % of slack for another libm; the profile holds the same numbers."""
    import test_gpu_rollout as tg
    floors = {f: 0.0 for f in rr.FAMILIES}
    for case, rows in walks.items():
        assert len(rows) == case[0] * case[2] * case[3] and all(r["h"] == 0 for r in rows)
        kept = [r for r in rows if r["kept"]]
        own = {f: max([r["dev"] for r in kept if r["family"] == f] or [0.0]) for f in rr.FAMILIES}
        print(case, "kept %d of %d (%.1f %%), floors" % (len(kept), len(rows), 100.0 * len(kept) / len(rows)), {f: "%.3e" % v for f, v in own.items()},
              "largest deviation left out %.2e" % max([r["dev"] for r in rows if not r["kept"]] or [0.0]))
        assert len(kept) >= 0.9 * len(rows), (case, len(kept), len(rows))
        assert all(any(r["family"] == f for r in kept) for f in rr.FAMILIES)
        assert any(np.asarray(r["ref"]["toe_lambda"])[:, 0].max() > 0 for r in kept) and any(np.abs(r["tau"]).max() > 3.0 for r in kept)
        floors = {f: max(floors[f], own[f]) for f in rr.FAMILIES}
    print("floors", {f: "%.3e" % v for f, v in floors.items()}, "written", tg.FLOORS, "bounds", tg.BOUNDS)
    assert tg.FACTOR == 4.0 and set(tg.BOUNDS) == set(tg.FLOORS) == set(rr.FAMILIES)
    profile = open(os.path.join(ROOT, "profiles", "rollout.md")).read()
    for f in rr.FAMILIES:
        assert tg.BOUNDS[f] <= tg.FACTOR * tg.FLOORS[f] * (1 + 1e-3)
        assert tg.FACTOR * floors[f] * 0.98 <= tg.BOUNDS[f] <= tg.FACTOR * floors[f] * 1.02, (f, tg.BOUNDS[f], floors[f])
        assert "%.3e" % tg.BOUNDS[f] in profile and "%.3e" % tg.FLOORS[f] in profile and "%.3e" % tg.BOUNDS[f] in tg.__doc__


# ---------------------------------------------------------------- 4. teeth
def test_a_held_torque_and_a_torque_off_by_one_percent_miss_the_bound():
    """The 5-env plane case at repeat = 3.  From every kept transition with h >= 1 of the walk: the reference that holds the control step's
    FIRST substep's torque instead of drawing it anew, and the one with the torque off by 1 %, each against the right one -- both miss the
    family's bound on at least half of those transitions."""
    import test_gpu_contact_solve as tc
    import test_gpu_kinematics as tk
    import test_gpu_rollout as tg
    n, ground, K, T = rr.CASES[0]
    rows = rr.walk(n, ground, K, T, tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"], tc.BOUNDS["v_next"], repeat=3)
    assert len(rows) == n * K * T * 3
    first = {(r["env"], r["cand"], r["t"]): r["tau"] for r in rows if r["h"] == 0}
    later = [r for r in rows if r["kept"] and r["h"] >= 1]
    held, off = [], []
    for r in later:
        kw = dict(field=r["field"], scales=r["scales"], mu=r["mu"])
        right = r["ref"]["v_next"]
        for wrong, tau in ((held, first[(r["env"], r["cand"], r["t"])]), (off, 1.01 * r["tau"])):
            wrong.append(sr.vel_error(rr.transition(r["state"], r["command"], tau=tau, **kw)["v_next"], right) > tg.BOUNDS[r["family"]])
    print("kept transitions with h >= 1: %d of %d; over the bound: held torque %d, torque off by 1 %% %d" % (len(later), 2 * n * K * T, sum(held), sum(off)))
    assert len(later) >= 0.9 * 2 * n * K * T
    assert np.mean(held) >= 0.5 and np.mean(off) >= 0.5, (np.mean(held), np.mean(off))
