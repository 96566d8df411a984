"""The contact solve, the parts that need no GPU: the numpy reference of tests/contact_solve_ref.py held to the C oracle, the round-off
floors behind the bounds of tests/test_gpu_contact_solve.py, what the scenes of that test cover, and the argument checks of
rex_gym_amd/contact.py and of the library that come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import contact_solve_ref as cr
import dynamics_ref as dr
import kinematics_ref as kr
from rex_gym_amd import _lib, build, contact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
VEL_WORDS = list(range(7, 13)) + list(range(25, 37))        # REX_S_LINVEL, REX_S_ANGVEL, REX_S_QD: the order of v
ORACLE_GAP = 5.2e-15          # measured, see test_reference_restates_the_oracle
ORACLE_BOUND = 100 * ORACLE_GAP


# ---------------------------------------------------------------- 1. the reference restates the oracle
@pytest.mark.parametrize("threshold", [0.0, cr.THRESHOLD], ids=["sixty_sweeps", "default_threshold"])
def test_reference_restates_the_oracle(threshold):
    """The synthetic columns of the four plane scenes with mass scales 1 and mu 0.5: v_next of the reference against the velocity words of
    Oracle(np.float64).physics_substep(st, tau, iterations=60, residual_threshold=threshold), relative to max(1, |v|).  Both are float64
    and the formulations differ (dense M and Jacobians in world axes here, an articulated-body recursion in body axes there).
    Measured: 5.2e-15 at both thresholds (318 states); asserted: 100 x that, 5.2e-13 -- five orders under the 1e-7 that would still tell
    the two problems apart.
    Both read the quaternion normalised in float64: the oracle normalises the quaternion it is given and kinematics_ref's forward kinematics
    does not, so on the float32 words as stored (|q| - 1 up to 3e-8) the two poses differ and v_next by 7.3e-7 -- a difference of the
    state that is read, not of the problem, and inside the float32 floor of v_next."""
    import orclib
    oracle = orclib.Oracle(np.float64)
    assert ORACLE_BOUND < 1e-7
    worst, states = 0.0, 0
    for _, n, ground in dr.SCENES:
        if ground != "plane":
            continue
        S, _ = cr.scene_states(n, ground)
        S64 = S.astype(np.float64)
        keep = kr.scene_keep(n)
        S64[3:7, keep:] /= np.linalg.norm(S64[3:7, keep:], axis=0)
        tau, _ = cr.scene_params(n)
        for g in range(keep, n):
            ref = cr.reference(S64, g, tau=tau[g], residual_threshold=threshold)
            st = np.zeros(orclib.STATE_WORDS)
            st[:S64.shape[0]] = S64[:, g]
            want = oracle.physics_substep(st, tau[g], dt=cr.DT, iterations=cr.ITERATIONS, residual_threshold=threshold)[VEL_WORDS]
            worst = max(worst, float(np.abs(ref["v_next"] - want).max() / max(1.0, np.abs(want).max())))
            states += 1
    print("reference against the oracle, threshold %g: %.3e over %d states (bound %.1e)" % (threshold, worst, states, ORACLE_BOUND))
    assert states == 1 + 3 + 63 + 126 and worst <= ORACLE_BOUND


# ---------------------------------------------------------------- 2., 3. floors and coverage of the GPU test's scenes
@pytest.fixture(scope="module")
def measured():
    import test_gpu_kinematics as tk
    return cr.measure_floors(tk.BOUNDS["toe_dist"], tk.BOUNDS["toe_pos"])


def test_bounds_of_the_gpu_test_are_the_stated_multiple_of_the_round_off_floor(measured):
    """reference() in float32 against float64 over the compared synthetic states of every scene, with the GPU test's torques, mass scales
    and friction, 60 sweeps: the GPU test's bound of each field is FACTOR (4) x that deviation, with 2 % of slack for another libm."""
    import test_gpu_contact_solve as tc
    floors, _ = measured
    print({k: "%.3e" % v for k, v in floors.items()})
    assert tc.FACTOR == 4.0 and set(tc.BOUNDS) == set(cr.FIELDS)
    for k in cr.FIELDS:
        assert 0 < tc.BOUNDS[k] <= tc.FACTOR * floors[k] * 1.02, (k, tc.BOUNDS[k], floors[k])


def test_scenes_cover_the_cases(measured):
    """From the reference alone: at least 90 % of every scene's synthetic envs are compared; of the compared envs at least 25 % have four or
    more points in reach, 10 % all four legs, 10 % a limit row; there are sticking and sliding friction rows, and envs that leave the sweep
    loop early and envs that run all 60 sweeps at the default threshold."""
    _, stats = measured
    print(stats)
    for scene, (envs, kept) in stats["scenes"].items():
        assert kept >= 0.9 * envs, (scene, envs, kept)
    n = stats["envs"]
    assert stats["four_points"] >= 0.25 * n and stats["four_legs"] >= 0.10 * n and stats["limit"] >= 0.10 * n, stats
    assert stats["sticking"] > 0 and stats["sliding"] > 0 and stats["early"] > 0 and stats["full"] > 0, stats


def test_reference_result_is_consistent_with_its_own_dynamics():
    """The stance state of the 67-env plane scene with the most loaded toe points: normal impulses are >= 0, friction impulses lie in their boxes, points out of
    reach carry nothing, and M (v_next - v*) is the generalized impulse of the forces and limit torques that are reported."""
    S, kinds = cr.scene_states(67, "plane")
    tau, mu = cr.scene_params(67)
    refs = {g: cr.reference(S, g, mu=float(mu[g]), tau=tau[g]) for g, kind in enumerate(kinds) if kind == "stance"}
    g = max(refs, key=lambda k: int((refs[k]["toe_lambda"][:, 0] > 0).sum()))
    r = refs[g]
    M, J, lam = r["dyn"]["mass_matrix"], r["dyn"]["toe_jacobian"], r["toe_lambda"]
    assert (lam[:, 0] > 0).sum() >= 2 and np.abs(lam[:, 1:]).max() > 0
    assert np.all(lam[:, 0] >= 0) and np.all(np.abs(lam[:, 1:]) <= float(mu[g]) * lam[:, 0:1] * (1 + 1e-12))
    assert np.all(lam[~r["in_reach"]] == 0) and np.all(r["toe_force"][~r["in_reach"]] == 0)
    gen = np.einsum("pcd,pc->d", J, r["toe_force"]) * cr.DT
    gen[6:] += r["limit_torque"] * cr.DT
    assert np.abs(M @ (r["v_next"] - r["v_star"]) - gen).max() <= 1e-10 * max(1.0, np.abs(gen).max())


# ---------------------------------------------------------------- 4. declarations, bindings, argument checks
def test_header_declares_the_call_and_the_structs_and_keeps_the_abi_version():
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    assert re.search(r"REX_API int rex_contact_solve\(RexSim\* sim, const int32_t\* d_env_ids, int n, const RexContactSolveIn\* in, "
                     r"const RexContactSolveOut\* out, void\* stream\)", flat)
    for name, mirror in (("RexContactSolveIn", _lib.RexContactSolveIn), ("RexContactSolveOut", _lib.RexContactSolveOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), flat).group(1)
        assert [m.split()[-1].strip("*") for m in body.split(";") if m.strip()] == [f[0] for f in mirror._fields_], name
    assert [f[0] for f in _lib.RexContactSolveOut._fields_] == list(contact.FIELDS)


def test_lib_binds_it_and_the_unit_is_built():
    assert "rex_contact_solve" in _lib.EXPORTED_SYMBOLS and len(_lib._SIGS["rex_contact_solve"][0]) == 6
    src = open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rexsim.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(RexContactSolveIn\) == (\d+) && sizeof\(RexContactSolveOut\) == (\d+)", src)
    assert asserted and ctypes.sizeof(_lib.RexContactSolveIn) == int(asserted.group(1)) == 24
    assert ctypes.sizeof(_lib.RexContactSolveOut) == int(asserted.group(2)) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert "rex_contact_solve.hip" in build.SOURCES and build.INCLUDED_IN["rex_contact_solve.hip"] == "rex_render.hip"
    assert "rex_contact_solve.hip" in open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rex_render.hip")).read()
    assert {"rex_contact_solve.h", "rex_dynamics_factor.h"} <= set(build.HEADERS)


def test_null_arguments_are_refused_with_a_message():
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    inp, out = _lib.RexContactSolveIn(), _lib.RexContactSolveOut(v_next=ctypes.addressof(buf))
    assert L.rex_contact_solve(None, None, 1, ctypes.byref(inp), ctypes.byref(out), None) < 0 and b"rex_contact_solve: null sim" in L.rex_last_error()
    assert L.rex_contact_solve(None, None, 1, None, ctypes.byref(out), None) < 0 and b"null pointer" in L.rex_last_error()
    assert L.rex_contact_solve(None, None, 1, ctypes.byref(inp), None, None) < 0 and b"null pointer" in L.rex_last_error()
    assert all(v == 0.0 for v in buf)


def test_check_fields_and_settings():
    assert contact.check_fields(None) == tuple(contact.FIELDS) == ("toe_force", "toe_lambda", "limit_torque", "v_next", "sweeps")
    assert contact.check_fields("sweeps") == ("sweeps",)
    assert contact.check_fields(["v_next", "toe_force"]) == ("toe_force", "v_next")          # the order of FIELDS
    for bad in ((), ("toe_forces",), ("v_next", "nope"), ""):
        with pytest.raises(ValueError):
            contact.check_fields(bad)
    assert contact.field_shape("toe_force", 7) == (7, 4, 2, 3) and contact.field_shape("sweeps", 7) == (7,) and contact.field_shape("v_next", 2) == (2, 18)
    assert contact.check_settings(None, None, None) == (0.0, 0, -1.0)                       # the config's
    assert contact.check_settings(0.002, 7, 0) == (0.002, 7, 0.0)
    for kw in (dict(dt=0.0), dict(dt=-1e-3), dict(dt=float("nan")), dict(dt="1"), dict(iterations=0), dict(iterations=1001), dict(iterations=2.0),
               dict(iterations=True), dict(residual_threshold=-1e-9), dict(residual_threshold=float("inf"))):
        with pytest.raises(ValueError):
            contact.check_settings(**{"dt": None, "iterations": None, "residual_threshold": None, **kw})


class _FakeEnv:
    """what contact.solve reads of an env before it touches the device"""
    def __init__(self, mark="base", on_rack=0, body_contacts=0):
        self.mark = mark
        self.config = type("C", (), dict(on_rack=on_rack, body_contacts=body_contacts))()
        self._torch = __import__("torch")


def test_unsupported_envs_and_bad_fields_raise_before_the_device_is_touched():
    with pytest.raises(NotImplementedError):
        contact.solve(_FakeEnv(mark="arm"))
    with pytest.raises(ValueError, match="on_rack"):
        contact.solve(_FakeEnv(on_rack=1))
    with pytest.raises(ValueError, match="body_contacts"):
        contact.solve(_FakeEnv(body_contacts=1))
    with pytest.raises(ValueError, match="fields"):
        contact.solve(_FakeEnv(), fields=("lambda",))
    with pytest.raises(ValueError, match="iterations"):
        contact.solve(_FakeEnv(), iterations=5000)
