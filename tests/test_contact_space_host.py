"""The contact-space readout and inverse dynamics, the parts that need no GPU: the C ABI's declarations (include/rexsim.h) and their ctypes
mirror (rex_gym_amd/_lib.py), the argument checks of the library that come before any launch, the numpy reference of
tests/contact_space_ref.py held to itself -- the drift against a central difference of J(q(t)) v, the Delassus matrix symmetric positive
semidefinite, inverse dynamics undoing forward dynamics -- and what it says about the scenes of tests/test_gpu_contact_space.py: the
round-off floors behind that file's bounds."""
import ctypes
import os
import re

import numpy as np
import pytest

import contact_space_ref as cs
import dynamics_ref as dr
import dynamics_solve_ref as sr
import kinematics_ref as kr
from rex_gym_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
CALLS = ("rex_inverse_dynamics", "rex_contact_space")


def test_header_declares_the_calls_and_the_struct_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert set(CALLS) <= declared
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    body = re.search(r"typedef struct RexContactSpaceOut \{(.*?)\} RexContactSpaceOut;", HEADER, re.S).group(1)
    members = re.findall(r"float\s*\*\s*(\w+)\s*;", body)
    assert members == ["delassus", "toe_drift", "toe_acc_free"] == [f[0] for f in _lib.RexContactSpaceOut._fields_]
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S))
    for call, args in (("rex_inverse_dynamics", r"RexSim\* sim, const int32_t\* d_env_ids, int n, const float\* d_vdot\s*, const RexDynamicsLoad\* load\s*, float\* d_force, void\* stream"),
                       ("rex_contact_space", r"RexSim\* sim, const int32_t\* d_env_ids, int n, const float\* d_tau\s*, const float\* d_base_wrench\s*, const RexContactSpaceOut\* out, void\* stream")):
        assert re.search(r"REX_API int %s\(%s\)" % (call, args), flat), call


def test_lib_binds_them_and_the_unit_is_built():
    assert set(CALLS) <= set(_lib.EXPORTED_SYMBOLS)
    src = open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rexsim.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(RexContactSpaceOut\) == (\d+)", src)
    assert asserted and ctypes.sizeof(_lib.RexContactSpaceOut) == int(asserted.group(1)) == 24 == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert [len(_lib._SIGS[c][0]) for c in CALLS] == [7, 7]
    assert "rex_contact_space.hip" in build.SOURCES and build.INCLUDED_IN["rex_contact_space.hip"] == "rex_render.hip"
    assert "rex_contact_space.hip" in open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rex_render.hip")).read()
    assert {"rex_contact_space.h", "rex_dynamics_factor.h", "rex_dynamics_leg.h", "rex_toe_point.h"} <= set(build.HEADERS)


def test_null_and_bad_arguments_are_refused_with_a_message():
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    out, empty, load = _lib.RexContactSpaceOut(toe_drift=p), _lib.RexContactSpaceOut(), _lib.RexDynamicsLoad(base=p)
    assert L.rex_inverse_dynamics(None, None, 1, p, ctypes.byref(load), p, None) < 0 and b"rex_inverse_dynamics: null sim" in L.rex_last_error()
    assert L.rex_inverse_dynamics(None, None, 1, None, None, p, None) < 0 and b"rex_inverse_dynamics: null sim" in L.rex_last_error()
    assert L.rex_inverse_dynamics(None, None, 1, p, ctypes.byref(load), None, None) < 0 and b"null pointer" in L.rex_last_error()
    assert L.rex_contact_space(None, None, 1, None, None, ctypes.byref(out), None) < 0 and b"rex_contact_space: null sim" in L.rex_last_error()
    assert L.rex_contact_space(None, None, 1, p, p, ctypes.byref(empty), None) < 0 and b"rex_contact_space: null sim" in L.rex_last_error()
    assert L.rex_contact_space(None, None, 1, p, p, None, None) < 0 and b"null pointer" in L.rex_last_error()
    assert all(v == 0.0 for v in buf)


# ---------------------------------------------------------------- the reference against itself (float64)
SCALES = (0.9, 1.25)
STEP = 1e-4          # s: the difference quotient's step


def _random_state(seed):
    return kr.synthetic_state(np.random.RandomState(seed), False, "random", None, (0.0, 0.0))[:, None].astype(np.float64)


def _point_velocities(s0, h):
    """[8, 3]: J(q(t0 + h)) v of the foot links' material points that are the toe points at t0, the state moved along its own (constant)
    velocities; the points are held in the foot links' frames, the ground is not queried again"""
    k0 = kr.reference(s0, 0, False)
    k1 = kr.reference(kr.advance(s0, 0, False, h)[:, None], 0, False)
    out = np.zeros((8, 3))
    for p in range(8):
        foot = 3 * (p // 2) + 3
        local = k0["link_rot"][foot].T @ (k0["toe_pos"][p] - k0["link_pos"][foot])
        out[p] = k1["link_linvel"][foot] + np.cross(k1["link_angvel"][foot], k1["link_rot"][foot] @ local)
    return out


@pytest.mark.parametrize("seed", range(5))
def test_drift_is_the_rate_of_the_toe_velocity_at_constant_generalized_velocity(seed):
    """drift = d/dt (J(q(t)) v) with v held constant, by a central difference at STEP and at twice STEP: the two quotients agree to 1e-6 of the
    scale (the quotient has converged: its truncation error falls with the square of the step), and so does the recursion."""
    s = _random_state(300 + seed)
    want = cs.drift(kr.reference(s, 0, False))
    scale = max(1.0, float(np.abs(want).max()))
    fine = (_point_velocities(s, STEP) - _point_velocities(s, -STEP)) / (2 * STEP)
    coarse = (_point_velocities(s, 2 * STEP) - _point_velocities(s, -2 * STEP)) / (4 * STEP)
    assert np.abs(want).max() > 1.0                                          # joint rates of up to 5 rad/s: there is a drift to compare
    assert np.abs(fine - coarse).max() <= 1e-6 * scale
    assert np.abs(fine - want).max() <= 1e-6 * scale


def test_drift_of_a_robot_at_rest_is_zero_and_of_a_spinning_rigid_robot_centripetal():
    s = _random_state(310)
    s[7:13, 0], s[25:37, 0] = 0.0, 0.0
    assert not cs.drift(kr.reference(s, 0, False)).any()
    s[10:13, 0] = [0.3, -0.2, 2.0]
    k = kr.reference(s, 0, False)
    w = s[10:13, 0]
    want = np.array([np.cross(w, np.cross(w, P - k["link_pos"][0])) for P in k["toe_pos"]])
    assert np.abs(cs.drift(k) - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("seed", range(4))
def test_delassus_is_symmetric_positive_semidefinite_and_the_free_acceleration_is_the_forward_one(seed):
    s = _random_state(320 + seed)
    p = sr.pick(sr.loads(4, seed), 2, ("tau", "toe", "wrench"))
    r = cs.reference(s, 0, None, SCALES, tau=p["tau"], wrench=p["wrench"])
    W, d = r["delassus"], r["dyn"]
    assert np.abs(W - W.T).max() <= 1e-12 * np.abs(W).max()
    eig = np.linalg.eigvalsh(0.5 * (W + W.T))
    assert eig.min() >= -1e-10 * eig.max() and (eig > 1e-8 * eig.max()).sum() <= 18        # rank: at most the 18 degrees of freedom
    vdot = sr.solve_ref(d["mass_matrix"], sr.load_rhs(d["toe_jacobian"], d["bias"], **p))[0]
    acc = d["toe_jacobian"].reshape(24, 18) @ vdot + r["toe_drift"].reshape(24)
    want = r["toe_acc_free"].reshape(24) + W @ p["toe"].reshape(24).astype(np.float64)
    assert np.abs(acc - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("seed", range(4))
def test_inverse_dynamics_undoes_forward_dynamics(seed):
    """inverse(forward(load), load) = 0, inverse(forward(tau, f, w), f, w) = (0, tau), inverse() = h, and the float32 routes stay within 1e-4 in
    the measure of the GPU test"""
    s = _random_state(330 + seed)
    d = dr.reference(s, 0, None, SCALES)
    M, h, J = d["mass_matrix"], d["bias"], d["toe_jacobian"]
    p = sr.pick(sr.loads(4, seed), 1, ("tau", "toe", "wrench"))
    vdot = sr.solve_ref(M, sr.load_rhs(J, h, **p))[0]
    scale = np.abs(h).max()
    assert np.abs(cs.inverse(M, h, J, vdot=vdot, **p)).max() <= 1e-10 * scale
    need = cs.inverse(M, h, J, vdot=vdot, toe=p["toe"], wrench=p["wrench"])
    assert np.abs(need - np.concatenate([np.zeros(6), p["tau"]])).max() <= 1e-10 * scale
    assert np.array_equal(cs.inverse(M, h, J), h)
    _, routes = cs.routes32(s, 0, None, SCALES)
    for _, M32, h32, J32, _, _ in routes:
        got = cs.inverse(M32, h32, J32, vdot=vdot.astype(np.float32), f=np.float32, **p)
        assert got.dtype == np.float32 and cs.force_errors(got, cs.inverse(M, h, J, vdot=vdot.astype(np.float32), **p), d).max() <= 1e-4


def test_error_measures_scale_as_documented():
    s = _random_state(340)
    r = cs.reference(s, 0, None, SCALES)
    _, kappa = sr.conditioning(r["dyn"]["mass_matrix"])
    e = cs.errors({"delassus": r["delassus"] * (1 + 1e-3), "toe_drift": r["toe_drift"] + 1e-3, "toe_acc_free": r["toe_acc_free"]}, r)
    assert np.diag(e["delassus"]) == pytest.approx(1e-3 / kappa, rel=1e-6) and e["delassus"].shape == (24, 24)
    assert e["toe_drift"] == pytest.approx(1e-3 / max(10.0, np.abs(r["toe_drift"]).max()), rel=1e-6) and not e["toe_acc_free"].any()
    assert cs.point_mask(np.array([1, 0, 1, 1, 1, 1, 1, 1], bool)).sum() == 21 * 21


# ---------------------------------------------------------------- what the reference says about the GPU test's scenes
@pytest.fixture(scope="module")
def measured():
    import test_gpu_kinematics as tk
    return cs.measure_floors(tk.BOUNDS["toe_pos"])


def test_bounds_of_the_gpu_test_are_the_stated_multiple_of_the_round_off_floor(measured):
    """Either float32 route against the float64 reference over the synthetic states of the mark-base scenes, with the GPU test's mass scales,
    loads and accelerations: the GPU test's bound of each kind is FACTOR (4) x the larger deviation, with 2 % of slack for another libm."""
    import test_gpu_contact_space as tc
    floors, points, kept = measured
    print({k: "%.3e" % v for k, v in floors.items()}, "toe points kept: %d of %d" % (kept, points))
    assert tc.FACTOR == 4.0 and set(tc.BOUNDS) == set(cs.KINDS)
    for k in cs.KINDS:
        assert 0 < tc.BOUNDS[k] <= tc.FACTOR * floors[k] * 1.02, (k, tc.BOUNDS[k], floors[k])
        assert tc.BOUNDS[k] >= tc.FACTOR * floors[k] * 0.98, (k, tc.BOUNDS[k], floors[k])
    assert kept >= 0.9 * points
