"""Solves with the mass matrix, the parts that need no GPU: the C ABI's declarations (include/rexsim.h) and their ctypes mirror
(rex_gym_amd/_lib.py), the argument checks of the library that come before any launch, the numpy reference of tests/dynamics_solve_ref.py
held to itself -- M x = b, the block elimination against the dense solve, the kinetic energy an impulse gives a robot at rest -- and what it
says about the scenes of tests/test_gpu_dynamics_solve.py: the round-off floors behind that file's bounds."""
import ctypes
import os
import re

import numpy as np
import pytest

import dynamics_ref as dr
import dynamics_solve_ref as sr
import kinematics_ref as kr
from rex_gym_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
CALLS = ("rex_dynamics_solve", "rex_forward_dynamics", "rex_apply_impulse")


def test_header_declares_the_calls_and_the_struct_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert set(CALLS) <= declared
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    body = re.search(r"typedef struct RexDynamicsLoad \{(.*?)\} RexDynamicsLoad;", HEADER, re.S).group(1)
    members = [n.strip(" *") for t, names in re.findall(r"(const float)\s*\*?\s*([^;]+);", body) for n in names.split(",")]
    assert members == ["joint", "toe", "base"] == [f[0] for f in _lib.RexDynamicsLoad._fields_]
    for call, args in (("rex_dynamics_solve", r"RexSim\*[^,]*,\s*const int32_t\*[^,]*,\s*int n,\s*int K,\s*const float\* d_rhs,\s*float\* d_x,\s*void\* stream"),
                       ("rex_forward_dynamics", r"RexSim\*[^,]*,\s*const int32_t\*[^,]*,\s*int n,\s*const RexDynamicsLoad\* load,\s*float\* d_vdot,\s*void\* stream"),
                       ("rex_apply_impulse", r"RexSim\*[^,]*,\s*const int32_t\*[^,]*,\s*int n,\s*const RexDynamicsLoad\* impulse,\s*float\* d_dv[^,]*,\s*void\* stream")):
        flat = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
        assert re.search(r"REX_API int %s\(%s\)" % (call, args), re.sub(r"\s+", " ", flat)), call


def test_lib_binds_them_and_the_unit_is_built():
    assert set(CALLS) <= set(_lib.EXPORTED_SYMBOLS)
    src = open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rexsim.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(RexDynamicsLoad\) == (\d+)", src)
    assert asserted and ctypes.sizeof(_lib.RexDynamicsLoad) == int(asserted.group(1)) == 24 == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert [len(_lib._SIGS[c][0]) for c in CALLS] == [7, 6, 6]
    assert "rex_dynamics_solve.hip" in build.SOURCES
    unit = build.INCLUDED_IN.get("rex_dynamics_solve.hip", "rex_dynamics_solve.hip")          # the object it is compiled into is built
    assert unit in build.SOURCES and unit in [s for s, _, _ in build.variant_jobs()]
    assert "rex_dynamics_leg.h" in build.HEADERS and "rex_dynamics_solve.h" in build.HEADERS


def test_null_and_bad_arguments_are_refused_with_a_message():
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    load = _lib.RexDynamicsLoad(base=p)
    assert L.rex_dynamics_solve(None, None, 1, 1, p, p, None) < 0 and b"rex_dynamics_solve: null sim" in L.rex_last_error()
    assert L.rex_dynamics_solve(None, None, 1, 1, None, p, None) < 0 and b"null pointer" in L.rex_last_error()
    assert L.rex_dynamics_solve(None, None, 1, 1, p, None, None) < 0 and b"null pointer" in L.rex_last_error()
    assert L.rex_forward_dynamics(None, None, 1, ctypes.byref(load), p, None) < 0 and b"rex_forward_dynamics: null sim" in L.rex_last_error()
    assert L.rex_forward_dynamics(None, None, 1, None, p, None) < 0 and b"null pointer" in L.rex_last_error()
    assert L.rex_forward_dynamics(None, None, 1, ctypes.byref(load), None, None) < 0 and b"null pointer" in L.rex_last_error()
    assert L.rex_apply_impulse(None, None, 1, ctypes.byref(load), p, None) < 0 and b"rex_apply_impulse: null sim" in L.rex_last_error()
    assert L.rex_apply_impulse(None, None, 1, None, p, None) < 0 and b"null pointer" in L.rex_last_error()
    assert all(v == 0.0 for v in buf)


# ---------------------------------------------------------------- the reference against itself (float64)
SCALES = (0.9, 1.25)


def _random_state(seed):
    return kr.synthetic_state(np.random.RandomState(seed), False, "random", None, (0.0, 0.0))[:, None].astype(np.float64)


@pytest.mark.parametrize("seed", range(4))
def test_reference_solves_the_equation_and_the_block_elimination_is_the_dense_solve(seed):
    """M_ref x_ref = b to 1e-10 of |b| in the D^-1/2 scaling; the block elimination and the dense Cholesky in float64 equal
    np.linalg.solve to 1e-10 in the error measure of the GPU test (which divides by kappa: looser by nothing that matters here)."""
    s = _random_state(90 + seed)
    r = dr.reference(s, 0, None, SCALES)
    M = r["mass_matrix"]
    B = np.concatenate([sr.rhs_set(r, 5 + seed).astype(np.float64),
                        [sr.load_rhs(r["toe_jacobian"], r["bias"], **sr.pick(sr.loads(3), 1, ("tau", "toe", "wrench")))]])
    X = sr.solve_ref(M, B)
    d = np.sqrt(np.diag(M))
    assert np.all(np.linalg.norm((X @ M - B) / d, axis=-1) <= 1e-10 * np.linalg.norm(B / d, axis=-1))
    _, kappa = sr.conditioning(M)
    assert 1.0 < kappa < 1e4
    assert sr.errors(sr.block_elimination(M, B), X, M).max() * kappa <= 1e-10
    assert sr.errors(sr.dense_cholesky(M, B), X, M).max() * kappa <= 1e-10
    assert sr.errors(X, X, M).max() == 0.0 and sr.errors(X * (1 + 1e-3), X, M).max() == pytest.approx(1e-3 / kappa, rel=1e-6)


@pytest.mark.parametrize("seed", range(4))
def test_an_impulse_from_rest_gains_the_kinetic_energy_of_its_solve(seed):
    """From rest an impulse g (base impulse, toe impulses, joint impulses) gives v = M^-1 g, and the kinetic energy of the links moving
    at v -- summed from kinematics_ref's link velocities, not from M -- is g^T M^-1 g / 2."""
    s = _random_state(95 + seed)
    s[7:13, 0], s[25:37, 0] = 0.0, 0.0
    r = dr.reference(s, 0, None, SCALES)
    g = sr.load_rhs(r["toe_jacobian"], None, **sr.pick(sr.loads(5, seed), 2, ("tau", "toe", "wrench")))
    v = sr.solve_ref(r["mass_matrix"], g)[0]
    s[7:13, 0], s[25:37, 0] = v[0:6], v[6:18]
    lks = dr.links(kr.reference(s, 0, False), SCALES, np.float64)
    T = sum(0.5 * lk["m"] * lk["vc"] @ lk["vc"] + 0.5 * lk["w"] @ lk["I"] @ lk["w"] for lk in lks)
    assert T > 0 and abs(T - 0.5 * g @ v) <= 1e-10 * T


def test_load_rhs_is_the_equation_of_motion():
    """vdot from the forward-dynamics right-hand side satisfies M vdot + h = S^T tau + sum J^T f + w, and the loads broadcast as documented"""
    s = _random_state(99)
    r = dr.reference(s, 0, None, SCALES)
    p = sr.pick(sr.loads(4), 3, ("tau", "toe", "wrench"))
    vdot = sr.solve_ref(r["mass_matrix"], sr.load_rhs(r["toe_jacobian"], r["bias"], **p))[0]
    rhs = np.concatenate([p["wrench"], p["tau"]]) + sum(r["toe_jacobian"][k].T @ p["toe"][k] for k in range(8))
    assert np.abs(r["mass_matrix"] @ vdot + r["bias"] - rhs).max() <= 1e-10 * np.abs(rhs).max()
    free_fall = sr.solve_ref(r["mass_matrix"], sr.load_rhs(r["toe_jacobian"], r["gravity"]))[0]
    assert np.allclose(free_fall[0:3], [0, 0, -dr.G], atol=1e-9) and np.abs(free_fall[3:]).max() <= 1e-9      # gravity alone: every point falls at g


# ---------------------------------------------------------------- what the reference says about the GPU test's scenes
@pytest.fixture(scope="module")
def measured():
    import test_gpu_kinematics as tk
    return sr.measure_floors(tk.BOUNDS["toe_pos"])


def test_bounds_of_the_gpu_test_are_the_stated_multiple_of_the_round_off_floor(measured):
    """Either float32 route against the float64 reference over the synthetic states of the mark-base scenes, with the GPU test's mass scales,
    right-hand sides and loads: the GPU test's bound of each kind is FACTOR (4) x the larger deviation, with 2 % of slack for another libm."""
    import test_gpu_dynamics_solve as ts
    floors, kappa, points, kept = measured
    print({k: "%.3e" % v for k, v in floors.items()}, "kappa %.1f .. %.1f" % kappa, "toe points with a force: %d of %d" % (kept, points))
    assert ts.FACTOR == 4.0 and set(ts.BOUNDS) == set(sr.KINDS)
    for k in sr.KINDS:
        assert 0 < ts.BOUNDS[k] <= ts.FACTOR * floors[k] * 1.02, (k, ts.BOUNDS[k], floors[k])
    assert kept >= 0.9 * points
