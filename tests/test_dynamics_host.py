"""Rigid-body dynamics readout, the parts that need no GPU: the C ABI's declarations (include/rexsim.h) and their ctypes mirror
(rex_gym_amd/_lib.py), the argument checks of the library that come before any launch, and the numpy reference of
tests/dynamics_ref.py held to itself -- its mass matrix against the kinetic energy of kinematics_ref's link velocities, its gravity
vector against the derivative of the potential energy, its bias against finite-difference accelerations, the power identities, its
two routes against each other, its toe Jacobians against kinematics_ref's toe velocities -- and what it says about the scenes of
tests/test_gpu_dynamics.py: the round-off floors behind that file's bounds and the share of toe points its comparison leaves out."""
import ctypes
import os
import re

import numpy as np
import pytest

import dynamics_ref as dr
import kinematics_ref as kr
from rex_gym_amd import _lib, build, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
MEMBERS = ["mass_matrix", "bias", "gravity", "toe_jacobian", "com", "momentum", "mass"]


def test_header_declares_the_struct_and_the_call_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert "rex_dynamics" in declared
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    body = re.search(r"typedef struct RexDynamicsOut \{(.*?)\} RexDynamicsOut;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, [n.strip(" *") for n in names.split(",")]) for t, names in re.findall(r"(float|uint8_t)\s*\*?\s*([^;]+);", body)]
    assert [n for _, names in fields for n in names] == MEMBERS
    assert all(t == "float" for t, _ in fields)


def test_lib_binds_it_and_the_struct_has_the_size_the_library_asserts():
    assert "rex_dynamics" in _lib.EXPORTED_SYMBOLS
    assert [f[0] for f in _lib.RexDynamicsOut._fields_] == MEMBERS == list(dynamics.FIELDS) == list(dr.FIELDS)
    src = open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rexsim.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(RexDynamicsOut\) == (\d+)", src)
    assert asserted and ctypes.sizeof(_lib.RexDynamicsOut) == int(asserted.group(1)) == 56 == 7 * ctypes.sizeof(ctypes.c_void_p)
    assert "rex_dynamics.hip" in build.SOURCES
    unit = build.INCLUDED_IN.get("rex_dynamics.hip", "rex_dynamics.hip")          # the object it is compiled into is built
    assert unit in build.SOURCES and unit in [s for s, _, _ in build.variant_jobs()]


def test_dof_names_come_from_the_model_tables():
    names = dynamics.dof_names()
    assert len(names) == 18 and names[:6] == dynamics.BASE_DOF_NAMES
    assert names[6:9] == ("motor_front_left_shoulder", "motor_front_left_leg", "foot_motor_front_left") and names[17] == "foot_motor_rear_right"
    with pytest.raises(ValueError):
        dynamics.check_fields(["bias", "toe_force"])
    with pytest.raises(ValueError):
        dynamics.check_fields([])
    assert dynamics.check_fields(("com", "bias")) == ("bias", "com") and dynamics.check_fields(None) == tuple(MEMBERS)
    assert dynamics.field_shape("toe_jacobian", 5) == (5, 4, 2, 3, 18) and dynamics.field_shape("mass", 5) == (5,)


def test_null_arguments_are_refused_with_a_message():
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    out = _lib.RexDynamicsOut(bias=ctypes.addressof(buf))
    assert L.rex_dynamics(None, None, 1, ctypes.byref(out), None) < 0 and b"null sim" in L.rex_last_error()
    assert L.rex_dynamics(None, None, 1, None, None) < 0 and b"null pointer" in L.rex_last_error()
    assert all(v == 0.0 for v in buf)


# ---------------------------------------------------------------- the reference against itself (float64)
SCALES = (0.9, 1.25)
H = 1e-6


def _random_state(seed):
    return kr.synthetic_state(np.random.RandomState(seed), False, "random", None, (0.0, 0.0))[:, None].astype(np.float64)


def _with_velocity(s, v):
    s = s.copy()
    s[7:13, 0], s[25:37, 0] = v[0:6], v[6:18]
    return s


def _velocity(s):
    return np.concatenate([s[7:13, 0], s[25:37, 0]])


def _energies(s):
    """(kinetic, potential) energy summed over links from kinematics_ref.reference's own poses and link velocities"""
    lks = dr.links(kr.reference(s, 0, False), SCALES, np.float64)
    return (sum(0.5 * lk["m"] * lk["vc"] @ lk["vc"] + 0.5 * lk["w"] @ lk["I"] @ lk["w"] for lk in lks), dr.G * sum(lk["m"] * lk["c"][2] for lk in lks))


def _advanced(s, h):
    return kr.advance(s, 0, False, h)[:, None]


@pytest.mark.parametrize("seed", range(4))
def test_reference_mass_matrix_is_the_kinetic_energy(seed):
    """M_ij = T(e_i + e_j) - T(e_i) - T(e_j), T the kinetic energy of the links at unit generalized velocities, to 1e-12 of sqrt(M_ii M_jj)"""
    s = _random_state(50 + seed)
    M = dr.reference(s, 0, None, SCALES)["mass_matrix"]
    eye = np.eye(18)
    T1 = [_energies(_with_velocity(s, eye[i]))[0] for i in range(18)]
    for i in range(18):
        assert abs(2 * T1[i] - M[i, i]) <= 1e-12 * M[i, i]
        for j in range(i):
            want = _energies(_with_velocity(s, eye[i] + eye[j]))[0] - T1[i] - T1[j]
            bound = 1e-12 * np.sqrt(M[i, i] * M[j, j])
            assert abs(want - M[i, j]) <= bound and abs(want - M[j, i]) <= bound, (i, j)
    assert np.linalg.eigvalsh(M).min() > 0


@pytest.mark.parametrize("seed", range(4))
def test_reference_gravity_is_the_gradient_of_the_potential_energy(seed):
    """gravity_i is the central difference of 10 sum m_b z_b along advance() at the unit velocity e_i (for the base rotation: a turn about a
    world axis through the base origin), h = 1e-6, to 1e-6 of the block's scale"""
    s = _random_state(60 + seed)
    r = dr.reference(s, 0, None, SCALES)
    assert np.array_equal(r["gravity"], dr.reference(_with_velocity(s, np.zeros(18)), 0, None, SCALES)["bias"])        # h(q, 0)
    fd = np.array([(_energies(_advanced(_with_velocity(s, e), H))[1] - _energies(_advanced(_with_velocity(s, e), -H))[1]) / (2 * H) for e in np.eye(18)])
    assert dr.errors(dict(gravity=fd), r)["gravity"].max() <= 1e-6
    assert np.allclose(r["gravity"][0:3], [0, 0, 10 * r["mass"]], atol=1e-12)


@pytest.mark.parametrize("seed", range(4))
def test_reference_bias_against_finite_difference_accelerations(seed):
    """bias is the J_b^T [m_b (a_b + g z); I_b alpha_b + w_b x I_b w_b] sum with the accelerations taken as central differences of
    kinematics_ref's link velocities between advance(+h) and advance(-h) at constant velocity words, to 1e-6 of the block's scale"""
    s = _random_state(70 + seed)
    r = dr.reference(s, 0, None, SCALES)
    lks = dr.links(r["kin"], SCALES, np.float64)
    plus, minus = (dr.links(kr.reference(_advanced(s, h), 0, False), SCALES, np.float64) for h in (H, -H))
    acc = [((p["vc"] - m["vc"]) / (2 * H), (p["w"] - m["w"]) / (2 * H)) for p, m in zip(plus, minus)]
    jac = [dr.link_jacobians(lk, r["kin"]["link_pos"][0], np.float64) for lk in lks]
    assert dr.errors(dict(bias=dr.project(lks, jac, acc, np.float64)), r)["bias"].max() <= 1e-6


@pytest.mark.parametrize("seed", range(4))
def test_reference_power_identities_routes_and_toe_jacobians(seed):
    """v . gravity = 10 mass com_vel_z (the rate of the potential energy) to 1e-10.  v . (bias - gravity) is the rate at which the kinetic
    energy changes at zero generalized acceleration, (1/2) v^T Mdot v: the velocity-dependent forces of these coordinates are not
    workless one by one (world-frame base velocities and joint rates: v^T (Mdot - 2 C) v = 0, so v^T C v = v^T Mdot v / 2), and the
    test holds it to the central difference of T along advance() at constant velocity words (on these four states it is -0.010, 3.251,
    0.430 and 0.274 W next to sum |v_i| |bias_i| of 21.9, 10.5, 44.8 and 31.6 W: not 0).  The two routes agree to 1e-12; J_p v is
    kinematics_ref's toe_vel[p]; M v gives the momentum."""
    s = _random_state(80 + seed)
    r, c = dr.reference(s, 0, None, SCALES), dr.reference_composite(s, 0, None, SCALES)
    v = _velocity(s)
    assert abs(v @ r["gravity"] - 10 * r["mass"] * r["com"][5]) <= 1e-10 * max(1.0, abs(v @ r["gravity"]))
    t_rate = (_energies(_advanced(s, H))[0] - _energies(_advanced(s, -H))[0]) / (2 * H)
    assert abs(v @ (r["bias"] - r["gravity"]) - t_rate) <= 1e-6 * np.abs(v * r["bias"]).sum()
    assert abs(0.5 * v @ r["mass_matrix"] @ v - _energies(s)[0]) <= 1e-12 * _energies(s)[0]
    e = dr.errors(c, r)
    assert e["mass_matrix"].max() <= 1e-12 and e["bias"].max() <= 1e-12 and e["gravity"].max() <= 1e-12
    assert np.abs(r["toe_jacobian"] @ v - r["kin"]["toe_vel"]).max() <= 1e-12
    p = r["mass_matrix"] @ v
    C = r["com"][0:3] - s[0:3, 0]
    assert np.abs(p[0:3] - r["momentum"][0:3]).max() <= 1e-12 and np.abs(p[3:6] - np.cross(C, p[0:3]) - r["momentum"][3:6]).max() <= 1e-12
    assert np.allclose(r["com"][3:6] * r["mass"], r["momentum"][0:3], atol=1e-12)


def test_reference_at_rest_and_mass_scales():
    """A level robot at rest: bias = gravity, bias[0:3] = (0, 0, +mass * 10).  The scales multiply the masses and nothing else: the rotational
    block of a base scaled by 2 grows by the legs' point masses only."""
    s = np.zeros((37, 1), np.float64)
    s[6] = 1.0
    s[2] = 0.25
    r = dr.reference(s, 0, None, (1.0, 1.0))
    total = float(re.search(r"#define\s+REX_TOTAL_MASS\s+([\d.]+)", open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rex_model_gen.h")).read()).group(1))
    assert abs(r["mass"] - total) <= 1e-12 and np.array_equal(r["bias"], r["gravity"]) and np.allclose(r["bias"][0:3], [0, 0, 10 * total], atol=1e-12)
    assert np.all(r["momentum"] == 0) and np.all(r["com"][3:6] == 0)
    r2 = dr.reference(s, 0, None, (2.0, 1.0))
    assert abs(r2["mass"] - (total + dr.MASS[0])) <= 1e-12
    assert np.allclose(r2["mass_matrix"][3:6, 3:6], r["mass_matrix"][3:6, 3:6], atol=1e-15)          # the base's centre of mass is its origin
    assert np.allclose(r2["mass_matrix"][6:, 6:], r["mass_matrix"][6:, 6:], atol=1e-15)


# ---------------------------------------------------------------- what the reference says about the GPU test's scenes
@pytest.fixture(scope="module")
def measured():
    import test_gpu_kinematics as tk
    return dr.measure_floors(tk.BOUNDS["toe_pos"])


def test_bounds_of_the_gpu_test_are_the_stated_multiple_of_the_round_off_floor(measured):
    """Either route of the reference in float32 against reference() in float64 over the synthetic states of the mark-base scenes, with the
    GPU test's per-env mass scales: the GPU test's bound of each field is FACTOR x the larger deviation (4 x: the kernel's operation order is
    neither route's), with 2 % of slack for another libm."""
    import test_gpu_dynamics as td
    floors, points, kept = measured
    print({k: "%.3e" % v for k, v in floors.items()}, "kept %d of %d" % (kept, points))
    assert set(td.BOUNDS) == set(dr.FIELDS) == set(td.FACTOR)
    for k in dr.FIELDS:
        assert td.FACTOR[k] == 4.0 or (k == "bias" and td.FACTOR[k] <= 16.0)
        assert 0 < td.BOUNDS[k] <= td.FACTOR[k] * floors[k] * 1.02, (k, td.BOUNDS[k], floors[k])


def test_reference_alone_keeps_nine_tenths_of_the_toe_points(measured):
    _, points, kept = measured
    print("kept %d of %d" % (kept, points))
    assert kept >= 0.9 * points, (kept, points)
