"""Body and foot kinematics, the parts that need no GPU: the C ABI's declarations (include/rexsim.h) and their ctypes mirror
(rex_gym_amd/_lib.py), the argument checks of the library that come before any launch, and the numpy reference of
tests/kinematics_ref.py held to itself -- its velocities against central differences of its own forward kinematics (which pins the
frames and the reference points before any GPU is involved), its toe points on a level standing pose, and what it says about the scenes
of tests/test_gpu_kinematics.py: the round-off floors behind that file's bounds, the share of points its comparisons leave out, and
the cases the kept ones cover."""
import ctypes
import os
import re

import numpy as np
import pytest

import kinematics_ref as kr
import test_gpu_render as col
from rex_gym_amd import _lib, build, kinematics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
ENTRY_POINTS = ("rex_num_bodies", "rex_kinematics")
MEMBERS = ["link_pos", "link_quat", "link_linvel", "link_angvel", "toe_pos", "toe_vel", "toe_dist", "toe_normal", "toe_in_reach", "base_body"]


def test_header_declares_the_struct_and_both_calls_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert set(ENTRY_POINTS) <= declared
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    body = re.search(r"typedef struct RexKinematicsOut \{(.*?)\} RexKinematicsOut;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, [n.strip(" *") for n in names.split(",")]) for t, names in re.findall(r"(float|uint8_t)\s*\*?\s*([^;]+);", body)]
    assert [n for _, names in fields for n in names] == MEMBERS
    assert [t for t, names in fields for _ in names] == ["float"] * 8 + ["uint8_t", "float"]


def test_lib_binds_them_and_the_struct_has_the_size_the_library_asserts():
    assert set(ENTRY_POINTS) <= set(_lib.EXPORTED_SYMBOLS)
    assert [f[0] for f in _lib.RexKinematicsOut._fields_] == MEMBERS == list(kinematics.FIELDS)
    src = open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rexsim.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(RexKinematicsOut\) == (\d+)", src)
    assert asserted and ctypes.sizeof(_lib.RexKinematicsOut) == int(asserted.group(1)) == 10 * ctypes.sizeof(ctypes.c_void_p)
    assert "rex_kinematics.hip" in build.SOURCES
    unit = build.INCLUDED_IN.get("rex_kinematics.hip", "rex_kinematics.hip")          # the object it is compiled into is built
    assert unit in build.SOURCES and unit in [s for s, _, _ in build.variant_jobs()]


def test_body_names_come_from_the_model_tables():
    base, arm = kinematics.body_names("base"), kinematics.body_names("arm")
    assert len(base) == 13 and len(arm) == 19 and arm[:13] == base
    assert base[0] == "base_link" and base[1:4] == ("front_left_shoulder_link", "front_left_leg_link", "front_left_foot_link")
    assert base[12] == "rear_right_foot_link" and arm[13] == "arm_long_U" and arm[18] == "arm_section_5"
    with pytest.raises(ValueError):
        kinematics.check_fields(["toe_pos", "toe_force"])
    with pytest.raises(ValueError):
        kinematics.check_fields([])
    assert kinematics.check_fields(("toe_dist", "link_pos")) == ("link_pos", "toe_dist") and kinematics.check_fields(None) == tuple(MEMBERS)


def test_null_arguments_are_refused_with_a_message():
    if not os.path.exists(build.LIB_PATH) or build.needs_build():
        pytest.skip("the library is not built")
    L = _lib.lib()
    cfg = _lib.RexConfig()
    assert L.rex_default_config(_lib.TASKS["walk"], _lib.SIGNALS["ik"], 3, ctypes.byref(cfg)) == 0
    assert L.rex_num_bodies(ctypes.byref(cfg)) == 13
    cfg.mark = _lib.MARKS["arm"]
    assert L.rex_num_bodies(ctypes.byref(cfg)) == 19 and L.rex_num_bodies(None) < 0
    buf = (ctypes.c_float * 64)()
    out = _lib.RexKinematicsOut(toe_dist=ctypes.addressof(buf))
    assert L.rex_kinematics(None, None, 1, ctypes.byref(out), None) < 0 and b"null sim" in L.rex_last_error()
    assert L.rex_kinematics(None, None, 1, None, None) < 0 and b"null pointer" in L.rex_last_error()
    assert all(v == 0.0 for v in buf)


# ---------------------------------------------------------------- the reference against itself
def _random_state(arm, seed):
    rng = np.random.RandomState(seed)
    return kr.synthetic_state(rng, arm, "random", None, (0.0, 0.0))[:, None]


@pytest.mark.parametrize("arm", [False, True])
def test_reference_velocities_are_the_derivative_of_its_forward_kinematics(arm):
    """Advance a random state by h = 1e-6 s both ways (position by the linear velocity, the quaternion by the exponential of w h, the joint
    angles by their rates): (fk(s+) - fk(s-)) / 2h is the reference's link and toe-centre velocity to 1e-6 relative, and the rotation's
    derivative is [w]x R.  float64 throughout: fk() is handed float64 states."""
    h = 1e-6
    for seed in range(4):
        s = _random_state(arm, 40 + seed).astype(np.float64)
        r = kr.reference(s, 0, arm)
        plus, minus = kr.advance(s, 0, arm, h)[:, None], kr.advance(s, 0, arm, -h)[:, None]
        (Rp, op), (Rm, om) = col.fk(plus, 0, arm), col.fk(minus, 0, arm)
        for b in range(len(op)):
            v = (op[b] - om[b]) / (2 * h)
            assert np.linalg.norm(v - r["link_linvel"][b]) <= 1e-6 * max(1.0, np.linalg.norm(v)), (seed, b)
            W = (Rp[b] - Rm[b]) / (2 * h) @ r["link_rot"][b].T           # [w]x
            w = np.array([W[2, 1], W[0, 2], W[1, 0]])
            assert np.linalg.norm(w - r["link_angvel"][b]) <= 1e-6 * max(1.0, np.linalg.norm(w)), (seed, b)
        for leg, k in enumerate(kr.TOE_PRIMS):
            b = int(col.P_BODY[k])
            v = ((op[b] + Rp[b] @ col.P_POS[k]) - (om[b] + Rm[b] @ col.P_POS[k])) / (2 * h)
            assert np.linalg.norm(v - r["toe_centre_vel"][leg]) <= 1e-6 * max(1.0, np.linalg.norm(v)), (seed, leg)
        # toe_vel is the foot link's material point at toe_pos
        for p in range(8):
            b = 3 + 3 * (p // 2)
            local = r["link_rot"][b].T @ (r["toe_pos"][p] - r["link_pos"][b])
            v = ((op[b] + Rp[b] @ local) - (om[b] + Rm[b] @ local)) / (2 * h)
            assert np.linalg.norm(v - r["toe_vel"][p]) <= 1e-6 * max(1.0, np.linalg.norm(v)), (seed, p)
        assert np.allclose(r["base_body"][0:3], r["link_rot"][0].T @ s[7:10, 0], atol=1e-15)
        assert np.allclose(r["base_body"][6:9], -r["link_rot"][0][2], atol=1e-15)


def test_reference_toe_points_on_a_level_standing_pose():
    """Level base, legs straight down: on the plane every toe point lies straight under its end's centre, a radius (with the margin) lower;
    toe_dist is its z, the normal +z, and the point is in reach exactly below the breaking threshold."""
    s = np.zeros((37, 1), np.float32)
    s[6] = 1.0
    for z, reach in ((0.25, True), (0.28, False)):
        s[2] = z
        r = kr.reference(s, 0, False)
        assert np.array_equal(r["toe_dist"], r["toe_pos"][:, 2]) and np.all(r["toe_normal"] == [0, 0, 1])
        assert np.all(r["fid0"] == 0) and np.all(r["fid1"] == 0) and not r["degenerate"].any()
        radius = float(col.P_EXT[kr.TOE_PRIMS[0]][0]) + kr.MARGIN
        for p in range(8):
            centre = r["toe_centre"][p // 2]
            assert np.allclose(r["toe_pos"][p], centre + [0, (-1 if p % 2 == 0 else 1) * float(col.P_EXT[kr.TOE_PRIMS[0]][2]), -radius], atol=1e-12)
        assert np.all(r["toe_in_reach"] == reach), (z, r["toe_dist"])


# ---------------------------------------------------------------- what the reference says about the GPU test's scenes
@pytest.fixture(scope="module")
def measured():
    return kr.measure_floors()


def test_bounds_of_the_gpu_test_are_four_times_the_round_off_floor(measured):
    """The float32 reference against the float64 one over the synthetic states of every scene: the GPU test's bound of each field is 4 x the
    largest deviation (the kernel's operation order is not numpy's, and the chain is three to nine rotations deep).  The constants there are
    the numbers measured here; 2 % of slack for another libm."""
    import test_gpu_kinematics as tk
    floors, shift, points, kept = measured
    print({k: "%.3e" % v for k, v in floors.items()}, "shift %.3e" % shift, "kept %d of %d" % (kept, points))
    assert set(tk.BOUNDS) == set(kr.FLOAT_FIELDS)
    for k in kr.FLOAT_FIELDS:
        assert 0 < tk.BOUNDS[k] <= 4.0 * floors[k] * 1.02, (k, tk.BOUNDS[k], floors[k])
    assert tk.BOUNDS["toe_pos"] <= shift * 1.02


def test_reference_alone_keeps_nine_tenths_of_the_points_and_covers_the_cases(measured):
    import test_gpu_kinematics as tk
    _, _, points, kept = measured
    assert kept >= 0.9 * points, (kept, points)
    seen = {}
    for mark, n, ground in kr.SCENES:
        if n >= 67:
            tk.count_cases(tk.scene_reference(mark, n, ground, None), seen)
    tk.assert_cases_cover(seen)


# ---------------------------------------------------------------- fields= and out= of the four readouts (rex_gym_amd/readout.py behind each module)
# module name -> (the query's name in its messages, how a message shows float32, the fields that are not float32: how it shows their dtype)
READOUTS = {"kinematics": ("kinematics", "torch.float32", {"toe_in_reach": "torch.uint8"}), "dynamics": ("dynamics", "float32", {}),
            "contact": ("contact_solve", "float32", {"sweeps": "int32"}), "contact_space": ("contact_space", "float32", {})}


def _readout(module):
    """-> (the module, its result class, a stub env on the CPU, the shape of every field at 5 rows and 13 bodies)"""
    import importlib
    import torch
    mod = importlib.import_module("rex_gym_amd." + module)
    cls = next(v for v in vars(mod).values() if isinstance(v, type) and v.__module__ == mod.__name__)
    env = type("StubEnv", (), dict(_torch=torch, device=torch.device("cpu"), num_bodies=13))()
    shapes = {n: mod.field_shape(n, 5, 13) if module == "kinematics" else mod.field_shape(n, 5) for n in mod.FIELDS}
    return mod, cls, env, shapes


def _result(module):
    import torch
    mod, cls, env, shapes = _readout(module)
    shown = READOUTS[module][2]
    return cls({n: torch.zeros(shapes[n], dtype=getattr(torch, shown.get(n, "float32").split(".")[-1])) for n in mod.FIELDS})


@pytest.mark.parametrize("module", list(READOUTS))
def test_every_readout_refuses_bad_fields_and_results_with_its_own_messages(module):
    """What check_fields and check_result of each of the four modules refuse, and the words they refuse it with: an unknown field, an empty
    field list, a result of another query or of other fields, and per field a wrong dtype, a wrong row count and a tensor that is not the
    one the struct points to."""
    import torch
    mod, cls, env, shapes = _readout(module)
    who, f32, shown = READOUTS[module]
    names = tuple(mod.FIELDS)
    for bad in (("nope",), (names[0], "nope"), ()):
        with pytest.raises(ValueError) as e:
            mod.check_fields(bad)
        assert str(e.value) == f"{who}: fields must be a non-empty subset of {names}, got {bad}"
    out = _result(module)
    assert out.fields == names and out.rows == 5 and mod.check_result(out, names, 5, env) is None
    other = _result("dynamics" if module != "dynamics" else "contact_space")
    for wrong, want in ((other, names), (out, names[:1]), (None, names)):
        with pytest.raises(ValueError) as e:
            mod.check_result(wrong, want, 5, env)
        assert str(e.value) == f"{who}: out must be a result of {who}() with the fields {want}"
    for n in names:
        def refused(k):
            with pytest.raises(ValueError) as e:
                mod.check_result(out, names, k, env)
            return str(e.value) == f"{who}: out.{n} must be the contiguous {shown.get(n, f32)} tensor of shape {(k,) + shapes[n][1:]} on cpu the result was made with"
        good = getattr(out, n)
        if n == names[0]:
            assert refused(6)                                                      # the row count: the first field reports it
        same_bytes = {torch.float32: torch.int32, torch.int32: torch.float32, torch.uint8: torch.int8}[good.dtype]
        for bad in (good.view(same_bytes), good.clone(), None):                     # the dtype alone; another tensor; no tensor
            setattr(out, n, bad)
            assert refused(5), (n, bad)
        setattr(out, n, good)
    assert mod.check_result(out, names, 5, env) is None
