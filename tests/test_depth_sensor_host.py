"""Onboard sensors, the parts that need no GPU: the C ABI's declarations (include/rexsim.h), their ctypes mirror (rex_gym_amd/_lib.py),
the mount's axes (rex_gym_amd/sensors.py) and the argument checks that raise before any launch."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from rex_gym_amd import _lib, build, sensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
ENTRY_POINTS = ("rex_default_depth_sensor", "rex_sense_depth", "rex_height_scan")


def test_header_declares_the_sensor_calls_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert set(ENTRY_POINTS) <= declared
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    body = re.search(r"typedef struct RexDepthSensor \{(.*?)\} RexDepthSensor;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, [n.strip() for n in names.split(",")]) for t, names in re.findall(r"(float|int32_t)\s+([^;]+);", body)]
    assert fields == [("float", ["pos[3]", "fwd[3]", "up[3]"]), ("float", ["fov_deg", "near_plane", "far_plane"]),
                      ("int32_t", ["width", "height"]), ("int32_t", ["see_robot"])]


def test_lib_binds_them_and_the_struct_has_the_size_the_library_asserts():
    assert set(ENTRY_POINTS) <= set(_lib.EXPORTED_SYMBOLS)
    assert [f[0] for f in _lib.RexDepthSensor._fields_] == ["pos", "fwd", "up", "fov_deg", "near_plane", "far_plane", "width", "height",
                                                           "see_robot"]
    src = open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rexsim.hip")).read()
    asserted = re.search(r"static_assert\(sizeof\(RexDepthSensor\) == (\d+)", src)
    assert asserted and ctypes.sizeof(_lib.RexDepthSensor) == int(asserted.group(1)) == 12 * 4 + 3 * 4
    assert "rex_sense.hip" in build.SOURCES


def right_of(fwd, up):
    return np.cross(fwd, up)


def test_mount_axes_zero_and_straight_down():
    fwd, up = sensors.mount_axes()
    np.testing.assert_allclose(fwd, [-1, 0, 0], atol=1e-15)
    np.testing.assert_allclose(up, [0, 0, 1], atol=1e-15)
    np.testing.assert_allclose(right_of(fwd, up), [0, 1, 0], atol=1e-15)
    fwd, up = sensors.mount_axes(-90.0)
    np.testing.assert_allclose(fwd, [0, 0, -1], atol=1e-15)
    np.testing.assert_allclose(up, [-1, 0, 0], atol=1e-15)        # looking down, the image's top is the walking direction


def test_mount_axes_orthonormal_over_a_grid_and_signs():
    for p, y, r in itertools.product((-90, -35, 0, 20, 75), (-180, -60, 0, 45, 130), (-90, 0, 30, 180)):
        fwd, up = sensors.mount_axes(p, y, r)
        assert abs(np.linalg.norm(fwd) - 1) < 1e-12 and abs(np.linalg.norm(up) - 1) < 1e-12 and abs(fwd @ up) < 1e-12, (p, y, r)
        assert abs(fwd[2] - np.sin(np.radians(p))) < 1e-12, (p, y, r)            # neither yaw nor roll changes the elevation
    assert sensors.mount_axes(-30)[0][2] < 0                                      # negative pitch looks down
    fwd, up = sensors.mount_axes(0, 90)
    np.testing.assert_allclose(fwd, [0, 1, 0], atol=1e-15)                        # positive yaw: towards body +y
    np.testing.assert_allclose(up, [0, 0, 1], atol=1e-15)
    fwd, up = sensors.mount_axes(0, 0, 90)                                         # roll: about the optical axis
    np.testing.assert_allclose(fwd, [-1, 0, 0], atol=1e-15)
    np.testing.assert_allclose(np.abs(up), [0, 1, 0], atol=1e-15)


def test_default_sensor_of_the_library_is_the_default_mount():
    if not os.path.exists(build.LIB_PATH) or build.needs_build():
        pytest.skip("the library is not built")
    L = _lib.lib()
    d = _lib.RexDepthSensor()
    assert L.rex_default_depth_sensor(ctypes.byref(d)) == 0
    fwd, up = sensors.mount_axes(-30.0)
    np.testing.assert_allclose(list(d.fwd), fwd, atol=1e-6)
    np.testing.assert_allclose(list(d.up), up, atol=1e-6)
    np.testing.assert_allclose(list(d.pos), [-0.18, 0, 0], atol=1e-7)
    assert (d.width, d.height, d.see_robot) == (32, 24, 1)
    assert (round(d.fov_deg, 5), round(d.near_plane, 5), round(d.far_plane, 5)) == (60.0, 0.02, 10.0)
    assert L.rex_default_depth_sensor(None) < 0
    # the checks that need no sim: a null sim after a good sensor, a null sensor
    buf = (ctypes.c_float * 4)()
    assert L.rex_sense_depth(None, ctypes.byref(d), None, 1, ctypes.addressof(buf), None) < 0 and b"null sim" in L.rex_last_error()
    assert L.rex_sense_depth(None, None, None, 1, ctypes.addressof(buf), None) < 0 and b"null pointer" in L.rex_last_error()
    assert L.rex_height_scan(None, None, 1, 1, None, 1, ctypes.addressof(buf), None) < 0 and b"null pointer" in L.rex_last_error()


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=1025), dict(fov_deg=0.0), dict(fov_deg=180.0), dict(near_plane=0.0),
                                dict(far_plane=0.02), dict(fwd=(-1, 0, 0.01)), dict(up=(0, 0, 1.01)), dict(up=(0.002, 0, 1)),
                                dict(position=(0, float("nan"), 0)), dict(far_plane=float("inf"))])
def test_check_mount_refuses(kw):
    args = dict(width=32, height=24, position=(-0.18, 0, 0), fwd=(-1, 0, 0), up=(0, 0, 1), fov_deg=60.0, near_plane=0.02, far_plane=10.0)
    sensors.check_mount(**args)
    with pytest.raises(ValueError):
        sensors.check_mount(**{**args, **kw})

