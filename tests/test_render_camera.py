"""The renderer's host side, without a GPU: the camera conventions of rex_gym_amd.render (restated from Bullet's
b3ComputeViewMatrixFromYawPitchRoll / b3ComputeProjectionMatrixFOV), the depth-buffer conversion, the generated render
table (rex_gym_amd/csrc/rex_render_gen.h) against literals copied by hand from the reference's URDFs, the C ABI's
RexCamera and the GIF writer."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from rex_gym_amd import render
from rex_gym_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rex_gym_amd", "csrc")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _define(src, name):
    return float(re.search(r"#define\s+%s\s+(\S+)" % name, src).group(1))


def _array(src, name):
    body = re.search(r"%s\[[^=]*=\s*\{(.*?)\};" % name, src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    return [float(v) for v in re.findall(r"-?\d+\.?\d*(?:e-?\d+)?", body)]


def _m(v16):
    return np.array(v16, dtype=np.float64).reshape(4, 4).T     # column-major 16 floats -> 4 x 4


# ---------------------------------------------------------------- camera
def test_view_matrix_side_view_of_the_reference_camera():
    target = (1.0, 2.0, 0.2)
    eye, up = render.camera_eye_up(target, 1.0, 0.0, -30.0)
    np.testing.assert_allclose(eye, np.array(target) + [0.0, -0.8660254037844386, 0.5], atol=1e-12)
    V = _m(render.view_matrix_from_yaw_pitch_roll(target, 1.0, 0.0, -30.0))
    R = V[:3, :3]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)                 # orthonormal
    assert abs(np.linalg.det(R) - 1.0) < 1e-12
    np.testing.assert_allclose(V @ np.array([*target, 1.0]), [0.0, 0.0, -1.0, 1.0], atol=1e-12)   # the target sits 1 m ahead
    np.testing.assert_allclose(V @ np.array([*eye, 1.0]), [0.0, 0.0, 0.0, 1.0], atol=1e-12)
    np.testing.assert_allclose(R[0], [1.0, 0.0, 0.0], atol=1e-12)               # image right = world +x: the robot walks left to right


def test_yaw_90_moves_the_eye_to_the_plus_x_side():
    eye, _ = render.camera_eye_up((0.0, 0.0, 0.0), 2.0, 90.0, -30.0)
    np.testing.assert_allclose(eye, [2.0 * math.cos(math.radians(30)), 0.0, 1.0], atol=1e-12)


def test_projection_is_the_opengl_perspective():
    fov, aspect, near, far = 60.0, 4.0 / 3.0, 0.1, 100.0
    f = 1.0 / math.tan(math.radians(fov) / 2)
    expect = np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0],
                       [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])
    P = render.projection_matrix_fov(fov, aspect, near, far)
    assert len(P) == 16
    np.testing.assert_allclose(_m(P), expect, rtol=1e-12, atol=1e-15)


def test_depth_buffer_round_trip():
    near, far = 0.1, 100.0
    z = np.geomspace(near, far, 257)
    b = render.depth_to_opengl_buffer(z, near, far)
    assert abs(b[0]) < 1e-12 and abs(b[-1] - 1.0) < 1e-12 and np.all(np.diff(b) > 0)
    np.testing.assert_allclose(render.opengl_buffer_to_depth(b, near, far), z, rtol=1e-6)
    # the buffer is what the projection's z row gives after the perspective divide, mapped to [0, 1]
    P = _m(render.projection_matrix_fov(60.0, 1.0, near, far))
    clip = P @ np.stack([np.zeros_like(z), np.zeros_like(z), -z, np.ones_like(z)])
    np.testing.assert_allclose(0.5 * (clip[2] / clip[3]) + 0.5, b, atol=1e-9)


# ---------------------------------------------------------------- the render table
RENDER = _read("rex_render_gen.h")
MODEL = _read("rex_model_gen.h")
YELLOW, BLACK, GREY = [0.92, 0.83, 0.0], [0.1, 0.1, 0.1], [0.6, 0.6, 0.6]     # rex.urdf:3-11


def test_render_table_base_primitives_are_the_physics_geometry():
    nb, na = int(_define(RENDER, "REX_RENDER_NPRIM_BASE")), int(_define(RENDER, "REX_RENDER_NPRIM_ARM"))
    assert (nb, na) == (15 + 4, 15 + 4 + 6)
    kind, body = _array(RENDER, "REX_RENDER_KIND"), _array(RENDER, "REX_RENDER_BODY")
    pos = np.array(_array(RENDER, "REX_RENDER_POS")).reshape(-1, 3)
    rot = np.array(_array(RENDER, "REX_RENDER_ROT")).reshape(-1, 3, 3)
    ext = np.array(_array(RENDER, "REX_RENDER_EXT")).reshape(-1, 3)
    # the 15 boxes, exactly REX_BOX_*
    assert kind[:15] == [0.0] * 15
    assert body[:15] == _array(MODEL, "REX_BOX_BODY")
    np.testing.assert_array_equal(pos[:15], np.array(_array(MODEL, "REX_BOX_CENTER")).reshape(-1, 3))
    np.testing.assert_array_equal(ext[:15], np.array(_array(MODEL, "REX_BOX_HALF")).reshape(-1, 3))
    for r in rot[:15]:
        np.testing.assert_array_equal(r, np.eye(3))
    # the 4 toes, exactly REX_TOE_*: full cylinders about the toe-link y axis
    assert kind[15:19] == [1.0] * 4 and body[15:19] == _array(MODEL, "REX_TOE_BODY")
    np.testing.assert_array_equal(pos[15:19], np.array(_array(MODEL, "REX_TOE_CENTER")).reshape(-1, 3))
    r_toe, hl_toe = _define(MODEL, "REX_TOE_RADIUS"), _define(MODEL, "REX_TOE_HALFLEN")
    for k in range(15, 19):
        np.testing.assert_array_equal(ext[k], [r_toe, r_toe, hl_toe])
        np.testing.assert_allclose(rot[k][:, 2], np.array(_array(MODEL, "REX_TOE_AXIS")).reshape(-1, 3)[k - 15], atol=1e-15)
    for r in rot:
        np.testing.assert_allclose(r @ r.T, np.eye(3), atol=1e-12)
        assert abs(np.linalg.det(r) - 1.0) < 1e-12


def test_render_table_arm_cylinders_and_colours():
    kind, body = _array(RENDER, "REX_RENDER_KIND"), _array(RENDER, "REX_RENDER_BODY")
    pos = np.array(_array(RENDER, "REX_RENDER_POS")).reshape(-1, 3)
    rot = np.array(_array(RENDER, "REX_RENDER_ROT")).reshape(-1, 3, 3)
    ext = np.array(_array(RENDER, "REX_RENDER_EXT")).reshape(-1, 3)
    rgb = np.array(_array(RENDER, "REX_RENDER_RGB")).reshape(-1, 3)
    # rex_arm.urdf:612-790: arm_long_U cylinder r 0.02 l 0.02 at z 0.01; sections 1, 2: r 0.02 l 0.05 at x 0.025, rpy (0, pi/2, 0);
    # section 3: l 0.05 at y -0.025, rpy (pi/2, 0, 0); section 4: l 0.06 at y -0.035, rpy (pi/2, 0, 0); section 5 (gripper):
    # l 0.06 at y -0.04, rpy (-pi/2, 0, 0)
    arm = [((0, 0, 0.01), 0.02, (0, 0, 1)), ((0.025, 0, 0), 0.05, (1, 0, 0)), ((0.025, 0, 0), 0.05, (1, 0, 0)),
           ((0, -0.025, 0), 0.05, (0, -1, 0)), ((0, -0.035, 0), 0.06, (0, -1, 0)), ((0, -0.04, 0), 0.06, (0, 1, 0))]
    for k, (p, length, axis) in enumerate(arm):
        i = 19 + k
        assert kind[i] == 1.0 and body[i] == 13 + k
        np.testing.assert_allclose(pos[i], p, atol=1e-12)
        np.testing.assert_allclose(ext[i], [0.02, 0.02, length / 2], atol=1e-12)
        np.testing.assert_allclose(rot[i][:, 2], axis, atol=1e-12)
        np.testing.assert_array_equal(rgb[i], BLACK)            # every arm link's visual is black
    # colours: base_link black, chassis rear / front yellow (merged into the base but keeping their own), leg links black,
    # toes grey (rex.urdf:20,69,92,117,149,168,187)
    np.testing.assert_array_equal(rgb[0], BLACK)
    np.testing.assert_array_equal(rgb[1], YELLOW)
    np.testing.assert_array_equal(rgb[2], YELLOW)
    for k in range(3, 15):
        np.testing.assert_array_equal(rgb[k], BLACK)
    for k in range(15, 19):
        np.testing.assert_array_equal(rgb[k], GREY)


def test_render_table_includes_only_the_model_headers():
    assert re.findall(r'#include\s+"([^"]+)"', RENDER) == ["rex_model_gen.h"]


# ---------------------------------------------------------------- ABI and GIF
def test_rex_camera_mirror_is_six_floats():
    assert ctypes.sizeof(_lib.RexCamera) == 6 * 4
    assert [f[0] for f in _lib.RexCamera._fields_] == ["distance", "yaw_deg", "pitch_deg", "fov_deg", "near_plane", "far_plane"]
    header = open(os.path.join(os.path.dirname(CSRC), "..", "include", "rexsim.h")).read()
    assert "typedef struct RexCamera { float distance, yaw_deg, pitch_deg, fov_deg, near_plane, far_plane; } RexCamera;" in header
    assert "rex_render" in _lib.EXPORTED_SYMBOLS and "rex_default_camera" in _lib.EXPORTED_SYMBOLS


def test_write_gif_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(0)
    frames = rng.randint(0, 256, size=(7, 12, 16, 3)).astype(np.uint8)
    path = render.write_gif(frames, str(tmp_path / "clip.gif"), fps=20)
    im = Image.open(path)
    assert im.n_frames == 7 and im.size == (16, 12)
