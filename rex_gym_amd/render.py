"""Camera helpers of the renderers (rex_render / rex_render_visual, csrc/rex_render.hip / rex_render_mesh.hip) and a GIF writer.

The reference renders with PyBullet's getCameraImage (rex_gym/envs/rex_gym_env.py:416-439): a view matrix from
computeViewMatrixFromYawPitchRoll, a projection from computeProjectionMatrixFOV, a 480 x 360 RGB frame.  The two matrix
functions below restate Bullet's conventions (b3ComputeViewMatrixFromYawPitchRoll and b3ComputeProjectionMatrixFOV, up
axis z) and return the same 16 floats, column-major, as PyBullet's functions of the same purpose do.  PyBullet is not
available to this project, so these conventions are restated from Bullet's source and have NOT been checked against it;
nor is the picture meant to agree pixel for pixel with PyBullet's renderer: the HIP renderer draws the collision geometry
the simulator uses (link boxes, full toe cylinders), or, once loaded, the URDF's visual meshes (flat-shaded, untextured).

The view convention: start from eye = (0, -distance, 0) and up = (0, 0, 1), rotate both by Bullet's setEulerZYX(yaw, roll,
pitch) -- Rz(yaw) Rx(pitch) when roll is 0 -- and add the target.  At yaw 0, pitch -30 the eye sits at
target + distance * (0, -0.866, 0.5): a side view in which the robot walks along +x, left to right across the image.
"""
import math

import numpy as np


def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def _rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def camera_eye_up(target, distance, yaw, pitch, roll=0.0, up_axis=2):
    """Eye position and up vector of b3ComputeViewMatrixFromYawPitchRoll (angles in degrees)."""
    y, p, r = math.radians(yaw), math.radians(pitch), math.radians(roll)
    if up_axis == 2:
        R = _rot_z(y) @ _rot_y(r) @ _rot_x(p)        # btQuaternion::setEulerZYX(yaw, roll, pitch)
        eye0, up0 = np.array([0.0, -distance, 0.0]), np.array([0.0, 0.0, 1.0])
    elif up_axis == 1:
        R = _rot_z(r) @ _rot_y(y) @ _rot_x(-p)       # setEulerZYX(roll, yaw, -pitch)
        eye0, up0 = np.array([0.0, 0.0, -distance]), np.array([0.0, 1.0, 0.0])
    else:
        raise ValueError("up_axis must be 1 (y) or 2 (z)")
    return np.asarray(target, dtype=np.float64) + R @ eye0, R @ up0


def look_at(eye, target, up):
    """16 floats, column-major: b3ComputeViewMatrixFromPositions (OpenGL's gluLookAt)."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[0, 3], m[1, 3], m[2, 3] = -s @ eye, -u @ eye, f @ eye
    return [float(v) for v in m.T.ravel()]


def view_matrix_from_yaw_pitch_roll(target, distance, yaw, pitch, roll=0.0, up_axis=2):
    """16 floats, column-major, as pybullet.computeViewMatrixFromYawPitchRoll returns them (angles in degrees)."""
    eye, up = camera_eye_up(target, distance, yaw, pitch, roll, up_axis)
    return look_at(eye, target, up)


def projection_matrix_fov(fov, aspect, near, far):
    """16 floats, column-major, as pybullet.computeProjectionMatrixFOV returns them: OpenGL perspective, VERTICAL fov in
    degrees."""
    yscale = 1.0 / math.tan(math.radians(fov) / 2.0)
    xscale = yscale / aspect
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1] = xscale, yscale
    m[2, 2], m[2, 3] = (far + near) / (near - far), 2.0 * far * near / (near - far)
    m[3, 2] = -1.0
    return [float(v) for v in m.T.ravel()]


def depth_to_opengl_buffer(depth, near, far):
    """Eye-space depth [m] (what rex_render writes) -> the nonlinear [0, 1] depth buffer getCameraImage returns."""
    z = np.asarray(depth, dtype=np.float64)
    return far * (z - near) / (z * (far - near))


def opengl_buffer_to_depth(buf, near, far):
    """The inverse of depth_to_opengl_buffer: z = far * near / (far - (far - near) * buf)."""
    b = np.asarray(buf, dtype=np.float64)
    return far * near / (far - (far - near) * b)


def write_gif(frames, path, fps):
    """Write uint8 [k, H, W, 3] frames (numpy or torch) as an animated GIF at `fps` frames per second.  Needs Pillow."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("write_gif needs Pillow (the PIL package), which is not importable here") from e
    if hasattr(frames, "detach"):
        frames = frames.detach().cpu().numpy()
    frames = [np.ascontiguousarray(np.asarray(f, dtype=np.uint8)) for f in frames]
    if not frames:
        raise ValueError("write_gif: no frames")
    images = [Image.fromarray(f, "RGB") for f in frames]
    duration = max(int(round(1000.0 / float(fps))), 1)    # GIF frame delays are whole centiseconds: Pillow rounds
    images[0].save(path, save_all=True, append_images=images[1:], duration=duration, loop=0, optimize=False)
    return path
