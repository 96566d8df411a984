"""Onboard sensors of a batch (include/rexsim.h: rex_sense_depth, rex_height_scan): a depth camera mounted on the base body and
the terrain's height at points around the base, for every env in one launch each, on the env's device and stream.

    cam = env.depth_sensor(width=32, height=24)          # just in front of the front face, pitched 30 degrees down
    depth = cam.read()                                   # float32 [num_envs, 24, 32], metres along the optical axis
    heights = env.height_scan(points)                    # points [K, 2] in the base's yaw frame -> float32 [num_envs, K], base z minus the ground's

The robot walks towards body -x, so a mount at zero angles looks along -x with z up and body +y to the image's right."""
import ctypes
import math

import numpy as np

from . import _lib

MAX_SIDE = 1024          # rex_sense_depth: width and height
MAX_POINTS = 4096        # rex_height_scan: K


def mount_axes(pitch_deg=0.0, yaw_deg=0.0, roll_deg=0.0):
    """(fwd, up): the optical axis and the image's up direction of a mount, unit vectors in the base frame (float64 [3] each).
    Zero angles: fwd (-1, 0, 0), up (0, 0, 1), hence right = fwd x up = (0, 1, 0).  Negative pitch looks down (as
    RexCamera.pitch_deg); then yaw turns about the base's z, positive towards body +y; then roll turns about the optical axis."""
    p, y, r = math.radians(pitch_deg), math.radians(yaw_deg), math.radians(roll_deg)
    fwd = np.array([-math.cos(p), 0.0, math.sin(p)])
    up = np.array([math.sin(p), 0.0, math.cos(p)])
    c, s = math.cos(y), math.sin(y)
    Rz = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])      # Rz(-yaw): -x turns towards +y
    fwd, up = Rz @ fwd, Rz @ up
    up = up * math.cos(r) + np.cross(fwd, up) * math.sin(r)
    return fwd, up


def check_mount(width, height, position, fwd, up, fov_deg, near_plane, far_plane):
    """The argument checks of rex_sense_depth, raised before any launch."""
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError(f"depth_sensor: width and height must lie in 1..{MAX_SIDE}, got {width} x {height}")
    vals = np.concatenate([np.asarray(position, float).reshape(-1), np.asarray(fwd, float).reshape(-1), np.asarray(up, float).reshape(-1),
                           [fov_deg, near_plane, far_plane]])
    if vals.size != 12 or not np.all(np.isfinite(vals)):
        raise ValueError("depth_sensor: position, fwd and up are 3-vectors, and every field must be finite")
    if not (0 < fov_deg < 180 and near_plane > 0 and far_plane > near_plane):
        raise ValueError("depth_sensor: fov must lie in (0, 180), the near plane be positive and far > near")
    f, u = vals[3:6], vals[6:9]
    if abs(np.linalg.norm(f) - 1) > 1e-3 or abs(np.linalg.norm(u) - 1) > 1e-3 or abs(f @ u) > 1e-3:
        raise ValueError("depth_sensor: fwd and up must be unit vectors orthogonal to each other")


class DepthSensor:
    """A depth camera rigidly mounted on the base of every env of `env` (RexBatchEnv.depth_sensor builds it)."""

    def __init__(self, env, width, height, position, fwd, up, fov_deg, near_plane, far_plane, see_robot):
        width, height = int(width), int(height)
        check_mount(width, height, position, fwd, up, fov_deg, near_plane, far_plane)
        self.env, self.width, self.height = env, width, height
        self.struct = _lib.RexDepthSensor((ctypes.c_float * 3)(*map(float, position)), (ctypes.c_float * 3)(*map(float, fwd)),
                                          (ctypes.c_float * 3)(*map(float, up)), float(fov_deg), float(near_plane), float(far_plane),
                                          width, height, 1 if see_robot else 0)
        self._out = None         # the caller's tensor validated last

    def read(self, env_ids=None, out=None):
        """Depth images float32 [k, height, width] (row 0 = the top): metres along the optical axis to the first hit between
        the near and the far plane, far_plane where there is none.  env_ids as in render() (default: every env, in order);
        out: a float32 tensor of that shape on the env's device to fill and return -- checked once, then reused, so that a
        sensor read every step allocates nothing."""
        env = self.env
        torch = env._torch
        with env._on_stream():
            ids, k = env._row_ids(env_ids, "depth_sensor.read")
            if k * self.width * self.height >= 2 ** 29:
                raise ValueError("depth_sensor.read: k * width * height must stay below 2^29")
            shape = (k, self.height, self.width)
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=env.device)
            elif out is not self._out or tuple(out.shape) != shape:
                check_out(out, shape, env, "depth_sensor.read")
                self._out = out
            _lib.check(env._L.rex_sense_depth(env._h, ctypes.byref(self.struct), ids.data_ptr() if ids is not None else None, k,
                                              out.data_ptr(), env._stream_ptr()), "rex_sense_depth")
        return out


def check_out(out, shape, env, who):
    torch = env._torch
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == env.device and tuple(out.shape) == shape
            and out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor of shape {shape} on {env.device}")
