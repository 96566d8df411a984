"""Onboard sensors on the GPU (rex_sense_depth, rex_height_scan) against the numpy caster of tests/test_gpu_render.py: the same
forward kinematics, ray tests, ground and heightfield functions, with the eye and the axes of a mount on the base.

Which pixels are held to the bound: those whose ambiguity flags are clear (a face edge, a tie between two primitives, a grazing
or tied heightfield facet) and where the reference gives the same label at four rays 1e-3 pixel off the centre ray, each within
1 % of the centre's depth -- rays within float32 reach of a silhouette or a depth step, and nothing else.  Bound: compare()'s own,
|gpu - ref| <= 1e-4 ref + 1e-5.  At least 0.9 of every image is compared."""
import ctypes
import math

import numpy as np
import pytest

import test_gpu_render as col
from rex_gym_amd import sensors

pytestmark = pytest.mark.gpu

MOUNTS = {"front": dict(position=(-0.18, 0.0, 0.0), pitch_deg=-30.0),                 # the default: in front of the front face
          "back_top": dict(position=(0.25, 0.0, 0.12), pitch_deg=-35.0)}              # behind and above the rear chassis, looking over the robot
SIZES = [(32, 24), (16, 12), (13, 7), (1, 1), (64, 48)]
FOV, NEAR, FAR = 60.0, 0.02, 10.0
JITTER = [(1e-3, 1e-3), (1e-3, -1e-3), (-1e-3, 1e-3), (-1e-3, -1e-3)]


def sensor_cast(state, env, arm, W, H, mount, field=None, see_robot=True, jitter=(0.0, 0.0)):
    """cast() of test_gpu_render with the camera on the base: eye = o0 + R0 pos, axes R0 fwd, R0 up and their cross product, and an
    optional sub-pixel offset.  -> depth [H, W], label [H, W] (primitive index; -1 plane, -2 field facet, -3 nothing), ambiguous
    [H, W], kind [H, W] (ground_shade's: 0 nothing, 1 plane, 2 field, 3 robot)"""
    fwd, up = sensors.mount_axes(mount["pitch_deg"])
    Rs, os_ = col.fk(state, env, arm)
    eye = os_[0] + Rs[0] @ np.asarray(mount["position"], float)
    f, u = Rs[0] @ fwd, Rs[0] @ up
    r = np.cross(f, u)
    ty = math.tan(math.radians(FOV) / 2)
    tx = ty * W / H
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    sx = (2 * (px + 0.5 + jitter[0]) / W - 1) * tx
    sy = (1 - 2 * (py + 0.5 + jitter[1]) / H) * ty
    d = (f[None, None] + sx[..., None] * r + sy[..., None] * u).reshape(-1, 3)
    N = len(d)
    best, second = np.full(N, np.inf), np.full(N, np.inf)
    label = np.full(N, -1)
    normal = np.zeros((N, 3))
    amb = np.zeros(N, dtype=bool)
    for k in range((25 if arm else 19) if see_robot else 0):
        b = col.P_BODY[k]
        c = os_[b] + Rs[b] @ col.P_POS[k]
        ax = Rs[b] @ col.P_ROT[k]
        t, nl, am = (col._hit_box if col.P_KIND[k] == 0 else col._hit_cyl)(ax.T @ (eye - c), d @ ax, col.P_EXT[k], NEAR)
        closer = t < best
        second = np.where(closer, best, np.minimum(second, t))
        best = np.where(closer, t, best)
        label = np.where(closer, k, label)
        normal = np.where(closer[:, None], nl @ ax.T, normal)
        amb = np.where(closer, am, amb)
    _, best, ground, hit, g = col.ground_shade(eye, d, best, normal, col.P_RGB[np.maximum(label, 0)], field, NEAR, FAR)
    kind = g["kind"]
    with np.errstate(invalid="ignore"):
        tie = (kind == 3) & (second - best < 1e-5 + 1e-6 * np.where(np.isfinite(best), best, 0.0))
    amb = hit & ((amb & (kind == 3)) | tie | g["amb"])
    label = np.where(kind == 3, label, -np.where(kind == 0, 3, kind))
    depth = np.where(hit, best, FAR)
    return depth.reshape(H, W), label.reshape(H, W), amb.reshape(H, W), kind.reshape(H, W)


def reference(state, env, arm, W, H, mount, field=None, see_robot=True):
    """-> depth, comparable, kind, label of one image"""
    dep, lab, amb, kind = sensor_cast(state, env, arm, W, H, mount, field, see_robot)
    ok = ~amb
    for j in JITTER:
        dj, lj, _, _ = sensor_cast(state, env, arm, W, H, mount, field, see_robot, j)
        ok &= (lj == lab) & (np.abs(dj - dep) <= 0.01 * dep)
    return dep, ok, kind, lab


def check_image(gpu, ref, what):
    dep, ok, _, _ = ref
    assert gpu.shape == dep.shape and gpu.dtype == np.float32, what
    err = np.abs(gpu.astype(np.float64) - dep)
    print(what, "compared %.3f" % ok.mean(), "max excess %.3g" % float((err - 1e-4 * dep - 1e-5)[ok].max() if ok.any() else 0.0))
    assert ok.mean() >= 0.9, (what, float(ok.mean()))
    assert np.all(err[ok] <= 1e-4 * dep[ok] + 1e-5), (what, float((err - 1e-4 * dep)[ok].max()), int((err > 1e-4 * dep + 1e-5)[ok].sum()))


def read(env, mount, W, H, **kw):
    import torch
    sensor = env.depth_sensor(width=W, height=H, fov_deg=FOV, near_plane=NEAR, far_plane=FAR, **MOUNTS[mount],
                              **{k: v for k, v in kw.items() if k == "see_robot"})
    out = sensor.read(**{k: v for k, v in kw.items() if k != "see_robot"})
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------- a. on the plane
@pytest.fixture(scope="module")
def plane_env():
    envs = {}

    def get(mark):
        if mark not in envs:
            env = col.plane_batch(mark)
            envs[mark] = (env, env.state.cpu().numpy())
        return envs[mark]
    yield get
    for env, _ in envs.values():
        env.close()


@pytest.mark.parametrize("mark", ["base", "arm"])
@pytest.mark.parametrize("mount", ["front", "back_top"])
@pytest.mark.parametrize("W,H", SIZES)
def test_plane(plane_env, mark, mount, W, H):
    """32 x 24: one env per workgroup and a remainder of idle threads; 16 x 12: 5 envs per workgroup, 4 envs read; 13 x 7: 91 pixels,
    a thread's 4 pixels straddle two envs on the element-store path; 1 x 1; 64 x 48: three tiles per env."""
    env, state = plane_env(mark)
    gpu = read(env, mount, W, H)
    assert gpu.shape == (4, H, W)
    for e in range(4):
        ref = reference(state, e, mark == "arm", W, H, MOUNTS[mount])
        check_image(gpu[e], ref, (mark, mount, W, H, e))
        if mount == "back_top" and (W, H) == (32, 24):
            # else this mount tests the ground and nothing more
            _, _, kind, lab = ref
            assert (kind == 3).mean() >= 0.3 and len(set(lab[kind == 3])) >= 6, (e, float((kind == 3).mean()), set(lab[kind == 3]))


# ---------------------------------------------------------------- b. the ground alone
def test_see_robot_false(plane_env):
    env, state = plane_env("base")
    W, H = 32, 24
    gpu, with_robot = read(env, "back_top", W, H, see_robot=False), read(env, "back_top", W, H)
    for e in range(4):
        check_image(gpu[e], reference(state, e, False, W, H, MOUNTS["back_top"], see_robot=False), ("ground only", e))
        assert (gpu[e] != with_robot[e]).mean() >= 0.3, (e, float((gpu[e] != with_robot[e]).mean()))


# ---------------------------------------------------------------- c. on a heightfield pool
@pytest.fixture(scope="module")
def field_scene():
    env, state, field_of = col.custom_field_scene()
    yield env, state, field_of, {}
    env.close()


@pytest.mark.parametrize("mount", ["front", "back_top"])
@pytest.mark.parametrize("W,H,ids", [(16, 12, [0, 1, 2, 3]), (32, 24, [0, 3])])
def test_heightfield(field_scene, mount, W, H, ids):
    env, state, field_of, seen = field_scene
    gpu = read(env, mount, W, H, env_ids=ids)
    for k, e in enumerate(ids):
        ref = reference(state, e, False, W, H, MOUNTS[mount], field_of(e))
        check_image(gpu[k], ref, ("field", mount, W, H, e))
        seen.setdefault(mount, []).append(float((ref[2] == 2).mean()))


def test_heightfield_cases_cover(field_scene):
    """From the reference alone: for each mount at least one image is 30 % heightfield facets (custom_field_scene asserts that both
    fields of the pool are in use)."""
    _, state, field_of, seen = field_scene
    for mount in MOUNTS:
        shares = seen.get(mount) or [float((sensor_cast(state, e, False, 16, 12, MOUNTS[mount], field_of(e))[3] == 2).mean()) for e in range(4)]
        assert max(shares) >= 0.3, (mount, shares)


# ---------------------------------------------------------------- d. plumbing
def test_env_ids_out_and_read_only(plane_env):
    import torch
    env, _ = plane_env("base")
    sensor = env.depth_sensor()
    before = env.state.clone()
    full = sensor.read()
    part = sensor.read(env_ids=[3, 0, 3])
    t = torch.full((4, 24, 32), -1.0, dtype=torch.float32, device=env.device)
    back = sensor.read(out=t)
    again = sensor.read(out=t)
    torch.cuda.synchronize()
    assert full.shape == (4, 24, 32) and full.dtype == torch.float32 and full.device == env.device
    bits = lambda x: x.view(torch.int32)
    assert torch.equal(bits(part[0]), bits(full[3])) and torch.equal(bits(part[1]), bits(full[0])) and torch.equal(bits(part[2]), bits(full[3]))
    assert not torch.equal(bits(full[0]), bits(full[3]))
    assert back is t and again is t and torch.equal(bits(t), bits(full))
    assert torch.equal(bits(env.state), bits(before))
    with pytest.raises(ValueError):
        sensor.read(out=torch.empty((3, 24, 32), dtype=torch.float32, device=env.device))
    with pytest.raises(ValueError):
        sensor.read(out=torch.empty((4, 24, 32), dtype=torch.float64, device=env.device))


@pytest.mark.parametrize("mount", ["front", "back_top"])
@pytest.mark.parametrize("W,H", [(13, 7), (16, 12)])
def test_guard_and_unaligned_output(plane_env, mount, W, H):
    """An output one float into a larger buffer: the sentinels in front of and behind it survive, and the element stores give the bits
    of the aligned read (16 x 12: whole 16-byte stores there)."""
    import torch
    env, _ = plane_env("base")
    sensor = env.depth_sensor(width=W, height=H, **MOUNTS[mount])
    n = 4 * H * W
    aligned = sensor.read()
    buf = torch.full((n + 64,), -7.0, dtype=torch.float32, device=env.device)
    assert buf.data_ptr() % 16 == 0
    rc = env._L.rex_sense_depth(env._h, ctypes.byref(sensor.struct), None, 4, buf.data_ptr() + 4, env._stream_ptr())
    assert rc == 0, env._L.rex_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:1] == -7.0).all()) and bool((buf[1 + n:] == -7.0).all())
    assert torch.equal(buf[1:1 + n].view(torch.int32), aligned.reshape(-1).view(torch.int32))
    assert bool((aligned > 0).all()) and bool((aligned <= FAR).all())


def test_bad_arguments_raise_before_any_launch(plane_env):
    import torch
    env, _ = plane_env("base")
    for kw in (dict(fwd=(-1, 0, 0), up=(0, 0.1, 1)), dict(fwd=(-1, 0, 0)), dict(fwd=(-1, 0, 0), up=(-0.1, 0, 0.995)),
               dict(near_plane=0.0), dict(far_plane=0.01), dict(fov_deg=0.0), dict(fov_deg=180.0), dict(width=0), dict(height=1025),
               dict(position=(0, 0, float("nan")))):
        with pytest.raises(ValueError):
            env.depth_sensor(**kw)
    sensor = env.depth_sensor()
    for ids in ([4], [-1], []):
        with pytest.raises(IndexError):
            sensor.read(env_ids=ids)
        with pytest.raises(IndexError):
            env.height_scan(np.zeros((1, 2), np.float32), env_ids=ids)
    for pts in (np.zeros((0, 2), np.float32), np.zeros((4097, 2), np.float32), np.zeros((3, 3), np.float32), np.full((2, 2), np.nan, np.float32)):
        with pytest.raises(ValueError):
            env.height_scan(pts)
    # the library's own checks, past the Python ones
    L, out = env._L, torch.zeros(64, dtype=torch.float32, device=env.device)
    d = sensor.struct
    bad = []
    for field, value in (("width", 0), ("height", 1025), ("fov_deg", 180.0), ("near_plane", 0.0), ("far_plane", 0.01), ("see_robot", 2),
                         ("fov_deg", float("nan"))):
        c = type(d).from_buffer_copy(d)
        setattr(c, field, value)
        bad.append(c)
    c = type(d).from_buffer_copy(d)
    c.up[1] = 0.1
    bad.append(c)
    for c in bad:
        assert L.rex_sense_depth(env._h, ctypes.byref(c), None, 1, out.data_ptr(), env._stream_ptr()) == -1
    assert L.rex_sense_depth(env._h, ctypes.byref(d), None, 0, out.data_ptr(), env._stream_ptr()) == -1
    assert L.rex_sense_depth(env._h, ctypes.byref(d), None, 5, out.data_ptr(), env._stream_ptr()) == -1       # no ids: n <= num_envs
    assert L.rex_sense_depth(env._h, ctypes.byref(d), None, 1, None, env._stream_ptr()) == -1
    for K, rel, n, pts, o in ((0, 0, 1, out, out), (4097, 0, 1, out, out), (1, 2, 1, out, out), (1, 0, 0, out, out), (1, 0, 1, None, out),
                              (1, 0, 1, out, None)):
        rc = L.rex_height_scan(env._h, pts.data_ptr() if pts is not None else None, K, rel, None, n, o.data_ptr() if o is not None else None,
                               env._stream_ptr())
        assert rc == -1, (K, rel, n)
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ---------------------------------------------------------------- e. the height scan
GRID = np.stack(np.meshgrid(np.linspace(-0.5, 0.5, 5), np.linspace(-0.5, 0.5, 5), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)


def world_points(state, e, rotate=True):
    """the scan's points of env e in the world, float64 from the float32 state"""
    s = state[:, e].astype(np.float64)
    x, y, z, w = s[3:7]
    yaw = math.atan2(2 * (x * y + z * w), 1 - 2 * (y * y + z * z)) if rotate else 0.0
    c, sn = math.cos(yaw), math.sin(yaw)
    g = GRID.astype(np.float64)
    return np.stack([s[0] + c * g[:, 0] - sn * g[:, 1], s[1] + sn * g[:, 0] + c * g[:, 1]], 1)


def test_height_scan_on_the_plane(plane_env):
    import torch
    env, state = plane_env("base")
    uploads = len(getattr(env, "_scan_points", {}))
    absolute, relative = env.height_scan(GRID, relative=False), env.height_scan(GRID)
    part = env.height_scan(torch.as_tensor(GRID, device=env.device), env_ids=[3, 0, 3], out=torch.empty((3, 25), dtype=torch.float32, device=env.device))
    torch.cuda.synchronize()
    assert absolute.shape == (4, 25) and absolute.dtype == torch.float32
    assert bool((absolute == 0).all())
    assert np.array_equal(relative.cpu().numpy(), np.repeat(state[2][:, None], 25, 1))
    assert torch.equal(part, relative[[3, 0, 3]])
    assert len(env._scan_points) == uploads + 1            # one upload for the two calls with the same array


def test_height_scan_on_the_heightfield(field_scene):
    import torch
    env, state, field_of, _ = field_scene
    absolute, relative = env.height_scan(GRID, relative=False), env.height_scan(GRID, relative=True)
    torch.cuda.synchronize()
    absolute, relative = absolute.cpu().numpy(), relative.cpu().numpy()
    left_out, off_grid, facets = 0, 0, 0
    for e in range(4):
        field = field_of(e)
        _, _, nx, ny, inv_x, inv_y, off_x, off_y = field
        pts = world_points(state, e)
        for k, (x, y) in enumerate(pts):
            gx, gy = x * inv_x + off_x, y * inv_y + off_y
            edge = min(abs(gx) / inv_x, abs(gx - (nx - 1)) / inv_x, abs(gy) / inv_y, abs(gy - (ny - 1)) / inv_y)     # metres to the footprint's edge
            if edge < 1e-4:
                left_out += 1
                continue
            want = col.field_height(field, x, y)
            bound = 1e-5 + max(abs(col.field_height(field, x + dx, y + dy) - want) for dx in (-1e-5, 0, 1e-5) for dy in (-1e-5, 0, 1e-5))
            assert abs(absolute[e, k] - want) <= bound, (e, k, float(absolute[e, k]), want, bound)
            assert abs(relative[e, k] - (float(state[2, e]) - want)) <= bound + 1e-6, (e, k)
            inside = 0 <= gx <= nx - 1 and 0 <= gy <= ny - 1
            off_grid += not inside
            facets += inside and want > 0
            if not inside:
                assert absolute[e, k] == 0.0
    assert left_out <= 0.05 * 100 and off_grid >= 10 and facets >= 10, (left_out, off_grid, facets)
    # env 3 is turned by 1 rad: an unrotated grid is another set of points, and the ground under them differs
    field = field_of(3)
    turned = [col.field_height(field, x, y) for x, y in world_points(state, 3)]
    straight = [col.field_height(field, x, y) for x, y in world_points(state, 3, rotate=False)]
    worst = 1e-5 + max(abs(col.field_height(field, x + dx, y + dy) - h) for (x, y), h in zip(world_points(state, 3), turned)
                       for dx in (-1e-5, 1e-5) for dy in (-1e-5, 1e-5))
    assert max(abs(a - b) for a, b in zip(turned, straight)) > 10 * worst
