"""The HIP renderer (rex_render, csrc/rex_render.hip) on the GPU, against a numpy ray caster of this file.

The reference here is independent of the kernel: forward kinematics from env.state with the tables parsed from
rex_model_gen.h / rex_arm_model_gen.h, the primitives parsed from rex_render_gen.h, the camera restated from Bullet's
convention (rex_gym_amd.render.camera_eye_up + a look-at basis), and slab / capped-cylinder / plane / heightfield
intersections in float64.  The shading constants are the ones csrc/rex_render.h documents."""
import math
import os
import re

import numpy as np
import pytest

from rex_gym_amd import render as rnd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rex_gym_amd", "csrc")
SRC = {n: open(os.path.join(CSRC, n)).read() for n in ("rex_model_gen.h", "rex_arm_model_gen.h", "rex_render_gen.h")}

LIGHT = np.array([0.36, -0.48, 0.8])
AMBIENT, DIFFUSE = 0.35, 0.65
SKY = np.array([0.70, 0.80, 0.92])
CHECK_A, CHECK_B = np.array([0.25, 0.40, 0.65]), np.array([0.85, 0.88, 0.92])
NEAR, FAR = 0.1, 100.0


def _arr(hdr, name):
    body = re.search(r"%s\[[^=]*=\s*\{(.*?)\};" % name, SRC[hdr], re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    return np.array([float(v) for v in re.findall(r"-?\d+\.?\d*(?:e-?\d+)?", body)])


PARENT = _arr("rex_model_gen.h", "REX_PARENT").astype(int)
JAXIS = _arr("rex_model_gen.h", "REX_JOINT_AXIS").astype(int)
JPOS = _arr("rex_model_gen.h", "REX_JOINT_POS").reshape(-1, 3)
A_PARENT = _arr("rex_arm_model_gen.h", "REXA_PARENT").astype(int)
A_POS = _arr("rex_arm_model_gen.h", "REXA_POS").reshape(-1, 3)
A_E0 = _arr("rex_arm_model_gen.h", "REXA_E0").reshape(-1, 3, 3)
A_SIGN = _arr("rex_arm_model_gen.h", "REXA_AXIS_SIGN")
P_KIND = _arr("rex_render_gen.h", "REX_RENDER_KIND").astype(int)
P_BODY = _arr("rex_render_gen.h", "REX_RENDER_BODY").astype(int)
P_POS = _arr("rex_render_gen.h", "REX_RENDER_POS").reshape(-1, 3)
P_ROT = _arr("rex_render_gen.h", "REX_RENDER_ROT").reshape(-1, 3, 3)
P_EXT = _arr("rex_render_gen.h", "REX_RENDER_EXT").reshape(-1, 3)
P_RGB = _arr("rex_render_gen.h", "REX_RENDER_RGB").reshape(-1, 3)


def _axis_rot(k, a):
    c, s = math.cos(a), math.sin(a)
    R = np.eye(3)
    i1, i2 = (k + 1) % 3, (k + 2) % 3
    R[i1, i1], R[i1, i2], R[i2, i1], R[i2, i2] = c, -s, s, c
    return R


def fk(state, env, arm):
    """World rotation and origin of every body of env `env` (state: numpy [words, n] float32)."""
    s = state[:, env].astype(np.float64)
    x, y, z, w = s[3:7]
    R0 = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Rs, os_ = [R0], [s[0:3]]
    for b in range(1, 13):
        p = PARENT[b]
        Rs.append(Rs[p] @ _axis_rot(JAXIS[b - 1], s[13 + b - 1]))
        os_.append(os_[p] + Rs[p] @ JPOS[b - 1])
    if arm:
        for k in range(6):
            p = A_PARENT[k]
            Rs.append(Rs[p] @ A_E0[k] @ _axis_rot(2, A_SIGN[k] * s[13 + 12 + k]))
            os_.append(os_[p] + Rs[p] @ A_POS[k])
    return Rs, os_


def rays(target, W, H, distance=1.0, yaw=0.0, pitch=-30.0, fov=60.0):
    eye, up = rnd.camera_eye_up(target, distance, yaw, pitch)
    f = np.asarray(target) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    ty = math.tan(math.radians(fov) / 2)
    tx = ty * W / H
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    sx = (2 * (px + 0.5) / W - 1) * tx
    sy = (1 - 2 * (py + 0.5) / H) * ty
    d = f[None, None] + sx[..., None] * r + sy[..., None] * u      # t along d = eye-space depth
    return eye, d.reshape(-1, 3)


def _hit_box(o, d, h):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        ta, tb = (-h - o) * inv, (h - o) * inv
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    t0, t1 = lo.max(1), hi.min(1)
    a0, a1 = lo.argmax(1), hi.argmin(1)
    ok = t0 <= t1
    use0 = ok & (t0 >= NEAR)
    use1 = ok & ~use0 & (t1 >= NEAR)
    t = np.where(use0, t0, np.where(use1, t1, np.inf))
    a = np.where(use0, a0, a1)
    dd = np.take_along_axis(d, a[:, None], 1)[:, 0]
    sgn = np.where(use0, np.where(dd > 0, -1.0, 1.0), np.where(dd > 0, 1.0, -1.0))
    n = np.zeros_like(d)
    n[np.arange(len(d)), a] = sgn
    # a hit within float32 reach (1e-5 m + 1e-6 t) of a box edge: the face (and so the shade) is a coin toss
    srt = np.sort(np.where(use0[:, None], lo, -hi), 1)
    amb = np.abs(srt[:, 2] - srt[:, 1]) < 1e-5 + 1e-6 * np.where(np.isfinite(t), t, 0.0)
    return t, n, amb


def _hit_cyl(o, d, h):
    r, hz = h[0], h[2]
    best = np.full(len(d), np.inf)
    which = np.full(len(d), -1)
    a = d[:, 0] ** 2 + d[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = -(o[0] * d[:, 0] + o[1] * d[:, 1]) / a
        px, py = o[0] + tc * d[:, 0], o[1] + tc * d[:, 1]
        q = r * r - (px * px + py * py)
        dt = np.sqrt(q / a)
        amb = np.zeros(len(d), dtype=bool)
        for ts in (tc - dt, tc + dt):
            z = o[2] + ts * d[:, 2]
            ok = (a > 0) & (q >= 0) & (ts >= NEAR) & (ts < best) & (np.abs(z) <= hz)
            best, which = np.where(ok, ts, best), np.where(ok, 0, which)
        for s, zc in ((1, -hz), (2, hz)):
            ts = (zc - o[2]) / d[:, 2]
            x, y = o[0] + ts * d[:, 0], o[1] + ts * d[:, 1]
            ok = (d[:, 2] != 0) & (ts >= NEAR) & (ts < best) & (x * x + y * y <= r * r)
            best, which = np.where(ok, ts, best), np.where(ok, s, which)
        x, y = o[0] + best * d[:, 0], o[1] + best * d[:, 1]
        z = o[2] + best * d[:, 2]
        rr = np.sqrt(x * x + y * y)
        n = np.where((which == 0)[:, None], np.stack([x / rr, y / rr, np.zeros_like(x)], 1),
                     np.stack([np.zeros_like(x), np.zeros_like(x), np.where(which == 1, -1.0, 1.0)], 1))
        amb = np.isfinite(best) & ((np.abs(np.abs(z) - hz) < 1e-5) | (np.abs(rr - r) < 1e-5) & (which > 0))
    return best, n, amb


def cast(state, env, arm, W, H, field=None, camera=None):
    """numpy image of one env: (rgb uint8 [H, W, 3], depth [H, W], seg [H, W], label [H, W] (primitive index, -2 ground,
    -1 nothing), ambiguous [H, W] (a face edge within 1e-5 m or a checker line within float32 reach of the hit))."""
    camera = camera or {}
    Rs, os_ = fk(state, env, arm)
    eye, d = rays(os_[0], W, H, camera.get("distance", 1.0), camera.get("yaw_deg", 0.0), camera.get("pitch_deg", -30.0))
    N = len(d)
    best = np.full(N, np.inf)
    label = np.full(N, -1)
    normal = np.zeros((N, 3))
    amb = np.zeros(N, dtype=bool)
    second = np.full(N, np.inf)      # the runner-up's distance: coplanar faces of two primitives (the toe caps lie in the foot
                                     # box's sides, y = +-0.01) z-fight, and which one wins is a float32 coin toss
    for k in range(25 if arm else 19):
        b = P_BODY[k]
        c = os_[b] + Rs[b] @ P_POS[k]
        ax = Rs[b] @ P_ROT[k]                 # columns: the local axes in world
        o, dl = ax.T @ (eye - c), d @ ax
        t, nl, am = (_hit_box if P_KIND[k] == 0 else _hit_cyl)(o, dl, P_EXT[k])
        closer = t < best
        second = np.where(closer, best, np.minimum(second, t))
        best = np.where(closer, t, best)
        label = np.where(closer, k, label)
        normal = np.where(closer[:, None], nl @ ax.T, normal)
        amb = np.where(closer, am, amb)
    with np.errstate(divide="ignore", invalid="ignore"):
        tplane = np.where(d[:, 2] < 0, -eye[2] / d[:, 2], np.inf)
    tg = np.where(tplane >= NEAR, tplane, np.inf)
    gn = np.tile([0.0, 0.0, 1.0], (N, 1))
    if field is not None:
        tf, fn = field_cast(field, eye, d, np.minimum(np.minimum(tplane, FAR), best))
        closer = tf < tg
        tg = np.where(closer, tf, tg)
        gn = np.where(closer[:, None], fn, gn)
    ground = tg < best
    best = np.where(ground, tg, best)
    label = np.where(ground, -2, label)
    normal = np.where(ground[:, None], gn, normal)
    hit = best <= FAR
    hx, hy = eye[0] + best * d[:, 0], eye[1] + best * d[:, 1]
    with np.errstate(invalid="ignore"):
        even = (np.floor(hx) + np.floor(hy)) % 2 == 0
        tol = 1e-5 + 2e-6 * best          # float32 hit points drift with the distance (eye + t d, t up to 100 m)
        near_line = (np.abs(hx - np.round(hx)) < tol) | (np.abs(hy - np.round(hy)) < tol)
    alb = np.where(label[:, None] >= 0, P_RGB[np.maximum(label, 0)], np.where(even[:, None], CHECK_A, CHECK_B))
    flip = (normal * d).sum(1) > 0
    normal = np.where(flip[:, None], -normal, normal)
    lam = AMBIENT + DIFFUSE * np.maximum(0.0, normal @ LIGHT)
    col = np.where(hit[:, None], alb * lam[:, None], SKY)
    rgb = np.minimum(np.floor(255 * col + 0.5), 255).astype(np.uint8)
    seg = np.where(hit, np.where(label >= 0, P_BODY[np.maximum(label, 0)] + 1, 0), -1)
    label = np.where(hit, label, -1)
    depth = np.where(hit, best, FAR)
    tie = (label >= 0) & (second - best < 1e-5 + 1e-6 * np.where(np.isfinite(best), best, 0.0))
    amb = hit & (amb | tie | ((label == -2) & near_line))
    return (rgb.reshape(H, W, 3), depth.reshape(H, W), seg.reshape(H, W), label.reshape(H, W), amb.reshape(H, W))


def field_cast(field, eye, d, tmax):
    """First heightfield facet along each ray (tests only rays that go down): candidate cells from samples along the ray's ground
    track plus their 3 x 3 neighbourhoods, both triangles of each (Bullet's diagonal), float64."""
    h, mid, nx, ny, inv, off = field
    N = len(d)
    tf = np.full(N, np.inf)
    fn = np.tile([0.0, 0.0, 1.0], (N, 1))
    for r in range(N):
        if d[r, 2] >= 0:
            continue
        gx0, gy0 = eye[0] * inv + off, eye[1] * inv + off
        gdx, gdy = d[r, 0] * inv, d[r, 1] * inv
        t1 = min(tmax[r], FAR)
        for g0, gd, n1 in ((gx0, gdx, nx - 1), (gy0, gdy, ny - 1)):     # leave the grid's footprint: plane only
            if gd != 0:
                t1 = min(t1, max((0 - g0) / gd, (n1 - g0) / gd))
        if not np.isfinite(t1) or t1 < NEAR:
            continue
        ts = np.linspace(NEAR, t1, max(int((t1 - NEAR) / 0.02) + 2, 2))     # < 0.05 m cells: every crossed cell is next to a sample
        ci, cj = np.floor(gx0 + ts * gdx).astype(int), np.floor(gy0 + ts * gdy).astype(int)
        nb = np.array([(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)])
        cells = np.unique((np.stack([ci, cj], 1)[:, None, :] + nb[None]).reshape(-1, 2), axis=0)
        cells = cells[(cells[:, 0] >= 0) & (cells[:, 0] <= nx - 2) & (cells[:, 1] >= 0) & (cells[:, 1] <= ny - 2)]
        if not len(cells):
            continue
        i, j = cells[:, 0], cells[:, 1]
        h00, h10 = h[j * nx + i] - mid, h[j * nx + i + 1] - mid
        h01, h11 = h[(j + 1) * nx + i] - mid, h[(j + 1) * nx + i + 1] - mid
        u0, v0 = gx0 - i, gy0 - j
        with np.errstate(divide="ignore", invalid="ignore"):
            a, b = h10 - h00, h01 - h00
            tl = (h00 + u0 * a + v0 * b - eye[2]) / (d[r, 2] - gdx * a - gdy * b)
            u, v = u0 + tl * gdx, v0 + tl * gdy
            okl = (u >= -1e-9) & (v >= -1e-9) & (u + v <= 1 + 1e-9) & (tl >= NEAR) & (tl <= t1)
            a2, b2 = h01 - h11, h10 - h11
            tu = (h11 + (1 - u0) * a2 + (1 - v0) * b2 - eye[2]) / (d[r, 2] + gdx * a2 + gdy * b2)
            u, v = u0 + tu * gdx, v0 + tu * gdy
            oku = (u <= 1 + 1e-9) & (v <= 1 + 1e-9) & (u + v >= 1 - 1e-9) & (tu >= NEAR) & (tu <= t1)
        cand = np.concatenate([np.where(okl, tl, np.inf), np.where(oku, tu, np.inf)])
        k = int(np.argmin(cand))
        if np.isfinite(cand[k]):
            tf[r] = cand[k]
            m = k % len(cells)
            gx, gy = ((a[m] * inv, b[m] * inv) if k < len(cells) else (-a2[m] * inv, -b2[m] * inv))
            nrm = np.array([-gx, -gy, 1.0])
            fn[r] = nrm / np.linalg.norm(nrm)
    return tf, fn


def _interior(lab):
    """pixels whose 3 x 3 neighbourhood holds one label (border pixels excluded)"""
    H, W = lab.shape
    ok = np.zeros_like(lab, dtype=bool)
    c = lab[1:-1, 1:-1]
    m = np.ones_like(c, dtype=bool)
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            m &= lab[1 + a:H - 1 + a, 1 + b:W - 1 + b] == c
    ok[1:-1, 1:-1] = m
    return ok


def compare(env, ids, W, H, full_ids=None, field_of=None):
    """Render rows `ids` of env on the GPU and check every one against the numpy caster (at most `full_ids` of them)."""
    import torch
    rgb, extra = env.render(env_ids=ids, width=W, height=H, depth=True, segmentation=True)
    torch.cuda.synchronize()
    rgb, dep, seg = rgb.cpu().numpy(), extra["depth"].cpu().numpy(), extra["segmentation"].cpu().numpy()
    assert rgb.shape == (len(ids), H, W, 3) and rgb.dtype == np.uint8
    assert dep.shape == (len(ids), H, W) and dep.dtype == np.float32 and seg.dtype == np.int16
    state = env.state.cpu().numpy()
    arm = env.mark == "arm"
    for k, e in enumerate(ids):
        if full_ids is not None and e not in full_ids:
            continue
        field = field_of(e) if field_of else None
        nrgb, ndep, nseg, lab, amb = cast(state, e, arm, W, H, field)
        inner = _interior(nseg)
        assert np.array_equal(seg[k][inner], nseg[inner]), (e, W, H, int((seg[k][inner] != nseg[inner]).sum()))
        assert (seg[k] == nseg).mean() >= 0.99, (e, W, H, (seg[k] == nseg).mean())
        pin = _interior(lab) & ~amb
        err = np.abs(dep[k].astype(np.float64) - ndep)
        assert np.all(err[pin] <= 1e-4 * ndep[pin] + 1e-5), (e, W, H, float((err - 1e-4 * ndep)[pin].max()))
        drgb = np.abs(rgb[k].astype(int) - nrgb.astype(int)).max(-1)
        assert np.all(drgb[pin] <= 2), (e, W, H, int((drgb[pin] > 2).sum()), int(drgb[pin].max()))
        assert pin.mean() > 0.5


def _steps(env, n, seed=0):
    import torch
    rng = np.random.RandomState(seed)
    lo, hi = np.minimum(env.action_space.low, env.action_space.high), np.maximum(env.action_space.low, env.action_space.high)
    for _ in range(n):
        env.step(torch.as_tensor(rng.uniform(lo, hi, (env.num_envs, env.action_dim)).astype(np.float32), device=env.device))


# ---------------------------------------------------------------- a. the single env returns a real frame
def test_single_env_rgb_array_is_a_frame():
    from rex_gym_amd.envs.gym.walk_env import RexWalkEnv
    env = RexWalkEnv()
    env.reset()
    img = env.render("rgb_array")
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (360, 480, 3)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 1
    assert env.render("human").size == 0
    env._cam_dist, env._cam_yaw = 2.0, 45        # the reference's attributes steer the camera
    far = env.render("rgb_array")
    assert far.shape == (360, 480, 3) and not np.array_equal(far, img)
    env.close()


# ---------------------------------------------------------------- b. against the numpy ray caster
@pytest.mark.parametrize("W,H", [(64, 48), (480, 360)])
def test_walk_ik_batch_after_random_steps(W, H):
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(8, task="walk", signal_type="ik", seed=3)
    env.reset()
    _steps(env, 30)
    compare(env, list(range(8)), W, H, full_ids=None if W == 64 else [0, 5])
    env.close()


@pytest.mark.parametrize("W,H", [(64, 48), (480, 360)])
def test_crouched_standup(W, H):
    from rex_gym_amd.envs.gym.standup_env import RexStandupEnv
    env = RexStandupEnv()
    env.reset()
    compare(env._batch, [0], W, H)
    env.close()


@pytest.mark.parametrize("W,H", [(64, 48), (480, 360)])
def test_mark_arm(W, H):
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(4, task="walk", signal_type="ik", mark="arm", seed=1)
    env.reset()
    _steps(env, 10)
    compare(env, [0, 1, 2, 3], W, H, full_ids=None if W == 64 else [2])
    env.close()


@pytest.mark.parametrize("W,H", [(64, 48), (480, 360)])
def test_mixed_task_batch_renders_state_indices(W, H):
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(48, task="mixed", signal_type="ik", seed=11)
    env.reset()
    _steps(env, 12, seed=4)
    ids = [0, 7, 19, 30, 47]
    compare(env, ids, W, H, full_ids=None if W == 64 else [7, 30])
    env.close()


# ---------------------------------------------------------------- c. heightfield
def test_random_terrain_ground_depth():
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(4, task="walk", signal_type="ik", terrain_type="random", terrain_pool=8, seed=2)
    env.reset()
    _steps(env, 5)
    import torch
    W, H = 64, 48
    rgb, extra = env.render(width=W, height=H, depth=True, segmentation=True)
    torch.cuda.synchronize()
    dep, seg = extra["depth"].cpu().numpy(), extra["segmentation"].cpu().numpy()
    state = env.state.cpu().numpy()
    heights, mids = env.terrain_heights.cpu().numpy().astype(np.float64), env.terrain_mids.cpu().numpy().astype(np.float64)
    k = heights.shape[0]
    episode = state[45].view(np.int32)          # REX_S_EPISODE
    for g in range(4):
        t = (g + 977 * int(episode[g])) % k
        field = (heights[t], mids[t], 256, 256, 20.0, 127.5)
        _, ndep, nseg, lab, _ = cast(state, g, False, W, H, field)
        inner = _interior(nseg) & (nseg == 0)
        # no occluding ridge inside the neighbourhood
        pad = np.pad(ndep, 1, mode="edge")
        win = np.stack([pad[1 + a:H + 1 + a, 1 + b:W + 1 + b] for a in (-1, 0, 1) for b in (-1, 0, 1)])
        smooth = (win.max(0) - win.min(0)) < 0.25 * ndep     # (a tilted plane alone changes by ~6 % across 3 pixels here)
        m = inner & smooth
        assert m.sum() > 0.3 * W * H
        assert np.array_equal(seg[g][inner], nseg[inner])
        err = np.abs(dep[g].astype(np.float64) - ndep)
        assert np.all(err[m] <= 1e-4 * ndep[m] + 1e-5), (g, float((err - 1e-4 * ndep)[m].max()))
        # the field is drawn: some ground pixels are off the z = 0 plane
        eye, d = rays(state[0:3, g].astype(np.float64), W, H)
        z = (eye[2] + ndep.reshape(-1) * d[:, 2]).reshape(H, W)
        assert np.abs(z[m]).max() > 1e-3
    env.close()


# ---------------------------------------------------------------- d. read-only and order-independent
def test_render_is_read_only_and_order_independent():
    import torch
    from rex_gym_amd import RexBatchEnv
    a = RexBatchEnv(8, task="walk", signal_type="ik", seed=9, check_actions=False)
    b = RexBatchEnv(8, task="walk", signal_type="ik", seed=9, check_actions=False)
    a.reset(); b.reset()
    rng = np.random.RandomState(1)
    for _ in range(20):
        act = torch.as_tensor(rng.uniform(-0.4, 0.4, (8, 2)).astype(np.float32), device=a.device)
        before = a.state.clone()
        a.render(width=64, height=48, depth=True, segmentation=True)
        torch.cuda.synchronize()
        assert torch.equal(before.view(torch.int32), a.state.view(torch.int32))
        a.step(act)
        b.step(act)
    torch.cuda.synchronize()
    assert torch.equal(a.state.view(torch.int32), b.state.view(torch.int32))
    full, fx = a.render(width=96, height=72, depth=True, segmentation=True)
    part, px = a.render(env_ids=[5, 2], width=96, height=72, depth=True, segmentation=True)
    again, ax = a.render(width=96, height=72, depth=True, segmentation=True)
    torch.cuda.synchronize()
    assert torch.equal(part, full[[5, 2]])
    assert torch.equal(px["depth"].view(torch.int32), fx["depth"][[5, 2]].view(torch.int32))
    assert torch.equal(px["segmentation"], fx["segmentation"][[5, 2]])
    assert torch.equal(full, again) and torch.equal(fx["depth"].view(torch.int32), ax["depth"].view(torch.int32))
    # an odd image size takes the element-by-element store path
    odd = a.render(env_ids=[3], width=97, height=73)
    assert odd.shape == (1, 73, 97, 3) and len(torch.unique(odd.reshape(-1, 3), dim=0)) > 1
    a.close(); b.close()


# ---------------------------------------------------------------- e. the camera follows the base
def test_centre_pixel_is_the_base():
    import torch
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(4, task="walk", signal_type="ik", seed=5)
    env.reset()
    _steps(env, 3)
    _, x = env.render(width=480, height=360, segmentation=True)
    torch.cuda.synchronize()
    seg = x["segmentation"].cpu().numpy()
    assert np.all(seg[:, 180, 240] == 1) and np.all(seg[:, 179, 239] == 1)
    assert x["depth"] is None
    env.close()


# ---------------------------------------------------------------- f. errors
def test_bad_arguments_raise_before_any_launch():
    import ctypes
    from rex_gym_amd import RexBatchEnv, _lib
    env = RexBatchEnv(4, task="walk", signal_type="ik")
    env.reset()
    with pytest.raises(IndexError):
        env.render(env_ids=[4])
    with pytest.raises(IndexError):
        env.render(env_ids=[-1])
    with pytest.raises(ValueError):
        env.render(width=0)
    with pytest.raises(ValueError):
        env.render(camera={"fov_deg": 0.0})
    with pytest.raises(NotImplementedError):
        env.render("human")
    # the C ABI's own checks (REX_EINVAL, nothing launched)
    L = _lib.lib()
    cam = _lib.RexCamera()
    assert L.rex_default_camera(ctypes.byref(cam)) == 0
    assert (cam.distance, cam.yaw_deg, cam.pitch_deg, cam.fov_deg) == (1.0, 0.0, -30.0, 60.0)
    assert abs(cam.near_plane - 0.1) < 1e-7 and cam.far_plane == 100.0
    import torch
    ids = torch.zeros(1, dtype=torch.int32, device=env.device)
    out = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=env.device)
    p = env._stream_ptr()
    assert L.rex_render(env._h, ctypes.byref(cam), ids.data_ptr(), 0, 4, 4, out.data_ptr(), None, None, p) == -1
    assert L.rex_render(env._h, ctypes.byref(cam), ids.data_ptr(), 1, 0, 4, out.data_ptr(), None, None, p) == -1
    assert L.rex_render(env._h, ctypes.byref(cam), ids.data_ptr(), 1, 4, 4097, out.data_ptr(), None, None, p) == -1
    assert L.rex_render(env._h, ctypes.byref(cam), ids.data_ptr(), 1, 4, 4, None, None, None, p) == -1
    assert L.rex_render(env._h, ctypes.byref(cam), ids.data_ptr(), 50000, 4096, 4096, out.data_ptr(), None, None, p) == -1
    for field, v in (("distance", 0.0), ("fov_deg", -1.0), ("near_plane", 0.0)):
        bad = _lib.RexCamera.from_buffer_copy(cam)
        setattr(bad, field, v)
        assert L.rex_render(env._h, ctypes.byref(bad), ids.data_ptr(), 1, 4, 4, out.data_ptr(), None, None, p) == -1
    torch.cuda.synchronize()
    assert int(out.sum()) == 0          # nothing was written
    env.close()


# ---------------------------------------------------------------- g. video
def test_policy_player_video(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import lzma
    import shutil
    from rex_gym_amd.agents import policy_player
    src = os.path.join(ROOT, "tests", "golden", "policies", "walk", "ik")
    dst = tmp_path / "walk_ik"
    dst.mkdir()
    for name in os.listdir(src):
        if name.endswith(".xz"):
            with lzma.open(os.path.join(src, name)) as f, open(dst / name[:-3], "wb") as g:
                shutil.copyfileobj(f, g)
        else:
            shutil.copyfile(os.path.join(src, name), dst / name)
    prefix = str(dst / "model.ckpt-2000000")
    gif = str(tmp_path / "walk.gif")
    policy_player.main(["--env", "walk", "--signal-type", "ik", "--checkpoint", prefix, "--num-envs", "2", "--max-steps", "50",
                        "--video", gif, "--video-env", "1"])
    im = Image.open(gif)
    assert im.n_frames == 50 and im.size == (480, 360)
    with pytest.raises(SystemExit):
        policy_player.main(["--env", "walk", "--checkpoint", prefix, "--fused", "--video", gif])
