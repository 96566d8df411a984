"""The HIP renderer (rex_render, csrc/rex_render.hip) on the GPU, against a numpy ray caster of this file.

The reference here is independent of the kernel: forward kinematics from env.state with the tables parsed from
rex_model_gen.h / rex_arm_model_gen.h, the primitives parsed from rex_render_gen.h, the camera restated from Bullet's
convention (rex_gym_amd.render.camera_eye_up + a look-at basis), and slab / capped-cylinder / plane / heightfield
intersections in float64.  The shading constants are the ones csrc/rex_render.h documents.

Sections a-g draw the default camera on the plane and on the reference's random terrain.  h-j hold the rest of the ABI to the
same caster at the same tolerances: every field of the camera (h), a caller-supplied heightfield pool with unequal sides and
cells, a shifted origin, relief under the plane and ridges that occlude (i), and the two store paths of store_pixels (j).
The mesh suite (tests/test_gpu_render_mesh.py) takes the camera, the ground (ground_shade) and the store checks from here."""
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
NEAR, FAR = 0.1, 100.0          # the planes of the default camera (rex_default_camera)
CAMERA = dict(distance=1.0, yaw_deg=0.0, pitch_deg=-30.0, fov_deg=60.0, near_plane=NEAR, far_plane=FAR)


def full_camera(camera=None):
    """the six fields of a camera: the ones given, the rest from the default"""
    cam = dict(CAMERA)
    cam.update(camera or {})
    assert set(cam) == set(CAMERA)
    return cam


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


def _quat(roll, yaw):
    """x y z w of Rz(yaw) Rx(roll)"""
    cr, sr, cy, sy = math.cos(roll / 2), math.sin(roll / 2), math.cos(yaw / 2), math.sin(yaw / 2)
    return [cy * sr, sy * sr, sy * cr, cy * cr]


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


def camera_rays(target, W, H, cam):
    return rays(target, W, H, cam["distance"], cam["yaw_deg"], cam["pitch_deg"], cam["fov_deg"])


def _hit_box(o, d, h, near=NEAR):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        ta, tb = (-h - o) * inv, (h - o) * inv
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    t0, t1 = lo.max(1), hi.min(1)
    a0, a1 = lo.argmax(1), hi.argmin(1)
    ok = t0 <= t1
    use0 = ok & (t0 >= near)
    use1 = ok & ~use0 & (t1 >= near)
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


def _hit_cyl(o, d, h, near=NEAR):
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
            ok = (a > 0) & (q >= 0) & (ts >= near) & (ts < best) & (np.abs(z) <= hz)
            best, which = np.where(ok, ts, best), np.where(ok, 0, which)
        for s, zc in ((1, -hz), (2, hz)):
            ts = (zc - o[2]) / d[:, 2]
            x, y = o[0] + ts * d[:, 0], o[1] + ts * d[:, 1]
            ok = (d[:, 2] != 0) & (ts >= near) & (ts < best) & (x * x + y * y <= r * r)
            best, which = np.where(ok, ts, best), np.where(ok, s, which)
        x, y = o[0] + best * d[:, 0], o[1] + best * d[:, 1]
        z = o[2] + best * d[:, 2]
        rr = np.sqrt(x * x + y * y)
        n = np.where((which == 0)[:, None], np.stack([x / rr, y / rr, np.zeros_like(x)], 1),
                     np.stack([np.zeros_like(x), np.zeros_like(x), np.where(which == 1, -1.0, 1.0)], 1))
        amb = np.isfinite(best) & ((np.abs(np.abs(z) - hz) < 1e-5) | (np.abs(rr - r) < 1e-5) & (which > 0))
    return best, n, amb


def cast(state, env, arm, W, H, field=None, camera=None, info=None):
    """numpy image of one env: (rgb uint8 [H, W, 3], depth [H, W], seg [H, W], label [H, W] (primitive index, -2 ground,
    -1 nothing), ambiguous [H, W] (a face edge within 1e-5 m or a checker line within float32 reach of the hit; on a
    heightfield the cases of ground_shade)).  camera: any of CAMERA's fields; field: field_cast's grid.  info: a dict that
    receives ground_shade's per-pixel facts [H, W] and "robot_t" (the robot's own hit, inf where none)."""
    cam = full_camera(camera)
    near, far = cam["near_plane"], cam["far_plane"]
    Rs, os_ = fk(state, env, arm)
    eye, d = camera_rays(os_[0], W, H, cam)
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
        t, nl, am = (_hit_box if P_KIND[k] == 0 else _hit_cyl)(o, dl, P_EXT[k], near)
        closer = t < best
        second = np.where(closer, best, np.minimum(second, t))
        best = np.where(closer, t, best)
        label = np.where(closer, k, label)
        normal = np.where(closer[:, None], nl @ ax.T, normal)
        amb = np.where(closer, am, amb)
    robot_t = best
    rgb, best, ground, hit, g = ground_shade(eye, d, best, normal, P_RGB[np.maximum(label, 0)], field, near, far)
    label = np.where(ground, -2, label)
    seg = np.where(hit, np.where(label >= 0, P_BODY[np.maximum(label, 0)] + 1, 0), -1)
    label = np.where(hit, label, -1)
    depth = np.where(hit, best, far)
    tie = (label >= 0) & (second - best < 1e-5 + 1e-6 * np.where(np.isfinite(best), best, 0.0))
    amb = hit & (amb | tie | ((label == -2) & g["near_line"]) | g["amb"])
    if info is not None:
        info.update({k: v.reshape(H, W) for k, v in g.items()}, robot_t=robot_t.reshape(H, W))
    return (rgb.reshape(H, W, 3), depth.reshape(H, W), seg.reshape(H, W), label.reshape(H, W), amb.reshape(H, W))


def ground_shade(eye, d, best, normal, alb, field, near, far):
    """The rest of a pixel behind the robot's nearest hit `best` [N] (inf: none; `normal` [N, 3] either side, `alb` [N, 3]): the
    z = 0 plane and, with `field`, the heightfield in front of it, the far plane, sky, checker and Lambert shading.  One function
    for the collision and the mesh reference.  -> rgb uint8 [N, 3], t [N] of the nearest hit, ground [N] (the ground is it),
    hit [N] (something within the far plane), facts: a dict of [N] arrays --
      near_line  a ground hit within float32 reach of a checker line
      amb        a heightfield pixel no float32 caster can be held to: a grazing facet (|n . d| / |d| < 0.05: the hit
                 parameter divides by d_z - g . grad h), or another candidate (facet, plane, robot) within 1e-3 m of the first
                 along the ray -- a nearer tie; a depth step to a facet further off than that stays in the comparison
      amb_rgb    a facet hit within 1e-4 grid units of a cell edge or the diagonal: the normal switches there, the depth not
      kind       0 nothing, 1 plane, 2 field, 3 robot;  inside: the hit's (x, y) within the grid's footprint
      far_sky    nothing within the far plane, though the ray goes down (ground beyond the far plane)
      gap        field pixels: metres along the ray from the hit facet to the next candidate facet behind it (inf: none)
      clipped    the footprint cut the ray's range;  field_t: the field's first facet whatever the robot hides (inf: none)"""
    N = len(d)
    dl = np.linalg.norm(d, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tplane = np.where(d[:, 2] < 0, -eye[2] / d[:, 2], np.inf)
    tg = np.where(tplane >= near, tplane, np.inf)
    gn = np.tile([0.0, 0.0, 1.0], (N, 1))
    facts = dict(amb=np.zeros(N, bool), amb_rgb=np.zeros(N, bool), gap=np.full(N, np.inf), clipped=np.zeros(N, bool),
                 field_t=np.full(N, np.inf))
    on_field = np.zeros(N, bool)
    reach = np.ones(N)                # the growth of a hit point's float32 error along the ray: 1 / (|n . d| / |d|) on a facet
    if field is not None:
        tr = field_cast(field, eye, d, near, far)
        tf = tr["t"]
        on_field = (tf <= best) & (tf < tg)          # the first facet in [near, min(plane, far, robot)]
        with np.errstate(invalid="ignore"):
            tie = (tr["gap"] < 1e-3) | ((tplane - tf) * dl < 1e-3) | (np.abs(best - tf) * dl < 1e-3)
        facts.update(amb=np.isfinite(tf) & (tf <= best + 1e-3 / dl) & (tr["graze"] | tie), amb_rgb=on_field & tr["edge"],
                     gap=np.where(on_field, tr["gap"], np.inf), clipped=tr["clipped"], field_t=tf)
        tg = np.where(on_field, tf, tg)
        gn = np.where(on_field[:, None], tr["n"], gn)
        reach = np.where(on_field, 1.0 / np.maximum(tr["ndot"], 0.05), 1.0)
    ground = tg < best
    best = np.where(ground, tg, best)
    normal = np.where(ground[:, None], gn, normal)
    hit = best <= far
    hx, hy = eye[0] + best * d[:, 0], eye[1] + best * d[:, 1]
    with np.errstate(invalid="ignore"):
        even = (np.floor(hx) + np.floor(hy)) % 2 == 0
        tol = (1e-5 + 2e-6 * best) * reach       # float32 hit points drift with the distance (eye + t d, t up to 100 m)
        near_line = (np.abs(hx - np.round(hx)) < tol) | (np.abs(hy - np.round(hy)) < tol)
    alb = np.where(ground[:, None], np.where(even[:, None], CHECK_A, CHECK_B), alb)
    flip = (normal * d).sum(1) > 0
    normal = np.where(flip[:, None], -normal, normal)
    lam = AMBIENT + DIFFUSE * np.maximum(0.0, normal @ LIGHT)
    col = np.where(hit[:, None], alb * lam[:, None], SKY)
    rgb = np.minimum(np.floor(255 * col + 0.5), 255).astype(np.uint8)
    facts["amb"] &= hit
    facts["amb_rgb"] &= hit
    facts["near_line"] = ground & hit & near_line
    facts["kind"] = np.where(~hit, 0, np.where(~ground, 3, np.where(on_field, 2, 1)))
    facts["far_sky"] = ~hit & (d[:, 2] < 0)
    facts["inside"] = hit & field_inside(field, hx, hy) if field is not None else np.zeros(N, bool)
    return rgb, best, ground, hit, facts


def field_inside(field, x, y):
    """(x, y) within the footprint of the grid"""
    _, _, nx, ny, inv_x, inv_y, off_x, off_y = field
    with np.errstate(invalid="ignore"):
        gx, gy = x * inv_x + off_x, y * inv_y + off_y
        return (gx >= 0) & (gx <= nx - 1) & (gy >= 0) & (gy <= ny - 1)


def field_cast(field, eye, d, near=NEAR, far=FAR):
    """The heightfield along each ray, whatever the robot hides: field = (heights [ny * nx] float64, mid, nx, ny, 1 / cell_x,
    1 / cell_y, off_x, off_y) with off = 0.5 (n - 1) - origin / cell (rex_set_heightfield; vertex index = x / cell + off).
    Each ray's range [near, min(plane, far)] is clipped to the grid's footprint on both axes (a ray may start outside it; a ray
    parallel to an axis is inside or outside by its start); candidate cells are those of samples along the ground track, 0.4 of
    a cell apart on the axis the track crosses faster (the smaller cell side), plus their 3 x 3 neighbourhoods, so no crossed
    cell is left out; both triangles of each (Bullet's diagonal), float64.  -> a dict of [N] arrays: t of the first facet (inf:
    none), its unit normal n, ndot = |n . d| / |d|, graze (ndot < 0.05), edge (the hit within 1e-4 grid units of a cell edge or
    the diagonal), gap (metres along the ray to the next candidate facet, inf: none), clipped."""
    h, mid, nx, ny, inv_x, inv_y, off_x, off_y = field
    N = len(d)
    dl = np.linalg.norm(d, axis=1)
    out = dict(t=np.full(N, np.inf), n=np.tile([0.0, 0.0, 1.0], (N, 1)), ndot=np.ones(N), graze=np.zeros(N, bool),
               edge=np.zeros(N, bool), gap=np.full(N, np.inf), clipped=np.zeros(N, bool))
    gx0, gy0 = eye[0] * inv_x + off_x, eye[1] * inv_y + off_y
    nb = np.array([(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)])
    for r in range(N):
        gdx, gdy = d[r, 0] * inv_x, d[r, 1] * inv_y
        tend = min(far, -eye[2] / d[r, 2]) if d[r, 2] < 0 else far
        t0, t1, outside = near, tend, False
        for g0, gd, n1 in ((gx0, gdx, nx - 1), (gy0, gdy, ny - 1)):     # outside the grid's footprint: plane only
            if gd != 0:
                ta, tb = sorted(((0 - g0) / gd, (n1 - g0) / gd))
                t0, t1 = max(t0, ta), min(t1, tb)
            elif g0 < 0 or g0 > n1:
                outside = True
        out["clipped"][r] = outside or t0 > near or t1 < tend
        if outside or not t0 <= t1:
            continue
        ts = np.linspace(t0, t1, int((t1 - t0) * max(abs(gdx), abs(gdy)) / 0.4) + 2)
        ci, cj = np.floor(gx0 + ts * gdx).astype(int), np.floor(gy0 + ts * gdy).astype(int)
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
            okl = (u >= -1e-9) & (v >= -1e-9) & (u + v <= 1 + 1e-9) & (tl >= near) & (tl <= tend)
            ul, vl = u, v
            a2, b2 = h01 - h11, h10 - h11
            tu = (h11 + (1 - u0) * a2 + (1 - v0) * b2 - eye[2]) / (d[r, 2] + gdx * a2 + gdy * b2)
            u, v = u0 + tu * gdx, v0 + tu * gdy
            oku = (u <= 1 + 1e-9) & (v <= 1 + 1e-9) & (u + v >= 1 - 1e-9) & (tu >= near) & (tu <= tend)
        cand = np.concatenate([np.where(okl, tl, np.inf), np.where(oku, tu, np.inf)])
        k = int(np.argmin(cand))
        if np.isfinite(cand[k]):
            out["t"][r] = cand[k]
            m = k % len(cells)
            gx, gy = ((a[m] * inv_x, b[m] * inv_y) if k < len(cells) else (-a2[m] * inv_x, -b2[m] * inv_y))
            nrm = np.array([-gx, -gy, 1.0])
            nrm /= np.linalg.norm(nrm)
            out["n"][r] = nrm
            out["ndot"][r] = abs(nrm @ d[r]) / dl[r]
            uh, vh = (ul[m], vl[m]) if k < len(cells) else (u[m], v[m])
            out["edge"][r] = min(abs(uh), abs(vh), abs(1 - uh), abs(1 - vh), abs(uh + vh - 1)) < 1e-4
            rest = np.delete(cand, k)
            out["gap"][r] = (rest.min() - cand[k]) * dl[r] if len(rest) else np.inf
    out["graze"] = np.isfinite(out["t"]) & (out["ndot"] < 0.05)
    return out


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


def compare(env, ids, W, H, full_ids=None, field_of=None, camera=None):
    """Render rows `ids` of env on the GPU and check every one against the numpy caster (at most `full_ids` of them).
    -> per checked row, cast()'s facts and "compared" (the pixels held to the depth and colour bounds)."""
    import torch
    rgb, extra = env.render(env_ids=ids, width=W, height=H, depth=True, segmentation=True, camera=camera)
    torch.cuda.synchronize()
    rgb, dep, seg = rgb.cpu().numpy(), extra["depth"].cpu().numpy(), extra["segmentation"].cpu().numpy()
    assert rgb.shape == (len(ids), H, W, 3) and rgb.dtype == np.uint8
    assert dep.shape == (len(ids), H, W) and dep.dtype == np.float32 and seg.dtype == np.int16
    state = env.state.cpu().numpy()
    arm = env.mark == "arm"
    facts = []
    for k, e in enumerate(ids):
        if full_ids is not None and e not in full_ids:
            continue
        field = field_of(e) if field_of else None
        info = {}
        nrgb, ndep, nseg, lab, amb = cast(state, e, arm, W, H, field, camera, info)
        inner = _interior(nseg)
        assert np.array_equal(seg[k][inner], nseg[inner]), (e, W, H, int((seg[k][inner] != nseg[inner]).sum()))
        assert (seg[k] == nseg).mean() >= 0.99, (e, W, H, (seg[k] == nseg).mean())
        pin = _interior(lab) & ~amb
        err = np.abs(dep[k].astype(np.float64) - ndep)
        assert np.all(err[pin] <= 1e-4 * ndep[pin] + 1e-5), (e, W, H, float((err - 1e-4 * ndep)[pin].max()))
        drgb = np.abs(rgb[k].astype(int) - nrgb.astype(int)).max(-1)
        flat = pin & ~info["amb_rgb"]
        assert np.all(drgb[flat] <= 2), (e, W, H, int((drgb[flat] > 2).sum()), int(drgb[flat].max()))
        assert pin.mean() > 0.5
        info["compared"] = pin
        facts.append(info)
    return facts


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
        field = (heights[t], mids[t], 256, 256, 20.0, 20.0, 127.5, 127.5)
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


# ---------------------------------------------------------------- h. cameras other than the default, on the plane
CAMERAS = {
    "default": {},
    "quadrant": dict(distance=2.5, yaw_deg=135.0, pitch_deg=-50.0, fov_deg=40.0),          # another quadrant, a narrow fov
    "near_far": dict(distance=0.6, yaw_deg=-100.0, pitch_deg=-10.0, fov_deg=90.0, near_plane=0.3, far_plane=3.0),
    "near_cut": dict(distance=0.3, yaw_deg=-100.0, pitch_deg=-10.0, fov_deg=90.0, near_plane=0.28, far_plane=3.0),  # the near plane cuts the base
    "down": dict(distance=1.5, yaw_deg=90.0, pitch_deg=-89.0, fov_deg=60.0),               # straight down: cos(pitch) ~ 0
    "fov120": dict(fov_deg=120.0),                                                         # the horizon is in the picture
}
# 80 x 40 and 40 x 80: tan_x comes from the aspect ratio; 63 x 47: the centre column has d_x == 0 exactly
PLANE_CASES = [("quadrant", 64, 48), ("near_far", 64, 48), ("near_cut", 64, 48), ("down", 64, 48), ("default", 80, 40), ("default", 40, 80),
               ("default", 63, 47), ("fov120", 64, 48)]


LIFTED = 3


def plane_batch(mark):
    """4 envs on the plane after a few random steps.  Early in an episode the envs of a batch still hold one pose and would give one
    picture, so each base is then moved and turned by its own amount (the renderer reads the state and nothing else): a
    row drawn from another env's state shows, and every env has its own checker phase.  Env LIFTED hangs 1.5 m up: from
    there the far-3 camera sees ground beyond its far plane in more than a fifth of the picture."""
    import torch
    from rex_gym_amd import RexBatchEnv
    env = RexBatchEnv(4, task="walk", signal_type="ik", mark=mark, seed=6)
    env.reset()
    _steps(env, 8, seed=2)
    pose = env.state[0:7].cpu().numpy()
    for g in range(4):
        pose[0:2, g] += [0.37 * g, -0.21 * g]
        pose[3:7, g] = _quat(0.04 * g, 0.5 * g)
    pose[2, LIFTED] = 1.5
    env.state[0:7] = torch.as_tensor(pose, device=env.device)       # REX_S_POS, REX_S_QUAT; on the env's stream
    torch.cuda.synchronize()
    return env


@pytest.fixture(scope="module")
def plane_env():
    """mark -> plane_batch(mark), shared by the cases of this file"""
    envs = {}

    def get(mark):
        if mark not in envs:
            envs[mark] = plane_batch(mark)
        return envs[mark]
    yield get
    for env in envs.values():
        env.close()


def near_cut_pixels(state, env, arm, W, H, camera):
    """From the reference alone: the robot pixels whose hit the camera's near plane moved (cut primitives)."""
    info, wide = {}, {}
    cast(state, env, arm, W, H, None, camera, info)
    cast(state, env, arm, W, H, None, dict(camera, near_plane=NEAR), wide)
    return int((np.isfinite(wide["robot_t"]) & (wide["robot_t"] != info["robot_t"])).sum())


@pytest.mark.parametrize("mark", ["base", "arm"])
@pytest.mark.parametrize("name,W,H", PLANE_CASES)
def test_cameras_on_the_plane(plane_env, mark, name, W, H):
    env = plane_env(mark)
    ids = [0, 1, 3]
    facts = compare(env, ids, W, H, camera=CAMERAS[name])
    if name == "near_far":
        # Else the far plane tests nothing: ground beyond 3 m along the view axis is sky.  From an eye 0.5 m up that is a tenth of
        # this picture (the rows within 10 degrees under the horizon); from the lifted base (LIFTED) more than a fifth.
        f = facts[ids.index(LIFTED)]
        assert f["far_sky"].mean() >= 0.2, float(f["far_sky"].mean())
        assert all(np.all(g["kind"][g["far_sky"]] == 0) for g in facts)
    if name == "near_cut":
        # At 0.6 m the robot's nearest face is 0.4 m from the eye and a near plane at 0.3 m cuts nothing; this one, 2 cm in
        # front of the base's centre, takes hit_box's "inside a primitive the exit is the hit" branch.
        state = env.state.cpu().numpy()
        for e in ids:
            cut = near_cut_pixels(state, e, mark == "arm", W, H, CAMERAS[name])
            assert cut >= 10, (e, cut)


# ---------------------------------------------------------------- i. a caller-supplied heightfield pool
FIELD_NX, FIELD_NY, FIELD_CELL, FIELD_ORIGIN = 40, 24, (0.10, 0.16), (0.6, -0.3, 0.10)
FIELD_CAMERAS = ["default", "quadrant", "near_far", "down"]


def custom_fields():
    """[2, ny, nx] float32: ridges of 0.28 m on the grid's own world coordinates (facets up to ~50 degrees, part of the relief
    under the plane once the pool's mid is taken off); field 1 another phase, seed and level, so that its mid differs."""
    x = (np.arange(FIELD_NX) - 0.5 * (FIELD_NX - 1)) * FIELD_CELL[0] + FIELD_ORIGIN[0]
    y = (np.arange(FIELD_NY) - 0.5 * (FIELD_NY - 1)) * FIELD_CELL[1] + FIELD_ORIGIN[1]
    X, Y = np.meshgrid(x, y)
    f0 = 0.30 + 0.28 * np.sin(4 * X) * np.cos(3 * Y) + 0.02 * np.random.RandomState(21).uniform(size=X.shape)
    f1 = 0.38 + 0.28 * np.sin(4 * X + 1.3) * np.cos(3 * Y - 0.7) + 0.02 * np.random.RandomState(22).uniform(size=X.shape)
    f = np.stack([f0, f1]).astype(np.float32)
    assert abs(f[1].min() - f[0].min()) >= 0.05 and abs(f[1].max() - f[0].max()) >= 0.05
    return f


def field_tuple(heights, mid):
    """field_cast's grid of one field of the pool (float64)"""
    inv_x, inv_y = 1.0 / FIELD_CELL[0], 1.0 / FIELD_CELL[1]
    return (np.asarray(heights, dtype=np.float64).reshape(-1), float(mid), FIELD_NX, FIELD_NY, inv_x, inv_y,
            0.5 * (FIELD_NX - 1) - FIELD_ORIGIN[0] * inv_x, 0.5 * (FIELD_NY - 1) - FIELD_ORIGIN[1] * inv_y)


def field_height(field, x, y):
    """the ground under (x, y): the facet's height where the field is above the plane, else 0"""
    h, mid, nx, ny, inv_x, inv_y, off_x, off_y = field
    gx, gy = x * inv_x + off_x, y * inv_y + off_y
    if not (0 <= gx <= nx - 1 and 0 <= gy <= ny - 1):
        return 0.0
    i, j = min(int(gx), nx - 2), min(int(gy), ny - 2)
    u, v = gx - i, gy - j
    h00, h10, h01, h11 = h[j * nx + i], h[j * nx + i + 1], h[(j + 1) * nx + i], h[(j + 1) * nx + i + 1]
    z = h00 + u * (h10 - h00) + v * (h01 - h00) if u + v <= 1 else h11 + (1 - u) * (h01 - h11) + (1 - v) * (h10 - h11)
    return max(z - mid, 0.0)


# base (x, y), height above the ground under it, quaternion.  The renderer reads the state and nothing else, so the bases are put
# where the cases are and not where a robot would settle on such slopes.
FIELD_POSES = [((0.6, -0.3), 0.25, _quat(0.0, 0.0)),       # above the centre of the field
               ((2.25, 1.24), 0.08, _quat(0.0, 0.0)),      # 0.3 m inside a corner of the footprint: most rays leave it; the legs in the field
               ((-1.7, -0.3), 0.45, _quat(0.0, 0.0)),      # outside the footprint, the field in view: rays start outside the grid
               ((0.2, 0.4), 0.03, _quat(0.3, 1.0))]        # rolled and turned, lower still: ridges in front of the legs and the body


def custom_field_scene():
    """-> (env, state [words, 4] numpy, field_of(env index)): 4 envs on the pool of custom_fields(), two of them one episode
    further (so the envs use both fields, picked by (g + 977 episode) mod 2), the bases at FIELD_POSES."""
    import torch
    from rex_gym_amd import RexBatchEnv
    fields = custom_fields()
    env = RexBatchEnv(4, task="walk", signal_type="ik", seed=8, terrain_type="custom", heightfield=fields, heightfield_cell=FIELD_CELL,
                      heightfield_origin=FIELD_ORIGIN, init_height=0.9)
    env.reset()
    env.reset([1, 2])
    torch.cuda.synchronize()
    state = env.state.cpu().numpy()
    episode = state[45].view(np.int32)          # REX_S_EPISODE
    assert len(set(int(v) for v in episode)) == 2
    mids = env.terrain_mids.cpu().numpy()
    grids = [field_tuple(fields[t], mids[t]) for t in range(2)]
    assert abs(grids[0][1] - grids[1][1]) >= 0.05
    pick = [(g + 977 * int(episode[g])) % 2 for g in range(4)]
    assert set(pick) == {0, 1} and pick != [0, 1, 0, 1]       # both fields, and not what the env index alone would pick
    pose = np.zeros((7, 4), np.float32)
    for g, ((x, y), dz, q) in enumerate(FIELD_POSES):
        pose[:, g] = [x, y, field_height(grids[pick[g]], x, y) + dz] + q
    env.state[0:7] = torch.as_tensor(pose, device=env.device)       # REX_S_POS, REX_S_QUAT; on the env's stream
    torch.cuda.synchronize()
    return env, env.state.cpu().numpy(), lambda g: grids[pick[g]]


@pytest.fixture(scope="module")
def field_scene():
    env, state, field_of = custom_field_scene()
    yield env, state, field_of, {}
    env.close()


def field_counts(facts):
    """what a set of heightfield images exercises, from the reference's facts alone"""
    tot = dict(field=0, plane_inside=0, plane_outside=0, sky=0, occluded_facet=0, robot_over_field=0, field_over_robot=0, clipped=0)
    for f in facts:
        c, kind = f["compared"], f["kind"]
        tot["field"] += int((kind == 2).sum())
        tot["plane_inside"] += int(((kind == 1) & f["inside"]).sum())          # the field under the plane
        tot["plane_outside"] += int(((kind == 1) & ~f["inside"]).sum())
        tot["sky"] += int((kind == 0).sum())
        tot["clipped"] += int(f["clipped"].sum())
        tot["occluded_facet"] += int((c & (kind == 2) & np.isfinite(f["gap"]) & (f["gap"] > 0.3)).sum())
        tot["robot_over_field"] += int((c & (kind == 3) & np.isfinite(f["field_t"])).sum())
        tot["field_over_robot"] += int((c & (kind == 2) & np.isfinite(f["robot_t"])).sum())
    return tot


@pytest.mark.parametrize("name", FIELD_CAMERAS)
def test_custom_heightfield(field_scene, name):
    env, _, field_of, seen = field_scene
    seen[name] = compare(env, [0, 1, 2, 3], 64, 48, field_of=field_of, camera=CAMERAS[name])


def test_custom_heightfield_cases_cover(field_scene):
    """From the reference alone, over the 16 images of test_custom_heightfield: more than half of every image is compared; there
    are field pixels, plane pixels inside the footprint (the field under the plane) and outside it, sky, and rays the footprint
    clips; compared facets hide a second facet more than 0.3 m behind them; compared robot pixels have field behind them and
    compared field pixels the robot."""
    _, state, field_of, seen = field_scene
    facts = []
    for name in FIELD_CAMERAS:
        if name in seen:
            facts += seen[name]
            continue
        for g in range(4):
            info = {}
            _, _, _, lab, amb = cast(state, g, False, 64, 48, field_of(g), CAMERAS[name], info)
            info["compared"] = _interior(lab) & ~amb
            facts.append(info)
    tot = field_counts(facts)
    assert all(f["compared"].mean() >= 0.5 for f in facts)
    assert min(tot["field"], tot["plane_inside"], tot["plane_outside"], tot["sky"], tot["clipped"]) >= 20, tot
    assert tot["occluded_facet"] >= 20, tot          # a ridge in front of a facet more than 0.3 m further along the ray
    assert tot["robot_over_field"] >= 10 and tot["field_over_robot"] >= 10, tot


# ---------------------------------------------------------------- j. the store paths
def raw_render(env, fn, ids, W, H, rgb, dep, seg, camera=None):
    """rex_render / rex_render_visual through the C ABI: rgb, dep, seg are device addresses (dep, seg may be None)"""
    import ctypes
    cam = env._camera(camera)
    rc = getattr(env._L, fn)(env._h, ctypes.byref(cam), ids.data_ptr(), int(ids.numel()), W, H, rgb, dep, seg, env._stream_ptr())
    assert rc == 0, env._L.rex_last_error()


@pytest.mark.parametrize("W,H", [(61, 47), (33, 31), (65, 63)])
def test_odd_sizes_against_the_caster(plane_env, W, H):
    """W H % 4 != 0: the element-by-element stores.  61 x 47: three pixels left over; 33 x 31 = 1023: the image ends one pixel
    before a thread's group of four does; 65 x 63 = 4095: four tiles, the last thread of the last one ragged.  Two rows, so
    that the second image starts at an odd byte of rgb."""
    assert (W * H) % 4 == 3
    compare(plane_env("base"), [0, 1], W, H)


def check_vector_stores_equal_scalar_stores(env, fn):
    """The same two envs at 64 x 48 into aligned buffers (whole-dword stores) and into views 1 / 4 / 2 bytes into larger ones
    (element by element), together and one at a time -- the launcher has one flag for three buffers: byte for byte equal."""
    import torch
    W, H = 64, 48
    ids = torch.arange(2, dtype=torch.int32, device=env.device)
    n = 2 * W * H

    def run(o_rgb, o_dep, o_seg):
        bufs = [torch.zeros(size * n + 64, dtype=torch.uint8, device=env.device) for size in (3, 4, 2)]
        assert all(b.data_ptr() % 16 == 0 for b in bufs)
        raw_render(env, fn, ids, W, H, *[b.data_ptr() + o for b, o in zip(bufs, (o_rgb, o_dep, o_seg))])
        torch.cuda.synchronize()
        return [b[o:o + size * n].clone() for b, o, size in zip(bufs, (o_rgb, o_dep, o_seg), (3, 4, 2))]
    ref = run(0, 0, 0)
    rgb, x = env.render(env_ids=[0, 1], width=W, height=H, depth=True, segmentation=True,
                        geometry="visual" if fn == "rex_render_visual" else "collision")
    torch.cuda.synchronize()
    for a, b in zip(ref, (rgb, x["depth"], x["segmentation"])):
        assert torch.equal(a, b.reshape(-1).view(torch.uint8))
    assert len(torch.unique(ref[0])) > 8 and len(torch.unique(ref[2].view(torch.int16))) > 2
    for offs in ((1, 4, 2), (1, 0, 0), (0, 4, 0), (0, 0, 2)):
        out = run(*offs)
        for a, b, what in zip(ref, out, ("rgb", "depth", "segmentation")):
            assert torch.equal(a, b), (offs, what, int((a != b).sum()))


def check_nothing_outside_the_images(env, fn, W, H, want_dep, want_seg):
    """64 sentinel bytes in front of and behind each output: untouched; every element of the images written (they equal
    render()'s; depth was NaN, the segments 0x7B7B); sky (the 120 degree camera shows some) holds the far plane and segment -1."""
    import torch
    ids = torch.arange(2, dtype=torch.int32, device=env.device)
    n, pad = 2 * W * H, 64
    bufs = []
    for size, fill, want in ((3, 0x3C, True), (4, 0xFF, want_dep), (2, 0x7B, want_seg)):
        b = torch.full((pad + size * n + pad,), fill, dtype=torch.uint8, device=env.device)
        b[:pad] = 0x5A
        b[pad + size * n:] = 0x5A
        bufs.append(b if want else None)
    raw_render(env, fn, ids, W, H, *[b.data_ptr() + pad if b is not None else None for b in bufs], camera=CAMERAS["fov120"])
    rgb, x = env.render(env_ids=[0, 1], width=W, height=H, depth=True, segmentation=True, camera=CAMERAS["fov120"],
                        geometry="visual" if fn == "rex_render_visual" else "collision")
    torch.cuda.synchronize()
    for b, size, want in zip(bufs, (3, 4, 2), (rgb, x["depth"], x["segmentation"])):
        if b is None:
            continue
        assert bool((b[:pad] == 0x5A).all()) and bool((b[pad + size * n:] == 0x5A).all()), (W, H, size)
        assert torch.equal(b[pad:pad + size * n], want.reshape(-1).view(torch.uint8)), (W, H, size)
    dep, seg = x["depth"], x["segmentation"]
    assert not bool(torch.isnan(dep).any()) and not bool((seg == 0x7B7B).any())
    assert bool((seg == -1).any()) and bool((dep[seg == -1] == 100.0).all()) and bool((dep[seg != -1] <= 100.0).all())


def test_vector_stores_equal_scalar_stores(plane_env):
    check_vector_stores_equal_scalar_stores(plane_env("base"), "rex_render")


@pytest.mark.parametrize("want_dep,want_seg", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("W,H", [(61, 47), (64, 48)])
def test_nothing_outside_the_images(plane_env, W, H, want_dep, want_seg):
    check_nothing_outside_the_images(plane_env("base"), "rex_render", W, H, want_dep, want_seg)


def test_duplicate_env_ids(plane_env):
    import torch
    env = plane_env("base")
    full, fx = env.render(width=64, height=48, depth=True, segmentation=True)
    part, px = env.render(env_ids=[2, 2, 0], width=64, height=48, depth=True, segmentation=True)
    torch.cuda.synchronize()
    for a, b in ((part, full), (px["depth"].view(torch.int32), fx["depth"].view(torch.int32)), (px["segmentation"], fx["segmentation"])):
        assert torch.equal(a[0], a[1]) and torch.equal(a[0], b[2]) and torch.equal(a[2], b[0])
    assert not torch.equal(px["depth"][0].view(torch.int32), px["depth"][2].view(torch.int32))      # two envs, two pictures
