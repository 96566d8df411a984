"""The numpy reference of rex_kinematics, independent of the kernel (tests/test_kinematics_host.py, tests/test_gpu_kinematics.py).

  - link poses: fk() of tests/test_gpu_render.py (float64); the same recursion restated for float32 only to measure round-off floors
  - velocities: the textbook recursion  w_b = w_p + qd_j a_j,  v_b = v_p + w_p x (o_b - o_p)  with a_j the joint's axis in world;
    REX_S_LINVEL / REX_S_ANGVEL are the world velocity of the base link frame's origin and the world angular velocity
  - the toe: centre, axis, radius and half length of the toe cylinder entries of rex_render_gen.h (pinned to the physics geometry by
    tests/test_render_camera.py) plus REX_COLLISION_MARGIN on the radius; REX_TOE_Z is not used
  - the ground: the facet rule of field_height (tests/test_gpu_render.py) as a two-stage query -- the normal under the end's centre,
    then the lowest point of the end's rim along it, then the height and normal under that point -- with rexsim's rule beside the
    footprint (the grid coordinate is clamped to [0, n - 1 - 0.001]: the border's height holds on) and the facet ids of both queries.

A field is field_cast's tuple (heights [ny * nx], mid, nx, ny, 1 / cell_x, 1 / cell_y, off_x, off_y); None is the plane.  The grid
constants -- 1 / cell, the offsets, the clamp limit -- are float32 values formed in float32 arithmetic, as the product's host code and the
oracle hold them (grid_constants, clamp_limit); the random pool's 20, 127.5 are exact and its limit is 254.999f."""
import math
import re

import numpy as np

import test_gpu_render as col

BREAKING = 0.02                      # contact breaking threshold (include/rexsim.h, toe_in_reach)
MARGIN = float(re.search(r"#define\s+REX_COLLISION_MARGIN\s+([\d.eE+-]+)", col.SRC["rex_model_gen.h"]).group(1))
TOE_PRIMS = [int(k) for k in np.nonzero((col.P_KIND == 1) & np.isin(col.P_BODY, (3, 6, 9, 12)))[0]]      # one cylinder per leg, in leg order
assert [int(col.P_BODY[k]) for k in TOE_PRIMS] == [3, 6, 9, 12]
JLOWER, JUPPER = col._arr("rex_model_gen.h", "REX_JOINT_LOWER"), col._arr("rex_model_gen.h", "REX_JOINT_UPPER")
A_LOWER, A_UPPER = col._arr("rex_arm_model_gen.h", "REXA_LOWER"), col._arr("rex_arm_model_gen.h", "REXA_UPPER")


def num_motors(arm):
    return 18 if arm else 12


def episode_word(arm):
    return 13 + 2 * num_motors(arm) + 8            # REX_S_EPISODE; Lay<NM>::EPISODE


def _fk32(state, env, arm):
    """fk() of test_gpu_render in float32 arithmetic (for the round-off floors only)"""
    f = np.float32
    s = state[:, env].astype(f)
    x, y, z, w = s[3:7]
    one, two = f(1), f(2)
    R0 = np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                   [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                   [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype=f)
    rot = lambda k, a: col._axis_rot(k, float(a)).astype(f)      # the sine and cosine rounded to float32
    Rs, os_ = [R0], [s[0:3]]
    for b in range(1, 13):
        p = col.PARENT[b]
        Rs.append(Rs[p] @ rot(col.JAXIS[b - 1], s[13 + b - 1]))
        os_.append(os_[p] + Rs[p] @ col.JPOS[b - 1].astype(f))
    if arm:
        for k in range(6):
            p = col.A_PARENT[k]
            Rs.append(Rs[p] @ col.A_E0[k].astype(f) @ rot(2, f(col.A_SIGN[k]) * s[13 + 12 + k]))
            os_.append(os_[p] + Rs[p] @ col.A_POS[k].astype(f))
    return Rs, os_


def quat_of(R):
    """x y z w of a rotation matrix (float64), w >= 0"""
    R = np.asarray(R, np.float64)
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    val, vec = np.linalg.eigh(K)
    q = vec[:, -1]
    return q if q[3] >= 0 else -q


def clamp_limit(n):
    """the largest grid coordinate of an axis of n vertices as the product holds it: a float32 value, formed in float32 arithmetic
    (csrc/rexsim.hip rex_set_heightfield: `g.max_x = (float)(nx - 1) - 0.001f`; for n = 256 that is the 254.999f of rex_set_terrain and
    of HF_RANDOM in oracle/rex_oracle.c), widened"""
    return float(np.float32(n - 1) - np.float32(0.001))


def grid_constants(n, cell, origin):
    """-> (1 / cell, offset) of one axis as csrc/rexsim.hip rex_set_heightfield and orc_set_heightfield of oracle/rex_oracle.c form them
    (`g.inv_cx = 1.0f / cell_x; g.off_x = 0.5f * (float)(nx - 1) - origin_x * g.inv_cx`): float32 arithmetic, then widened, so that the
    reference stands on the grid the kernels see and not on one 1e-8 m beside it"""
    f = np.float32
    inv = f(1) / f(cell)
    return float(inv), float(f(0.5) * f(n - 1) - f(origin) * inv)


def ground_query(field, x, y, dtype=np.float64):
    """-> (height over the z = 0 plane, unit normal [3], facet id): the facet the point (x, y) stands on, 1 + 2 (cell index) + (upper
    triangle), where it is above the plane; else the plane, id 0"""
    f = dtype
    up = np.array([0, 0, 1], dtype=f)
    if field is None:
        return f(0), up, 0
    h, mid, nx, ny, inv_x, inv_y, off_x, off_y = field
    fx = min(max(f(x) * f(inv_x) + f(off_x), f(0)), f(clamp_limit(nx)))
    fy = min(max(f(y) * f(inv_y) + f(off_y), f(0)), f(clamp_limit(ny)))
    i, j = int(fx), int(fy)
    u, v = fx - f(i), fy - f(j)
    h00, h10, h01, h11 = (f(h[j * nx + i]), f(h[j * nx + i + 1]), f(h[(j + 1) * nx + i]), f(h[(j + 1) * nx + i + 1]))
    if u + v <= 1:
        z, gx, gy, upper = h00 + u * (h10 - h00) + v * (h01 - h00), (h10 - h00) * f(inv_x), (h01 - h00) * f(inv_y), 0
    else:
        z, gx, gy, upper = h11 + (f(1) - u) * (h01 - h11) + (f(1) - v) * (h10 - h11), (h11 - h01) * f(inv_x), (h11 - h10) * f(inv_y), 1
    z = z - f(mid)
    if not z > 0:
        return f(0), up, 0
    n = np.array([-gx, -gy, f(1)], dtype=f)
    return z, (n / np.sqrt(n @ n)).astype(f), 1 + 2 * (j * nx + i) + upper


def toe_points(centre, axis, radius, half, field, dtype=np.float64, shift=(0.0, 0.0)):
    """The two contact candidates of one toe cylinder (world centre and unit axis): per end e, the end's centre ce = centre -+ half axis,
    the normal n0 under it, the rim's lowest point along n0, P = ce - radius d / |d| with d = n0 - (n0 . axis) axis (P = ce when
    |d|^2 <= 1e-18: the axis is parallel to the normal), and the ground under P.  `shift` moves both query points in (x, y): the
    facet-stability probe of the tests.  -> per end a dict(pos, dist, normal, fid0, fid1, degenerate, centre)"""
    f = dtype
    out = []
    for e in range(2):
        ce = (centre + (f(-half) if e == 0 else f(half)) * axis).astype(f)
        _, n0, fid0 = ground_query(field, ce[0] + f(shift[0]), ce[1] + f(shift[1]), f)
        d = (n0 - (n0 @ axis) * axis).astype(f)
        dn2 = d @ d
        degenerate = not dn2 > 1e-18
        P = ce if degenerate else (ce - (f(radius) / np.sqrt(dn2)) * d).astype(f)
        h, n, fid1 = ground_query(field, P[0] + f(shift[0]), P[1] + f(shift[1]), f)
        out.append(dict(pos=P, dist=(P[2] - h) * n[2], normal=n, fid0=fid0, fid1=fid1, degenerate=degenerate, centre=ce))
    return out


def reference(state, env, arm, field=None, dtype=np.float64, shift=(0.0, 0.0)):
    """Every output of rex_kinematics for env `env` of `state` (numpy [words, n] float32), in `dtype` arithmetic: link_pos [NB, 3],
    link_rot [NB, 3, 3], link_quat [NB, 4] (from the float64 value of link_rot), link_linvel, link_angvel [NB, 3], toe_pos, toe_vel,
    toe_normal [8, 3], toe_dist [8], toe_in_reach [8] bool, base_body [9]; and what the tests sort cases by: fid0, fid1 [8] (the
    facets of the two queries), degenerate [8], toe_centre [4, 3] and toe_centre_vel [4, 3] (the cylinder's centre and its velocity)."""
    f = dtype
    nm = num_motors(arm)
    s = state[:, env].astype(f)
    Rs, os_ = col.fk(state, env, arm) if f == np.float64 else _fk32(state, env, arm)
    nb = len(Rs)
    qd = s[13 + nm:13 + 2 * nm]
    v, w = [s[7:10]], [s[10:13]]
    for b in range(1, nb):
        if b < 13:
            p, axis, rate = col.PARENT[b], Rs[b][:, col.JAXIS[b - 1]], qd[b - 1]
        else:
            p, axis, rate = col.A_PARENT[b - 13], f(col.A_SIGN[b - 13]) * Rs[b][:, 2], qd[12 + b - 13]
        v.append((v[p] + np.cross(w[p], os_[b] - os_[p])).astype(f))
        w.append((w[p] + rate * axis).astype(f))
    out = dict(link_pos=np.array(os_, dtype=f), link_rot=np.array(Rs, dtype=f), link_linvel=np.array(v, dtype=f), link_angvel=np.array(w, dtype=f))
    out["link_quat"] = np.array([quat_of(R) for R in Rs])
    R0 = Rs[0]
    out["base_body"] = np.concatenate([R0.T @ v[0], R0.T @ w[0], R0.T @ np.array([0, 0, -1], dtype=f)]).astype(f)
    keys = ("pos", "dist", "normal", "fid0", "fid1", "degenerate")
    toe = {k: [] for k in keys}
    toe_vel, centres, centre_vel = [], [], []
    for leg, k in enumerate(TOE_PRIMS):
        b = int(col.P_BODY[k])
        centre = (os_[b] + Rs[b] @ col.P_POS[k].astype(f)).astype(f)
        axis = (Rs[b] @ col.P_ROT[k][:, 2].astype(f)).astype(f)           # a cylinder's axis is its local z
        centres.append(centre)
        centre_vel.append(v[b] + np.cross(w[b], centre - os_[b]))
        for end in toe_points(centre, axis, float(col.P_EXT[k][0]) + MARGIN, float(col.P_EXT[k][2]), field, f, shift):
            for key in keys:
                toe[key].append(end[key])
            toe_vel.append((v[b] + np.cross(w[b], end["pos"] - os_[b])).astype(f))
    out.update(toe_pos=np.array(toe["pos"], dtype=f), toe_dist=np.array(toe["dist"], dtype=f), toe_normal=np.array(toe["normal"], dtype=f),
               toe_vel=np.array(toe_vel, dtype=f), fid0=np.array(toe["fid0"]), fid1=np.array(toe["fid1"]), degenerate=np.array(toe["degenerate"]),
               toe_centre=np.array(centres, dtype=f), toe_centre_vel=np.array(centre_vel, dtype=f))
    out["toe_in_reach"] = out["toe_dist"] < f(BREAKING)
    return out


def advance(state, env, arm, h):
    """The state of env `env` moved by h seconds along its own velocities, float64 [words]: position by the linear velocity, the
    quaternion by the exponential of w h (world frame: q' = exp(w h / 2) q), the joint angles by their rates."""
    nm = num_motors(arm)
    s = state[:, env].astype(np.float64).copy()
    s[0:3] += h * s[7:10]
    w = s[10:13]
    a = np.linalg.norm(w) * h
    ax = w / np.linalg.norm(w) if a != 0 else np.zeros(3)
    dx, dy, dz, dw = list(math.sin(a / 2) * ax) + [math.cos(a / 2)]
    x, y, z, ww = s[3:7]
    s[3:7] = [dw * x + dx * ww + dy * z - dz * y, dw * y - dx * z + dy * ww + dz * x, dw * z + dx * y - dy * x + dz * ww,
              dw * ww - dx * x - dy * y - dz * z]
    s[13:13 + nm] += h * s[13 + nm:13 + 2 * nm]
    return s


def random_terrain_field(heights, mids, t):
    """field tuple of entry t of the reference's random terrain pool (256 x 256 vertices, 5 cm cells, centred)"""
    return (np.asarray(heights[t], np.float64).reshape(-1), float(mids[t]), 256, 256, 20.0, 20.0, 127.5, 127.5)


# ---------------------------------------------------------------- the test scenes: synthetic states, fixed seeds, CPU only
# A scene is (mark, num_envs, ground).  Its synthetic columns -- the words 0 .. 13 + 2 NM of the state and the episode word, which picks the
# env's field -- are a function of the scene alone, so the round-off floors and the excluded shares are measured without a GPU over the
# very states the GPU test writes into env.state.  The first `keep` columns are left to the env (real states after random steps).
POOL = 8                                              # fields of the reference's random terrain
CUSTOM_NX, CUSTOM_NY, CUSTOM_CELL, CUSTOM_ORIGIN = 13, 9, (0.5, 0.7), (0.4, -0.3, 0.05)
CORNERS = ("degenerate", "off", "upside", "origin")
OFF_XY = {"plane": (7.5, -7.0), "random": (7.5, -7.0), "custom": (-5.5, 4.5)}       # beside every footprint (random: +-6.4 m; custom: x -2.6 .. 3.4, y -3.1 .. 2.5)


def custom_fields():
    """[2, 9, 13] float32: unequal cells (0.5 x 0.7 m), relief of 0.3 m, a third of it under the plane once the pool's mid is taken off"""
    return np.stack([np.random.RandomState(31 + t).uniform(0.0, 0.3 + 0.05 * t, (CUSTOM_NY, CUSTOM_NX)) for t in range(2)]).astype(np.float32)


def custom_mids(fields):
    return np.array([0.5 * (float(f.min()) + float(f.max())) - CUSTOM_ORIGIN[2] for f in fields], dtype=np.float32)      # RexBatchEnv(heightfield=...)


def scene_fields(ground, heights=None, mids=None):
    """ground -> the list of field tuples of its pool (None: the plane); heights / mids: the env's own tensors, else rebuilt here"""
    if ground == "plane":
        return None
    if ground == "random":
        if heights is None:
            from rex_gym_amd.terrain import random_terrain_pool
            heights, mids = random_terrain_pool(POOL)
        return [random_terrain_field(heights, mids, t) for t in range(POOL)]
    fields = custom_fields() if heights is None else heights
    mids = custom_mids(fields) if mids is None else mids
    (inv_x, off_x), (inv_y, off_y) = grid_constants(CUSTOM_NX, CUSTOM_CELL[0], CUSTOM_ORIGIN[0]), grid_constants(CUSTOM_NY, CUSTOM_CELL[1], CUSTOM_ORIGIN[1])
    return [(np.asarray(fields[t], np.float64).reshape(-1), float(mids[t]), CUSTOM_NX, CUSTOM_NY, inv_x, inv_y, off_x, off_y) for t in range(2)]


def field_of(fields, g, episode, env_index_base=0):
    """the field env g stands on in `episode` (terrain_index of csrc/rex_kernels.h: (global index + 977 episode) mod pool size)"""
    return None if fields is None else fields[(g + env_index_base + 977 * int(episode)) % len(fields)]


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def synthetic_state(rng, arm, kind, field, off_xy):
    """One env's words 0 .. 13 + 2 NM, float32: base (x, y) within +-3 m, a tilt of up to 1.2 rad about a horizontal axis after a random
    yaw, joint angles uniform inside their limits, random twists and joint rates, and the base height that puts the LOWEST toe point at a
    distance drawn from -0.01 .. 0.06 m (both sides of the 0.02 m breaking threshold).  kind: "random", or one of CORNERS --
      degenerate  quaternion (.5, .5, .5, .5), exact in float32: a roll of exactly 90 degrees (then a yaw of 90): with the shoulders at 0 the
                  toe axes are exactly +z, parallel to the plane's normal (and to every level facet's)
      off         the base beside the heightfield's footprint;  upside  rolled by 180 degrees
      origin      at the origin, level, joints and every velocity 0"""
    nm = num_motors(arm)
    lo, hi = (np.concatenate([JLOWER, A_LOWER]), np.concatenate([JUPPER, A_UPPER])) if arm else (JLOWER, JUPPER)
    s = np.zeros((13 + 2 * nm, 1), np.float64)
    tilt, heading, yaw = rng.uniform(0, 1.2), rng.uniform(0, 2 * math.pi), rng.uniform(-math.pi, math.pi)
    s[0:2, 0] = rng.uniform(-3, 3, 2)
    s[3:7, 0] = _quat_mul([0, 0, math.sin(yaw / 2), math.cos(yaw / 2)],
                          [math.sin(tilt / 2) * math.cos(heading), math.sin(tilt / 2) * math.sin(heading), 0, math.cos(tilt / 2)])
    s[7:10, 0], s[10:13, 0] = rng.uniform(-1, 1, 3), rng.uniform(-3, 3, 3)
    s[13:13 + nm, 0], s[13 + nm:, 0] = rng.uniform(lo, hi), rng.uniform(-5, 5, nm)
    target = rng.uniform(-0.01, 0.06)
    if kind == "degenerate":
        s[3:7, 0], s[13:13 + nm, 0] = 0.5, 0.0
    elif kind == "off":
        s[0:2, 0] = off_xy
    elif kind == "upside":
        s[3:7, 0] = [1, 0, 0, 0]
    elif kind == "origin":
        s[0:2, 0], s[3:7, 0], s[7:, 0] = 0.0, [0, 0, 0, 1], 0.0
    s = s.astype(np.float32)
    r = reference(s, 0, arm, field)
    s[2, 0] = target - float((r["toe_dist"] / r["toe_normal"][:, 2]).min())     # dist / n_z = z - ground height
    return s[:, 0]


def scene_states(arm, n, ground, keep=0, seed=0):
    """-> (S float32 [episode word + 1, n], kinds [n]): the synthetic columns keep .. n - 1 of a scene (columns below `keep` are zero and
    kind "real"); with 8 or more of them the last four are CORNERS.  S's last row holds the episode, alternating 1 and 2 with a period of
    three envs, as the int32's bits."""
    fields = scene_fields(ground)
    rng = np.random.RandomState(1000 * seed + 17 * n + (7 if arm else 0) + {"plane": 0, "random": 1, "custom": 2}[ground])
    ew = episode_word(arm)
    S = np.zeros((ew + 1, n), np.float32)
    kinds = ["real"] * keep + ["random"] * (n - keep)
    if n - keep >= 8:
        kinds[-4:] = CORNERS
    episode = np.array([1 + (g % 3 == 1) for g in range(n)], dtype=np.int32)
    S[ew] = episode.view(np.float32)
    for g in range(keep, n):
        S[:13 + 2 * num_motors(arm), g] = synthetic_state(rng, arm, kinds[g], field_of(fields, g, episode[g]), OFF_XY[ground])
    return S, kinds


# ---------------------------------------------------------------- comparing a set of outputs with the float64 reference
FLOAT_FIELDS = ("link_pos", "link_quat", "link_linvel", "link_angvel", "toe_pos", "toe_vel", "toe_dist", "toe_normal", "base_body")


def _rel(a, r):
    """|a - r| of 3-vectors relative to max(1, |r|)"""
    a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
    return np.linalg.norm(a - r, axis=-1) / np.maximum(1.0, np.linalg.norm(r, axis=-1))


def errors(a, r):
    """Deviation of the outputs `a` of one env (a dict of arrays shaped as reference()'s, any float dtype) from the float64 reference r,
    per link or toe point: positions, distances and normals absolute (normals: the largest component), rotations as 1 - |q_a . q_r|,
    velocities relative to max(1, |v|); base_body: its three vectors, the velocities relative, the gravity direction absolute."""
    d = lambda k: np.asarray(a[k], np.float64) - np.asarray(r[k], np.float64)
    bb_a, bb_r = np.asarray(a["base_body"], np.float64).reshape(3, 3), np.asarray(r["base_body"], np.float64).reshape(3, 3)
    return dict(link_pos=np.abs(d("link_pos")).max(-1), link_quat=1.0 - np.abs((np.asarray(a["link_quat"], np.float64) * r["link_quat"]).sum(-1)),
                link_linvel=_rel(a["link_linvel"], r["link_linvel"]), link_angvel=_rel(a["link_angvel"], r["link_angvel"]),
                toe_pos=np.abs(d("toe_pos")).max(-1), toe_vel=_rel(a["toe_vel"], r["toe_vel"]), toe_dist=np.abs(d("toe_dist")),
                toe_normal=np.abs(d("toe_normal")).max(-1),
                base_body=np.array([_rel(bb_a[0], bb_r[0]), _rel(bb_a[1], bb_r[1]), np.abs(bb_a[2] - bb_r[2]).max()]))


def quat32(R):
    """unit quaternion of a float32 rotation matrix in float32 arithmetic: the largest pivot's branch, then normalised"""
    f = np.float32
    R = np.asarray(R, f)
    one = f(1)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        q = [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], one + tr]
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        q = [one + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]]
    elif R[1, 1] >= R[2, 2]:
        q = [R[0, 1] + R[1, 0], one + R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]]
    else:
        q = [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], one + R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]]
    q = np.array(q, dtype=f)
    return (q / np.sqrt(q @ q)).astype(f)


def reference32(state, env, arm, field=None):
    """reference() in float32 arithmetic, the quaternions too: what round-off alone does to every output"""
    r = reference(state, env, arm, field, np.float32)
    r["link_quat"] = np.array([quat32(R) for R in r["link_rot"]])
    return r


def stable_points(state, env, arm, field, r, shift):
    """[8] bool: the toe points whose two facet ids stay what they are in r when both query points move by `shift` in +-x and +-y
    (all of them on the plane)"""
    ok = np.ones(8, bool)
    if field is None:
        return ok
    for sx, sy in ((shift, 0.0), (-shift, 0.0), (0.0, shift), (0.0, -shift)):
        p = reference(state, env, arm, field, shift=(sx, sy))
        ok &= (p["fid0"] == r["fid0"]) & (p["fid1"] == r["fid1"])
    return ok


# ---------------------------------------------------------------- the scenes of the GPU test, and what the reference alone says about them
SCENES = [("base", 1, "plane"), ("base", 5, "plane"), ("base", 67, "plane"), ("base", 130, "plane"), ("arm", 5, "plane"), ("arm", 67, "plane"),
          ("base", 67, "random"), ("arm", 5, "random"), ("base", 67, "custom"), ("arm", 67, "custom")]


def scene_keep(n):
    """how many leading columns of a scene keep the env's own state (after random steps)"""
    return min(4, n // 2)


def measure_floors(scenes=SCENES, position_shift=None):
    """Over the synthetic columns of `scenes`: the largest deviation of the float32 reference from the float64 one per field (errors()),
    and the share of toe points left out of the ground-dependent comparisons.  Two passes when position_shift is None: the toe_pos floor over
    the points whose facets the two precisions agree on, then everything with the stability probe at 4 x that floor -- the position bound
    of the GPU test.  -> (floors, position_shift, points, kept)"""
    rows = []
    for mark, n, ground in scenes:
        arm = mark == "arm"
        S, kinds = scene_states(arm, n, ground, scene_keep(n))
        fields = scene_fields(ground)
        ep = S[episode_word(arm)].view(np.int32)
        for g in range(scene_keep(n), n):
            f = field_of(fields, g, ep[g])
            r64, r32 = reference(S, g, arm, f), reference32(S, g, arm, f)
            rows.append((S, g, arm, f, r64, r32, errors(r32, r64), (r32["fid0"] == r64["fid0"]) & (r32["fid1"] == r64["fid1"])))
    if position_shift is None:
        position_shift = 4.0 * max(float(e["toe_pos"][same].max()) for *_, e, same in rows if same.any())
    floors = {k: 0.0 for k in FLOAT_FIELDS}
    points = kept = 0
    for S, g, arm, f, r64, r32, e, same in rows:
        ok = stable_points(S, g, arm, f, r64, position_shift)
        points, kept = points + 8, kept + int(ok.sum())
        for k in FLOAT_FIELDS:
            v = e[k][ok & same] if k.startswith("toe_") else e[k]
            if v.size:
                floors[k] = max(floors[k], float(v.max()))
    return floors, position_shift, points, kept
