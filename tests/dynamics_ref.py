"""The numpy reference of rex_dynamics, independent of the kernel (tests/test_dynamics_host.py, tests/test_gpu_dynamics.py), float64
unless asked for float32 (for the round-off floors only).  Poses, link velocities and toe points are kinematics_ref.reference's; the
model tables REX_MASS, REX_COM, REX_INERTIA are parsed from csrc/rex_model_gen.h with test_gpu_render's helper.

Generalized velocity v[18] = (world linear velocity of the base origin, world angular velocity of the base, 12 joint rates), and
    M(q) vdot + h(q, v) = S^T tau + sum_p J_p^T f_p,     g = 10 m/s^2 along -z.
Masses are REX_MASS times the env's (base_mass_scale, leg_mass_scale); the rotational inertias about the links' centres of mass are the
table's, unscaled (what the step does).

Two routes:
  reference()            per link b the centre-of-mass Jacobians Jv_b, Jw_b [3, 18]:
                           M = sum_b m_b Jv_b^T Jv_b + Jw_b^T (R_b I_b R_b^T) Jw_b
                           h = sum_b Jv_b^T m_b (a_b + g z) + Jw_b^T (I_b alpha_b + w_b x I_b w_b)
                         with the textbook bias accelerations (zero generalized acceleration) down the chains; centre of mass and
                         momentum as sums over links
  reference_composite()  composite inertias in world axes about the base origin and recursive Newton-Euler with subtree wrenches
                         (the same quantities by the other classic algorithm; M, bias and gravity only)
The float32 floor of a field is the larger deviation of the two routes in float32 from reference() in float64: the kernel's operation
order matches neither exactly."""
import numpy as np

import kinematics_ref as kr
import test_gpu_render as col

G = 10.0
NDOF = 18
MASS = col._arr("rex_model_gen.h", "REX_MASS")
COM = col._arr("rex_model_gen.h", "REX_COM").reshape(-1, 3)
INERTIA = col._arr("rex_model_gen.h", "REX_INERTIA").reshape(-1, 6)
assert MASS.shape == (13,) and COM.shape == (13, 3) and INERTIA.shape == (13, 6)
FIELDS = ("mass_matrix", "bias", "gravity", "toe_jacobian", "com", "momentum", "mass")
BASE_SCALE_RANGE, LEG_SCALE_RANGE = (0.8, 1.2), (0.7, 1.3)


def scene_scales(n, seed=23):
    """per-env (base_mass_scale [n], leg_mass_scale [n]) float32 of the test scenes: fixed seed, base 0.8 .. 1.2, legs 0.7 .. 1.3"""
    rng = np.random.RandomState(seed + n)
    return rng.uniform(*BASE_SCALE_RANGE, n).astype(np.float32), rng.uniform(*LEG_SCALE_RANGE, n).astype(np.float32)


def _skew(a, f):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=f)


def _inertia_body(b, f):
    xx, yy, zz, xy, xz, yz = INERTIA[b]
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]], dtype=f)


def links(r, scales, f):
    """per body of kinematics_ref.reference()'s result r: dict(m, c, I (world axes, about c), w, vc, chain [(joint, axis, joint point)])"""
    out = []
    for b in range(13):
        R, o = r["link_rot"][b].astype(f), r["link_pos"][b].astype(f)
        c = (o + R @ COM[b].astype(f)).astype(f)
        w = r["link_angvel"][b].astype(f)
        chain, k = [], b
        while k > 0:
            chain.append((k - 1, r["link_rot"][k][:, col.JAXIS[k - 1]].astype(f), r["link_pos"][k].astype(f)))
            k = int(col.PARENT[k])
        out.append(dict(m=f(MASS[b]) * f(scales[0] if b == 0 else scales[1]), c=c, I=(R @ _inertia_body(b, f) @ R.T).astype(f), w=w,
                        vc=(r["link_linvel"][b].astype(f) + np.cross(w, c - o)).astype(f), chain=chain[::-1], o=o))
    return out


def link_jacobians(lk, o0, f):
    """-> (Jv [3, 18], Jw [3, 18]) of the link's centre of mass"""
    Jv, Jw = np.zeros((3, NDOF), dtype=f), np.zeros((3, NDOF), dtype=f)
    Jv[:, 0:3] = np.eye(3, dtype=f)
    Jv[:, 3:6] = -_skew(lk["c"] - o0, f)
    Jw[:, 3:6] = np.eye(3, dtype=f)
    for j, axis, point in lk["chain"]:
        Jv[:, 6 + j] = np.cross(axis, lk["c"] - point)
        Jw[:, 6 + j] = axis
    return Jv, Jw


def bias_accelerations(r, lks, f, with_velocity=True):
    """The textbook recursion at zero generalized acceleration: per body (a_c, alpha), the acceleration of its centre of mass and its
    angular acceleration.  The base origin moves at constant world velocity and the base turns at constant world angular velocity."""
    zero = np.zeros(3, dtype=f)
    if not with_velocity:
        return [(zero, zero) for _ in range(13)]
    ao, al, acc = [zero], [zero], []
    for b in range(13):
        lk = lks[b]
        if b > 0:
            p = int(col.PARENT[b])
            wp, d = lks[p]["w"], (lk["o"] - lks[p]["o"]).astype(f)
            j, axis, _ = lk["chain"][-1]
            rate = (lk["w"] - wp) @ axis                         # the joint's rate, as the reference's angular velocities hold it
            ao.append((ao[p] + np.cross(al[p], d) + np.cross(wp, np.cross(wp, d))).astype(f))
            al.append((al[p] + rate * np.cross(wp, axis)).astype(f))
        rc = (lk["c"] - lk["o"]).astype(f)
        acc.append(((ao[b] + np.cross(al[b], rc) + np.cross(lk["w"], np.cross(lk["w"], rc))).astype(f), al[b]))
    return acc


def project(lks, jac, acc, f, spin=True):
    """sum_b Jv_b^T m_b (a_b + g z) + Jw_b^T (I_b alpha_b + w_b x I_b w_b)  [18]; spin=False leaves the gyroscopic term out (v = 0)"""
    h = np.zeros(NDOF, dtype=f)
    gz = np.array([0, 0, G], dtype=f)
    for lk, (Jv, Jw), (ac, al) in zip(lks, jac, acc):
        N = lk["I"] @ al + (np.cross(lk["w"], lk["I"] @ lk["w"]) if spin else 0)
        h = (h + Jv.T @ (lk["m"] * (ac + gz)) + Jw.T @ N.astype(f)).astype(f)
    return h


def reference(state, env, field=None, scales=(1.0, 1.0), dtype=np.float64, kin=None):
    """Every output of rex_dynamics for env `env` of `state` (numpy [words, n] float32), mark base, in `dtype` arithmetic: mass_matrix
    [18, 18], bias, gravity [18], toe_jacobian [8, 3, 18], com [6], momentum [6], mass; and `kin`, kinematics_ref.reference()'s result."""
    f = dtype
    r = kin if kin is not None else kr.reference(state, env, False, field, f)
    lks = links(r, scales, f)
    o0 = r["link_pos"][0].astype(f)
    jac = [link_jacobians(lk, o0, f) for lk in lks]
    M = np.zeros((NDOF, NDOF), dtype=f)
    for lk, (Jv, Jw) in zip(lks, jac):
        M = (M + lk["m"] * (Jv.T @ Jv) + Jw.T @ lk["I"] @ Jw).astype(f)
    bias = project(lks, jac, bias_accelerations(r, lks, f), f)
    gravity = project(lks, jac, bias_accelerations(r, lks, f, False), f, spin=False)
    mass = f(sum(lk["m"] for lk in lks))
    C = (sum(lk["m"] * lk["c"] for lk in lks) / mass).astype(f)
    p = sum(lk["m"] * lk["vc"] for lk in lks).astype(f)
    L = sum(lk["I"] @ lk["w"] + lk["m"] * np.cross(lk["c"] - C, lk["vc"]) for lk in lks).astype(f)
    J = np.zeros((8, 3, NDOF), dtype=f)
    for pt in range(8):
        P, foot = r["toe_pos"][pt].astype(f), lks[3 + 3 * (pt // 2)]
        J[pt, :, 0:3] = np.eye(3, dtype=f)
        J[pt, :, 3:6] = -_skew(P - o0, f)
        for j, axis, point in foot["chain"]:
            J[pt, :, 6 + j] = np.cross(axis, P - point)
    carried = np.array([sum(float(lks[k]["m"]) for k in range(b, 4 + 3 * ((b - 1) // 3))) for b in range(1, 13)])     # per joint: its subtree's mass
    return dict(mass_matrix=M, bias=bias, gravity=gravity, toe_jacobian=J, com=np.concatenate([C, p / mass]).astype(f),
                momentum=np.concatenate([p, L]).astype(f), mass=mass, kin=r, carried=carried)


def reference_composite(state, env, field=None, scales=(1.0, 1.0), dtype=np.float64, kin=None):
    """mass_matrix, bias and gravity by the other route: composite rigid bodies and recursive Newton-Euler, every spatial quantity in
    world axes about the base origin o_0.  Subtree i of a leg has mass mc, first moment hc and rotational inertia Ic about o_0; a unit rate of
    joint i (axis a, point p relative to o_0) gives it the momentum f = mc u + a x hc, n = Ic a + hc x u with u = p x a."""
    f = dtype
    r = kin if kin is not None else kr.reference(state, env, False, field, f)
    lks = links(r, scales, f)
    o0 = r["link_pos"][0].astype(f)
    eye = np.eye(3, dtype=f)
    gz = np.array([0, 0, G], dtype=f)
    acc = bias_accelerations(r, lks, f)
    M, bias, gravity = np.zeros((NDOF, NDOF), dtype=f), np.zeros(NDOF, dtype=f), np.zeros(NDOF, dtype=f)
    # subtree sums from the tips inwards (the bodies of a leg are numbered parent first)
    mc, hc, Ic, Fs, Ns = [None] * 13, [None] * 13, [None] * 13, [None] * 13, [None] * 13
    for b in range(12, -1, -1):
        lk = lks[b]
        rr = (lk["c"] - o0).astype(f)
        F = (lk["m"] * (acc[b][0] + gz)).astype(f)
        N = (lk["I"] @ acc[b][1] + np.cross(lk["w"], lk["I"] @ lk["w"]) + np.cross(rr, F)).astype(f)
        mc[b], hc[b], Ic[b], Fs[b], Ns[b] = lk["m"], (lk["m"] * rr).astype(f), (lk["I"] + lk["m"] * ((rr @ rr) * eye - np.outer(rr, rr))).astype(f), F, N
        for k in range(b + 1, 13):
            if int(col.PARENT[k]) == b:
                mc[b], hc[b], Ic[b], Fs[b], Ns[b] = mc[b] + mc[k], hc[b] + hc[k], Ic[b] + Ic[k], Fs[b] + Fs[k], Ns[b] + Ns[k]
    M[0:3, 0:3], M[0:3, 3:6], M[3:6, 0:3], M[3:6, 3:6] = mc[0] * eye, -_skew(hc[0], f), _skew(hc[0], f), Ic[0]
    bias[0:3], bias[3:6] = Fs[0], Ns[0]
    gravity[0:3], gravity[3:6] = mc[0] * gz, np.cross(hc[0], gz)
    for b in range(1, 13):
        i, a, p = b - 1, lks[b]["chain"][-1][1], (lks[b]["o"] - o0).astype(f)
        u = np.cross(p, a).astype(f)
        fi, ni = (mc[b] * u + np.cross(a, hc[b])).astype(f), (Ic[b] @ a + np.cross(hc[b], u)).astype(f)
        M[0:3, 6 + i], M[3:6, 6 + i], M[6 + i, 0:3], M[6 + i, 3:6] = fi, ni, fi, ni
        for j, aj, pj in lks[b]["chain"]:                       # the joints above, and joint i itself
            M[6 + i, 6 + j] = M[6 + j, 6 + i] = np.cross((pj - o0).astype(f), aj) @ fi + aj @ ni
        bias[6 + i] = a @ (Ns[b] - np.cross(p, Fs[b]))
        gravity[6 + i] = a @ np.cross(hc[b] - mc[b] * p, gz)
    return dict(mass_matrix=M, bias=bias, gravity=gravity)


# ---------------------------------------------------------------- comparing a set of outputs with the float64 reference
LEVER = 0.1          # m: torque scales are force scales times this lever (the legs are 0.12 m long, the hips 0.1 m from the origin)


def errors(a, r):
    """Deviation of the outputs `a` of one env (a dict of arrays shaped as reference()'s; any subset of FIELDS) from the float64 reference
    r, chosen so that no block's error is divided by another block's magnitude:
      mass_matrix   |dM_ij| / sqrt(M_ii M_jj) with the reference's diagonal                                   [18, 18]
      toe_jacobian  absolute, the largest component of each point                                            [8]
      bias, gravity per block -- base force (3-vector), base torque (3-vector), each joint -- |d| / max(scale, |ref|) with the fixed scales
                    10 * mass [N] for the force, 10 * mass * LEVER [N m] for the base torque, and for a joint 10 * LEVER times the mass of
                    the links it carries                                                                     [14]
      com           position absolute (largest component), velocity |dv| / max(1, |v|)                        [2]
      momentum      linear |d| / max(mass * 1 m/s, |ref|); angular |d| / max(sqrt(trace M[3:6, 3:6]), |ref|)  [2]
      mass          relative"""
    out = {}
    d = lambda k: np.asarray(a[k], np.float64) - np.asarray(r[k], np.float64)
    mass = float(r["mass"])
    M = np.asarray(r["mass_matrix"], np.float64)
    if "mass_matrix" in a:
        s = np.sqrt(np.diag(M))
        out["mass_matrix"] = np.abs(d("mass_matrix")) / np.outer(s, s)
    if "toe_jacobian" in a:
        out["toe_jacobian"] = np.abs(d("toe_jacobian")).reshape(8, -1).max(-1)
    scales = np.concatenate([[G * mass, G * mass * LEVER], G * LEVER * np.asarray(r["carried"], np.float64)])
    for k in ("bias", "gravity"):
        if k in a:
            dd, ref = d(k), np.asarray(r[k], np.float64)
            blocks = [np.linalg.norm(dd[0:3]), np.linalg.norm(dd[3:6])] + list(np.abs(dd[6:]))
            mags = [np.linalg.norm(ref[0:3]), np.linalg.norm(ref[3:6])] + list(np.abs(ref[6:]))
            out[k] = np.array(blocks) / np.maximum(scales, np.array(mags))
    if "com" in a:
        out["com"] = np.array([np.abs(d("com")[0:3]).max(), kr._rel(np.asarray(a["com"])[3:6], np.asarray(r["com"])[3:6])])
    if "momentum" in a:
        dd, ref = d("momentum"), np.asarray(r["momentum"], np.float64)
        out["momentum"] = np.array([np.linalg.norm(dd[0:3]) / max(mass * 1.0, np.linalg.norm(ref[0:3])),
                                    np.linalg.norm(dd[3:6]) / max(np.sqrt(np.trace(M[3:6, 3:6])), np.linalg.norm(ref[3:6]))])
    if "mass" in a:
        out["mass"] = np.array([abs(float(a["mass"]) - mass) / mass])
    return out


def stable_points(state, env, field, kin, shift):
    return kr.stable_points(state, env, False, field, kin, shift)


# ---------------------------------------------------------------- the scenes of the GPU test, and what the reference alone says about them
SCENES = [s for s in kr.SCENES if s[0] == "base"]


def measure_floors(position_shift):
    """Over the synthetic columns of SCENES with scene_scales(): per field the largest deviation (errors()) of either route evaluated in
    float32 from reference() in float64; toe_jacobian over the points that kr.stable_points keeps at `position_shift` (the toe_pos bound of
    the kinematics test) and whose facets the two precisions agree on.  -> (floors, points, kept)"""
    floors = {k: 0.0 for k in FIELDS}
    points = kept = 0
    for _, n, ground in SCENES:
        S, _ = kr.scene_states(False, n, ground, kr.scene_keep(n))
        fields = kr.scene_fields(ground)
        ep = S[kr.episode_word(False)].view(np.int32)
        bs, ls = scene_scales(n)
        for g in range(kr.scene_keep(n), n):
            fld, sc = kr.field_of(fields, g, ep[g]), (bs[g], ls[g])
            r64 = reference(S, g, fld, sc)
            k32 = kr.reference(S, g, False, fld, np.float32)
            r32, c32 = reference(S, g, fld, sc, np.float32, kin=k32), reference_composite(S, g, fld, sc, np.float32, kin=k32)
            ok = stable_points(S, g, fld, r64["kin"], position_shift) & (k32["fid0"] == r64["kin"]["fid0"]) & (k32["fid1"] == r64["kin"]["fid1"])
            points, kept = points + 8, kept + int(ok.sum())
            for e in (errors(r32, r64), errors(c32, r64)):
                for k, v in e.items():
                    v = v[ok] if k == "toe_jacobian" else v
                    if v.size:
                        floors[k] = max(floors[k], float(np.max(v)))
    return floors, points, kept
