"""The numpy reference of rex_contact_space and rex_inverse_dynamics, independent of the kernel (tests/test_contact_space_host.py,
tests/test_gpu_contact_space.py).  M, h and the toe Jacobians J [24, 18] (row 3 p + c) are dynamics_ref.reference's, float64:

    delassus      = J solve(M, J^T)
    toe_acc_free  = J solve(M, S^T tau + w - h) + drift
    force         = M vdot - (S^T tau + sum_p J_p^T f_p + w - h)          (the bracket: dynamics_solve_ref.load_rhs)
    drift_p       the recursion of include/rexsim.h on kinematics_ref's link data: with w_0 the base's angular velocity,
                  w_i = w_i-1 + qd_i a_i and joint points o_i carried by their parents,  alpha_0 = 0, acc(o_0) = 0,
                  alpha_i = alpha_i-1 + w_i-1 x (qd_i a_i),  acc(o_i) = acc(o_i-1) + alpha_i-1 x (o_i - o_i-1) + w_i-1 x (w_i-1 x (o_i - o_i-1)),
                  drift_p = acc(o_3) + alpha_3 x (P - o_3) + w_3 x (w_3 x (P - o_3))

Two float32 routes for the round-off floors, as dynamics_ref and dynamics_solve_ref have them:
    "dense"   the Jacobian-route M of dynamics_ref.reference() in float32 with a dense Cholesky (dynamics_solve_ref.dense_cholesky)
    "block"   the composite-route M of dynamics_ref.reference_composite() in float32 with the block elimination
each with the float32 J, h of its own route, the drift recursion in float32 and float32 products.  The kernel's operation order is neither's.

Error measures, chosen so that no block is divided by another's magnitude:
    delassus      |dL_rs| / (kappa sqrt(L_rr L_ss))  with L the float64 reference and kappa = cond_2(D^-1/2 M D^-1/2) of the env
                  (dynamics_solve_ref.conditioning): an entry comes from a solve with M, which loses about kappa times the unit
                  round-off, and a nearly straight leg does not set the bound of every other state                            [24, 24]
    toe_drift,    per point the largest component of the difference / max(10 m/s^2, the env's largest reference component of that
    toe_acc_free  field)                                                                                                      [8]
    force         dynamics_ref.errors' scaling of bias: per block -- base force, base moment, each joint -- |d| / max(scale, |ref|) with
                  the scales 10 mass, 10 mass 0.1 m and 10 (carried mass) 0.1 m                                               [14]"""
import numpy as np

import dynamics_ref as dr
import dynamics_solve_ref as sr
import kinematics_ref as kr
import test_gpu_render as col

FIELDS = ("delassus", "toe_drift", "toe_acc_free")
KINDS = FIELDS + ("force",)
ACC_SCALE = 10.0                                           # m/s^2
# the inputs of inverse dynamics given alone, and all together
COMBOS = (("vdot",), ("tau",), ("toe",), ("wrench",), ("vdot", "tau", "toe", "wrench"))
# the inputs of toe_acc_free: none, and both
FREE_COMBOS = ((), ("tau", "wrench"))


def accelerations(n, seed=53):
    """the wanted generalized accelerations of a scene, float32 [n, 18]: base m/s^2 and rad/s^2, joints rad/s^2"""
    rng = np.random.RandomState(seed + n)
    return (rng.standard_normal((n, 18)) * ([5.0] * 3 + [10.0] * 3 + [50.0] * 12)).astype(np.float32)


def drift(kin, f=np.float64):
    """[8, 3]: Jdot v of the toe points of kinematics_ref.reference()'s result, in dtype f"""
    o, w, R = kin["link_pos"].astype(f), kin["link_angvel"].astype(f), kin["link_rot"].astype(f)
    out = np.zeros((8, 3), f)
    for leg in range(4):
        acc, alpha = np.zeros(3, f), np.zeros(3, f)
        for b in range(3 * leg + 1, 3 * leg + 4):
            p = int(col.PARENT[b])
            axis = R[b][:, col.JAXIS[b - 1]]
            rate = (w[b] - w[p]) @ axis                    # the joint's rate, as the reference's angular velocities hold it
            d = (o[b] - o[p]).astype(f)
            acc = (acc + np.cross(alpha, d) + np.cross(w[p], np.cross(w[p], d))).astype(f)
            alpha = (alpha + np.cross(w[p], rate * axis)).astype(f)
        foot = 3 * leg + 3
        for e in range(2):
            rp = (kin["toe_pos"][2 * leg + e].astype(f) - o[foot]).astype(f)
            out[2 * leg + e] = acc + np.cross(alpha, rp) + np.cross(w[foot], np.cross(w[foot], rp))
    return out


def contact_space(M, h, J, kin, tau=None, wrench=None, f=np.float64, solve=None):
    """delassus [24, 24], toe_drift [8, 3], toe_acc_free [8, 3] from M, h, J [8, 3, 18] and the link data `kin`, in dtype f;
    solve(M, B [K, 18], f) -> X [K, 18] (default: np.linalg.solve)"""
    solve = solve or (lambda M, B, f: sr.solve_ref(M, B))
    J24 = np.asarray(J, f).reshape(24, sr.NDOF)
    X = np.asarray(solve(M, J24, f), f)                                    # rows M^-1 J_r^T
    b = sr.load_rhs(J, h, tau=tau, wrench=wrench, f=f)
    x = np.asarray(solve(M, b[None], f), f)[0]
    dft = drift(kin, f)
    return dict(delassus=(J24 @ X.T).astype(f), toe_drift=dft, toe_acc_free=((J24 @ x).astype(f).reshape(8, 3) + dft).astype(f))


def reference(state, env, field=None, scales=(1.0, 1.0), tau=None, wrench=None, dyn=None):
    """float64: contact_space() on dynamics_ref.reference (given as `dyn`, or evaluated here); the result also holds `dyn`"""
    r = dyn if dyn is not None else dr.reference(state, env, field, scales)
    out = contact_space(r["mass_matrix"], r["bias"], r["toe_jacobian"], r["kin"], tau, wrench)
    out["dyn"] = r
    return out


def inverse(M, h, J, vdot=None, tau=None, toe=None, wrench=None, f=np.float64):
    """force [18] = M vdot + h - S^T tau - sum_p J_p^T f_p - w in dtype f"""
    y = np.zeros(sr.NDOF, f) if vdot is None else (np.asarray(M, f) @ np.asarray(vdot, f)).astype(f)
    return (y - sr.load_rhs(J, h, tau=tau, toe=toe, wrench=wrench, f=f)).astype(f)


def routes32(state, env, field, scales):
    """the two float32 routes of one env: [(name, M, h, J, kin, solve)]"""
    f = np.float32
    k32 = kr.reference(state, env, False, field, f)
    r32 = dr.reference(state, env, field, scales, f, kin=k32)
    c32 = dr.reference_composite(state, env, field, scales, f, kin=k32)
    return k32, [("dense", r32["mass_matrix"], r32["bias"], r32["toe_jacobian"], k32, sr.dense_cholesky),
                 ("block", c32["mass_matrix"], c32["bias"], r32["toe_jacobian"], k32, sr.block_elimination)]


# ---------------------------------------------------------------- the error measures (module docstring)
def point_mask(ok):
    """[24, 24] bool: the entries of delassus whose two points are both kept"""
    rows = np.repeat(np.asarray(ok, bool), 3)
    return np.outer(rows, rows)


def errors(a, ref):
    """a: any subset of FIELDS of one env; ref: reference()'s result -> per field the measures of the module docstring"""
    out = {}
    if "delassus" in a:
        L = np.asarray(ref["delassus"], np.float64)
        s = np.sqrt(np.diag(L))
        _, kappa = sr.conditioning(ref["dyn"]["mass_matrix"])
        out["delassus"] = np.abs(np.asarray(a["delassus"], np.float64) - L) / (kappa * np.outer(s, s))
    for k in ("toe_drift", "toe_acc_free"):
        if k in a:
            want = np.asarray(ref[k], np.float64).reshape(8, 3)
            out[k] = np.abs(np.asarray(a[k], np.float64).reshape(8, 3) - want).max(-1) / max(ACC_SCALE, float(np.abs(want).max()))
    return out


def force_errors(force, want, dyn):
    """[14]: dynamics_ref.errors' measure of bias applied to a force"""
    return dr.errors({"bias": force}, {**dyn, "bias": np.asarray(want, np.float64)})["bias"]


# ---------------------------------------------------------------- what the reference alone says about the GPU test's scenes
def scene_inputs(n):
    """the loads and accelerations of a scene: dynamics_solve_ref.loads(n) plus vdot"""
    return {**sr.loads(n), "vdot": accelerations(n)}


def measure_floors(position_shift):
    """Over the synthetic columns of dynamics_ref.SCENES with scene_scales() and scene_inputs(): per kind the larger error of the two float32
    routes against the float64 reference -- delassus and the accelerations over the points dynamics_ref.measure_floors keeps, toe_acc_free
    over FREE_COMBOS, force over COMBOS with toe forces only at the kept points.  -> (floors, points, points kept)"""
    f = np.float32
    floors = {k: 0.0 for k in KINDS}
    points = kept = 0
    for _, n, ground in dr.SCENES:
        S, _ = kr.scene_states(False, n, ground, kr.scene_keep(n))
        fields = kr.scene_fields(ground)
        ep = S[kr.episode_word(False)].view(np.int32)
        bs, ls = dr.scene_scales(n)
        inp = scene_inputs(n)
        for g in range(kr.scene_keep(n), n):
            fld, sc = kr.field_of(fields, g, ep[g]), (bs[g], ls[g])
            r64 = dr.reference(S, g, fld, sc)
            k32, routes = routes32(S, g, fld, sc)
            ok = dr.stable_points(S, g, fld, r64["kin"], position_shift) & (k32["fid0"] == r64["kin"]["fid0"]) & (k32["fid1"] == r64["kin"]["fid1"])
            points, kept = points + 8, kept + int(ok.sum())
            mask = point_mask(ok)
            for combo in FREE_COMBOS:
                p = {k: (inp[k][g] if k in combo else None) for k in ("tau", "wrench")}
                want = reference(S, g, fld, sc, dyn=r64, **p)
                for _, M, h, J, kin, solve in routes:
                    e = errors(contact_space(M, h, J, kin, f=f, solve=solve, **p), want)
                    for k, v in e.items():
                        v = v[mask] if k == "delassus" else v[ok]
                        if v.size:
                            floors[k] = max(floors[k], float(v.max()))
            for combo in COMBOS:
                p = {k: (inp[k][g].copy() if k in combo else None) for k in ("vdot", "tau", "toe", "wrench")}
                if p["toe"] is not None:
                    p["toe"][~ok] = 0.0
                want = inverse(r64["mass_matrix"], r64["bias"], r64["toe_jacobian"], **p)
                for _, M, h, J, _, _ in routes:
                    floors["force"] = max(floors["force"], float(force_errors(inverse(M, h, J, f=f, **p), want, r64).max()))
    return floors, points, kept
