"""The numpy reference of rex_contact_solve, independent of the kernel (tests/test_contact_solve_host.py, tests/test_gpu_contact_solve.py):
one substep's contact problem of one env, float64 unless asked for float32 (for the round-off floors only).

M, h (bias) and the toe Jacobians J_p are dynamics_ref.reference's, the toe points, normals, distances and `in reach` are
kinematics_ref.reference's; the damping force and the solver are restated here:

    v*      = v + dt M^-1 (S^T tau - h - d),   d = sum_b Jv_b^T m_b (c + c |vc_b|) vc_b + Jw_b^T (c + c |w_b|) I_b w_b,  c = 0.04
    rows    (a) joint j beyond its bound (gap = min(q - lower, upper - q) < 0):  J = sgn e_j, 0 <= lambda,
                rhs = (-gap ERP / dt - sgn v*_j) / diag
            (b) toe point p in reach (dist < 0.02):  J = n^T J_p, 0 <= lambda,  rhs = (poserr + velerr) / diag,
                velerr = -J v* - (dist > 0 ? dist / dt : 0),  poserr = dist > 0 ? 0 : -dist ERP / dt
            (c) per such point the rows t1^T J_p, t2^T J_p, (t1, t2) = plane_space(n):  rhs = -(J v*) / diag,  |lambda| <= mu lambda_n
            diag = J M^-1 J^T, every response M^-1 J^T by a dense solve
    PGS     lambda = 0; per sweep the rows in that order:  dl = rhs - (J dv) / diag, clamped to the bounds,  dv += M^-1 J^T dl;
            stop after `iterations` sweeps or after the first sweep with max (dl diag)^2 <= residual_threshold
    v_next  = clamp(v* + dv, +-100)

This is the statement of oracle/rex_oracle.c physics_substep (body_contacts off) in the coordinates of env.dynamics(); the oracle works in
body coordinates with an articulated-body recursion, so the two are independent formulations (test_contact_solve_host.py compares them).

The module also holds the scenes of the GPU test: sizes and grounds of dynamics_ref.SCENES, the leading kinematics_ref.scene_keep(n)
columns real.  Of the synthetic columns every second one is kinematics_ref.synthetic_state's -- in every third of those two joints are
moved 0.01 .. 0.02 rad beyond a bound (as generated the joints lie inside their limits: no limit row at all) and the base is levelled
again -- and the others are the "stance" family: the settled reset pose with a random yaw, a tilt of up to 0.12 rad, joints moved by
+-0.15 rad, a base velocity of up to 0.3 m/s and 1 rad/s, joint rates of up to 2 rad/s, and the base height that puts the lowest toe
point at -0.008 .. 0.012 m."""
import math

import numpy as np

import dynamics_ref as dr
import kinematics_ref as kr

NDOF = 18
ERP = 0.2                    # csrc/rex_device.h kErp
DAMP = 0.04                  # kLinDamp, kAngDamp
MAX_VEL = 100.0              # kMaxCoordVel
UNBOUNDED = 1e10
DT, ITERATIONS, THRESHOLD = 0.001, 60, 1e-7        # the config's defaults (walk: 300 // action_repeat sweeps)
LEVER = dr.LEVER
FIELDS = ("toe_force", "toe_lambda", "limit_torque", "v_next")
GAP_MARGIN = 1e-6            # rad: a joint this near its bound may take either side in float32
MU_RANGE = (0.3, 0.9)
TAU_RANGE = 3.0
# the settled reset pose (walk, ik signal, on the plane): pitch and joint angles the oracle's reset leaves, rounded
STANCE_PITCH = -0.0099
STANCE_Q = np.array([0.0, -0.916, 1.3457, 0.0, -0.916, 1.3457, 0.0, -0.9006, 1.3202, 0.0, -0.9006, 1.3202])


def plane_space(n, f=np.float64):
    """btPlaneSpace1 (csrc/rex_device.h plane_space)"""
    n = np.asarray(n, f)
    if abs(n[2]) > f(0.7071067811865475244):
        a = n[1] * n[1] + n[2] * n[2]
        k = f(1) / np.sqrt(a)
        p = np.array([0, -n[2] * k, n[1] * k], dtype=f)
        q = np.array([a * k, -n[0] * p[2], n[0] * p[1]], dtype=f)
    else:
        a = n[0] * n[0] + n[1] * n[1]
        k = f(1) / np.sqrt(a)
        p = np.array([-n[1] * k, n[0] * k, 0], dtype=f)
        q = np.array([-n[2] * p[1], n[2] * p[0], a * k], dtype=f)
    return p, q


def damping_force(lks, jac, f):
    """the generalized force of the per-link damping, [18] in dtype f"""
    d = np.zeros(NDOF, dtype=f)
    c = f(DAMP)
    for lk, (Jv, Jw) in zip(lks, jac):
        F = (lk["m"] * (c + c * np.sqrt(lk["vc"] @ lk["vc"])) * lk["vc"]).astype(f)
        N = ((c + c * np.sqrt(lk["w"] @ lk["w"])) * (lk["I"] @ lk["w"])).astype(f)
        d = (d + Jv.T @ F + Jw.T @ N).astype(f)
    return d


def gaps(q):
    """-> (gap [12], sgn [12]): the distance of each joint to its nearer bound (negative beyond it) and the row's sign"""
    q = np.asarray(q)
    lo, hi = q - kr.JLOWER.astype(q.dtype), kr.JUPPER.astype(q.dtype) - q
    lower = lo < hi
    return np.where(lower, lo, hi), np.where(lower, 1.0, -1.0).astype(q.dtype)


def pgs(M, rows, iterations, threshold, f):
    """rows: list of dict(J [18], rhs_num, lo, hi, normal (index of its normal row or -1), mu): rhs = rhs_num / diag.
    -> (dv [18], lambda [len(rows)], sweeps, the per-sweep `worst`)"""
    if not rows:
        return np.zeros(NDOF, dtype=f), np.zeros(0, dtype=f), 1 if iterations >= 1 else 0, [0.0]
    J = np.array([r["J"] for r in rows], dtype=f)
    resp = np.linalg.solve(np.asarray(M, f), J.T).T.astype(f)
    diag = np.einsum("rk,rk->r", J, resp).astype(f)
    rhs = (np.array([r["rhs_num"] for r in rows], dtype=f) / diag).astype(f)
    lam = np.zeros(len(rows), dtype=f)
    dv = np.zeros(NDOF, dtype=f)
    sweeps, trace = 0, []
    for _ in range(iterations):
        worst = f(0)
        for i, r in enumerate(rows):
            lo, hi = f(r["lo"]), f(r["hi"])
            if r["normal"] >= 0:
                hi = f(r["mu"]) * lam[r["normal"]]
                lo = -hi
            dl = rhs[i] - (J[i] @ dv) / diag[i]
            s = lam[i] + dl
            if s < lo:
                dl, s = lo - lam[i], lo
            elif s > hi:
                dl, s = hi - lam[i], hi
            lam[i] = s
            dv = (dv + resp[i] * dl).astype(f)
            worst = max(worst, (dl * diag[i]) ** 2)
        sweeps += 1
        trace.append(float(worst))
        if worst <= threshold:
            break
    return dv, lam, sweeps, trace


def reference(state, env, field=None, scales=(1.0, 1.0), mu=0.5, tau=None, dt=DT, iterations=ITERATIONS, residual_threshold=0.0, damping=True,
              dtype=np.float64, dyn=None):
    """Every output of rex_contact_solve for env `env` of `state` (numpy [words, n] float32) in `dtype` arithmetic: toe_force, toe_lambda
    [8, 3], limit_torque [12], v_next [18], sweeps; and what the tests sort cases by: v_star, in_reach [8], gap [12], limit [12] bool,
    trace (the residual of every sweep), dyn (dynamics_ref.reference's result).  residual_threshold 0: `iterations` sweeps, as the kernel
    counts them (the loop itself ends earlier only once a sweep changed nothing at all)."""
    f = dtype
    r = dyn if dyn is not None else dr.reference(state, env, field, scales, f)
    kin = r["kin"]
    M, h, Jp = np.asarray(r["mass_matrix"], f), np.asarray(r["bias"], f), np.asarray(r["toe_jacobian"], f)
    s = state[:, env].astype(f)
    v = np.concatenate([s[7:13], s[25:37]]).astype(f)
    q = s[13:25]
    b = np.zeros(NDOF, dtype=f)
    if tau is not None:
        b[6:] = np.asarray(tau, f)
    b = (b - h).astype(f)
    if damping:
        lks = dr.links(kin, scales, f)
        o0 = kin["link_pos"][0].astype(f)
        b = (b - damping_force(lks, [dr.link_jacobians(lk, o0, f) for lk in lks], f)).astype(f)
    dt = f(dt)
    v_star = (v + dt * np.linalg.solve(M, b).astype(f)).astype(f)
    gap, sgn = gaps(q)
    rows, limit_rows, normal_rows = [], {}, {}
    for j in range(12):
        if gap[j] < 0:
            J = np.zeros(NDOF, dtype=f)
            J[6 + j] = sgn[j]
            limit_rows[j] = len(rows)
            rows.append(dict(J=J, rhs_num=-gap[j] * f(ERP) / dt - sgn[j] * v_star[6 + j], lo=0.0, hi=UNBOUNDED, normal=-1, mu=0.0))
    dist, nrm, reach = np.asarray(kin["toe_dist"], f), np.asarray(kin["toe_normal"], f), np.asarray(kin["toe_in_reach"], bool)
    for p in range(8):
        if reach[p]:
            J = (nrm[p] @ Jp[p]).astype(f)
            poserr = f(0) if dist[p] > 0 else -dist[p] * f(ERP) / dt
            velerr = -(J @ v_star) - (dist[p] / dt if dist[p] > 0 else f(0))
            normal_rows[p] = len(rows)
            rows.append(dict(J=J, rhs_num=poserr + velerr, lo=0.0, hi=UNBOUNDED, normal=-1, mu=0.0))
    tangents = {}
    for p in range(8):
        if reach[p]:
            tangents[p] = plane_space(nrm[p], f)
            for t in tangents[p]:
                J = (t @ Jp[p]).astype(f)
                rows.append(dict(J=J, rhs_num=-(J @ v_star), lo=0.0, hi=0.0, normal=normal_rows[p], mu=mu))
    dv, lam, sweeps, trace = pgs(M, rows, iterations, residual_threshold, f)
    toe_lambda, toe_force, limit_torque = np.zeros((8, 3), dtype=f), np.zeros((8, 3), dtype=f), np.zeros(12, dtype=f)
    k = len(limit_rows) + len(normal_rows)
    for p in sorted(normal_rows):
        toe_lambda[p] = [lam[normal_rows[p]], lam[k], lam[k + 1]]
        k += 2
        toe_force[p] = (toe_lambda[p, 0] * nrm[p] + toe_lambda[p, 1] * tangents[p][0] + toe_lambda[p, 2] * tangents[p][1]) / dt
    for j, i in limit_rows.items():
        limit_torque[j] = sgn[j] * lam[i] / dt
    if residual_threshold == 0:
        sweeps = iterations
    return dict(toe_force=toe_force, toe_lambda=toe_lambda, limit_torque=limit_torque, v_next=np.clip(v_star + dv, -MAX_VEL, MAX_VEL).astype(f),
                sweeps=sweeps, v_star=v_star, in_reach=reach, gap=gap, limit=gap < 0, trace=trace, dyn=r, mu=mu)


# ---------------------------------------------------------------- the error measure
def errors(a, r, dt=DT):
    """Deviation of the outputs `a` of one env (any subset of FIELDS, shaped as reference()'s) from the float64 reference r, one number per
    field, each relative to a scale of that env:
      v_next        largest component of the difference / max(1, largest |component| of the reference)
      toe_lambda    largest component / max(largest |lambda_ref| of the env, total mass x 10 x dt)  -- the impulse that carries the robot
      toe_force     largest component / max(largest |force_ref| component of the env, total mass x 10)
      limit_torque  largest component / max(largest |torque_ref| of the env, total mass x 10 x LEVER (0.1 m))"""
    mass = float(r["dyn"]["mass"])
    scale = dict(v_next=1.0, toe_lambda=mass * 10.0 * dt, toe_force=mass * 10.0, limit_torque=mass * 10.0 * LEVER)
    out = {}
    for k in FIELDS:
        if k in a:
            ref = np.asarray(r[k], np.float64)
            out[k] = float(np.abs(np.asarray(a[k], np.float64).reshape(ref.shape) - ref).max() / max(scale[k], np.abs(ref).max()))
    return out


# ---------------------------------------------------------------- the scenes
def _level(s, field, lo, hi, rng):
    """the base height that puts the lowest toe point at a distance drawn from lo .. hi"""
    s[2, 0] = 0.0
    r = kr.reference(s, 0, False, field)
    s[2, 0] = rng.uniform(lo, hi) - float((r["toe_dist"] / r["toe_normal"][:, 2]).min())


def stance_state(rng, field, off_xy=None):
    """one env's words 0 .. 36, float32: the "stance" family of the module docstring"""
    s = np.zeros((37, 1), np.float64)
    yaw, tilt, heading = rng.uniform(-math.pi, math.pi), rng.uniform(0, 0.12), rng.uniform(0, 2 * math.pi)
    s[0:2, 0] = rng.uniform(-3, 3, 2)
    q = kr._quat_mul([math.sin(tilt / 2) * math.cos(heading), math.sin(tilt / 2) * math.sin(heading), 0, math.cos(tilt / 2)],
                     [0, math.sin(STANCE_PITCH / 2), 0, math.cos(STANCE_PITCH / 2)])
    s[3:7, 0] = kr._quat_mul([0, 0, math.sin(yaw / 2), math.cos(yaw / 2)], q)
    u = rng.standard_normal(3)
    s[7:10, 0] = rng.uniform(0, 0.3) * u / np.linalg.norm(u)
    u = rng.standard_normal(3)
    s[10:13, 0] = rng.uniform(0, 1.0) * u / np.linalg.norm(u)
    s[13:25, 0] = STANCE_Q + rng.uniform(-0.15, 0.15, 12)
    s[25:37, 0] = rng.uniform(-2, 2, 12)
    s = s.astype(np.float32)
    _level(s, field, -0.008, 0.012, rng)
    return s[:, 0]


def scene_states(n, ground):
    """-> (S float32 [episode word + 1, n], kinds [n]) of a mark-base scene: kinematics_ref.scene_states with the columns rewritten as the
    module docstring says; kinds: "real", kinematics_ref's kind, that + "+limit", or "stance" """
    keep = kr.scene_keep(n)
    S, kinds = kr.scene_states(False, n, ground, keep)
    fields = kr.scene_fields(ground)
    ep = S[kr.episode_word(False)].view(np.int32)
    rng = np.random.RandomState(4000 + 17 * n + {"plane": 0, "random": 1, "custom": 2}[ground])
    for g in range(keep, n):
        i, fld = g - keep, kr.field_of(fields, g, ep[g])
        if i % 2 == 1:
            S[0:37, g] = stance_state(rng, fld)
            kinds[g] = "stance"
        elif (i // 2) % 3 == 0 and kinds[g] == "random":
            s = S[0:37, g:g + 1].copy()
            for j in rng.choice(12, 2, replace=False):
                beyond = rng.uniform(0.01, 0.02)
                s[13 + j, 0] = kr.JLOWER[j] - beyond if rng.rand() < 0.5 else kr.JUPPER[j] + beyond
            _level(s, fld, -0.01, 0.06, rng)
            S[0:37, g] = s[:, 0]
            kinds[g] = "random+limit"
    return S, kinds


def scene_params(n, seed=61):
    """-> (tau [n, 12] float32 uniform in +-3 N m, mu [n] float32 in MU_RANGE) of a scene; the mass scales are dynamics_ref.scene_scales(n)"""
    rng = np.random.RandomState(seed + n)
    return rng.uniform(-TAU_RANGE, TAU_RANGE, (n, 12)).astype(np.float32), rng.uniform(*MU_RANGE, n).astype(np.float32)


def compared(state, g, field, ref, toe_dist_bound, position_shift):
    """whether env g enters the numerical comparison: no discrete decision of its problem within round-off of its threshold -- a toe_dist
    within `toe_dist_bound` of the breaking distance, a gap within GAP_MARGIN of 0, a toe point kinematics_ref.stable_points rejects"""
    kin = ref["dyn"]["kin"]
    if np.any(np.abs(np.asarray(kin["toe_dist"], np.float64) - kr.BREAKING) <= toe_dist_bound) or np.any(np.abs(ref["gap"]) <= GAP_MARGIN):
        return False
    return bool(np.all(dr.stable_points(state, g, field, kin, position_shift)))


def scene_reference(n, ground, state=None, heights=None, mids=None, dtype=np.float64, unit=False, **kw):
    """per env of a scene: reference() with the scene's tau, mass scales and friction (unit=True: scales 1, mu 0.5), on `state` (default:
    scene_states alone, whose leading columns are zero and are skipped: None)"""
    S, kinds = scene_states(n, ground)
    keep = kr.scene_keep(n) if state is None else 0
    state = S if state is None else state
    fields = kr.scene_fields(ground, heights, mids)
    ep = state[kr.episode_word(False)].view(np.int32)
    tau, mu = scene_params(n)
    bs, ls = dr.scene_scales(n)
    rows = []
    for g in range(n):
        if g < keep:
            rows.append(None)
            continue
        fld = kr.field_of(fields, g, ep[g])
        sc, m = ((1.0, 1.0), 0.5) if unit else ((bs[g], ls[g]), float(mu[g]))
        ref = reference(state, g, fld, sc, m, tau[g], dtype=dtype, **kw)
        ref.update(env=g, kind=kinds[g], field=fld)
        rows.append(ref)
    return rows


# ---------------------------------------------------------------- what the reference alone says about the GPU test's scenes
def measure_floors(toe_dist_bound, position_shift):
    """Over the synthetic columns of every scene with scene_params() and dynamics_ref.scene_scales(), at residual_threshold 0 and ITERATIONS
    sweeps: per field the largest errors() of reference() evaluated in float32 from float64 over the compared envs (compared()), and the
    coverage of the scenes.  -> (floors, stats): stats holds per scene (envs, compared) and, over all compared envs, the counts `envs`,
    `four_points` (four or more points in reach), `four_legs` (every leg has a point in reach), `limit` (a limit row), `sticking` and
    `sliding` (friction rows of loaded points), `early` and `full` (envs that leave before / run all ITERATIONS sweeps at THRESHOLD)."""
    floors = {k: 0.0 for k in FIELDS}
    stats = dict(scenes={}, envs=0, four_points=0, four_legs=0, limit=0, sticking=0, sliding=0, early=0, full=0)
    for _, n, ground in dr.SCENES:
        S, _ = scene_states(n, ground)
        r64 = scene_reference(n, ground)
        r32 = scene_reference(n, ground, dtype=np.float32)
        kept = 0
        for g in range(kr.scene_keep(n), n):
            a, b = r64[g], r32[g]
            if not compared(S, g, a["field"], a, toe_dist_bound, position_shift):
                continue
            kept += 1
            for k, v in errors(b, a).items():
                floors[k] = max(floors[k], v)
            reach, lam = a["in_reach"], a["toe_lambda"]
            stats["envs"] += 1
            stats["four_points"] += int(reach.sum() >= 4)
            stats["four_legs"] += int(reach.reshape(4, 2).any(1).all())
            stats["limit"] += int(a["limit"].any())
            loaded = lam[:, 0] > 0
            slide = np.abs(lam[:, 1:]) >= a["mu"] * lam[:, 0:1]
            stats["sliding"] += int((slide & loaded[:, None]).sum())
            stats["sticking"] += int((~slide & loaded[:, None]).sum())
            first = next((i + 1 for i, w in enumerate(a["trace"]) if w <= THRESHOLD), ITERATIONS)
            stats["early"] += int(first < ITERATIONS)
            stats["full"] += int(first >= ITERATIONS and a["trace"][-1] > THRESHOLD)
        stats["scenes"][(n, ground)] = (n - kr.scene_keep(n), kept)
    return floors, stats
