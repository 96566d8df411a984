"""The numpy reference of rex_force_distribution, independent of the kernel (tests/test_force_distribution_host.py,
tests/test_gpu_force_distribution.py): the problem and the iteration of include/rexsim.h restated on dynamics_ref.reference's M, h and toe
Jacobians and kinematics_ref's toe points, normals and distances, vectorised over the envs of a scene.

    r = (M vdot + h - w)[0:6];   A f = (sum_p f_p, sum_p d_p x f_p),  d_p = P_p - o_0
    minimise  1/2 (A f - r)^T W (A f - r) + 1/2 eps sum_p |f_p|^2   over f_p in K_p (p in S), f_p = 0 otherwise
    L = eps + sum_{p in S} [w_0 + w_1 + w_2 + w_3 (d_y^2 + d_z^2) + w_4 (d_x^2 + d_z^2) + w_5 (d_x^2 + d_y^2)],  beta from kappa = L / eps
    u = W (A y - r);  g_p = u_lin + u_ang x d_p + eps y_p;  f+_p = Proj_Kp(y_p - g_p / L);  y = f+ + beta (f+ - f);  f = f+       (`iterations` times)
    tau = (M vdot + h)[6:] - (sum_p J_p^T f_p)[6:];  base_residual = r - A f;  residual = L max_p |Proj(f - g(f) / L) - f|_inf

The float64 reference follows the same iteration step for step, so a comparison at a fixed step count does not depend on how far the
iteration has converged.  Two float32 routes for the round-off floors, as the other *_ref.py have them:
    "forward"  M, h, J of dynamics_ref.reference() in float32; the net wrench A y summed over the points p = 0 .. 7
    "reverse"  M, h of dynamics_ref.reference_composite() in float32; the net wrench summed over the points p = 7 .. 0
The kernel's operation order is neither's (it sums a leg's two points, then the four legs as (0 + 1) + (2 + 3)).

Error measures (the torques here carry ground forces, so the total weight is the scale, not the carried mass):
    toe_force      per point, the largest component of the difference / (10 mass)                                               [8]
    tau            per joint |d| / (10 mass 0.1 m)                                                                              [12]
    base_residual  per component |d| / (10 mass) for the force, / (10 mass 0.1 m) for the moment                                [6]
    residual       |d| / (10 mass)                                                                                              [1]"""
import numpy as np

import contact_space_ref as cs
import dynamics_ref as dr
import dynamics_solve_ref as sr
import kinematics_ref as kr

FIELDS = ("toe_force", "tau", "base_residual", "residual")
WEIGHTS = (1.0, 1.0, 1.0, 100.0, 100.0, 100.0)
EPS = 1e-2
GPU_ITERATIONS = 300                                       # what the GPU test runs: parity does not need convergence
STANCES = ("all", "trot_a", "trot_b", "three", "one", "none", "mix", "reach")
FRICTION_RANGE = (0.3, 0.9)


def scene_friction(n, seed=71):
    """per-env foot friction float32 [n] of the test scenes: fixed seed, 0.3 .. 0.9"""
    return np.random.RandomState(seed + n).uniform(*FRICTION_RANGE, n).astype(np.float32)


def stance_of(name, n, seed=83):
    """the stance set `name` of a scene: uint8 [n, 4] per leg, or None for "reach" (the points in reach)"""
    legs = {"all": (1, 1, 1, 1), "trot_a": (1, 0, 0, 1), "trot_b": (0, 1, 1, 0), "three": (1, 1, 0, 1), "one": (0, 1, 0, 0), "none": (0, 0, 0, 0)}
    if name == "reach":
        return None
    if name == "mix":
        return (np.random.RandomState(seed + n).uniform(size=(n, 4)) < 0.7).astype(np.uint8)
    return np.tile(np.array(legs[name], np.uint8), (n, 1))


def scene_inputs(n):
    """the wanted accelerations and base wrenches of a scene, float32: contact_space_ref.accelerations, dynamics_solve_ref.loads' wrench"""
    return {"vdot": cs.accelerations(n), "wrench": sr.loads(n)["wrench"]}


def problem(dyns, mu, stance=None, vdot=None, wrench=None, f=np.float64, bias=None):
    """dyns: dynamics_ref.reference()'s results of the envs (in dtype f for a float32 route); mu [n]; stance uint8 [n, 4] or None;
    vdot [n, 18], wrench [n, 6] or None; bias: another route's (M, h) per env.  -> the arrays of the problem in dtype f"""
    n = len(dyns)
    P = dict(r=np.zeros((n, 6), f), joint=np.zeros((n, 12), f), d=np.zeros((n, 8, 3), f), nrm=np.zeros((n, 8, 3), f), inS=np.zeros((n, 8), bool),
             col=np.zeros((n, 8, 3, 12), f), mu=np.asarray(mu, f), mass=np.array([float(r["mass"]) for r in dyns]))
    for g, r in enumerate(dyns):
        M, h = (r["mass_matrix"], r["bias"]) if bias is None else bias[g]
        y = np.asarray(h, f).copy()
        if vdot is not None:
            y = (y + np.asarray(M, f) @ np.asarray(vdot[g], f)).astype(f)
        P["joint"][g] = y[6:]
        P["r"][g] = y[:6] if wrench is None else (y[:6] - np.asarray(wrench[g], f)).astype(f)
        kin = r["kin"]
        P["d"][g] = (kin["toe_pos"].astype(f) - kin["link_pos"][0].astype(f)).astype(f)
        P["nrm"][g] = kin["toe_normal"].astype(f)
        P["inS"][g] = kin["toe_in_reach"] if stance is None else np.repeat(np.asarray(stance[g]) != 0, 2)
        P["col"][g] = np.asarray(r["toe_jacobian"], f)[:, :, 6:]
    return P


def project(P, x, f):
    """Proj_K of x [n, 8, 3] onto each point's cone; zero outside the stance set"""
    mu = P["mu"][:, None]
    nrm = P["nrm"]
    s = (nrm * x).sum(-1).astype(f)
    t = (x - s[..., None] * nrm).astype(f)
    tn = np.sqrt((t * t).sum(-1)).astype(f)
    sp = ((s + mu * tn) / (f(1) + mu * mu)).astype(f)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(tn > 0, mu * sp / tn, f(0)).astype(f)
    edge = (sp[..., None] * nrm + k[..., None] * t).astype(f)
    keep, none = tn <= mu * s, mu * tn <= -s
    q = np.where(keep[..., None], x, np.where(none[..., None], f(0), edge))
    return np.where(P["inS"][..., None], q, f(0)).astype(f)


def net_wrench(P, x, f, reverse=False):
    """A x [n, 6]: the points summed one after the other, p = 0 .. 7 or 7 .. 0"""
    lin, ang = np.zeros((x.shape[0], 3), f), np.zeros((x.shape[0], 3), f)
    for p in (range(7, -1, -1) if reverse else range(8)):
        lin = (lin + x[:, p]).astype(f)
        ang = (ang + np.cross(P["d"][:, p], x[:, p]).astype(f)).astype(f)
    return np.concatenate([lin, ang], -1)


def gradient(P, x, W, eps, f, reverse=False):
    u = (W * (net_wrench(P, x, f, reverse) - P["r"])).astype(f)
    return (u[:, None, 0:3] + np.cross(u[:, None, 3:6], P["d"]).astype(f) + eps * x).astype(f)


def lipschitz(P, W, eps, f):
    d2 = (P["d"] * P["d"]).astype(f)
    t = (W[0] + W[1] + W[2] + W[3] * (d2[..., 1] + d2[..., 2]) + W[4] * (d2[..., 0] + d2[..., 2]) + W[5] * (d2[..., 0] + d2[..., 1])).astype(f)
    return (eps + np.where(P["inS"], t, f(0)).sum(-1, dtype=f)).astype(f)


def outputs(P, x, W, eps, f, reverse=False):
    """the four outputs at the forces x [n, 8, 3]"""
    L = lipschitz(P, W, eps, f)
    g = gradient(P, x, W, eps, f, reverse)
    move = (project(P, (x - g / L[:, None, None]).astype(f), f) - x).astype(f)
    tau = (P["joint"] - np.einsum("gpcj,gpc->gj", P["col"], x).astype(f)).astype(f)
    return dict(toe_force=x.reshape(-1, 4, 2, 3), tau=tau, base_residual=(P["r"] - net_wrench(P, x, f, reverse)).astype(f),
                residual=(L * np.abs(move).max((-1, -2))).astype(f))


def solve(P, iterations, weights=WEIGHTS, eps=EPS, f=np.float64, reverse=False, keep=()):
    """`iterations` steps from f = y = 0 -> outputs(); keep: step counts whose forces are kept too, under the key "at" {count: x}"""
    W, eps = np.asarray(weights, f), f(eps)
    L = lipschitz(P, W, eps, f)
    sk = np.sqrt(L / eps).astype(f)
    beta = ((sk - f(1)) / (sk + f(1))).astype(f)[:, None, None]
    step = L[:, None, None]
    x, y = np.zeros_like(P["d"]), np.zeros_like(P["d"])
    at = {}
    for it in range(1, iterations + 1):
        xn = project(P, (y - gradient(P, y, W, eps, f, reverse) / step).astype(f), f)
        y = (xn + beta * (xn - x)).astype(f)
        x = xn
        if it in keep:
            at[it] = x.copy()
    out = outputs(P, x, W, eps, f, reverse)
    out["at"] = at
    return out


def objective(P, x, weights=WEIGHTS, eps=EPS):
    """[n]: the problem's objective at the forces x [n, 8, 3], float64"""
    e = net_wrench(P, x, np.float64) - P["r"]
    return 0.5 * (np.asarray(weights) * e * e).sum(-1) + 0.5 * eps * (x * x).sum((-1, -2))


def ridge(P, weights=WEIGHTS, eps=EPS):
    """[n, 8, 3]: A^T (A A^T + eps W^-1)^-1 r over the stance points, the solution when no cone binds"""
    out = np.zeros_like(P["d"])
    for g in range(P["d"].shape[0]):
        A = np.zeros((6, 24))
        for p in range(8):
            if P["inS"][g, p]:
                A[0:3, 3 * p:3 * p + 3] = np.eye(3)
                A[3:6, 3 * p:3 * p + 3] = dr._skew(P["d"][g, p], np.float64)
        out[g] = (A.T @ np.linalg.solve(A @ A.T + eps * np.diag(1.0 / np.asarray(weights)), P["r"][g])).reshape(8, 3)
    return out


def in_cones(P, x, slack=0.0):
    """[n, 8] bool: x_p inside K_p (to `slack` newtons), zero outside the stance set"""
    s = (P["nrm"] * x).sum(-1)
    t = np.linalg.norm(x - s[..., None] * P["nrm"], axis=-1)
    return np.where(P["inS"], t <= P["mu"][:, None] * s + slack, ~x.any(-1))


# ---------------------------------------------------------------- the error measures (module docstring)
def errors(a, ref, mass):
    """a: any subset of FIELDS over n envs; ref: solve()'s result; mass [n] -> per field the measures of the module docstring, [n, ...]"""
    out = {}
    force = 10.0 * np.asarray(mass, np.float64)
    d = lambda k: np.abs(np.asarray(a[k], np.float64) - np.asarray(ref[k], np.float64))
    if "toe_force" in a:
        out["toe_force"] = d("toe_force").reshape(-1, 8, 3).max(-1) / force[:, None]
    if "tau" in a:
        out["tau"] = d("tau") / (force[:, None] * dr.LEVER)
    if "base_residual" in a:
        out["base_residual"] = d("base_residual") / (force[:, None] * np.array([1.0] * 3 + [dr.LEVER] * 3))
    if "residual" in a:
        out["residual"] = d("residual").reshape(-1, 1) / force[:, None]
    return out


# ---------------------------------------------------------------- what the reference alone says about the GPU test's scenes
_SYNTHETIC = {}


def synthetic(position_shift):
    """The synthetic columns of every scene of dynamics_ref.SCENES as ONE batch (evaluated once and kept): dict(d64, d32: dynamics_ref.reference
    per env in float64 and float32; c32: (M, h) of reference_composite in float32; kept [k] bool: every toe point of the env is stable
    and found the same facets and the same in-reach flag in both precisions; mu, vdot, wrench: scene_friction and scene_inputs of those
    envs; stance: {name: uint8 [k, 4] or None}; plane [k] bool: the env stands on the plane)"""
    if position_shift in _SYNTHETIC:
        return _SYNTHETIC[position_shift]
    f = np.float32
    B = dict(d64=[], d32=[], c32=[], kept=[], mu=[], vdot=[], wrench=[], plane=[], stance={k: [] for k in STANCES})
    for _, n, ground in dr.SCENES:
        S, _ = kr.scene_states(False, n, ground, kr.scene_keep(n))
        fields = kr.scene_fields(ground)
        ep = S[kr.episode_word(False)].view(np.int32)
        bs, ls = dr.scene_scales(n)
        envs = list(range(kr.scene_keep(n), n))
        for g in envs:
            fld, sc = kr.field_of(fields, g, ep[g]), (bs[g], ls[g])
            r64 = dr.reference(S, g, fld, sc)
            k32 = kr.reference(S, g, False, fld, f)
            c = dr.reference_composite(S, g, fld, sc, f, kin=k32)
            ok = dr.stable_points(S, g, fld, r64["kin"], position_shift) & (k32["fid0"] == r64["kin"]["fid0"]) & (k32["fid1"] == r64["kin"]["fid1"])
            ok &= k32["toe_in_reach"] == r64["kin"]["toe_in_reach"]
            B["d64"].append(r64); B["d32"].append(dr.reference(S, g, fld, sc, f, kin=k32)); B["c32"].append((c["mass_matrix"], c["bias"]))
            B["kept"].append(bool(ok.all())); B["plane"].append(ground == "plane")
        inp = scene_inputs(n)
        B["mu"].append(scene_friction(n)[envs]); B["vdot"].append(inp["vdot"][envs]); B["wrench"].append(inp["wrench"][envs])
        for k in STANCES:
            if k != "reach":
                B["stance"][k].append(stance_of(k, n)[envs])
    for k in ("mu", "vdot", "wrench"):
        B[k] = np.concatenate(B[k])
    B["kept"], B["plane"] = np.array(B["kept"]), np.array(B["plane"])
    B["stance"] = {k: (None if k == "reach" else np.concatenate(v)) for k, v in B["stance"].items()}
    _SYNTHETIC[position_shift] = B
    return B


def problems(B, stance, given, rows=None):
    """(the float64 problem, route -> the float32 problem of that route) of the batch B for the stance set named `stance`, with B's (vdot,
    wrench) or with neither; rows: a bool mask over the batch"""
    rows = np.ones(len(B["d64"]), bool) if rows is None else rows
    pick = lambda v: None if v is None else v[rows]
    lst = lambda v: [x for x, r in zip(v, rows) if r]
    kw = dict(stance=pick(B["stance"][stance]), vdot=pick(B["vdot"]) if given else None, wrench=pick(B["wrench"]) if given else None)
    mu = B["mu"][rows]
    return problem(lst(B["d64"]), mu, **kw), lambda route: problem(lst(B["d32"]), mu, f=np.float32, bias=lst(B["c32"]) if route == "reverse" else None, **kw)


def stack(Ps):
    """several problems as one batch"""
    return {k: np.concatenate([P[k] for P in Ps]) for k in Ps[0]}


def routes32(P_of, iterations, **kw):
    """the two float32 routes: P_of(route) -> problem() of that route's data"""
    f = np.float32
    return [solve(P_of("forward"), iterations, f=f, reverse=False, **kw), solve(P_of("reverse"), iterations, f=f, reverse=True, **kw)]


def measure_floors(position_shift, iterations=GPU_ITERATIONS, stances=STANCES, givens=(True, False), rows=None):
    """Over synthetic(): per field the larger error of the two float32 routes against the float64 reference at the same step count, over the
    stance sets, with (vdot, wrench) and with neither, over the envs whose eight points are all kept.  -> (floors, envs, envs kept)"""
    B = synthetic(position_shift)
    kept = B["kept"] if rows is None else B["kept"][rows]
    floors = {k: 0.0 for k in FIELDS}
    for name in stances:
        for given in givens:
            P64, P_of = problems(B, name, given, rows)
            want = solve(P64, iterations)
            for got in routes32(P_of, iterations):
                for k, v in errors({k: got[k] for k in FIELDS}, want, P64["mass"]).items():
                    floors[k] = max(floors[k], float(v[kept].max()))
    return floors, len(kept), int(kept.sum())
