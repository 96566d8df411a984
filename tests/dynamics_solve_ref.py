"""The numpy reference of the solves with the mass matrix (rex_dynamics_solve, rex_forward_dynamics, rex_apply_impulse), independent of the
kernel (tests/test_dynamics_solve_host.py, tests/test_gpu_dynamics_solve.py).  M, h and the toe Jacobians J are dynamics_ref.reference's,
float64:

    x_ref = np.linalg.solve(M_ref, b)
    forward dynamics   b = S^T tau + sum_p J_p^T f_p + w - h          (w: force at the base origin and moment, rows 0..5)
    impulse            b = S^T j   + sum_p J_p^T p_p + w

Two float32 routes for the round-off floor, as dynamics_ref has two:
    dense_cholesky()     M = G G^T of the whole 18 x 18 of dynamics_ref.reference() evaluated in float32, two triangular solves
    block_elimination()  over M's structure -- the leg blocks H_f = L D L^T, Y_f = H_f^-1 B_f^T, the Schur complement
                         A = Mb - sum_f B_f Y_f = G G^T, x_0 = A^-1 (b_0 - sum_f Y_f^T b_f), x_f = H_f^-1 b_f - Y_f x_0 -- on the M of
                         dynamics_ref.reference_composite() evaluated in float32
with right-hand sides assembled in float32 from the same route's h (and the float32 J).  The kernel's operation order is neither's.

Error measure of one right-hand side:  |D^1/2 (x - x_ref)|_2 / (kappa |D^1/2 x_ref|_2)  with D = diag(M_ref) and
kappa = cond_2(D^-1/2 M_ref D^-1/2) of that env in float64: a solve loses about kappa times the unit round-off, so a nearly straight leg
(a large kappa) does not set the bound of every other state."""
import numpy as np

import dynamics_ref as dr
import kinematics_ref as kr

NDOF = 18
KINDS = ("solve", "forward", "impulse")
COMBOS = (("tau",), ("toe",), ("wrench",), ("tau", "toe", "wrench"))       # the inputs of a load given alone, and all together
K_SET = 6


# ---------------------------------------------------------------- small dense routines in a chosen precision
def cholesky(A, f):
    """lower G with A = G G^T, every operation in dtype f"""
    A = np.asarray(A, f)
    n = A.shape[0]
    G = np.zeros((n, n), f)
    for j in range(n):
        s = f(A[j, j] - f(G[j, :j] @ G[j, :j]))
        G[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            G[i, j] = f(A[i, j] - f(G[i, :j] @ G[j, :j])) / G[j, j]
    return G


def cholesky_solve(G, b, f):
    n = G.shape[0]
    y, x = np.zeros(n, f), np.zeros(n, f)
    for i in range(n):
        y[i] = f(b[i] - f(G[i, :i] @ y[:i])) / G[i, i]
    for i in range(n - 1, -1, -1):
        x[i] = f(y[i] - f(G[i + 1:, i] @ x[i + 1:])) / G[i, i]
    return x


def ldl(H, f):
    """unit lower L and d with H = L diag(d) L^T, in dtype f"""
    H = np.asarray(H, f)
    n = H.shape[0]
    L, d = np.eye(n, dtype=f), np.zeros(n, f)
    for j in range(n):
        d[j] = f(H[j, j] - f((L[j, :j] * L[j, :j]) @ d[:j]))
        for i in range(j + 1, n):
            L[i, j] = f(H[i, j] - f((L[i, :j] * L[j, :j]) @ d[:j])) / d[j]
    return L, d


def ldl_solve(L, d, b, f):
    n = L.shape[0]
    y, x = np.zeros(n, f), np.zeros(n, f)
    for i in range(n):
        y[i] = f(b[i] - f(L[i, :i] @ y[:i]))
    for i in range(n - 1, -1, -1):
        x[i] = f(y[i] / d[i] - f(L[i + 1:, i] @ x[i + 1:]))
    return x


def dense_cholesky(M, B, f=np.float64):
    """X [K, 18] with M X_k = B_k by a Cholesky factorisation of the whole matrix in dtype f"""
    G = cholesky(M, f)
    return np.array([cholesky_solve(G, b, f) for b in np.asarray(B, f).reshape(-1, NDOF)], dtype=f)


def block_elimination(M, B, f=np.float64):
    """the same by elimination of the four leg blocks (module docstring) in dtype f"""
    M, B = np.asarray(M, f), np.asarray(B, f).reshape(-1, NDOF)
    legs = [slice(6 + 3 * l, 9 + 3 * l) for l in range(4)]
    fac = [ldl(M[s, s], f) for s in legs]
    Y = [np.array([ldl_solve(L, d, M[k, s], f) for k in range(6)], dtype=f).T for (L, d), s in zip(fac, legs)]         # [3, 6] each
    A = M[0:6, 0:6].copy()
    for s, Yf in zip(legs, Y):
        A = (A - M[0:6, s] @ Yf).astype(f)
    G = cholesky(A, f)
    X = np.zeros_like(B)
    for x, b in zip(X, B):
        c = b[0:6].copy()
        for s, Yf in zip(legs, Y):
            c = (c - Yf.T @ b[s]).astype(f)
        x[0:6] = cholesky_solve(G, c, f)
        for s, Yf, (L, d) in zip(legs, Y, fac):
            x[s] = (ldl_solve(L, d, b[s], f) - Yf @ x[0:6]).astype(f)
    return X


# ---------------------------------------------------------------- right-hand sides
def rhs_set(r, seed):
    """K_SET right-hand sides [6, 18] float32 for one env with reference r: three with entries sqrt(M_ii) times a standard normal, J_p^T of a
    unit force at one toe point, h itself, one unit vector on a foot joint."""
    rng = np.random.RandomState(seed)
    M = np.asarray(r["mass_matrix"], np.float64)
    B = np.zeros((K_SET, NDOF))
    B[0:3] = np.sqrt(np.diag(M)) * rng.standard_normal((3, NDOF))
    u = rng.standard_normal(3)
    B[3] = np.asarray(r["toe_jacobian"], np.float64)[rng.randint(8)].T @ (u / np.linalg.norm(u))
    B[4] = r["bias"]
    B[5, 8 + 3 * rng.randint(4)] = 1.0
    return B.astype(np.float32)


def loads(n, seed=41):
    """the loads of a scene, float32: tau [n, 12] N m (impulses: N m s), toe [n, 8, 3] N with a push from below, wrench [n, 6]"""
    rng = np.random.RandomState(seed + n)
    toe = rng.normal(0.0, 4.0, (n, 8, 3))
    toe[:, :, 2] += 8.0
    return dict(tau=rng.normal(0.0, 2.0, (n, 12)).astype(np.float32), toe=toe.astype(np.float32),
                wrench=(rng.normal(0.0, 1.0, (n, 6)) * [20, 20, 20, 3, 3, 3]).astype(np.float32))


def load_rhs(J, h, tau=None, toe=None, wrench=None, f=np.float64):
    """b = S^T tau + sum_p J_p^T f_p + w - h in dtype f; J [8, 3, 18]; h None: an impulse"""
    b = np.zeros(NDOF, f)
    if tau is not None:
        b[6:] = np.asarray(tau, f)
    if toe is not None:
        b = (b + np.einsum("pcd,pc->d", np.asarray(J, f), np.asarray(toe, f)).astype(f)).astype(f)
    if wrench is not None:
        b[0:6] = b[0:6] + np.asarray(wrench, f)
    if h is not None:
        b = (b - np.asarray(h, f)).astype(f)
    return b


def pick(load, g, combo, ok=None):
    """the members `combo` of a scene's loads for env g (the others None); toe forces zero at the points ~ok"""
    out = {k: (load[k][g].copy() if k in combo else None) for k in ("tau", "toe", "wrench")}
    if out["toe"] is not None and ok is not None:
        out["toe"][~ok] = 0.0
    return out


# ---------------------------------------------------------------- the error measure
def conditioning(M):
    """(D^1/2 [18], kappa) of a float64 mass matrix"""
    M = np.asarray(M, np.float64)
    s = np.sqrt(np.diag(M))
    return s, float(np.linalg.cond(M / np.outer(s, s), 2))


def errors(X, X_ref, M_ref):
    """[K]: |D^1/2 (x - x_ref)| / (kappa |D^1/2 x_ref|) per right-hand side"""
    s, kappa = conditioning(M_ref)
    X, X_ref = np.asarray(X, np.float64).reshape(-1, NDOF), np.asarray(X_ref, np.float64).reshape(-1, NDOF)
    return np.linalg.norm((X - X_ref) * s, axis=-1) / (kappa * np.linalg.norm(X_ref * s, axis=-1))


def solve_ref(M, B):
    return np.linalg.solve(np.asarray(M, np.float64), np.asarray(B, np.float64).reshape(-1, NDOF).T).T


def rhs_seed(n, g):
    return 7000 + 131 * n + g


# ---------------------------------------------------------------- what the reference alone says about the GPU test's scenes
def measure_floors(position_shift):
    """Over the synthetic columns of dynamics_ref.SCENES with scene_scales() and loads(): per kind the larger error (errors()) of the two
    float32 routes against the float64 reference, the forward and impulse right-hand sides over COMBOS with toe forces only at the points
    dynamics_ref.measure_floors keeps.  -> (floors, (smallest, largest kappa), points, points that carry a force)"""
    f = np.float32
    floors = {k: 0.0 for k in KINDS}
    kappas, points, kept = [], 0, 0
    for _, n, ground in dr.SCENES:
        S, _ = kr.scene_states(False, n, ground, kr.scene_keep(n))
        fields = kr.scene_fields(ground)
        ep = S[kr.episode_word(False)].view(np.int32)
        bs, ls = dr.scene_scales(n)
        load = loads(n)
        for g in range(kr.scene_keep(n), n):
            fld, sc = kr.field_of(fields, g, ep[g]), (bs[g], ls[g])
            r64 = dr.reference(S, g, fld, sc)
            k32 = kr.reference(S, g, False, fld, f)
            r32, c32 = dr.reference(S, g, fld, sc, f, kin=k32), dr.reference_composite(S, g, fld, sc, f, kin=k32)
            ok = dr.stable_points(S, g, fld, r64["kin"], position_shift) & (k32["fid0"] == r64["kin"]["fid0"]) & (k32["fid1"] == r64["kin"]["fid1"])
            points, kept = points + 8, kept + int(ok.sum())
            M = r64["mass_matrix"]
            kappas.append(conditioning(M)[1])
            routes = ((dense_cholesky, r32["mass_matrix"], r32["bias"]), (block_elimination, c32["mass_matrix"], c32["bias"]))
            B = rhs_set(r64, rhs_seed(n, g))
            want = solve_ref(M, B)
            for route, M32, _ in routes:
                floors["solve"] = max(floors["solve"], float(errors(route(M32, B, f), want, M).max()))
            for combo in COMBOS:
                p = pick(load, g, combo, ok)
                for kind, h64 in (("forward", r64["bias"]), ("impulse", None)):
                    want = solve_ref(M, load_rhs(r64["toe_jacobian"], h64, **p))
                    for route, M32, h32 in routes:
                        b32 = load_rhs(r32["toe_jacobian"], h32 if kind == "forward" else None, f=f, **p)
                        floors[kind] = max(floors[kind], float(errors(route(M32, b32, f), want, M).max()))
    return floors, (min(kappas), max(kappas)), points, kept
