"""Force distribution of a batch (include/rexsim.h: rex_force_distribution): the ground forces inside the friction cones of the stance toe
points that best produce a wanted generalized acceleration, and the joint torques that go with them -- per env a cone-constrained
regularised least-squares problem, solved by a fixed number of accelerated projected-gradient steps in one read-only launch on the env's
device and stream.  Mark base.

    fd = env.force_distribution(vdot=vdot, stance=stance)  # every field; stance [k, 4] bool per leg, None: the toe points in reach
    fd.toe_force                                           # float32 [k, 4, 2, 3]: world N at kinematics().toe_pos, inside the cones
    fd.tau                                                 # float32 [k, 12]: the joint torques that realise vdot under those forces
    fd.base_residual                                       # float32 [k, 6]: the base wrench the ground does not supply
    fd.residual                                            # float32 [k]: the fixed-point residual, N -- how far the solve is from done
    small = env.force_distribution(fields=("tau",))        # vdot None: hold still
    env.force_distribution(fields=("tau",), out=small)     # refilled in place: a per-step read allocates nothing

The problem, with r = (M vdot + bias - base_wrench)[:6] the base rows of the equation of motion and A f = (sum_p f_p, sum_p d_p x f_p):

    minimise  1/2 (A f - r)^T diag(weights) (A f - r) + 1/2 eps sum_p |f_p|^2    over f_p in its cone, f_p = 0 outside the stance set

eps > 0 makes the solution unique and biases it: A f falls short of a reachable r by a ridge shrinkage of the order eps / sigma_min(A)^2.
Conventions of env.dynamics(); like bias, tau holds no damping, joint-limit or motor terms."""
import ctypes

from . import _lib, readout

# name -> trailing shape after the row count
FIELDS = {"toe_force": (4, 2, 3), "tau": (12,), "base_residual": (6,), "residual": ()}
assert list(FIELDS) == [f[0] for f in _lib.RexForceDistributionOut._fields_]
WEIGHTS = (1.0, 1.0, 1.0, 100.0, 100.0, 100.0)             # a moment counted over a 0.1 m lever
EPS = 1e-2
ITERATIONS = 1500                                          # tests/test_force_distribution_host.py derives it
MAX_ITERATIONS = 10000


def field_shape(name, k):
    return (k,) + FIELDS[name]


class ForceDistribution(readout.Result):
    """The result of RexBatchEnv.force_distribution: one tensor attribute per computed field (the others are None), `fields` their names,
    and `struct` the RexForceDistributionOut the launch was given."""
    WHO, FIELDS, STRUCT = "force_distribution", FIELDS, _lib.RexForceDistributionOut


def check_fields(fields):
    """fields of RexBatchEnv.force_distribution -> their names in the order of FIELDS"""
    return readout.check_fields(FIELDS, "force_distribution", fields)


def check_result(out, names, k, env):
    """a result handed back through out=: its fields, shapes, dtypes, device"""
    readout.check_result(ForceDistribution, out, names, k, env)


def check_params(weights=None, eps=None, friction_scale=1.0, iterations=None, who="force_distribution"):
    """the launch-uniform settings -> RexForceDistributionParams; None takes the default"""
    weights = WEIGHTS if weights is None else tuple(float(w) for w in weights)
    eps = EPS if eps is None else float(eps)
    friction_scale = float(friction_scale)
    iterations = ITERATIONS if iterations is None else iterations
    finite = lambda v: v == v and abs(v) != float("inf")
    if len(weights) != 6 or not all(finite(w) and w > 0 for w in weights):
        raise ValueError(f"{who}: weights must be 6 finite positive numbers, got {weights}")
    if not (finite(eps) and eps > 0):
        raise ValueError(f"{who}: eps must be finite and positive (the problem has 24 unknowns and at most 6 equations), got {eps}")
    if not (finite(friction_scale) and friction_scale >= 0):
        raise ValueError(f"{who}: friction_scale must be finite and not negative, got {friction_scale}")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"{who}: iterations must be an int in 1 .. {MAX_ITERATIONS}, got {iterations!r}")
    return _lib.RexForceDistributionParams((ctypes.c_float * 6)(*weights), eps, friction_scale, iterations)


def stance_tensor(env, stance, k, who):
    """stance= -> a contiguous uint8 [k, 4] tensor on the env's device (bool is viewed, not copied)"""
    torch = env._torch
    if not (isinstance(stance, torch.Tensor) and stance.dtype in (torch.bool, torch.uint8) and stance.device == env.device):
        raise ValueError(f"{who}: stance must be a bool or uint8 tensor on {env.device}")
    if tuple(stance.shape) != (k, 4) or not stance.is_contiguous():
        raise ValueError(f"{who}: stance must be contiguous with shape {(k, 4)}, got {tuple(stance.shape)}")
    return stance.view(torch.uint8) if stance.dtype == torch.bool else stance


def solve(env, vdot=None, base_wrench=None, stance=None, weights=None, eps=None, friction_scale=1.0, iterations=None, fields=None,
          env_ids=None, out=None):
    """RexBatchEnv.force_distribution (documented there)."""
    who = "force_distribution"
    readout.not_arm(env, who)
    if env.config.on_rack:
        raise ValueError(f"{who}: an on_rack env holds its base with an anchor the problem leaves out")
    if env.config.body_contacts:
        raise ValueError(f"{who}: an env with body_contacts pushes with link boxes the problem leaves out")
    names = check_fields(fields)
    params = check_params(weights, eps, friction_scale, iterations, who)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        vdot = None if vdot is None else readout.load_tensor(env, vdot, k, (readout.NDOF,), who, "vdot")
        base_wrench = None if base_wrench is None else readout.load_tensor(env, base_wrench, k, (6,), who, "base_wrench")
        stance = None if stance is None else stance_tensor(env, stance, k, who)
        out = readout.result(ForceDistribution, env, out, names, k)
        _lib.check(env._L.rex_force_distribution(env._h, readout.ptr(ids), k, readout.ptr(vdot), readout.ptr(base_wrench), readout.ptr(stance),
                                                 ctypes.byref(params), ctypes.byref(out.struct), env._stream_ptr()), "rex_force_distribution")
    return out
