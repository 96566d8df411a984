"""The contact solve of a batch (include/rexsim.h: rex_contact_solve): ground reaction forces at the toe points, foot contact flags,
joint-limit torques and the contact-consistent next velocity of every env -- one substep of the step's physics restated for the current
state and solved in a read-only launch on the env's device and stream.  Mark base.

    con = env.contact_solve(tau=tau)                       # every field
    con.toe_force, con.foot_force                          # float32 [k, 4, 2, 3] world N at kinematics().toe_pos; [k, 4, 3] per leg
    con.foot_contact                                       # bool [k, 4]: a normal impulse > 0 at either end of the toe
    small = env.contact_solve(tau=tau, fields=("toe_force", "sweeps"))
    env.contact_solve(tau=tau, fields=("toe_force", "sweeps"), out=small)     # refilled in place: a per-step read allocates nothing

The problem (conventions of env.dynamics(): v = (base linear velocity, base angular velocity, 12 joint rates), world axes):
free velocity  v* = v + dt M^-1 (S^T tau - bias - damping);  rows in the solver's order -- a joint-limit row for every joint beyond its
bound, a normal row for every toe point in reach (toe_dist < 0.02 m), two friction rows per such point bounded by mu times the normal
impulse --;  projected Gauss-Seidel from zero impulses for `iterations` sweeps, or until a sweep's largest squared residual is within
`residual_threshold`;  v_next = clamp(v* + dv, +-100).

What tau has to be for the result to be the step's own forces: the step draws the torques from the motor model anew in every substep
(rex_motor_torque_params reproduces it) and the state holds no last torque, so the caller supplies tau; tau=None is zero torque."""
import ctypes

from . import _lib, readout

# name -> (trailing shape after the row count, dtype name)
FIELDS = {"toe_force": ((4, 2, 3), "float32"), "toe_lambda": ((4, 2, 3), "float32"), "limit_torque": ((12,), "float32"), "v_next": ((18,), "float32"),
          "sweeps": ((), "int32")}
assert list(FIELDS) == [f[0] for f in _lib.RexContactSolveOut._fields_]
MAX_ITERATIONS = 1000


def field_shape(name, k):
    return (k,) + FIELDS[name][0]


class ContactSolve(readout.Result):
    """The result of RexBatchEnv.contact_solve: one tensor attribute per computed field (the others are None), `fields` their names, and
    `struct` the RexContactSolveOut the launch was given."""
    WHO, FIELDS, STRUCT = "contact_solve", FIELDS, _lib.RexContactSolveOut

    @classmethod
    def shape_of(cls, name, k, env):
        return field_shape(name, k)

    @classmethod
    def dtype_of(cls, name):
        return FIELDS[name][1]

    @property
    def foot_force(self):
        """[k, 4, 3]: world force on each foot, the sum over the two ends of its toe"""
        if self.toe_force is None:
            raise AttributeError("foot_force needs the field toe_force")
        return self.toe_force.sum(dim=2)

    @property
    def foot_contact(self):
        """[k, 4] bool: a normal impulse > 0 at either end of the toe"""
        if self.toe_lambda is None:
            raise AttributeError("foot_contact needs the field toe_lambda")
        return (self.toe_lambda[..., 0] > 0).any(dim=2)


def check_fields(fields):
    """fields of RexBatchEnv.contact_solve -> their names in the order of FIELDS"""
    return readout.check_fields(FIELDS, "contact_solve", fields)


def check_settings(dt, iterations, residual_threshold):
    """the solver settings -> (dt, iterations, residual_threshold) of RexContactSolveIn; None: the config's (0, 0, -1)"""
    import math
    if dt is not None and not (isinstance(dt, (int, float)) and math.isfinite(dt) and dt > 0):
        raise ValueError(f"contact_solve: dt must be a finite number > 0, got {dt!r}")
    if iterations is not None and not (isinstance(iterations, int) and not isinstance(iterations, bool) and 1 <= iterations <= MAX_ITERATIONS):
        raise ValueError(f"contact_solve: iterations must be an int in 1..{MAX_ITERATIONS}, got {iterations!r}")
    if residual_threshold is not None and not (isinstance(residual_threshold, (int, float)) and math.isfinite(residual_threshold) and residual_threshold >= 0):
        raise ValueError(f"contact_solve: residual_threshold must be a finite number >= 0, got {residual_threshold!r}")
    return (0.0 if dt is None else float(dt), 0 if iterations is None else iterations, -1.0 if residual_threshold is None else float(residual_threshold))


def check_result(out, names, k, env):
    """a result handed back through out=: its fields, shapes, dtypes, device"""
    readout.check_result(ContactSolve, out, names, k, env)


def solve(env, tau=None, env_ids=None, fields=None, out=None, dt=None, iterations=None, residual_threshold=None, damping=True):
    """RexBatchEnv.contact_solve (documented there)."""
    who = "contact_solve"
    readout.not_arm(env, who)
    if env.config.on_rack:
        raise ValueError(f"{who}: an on_rack env holds its base with an anchor the solve leaves out")
    if env.config.body_contacts:
        raise ValueError(f"{who}: an env with body_contacts solves link-box rows the solve leaves out")
    names = check_fields(fields)
    settings = check_settings(dt, iterations, residual_threshold)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        tau = None if tau is None else readout.load_tensor(env, tau, k, (12,), who, "tau")
        out = readout.result(ContactSolve, env, out, names, k)
        inp = _lib.RexContactSolveIn(readout.ptr(tau), settings[0], settings[1], settings[2], 1 if damping else 0)
        _lib.check(env._L.rex_contact_solve(env._h, readout.ptr(ids), k, ctypes.byref(inp), ctypes.byref(out.struct), env._stream_ptr()),
                   "rex_contact_solve")
    return out
