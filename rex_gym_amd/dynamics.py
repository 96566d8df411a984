"""Rigid-body dynamics of a batch (include/rexsim.h: rex_dynamics): the joint-space mass matrix, the bias forces and their gravity
part, the Jacobians of the 8 toe contact candidates, the centre of mass and the momentum of every env in one launch, on the env's
device and stream.  Mark base.

    dyn = env.dynamics()                                 # every field
    dyn.mass_matrix, dyn.bias                            # float32 [num_envs, 18, 18], [num_envs, 18]; rows and columns = env.dof_names
    tau = torch.einsum("klecd,klec->kd", dyn.toe_jacobian, f)[:, 6:]      # tau = J^T f of world forces f [k, 4, 2, 3] at the toe points
    small = env.dynamics(fields=("bias", "com"))
    env.dynamics(fields=("bias", "com"), out=small)      # refilled in place: a per-step read allocates nothing

The generalized velocity is v = (world linear velocity of the base origin, world angular velocity of the base, 12 joint rates in
motor order), and  M(q) vdot + bias(q, v) = S^T tau + sum_p J_p^T f_p:  bias holds Coriolis, centrifugal, gyroscopic terms and
gravity (g = 10 m/s^2; a robot at rest has bias[0:3] = (0, 0, +mass * 10)), not the sim's damping forces.  toe_jacobian is shaped
[k, 4, 2, 3, 18] as (leg, end, world axis, dof): leg order front_left, front_right, rear_left, rear_right."""
import ctypes
import os
import re

from . import _lib

# name -> trailing shape after the row count
FIELDS = {"mass_matrix": (18, 18), "bias": (18,), "gravity": (18,), "toe_jacobian": (4, 2, 3, 18), "com": (6,), "momentum": (6,), "mass": ()}
assert list(FIELDS) == [f[0] for f in _lib.RexDynamicsOut._fields_]

BASE_DOF_NAMES = ("base_lin_x", "base_lin_y", "base_lin_z", "base_ang_x", "base_ang_y", "base_ang_z")
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")


def dof_names():
    """The 18 names of the generalized velocity's components: six of the base, then the motor names in motor order, from the row
    comments of REX_JOINT_POS (csrc/rex_model_gen.h)."""
    with open(os.path.join(_CSRC, "rex_model_gen.h")) as f:
        body = re.search(r"REX_JOINT_POS\[[^=]*=\s*\{(.*?)\n\};", f.read(), re.S).group(1)
    return BASE_DOF_NAMES + tuple(re.findall(r"/\*\s*(\w+)\s*\*/", body))


def field_shape(name, k):
    return (k,) + FIELDS[name]


class Dynamics:
    """The result of RexBatchEnv.dynamics: one tensor attribute per computed field (the others are None), `fields` their names, and
    `struct` the RexDynamicsOut the launch was given."""

    def __init__(self, tensors):
        self.fields = tuple(n for n in FIELDS if n in tensors)
        for n in FIELDS:
            setattr(self, n, tensors.get(n))
        self.struct = _lib.RexDynamicsOut(**{n: t.data_ptr() for n, t in tensors.items()})
        self.rows = int(next(iter(tensors.values())).shape[0])

    @property
    def com_pos(self):
        """[k, 3]: world position of the centre of mass"""
        if self.com is None:
            raise AttributeError("com_pos needs the field com")
        return self.com[:, 0:3]

    @property
    def com_vel(self):
        """[k, 3]: world velocity of the centre of mass"""
        if self.com is None:
            raise AttributeError("com_vel needs the field com")
        return self.com[:, 3:6]


def check_fields(fields):
    """fields of RexBatchEnv.dynamics -> their names in the order of FIELDS"""
    if fields is None:
        return tuple(FIELDS)
    if isinstance(fields, str):
        fields = (fields,)
    fields = tuple(fields)
    unknown = [f for f in fields if f not in FIELDS]
    if unknown or not fields:
        raise ValueError(f"dynamics: fields must be a non-empty subset of {tuple(FIELDS)}, got {fields}")
    return tuple(n for n in FIELDS if n in fields)


def check_result(out, names, k, env):
    """a result handed back through out=: its fields, shapes, dtypes, device"""
    torch = env._torch
    if not isinstance(out, Dynamics) or out.fields != names:
        raise ValueError(f"dynamics: out must be a result of dynamics() with the fields {names}")
    for n in names:
        t = getattr(out, n)
        shape = field_shape(n, k)
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == env.device and tuple(t.shape) == shape and t.is_contiguous()
                and t.data_ptr() == getattr(out.struct, n)):
            raise ValueError(f"dynamics: out.{n} must be the contiguous float32 tensor of shape {shape} on {env.device} the result was made with")


def read(env, env_ids=None, fields=None, out=None):
    """RexBatchEnv.dynamics (documented there)."""
    torch = env._torch
    if env.mark == "arm":
        raise NotImplementedError("dynamics: mark 'arm' (24 degrees of freedom) is not supported")
    names = check_fields(fields)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, "dynamics")
        if out is None:
            out = Dynamics({n: torch.empty(field_shape(n, k), dtype=torch.float32, device=env.device) for n in names})
        elif out is not env.__dict__.get("_dyn_out") or out.fields != names or out.rows != k:
            check_result(out, names, k, env)
            env._dyn_out = out
        _lib.check(env._L.rex_dynamics(env._h, ids.data_ptr() if ids is not None else None, k, ctypes.byref(out.struct), env._stream_ptr()),
                   "rex_dynamics")
    return out
