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
[k, 4, 2, 3, 18] as (leg, end, world axis, dof): leg order front_left, front_right, rear_left, rear_right.

The same equation solved on the device, M never written out (rex_dynamics_solve, rex_forward_dynamics, rex_apply_impulse):

    x = env.dynamics_solve(rhs)                          # M^-1 rhs, rhs [k, 18] or [k, K, 18]
    vdot = env.forward_dynamics(tau=tau, toe_forces=f)   # [k, 18]
    dv = env.push(base_impulse=p, env_ids=ids)           # dv = M^-1 impulse, added to the envs' velocities in the state"""
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


# ---------------------------------------------------------------- solves with the mass matrix (include/rexsim.h: rex_dynamics_solve, rex_forward_dynamics,
# rex_apply_impulse): M stays in the kernel's registers
NDOF = 18
# argument name -> (member of RexDynamicsLoad, trailing shape after the row count)
LOAD = {"joint": ("joint", (12,)), "toe": ("toe", (4, 2, 3)), "base": ("base", (6,))}


def _not_arm(env, who):
    if env.mark == "arm":
        raise NotImplementedError(f"{who}: mark 'arm' (24 degrees of freedom) is not supported")


def _load_tensor(env, t, k, shape, who, name):
    """one member of a load: a contiguous float32 tensor on the env's device, [k, *shape] or [*shape] (the same for every row)"""
    torch = env._torch
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == env.device):
        raise ValueError(f"{who}: {name} must be a float32 tensor on {env.device}")
    if tuple(t.shape) == shape:
        t = t.expand((k,) + shape).contiguous()
    if tuple(t.shape) != (k,) + shape or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous with shape {(k,) + shape} or {shape}, got {tuple(t.shape)}")
    return t


def _load(env, k, who, **members):
    """-> (RexDynamicsLoad, the tensors it points to) of the members that are not None; none at all raises"""
    if all(t is None for t in members.values()):
        raise ValueError(f"{who}: give at least one of {tuple(members)}")
    kept, ptrs = [], {}
    for (name, t), (member, shape) in zip(members.items(), LOAD.values()):
        if t is not None:
            kept.append(_load_tensor(env, t, k, shape, who, name))
            ptrs[member] = kept[-1].data_ptr()
    return _lib.RexDynamicsLoad(**ptrs), kept


def _out(env, out, shape, who):
    torch = env._torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=env.device)
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == env.device and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor of shape {shape} on {env.device}")
    return out


def solve(env, rhs, env_ids=None, out=None):
    """RexBatchEnv.dynamics_solve (documented there)."""
    torch, who = env._torch, "dynamics_solve"
    _not_arm(env, who)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        if not (isinstance(rhs, torch.Tensor) and rhs.dtype == torch.float32 and rhs.device == env.device and rhs.is_contiguous()
                and rhs.dim() in (2, 3) and rhs.shape[0] == k and rhs.shape[-1] == NDOF and rhs.shape[1] >= 1):
            raise ValueError(f"{who}: rhs must be a contiguous float32 tensor of shape [{k}, 18] or [{k}, K, 18] on {env.device}")
        K = 1 if rhs.dim() == 2 else int(rhs.shape[1])
        if k * K * NDOF >= 2 ** 31:
            raise ValueError(f"{who}: k * K * 18 must stay below 2^31")
        out = _out(env, out, tuple(rhs.shape), who)
        if out.data_ptr() != rhs.data_ptr() and out.data_ptr() < rhs.data_ptr() + rhs.numel() * 4 and rhs.data_ptr() < out.data_ptr() + out.numel() * 4:
            raise ValueError(f"{who}: out overlaps rhs in part (out=rhs solves in place)")
        _lib.check(env._L.rex_dynamics_solve(env._h, ids.data_ptr() if ids is not None else None, k, K, rhs.data_ptr(), out.data_ptr(), env._stream_ptr()),
                   "rex_dynamics_solve")
    return out


def forward(env, tau=None, toe_forces=None, base_wrench=None, env_ids=None, out=None):
    """RexBatchEnv.forward_dynamics (documented there)."""
    who = "forward_dynamics"
    _not_arm(env, who)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        load, kept = _load(env, k, who, tau=tau, toe_forces=toe_forces, base_wrench=base_wrench)
        out = _out(env, out, (k, NDOF), who)
        _lib.check(env._L.rex_forward_dynamics(env._h, ids.data_ptr() if ids is not None else None, k, ctypes.byref(load), out.data_ptr(), env._stream_ptr()),
                   "rex_forward_dynamics")
    return out


def push(env, base_impulse=None, toe_impulses=None, joint_impulses=None, env_ids=None, out=None):
    """RexBatchEnv.push (documented there)."""
    import numpy as np
    who = "push"
    _not_arm(env, who)
    if env.config.on_rack:
        raise ValueError(f"{who}: an on_rack env holds its base with an anchor the solve leaves out")
    if env._needs_reset:
        raise RuntimeError(f"{who}: Must reset environment.")
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        if env_ids is not None:
            host = np.asarray(env_ids.cpu() if hasattr(env_ids, "cpu") else env_ids, dtype=np.int64).reshape(-1)
            if np.unique(host).size != host.size:
                raise ValueError(f"{who}: env_ids must be distinct (every row adds to its env's velocity)")
        load, kept = _load(env, k, who, joint_impulses=joint_impulses, toe_impulses=toe_impulses, base_impulse=base_impulse)
        out = _out(env, out, (k, NDOF), who)
        _lib.check(env._L.rex_apply_impulse(env._h, ids.data_ptr() if ids is not None else None, k, ctypes.byref(load), out.data_ptr(), env._stream_ptr()),
                   "rex_apply_impulse")
    return out
