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

from . import _lib, readout

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


class Dynamics(readout.Result):
    """The result of RexBatchEnv.dynamics: one tensor attribute per computed field (the others are None), `fields` their names, and
    `struct` the RexDynamicsOut the launch was given."""
    WHO, FIELDS, STRUCT = "dynamics", FIELDS, _lib.RexDynamicsOut

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
    return readout.check_fields(FIELDS, "dynamics", fields)


def check_result(out, names, k, env):
    """a result handed back through out=: its fields, shapes, dtypes, device"""
    readout.check_result(Dynamics, out, names, k, env)


def read(env, env_ids=None, fields=None, out=None):
    """RexBatchEnv.dynamics (documented there)."""
    readout.not_arm(env, "dynamics")
    names = check_fields(fields)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, "dynamics")
        out = readout.result(Dynamics, env, out, names, k)
        _lib.check(env._L.rex_dynamics(env._h, readout.ptr(ids), k, ctypes.byref(out.struct), env._stream_ptr()), "rex_dynamics")
    return out


# ---------------------------------------------------------------- solves with the mass matrix (include/rexsim.h: rex_dynamics_solve, rex_forward_dynamics,
# rex_apply_impulse): M stays in the kernel's registers
NDOF = readout.NDOF


def solve(env, rhs, env_ids=None, out=None):
    """RexBatchEnv.dynamics_solve (documented there)."""
    torch, who = env._torch, "dynamics_solve"
    readout.not_arm(env, who)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        if not (isinstance(rhs, torch.Tensor) and rhs.dtype == torch.float32 and rhs.device == env.device and rhs.is_contiguous()
                and rhs.dim() in (2, 3) and rhs.shape[0] == k and rhs.shape[-1] == NDOF and rhs.shape[1] >= 1):
            raise ValueError(f"{who}: rhs must be a contiguous float32 tensor of shape [{k}, 18] or [{k}, K, 18] on {env.device}")
        K = 1 if rhs.dim() == 2 else int(rhs.shape[1])
        if k * K * NDOF >= 2 ** 31:
            raise ValueError(f"{who}: k * K * 18 must stay below 2^31")
        out = readout.out_tensor(env, out, tuple(rhs.shape), who)
        if out.data_ptr() != rhs.data_ptr() and out.data_ptr() < rhs.data_ptr() + rhs.numel() * 4 and rhs.data_ptr() < out.data_ptr() + out.numel() * 4:
            raise ValueError(f"{who}: out overlaps rhs in part (out=rhs solves in place)")
        _lib.check(env._L.rex_dynamics_solve(env._h, readout.ptr(ids), k, K, rhs.data_ptr(), out.data_ptr(), env._stream_ptr()), "rex_dynamics_solve")
    return out


def forward(env, tau=None, toe_forces=None, base_wrench=None, env_ids=None, out=None):
    """RexBatchEnv.forward_dynamics (documented there)."""
    who = "forward_dynamics"
    readout.not_arm(env, who)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        load, kept = readout.load(env, k, who, tau=tau, toe_forces=toe_forces, base_wrench=base_wrench)
        out = readout.out_tensor(env, out, (k, NDOF), who)
        _lib.check(env._L.rex_forward_dynamics(env._h, readout.ptr(ids), k, ctypes.byref(load), out.data_ptr(), env._stream_ptr()), "rex_forward_dynamics")
    return out


def push(env, base_impulse=None, toe_impulses=None, joint_impulses=None, env_ids=None, out=None):
    """RexBatchEnv.push (documented there)."""
    import numpy as np
    who = "push"
    readout.not_arm(env, who)
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
        load, kept = readout.load(env, k, who, joint_impulses=joint_impulses, toe_impulses=toe_impulses, base_impulse=base_impulse)
        out = readout.out_tensor(env, out, (k, NDOF), who)
        _lib.check(env._L.rex_apply_impulse(env._h, readout.ptr(ids), k, ctypes.byref(load), out.data_ptr(), env._stream_ptr()), "rex_apply_impulse")
    return out
