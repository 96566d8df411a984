"""The acceleration level of a batch (include/rexsim.h: rex_contact_space, rex_inverse_dynamics): the contact-space (Delassus) matrix
J M^-1 J^T of the 8 toe points, their drift acceleration Jdot v, their acceleration under no ground force, and the equation of motion
solved for the force -- each in one read-only launch on the env's device and stream; M is never written out.  Mark base.

    cs = env.contact_space(tau=tau)                        # every field
    cs.delassus                                            # float32 [k, 24, 24]: row and column 3 p + c, point p = 2 leg + end, world axis c
    cs.toe_drift, cs.toe_acc_free                          # float32 [k, 4, 2, 3]
    acc = cs.toe_acc_free.view(k, 24) + torch.einsum("kpq,kq->kp", cs.delassus, f.view(k, 24))     # under ground forces f [k, 4, 2, 3]
    small = env.contact_space(fields=("delassus",))
    env.contact_space(fields=("delassus",), out=small)     # refilled in place: a per-step read allocates nothing
    need = env.inverse_dynamics(vdot=vdot, toe_forces=f)   # [k, 18]: need[:, 6:] the joint torques, need[:, :6] the base wrench left over

Conventions of env.dynamics(): v = (base linear velocity, base angular velocity, 12 joint rates), world axes, and
M vdot + bias = S^T tau + sum_p J_p^T f_p + w.  toe_acc = J vdot + toe_drift;  toe_acc_free = J M^-1 (S^T tau + w - bias) + toe_drift.
Like bias, nothing here holds the sim's damping, joint limits, contacts or the on_rack anchor."""
import ctypes

from . import _lib
from . import dynamics as _dyn

# name -> trailing shape after the row count
FIELDS = {"delassus": (24, 24), "toe_drift": (4, 2, 3), "toe_acc_free": (4, 2, 3)}
assert list(FIELDS) == [f[0] for f in _lib.RexContactSpaceOut._fields_]


def field_shape(name, k):
    return (k,) + FIELDS[name]


class ContactSpace:
    """The result of RexBatchEnv.contact_space: one tensor attribute per computed field (the others are None), `fields` their names, and
    `struct` the RexContactSpaceOut the launch was given."""

    def __init__(self, tensors):
        self.fields = tuple(n for n in FIELDS if n in tensors)
        for n in FIELDS:
            setattr(self, n, tensors.get(n))
        self.struct = _lib.RexContactSpaceOut(**{n: t.data_ptr() for n, t in tensors.items()})
        self.rows = int(next(iter(tensors.values())).shape[0])


def check_fields(fields):
    """fields of RexBatchEnv.contact_space -> their names in the order of FIELDS"""
    if fields is None:
        return tuple(FIELDS)
    if isinstance(fields, str):
        fields = (fields,)
    fields = tuple(fields)
    unknown = [f for f in fields if f not in FIELDS]
    if unknown or not fields:
        raise ValueError(f"contact_space: fields must be a non-empty subset of {tuple(FIELDS)}, got {fields}")
    return tuple(n for n in FIELDS if n in fields)


def check_result(out, names, k, env):
    """a result handed back through out=: its fields, shapes, dtypes, device"""
    torch = env._torch
    if not isinstance(out, ContactSpace) or out.fields != names:
        raise ValueError(f"contact_space: out must be a result of contact_space() with the fields {names}")
    for n in names:
        t = getattr(out, n)
        shape = field_shape(n, k)
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == env.device and tuple(t.shape) == shape and t.is_contiguous()
                and t.data_ptr() == getattr(out.struct, n)):
            raise ValueError(f"contact_space: out.{n} must be the contiguous float32 tensor of shape {shape} on {env.device} the result was made with")


def read(env, tau=None, base_wrench=None, fields=None, env_ids=None, out=None):
    """RexBatchEnv.contact_space (documented there)."""
    torch, who = env._torch, "contact_space"
    _dyn._not_arm(env, who)
    names = check_fields(fields)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        if k * 576 >= 2 ** 31:
            raise ValueError(f"{who}: k * 24 * 24 must stay below 2^31")
        tau = None if tau is None else _dyn._load_tensor(env, tau, k, (12,), who, "tau")
        base_wrench = None if base_wrench is None else _dyn._load_tensor(env, base_wrench, k, (6,), who, "base_wrench")
        if out is None:
            out = ContactSpace({n: torch.empty(field_shape(n, k), dtype=torch.float32, device=env.device) for n in names})
        elif out is not env.__dict__.get("_contact_space_out") or out.fields != names or out.rows != k:
            check_result(out, names, k, env)
            env._contact_space_out = out
        _lib.check(env._L.rex_contact_space(env._h, ids.data_ptr() if ids is not None else None, k, tau.data_ptr() if tau is not None else None,
                                            base_wrench.data_ptr() if base_wrench is not None else None, ctypes.byref(out.struct), env._stream_ptr()),
                   "rex_contact_space")
    return out


def inverse(env, vdot=None, tau=None, toe_forces=None, base_wrench=None, env_ids=None, out=None):
    """RexBatchEnv.inverse_dynamics (documented there)."""
    who = "inverse_dynamics"
    _dyn._not_arm(env, who)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        vdot = None if vdot is None else _dyn._load_tensor(env, vdot, k, (_dyn.NDOF,), who, "vdot")
        kept, ptrs = [], {}
        for name, t, (member, shape) in zip(("tau", "toe_forces", "base_wrench"), (tau, toe_forces, base_wrench), _dyn.LOAD.values()):
            if t is not None:
                kept.append(_dyn._load_tensor(env, t, k, shape, who, name))
                ptrs[member] = kept[-1].data_ptr()
        load = _lib.RexDynamicsLoad(**ptrs)
        out = _dyn._out(env, out, (k, _dyn.NDOF), who)
        _lib.check(env._L.rex_inverse_dynamics(env._h, ids.data_ptr() if ids is not None else None, k, vdot.data_ptr() if vdot is not None else None,
                                               ctypes.byref(load), out.data_ptr(), env._stream_ptr()), "rex_inverse_dynamics")
    return out
