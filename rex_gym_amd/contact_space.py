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

from . import _lib, readout

# name -> trailing shape after the row count
FIELDS = {"delassus": (24, 24), "toe_drift": (4, 2, 3), "toe_acc_free": (4, 2, 3)}
assert list(FIELDS) == [f[0] for f in _lib.RexContactSpaceOut._fields_]


def field_shape(name, k):
    return (k,) + FIELDS[name]


class ContactSpace(readout.Result):
    """The result of RexBatchEnv.contact_space: one tensor attribute per computed field (the others are None), `fields` their names, and
    `struct` the RexContactSpaceOut the launch was given."""
    WHO, FIELDS, STRUCT = "contact_space", FIELDS, _lib.RexContactSpaceOut


def check_fields(fields):
    """fields of RexBatchEnv.contact_space -> their names in the order of FIELDS"""
    return readout.check_fields(FIELDS, "contact_space", fields)


def check_result(out, names, k, env):
    """a result handed back through out=: its fields, shapes, dtypes, device"""
    readout.check_result(ContactSpace, out, names, k, env)


def read(env, tau=None, base_wrench=None, fields=None, env_ids=None, out=None):
    """RexBatchEnv.contact_space (documented there)."""
    who = "contact_space"
    readout.not_arm(env, who)
    names = check_fields(fields)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        if k * 576 >= 2 ** 31:
            raise ValueError(f"{who}: k * 24 * 24 must stay below 2^31")
        tau = None if tau is None else readout.load_tensor(env, tau, k, (12,), who, "tau")
        base_wrench = None if base_wrench is None else readout.load_tensor(env, base_wrench, k, (6,), who, "base_wrench")
        out = readout.result(ContactSpace, env, out, names, k)
        _lib.check(env._L.rex_contact_space(env._h, readout.ptr(ids), k, readout.ptr(tau), readout.ptr(base_wrench), ctypes.byref(out.struct),
                                            env._stream_ptr()), "rex_contact_space")
    return out


def inverse(env, vdot=None, tau=None, toe_forces=None, base_wrench=None, env_ids=None, out=None):
    """RexBatchEnv.inverse_dynamics (documented there)."""
    who = "inverse_dynamics"
    readout.not_arm(env, who)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        vdot = None if vdot is None else readout.load_tensor(env, vdot, k, (readout.NDOF,), who, "vdot")
        load, kept = readout.load(env, k, who, allow_empty=True, tau=tau, toe_forces=toe_forces, base_wrench=base_wrench)
        out = readout.out_tensor(env, out, (k, readout.NDOF), who)
        _lib.check(env._L.rex_inverse_dynamics(env._h, readout.ptr(ids), k, readout.ptr(vdot), ctypes.byref(load), out.data_ptr(), env._stream_ptr()),
                   "rex_inverse_dynamics")
    return out
