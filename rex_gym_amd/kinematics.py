"""Body and foot kinematics of a batch (include/rexsim.h: rex_kinematics): the pose and velocity of every link, the 8 toe contact
candidates of the physics with their distance to the ground, and the base's velocity and the gravity direction in the base frame,
for every env in one launch, on the env's device and stream.

    kin = env.kinematics()                               # every field
    kin.link_pos                                         # float32 [num_envs, NB, 3], body order env.body_names
    kin.foot_clearance, kin.foot_in_reach                # [num_envs, 4]: the nearer end of each toe, and whether either end is in reach
    feet = env.kinematics(fields=("toe_pos", "toe_dist"))
    env.kinematics(fields=("toe_pos", "toe_dist"), out=feet)      # refilled in place: a per-step read allocates nothing

Toe arrays are shaped [k, 4, 2, ...] as (leg, end): leg order front_left, front_right, rear_left, rear_right."""
import ctypes
import os
import re

from . import _lib

# name -> (trailing shape after the row count, with NB for the number of bodies; uint8?)
FIELDS = {"link_pos": (("NB", 3), False), "link_quat": (("NB", 4), False), "link_linvel": (("NB", 3), False), "link_angvel": (("NB", 3), False),
          "toe_pos": ((4, 2, 3), False), "toe_vel": ((4, 2, 3), False), "toe_dist": ((4, 2), False), "toe_normal": ((4, 2, 3), False),
          "toe_in_reach": ((4, 2), True), "base_body": ((9,), False)}
assert list(FIELDS) == [f[0] for f in _lib.RexKinematicsOut._fields_]

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")


def body_names(mark="base"):
    """The link names in body order, from the model tables: the row comments of REX_COM (csrc/rex_model_gen.h), then for mark
    'arm' those of REXA_COM (csrc/rex_arm_model_gen.h)."""
    names = []
    for header, table in (("rex_model_gen.h", "REX_COM"),) + ((("rex_arm_model_gen.h", "REXA_COM"),) if mark == "arm" else ()):
        with open(os.path.join(_CSRC, header)) as f:
            body = re.search(r"%s\[[^=]*=\s*\{(.*?)\n\};" % table, f.read(), re.S).group(1)
        names += re.findall(r"/\*\s*(\w+)\s*\*/", body)
    return tuple(names)


def field_shape(name, k, num_bodies):
    return (k,) + tuple(num_bodies if d == "NB" else d for d in FIELDS[name][0])


class Kinematics:
    """The result of RexBatchEnv.kinematics: one tensor attribute per computed field (the others are None), `fields` their names,
    and `struct` the RexKinematicsOut the launch was given."""

    def __init__(self, tensors):
        self.fields = tuple(n for n in FIELDS if n in tensors)
        for n in FIELDS:
            setattr(self, n, tensors.get(n))
        self.struct = _lib.RexKinematicsOut(**{n: t.data_ptr() for n, t in tensors.items()})
        self.rows = int(next(iter(tensors.values())).shape[0])

    @property
    def foot_clearance(self):
        """[k, 4]: the smaller toe_dist of each foot's two ends"""
        if self.toe_dist is None:
            raise AttributeError("foot_clearance needs the field toe_dist")
        return self.toe_dist.amin(dim=2)

    @property
    def foot_in_reach(self):
        """[k, 4] bool: either end of the foot within contact range of the ground"""
        if self.toe_in_reach is None:
            raise AttributeError("foot_in_reach needs the field toe_in_reach")
        return self.toe_in_reach.any(dim=2)


def check_fields(fields):
    """fields of RexBatchEnv.kinematics -> their names in the order of FIELDS"""
    if fields is None:
        return tuple(FIELDS)
    if isinstance(fields, str):
        fields = (fields,)
    fields = tuple(fields)
    unknown = [f for f in fields if f not in FIELDS]
    if unknown or not fields:
        raise ValueError(f"kinematics: fields must be a non-empty subset of {tuple(FIELDS)}, got {fields}")
    return tuple(n for n in FIELDS if n in fields)


def check_result(out, names, k, env):
    """a result handed back through out=: its fields, shapes, dtypes, device"""
    torch = env._torch
    if not isinstance(out, Kinematics) or out.fields != names:
        raise ValueError(f"kinematics: out must be a result of kinematics() with the fields {names}")
    for n in names:
        t = getattr(out, n)
        dtype = torch.uint8 if FIELDS[n][1] else torch.float32
        shape = field_shape(n, k, env.num_bodies)
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == env.device and tuple(t.shape) == shape and t.is_contiguous()
                and t.data_ptr() == getattr(out.struct, n)):
            raise ValueError(f"kinematics: out.{n} must be the contiguous {dtype} tensor of shape {shape} on {env.device} the result was made with")


def read(env, env_ids=None, fields=None, out=None):
    """RexBatchEnv.kinematics (documented there)."""
    torch = env._torch
    names = check_fields(fields)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, "kinematics")
        if out is None:
            out = Kinematics({n: torch.empty(field_shape(n, k, env.num_bodies), dtype=torch.uint8 if FIELDS[n][1] else torch.float32, device=env.device)
                              for n in names})
        elif out is not env.__dict__.get("_kin_out") or out.fields != names or out.rows != k:
            check_result(out, names, k, env)
            env._kin_out = out
        _lib.check(env._L.rex_kinematics(env._h, ids.data_ptr() if ids is not None else None, k, ctypes.byref(out.struct), env._stream_ptr()),
                   "rex_kinematics")
    return out
