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

from . import _lib, readout

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


class Kinematics(readout.Result):
    """The result of RexBatchEnv.kinematics: one tensor attribute per computed field (the others are None), `fields` their names,
    and `struct` the RexKinematicsOut the launch was given."""
    WHO, FIELDS, STRUCT, DTYPE_SHOWN = "kinematics", FIELDS, _lib.RexKinematicsOut, "torch.%s"

    @classmethod
    def shape_of(cls, name, k, env):
        return field_shape(name, k, env.num_bodies)

    @classmethod
    def dtype_of(cls, name):
        return "uint8" if FIELDS[name][1] else "float32"

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
    return readout.check_fields(FIELDS, "kinematics", fields)


def check_result(out, names, k, env):
    """a result handed back through out=: its fields, shapes, dtypes, device"""
    readout.check_result(Kinematics, out, names, k, env)


def read(env, env_ids=None, fields=None, out=None):
    """RexBatchEnv.kinematics (documented there)."""
    names = check_fields(fields)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, "kinematics")
        out = readout.result(Kinematics, env, out, names, k)
        _lib.check(env._L.rex_kinematics(env._h, readout.ptr(ids), k, ctypes.byref(out.struct), env._stream_ptr()), "rex_kinematics")
    return out
