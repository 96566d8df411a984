"""What the read-only queries on a batch share on the host (kinematics.py, dynamics.py, contact.py, contact_space.py): the result object
with one tensor per computed field, the checks of `fields=` and of a result handed back through `out=`, and the loads and outputs of the
calls that take plain tensors.  Each query's module binds these to its own table of fields and keeps its public names."""
from . import _lib

NDOF = 18
# member of RexDynamicsLoad -> trailing shape after the row count
LOAD = {"joint": (12,), "toe": (4, 2, 3), "base": (6,)}
assert list(LOAD) == [f[0] for f in _lib.RexDynamicsLoad._fields_]


def ptr(t):
    """the device pointer of an optional tensor (env ids, a load): None, a null pointer, for None"""
    return t.data_ptr() if t is not None else None


def not_arm(env, who):
    if env.mark == "arm":
        raise NotImplementedError(f"{who}: mark 'arm' (24 degrees of freedom) is not supported")


class Result:
    """One tensor attribute per computed field (the others are None), `fields` their names, `struct` the ctypes struct of output
    pointers the launch is given, `rows` the row count.  A query's class sets WHO (the query's name in messages), FIELDS (a dict keyed
    by the field names in the struct's order) and STRUCT, and overrides shape_of / dtype_of where FIELDS holds more than a shape.
    DTYPE_SHOWN is how check_result's message writes a dtype's name."""
    WHO, FIELDS, STRUCT, DTYPE_SHOWN = None, {}, None, "%s"

    def __init__(self, tensors):
        self.fields = tuple(n for n in self.FIELDS if n in tensors)
        for n in self.FIELDS:
            setattr(self, n, tensors.get(n))
        self.struct = self.STRUCT(**{n: t.data_ptr() for n, t in tensors.items()})
        self.rows = int(next(iter(tensors.values())).shape[0])

    @classmethod
    def shape_of(cls, name, k, env):
        return (k,) + cls.FIELDS[name]

    @classmethod
    def dtype_of(cls, name):
        """the name of the field's dtype in torch"""
        return "float32"


def check_fields(FIELDS, who, fields):
    """fields= of a query -> their names in the order of FIELDS"""
    if fields is None:
        return tuple(FIELDS)
    if isinstance(fields, str):
        fields = (fields,)
    fields = tuple(fields)
    unknown = [f for f in fields if f not in FIELDS]
    if unknown or not fields:
        raise ValueError(f"{who}: fields must be a non-empty subset of {tuple(FIELDS)}, got {fields}")
    return tuple(n for n in FIELDS if n in fields)


def check_result(cls, out, names, k, env):
    """a result handed back through out=: its class and fields, then each tensor's shape, dtype, device and identity"""
    torch, who = env._torch, cls.WHO
    if not isinstance(out, cls) or out.fields != names:
        raise ValueError(f"{who}: out must be a result of {who}() with the fields {names}")
    for n in names:
        t = getattr(out, n)
        shape, dtype = cls.shape_of(n, k, env), cls.dtype_of(n)
        if not (isinstance(t, torch.Tensor) and t.dtype == getattr(torch, dtype) and t.device == env.device and tuple(t.shape) == shape
                and t.is_contiguous() and t.data_ptr() == getattr(out.struct, n)):
            raise ValueError(f"{who}: out.{n} must be the contiguous {cls.DTYPE_SHOWN % dtype} tensor of shape {shape} on {env.device} "
                             "the result was made with")


def result(cls, env, out, names, k):
    """out=None: a new result of empty tensors.  Else the caller's, checked unless it is the one checked last for this query on this env
    with the same fields and rows -- a per-step read with out= allocates and validates nothing."""
    torch, slot = env._torch, "_%s_out" % cls.WHO
    if out is None:
        return cls({n: torch.empty(cls.shape_of(n, k, env), dtype=getattr(torch, cls.dtype_of(n)), device=env.device) for n in names})
    if out is not env.__dict__.get(slot) or out.fields != names or out.rows != k:
        check_result(cls, out, names, k, env)
        setattr(env, slot, out)
    return out


def load_tensor(env, t, k, shape, who, name):
    """one member of a load: a contiguous float32 tensor on the env's device, [k, *shape] or [*shape] (the same for every row)"""
    torch = env._torch
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == env.device):
        raise ValueError(f"{who}: {name} must be a float32 tensor on {env.device}")
    if tuple(t.shape) == shape:
        t = t.expand((k,) + shape).contiguous()
    if tuple(t.shape) != (k,) + shape or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous with shape {(k,) + shape} or {shape}, got {tuple(t.shape)}")
    return t


def load(env, k, who, allow_empty=False, **members):
    """members: the caller's names for joint, toe, base in that order -> (RexDynamicsLoad, the tensors it points to) of those that are
    not None; none at all raises unless allow_empty"""
    if not allow_empty and all(t is None for t in members.values()):
        raise ValueError(f"{who}: give at least one of {tuple(members)}")
    kept, ptrs = [], {}
    for (name, t), (member, shape) in zip(members.items(), LOAD.items()):
        if t is not None:
            kept.append(load_tensor(env, t, k, shape, who, name))
            ptrs[member] = kept[-1].data_ptr()
    return _lib.RexDynamicsLoad(**ptrs), kept


def out_tensor(env, out, shape, who):
    """out= of a call that returns one float32 tensor: a new one, or the caller's checked"""
    torch = env._torch
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=env.device)
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == env.device and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor of shape {shape} on {env.device}")
    return out
