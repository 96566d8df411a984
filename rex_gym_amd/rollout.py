"""Candidate rollouts of a batch (include/rexsim.h: rex_rollout): for every env K candidate command sequences simulated over T control steps
of `repeat` substeps each, from the env's current state, in one read-only launch on the env's device and stream -- what a sampling planner
(MPPI, CEM), a safety check before an action is applied or the scoring of a policy against its alternatives asks for.  Mark base.

    ro = env.rollout(targets=targets)                      # targets float32 [k, K, T, 12]: motor angle commands (what info['action'] holds)
    state, trajectory, foot_contact, sweeps = ro           # a namedtuple-like result: unpacks in the order of its fields
    ro.trajectory                                          # float32 [k, K, T, 37]: the state's words 0..36 after every control step
    ro.base_pos, ro.joint_angles                           # views of ro.state: [k, K, 3], [k, K, 12] after the last substep
    cost = (ro.trajectory[..., 0:3] - goal).norm(dim=-1).sum(-1)              # the cost and the sampler are the caller's, in torch
    small = env.rollout(targets=targets, fields=("state",))
    env.rollout(targets=targets, fields=("state",), out=small)                # refilled in place: a per-step read allocates nothing

One substep of a row, on its private copy of the state's words 0..36:  the torque -- the step's motor model on (command, q, qd, qd) with the
config's gains or the env's actuator parameters, times the env's motor enable bit as it stands at the call, or tau [k, K, T, 12] as given --;
v_next of contact_solve() under that torque (the env's mass scales, friction and terrain field of its current episode);  the step's
integrator: pos += dt lin, q += dt qd, the quaternion turned by exp(dt w / 2) and normalised.  The command of control step t holds for its
`repeat` substeps; the torque is drawn anew in each.

Not advanced: the overheat counters and the motor mask, controller and gait words, step and episode counters (no reset, no done), sensor
noise.  The env's state is never written.

From given states, under base pushes, in other bodies (rex_rollout_from; each input is per row, any may be left out):

    nxt = env.rollout(targets=targets[:, :, 2:], init_state=ro.state)          # continue where `ro` stopped: bit for bit the unsplit call
    env.rollout(targets=targets, base_wrench=w)                                # w [k, K, T, 6]: world force at the base origin, N, and moment, N m
    env.rollout(targets=targets, body=b)                                       # b [k, K, 3]: base mass scale, leg mass scale, toe friction

init_state [k, K, 37] (or [k, 37], the same for every candidate) is taken as given -- not normalised, not checked: a bad row yields garbage
in that row only.  The wrench of control step t holds over its substeps and enters the free velocity, v* = v + dt M^-1 (S^T tau + w - h - d).
Everything else a row reads -- terrain field, actuator parameters, motor enable bits -- stays its env's at the call."""
import ctypes

from . import _lib, contact, readout

WORDS = 37                                                 # words 0..36 of the state: pos 0:3, quat 3:7, lin 7:10, ang 10:13, q 13:25, qd 25:37
MAX_SUBSTEPS = 4096
# name -> (trailing shape after (k, K) as a function of T, dtype name)
FIELDS = {"state": (lambda T: (WORDS,), "float32"), "trajectory": (lambda T: (T, WORDS), "float32"), "foot_contact": (lambda T: (T, 4), "uint8"),
          "sweeps": (lambda T: (), "int32")}
assert list(FIELDS) == [f[0] for f in _lib.RexRolloutOut._fields_]


def field_shape(name, k, K, T):
    return (k, K) + FIELDS[name][0](T)


class Rollout(readout.Result):
    """The result of RexBatchEnv.rollout: one tensor attribute per computed field (the others are None), `fields` their names, `struct` the
    RexRolloutOut the launch was given, `rows`, `candidates`, `steps` the shape.  It unpacks and indexes like the namedtuple (state, trajectory,
    foot_contact, sweeps), with None for a field that was not asked for."""
    WHO, FIELDS, STRUCT = "rollout", FIELDS, _lib.RexRolloutOut
    _fields = tuple(FIELDS)

    def __init__(self, tensors, candidates=None, steps=None):
        super().__init__(tensors)
        first = next(iter(tensors.values()))
        self.candidates = int(first.shape[1]) if candidates is None else candidates
        self.steps = steps

    def _astuple(self):
        return tuple(getattr(self, n) for n in self._fields)

    def __iter__(self):
        return iter(self._astuple())

    def __len__(self):
        return len(self._fields)

    def __getitem__(self, i):
        return self._astuple()[i]

    @classmethod
    def dtype_of(cls, name):
        return FIELDS[name][1]

    def _words(self, lo, hi, what):
        if self.state is None:
            raise AttributeError(f"{what} needs the field state")
        return self.state[..., lo:hi]

    base_pos = property(lambda self: self._words(0, 3, "base_pos"), doc="[k, K, 3] after the last substep")
    base_quat = property(lambda self: self._words(3, 7, "base_quat"), doc="[k, K, 4] x y z w")
    base_linvel = property(lambda self: self._words(7, 10, "base_linvel"), doc="[k, K, 3] world")
    base_angvel = property(lambda self: self._words(10, 13, "base_angvel"), doc="[k, K, 3] world")
    joint_angles = property(lambda self: self._words(13, 25, "joint_angles"), doc="[k, K, 12] motor order")
    joint_rates = property(lambda self: self._words(25, 37, "joint_rates"), doc="[k, K, 12] motor order")


def check_fields(fields):
    """fields of RexBatchEnv.rollout -> their names in the order of FIELDS"""
    return readout.check_fields(FIELDS, "rollout", fields)


def check_repeat(repeat, steps, action_repeat):
    """repeat -> RexRolloutIn's (None: 0, the config's action_repeat); steps x repeat is held to MAX_SUBSTEPS"""
    if repeat is not None and not (isinstance(repeat, int) and not isinstance(repeat, bool) and repeat >= 1):
        raise ValueError(f"rollout: repeat must be an int >= 1, got {repeat!r}")
    if steps * (action_repeat if repeat is None else repeat) > MAX_SUBSTEPS:
        raise ValueError(f"rollout: {steps} control steps x {action_repeat if repeat is None else repeat} substeps: at most {MAX_SUBSTEPS} substeps")
    return 0 if repeat is None else repeat


def check_settings(dt, iterations, residual_threshold):
    """the solver settings -> (dt, iterations, residual_threshold) of RexRolloutIn, as contact_solve()'s"""
    try:
        return contact.check_settings(dt, iterations, residual_threshold)
    except ValueError as e:
        raise ValueError(str(e).replace("contact_solve:", "rollout:", 1)) from None


def check_commands(env, targets, tau, k):
    """exactly one of targets and tau, float32 on the env's device, contiguous [k, K, T, 12] -> (the tensor, K, T)"""
    torch, who = env._torch, "rollout"
    if (targets is None) == (tau is None):
        raise ValueError(f"{who}: give exactly one of targets and tau")
    name, t = ("targets", targets) if tau is None else ("tau", tau)
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == env.device):
        raise ValueError(f"{who}: {name} must be a float32 tensor on {env.device}")
    if t.dim() != 4 or t.shape[0] != k or t.shape[1] < 1 or t.shape[2] < 1 or t.shape[3] != 12 or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous with shape ({k}, K, T, 12), K >= 1 and T >= 1, got {tuple(t.shape)}")
    K, T = int(t.shape[1]), int(t.shape[2])
    if k * K * T * WORDS >= 2 ** 31:
        raise ValueError(f"{who}: {k} rows x {K} candidates x {T} steps x {WORDS} words must stay below 2^31")
    return t, K, T


def check_from(env, init_state, base_wrench, body, k, K, T):
    """the per-row inputs of rex_rollout_from, each None or float32 on the env's device, contiguous: init_state [k, K, 37] (or [k, 37], the
    same for every candidate), base_wrench [k, K, T, 6], body [k, K, 3] -> the three tensors as the launch reads them (None stays None)"""
    torch, who = env._torch, "rollout"
    shapes = {"init_state": (k, K, WORDS), "base_wrench": (k, K, T, 6), "body": (k, K, 3)}
    given = {"init_state": init_state, "base_wrench": base_wrench, "body": body}
    for name, t in given.items():
        if t is None:
            continue
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == env.device):
            raise ValueError(f"{who}: {name} must be a float32 tensor on {env.device}")
        either = " or (%d, %d)" % (k, WORDS) if name == "init_state" else ""
        if not ((tuple(t.shape) == shapes[name] or (name == "init_state" and tuple(t.shape) == (k, WORDS))) and t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be contiguous with shape {shapes[name]}{either}, got {tuple(t.shape)}")
    if init_state is not None and init_state.dim() == 2:
        given["init_state"] = init_state[:, None, :].expand(k, K, WORDS).contiguous()
    return given["init_state"], given["base_wrench"], given["body"]


def check_result(out, names, k, K, T, env):
    """a result handed back through out=: its class and fields, then each tensor's shape, dtype, device and identity"""
    torch, who = env._torch, "rollout"
    if not isinstance(out, Rollout) or out.fields != names:
        raise ValueError(f"{who}: out must be a result of {who}() with the fields {names}")
    for n in names:
        t = getattr(out, n)
        shape, dtype = field_shape(n, k, K, T), FIELDS[n][1]
        if not (isinstance(t, torch.Tensor) and t.dtype == getattr(torch, dtype) and t.device == env.device and tuple(t.shape) == shape
                and t.is_contiguous() and t.data_ptr() == getattr(out.struct, n)):
            raise ValueError(f"{who}: out.{n} must be the contiguous {dtype} tensor of shape {shape} on {env.device} the result was made with")


def result(env, out, names, k, K, T):
    """out=None: a new result of empty tensors.  Else the caller's, checked unless it is the one checked last on this env with the same
    fields and shape -- a per-step read with out= allocates and validates nothing."""
    torch = env._torch
    if out is None:
        return Rollout({n: torch.empty(field_shape(n, k, K, T), dtype=getattr(torch, FIELDS[n][1]), device=env.device) for n in names}, K, T)
    if out is not env.__dict__.get("_rollout_out") or out.fields != names or (out.rows, out.candidates, out.steps) != (k, K, T):
        check_result(out, names, k, K, T, env)
        out.candidates, out.steps = K, T
        env._rollout_out = out
    return out


def run(env, targets=None, tau=None, repeat=None, env_ids=None, fields=None, out=None, dt=None, iterations=None, residual_threshold=None,
        init_state=None, base_wrench=None, body=None):
    """RexBatchEnv.rollout (documented there).  With init_state, base_wrench and body all None the call is rex_rollout, else rex_rollout_from."""
    who = "rollout"
    readout.not_arm(env, who)
    if env.config.on_rack:
        raise ValueError(f"{who}: an on_rack env holds its base with an anchor the rollout leaves out")
    if env.config.body_contacts:
        raise ValueError(f"{who}: an env with body_contacts solves link-box rows the rollout leaves out")
    if env.config.pd_latency > 0 or env.config.control_latency > 0:
        raise ValueError(f"{who}: an env with the latency model on draws its torques from an observation ring the rollout does not restate")
    names = check_fields(fields)
    settings = check_settings(dt, iterations, residual_threshold)
    with env._on_stream():
        ids, k = env._row_ids(env_ids, who)
        commands, K, T = check_commands(env, targets, tau, k)
        repeat = check_repeat(repeat, T, int(env.config.action_repeat))
        start = check_from(env, init_state, base_wrench, body, k, K, T)
        out = result(env, out, names, k, K, T)
        inp = _lib.RexRolloutIn(readout.ptr(targets), readout.ptr(tau), K, T, repeat, settings[0], settings[1], settings[2])
        if all(t is None for t in start):
            _lib.check(env._L.rex_rollout(env._h, readout.ptr(ids), k, ctypes.byref(inp), ctypes.byref(out.struct), env._stream_ptr()), "rex_rollout")
        else:
            src = _lib.RexRolloutFrom(*(readout.ptr(t) for t in start))
            _lib.check(env._L.rex_rollout_from(env._h, readout.ptr(ids), k, ctypes.byref(inp), ctypes.byref(src), ctypes.byref(out.struct),
                                               env._stream_ptr()), "rex_rollout_from")
    return out
