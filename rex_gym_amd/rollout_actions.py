"""The env's controller as a readout, and rollouts in the env's own action space (include/rexsim.h: rex_command, rex_rollout_actions): what
shielding a policy action, sampling in 2 dimensions instead of 12 x T and scoring a policy against alternatives ask for.  Mark base,
single-task envs.

    targets, ctrl = env.command(actions)                   # actions [k, K, A] (or [k, A]): ONE control step of the env's controller per row --
                                                           # targets [k, K, 12] what info['action'] of env.step would hold, ctrl [k, K, 8] the
                                                           # controller words 37..44 as the step would store them (done = 0)
    ro = env.rollout_actions(actions)                      # actions [T, k, K, A], TIME-MAJOR like step_segment: T control steps per row
    ro.state, ro.ctrl                                      # [k, K, 37], [k, K, 8] after the last step
    ro.trajectory, ro.ctrl_trajectory, ro.targets          # [T, k, K, 37], [T, k, K, 8], [T, k, K, 12]
    ro.foot_contact, ro.sweeps                             # [T, k, K, 4] uint8, [T, k, K] int32 per control step
    ro.flags, ro.steps                                     # int32 views of ro.ctrl: the REX_F_* bits and the step counter
    nxt = env.rollout_actions(more, init_state=ro.state, ctrl=ro.ctrl)        # continue where `ro` stopped: bit for bit the unsplit call

The controller is closed-loop through its latches (the goal tests read base x or yaw), so the call is 2 T launches on the env's stream --
per control step rex_command on the row's current (state, ctrl), then the rollout kernel for one control step from the previous state --
with no host sync and no copies between them.  The physics is env.rollout's kernel, the controller the step kernels' own functions.
The controller's clock is the env's (action_repeat x dt of the config) whatever `repeat` and `dt` the physics is given.

    ro = env.rollout_actions(actions, fields=("state", "ctrl", "reward", "done", "obs", "motor_torque"))      # the forked env: what the env
    ro.reward, ro.done, ro.obs, ro.motor_torque            # would SAY per control step -- [T, k, K], [T, k, K] uint8, [T, k, K, obs_dim] -- and
                                                           # [T, k, K, 12] the observed motor torques of each step's last substep; computed
                                                           # only when named (rex_rollout_actions_outcome: the same 2 T launches)
    alive = 1 - (ro.done.cumsum(0) - ro.done).clamp(max=1) # rows run on after done: mask with the running OR of done --
    disc = gamma ** torch.arange(T, device=ro.reward.device)[:, None, None]
    ret = (ro.reward * alive * disc).sum(0)                # -- a discounted return per candidate, [k, K]

Not advanced: the overheat counters and the motor mask, resets, episode counters, sensor noise (the turn goal test sees the row's true
yaw).  The env's state is never written."""
import ctypes

import numpy as np

from . import _lib, readout, rollout

WORDS = rollout.WORDS
CTRL = 8                                                   # words 37..44: phi, last step, alpha, target, end step, aux, flags, steps
CTRL_FLAGS, CTRL_STEPS = 6, 7
# name -> (time-major, trailing shape after ([T,] k, K), dtype name)
FIELDS = {"state": (False, (WORDS,), "float32"), "trajectory": (True, (WORDS,), "float32"), "foot_contact": (True, (4,), "uint8"),
          "sweeps": (True, (), "int32"), "ctrl": (False, (CTRL,), "float32"), "ctrl_trajectory": (True, (CTRL,), "float32"),
          "targets": (True, (12,), "float32")}
assert list(FIELDS) == [f[0] for f in _lib.RexRolloutActionsOut._fields_]
# the step's epilogue per control step (rex_rollout_actions_outcome): computed only when named in fields=; None: the env's obs_dim
OUTCOME_FIELDS = {"reward": (True, (), "float32"), "done": (True, (), "uint8"), "obs": (True, (None,), "float32"), "motor_torque": (True, (12,), "float32")}
assert list(OUTCOME_FIELDS) == [f[0] for f in _lib.RexRolloutActionsOutcome._fields_]
ALL_FIELDS = {**FIELDS, **OUTCOME_FIELDS}


def field_shape(name, k, K, T, obs_dim=None):
    major, tail, _ = ALL_FIELDS[name]
    return ((T,) if major else ()) + (k, K) + tuple(obs_dim if d is None else d for d in tail)


def workspace_floats(k, K):
    """rex_rollout_actions_workspace_bytes(k, K) in float32 elements: per row the state ping-pong, the ctrl ping-pong, one step of targets"""
    return k * K * (2 * WORDS + 2 * CTRL + 12)


class ActionRollout(readout.Result):
    """The result of RexBatchEnv.rollout_actions: one tensor attribute per computed field (the others are None), `fields` their names,
    `struct` the RexRolloutActionsOut the call was given, `rows`, `candidates`, `horizon` the shape (k, K, T).  It unpacks and indexes like
    the namedtuple (state, trajectory, foot_contact, sweeps, ctrl, ctrl_trajectory, targets), with None for a field that was not asked for."""
    WHO, FIELDS, STRUCT = "rollout_actions", FIELDS, _lib.RexRolloutActionsOut
    _fields = tuple(FIELDS)

    def __init__(self, tensors, rows, candidates, horizon):
        super().__init__(tensors)
        self.rows, self.candidates, self.horizon = rows, candidates, horizon

    def _astuple(self):
        return tuple(getattr(self, n) for n in self._fields)

    def __iter__(self):
        return iter(self._astuple())

    def __len__(self):
        return len(self._fields)

    def __getitem__(self, i):
        return self._astuple()[i]

    def _words(self, lo, hi, what):
        if self.state is None:
            raise AttributeError(f"{what} needs the field state")
        return self.state[..., lo:hi]

    def _ctrl_word(self, w, what):
        if self.ctrl is None:
            raise AttributeError(f"{what} needs the field ctrl")
        return as_int32(self.ctrl)[..., w]

    base_pos = property(lambda self: self._words(0, 3, "base_pos"), doc="[k, K, 3] after the last substep")
    base_quat = property(lambda self: self._words(3, 7, "base_quat"), doc="[k, K, 4] x y z w")
    base_linvel = property(lambda self: self._words(7, 10, "base_linvel"), doc="[k, K, 3] world")
    base_angvel = property(lambda self: self._words(10, 13, "base_angvel"), doc="[k, K, 3] world")
    joint_angles = property(lambda self: self._words(13, 25, "joint_angles"), doc="[k, K, 12] motor order")
    joint_rates = property(lambda self: self._words(25, 37, "joint_rates"), doc="[k, K, 12] motor order")
    flags = property(lambda self: self._ctrl_word(CTRL_FLAGS, "flags"), doc="[k, K] int32 view of ctrl: the REX_F_* bits after the last step")
    steps = property(lambda self: self._ctrl_word(CTRL_STEPS, "steps"), doc="[k, K] int32 view of ctrl: env steps of the episode after the last step")


class ActionOutcomeRollout(ActionRollout):
    """The result of a rollout_actions call that names one of reward, done, obs, motor_torque: an ActionRollout -- it unpacks like the same
    seven-tuple, `struct` is the RexRolloutActionsOut of those seven -- with the four fields beside them and `outcome_struct`, the
    RexRolloutActionsOutcome the call was given."""
    FIELDS = ALL_FIELDS

    def __init__(self, tensors, rows, candidates, horizon):
        self.fields = tuple(n for n in ALL_FIELDS if n in tensors)
        for n in ALL_FIELDS:
            setattr(self, n, tensors.get(n))
        self.struct = _lib.RexRolloutActionsOut(**{n: t.data_ptr() for n, t in tensors.items() if n in FIELDS})
        self.outcome_struct = _lib.RexRolloutActionsOutcome(**{n: t.data_ptr() for n, t in tensors.items() if n in OUTCOME_FIELDS})
        self.rows, self.candidates, self.horizon = rows, candidates, horizon

    def pointer(self, name):
        return getattr(self.outcome_struct if name in OUTCOME_FIELDS else self.struct, name)


def as_int32(ctrl):
    """the controller words [..., 8] as their int32 bit patterns (a view): words 1, 4, 6, 7 -- last step, end step, flags, steps -- are ints"""
    import torch
    return ctrl.view(torch.int32)


def check_sim(env, who, physics):
    """what the calls refuse of an env before looking at an argument: mark arm, a mixed batch, the latency model; with the physics also
    on_rack and body_contacts"""
    readout.not_arm(env, who)
    if env.task == "mixed":
        raise ValueError(f"{who}: a mixed batch runs a task per env: single-task envs only")
    if env.config.pd_latency > 0 or env.config.control_latency > 0:
        raise ValueError(f"{who}: an env with the latency model on reads its orientation from an observation ring the readout does not restate")
    if physics and env.config.on_rack:
        raise ValueError(f"{who}: an on_rack env holds its base with an anchor the rollout leaves out")
    if physics and env.config.body_contacts:
        raise ValueError(f"{who}: an env with body_contacts solves link-box rows the rollout leaves out")


def row_ids(env, env_ids, who):
    """env_ids -> (int32 device tensor or None, the number of rows): as render()'s, and no env twice"""
    if env_ids is not None:
        host = np.asarray(env_ids.cpu() if hasattr(env_ids, "cpu") else env_ids, dtype=np.int64).reshape(-1)
        if np.unique(host).size != host.size:
            raise ValueError(f"{who}: env_ids names an env twice")
    return env._row_ids(env_ids, who)


def check_tensor(env, t, shape, who, name, shown=None):
    """a float32 tensor on the env's device, contiguous, of the given shape"""
    torch = env._torch
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == env.device):
        raise ValueError(f"{who}: {name} must be a float32 tensor on {env.device}")
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous with shape {shown or tuple(shape)}, got {tuple(t.shape)}")
    return t


def check_rows(env, t, k, K, width, who, name):
    """a per-row input [k, K, width], or [k, width] for every candidate alike; None stays None"""
    if t is None:
        return None
    torch = env._torch
    if isinstance(t, torch.Tensor) and t.dim() == 2 and tuple(t.shape) == (k, width) and t.dtype == torch.float32 and t.device == env.device:
        return t[:, None, :].expand(k, K, width).contiguous()
    return check_tensor(env, t, (k, K, width), who, name, f"({k}, {K}, {width}) or ({k}, {width})")


def check_actions(env, actions, k, who, time_major):
    """actions: float32 on the env's device, contiguous, [k, K, A] (or [k, A], K = 1) -- with a leading T when time_major -- -> (tensor, K, T)"""
    torch, A = env._torch, env.action_dim
    if not (isinstance(actions, torch.Tensor) and actions.dtype == torch.float32 and actions.device == env.device):
        raise ValueError(f"{who}: actions must be a float32 tensor on {env.device}")
    lead = 1 if time_major else 0
    a = actions
    if a.dim() == lead + 2:
        a = a.unsqueeze(lead + 1)
    want = ("(T, " if time_major else "(") + f"{k}, K, {A})"
    if a.dim() != lead + 3 or a.shape[lead] != k or a.shape[lead + 1] < 1 or a.shape[lead + 2] != A or (time_major and a.shape[0] < 1) or not a.is_contiguous():
        raise ValueError(f"{who}: actions must be contiguous with shape {want}, K >= 1" + (" and T >= 1" if time_major else "") + f", got {tuple(actions.shape)}")
    K, T = int(a.shape[lead + 1]), int(a.shape[0]) if time_major else 1
    if k * K * T * WORDS >= 2 ** 31:
        raise ValueError(f"{who}: {k} rows x {K} candidates x {T} steps x {WORDS} words must stay below 2^31")
    return a, K, T


def command(env, actions, state=None, ctrl=None, env_ids=None, out=None):
    """RexBatchEnv.command (documented there)"""
    who, torch = "command", env._torch
    check_sim(env, who, physics=False)
    with env._on_stream():
        ids, k = row_ids(env, env_ids, who)
        a, K, _ = check_actions(env, actions, k, who, time_major=False)
        state = check_rows(env, state, k, K, WORDS, who, "state")
        ctrl = check_rows(env, ctrl, k, K, CTRL, who, "ctrl")
        if out is None:
            out = (torch.empty((k, K, 12), dtype=torch.float32, device=env.device), torch.empty((k, K, CTRL), dtype=torch.float32, device=env.device))
        else:
            if not (isinstance(out, (tuple, list)) and len(out) == 2):
                raise ValueError(f"{who}: out must be the pair (targets, ctrl) a call returned")
            check_tensor(env, out[0], (k, K, 12), who, "out[0]")
            check_tensor(env, out[1], (k, K, CTRL), who, "out[1]")
        _lib.check(env._L.rex_command(env._h, readout.ptr(ids), k, K, a.data_ptr(), readout.ptr(state), readout.ptr(ctrl), out[0].data_ptr(),
                                      out[1].data_ptr(), env._stream_ptr()), "rex_command")
    return out[0], out[1]


def result(env, out, names, k, K, T):
    """out=None: a new result of empty tensors.  Else the caller's, checked unless it is the one checked last on this env with the same
    fields and shape -- a per-step read with out= allocates and validates nothing."""
    torch, who = env._torch, "rollout_actions"
    cls = ActionOutcomeRollout if any(n in OUTCOME_FIELDS for n in names) else ActionRollout
    shape_of = lambda n: field_shape(n, k, K, T, getattr(env, "obs_dim", None))
    if out is None:
        return cls({n: torch.empty(shape_of(n), dtype=getattr(torch, ALL_FIELDS[n][2]), device=env.device) for n in names}, k, K, T)
    if out is not env.__dict__.get("_rollout_actions_out") or out.fields != names or (out.rows, out.candidates, out.horizon) != (k, K, T):
        if type(out) is not cls or out.fields != names:
            raise ValueError(f"{who}: out must be a result of {who}() with the fields {names}")
        for n in names:
            t, shape, dtype = getattr(out, n), shape_of(n), ALL_FIELDS[n][2]
            if not (isinstance(t, torch.Tensor) and t.dtype == getattr(torch, dtype) and t.device == env.device and tuple(t.shape) == shape
                    and t.is_contiguous() and t.data_ptr() == (out.pointer(n) if cls is ActionOutcomeRollout else getattr(out.struct, n))):
                raise ValueError(f"{who}: out.{n} must be the contiguous {dtype} tensor of shape {shape} on {env.device} the result was made with")
        out.rows, out.candidates, out.horizon = k, K, T
        env._rollout_actions_out = out
    return out


def workspace(env, k, K):
    """the call's workspace: allocated once per shape and kept on the env"""
    kept = env.__dict__.get("_rollout_actions_ws")
    if kept is None or kept[0] != (k, K):
        kept = ((k, K), env._torch.empty(workspace_floats(k, K), dtype=env._torch.float32, device=env.device))
        env._rollout_actions_ws = kept
    return kept[1]


def run(env, actions, repeat=None, init_state=None, ctrl=None, base_wrench=None, body=None, env_ids=None, fields=None, out=None, dt=None,
        iterations=None, residual_threshold=None):
    """RexBatchEnv.rollout_actions (documented there)"""
    who = "rollout_actions"
    check_sim(env, who, physics=True)
    # fields=None: the seven of rex_rollout_actions, as ever; the step's epilogue is computed only where it is named
    names = readout.check_fields(FIELDS if fields is None else ALL_FIELDS, who, fields)
    try:
        settings = rollout.check_settings(dt, iterations, residual_threshold)
    except ValueError as e:
        raise ValueError(str(e).replace("rollout:", who + ":", 1)) from None
    with env._on_stream():
        ids, k = row_ids(env, env_ids, who)
        a, K, T = check_actions(env, actions, k, who, time_major=True)
        try:
            repeat = rollout.check_repeat(repeat, T, int(env.config.action_repeat))
        except ValueError as e:
            raise ValueError(str(e).replace("rollout:", who + ":", 1)) from None
        init_state = check_rows(env, init_state, k, K, WORDS, who, "init_state")
        ctrl = check_rows(env, ctrl, k, K, CTRL, who, "ctrl")
        if base_wrench is not None:
            check_tensor(env, base_wrench, (T, k, K, 6), who, "base_wrench")
        if body is not None:
            check_tensor(env, body, (k, K, 3), who, "body")
        out = result(env, out, names, k, K, T)
        ws = workspace(env, k, K)
        inp = _lib.RexRolloutActionsIn(a.data_ptr(), readout.ptr(ctrl), K, T, repeat, settings[0], settings[1], settings[2])
        src = _lib.RexRolloutFrom(readout.ptr(init_state), readout.ptr(base_wrench), readout.ptr(body))
        if isinstance(out, ActionOutcomeRollout):
            _lib.check(env._L.rex_rollout_actions_outcome(env._h, readout.ptr(ids), k, ctypes.byref(inp), ctypes.byref(src), ctypes.byref(out.struct),
                                                          ctypes.byref(out.outcome_struct), ws.data_ptr(), ws.numel() * 4, env._stream_ptr()),
                       "rex_rollout_actions_outcome")
        else:
            _lib.check(env._L.rex_rollout_actions(env._h, readout.ptr(ids), k, ctypes.byref(inp), ctypes.byref(src), ctypes.byref(out.struct), ws.data_ptr(),
                                                  ws.numel() * 4, env._stream_ptr()), "rex_rollout_actions")
    return out
