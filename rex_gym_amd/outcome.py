"""The step's epilogue as a readout (include/rexsim.h: rex_outcome): what env.step() would SAY of a row whose control step ended in a
given state -- reward, done and observation -- without stepping anything.  Mark base, single-task envs.

    oc = env.outcome()                                     # the env's own state and controller words; no torques: the energy term is left out
    oc.reward, oc.done, oc.obs                             # [k], [k] uint8, [k, obs_dim]
    oc = env.outcome(state, ctrl, motor_torque)            # [k, K, 37], [k, K, 8], [k, K, 12] -> [k, K], [k, K], [k, K, obs_dim]
    ro = env.rollout_actions(acts, fields=("trajectory", "ctrl_trajectory", "reward", "done", "obs", "motor_torque"))
    env.outcome(ro.trajectory[t], ro.ctrl_trajectory[t], ro.motor_torque[t])      # bit for bit ro.reward[t], ro.done[t], ro.obs[t]

state: the words 0..36 AFTER the control step; ctrl: the controller words 37..44 after it, as env.command's second result and the state
block hold them (target already |target|, steps already + 1; the done flag in them is ignored); motor_torque: the OBSERVED motor torques
of the step's last substep (rex_motor_torque_params' second result, rollout_actions' motor_torque) -- the reward's energy term is
-|sum tau x qd| x dt and cannot be recovered from the states.  The kernel calls the step kernels' own functions; sensor noise is not
drawn; there is no reset: on an auto_reset env `obs` is the terminal observation, which env.step never returns; nothing is written."""
import ctypes

from . import _lib, readout, rollout_actions as ra

WORDS, CTRL = ra.WORDS, ra.CTRL
# name -> (trailing shape after (k[, K]) with None for obs_dim, dtype name)
FIELDS = {"reward": ((), "float32"), "done": ((), "uint8"), "obs": ((None,), "float32")}
assert list(FIELDS) == [f[0] for f in _lib.RexOutcomeOut._fields_]


def tail(name, env):
    return tuple(env.obs_dim if d is None else d for d in FIELDS[name][0])


class Outcome(readout.Result):
    """The result of RexBatchEnv.outcome: `reward`, `done` (uint8 0 / 1), `obs` -- a tensor per computed field, None for the others --,
    `fields` their names, `struct` the RexOutcomeOut the launch is given, `rows` k and `candidates` K (None: the inputs were per env and
    the tensors carry no candidate axis)."""
    WHO, FIELDS, STRUCT = "outcome", FIELDS, _lib.RexOutcomeOut

    def __init__(self, tensors, candidates=None):
        super().__init__(tensors)
        self.candidates = candidates

    @classmethod
    def dtype_of(cls, name):
        return FIELDS[name][1]


def lead_shape(k, K):
    return (k,) if K is None else (k, K)


def check_input(env, t, k, K, width, who, name):
    """one of state / ctrl / motor_torque: None, or a contiguous float32 tensor on the env's device, [k, width] when K is None, else
    [k, K, width] or [k, width] for every candidate alike"""
    if t is None:
        return None
    if K is None:
        return ra.check_tensor(env, t, (k, width), who, name)
    return ra.check_rows(env, t, k, K, width, who, name)


def candidates_of(env, inputs):
    """K of the call: the middle axis of the first three-dimensional input; None when every given input is per env"""
    torch = env._torch
    for t in inputs:
        if isinstance(t, torch.Tensor) and t.dim() == 3:
            return int(t.shape[1])
    return None


def run(env, state=None, ctrl=None, motor_torque=None, env_ids=None, fields=None, out=None):
    """RexBatchEnv.outcome (documented there)"""
    who, torch = "outcome", env._torch
    ra.check_sim(env, who, physics=False)
    names = readout.check_fields(FIELDS, who, fields)
    with env._on_stream():
        ids, k = ra.row_ids(env, env_ids, who)
        K = candidates_of(env, (state, ctrl, motor_torque))
        if K is not None and (K < 1 or k * K * WORDS >= 2 ** 31):
            raise ValueError(f"{who}: {k} rows x {K} candidates: at least one candidate, and rows x candidates x {WORDS} below 2^31")
        state = check_input(env, state, k, K, WORDS, who, "state")
        ctrl = check_input(env, ctrl, k, K, CTRL, who, "ctrl")
        motor_torque = check_input(env, motor_torque, k, K, 12, who, "motor_torque")
        lead = lead_shape(k, K)
        if out is None:
            out = Outcome({n: torch.empty(lead + tail(n, env), dtype=getattr(torch, FIELDS[n][1]), device=env.device) for n in names}, K)
        elif out is not env.__dict__.get("_outcome_out") or out.fields != names or (out.rows, out.candidates) != (k, K):
            if not isinstance(out, Outcome) or out.fields != names:
                raise ValueError(f"{who}: out must be a result of {who}() with the fields {names}")
            for n in names:
                t, shape, dtype = getattr(out, n), lead + tail(n, env), FIELDS[n][1]
                if not (isinstance(t, torch.Tensor) and t.dtype == getattr(torch, dtype) and t.device == env.device and tuple(t.shape) == shape
                        and t.is_contiguous() and t.data_ptr() == getattr(out.struct, n)):
                    raise ValueError(f"{who}: out.{n} must be the contiguous {dtype} tensor of shape {shape} on {env.device} the result was made with")
            out.candidates = K
            env._outcome_out = out
        _lib.check(env._L.rex_outcome(env._h, readout.ptr(ids), k, K or 1, readout.ptr(state), readout.ptr(ctrl), readout.ptr(motor_torque),
                                      ctypes.byref(out.struct), env._stream_ptr()), "rex_outcome")
    return out
