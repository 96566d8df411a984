"""The fused recurrent PPO learner (csrc/rex_learner_rnn.h behind agents/fused_learner.py) on the GPU, against PyTorch autograd.

Yardstick: the rule of tests/test_gpu_fused_learner.py, taken over as it is.  The reference is the same loss by fp64 autograd on the CPU,
err(x) = max|x - x64| / max|x64|.  FLOOR is the largest err the existing fp32 autograd path on the device shows over the case's nine gradient
tensors, measured in the run.  Every gradient tensor is held to 8 x FLOOR; the loss and kl_row to 8 x max(FLOOR, fp32 autograd's own err of
that quantity).  REX_PARITY_JSON=<path> makes the run write every measured error of both paths there
(profiles/fused_recurrent_learner_parity.json is such a run's file).

Shapes: 5 x 37 (an empty, a one-step and a full row; T no multiple of the 64-step tile), 67 x 130 (nine scan workgroups of 8 rows, mixed
lengths inside a group, several groups' partials), 1 x 1 (only the distance from the cutoff is asserted for it, as in the existing test) and
3 x 200 (a long recurrence with fewer rows than a scan workgroup).  F = 200, plus one case each of F = 40 and F = 256."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from rex_gym_amd.agents import PPOAgent, PPOConfig, train
from rex_gym_amd.agents import ppo

import fused_recurrent_cases as rc

pytestmark = pytest.mark.gpu

DIMS = [(4, 2), (16, 4), (22, 4), (4, 1), (4, 8)]
CASES = [(s, o, a, 200) for s in ("r5", "r67", "r1", "r3") for (o, a) in DIMS] + [("r5", 4, 2, 40), ("r67", 16, 4, 256)]
PENALTY, CUTOFF, COEF = rc.PENALTY, rc.CUTOFF, rc.COEF


def _id(case):
    s, o, a, f = case
    return "%s-O%d-A%d" % (s, o, a) + ("" if f == 200 else "-F%d" % f)
_PARITY = {}
_REFS = {}


def _err(x, x64):
    return float((x.detach().double().cpu() - x64).abs().max() / x64.abs().max().clamp_min(1e-300))


def _reference(case):
    """The fp64 yardstick and the fp32 autograd path's errors against it, once per case."""
    if case not in _REFS:
        c = rc.make_case(*case)
        r64 = rc.autograd(c, "cpu", torch.float64)
        kl = r64["kl_row"]
        if case[0] in ("r5", "r67"):     # the discrete branch [kl_r > c] must be exercised on both sides (r3's three long rows all lie above) ...
            assert int((kl > CUTOFF).sum()) >= 1 and int((kl <= CUTOFF).sum()) >= 1, kl
        assert float(((kl - CUTOFF).abs() / CUTOFF).min()) > 1e-3, kl      # ... and decided the same way by every fp32 evaluation
        r32 = rc.autograd(c, "cuda", torch.float32)
        floor = {"policy_grads": [_err(a, b) for a, b in zip(r32["policy_grads"], r64["policy_grads"])]}
        for key in ("policy_loss", "kl_row"):
            floor[key] = _err(r32[key], r64[key])
        _REFS[case] = (c, r64, floor)
    return _REFS[case]


def _learner(c):
    from rex_gym_amd.agents.fused_learner import FusedRecurrentLearner
    g = rc.to(c, "cuda", torch.float32)
    fl = FusedRecurrentLearner(g["net"], c["R"], c["T"], "cuda")
    fl.set_length(g["length"])
    return g, fl


def _run(g, fl, grad=True):
    loss = torch.zeros(1, device="cuda")
    fl.policy_flat.fill_(float("nan"))       # every gradient element must be written
    fl.kl_row.fill_(float("nan"))
    fl.policy_loss(g["observ"], g["action"], g["old_mean"], g["old_logstd"], g["advantage"], PENALTY, CUTOFF, COEF, loss, grad=grad)
    torch.cuda.synchronize()
    return dict(policy_grads=[v.clone() for v in fl.policy_grads], policy_loss=loss.clone(), kl_row=fl.kl_row.clone())


def _flat(res):
    return [res["policy_loss"], res["kl_row"]] + res["policy_grads"]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gradients_loss_and_kl_match_fp64_autograd_within_8x_the_fp32_autograd_floor(case):
    c, r64, floor = _reference(case)
    g, fl = _learner(c)
    res = _run(g, fl)
    report, bad = {}, []
    bound = 8.0 * max(floor["policy_grads"])
    for n, got, want, fl32 in zip(rc.NAMES, res["policy_grads"], r64["policy_grads"], floor["policy_grads"]):
        e = _err(got, want)
        report["policy_grads.%s" % n] = {"fused": e, "autograd_fp32": fl32}
        print("%s policy_grads.%s: fused %.3e, fp32 autograd %.3e, bound %.3e" % (case, n, e, fl32, bound))
        if not e <= bound:
            bad.append((n, e, bound))
    for s in ("policy_loss", "kl_row"):
        e, sbound = _err(res[s], r64[s]), max(bound, 8.0 * floor[s])
        report[s] = {"fused": e, "autograd_fp32": floor[s]}
        print("%s %s: fused %.3e, fp32 autograd %.3e, bound %.3e" % (case, s, e, floor[s], sbound))
        if not e <= sbound:
            bad.append((s, e, sbound))
    _PARITY[_id(case)] = report
    if os.environ.get("REX_PARITY_JSON"):
        with open(os.environ["REX_PARITY_JSON"], "w") as f:
            json.dump({"yardstick": "fp64 autograd (CPU); err = max|x - x64| / max|x64|", "bound": "gradients: 8 x the largest autograd_fp32 err over the nine gradient tensors; loss, kl_row: 8 x max(that, the quantity's own autograd_fp32 err)",
                       "cases": _PARITY}, f, indent=1, sort_keys=True)
    assert not bad, bad


def test_two_calls_give_the_same_bits():
    c, _, _ = _reference(("r67", 4, 2, 200))
    g, fl = _learner(c)
    a, b = _run(g, fl), _run(g, fl)
    for x, y in zip(_flat(a), _flat(b)):
        assert torch.equal(x, y)


def test_padded_slots_are_never_read():
    c, _, _ = _reference(("r67", 16, 4, 200))
    outs = []
    for fill in (0.0, float("nan")):
        g, fl = _learner(c)
        pad = ~ppo._mask(g["length"], c["T"]).bool()
        for k in ("observ", "action", "old_mean", "old_logstd", "advantage"):
            g[k] = g[k].clone()
            g[k][pad] = fill
        outs.append(_run(g, fl))
    for x, y in zip(_flat(outs[0]), _flat(outs[1])):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_forward_only_mode_returns_the_same_loss_and_kl():
    c, _, _ = _reference(("r67", 4, 2, 200))
    g, fl = _learner(c)
    full = _run(g, fl)
    fwd = _run(g, fl, grad=False)
    for k in ("policy_loss", "kl_row"):
        assert torch.equal(full[k], fwd[k]), k
    assert all(bool(torch.isnan(v).all()) for v in fwd["policy_grads"])      # and writes no gradient


def test_unsupported_dims_are_refused_with_a_message_and_without_a_launch():
    from rex_gym_amd import _lib
    from rex_gym_amd.agents.fused_learner import FusedRecurrentLearner, rnn_net_struct
    L = _lib.lib()
    for dims, field in (((5, 37, 5, 2, 200, 100), b"obs_dim 5"), ((5, 37, 4, 3, 200, 100), b"out_dim 3"), ((5, 37, 4, 2, 300, 100), b"hidden1 300"),
                        ((5, 37, 4, 2, 200, 64), b"state 64"), ((0, 37, 4, 2, 200, 100), b"0 rows")):
        assert L.rex_ppo_recurrent_workspace_bytes(*dims) == -1
        assert b"rex_ppo_recurrent_workspace_bytes" in L.rex_last_error() and field in L.rex_last_error()
    net = ppo.RecurrentGaussianPolicy(5, 3, PPOConfig(network="recurrent")).cuda()
    with pytest.raises(ValueError, match="obs_dim 5"):
        FusedRecurrentLearner(net, 5, 37, "cuda")
    n = rnn_net_struct(net.policy_parameters())
    b = _lib.RexPpoBatch()
    b.rows, b.steps = 5, 37
    buf = torch.full((64,), 7.0, device="cuda")
    assert L.rex_ppo_recurrent_policy_loss(ctypes.byref(n), ctypes.byref(b), None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) == -1
    assert b"obs_dim 5" in L.rex_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())                                           # nothing was launched on the outputs
    with pytest.raises(ValueError, match="fused_recurrent"):
        PPOAgent(4, 4, 2, PPOConfig(network="recurrent", learner="fused"), device="cuda")


# ---- end to end: the toy point task of tests/test_gpu_fused_learner.py under the recurrent network ----
class _PointEnv:
    """N points on a line; action moves the point, reward = -|x|; episodes of fixed length."""
    def __init__(self, n, seed=0, device="cuda"):
        self.n, self.g, self.device = n, torch.Generator().manual_seed(seed), device
        self.x = torch.zeros(n, 1, device=device)
    def _obs(self, x):
        return torch.cat([x, torch.zeros((x.shape[0], 3), device=self.device)], 1)
    def reset(self, indices=None):
        if indices is None:
            self.x = (torch.rand((self.n, 1), generator=self.g) * 4 - 2).to(self.device)
            return self._obs(self.x)
        idx = indices.long()
        self.x[idx] = (torch.rand((idx.numel(), 1), generator=self.g) * 4 - 2).to(self.device)
        return self._obs(self.x[idx])
    def step(self, a):
        self.x = self.x + 0.5 * a.clamp(-1, 1)
        return self._obs(self.x), -self.x[:, 0].abs(), torch.zeros(self.n, dtype=torch.bool, device=self.device), {}


def _toy_cfg(learner, **kw):
    return PPOConfig(policy_layers=(200, 100), value_layers=(200, 100), update_every=64, update_epochs_policy=15, update_epochs_value=15,
                     policy_lr=3e-3, value_lr=3e-3, max_length=12, discount=0.9, init_mean_factor=0.1, network="recurrent", learner=learner, **kw)


def test_fused_recurrent_ppo_learns_the_toy_task_and_adapts_its_penalty():
    torch.manual_seed(0)
    n = 64
    env, agent = _PointEnv(n), PPOAgent(n, 4, 1, _toy_cfg("fused_recurrent"), device="cuda", seed=3)
    first, _ = train(env, agent, 12 * 3)
    for _ in range(12):
        last, length = train(env, agent, 12 * 3)
    assert agent.updates >= 30 and length == 12
    assert last > first + 1.0, (first, last)
    kls = [s["kl_change"] for s in agent.log]
    assert all(np.isfinite(k) for k in kls) and max(kls) < 1.0
    pens = [s["penalty"] for s in agent.log]
    assert len(set(pens)) > 1
    assert all(abs(abs(math.log(pens[i + 1] / pens[i]) / math.log(1.5)) - round(abs(math.log(pens[i + 1] / pens[i]) / math.log(1.5)))) < 1e-6
               for i in range(len(pens) - 1))


def test_one_training_from_identical_state_agrees_under_both_learners():
    """8 rows x 40 steps; the tolerance is the existing test's: 1e-3 relative on the statistics of one whole update (15 + 15 Adam steps, each
    amplifying the learners' last-bit differences), and the same penalty decision."""
    n = 8
    cfg = dict(update_every=n, max_length=40)
    agents = {k: PPOAgent(n, 4, 1, PPOConfig(**{**_toy_cfg(k).__dict__, **cfg}), device="cuda", seed=3) for k in ("autograd", "fused_recurrent")}
    torch.manual_seed(0)
    train(_PointEnv(n), agents["autograd"], 39)           # 39 steps of experience: the episodes end at the fortieth, below, in both agents
    a, f = agents["autograd"], agents["fused_recurrent"]
    for dst, src in zip(f.episodes, a.episodes):
        dst.copy_(src)
    f.episode_length.copy_(a.episode_length)
    for name in ("observ_filter", "reward_filter"):
        fa, ff = getattr(a, name), getattr(f, name)
        ff.count, ff.mean, ff.var_sum = fa.count, fa.mean.clone(), fa.var_sum.clone()
    for p, q in zip(f.net.parameters(), a.net.parameters()):
        assert torch.equal(p, q)
    stats = {k: ag.end_episode(torch.arange(n, device="cuda")) for k, ag in agents.items()}
    for key in ("policy_loss", "value_loss", "kl_change"):
        x, y = stats["autograd"][key], stats["fused_recurrent"][key]
        print("%s: autograd %.9g, fused_recurrent %.9g, relative %.3e" % (key, x, y, abs(x - y) / abs(x)))
        assert abs(x - y) <= 1e-3 * abs(x), (key, x, y)
    assert stats["autograd"]["penalty"] == stats["fused_recurrent"]["penalty"]
