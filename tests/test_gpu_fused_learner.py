"""The fused PPO learner (csrc/rex_learner.h behind agents/fused_learner.py) on the GPU, against PyTorch autograd.

Yardstick: the same loss evaluated by autograd in fp64 (CPU).  For a tensor x, err(x) = max|x - x64| / max|x64|.  The fused kernels and the
existing fp32 autograd path are both fp32 evaluations of one formula in different summation orders, so the kernels are held to
8 x FLOOR, where FLOOR is the largest err the fp32 autograd path (on the device, as users run it) shows over the parameter-gradient tensors
of the same case and network -- measured in the run, nothing hard-coded; a wrong term shows at 1e-2 or more.  Every gradient tensor is held to
8 x FLOOR.  Loss, kl_row and the masked value output are held to 8 x max(FLOOR, the fp32 autograd path's own err of that quantity): a scalar
is conditioned differently from the gradients -- the loss is a sum of terms of both signs (surrogate, penalty, cutoff), and with a single
sample nothing averages out -- so that fp32 autograd itself can miss 8 x FLOOR on it (one row of one step, O = 4, A = 1: its kl_row err is
several times its gradient floor); what fp32 autograd reaches on the quantity is the measure of what an fp32 evaluation can reach.
Measured on an MI355X: of the seventeen cases' scalars, the kernels exceed 8 x FLOOR in one -- the single value of (one row of one step, O = 16,
A = 4): 7.4e-6, fp32 autograd 1.0e-5, 8 x FLOOR 1.6e-6; fp32 autograd exceeds it in three more.
REX_PARITY_JSON=<path> makes the run write every measured error of both paths there (profiles/fused_learner_parity.json is such a run's file).

Shapes: the smallest at which the kernels can still go wrong -- T no multiple of the 64-step tile with an empty, a one-step and a full row;
67 rows x 3 tiles, which takes many workgroups and the cross-workgroup reduction; one row of one step (a single row cannot lie on both sides
of the KL cutoff: for that shape only the distance from the cutoff is asserted).  Hidden layers of 200 and 100 units, plus one case each of
(40, 24) -- fewer 32-unit tiles than waves -- and of the widest the kernels offer, (256, 128)."""
import copy
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from rex_gym_amd.agents import PPOAgent, PPOConfig, train
from rex_gym_amd.agents import ppo

pytestmark = pytest.mark.gpu

SEED = 3
PENALTY, CUTOFF, COEF = 0.7, 0.02, 1000.0
SHAPES = {"r5": (5, 37, [37, 0, 1, 20, 33]), "r67": (67, 130, [(i * 37) % 131 for i in range(67)]), "r1": (1, 1, [1])}
DIMS = [(4, 2), (16, 4), (22, 4), (4, 1), (4, 8)]
CASES = [(s, o, a, (200, 100)) for s in ("r5", "r67", "r1") for (o, a) in DIMS] + [("r5", 4, 2, (40, 24)), ("r67", 16, 4, (256, 128))]


def _id(case):
    s, o, a, h = case
    return "%s-O%d-A%d" % (s, o, a) + ("" if h == (200, 100) else "-H%dx%d" % h)
_PARITY = {}


def _err(x, x64):
    return float((x.detach().double().cpu() - x64).abs().max() / x64.abs().max().clamp_min(1e-300))


def _case(shape, O, A, hidden=(200, 100)):
    """The inputs of one case (CPU, fp32; padded slots zero): a ForwardGaussianPolicy at init is the OLD policy, the same net with every
    parameter perturbed by 0.15 N(0,1) (mean|p| + 0.05) the CURRENT one."""
    R, T, lengths = SHAPES[shape]
    g = torch.Generator().manual_seed(SEED)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(SEED)
        old = ppo.ForwardGaussianPolicy(O, A, PPOConfig(policy_layers=hidden, value_layers=hidden))
    net = copy.deepcopy(old)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.15 * torch.randn(p.shape, generator=g) * (p.abs().mean() + 0.05))
    length = torch.tensor(lengths, dtype=torch.long)
    mask = ppo._mask(length, T)
    observ = torch.randn((R, T, O), generator=g) * mask[..., None]
    with torch.no_grad():
        old_mean = old(observ)[0] * mask[..., None]
    old_logstd = (old.logstd.detach() + 0.1 * torch.randn((R, T, A), generator=g)) * mask[..., None]
    action = (old_mean + torch.exp(old_logstd) * torch.randn((R, T, A), generator=g)) * mask[..., None]
    advantage = torch.randn((R, T), generator=g) * mask
    return_ = torch.randn((R, T), generator=g) * mask
    return dict(R=R, T=T, O=O, A=A, net=net, length=length, observ=observ, action=action, old_mean=old_mean, old_logstd=old_logstd,
                advantage=advantage, return_=return_)


def _policy_loss(net, c, dtype):
    """`_update_policy`'s loss, line by line (agents/ppo.py)"""
    mask = ppo._mask(c["length"], c["T"], dtype)
    mean, logstd, _ = net(c["observ"])
    kl = (mask * ppo.diag_normal_kl(c["old_mean"], c["old_logstd"], mean, logstd)).mean(1)
    ratio = torch.exp(ppo.diag_normal_logpdf(mean, logstd, c["action"]) - ppo.diag_normal_logpdf(c["old_mean"], c["old_logstd"], c["action"]))
    surrogate = -(mask * ratio * c["advantage"]).mean(1)
    kl_cutoff = COEF * (kl > CUTOFF).to(dtype) * (kl - CUTOFF) ** 2
    return (surrogate + PENALTY * kl + kl_cutoff).mean(), kl


def _value_loss(net, c, dtype):
    mask = ppo._mask(c["length"], c["T"], dtype)
    value = net(c["observ"])[2] * mask
    return (0.5 * mask * (c["return_"] - value) ** 2).mean(), value


def _to(c, device, dtype):
    out = {}
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            v = v.to(device=device, dtype=dtype if v.is_floating_point() else None)
        elif isinstance(v, torch.nn.Module):
            v = copy.deepcopy(v).to(device=device, dtype=dtype)
        out[k] = v
    return out


def _autograd(c, device, dtype):
    c = _to(c, device, dtype)
    net = c["net"]
    loss, kl = _policy_loss(net, c, dtype)
    pg = torch.autograd.grad(loss, net.policy_parameters())
    vloss, value = _value_loss(net, c, dtype)
    vg = torch.autograd.grad(vloss, net.value_parameters())
    return dict(policy_grads=[g.detach() for g in pg], value_grads=[g.detach() for g in vg], policy_loss=loss.detach().reshape(1), kl_row=kl.detach(),
                value_loss=vloss.detach().reshape(1), value=value.detach())


_REFS = {}


def _reference(case):
    """The fp64 yardstick and the fp32 autograd path's errors against it, once per case."""
    if case not in _REFS:
        c = _case(*case)
        r64 = _autograd(c, "cpu", torch.float64)
        kl = r64["kl_row"]
        if c["R"] > 1:     # the discrete branch [kl_r > c] must be exercised on both sides ...
            assert int((kl > CUTOFF).sum()) >= 1 and int((kl <= CUTOFF).sum()) >= 1, kl
        assert float(((kl - CUTOFF).abs() / CUTOFF).min()) > 1e-3, kl      # ... and decided the same way by every fp32 evaluation
        r32 = _autograd(c, "cuda", torch.float32)
        floor = {}
        for key in ("policy_grads", "value_grads"):
            floor[key] = [_err(a, b) for a, b in zip(r32[key], r64[key])]
        for key in ("policy_loss", "kl_row", "value_loss", "value"):
            floor[key] = _err(r32[key], r64[key])
        _REFS[case] = (c, r64, floor)
    return _REFS[case]


def _learner(c):
    from rex_gym_amd.agents.fused_learner import FusedLearner
    g = _to(c, "cuda", torch.float32)
    fl = FusedLearner(g["net"], c["R"], c["T"], "cuda")
    fl.set_length(g["length"])
    return g, fl


def _run(g, fl, grad=True):
    loss, vloss = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    fl.policy_flat.fill_(float("nan")); fl.value_flat.fill_(float("nan"))       # every gradient element must be written
    fl.policy_loss(g["observ"], g["action"], g["old_mean"], g["old_logstd"], g["advantage"], PENALTY, CUTOFF, COEF, loss, grad=grad)
    value = torch.full((g["R"], g["T"]), float("nan"), device="cuda")
    fl.value_loss(g["observ"], g["return_"], vloss, grad=grad, value_out=value)
    torch.cuda.synchronize()
    return dict(policy_grads=[v.clone() for v in fl.policy_grads], value_grads=[v.clone() for v in fl.value_grads], policy_loss=loss.clone(),
                kl_row=fl.kl_row.clone(), value_loss=vloss.clone(), value=value)


def _flat(res):
    return [res["policy_loss"], res["kl_row"], res["value_loss"], res["value"]] + res["policy_grads"] + res["value_grads"]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gradients_losses_and_kl_match_fp64_autograd_within_8x_the_fp32_autograd_floor(case):
    c, r64, floor = _reference(case)
    g, fl = _learner(c)
    res = _run(g, fl)
    names = {"policy_grads": ["w1", "b1", "w2", "b2", "w3", "b3", "logstd"], "value_grads": ["w1", "b1", "w2", "b2", "w3", "b3"]}
    report, bad = {}, []
    for key, scalars in (("policy_grads", ("policy_loss", "kl_row")), ("value_grads", ("value_loss", "value"))):
        bound = 8.0 * max(floor[key])
        for n, got, want, fl32 in zip(names[key], res[key], r64[key], floor[key]):
            e = _err(got, want)
            report["%s.%s" % (key, n)] = {"fused": e, "autograd_fp32": fl32}
            print("%s %s.%s: fused %.3e, fp32 autograd %.3e, bound %.3e" % (case, key, n, e, fl32, bound))
            if not e <= bound:
                bad.append((key, n, e, bound))
        for s in scalars:
            e, sbound = _err(res[s], r64[s]), max(bound, 8.0 * floor[s])
            report[s] = {"fused": e, "autograd_fp32": floor[s]}
            print("%s %s: fused %.3e, fp32 autograd %.3e, bound %.3e" % (case, s, e, floor[s], sbound))
            if not e <= sbound:
                bad.append((s, e, sbound))
    _PARITY[_id(case)] = report
    if os.environ.get("REX_PARITY_JSON"):
        with open(os.environ["REX_PARITY_JSON"], "w") as f:
            json.dump({"yardstick": "fp64 autograd (CPU); err = max|x - x64| / max|x64|", "bound": "gradients: 8 x the largest autograd_fp32 err over the net's gradient tensors; loss, kl_row, value: 8 x max(that, the quantity's own autograd_fp32 err)",
                       "cases": _PARITY}, f, indent=1, sort_keys=True)
    assert not bad, bad


@pytest.mark.parametrize("shape", list(SHAPES))
def test_returns_match_the_python_loops(shape):
    R, T, lengths = SHAPES[shape]
    g = torch.Generator().manual_seed(SEED)
    reward, value = torch.randn((R, T), generator=g), torch.randn((R, T), generator=g)
    length = torch.tensor(lengths)
    disc, lam = 0.985, 0.8
    want_r = ppo.discounted_return(reward.double(), length, disc)
    want_l = ppo.lambda_return(reward.double(), value.double(), length, disc, lam)
    dr, dv, dl = reward.cuda(), value.cuda(), length.cuda()
    floor_r, floor_l = _err(ppo.discounted_return(dr, dl, disc), want_r), _err(ppo.lambda_return(dr, dv, dl, disc, lam), want_l)
    from rex_gym_amd.agents.fused_learner import FusedLearner
    fl = FusedLearner(ppo.ForwardGaussianPolicy(4, 2, PPOConfig()).cuda(), R, T, "cuda")
    fl.set_length(dl)
    got_r, got_l = fl.returns(dr, disc, dv, lam)
    only_r, none = fl.returns(dr, disc)
    e_r, e_l = _err(got_r, want_r), _err(got_l, want_l)
    print("%s: return fused %.3e / torch %.3e, lambda return fused %.3e / torch %.3e" % (shape, e_r, floor_r, e_l, floor_l))
    assert none is None and torch.equal(only_r, got_r)
    assert e_r <= 8 * floor_r and e_l <= 8 * floor_l
    m = ppo._mask(length, T).bool()
    assert float(got_r.cpu()[~m].abs().sum()) == 0.0          # zero beyond the length


def test_two_calls_give_the_same_bits():
    c, _, _ = _reference(("r67", 4, 2, (200, 100)))
    g, fl = _learner(c)
    a, b = _run(g, fl), _run(g, fl)
    for x, y in zip(_flat(a), _flat(b)):
        assert torch.equal(x, y)


def test_padded_slots_are_never_read():
    c, _, _ = _reference(("r67", 16, 4, (200, 100)))
    outs = []
    for fill in (0.0, 50.0):
        g, fl = _learner(c)
        pad = ~ppo._mask(g["length"], c["T"]).bool()
        for k in ("observ", "action", "old_mean", "old_logstd", "advantage", "return_"):
            g[k] = g[k].clone()
            g[k][pad] = fill
        outs.append(_run(g, fl))
    for x, y in zip(_flat(outs[0]), _flat(outs[1])):
        assert torch.equal(x, y)
    assert float(outs[1]["value"][pad].abs().sum()) == 0.0


def test_forward_only_mode_returns_the_same_loss_and_kl():
    c, _, _ = _reference(("r67", 4, 2, (200, 100)))
    g, fl = _learner(c)
    full = _run(g, fl)
    fwd = _run(g, fl, grad=False)
    for k in ("policy_loss", "kl_row", "value_loss", "value"):
        assert torch.equal(full[k], fwd[k]), k
    assert all(bool(torch.isnan(v).all()) for v in fwd["policy_grads"] + fwd["value_grads"])      # and writes no gradient


def test_unsupported_dims_are_refused_with_a_message():
    from rex_gym_amd import _lib
    from rex_gym_amd.agents.fused_learner import FusedLearner, net_struct
    L = _lib.lib()
    for dims in ((5, 37, 5, 2, 200, 100), (5, 37, 4, 3, 200, 100), (5, 37, 4, 2, 300, 100), (5, 37, 4, 2, 200, 129), (0, 37, 4, 2, 200, 100)):
        assert L.rex_ppo_workspace_bytes(*dims) == -1
        assert b"rex_ppo_workspace_bytes" in L.rex_last_error()
    net = ppo.ForwardGaussianPolicy(5, 3, PPOConfig()).cuda()
    with pytest.raises(ValueError, match="obs_dim 5"):
        FusedLearner(net, 5, 37, "cuda")
    n = net_struct(net.policy_parameters())
    b = _lib.RexPpoBatch()
    b.rows, b.steps = 5, 37
    buf = torch.zeros(64, device="cuda")
    assert L.rex_ppo_policy_loss(ctypes.byref(n), ctypes.byref(b), None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) == -1
    assert b"obs_dim 5" in L.rex_last_error()
    with pytest.raises(ValueError, match="recurrent"):
        PPOAgent(4, 4, 2, PPOConfig(network="recurrent", learner="fused"), device="cuda")


# ---- end to end: the toy task of tests/test_agents_ppo.py, on the device.  The point's position is the first of FOUR observation columns (the
# narrowest observation the kernels offer; the other three are zero): the task, the rewards and every setting but the layers are that test's ----
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


def _toy_cfg(learner):
    return PPOConfig(policy_layers=(200, 100), value_layers=(200, 100), update_every=64, update_epochs_policy=15, update_epochs_value=15,
                     policy_lr=3e-3, value_lr=3e-3, max_length=12, discount=0.9, init_mean_factor=0.1, learner=learner)


def test_fused_ppo_learns_the_toy_task_and_adapts_its_penalty():
    torch.manual_seed(0)
    n = 64
    env, agent = _PointEnv(n), PPOAgent(n, 4, 1, _toy_cfg("fused"), device="cuda", seed=3)
    first, _ = train(env, agent, 12 * 3)
    for _ in range(12):
        last, length = train(env, agent, 12 * 3)
    assert agent.updates >= 30 and length == 12
    assert last > first + 1.0, (first, last)
    kls = [s["kl_change"] for s in agent.log]
    assert all(np.isfinite(k) for k in kls) and max(kls) < 1.0
    pens = [s["penalty"] for s in agent.log]
    assert len(set(pens)) > 1
    assert all(abs(math.log(pens[i + 1] / pens[i]) / math.log(1.5)) in (0.0, 1.0) or abs(abs(math.log(pens[i + 1] / pens[i]) / math.log(1.5)) - 1) < 1e-6
               for i in range(len(pens) - 1))


def test_one_training_from_identical_state_agrees_under_both_learners():
    n = 64
    agents = {k: PPOAgent(n, 4, 1, _toy_cfg(k), device="cuda", seed=3) for k in ("autograd", "fused")}
    torch.manual_seed(0)
    train(_PointEnv(n), agents["autograd"], 11)           # eleven steps of experience: the episodes end at the twelfth, below, in both agents
    a, f = agents["autograd"], agents["fused"]
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
        x, y = stats["autograd"][key], stats["fused"][key]
        print("%s: autograd %.9g, fused %.9g, relative %.3e" % (key, x, y, abs(x - y) / abs(x)))
        assert abs(x - y) <= 1e-3 * abs(x), (key, x, y)
