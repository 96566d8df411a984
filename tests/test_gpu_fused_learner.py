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
import ctypes

import pytest
import torch

from rex_gym_amd.agents import PPOAgent, PPOConfig
from rex_gym_amd.agents import ppo

import fused_cases as fc

pytestmark = pytest.mark.gpu

BOUND = "gradients: 8 x the largest autograd_fp32 err over the net's gradient tensors; loss, kl_row, value: 8 x max(that, the quantity's own autograd_fp32 err)"
_PARITY = {}


@pytest.mark.parametrize("case", fc.CASES["forward"], ids=lambda c: fc.case_id("forward", c))
def test_gradients_losses_and_kl_match_fp64_autograd_within_8x_the_fp32_autograd_floor(case):
    c, r64, floor = fc.reference("forward", case)
    g, fl = fc.learner("forward", c)
    res = fc.run(g, fl)
    bad, _PARITY[fc.case_id("forward", case)] = fc.hold_to_the_floor(case, res, r64, floor, (("policy_grads", fc.NAMES["forward"], ("policy_loss", "kl_row")),
                                                                                                 ("value_grads", fc.VALUE_NAMES, ("value_loss", "value"))))
    fc.write_parity_report(_PARITY, BOUND)
    assert not bad, bad


@pytest.mark.parametrize("shape", ["r5", "r67", "r1"])
def test_returns_match_the_python_loops(shape):
    R, T, lengths = fc.SHAPES[shape]
    g = torch.Generator().manual_seed(fc.SEED)
    reward, value = torch.randn((R, T), generator=g), torch.randn((R, T), generator=g)
    length = torch.tensor(lengths)
    disc, lam = 0.985, 0.8
    want_r = ppo.discounted_return(reward.double(), length, disc)
    want_l = ppo.lambda_return(reward.double(), value.double(), length, disc, lam)
    dr, dv, dl = reward.cuda(), value.cuda(), length.cuda()
    floor_r, floor_l = fc.err(ppo.discounted_return(dr, dl, disc), want_r), fc.err(ppo.lambda_return(dr, dv, dl, disc, lam), want_l)
    from rex_gym_amd.agents.fused_learner import FusedLearner
    fl = FusedLearner(ppo.ForwardGaussianPolicy(4, 2, PPOConfig()).cuda(), R, T, "cuda")
    fl.set_length(dl)
    got_r, got_l = fl.returns(dr, disc, dv, lam)
    only_r, none = fl.returns(dr, disc)
    e_r, e_l = fc.err(got_r, want_r), fc.err(got_l, want_l)
    print("%s: return fused %.3e / torch %.3e, lambda return fused %.3e / torch %.3e" % (shape, e_r, floor_r, e_l, floor_l))
    assert none is None and torch.equal(only_r, got_r)
    assert e_r <= 8 * floor_r and e_l <= 8 * floor_l
    m = ppo._mask(length, T).bool()
    assert float(got_r.cpu()[~m].abs().sum()) == 0.0          # zero beyond the length


def test_two_calls_give_the_same_bits():
    c, _, _ = fc.reference("forward", ("r67", 4, 2, (200, 100)))
    g, fl = fc.learner("forward", c)
    a, b = fc.run(g, fl), fc.run(g, fl)
    for x, y in zip(fc.flat(a), fc.flat(b)):
        assert torch.equal(x, y)


def test_padded_slots_are_never_read():
    c, _, _ = fc.reference("forward", ("r67", 16, 4, (200, 100)))
    outs = []
    for fill in (0.0, 50.0):
        g, fl = fc.learner("forward", c)
        pad = ~ppo._mask(g["length"], c["T"]).bool()
        for k in ("observ", "action", "old_mean", "old_logstd", "advantage", "return_"):
            g[k] = g[k].clone()
            g[k][pad] = fill
        outs.append(fc.run(g, fl))
    for x, y in zip(fc.flat(outs[0]), fc.flat(outs[1])):
        assert torch.equal(x, y)
    assert float(outs[1]["value"][pad].abs().sum()) == 0.0


def test_forward_only_mode_returns_the_same_loss_and_kl():
    c, _, _ = fc.reference("forward", ("r67", 4, 2, (200, 100)))
    g, fl = fc.learner("forward", c)
    full = fc.run(g, fl)
    fwd = fc.run(g, fl, grad=False)
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


# ---- end to end: the toy point task (fused_cases.py) ----
def test_fused_ppo_learns_the_toy_task_and_adapts_its_penalty():
    fc.assert_learns_the_toy_task(fc.toy_cfg("fused"))


def test_one_training_from_identical_state_agrees_under_both_learners():
    # eleven steps of experience: the episodes end at the twelfth in both agents
    fc.one_training_under_both_learners(64, {k: fc.toy_cfg(k) for k in ("autograd", "fused")}, 11)
