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

import pytest
import torch

from rex_gym_amd.agents import PPOAgent, PPOConfig
from rex_gym_amd.agents import ppo

import fused_cases as fc

pytestmark = pytest.mark.gpu

BOUND = "gradients: 8 x the largest autograd_fp32 err over the nine gradient tensors; loss, kl_row: 8 x max(that, the quantity's own autograd_fp32 err)"
_PARITY = {}


@pytest.mark.parametrize("case", fc.CASES["recurrent"], ids=lambda c: fc.case_id("recurrent", c))
def test_gradients_loss_and_kl_match_fp64_autograd_within_8x_the_fp32_autograd_floor(case):
    c, r64, floor = fc.reference("recurrent", case)
    g, fl = fc.learner("recurrent", c)
    res = fc.run(g, fl)
    bad, _PARITY[fc.case_id("recurrent", case)] = fc.hold_to_the_floor(case, res, r64, floor, (("policy_grads", fc.NAMES["recurrent"], ("policy_loss", "kl_row")),))
    fc.write_parity_report(_PARITY, BOUND)
    assert not bad, bad


def test_two_calls_give_the_same_bits():
    c, _, _ = fc.reference("recurrent", ("r67", 4, 2, (200, 100)))
    g, fl = fc.learner("recurrent", c)
    a, b = fc.run(g, fl), fc.run(g, fl)
    for x, y in zip(fc.flat(a), fc.flat(b)):
        assert torch.equal(x, y)


def test_padded_slots_are_never_read():
    c, _, _ = fc.reference("recurrent", ("r67", 16, 4, (200, 100)))
    outs = []
    for fill in (0.0, float("nan")):
        g, fl = fc.learner("recurrent", c)
        pad = ~ppo._mask(g["length"], c["T"]).bool()
        for k in ("observ", "action", "old_mean", "old_logstd", "advantage"):
            g[k] = g[k].clone()
            g[k][pad] = fill
        outs.append(fc.run(g, fl))
    for x, y in zip(fc.flat(outs[0]), fc.flat(outs[1])):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_forward_only_mode_returns_the_same_loss_and_kl():
    c, _, _ = fc.reference("recurrent", ("r67", 4, 2, (200, 100)))
    g, fl = fc.learner("recurrent", c)
    full = fc.run(g, fl)
    fwd = fc.run(g, fl, grad=False)
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


# ---- end to end: the toy point task (fused_cases.py) under the recurrent network ----
def test_fused_recurrent_ppo_learns_the_toy_task_and_adapts_its_penalty():
    fc.assert_learns_the_toy_task(fc.toy_cfg("fused_recurrent", network="recurrent"))


def test_one_training_from_identical_state_agrees_under_both_learners():
    """8 rows x 40 steps; the tolerance is the forward test's: 1e-3 relative on the statistics of one whole update (15 + 15 Adam steps, each
    amplifying the learners' last-bit differences), and the same penalty decision."""
    n = 8
    cfgs = {k: PPOConfig(**{**fc.toy_cfg(k, network="recurrent").__dict__, "update_every": n, "max_length": 40}) for k in ("autograd", "fused_recurrent")}
    stats = fc.one_training_under_both_learners(n, cfgs, 39)      # 39 steps of experience: the episodes end at the fortieth in both agents
    assert stats["autograd"]["penalty"] == stats["fused_recurrent"]["penalty"]
