"""The cases of the fused recurrent learner's tests (test_fused_recurrent_learner_host.py, test_gpu_fused_recurrent_learner.py): a
RecurrentGaussianPolicy at init is the OLD policy, the same net with every parameter perturbed by 0.15 N(0,1) (mean|p| + 0.05) the CURRENT
one -- the construction of tests/test_gpu_fused_learner.py, its constants and its loss, for the recurrent network."""
import copy

import torch

from rex_gym_amd.agents import PPOConfig
from rex_gym_amd.agents import ppo

SEED = 3
PENALTY, CUTOFF, COEF = 0.7, 0.02, 1000.0
SHAPES = {"r5": (5, 37, [37, 0, 1, 20, 33]), "r67": (67, 130, [(i * 37) % 131 for i in range(67)]), "r1": (1, 1, [1]), "r3": (3, 200, [200, 129, 64])}
NAMES = ("w1", "b1", "wm", "bm", "logstd", "wg", "bg", "wc", "bc")       # the order of RecurrentGaussianPolicy.policy_parameters()


def make_case(shape, O, A, F=200):
    """The inputs of one case (CPU, fp32; padded slots zero)."""
    R, T, lengths = SHAPES[shape]
    g = torch.Generator().manual_seed(SEED)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(SEED)
        old = ppo.RecurrentGaussianPolicy(O, A, PPOConfig(policy_layers=(F, 100), value_layers=(F, 100), network="recurrent"))
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
    return dict(R=R, T=T, O=O, A=A, net=net, length=length, observ=observ, action=action, old_mean=old_mean, old_logstd=old_logstd, advantage=advantage)


def policy_loss(net, c, dtype):
    """`_update_policy`'s loss, line by line (agents/ppo.py)"""
    mask = ppo._mask(c["length"], c["T"], dtype)
    mean, logstd, _ = net(c["observ"])
    kl = (mask * ppo.diag_normal_kl(c["old_mean"], c["old_logstd"], mean, logstd)).mean(1)
    ratio = torch.exp(ppo.diag_normal_logpdf(mean, logstd, c["action"]) - ppo.diag_normal_logpdf(c["old_mean"], c["old_logstd"], c["action"]))
    surrogate = -(mask * ratio * c["advantage"]).mean(1)
    kl_cutoff = COEF * (kl > CUTOFF).to(dtype) * (kl - CUTOFF) ** 2
    return (surrogate + PENALTY * kl + kl_cutoff).mean(), kl


def to(c, device, dtype):
    out = {}
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            v = v.to(device=device, dtype=dtype if v.is_floating_point() else None)
        elif isinstance(v, torch.nn.Module):
            v = copy.deepcopy(v).to(device=device, dtype=dtype)
        out[k] = v
    return out


def autograd(c, device, dtype):
    """loss, kl_row and the nine gradients (policy_parameters() order) by autograd"""
    c = to(c, device, dtype)
    loss, kl = policy_loss(c["net"], c, dtype)
    grads = torch.autograd.grad(loss, c["net"].policy_parameters())
    return dict(policy_grads=[g.detach() for g in grads], policy_loss=loss.detach().reshape(1), kl_row=kl.detach())
