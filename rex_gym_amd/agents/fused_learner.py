"""The fused PPO learners: `PPOConfig(learner="fused")` runs the losses of agents/ppo.py and their parameter gradients in the HIP
kernels of csrc/rex_learner.h (rex_ppo_policy_loss, rex_ppo_value_loss, rex_ppo_returns; entry points in csrc/rex_learner.hip, formulas in
include/rexsim.h) instead of PyTorch autograd.  Adam, the gradient all-reduce (`PPOAgent._sync`), the filters and the penalty adaptation
stay in PyTorch: the kernels write the gradients straight into the tensors that ARE the parameters' `.grad`.

`PPOConfig(learner="fused_recurrent")` is the same for the RecurrentGaussianPolicy: its policy loss and the nine gradients by backpropagation
through time run in the kernels of csrc/rex_learner_rnn.h (rex_ppo_recurrent_policy_loss); the value net is the plain two-layer network and
stays on rex_ppo_value_loss.  One class does the work: `FusedLearner` holds the buffers, the workspace sizing and the calls;
`FusedRecurrentLearner` only overrides what differs -- its struct builders, its workspace-size call, its entry point and that the policy keeps
a workspace of its own.  `check_config(cfg, device, learner)` states what either needs.

Host-only pieces (no GPU needed): `output_seeds`, the hand-derived backward seeds of the policy loss in plain torch -- what the kernels
compute per sample, checked against autograd in tests/test_fused_learner_host.py; `recurrent_backward`, the restatement of the backward
recurrence (tests/test_fused_recurrent_learner_host.py holds it to autograd); and `flat_gradients` / `net_struct` / `grad_struct` /
`rnn_net_struct` / `rnn_grad_struct`, which lay parameters and gradients out for the C ABI (one filler, `_pointer_struct`, behind the four).
"""
import ctypes

import torch

from .. import _lib


def output_seeds(mean, logstd, old_mean, old_logstd, action, advantage, length, penalty, cutoff, coef):
    """d loss / d mean, d loss / d logstd (both [R, T, A]) and kl_row [R] of `_update_policy`'s loss, derived by hand:

        loss = (1/R) sum_r [ -(1/T) sum_t m ratio adv + penalty kl_r + coef [kl_r > c] (kl_r - c)^2 ],  kl_r = (1/T) sum_t m KL_t
        w_r = penalty + 2 coef [kl_r > c] (kl_r - c)
        dKL/dm = (m - m0) / e^2l         dKL/dl   = 1 - e^(2 l0 - 2 l) - (m - m0)^2 / e^2l
        dlogp/dm = (x - m) / e^2l        dlogp/dl = -0.5 + ((x - m) / e^l)^2      (diag_normal_logpdf as written: its -0.5 logstd)
        g = (-ratio adv dlogp + w_r dKL) / (R T) on valid steps, 0 on padded ones

    mean, logstd, old_mean, old_logstd, action: [R, T, A]; advantage: [R, T]; length: [R]."""
    R, T, _ = mean.shape
    mask = (torch.arange(T, device=mean.device)[None, :] < length[:, None]).to(mean.dtype)
    ie2 = torch.exp(-2 * logstd)
    dm, dx = mean - old_mean, action - mean
    ev = torch.exp(2 * old_logstd - 2 * logstd)
    kl_t = 0.5 * (ev + dm ** 2 * ie2 + 2 * logstd - 2 * old_logstd - 1).sum(-1)
    kl_row = (mask * kl_t).mean(1)
    u2, u02 = (dx * torch.exp(-logstd)) ** 2, ((action - old_mean) * torch.exp(-old_logstd)) ** 2
    ratio = torch.exp((-0.5 * (logstd - old_logstd) - 0.5 * (u2 - u02)).sum(-1))
    w = penalty + 2 * coef * (kl_row > cutoff).to(mean.dtype) * (kl_row - cutoff)
    ra = (mask * ratio * advantage)[..., None]
    wk = (mask * w[:, None])[..., None]
    g_mean = (wk * dm * ie2 - ra * dx * ie2) / (R * T)
    g_logstd = (wk * (1 - ev - dm ** 2 * ie2) - ra * (-0.5 + u2)) / (R * T)
    return g_mean, g_logstd, kl_row


def recurrent_backward(w1, b1, wg, bg, wc, bc, wm, bm, logstd, observ, old_mean, old_logstd, action, advantage, length, penalty, cutoff, coef):
    """The policy loss of a RecurrentGaussianPolicy and its nine parameter gradients WITHOUT autograd: the forward recurrence, `output_seeds`,
    then the backward recurrence of include/rexsim.h in reverse t with carry_T = 0 -- what the kernels of csrc/rex_learner_rnn.h compute.
    Weights in torch layout (W1 [F, O], Wg [2H, F + H], Wc [H, F + H], Wm [A, H]); observ [R, T, O].  Returns (grads, kl_row) with grads a
    dict keyed w1, b1, wg, bg, wc, bc, wm, bm, logstd."""
    R, T, _ = observ.shape
    F, H = w1.shape[0], wc.shape[0]
    a1 = observ @ w1.T + b1
    x = torch.relu(a1)
    h = torch.zeros((R, H), dtype=observ.dtype, device=observ.device)
    hp, rs, us, cs, hs = [], [], [], [], []
    for t in range(T):
        r, u = torch.sigmoid(torch.cat([x[:, t], h], -1) @ wg.T + bg).chunk(2, -1)
        c = torch.tanh(torch.cat([x[:, t], r * h], -1) @ wc.T + bc)
        hp.append(h)
        h = u * h + (1 - u) * c
        rs.append(r); us.append(u); cs.append(c); hs.append(h)
    hs_ = torch.stack(hs, 1)
    m = torch.tanh(hs_ @ wm.T + bm)
    g_m, g_l, kl_row = output_seeds(m, logstd.expand_as(m), old_mean, old_logstd, action, advantage, length, penalty, cutoff, coef)
    g_z = g_m * (1 - m ** 2)
    grads = {"w1": torch.zeros_like(w1), "b1": torch.zeros_like(b1), "wg": torch.zeros_like(wg), "bg": torch.zeros_like(bg), "wc": torch.zeros_like(wc),
             "bc": torch.zeros_like(bc), "wm": torch.einsum("rta,rth->ah", g_z, hs_), "bm": g_z.sum((0, 1)), "logstd": g_l.sum((0, 1))}
    carry = torch.zeros_like(h)
    for t in range(T - 1, -1, -1):
        r, u, c, h0 = rs[t], us[t], cs[t], hp[t]
        dh = g_z[:, t] @ wm + carry
        du, dc, carry = dh * (h0 - c), dh * (1 - u), dh * u
        da_c = dc * (1 - c ** 2)
        dxh = da_c @ wc
        dx_c, drh = dxh[:, :F], dxh[:, F:]
        dr = drh * h0
        carry = carry + drh * r
        da_g = torch.cat([dr * r * (1 - r), du * u * (1 - u)], -1)
        dxh = da_g @ wg
        carry = carry + dxh[:, F:]
        da1 = (dx_c + dxh[:, :F]) * (a1[:, t] > 0).to(observ.dtype)
        grads["wg"] += da_g.T @ torch.cat([x[:, t], h0], -1); grads["bg"] += da_g.sum(0)
        grads["wc"] += da_c.T @ torch.cat([x[:, t], r * h0], -1); grads["bc"] += da_c.sum(0)
        grads["w1"] += da1.T @ observ[:, t]; grads["b1"] += da1.sum(0)
    return grads, kl_row


def flat_gradients(params):
    """One flat float32 buffer on the parameters' device, and every parameter's `.grad` set to its own view into it (torch layout, the
    order of `params`): the kernels write the gradients where Adam and the all-reduce read them.  Returns (flat, views)."""
    params = list(params)
    flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=params[0].device)
    views, at = [], 0
    for p in params:
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError("the fused learner needs contiguous float32 parameters")
        v = flat[at:at + p.numel()].view(p.shape)
        p.grad = v
        views.append(v)
        at += p.numel()
    return flat, views


FORWARD_FIELDS = ("d_w1", "d_b1", "d_w2", "d_b2", "d_w3", "d_b3", "d_logstd")                 # a two-layer net's parameters (the value net: no logstd)
RNN_FIELDS = ("d_w1", "d_b1", "d_wm", "d_bm", "d_logstd", "d_wg", "d_bg", "d_wc", "d_bc")     # the order of RecurrentGaussianPolicy.policy_parameters()


def _pointer_struct(cls, fields, tensors, counts, what):
    """The d_* pointer fields of a RexPpo*Net / RexPpo*Grad from tensors in the order of `fields`; `counts`: how many there may be."""
    tensors = list(tensors)
    if len(tensors) not in counts:
        raise ValueError(what)
    s = cls()
    for n, t in zip(fields, tensors):
        setattr(s, n, t.data_ptr())
    return s


def _forward_struct(cls, tensors):
    return _pointer_struct(cls, FORWARD_FIELDS, tensors, (6, 7), "a two-layer network has six tensors (and logstd): W1, b1, W2, b2, W3, b3")


def _rnn_struct(cls, tensors):
    return _pointer_struct(cls, RNN_FIELDS, tensors, (9,), "a recurrent policy has nine tensors: W1, b1, Wm, bm, logstd, Wg, bg, Wc, bc")


def net_struct(params):
    """RexPpoNet of a network given as its tensors in torch order and layout: Linear weights [out][in] as they are."""
    params = list(params)
    s = _forward_struct(_lib.RexPpoNet, params)
    w1, w2, w3 = params[0], params[2], params[4]
    if w2.shape[1] != w1.shape[0] or w3.shape[1] != w2.shape[0] or any(params[2 * k + 1].shape != (params[2 * k].shape[0],) for k in range(3)):
        raise ValueError("the tensors are not a chain of three Linear layers")
    s.hidden1, s.obs_dim = w1.shape
    s.hidden2 = w2.shape[0]
    s.out_dim = w3.shape[0]
    return s


def grad_struct(views):
    return _forward_struct(_lib.RexPpoGrad, views)


def rnn_net_struct(params):
    """RexPpoRnnNet of a RecurrentGaussianPolicy's policy_parameters(): W1, b1, Wm, bm, logstd, Wg, bg, Wc, bc, torch layout as they are."""
    params = list(params)
    s = _rnn_struct(_lib.RexPpoRnnNet, params)
    w1, wm, wg, wc = params[0], params[2], params[5], params[7]
    F, H = w1.shape[0], wc.shape[0]
    if wg.shape != (2 * H, F + H) or wc.shape != (H, F + H) or wm.shape[1] != H:
        raise ValueError("the tensors are not a Linear layer, a GRU cell and a mean layer")
    s.hidden1, s.obs_dim = w1.shape
    s.out_dim, s.state = wm.shape
    return s


def rnn_grad_struct(views):
    return _rnn_struct(_lib.RexPpoRnnGrad, views)


# learner -> its network, what it says of another one, and its (layer settings, what it says unless each has two entries)
_CONFIG_NEEDS = {
    "fused": ("forward", "is the ForwardGaussianPolicy's learner (network='forward'); the recurrent policy's update is out of its scope: it runs on "
                         "learner='fused_recurrent' (or 'autograd')",
              [(("policy_layers", "value_layers"), "needs two policy layers and two value layers (the shape of every shipped config)")]),
    "fused_recurrent": ("recurrent", "is the RecurrentGaussianPolicy's learner (network='recurrent'); the forward network runs on learner='fused'",
                        [(("policy_layers",), "needs two policy layers: one Linear layer in front of the GRU cell"),
                         (("value_layers",), "needs two value layers (the shape of every shipped config)")]),
}


def check_config(cfg, device, learner):
    """What PPOConfig(learner="fused" / "fused_recurrent") needs; raises ValueError otherwise (PPOAgent.__init__)."""
    network, other_network, layers = _CONFIG_NEEDS[learner]
    who = "PPOConfig(learner=%r) " % learner
    if cfg.network != network:
        raise ValueError(who + other_network)
    for fields, message in layers:
        if any(len(getattr(cfg, f)) != 2 for f in fields):
            raise ValueError(who + message)
    if torch.device(device).type != "cuda":
        raise ValueError(who + "runs HIP kernels: it needs a CUDA/HIP device, not %r" % (str(device),))


class FusedLearner:
    """The kernels behind a PPOAgent: owns the flat gradient buffers (every parameter's .grad is a view into them), the workspaces and the
    int32 copy of the memory's lengths.  Every call launches on the current stream and does not synchronise with the host.  A subclass for
    another policy network overrides the four `_policy_*` methods and, for a policy workspace of its own, `_make_workspaces`."""
    what = "the fused learner"

    def __init__(self, net, rows, steps, device):
        self.device = torch.device(device)
        self.rows, self.steps = int(rows), int(steps)
        self.policy_params, self.value_params = net.policy_parameters(), net.value_parameters()
        self.policy_flat, self.policy_grads = flat_gradients(self.policy_params)
        self.value_flat, self.value_grads = flat_gradients(self.value_params)
        self._L = _lib.lib()
        policy_bytes = self._policy_workspace_bytes(self._policy_net())
        value_bytes = self._two_layer_workspace_bytes(net_struct(self.value_params)) if policy_bytes >= 0 else -1
        if value_bytes < 0:
            raise ValueError(self.what + " does not offer this shape: " + self._L.rex_last_error().decode("utf-8", "replace"))
        self._make_workspaces(policy_bytes, value_bytes)
        self.length = torch.zeros(self.rows, dtype=torch.int32, device=self.device)
        self.kl_row = torch.zeros(self.rows, device=self.device)
        self._scratch_loss = torch.zeros(1, device=self.device)

    def _two_layer_workspace_bytes(self, n):
        return self._L.rex_ppo_workspace_bytes(self.rows, self.steps, n.obs_dim, n.out_dim, n.hidden1, n.hidden2)

    def _policy_net(self):
        return net_struct(self.policy_params)

    def _policy_grad(self):
        return grad_struct(self.policy_grads)

    def _policy_workspace_bytes(self, n):
        return self._two_layer_workspace_bytes(n)

    def _policy_entry(self):
        return self._L.rex_ppo_policy_loss, "rex_ppo_policy_loss"

    def _make_workspaces(self, policy_bytes, value_bytes):
        """one workspace: the policy and the value net take turns in it"""
        self.workspace = self.policy_workspace = torch.empty(max(policy_bytes, value_bytes) // 4, dtype=torch.float32, device=self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _batch(self, observ, **blocks):
        b = _lib.RexPpoBatch()
        b.rows, b.steps = self.rows, self.steps
        if observ.shape[:2] != (self.rows, self.steps):
            raise ValueError("the memory is %s, the learner was made for %d x %d" % (tuple(observ.shape[:2]), self.rows, self.steps))
        keep = [observ.contiguous()]
        b.d_observ, b.d_length = keep[0].data_ptr(), self.length.data_ptr()
        for name, t in blocks.items():
            t = t.contiguous()
            keep.append(t)
            setattr(b, "d_" + name, t.data_ptr())
        return b, keep

    def set_length(self, length):
        self.length.copy_(length)
        return self.length

    def returns(self, reward, discount, value=None, lambda_=None):
        """discounted_return, and lambda_return when a value block is given: (return, lambda_return or None)"""
        reward = reward.contiguous()
        ret = torch.empty_like(reward)
        lam = torch.empty_like(reward) if value is not None else None
        value = value.contiguous() if value is not None else None
        with torch.cuda.device(self.device):
            _lib.check(self._L.rex_ppo_returns(reward.shape[0], reward.shape[1], reward.data_ptr(), self.length.data_ptr(), float(discount), ret.data_ptr(),
                                               value.data_ptr() if value is not None else None, float(lambda_ or 0.0),
                                               lam.data_ptr() if lam is not None else None, self._stream()), "rex_ppo_returns")
        return ret, lam

    def policy_loss(self, observ, action, old_mean, old_logstd, advantage, penalty, cutoff, coef, loss_out=None, grad=True):
        """One epoch's policy loss into loss_out[0] (a device tensor), the rows' KL into self.kl_row, the gradients into the .grad views."""
        b, keep = self._batch(observ, action=action, old_mean=old_mean, old_logstd=old_logstd, advantage=advantage)
        b.penalty, b.kl_cutoff, b.kl_cutoff_coef = float(penalty), float(cutoff), float(coef)
        loss_out = self._scratch_loss if loss_out is None else loss_out
        net, g = self._policy_net(), self._policy_grad()
        entry, name = self._policy_entry()
        with torch.cuda.device(self.device):
            _lib.check(entry(ctypes.byref(net), ctypes.byref(b), ctypes.byref(g) if grad else None, loss_out.data_ptr(), self.kl_row.data_ptr(),
                             self.policy_workspace.data_ptr(), self._stream()), name)
        return loss_out, self.kl_row

    def value_loss(self, observ, return_, loss_out=None, grad=True, value_out=None):
        """One epoch's value loss into loss_out[0], the gradients into the .grad views; value_out [R, T]: the masked values."""
        b, keep = self._batch(observ, **{"return": return_})
        loss_out = self._scratch_loss if loss_out is None else loss_out
        net, g = net_struct(self.value_params), grad_struct(self.value_grads)
        with torch.cuda.device(self.device):
            _lib.check(self._L.rex_ppo_value_loss(ctypes.byref(net), ctypes.byref(b), ctypes.byref(g) if grad else None, loss_out.data_ptr(),
                                                  value_out.data_ptr() if value_out is not None else None, self.workspace.data_ptr(), self._stream()),
                       "rex_ppo_value_loss")
        return loss_out

    def values(self, observ):
        """The value net's forward pass over the memory, zero beyond every row's length (the advantage's baseline)."""
        out = torch.empty((self.rows, self.steps), device=self.device)
        self.value_loss(observ, torch.zeros_like(out), grad=False, value_out=out)     # (the return block only feeds the loss, which is dropped)
        return out


class FusedRecurrentLearner(FusedLearner):
    """The same for a RecurrentGaussianPolicy: the policy loss runs on rex_ppo_recurrent_policy_loss (its own workspace: the stored activations
    of every memory slot), the value net and the return scans on FusedLearner's calls."""
    what = "the fused recurrent learner"

    def _policy_net(self):
        return rnn_net_struct(self.policy_params)

    def _policy_grad(self):
        return rnn_grad_struct(self.policy_grads)

    def _policy_workspace_bytes(self, n):
        return self._L.rex_ppo_recurrent_workspace_bytes(self.rows, self.steps, n.obs_dim, n.out_dim, n.hidden1, n.state)

    def _policy_entry(self):
        return self._L.rex_ppo_recurrent_policy_loss, "rex_ppo_recurrent_policy_loss"

    def _make_workspaces(self, policy_bytes, value_bytes):
        self.policy_workspace = torch.empty(policy_bytes // 4, dtype=torch.float32, device=self.device)
        self.workspace = torch.empty(value_bytes // 4, dtype=torch.float32, device=self.device)
