"""The agent's actor, handed to the simulator: closed-loop rollouts without a launch (or a host round trip) per step.

The reference's rollout loop is `action = algo.perform(prevob)` -> `batch_env.simulate(action)` for every step
(rex_gym/agents/tools/simulate.py:57-76, agents/ppo/algorithm.py:105-134).  `FusedActor` packs what perform() evaluates
-- the observ filter's statistics (agents/ppo/normalize.py:47-66) and the ForwardGaussianPolicy weights
(agents/scripts/networks.py:66-110) -- into the device buffers `RexBatchEnv.set_policy` hands to the library, in the
ABI's layout (input-major weight matrices), so that `env.step_policy` / `env.step_segment_policy` run perform() inside
the step launch (csrc/rex_policy.h).  `sync()` refreshes the buffers from the torch module and the filter and hands them to
the library again (which snapshots them: `rex_set_policy`): the learner calls it after every update (and whenever it wants the
filter statistics of the rollout refreshed); between two sync() calls the actor is frozen, as the reference's is between two
training phases.

The RECURRENT network of the reference's agents (networks.py:113-159 RecurrentGaussianPolicy, PPOConfig(network="recurrent")) runs the
same way through `RexBatchEnv.set_policy_recurrent` (rex_set_policy_recurrent): one ReLU layer, TensorFlow's GRU cell, the tanh mean
layer.  `pack_recurrent` turns the module into the ABI's input-major arrays and `recurrent_reference` evaluates them in plain torch (both
host-only: the layout is testable without a GPU).  The per-env GRU state is `FusedActor.state`, a live device buffer the launches read
and write at every step; the kernel starts an episode from a zero state, and `env.reset` zeroes the rows of the envs it resets.
"""
import torch


def pack_recurrent(net):
    """A RecurrentGaussianPolicy with ONE feed-forward policy layer in front of the cell (policy_layers=(H1, anything)) -> the arrays of
    `RexRecurrentPolicy`, input-major (the transposes of the torch.nn.Linear weights), in the module's dtype and on its device:
    w1 [O, H1], b1, wg [H1 + S, 2 S] (inputs x then h; units r then u), bg, wc [H1 + S, S] (inputs x then r.h), bc, w3 [S, A], b3, logstd."""
    if not getattr(net, "state_size", None):
        raise ValueError("pack_recurrent: not a recurrent policy")
    lins = [m for m in net.policy if isinstance(m, torch.nn.Linear)]
    if len(lins) != 1:
        raise NotImplementedError("the fused recurrent actor is built for ONE feed-forward policy layer in front of the GRU cell "
                                  "(policy_layers=(200, 100): networks.py:113-159 replaces the last layer by the cell)")
    t = lambda lin: lin.weight.detach().t().contiguous()
    v = lambda x: x.detach().clone()
    return dict(w1=t(lins[0]), b1=v(lins[0].bias), wg=t(net.gates), bg=v(net.gates.bias), wc=t(net.candidate), bc=v(net.candidate.bias),
                w3=t(net.mean), b3=v(net.mean.bias), logstd=v(net.logstd))


def recurrent_reference(pk, x, h, gates=False):
    """One cell step on the packed arrays `pk` (pack_recurrent) in plain torch: x [..., O] the FILTERED observation, h [..., S] the state
    -> (mean, new state) -- and the reset and update gates with gates=True.  TensorFlow's GRUBlockCell: r acts before the candidate's product."""
    S = h.shape[-1]
    a = torch.relu(x @ pk["w1"] + pk["b1"])
    g = torch.sigmoid(torch.cat([a, h], -1) @ pk["wg"] + pk["bg"])
    r, u = g[..., :S], g[..., S:]
    c = torch.tanh(torch.cat([a, r * h], -1) @ pk["wc"] + pk["bc"])
    hn = u * h + (1.0 - u) * c
    mean = torch.tanh(hn @ pk["w3"] + pk["b3"])
    return (mean, hn, r, u) if gates else (mean, hn)


class FusedActor:
    def __init__(self, env, net, observ_filter=None, sample=True, seed=0):
        """env: a RexBatchEnv created with range_normalize=True; net: agents.ppo.ForwardGaussianPolicy (two hidden policy
        layers) or RecurrentGaussianPolicy (one hidden policy layer in front of the cell); observ_filter: agents.ppo.StreamingNormalize or None."""
        self.recurrent = bool(getattr(net, "state_size", None))
        if self.recurrent:
            pk = pack_recurrent(net)              # (raises NotImplementedError for other depths)
            self.env, self.net, self.filter = env, net, observ_filter
            dev, O = env.device, env.obs_dim
            self._names = tuple(pk)
            for name, t in pk.items():
                setattr(self, name, torch.zeros(t.shape, dtype=torch.float32, device=dev))
            self._state = torch.zeros((net.state_size, env.num_envs), dtype=torch.float32, device=dev)   # the ABI's [S][N]
            self.obs_mean, self.obs_scale = (torch.zeros(O, device=dev), torch.zeros(O, device=dev)) if observ_filter is not None else (None, None)
            self.obs_clip = float(observ_filter.clip) if observ_filter is not None and observ_filter.clip else 5.0
            self.sample, self.seed = bool(sample), int(seed)
            self.sync()
            return
        lins = [m for m in net.policy if isinstance(m, torch.nn.Linear)]
        if len(lins) != 2:
            raise NotImplementedError("the fused actor is built for two hidden policy layers (configs.py:31: 200, 100)")
        self.env, self.net, self.filter = env, net, observ_filter
        self.l1, self.l2 = lins
        dev, O, A = env.device, env.obs_dim, env.action_dim
        h1, h2 = self.l1.out_features, self.l2.out_features
        f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        self.w1, self.b1, self.w2, self.b2, self.w3, self.b3, self.logstd = f(O, h1), f(h1), f(h1, h2), f(h2), f(h2, A), f(A), f(A)
        self.obs_mean, self.obs_scale = (f(O), f(O)) if observ_filter is not None else (None, None)
        self.obs_clip = float(observ_filter.clip) if observ_filter is not None and observ_filter.clip else 5.0
        self.sample, self.seed = bool(sample), int(seed)
        self.sync()

    @torch.no_grad()
    def sync(self):
        """copy the module's weights (transposed to input-major) and the filter's statistics into the kernel's buffers (the recurrent
        actor's GRU state is left alone)"""
        if self.recurrent:
            for name, t in pack_recurrent(self.net).items():
                getattr(self, name).copy_(t)
            self._sync_filter()
            self.env.set_policy_recurrent(*(getattr(self, n) for n in self._names), state=self._state, obs_mean=self.obs_mean,
                                          obs_scale=self.obs_scale, obs_clip=self.obs_clip, sample=self.sample, seed=self.seed)
            return
        self.w1.copy_(self.l1.weight.t()); self.b1.copy_(self.l1.bias)
        self.w2.copy_(self.l2.weight.t()); self.b2.copy_(self.l2.bias)
        self.w3.copy_(self.net.mean.weight.t()); self.b3.copy_(self.net.mean.bias)
        self.logstd.copy_(self.net.logstd)
        self._sync_filter()
        # the library snapshots (packs) the arrays on the env's stream
        self.env.set_policy(self.w1, self.b1, self.w2, self.b2, self.w3, self.b3, self.logstd, self.obs_mean, self.obs_scale,
                            obs_clip=self.obs_clip, sample=self.sample, seed=self.seed)

    def _sync_filter(self):
        if self.filter is not None:
            flt = self.filter
            self.obs_mean.copy_(flt.mean if flt.center else torch.zeros_like(flt.mean))
            if flt.scale and flt.count > 1:
                self.obs_scale.copy_(1.0 / (flt.std() + 1e-8))      # normalize.py:60-62
            else:
                self.obs_scale.fill_(1.0)

    @property
    def state(self):
        """the recurrent actor's live GRU state as [N, S] (a view of the device buffer the launches read and write); None for the forward actor"""
        return self._state.t() if self.recurrent else None

    def packed(self, dtype=None, device=None):
        """the recurrent actor's packed arrays (what the library snapshotted at the last sync()), for recurrent_reference"""
        return {n: getattr(self, n).to(dtype=dtype, device=device) for n in self._names}

    def filtered(self, observ):
        """the observ filter as frozen at the last sync(), in observ's dtype"""
        if self.obs_mean is None:
            return observ
        return ((observ - self.obs_mean.to(observ)) * self.obs_scale.to(observ)).clamp(-self.obs_clip, self.obs_clip)

    @torch.no_grad()
    def forward_reference(self, observ, state=None):
        """the kernel's arithmetic in plain torch fp32 on the packed buffers (tests): observation -> mean; the recurrent actor:
        (observation, state [N, S]) -> (mean, new state)"""
        if self.recurrent:
            return recurrent_reference(self.packed(), self.filtered(observ), state)
        x = observ
        if self.obs_mean is not None:
            x = ((x - self.obs_mean) * self.obs_scale).clamp(-self.obs_clip, self.obs_clip)
        h = torch.relu(x @ self.w1 + self.b1)
        h = torch.relu(h @ self.w2 + self.b2)
        return torch.tanh(h @ self.w3 + self.b3)
