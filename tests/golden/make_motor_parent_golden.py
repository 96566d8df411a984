#!/usr/bin/env python3
"""Records tests/golden/motor_parent_commit_rollout.npz: a walk-IK rollout with mass / friction ranges alone (16 envs, auto_reset,
episode cap 5, 12 steps, 32 in-launch resets), as the commit BEFORE the per-env motor parameters computes it on an MI355X.
tests/test_gpu_motor_params.py::test_mass_and_friction_draws_are_what_the_parent_commit_drew compares the current library with it
bit for bit: the motor draws use Philox counter words of their own and leave the product kernels' arithmetic alone.

It uses nothing newer than that commit's Python surface, so it runs there unchanged.  Recipe (on a GPU machine):
    git worktree add /tmp/parent <the commit before "Per-env motor randomisation">
    cd /tmp/parent && python -m rex_gym_amd.build
    python <this file> <this repository>/tests/golden/motor_parent_commit_rollout.npz      # cwd = the parent checkout
A deliberate change of the step kernels' arithmetic in a later commit makes the recording stale: record it again from the commit
before that change with the same recipe (the comparison is then against that commit)."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np                                   # noqa: E402
import torch                                         # noqa: E402
from rex_gym_amd import RexBatchEnv                  # noqa: E402

N, T = 16, 12
KW = dict(task="walk", signal_type="ik", seed=9, auto_reset=True, max_episode_steps=5, mass_scale_range=(0.8, 1.2), friction_range=(0.25, 0.625))


def main(out):
    env = RexBatchEnv(N, **KW)
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    acts = [(torch.rand((N, 2), device="cuda", generator=g) * 2 - 1) * 0.4 for _ in range(T)]
    reset_obs = env.reset().cpu().numpy().copy()
    o_, r_, d_ = [], [], []
    for a in acts:
        o, r, d, _ = env.step(a)
        o_.append(o.cpu().numpy().copy()); r_.append(r.cpu().numpy().copy()); d_.append(d.cpu().numpy().astype(np.uint8).copy())
    np.savez(out, actions=np.stack([a.cpu().numpy() for a in acts]), reset_obs=reset_obs, obs=np.stack(o_), reward=np.stack(r_), done=np.stack(d_),
             state=env.state.cpu().numpy().copy())
    print("recorded", out, "dones", int(np.stack(d_).sum()))


if __name__ == "__main__":
    main(sys.argv[1])
