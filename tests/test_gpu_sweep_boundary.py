"""The sweep loop of the paired-sweep base kernels (csrc/rex_device.h, pgs_dv) at its boundaries: product against `_trace` kernels.

The product kernels read the joint-limit rows a leg ahead (REX_LIMIT_ROWS_AHEAD) and form the toe rows' residual on demand; the
`_trace` instantiations read the limit rows at their use and keep the residual in every row.  Both must give the same bits and the
same sweep counts: from reset (the long-solve case: every env sweeps for a long time), at sweep caps that end a solve behind the first
sweep of a pair, behind the second, and one short of the default (1, 2, 3, 59), with joint-limit rows in reach, and in one segment
launch of 10 steps against 10 single steps.  (Written with the carried row-0 sum of profiles/sweep_boundary.md, which was measured and
not kept; they hold any later form of the sweep boundary to the trace kernels.)

Limit rows in reach: the issue that asked for these tests named gallop-OL from reset.  That batch never has one: on the fp32 oracle
the 64 envs below stay 0.8 rad away from every bound for 400 steps (profiles/r03p_sections.txt reads 0.00 % for gallop; its 3.64 %
is the standup section).  Standup-OL has them: its reset ends crouched BEYOND the upper bound of the four foot joints (2.5905 rad
against 2.59), so the first substep of the first step runs limit rows in every env of every wave.  The event trace words are chained
hashes (a planner word is folded in every step next to the substeps' events) and cannot be read back into single events; that a
bound is in reach is asserted on the reset state instead, by the kernels' own rule (gap <= kLimitActivation = 0), and on the oracle's
(first test, no GPU needed).
"""
import os
import re

import numpy as np
import pytest

N, STEPS, SEED, ACT_SEED = 64, 30, 17, 3
LIMIT_STEPS = 20
WALK = dict(task="walk", signal_type="ik")
STANDUP = dict(task="standup", signal_type="ol")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need an MI355X"
    return t


def _actions(kw, steps):
    from rex_gym_amd.envs.batch_env import _spaces
    box = _spaces(kw["task"], kw["signal_type"], 0.001)[0]
    lo, hi = np.minimum(box.low, box.high), np.maximum(box.low, box.high)
    return np.random.RandomState(ACT_SEED).uniform(lo, hi, (steps, N, lo.size)).astype(np.float32)


def _joint_bounds():
    src = open(os.path.join(ROOT, "rex_gym_amd", "csrc", "rex_model_gen.h")).read()
    arr = lambda name: np.array([float(v) for v in re.search(name + r"\[REX_NJ\] = \{([^}]*)\}", src).group(1).split(",")], np.float32)
    return arr("REX_JOINT_LOWER"), arr("REX_JOINT_UPPER")


def _envs_on_a_bound(q):
    """q [12, n] float32: the envs with a leg joint at or beyond a bound (physics_substep: gap <= kLimitActivation = 0)."""
    lo, hi = _joint_bounds()
    return (np.minimum(q - lo[:, None], hi[:, None] - q) <= 0).any(0)


def _sweeps(torch, env):
    from rex_gym_amd import _lib
    buf = torch.zeros(env.num_envs, dtype=torch.int32, device="cuda")
    _lib.check(env._L.rex_get_sweeps(env._h, buf.data_ptr(), env._stream_ptr()), "rex_get_sweeps")
    return buf.cpu().numpy().astype(np.int64)


def _same_bits(torch, x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)   # (a NaN equals itself)


def _product_against_trace(torch, monkeypatch, kw, epw, steps, **extra):
    """Steps a product env and a trace env side by side from reset; state, observation, reward and done after every step, in the
    natural grouping and under REX_REGROUP=1 (the sims that keep per-env sweep counts), there the counts as well.  Returns the counts
    [steps, N] and the reset state."""
    from rex_gym_amd import RexBatchEnv
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    acts = torch.as_tensor(_actions(kw, steps), device="cuda")
    counts = np.zeros((steps, N), np.int64)
    for regroup in (False, True):
        monkeypatch.setenv("REX_REGROUP", "1" if regroup else "0")
        prod, dbg = RexBatchEnv(N, seed=SEED, **kw, **extra), RexBatchEnv(N, seed=SEED, **kw, **extra)
        assert prod._L.rex_envs_per_wave(prod._h) == epw and dbg._L.rex_envs_per_wave(dbg._h) == epw
        assert torch.equal(prod.reset(), dbg.reset()) and torch.equal(prod.state, dbg.state)
        state0 = prod.state.clone()
        tr = dbg.set_event_trace(True)
        for k in range(steps):
            po, pr, pd, _ = prod.step(acts[k])
            do, dr, dd, _ = dbg.step(acts[k])
            for name, x, y in (("state", prod.state, dbg.state), ("obs", po, do), ("reward", pr, dr), ("done", pd, dd)):
                assert _same_bits(torch, x, y), (kw["task"], epw, extra, regroup, k, name, int((x != y).sum()))
            if regroup:
                counts[k] = _sweeps(torch, prod)
                assert np.array_equal(counts[k], _sweeps(torch, dbg)), (kw["task"], epw, extra, k)
        assert int((tr[0] != 0).sum()) == N         # the debug env really ran the trace instantiation
        prod.close(); dbg.close()
    return counts, state0


def test_standup_resets_onto_a_joint_bound_and_gallop_stays_clear_in_the_oracle():
    import orclib
    for task, steps in (("standup", 0), ("gallop", 30)):
        orc = orclib.OracleEnv(orclib.default_config(task, "ol", N, seed=SEED), np.float32)
        orc.reset()
        acts = _actions(dict(task=task, signal_type="ol"), max(steps, 1))
        on = _envs_on_a_bound(np.asarray(orc.get_state())[orclib.S_Q:orclib.S_Q + 12].astype(np.float32))
        for k in range(steps):
            orc.step(acts[k])
            on |= _envs_on_a_bound(np.asarray(orc.get_state())[orclib.S_Q:orclib.S_Q + 12].astype(np.float32))
        orc.close()
        assert int(on.sum()) == (N if task == "standup" else 0), (task, int(on.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("epw", [4, 8, 16])
def test_product_and_trace_kernels_agree_from_reset(torch, epw, monkeypatch):
    counts, _ = _product_against_trace(torch, monkeypatch, WALK, epw, STEPS)
    print("walk-IK from reset,", epw, "envs per wave, sweeps per step: max", counts.max(1).tolist(), "min", counts.min(1).tolist())
    assert counts.min() > 0 and (counts[1:] != counts[:-1]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("epw", [4, 8, 16])
@pytest.mark.parametrize("cap", [1, 2, 3, 59])
def test_product_and_trace_kernels_agree_at_odd_and_tiny_sweep_caps(torch, cap, epw, monkeypatch):
    counts, _ = _product_against_trace(torch, monkeypatch, WALK, epw, STEPS, solver_iterations=cap)
    per_step = cap * 5                                        # action_repeat substeps, each capped
    print("cap", cap, epw, "envs per wave, sweeps per step: max", counts.max(1).tolist(), "min", counts.min(1).tolist())
    assert counts.max() <= per_step
    if cap == 1:                                              # a solve runs one sweep at least
        assert (counts == per_step).all(), (cap, epw, counts.min())
    elif cap <= 3:                                            # a standing robot's solve takes 16 sweeps and more: some env ends every solve at the cap
        assert (counts == per_step).any(), (cap, epw, counts.max())
    else:
        assert counts.max() > 3 * 5


@pytest.mark.gpu
@pytest.mark.parametrize("epw", [4, 8, 16])
def test_product_and_trace_kernels_agree_with_limit_rows_in_reach(torch, epw, monkeypatch):
    import orclib
    from helpers import product_state_to_numeric
    counts, state0 = _product_against_trace(torch, monkeypatch, STANDUP, epw, LIMIT_STEPS)
    q0 = product_state_to_numeric(state0)[orclib.S_Q:orclib.S_Q + 12].astype(np.float32)
    on = _envs_on_a_bound(q0)
    print("standup-OL from reset,", epw, "envs per wave: envs on a joint bound at reset", int(on.sum()), "sweeps per step: max", counts.max(1).tolist())
    assert on.all(), int(on.sum())      # the first substep solves limit rows in every wave
    assert counts.min() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("epw", [4, 8, 16])
def test_one_segment_launch_of_ten_steps_equals_ten_single_steps_with_limit_rows_in_reach(torch, epw, monkeypatch):
    from rex_gym_amd import RexBatchEnv
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    acts = torch.as_tensor(_actions(STANDUP, 10), device="cuda")
    seg, single = RexBatchEnv(N, seed=SEED, **STANDUP), RexBatchEnv(N, seed=SEED, **STANDUP)
    assert torch.equal(seg.reset(), single.reset())
    so, sr, sd, _ = seg.step_segment(acts)
    for k in range(10):
        o, r, d, _ = single.step(acts[k])
        for name, x, y in (("obs", so[k], o), ("reward", sr[k], r), ("done", sd[k], d)):
            assert _same_bits(torch, x, y), (epw, k, name, int((x != y).sum()))
    assert _same_bits(torch, seg.state, single.state)
    seg.close(); single.close()
