"""The front and back end of a substep -- leg pass, row finishing and couplings, the set-up and hand-back of the sweep loop, the
back-substitution (csrc/rex_device.h, physics_substep / pgs_dv) -- and the step's own ends: product against `_trace` kernels.

The `_trace` instantiations keep the form of these parts, and the compiler's schedule of them, that the product kernels had before
`REX_ONE_WAVE_PER_SIMD` (csrc/rex_kernels.h): today the one difference this file sees between the two, next to the residual on demand and
the limit rows read ahead of tests/test_gpu_sweep_boundary.py, is that `<4, base>` is compiled as a one-wave-per-SIMD kernel and its
`_trace` twin is not.  Same source, same arithmetic: the bits must agree.  A later change to these parts of the product kernels (another
LDS layout for the finished rows, another lane forming a value, another fence: profiles/critical_wave.md lists what was considered) is
held to the same check.  Batches of 5, 64 and 130 envs: one partly filled wave, whole waves, and a ragged last wave at 4, 8 and 16 envs
per wave.

  * walk-IK on the plane and turn-IK on the heightfield pool (toe rows in facet frames: the couplings of consecutive rows cross frames);
  * standup from reset: the reset ends beyond the upper bound of the foot joints (tests/test_gpu_sweep_boundary.py), so joint-limit
    rows are finished and swept from the first substep on;
  * a 10-step segment launch against 10 single steps (the SEG instantiations carry the env through the same front end step after step);
  * sweep caps of 1 and 59: the set-up and the hand-back around one sweep, and around a solve one short of the default.

The helpers that do not depend on the batch size come from tests/test_gpu_sweep_boundary.py; its `_actions` and `_product_against_trace`
are written for its one batch of 64 envs, so the versions here take the batch size.
"""
import numpy as np
import pytest

from test_gpu_sweep_boundary import _envs_on_a_bound, _same_bits, _sweeps

STEPS, SEED, ACT_SEED = 40, 23, 5
BATCHES = [5, 64, 130]
EPWS = [4, 8, 16]
WALK = dict(task="walk", signal_type="ik")
TURN_HF = dict(task="turn", signal_type="ik", terrain_type="random", terrain_pool=8)
STANDUP = dict(task="standup", signal_type="ol")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need an MI355X"
    return t


def _actions(kw, n, steps):
    from rex_gym_amd.envs.batch_env import _spaces
    box = _spaces(kw["task"], kw["signal_type"], 0.001)[0]
    lo, hi = np.minimum(box.low, box.high), np.maximum(box.low, box.high)
    return np.random.RandomState(ACT_SEED).uniform(lo, hi, (steps, n, lo.size)).astype(np.float32)


def _product_against_trace(torch, monkeypatch, kw, n, epw, steps=STEPS, regroup=False, **extra):
    """A product env and a trace env side by side from reset: state, observation, reward and done bit for bit after every step.
    regroup (REX_REGROUP=1: the sims that keep per-env sweep counts): the counts as well; returns them [steps, n], and the reset state."""
    from rex_gym_amd import RexBatchEnv
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    monkeypatch.setenv("REX_REGROUP", "1" if regroup else "0")
    acts = torch.as_tensor(_actions(kw, n, steps), device="cuda")
    prod, dbg = RexBatchEnv(n, seed=SEED, **kw, **extra), RexBatchEnv(n, seed=SEED, **kw, **extra)
    assert prod._L.rex_envs_per_wave(prod._h) == epw and dbg._L.rex_envs_per_wave(dbg._h) == epw
    assert torch.equal(prod.reset(), dbg.reset()) and torch.equal(prod.state, dbg.state)
    state0 = prod.state.clone()
    tr = dbg.set_event_trace(True)
    counts = np.zeros((steps, n), np.int64)
    for k in range(steps):
        po, pr, pd, _ = prod.step(acts[k])
        do, dr, dd, _ = dbg.step(acts[k])
        for name, x, y in (("state", prod.state, dbg.state), ("obs", po, do), ("reward", pr, dr), ("done", pd, dd)):
            assert _same_bits(torch, x, y), (kw["task"], n, epw, extra, k, name, int((x != y).sum()))
        if regroup:
            counts[k] = _sweeps(torch, prod)
            assert np.array_equal(counts[k], _sweeps(torch, dbg)), (kw["task"], n, epw, extra, k)
    assert int((tr[0] != 0).sum()) == n         # the debug env really ran the trace instantiation
    moved = not torch.equal(prod.state, state0)
    prod.close(); dbg.close()
    assert moved
    return counts, state0


@pytest.mark.gpu
@pytest.mark.parametrize("epw", EPWS)
@pytest.mark.parametrize("n", BATCHES)
def test_walk_on_the_plane_product_and_trace_kernels_agree(torch, n, epw, monkeypatch):
    _product_against_trace(torch, monkeypatch, WALK, n, epw)


@pytest.mark.gpu
@pytest.mark.parametrize("epw", EPWS)
@pytest.mark.parametrize("n", BATCHES)
def test_turn_on_the_heightfield_pool_product_and_trace_kernels_agree(torch, n, epw, monkeypatch):
    _product_against_trace(torch, monkeypatch, TURN_HF, n, epw)


@pytest.mark.gpu
@pytest.mark.parametrize("epw", EPWS)
@pytest.mark.parametrize("n", BATCHES)
def test_standup_from_reset_product_and_trace_kernels_agree_with_limit_rows_in_reach(torch, n, epw, monkeypatch):
    import orclib
    from helpers import product_state_to_numeric
    _, state0 = _product_against_trace(torch, monkeypatch, STANDUP, n, epw)
    q0 = product_state_to_numeric(state0)[orclib.S_Q:orclib.S_Q + 12].astype(np.float32)
    assert _envs_on_a_bound(q0).all()           # the first substep finishes and solves limit rows in every wave


@pytest.mark.gpu
@pytest.mark.parametrize("epw", EPWS)
@pytest.mark.parametrize("n", BATCHES)
def test_one_segment_launch_of_ten_steps_equals_ten_single_steps(torch, n, epw, monkeypatch):
    from rex_gym_amd import RexBatchEnv
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    acts = torch.as_tensor(_actions(WALK, n, 10), device="cuda")
    seg, single = RexBatchEnv(n, seed=SEED, **WALK), RexBatchEnv(n, seed=SEED, **WALK)
    assert seg._L.rex_envs_per_wave(seg._h) == epw
    assert torch.equal(seg.reset(), single.reset())
    so, sr, sd, _ = seg.step_segment(acts)
    for k in range(10):
        o, r, d, _ = single.step(acts[k])
        for name, x, y in (("obs", so[k], o), ("reward", sr[k], r), ("done", sd[k], d)):
            assert _same_bits(torch, x, y), (n, epw, k, name, int((x != y).sum()))
    assert _same_bits(torch, seg.state, single.state)
    seg.close(); single.close()


@pytest.mark.gpu
@pytest.mark.parametrize("epw", EPWS)
@pytest.mark.parametrize("cap", [1, 59])
def test_set_up_and_hand_back_around_one_sweep_and_around_a_full_solve(torch, cap, epw, monkeypatch):
    counts, _ = _product_against_trace(torch, monkeypatch, WALK, 130, epw, regroup=True, solver_iterations=cap)
    per_step = cap * 5                          # action_repeat substeps, each capped
    assert counts.max() <= per_step
    if cap == 1:
        assert (counts == per_step).all(), (epw, counts.min())      # a solve runs one sweep at least
    else:
        assert counts.max() > 3 * 5, (epw, counts.max())            # from reset the solves are long
