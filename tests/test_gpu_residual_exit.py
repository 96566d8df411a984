"""The sweep loop's exit test with the toe rows' residual formed on demand (csrc/rex_device.h, REX_RESIDUAL_ON_DEMAND).

The product kernels of the paired-sweep variants form the velocity residual inside the row block for the certificate rows only
and for the other rows in an out-of-line block, from the two impulse sets, when the certificate rows leave an env undecided.
The `_trace` instantiations keep the residual in every row.  Both must stop every env after the same sweep: the batches below
hold freshly reset envs (which sweep to the cap) next to converged ones in the same wave -- 37 envs: ragged, one partial lane
group; every third env reset again at steps 7 and 19 -- and compare product against trace pass bit for bit after every step,
first in the natural grouping (state, observation, reward, done: an env stopped a sweep early or late shows in its state), then
under REX_REGROUP=1, the only sims that keep per-env sweep counts (rex_get_sweeps, as bench.py reads them): there the counts are
compared as well, and the states against the natural grouping's -- but envs are sorted into waves by their counts, so capped envs
no longer sit next to converged ones.  Only the walk-IK cases have an env at the cap next to a converged one (asserted); the
gallop and mark-arm cases assert that counts change from step to step.

The seed and the window were picked on the fp64 oracle (CPU): its own per-env sweep counts have an env at the cap next to one
below a third of it in the same step, and counts that change from step to step (the first test, no GPU needed).
"""
import ctypes

import numpy as np
import pytest

N, STEPS, SEED, ACT_SEED = 37, 40, 17, 3
RESET_AT = (7, 19)
RESET_IDX = np.arange(0, N, 3)
CASES = {
    "walk_ik": dict(task="walk", signal_type="ik"),
    "gallop_ol": dict(task="gallop", signal_type="ol"),       # flight phases: sweeps in which no toe row is loaded
    "walk_ik_arm": dict(task="walk", signal_type="ik", mark="arm"),
}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need an MI355X"
    return t


def _actions(kw):
    from rex_gym_amd.envs.batch_env import _spaces
    box = _spaces(kw["task"], kw["signal_type"], 0.001)[0]
    lo, hi = np.minimum(box.low, box.high), np.maximum(box.low, box.high)
    return np.random.RandomState(ACT_SEED).uniform(lo, hi, (STEPS, N, lo.size)).astype(np.float32)


def _covers(sw, cap):
    """[steps, n] per-env sweep counts: some env at the cap and some below a third of it in the same step; some env's count changes."""
    mixed = bool(((sw >= cap).any(1) & (sw < cap / 3).any(1)).any())
    changes = bool((sw[1:] != sw[:-1]).any())
    return mixed, changes


_ORACLE = {}


def _oracle_sweeps(case):
    """Per-env sweep counts of the fp64 oracle over the window: one single-env oracle per env (orc_solver_stats counts a whole batch)."""
    if case not in _ORACLE:
        import orclib
        from rex_gym_amd import _lib
        kw = CASES[case]
        acts = _actions(kw)
        out = np.zeros((STEPS, N), np.int64)
        cap = 0
        for i in range(N):
            cfg = _lib.RexConfig()
            assert _lib.lib().rex_default_config(_lib.TASKS[kw["task"]], _lib.SIGNALS[kw["signal_type"]], 1, ctypes.byref(cfg)) == 0
            cfg.seed, cfg.env_index_base, cfg.mark = SEED, i, _lib.MARKS[kw.get("mark", "base")]
            cap = cfg.solver_iterations * cfg.action_repeat
            orc = orclib.OracleEnv(orclib.RexConfig.from_buffer_copy(bytes(cfg)), np.float64, kw.get("mark", "base"))
            orc.o.lib.orc_set_threads(1)
            sweeps, substeps = ctypes.c_long(0), ctypes.c_long(0)
            orc.o.lib.orc_solver_stats(ctypes.byref(sweeps), ctypes.byref(substeps), 1)
            orc.reset()
            for k in range(STEPS):
                if k in RESET_AT and i in RESET_IDX:
                    orc.reset([0])
                orc.step(acts[k, i:i + 1])
                orc.o.lib.orc_solver_stats(ctypes.byref(sweeps), ctypes.byref(substeps), 1)
                out[k, i] = sweeps.value
            orc.close()
        _ORACLE[case] = (out, cap)
    return _ORACLE[case]


def test_the_window_covers_capped_and_converged_envs_in_the_oracle():
    sw, cap = _oracle_sweeps("walk_ik")
    assert cap == 300
    assert _covers(sw, cap) == (True, True), (sw.max(1), sw.min(1))


def _pair(torch, kw, **extra):
    from rex_gym_amd import RexBatchEnv
    return RexBatchEnv(N, seed=SEED, **kw, **extra), RexBatchEnv(N, seed=SEED, **kw, **extra)


def _sweeps(torch, env):
    from rex_gym_amd import _lib
    buf = torch.zeros(env.num_envs, dtype=torch.int32, device="cuda")
    _lib.check(env._L.rex_get_sweeps(env._h, buf.data_ptr(), env._stream_ptr()), "rex_get_sweeps")
    return buf.cpu().numpy().astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("case,epw", [("walk_ik", 4), ("walk_ik", 8), ("walk_ik", 16), ("gallop_ol", 4), ("walk_ik_arm", 4)])
def test_product_kernels_stop_every_env_where_the_trace_kernels_do(torch, case, epw, monkeypatch):
    kw = CASES[case]
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    acts = torch.as_tensor(_actions(kw), device="cuda")
    idx = torch.as_tensor(RESET_IDX, device="cuda")
    natural = None
    for regroup in (False, True):      # natural grouping (resets next to converged envs in a wave), then the sims that keep the sweep counts
        monkeypatch.setenv("REX_REGROUP", "1" if regroup else "0")
        prod, dbg = _pair(torch, kw)
        assert prod._L.rex_envs_per_wave(prod._h) == epw and dbg._L.rex_envs_per_wave(dbg._h) == epw
        o0, o1 = prod.reset(), dbg.reset()
        tr = dbg.set_event_trace(True)
        assert torch.equal(o0, o1) and torch.equal(prod.state, dbg.state)
        states, counts = [], np.zeros((STEPS, N), np.int64)
        for k in range(STEPS):
            if k in RESET_AT:
                assert torch.equal(prod.reset(idx), dbg.reset(idx))
            po, pr, pd, _ = prod.step(acts[k])
            do, dr, dd, _ = dbg.step(acts[k])
            for name, x, y in (("state", prod.state, dbg.state), ("obs", po, do), ("reward", pr, dr), ("done", pd, dd)):
                assert torch.equal(x, y), (case, epw, regroup, k, name, int((x != y).sum()))
            if regroup:
                counts[k] = _sweeps(torch, prod)
                assert np.array_equal(counts[k], _sweeps(torch, dbg)), (case, epw, k)
                assert torch.equal(prod.state, natural[k]), (case, epw, k, "regrouped against natural grouping")
            else:
                states.append(prod.state.clone())
        assert int((tr[0] != 0).sum()) == N         # the debug env really ran the trace instantiation
        natural = natural or states
        cap = prod.config.solver_iterations * prod.config.action_repeat
        prod.close(); dbg.close()
    print(case, epw, "sweeps per step: max", counts.max(1).tolist(), "min", counts.min(1).tolist())
    assert counts.max() <= cap
    if case == "walk_ik":
        assert _covers(counts, cap) == (True, True), (counts.max(1), counts.min(1))
    else:
        assert _covers(counts, cap)[1], (counts.max(1), counts.min(1))


@pytest.mark.gpu
@pytest.mark.parametrize("epw", [4, 8, 16])
def test_an_env_stops_where_it_would_without_its_wave_mates(torch, epw, monkeypatch):
    """The same 37 envs as one batch and as 36 + 1 (env_index_base keeps every env's draws): with resets in flight the last env's
    result -- alone in its wave in the second shape -- and everybody else's are the same bits."""
    from rex_gym_amd import RexBatchEnv
    kw = CASES["walk_ik"]
    monkeypatch.setenv("REX_ENVS_PER_WAVE", str(epw))
    acts = torch.as_tensor(_actions(kw), device="cuda")
    whole = RexBatchEnv(N, seed=SEED, **kw)
    head, tail = RexBatchEnv(N - 1, seed=SEED, **kw), RexBatchEnv(1, seed=SEED, env_index_base=N - 1, **kw)
    assert (N - 1) in RESET_IDX
    idx = torch.as_tensor(RESET_IDX, device="cuda")
    assert torch.equal(whole.reset(), torch.cat([head.reset(), tail.reset()]))
    for k in range(STEPS):
        if k in RESET_AT:
            assert torch.equal(whole.reset(idx), torch.cat([head.reset(idx[:-1]), tail.reset(torch.zeros(1, dtype=idx.dtype, device="cuda"))]))
        wo, wr, wd, _ = whole.step(acts[k])
        ho, hr, hd, _ = head.step(acts[k, :N - 1])
        to, tr_, td, _ = tail.step(acts[k, N - 1:])
        for name, x, y in (("state", whole.state, torch.cat([head.state, tail.state], 1)), ("obs", wo, torch.cat([ho, to])),
                           ("reward", wr, torch.cat([hr, tr_])), ("done", wd, torch.cat([hd, td]))):
            assert torch.equal(x, y), (epw, k, name)
    whole.close(); head.close(); tail.close()
