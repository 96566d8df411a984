"""The latency model's float64 reference (tests/latency_ref.py) against the reference's own Rex._GetDelayedObservation (the records of
tests/golden/latency_golden.json, made by tests/golden/make_latency_golden.py), and the float32 floors tests/test_gpu_latency.py holds the
roll and pitch of the control-delayed observation to.  No GPU.

Floors (blend of two ring entries, then quat_to_euler, in numpy float32 against float64 on the same float32 ring; over
latency_ref.make_ring rings of latency_ref.tilted_states, seed 11, under the cursors of every pair of latency_ref.PAIRS; absolute, rad):

    states                 roll        pitch
    tilted_states(67, 3)   2.048e-07   2.658e-07
    tilted_states(130, 4)  2.306e-07   2.234e-07
    tilted_states(75, 5)   1.928e-07   3.889e-07

latency_ref.EULER_FLOOR is the larger of each column; the GPU test allows FACTOR (4) times it."""
import json
import os

import numpy as np
import pytest

import latency_ref as lr
import step_readout_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latency_golden.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_delayed_reproduces_the_reference(golden):
    """every (deque length, latency) record, from a ring whose unused slots hold NaN, under heads that wrap through slot 99 -> 0"""
    dt, seed = golden["time_step"], golden["seed"]
    assert len(golden["records"]) == len(golden["latencies"]) * len(golden["lengths"]) == 77
    worst = 0.0
    for k, rec in enumerate(golden["records"]):
        length, latency = rec["length"], rec["latency"]
        rows = np.random.RandomState(seed + length).uniform(-3.0, 3.0, (length, 43)).astype(np.float32).astype(np.float64)   # oldest first
        for head in (0, 1, 42, 98, 99)[k % 5], (k * 7) % 100:
            ring = np.full((lr.LEN, 43), np.nan)
            ring[(head - np.arange(length)) % lr.LEN] = rows[::-1]
            got = lr.delayed(ring, head, length, latency, dt)
            assert np.all(np.isfinite(got)), (length, latency, head)
            worst = max(worst, np.abs(got - np.array(rec["control"])).max(), np.abs(got[0:12] - np.array(rec["pd_q"])).max(),
                        np.abs(got[12:24] - np.array(rec["pd_qd"])).max())
    print("largest deviation from the reference's records: %.3e" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("latency,want", [(0.0003, (0, 0.3)), (0.0013, (1, 0.3)), (0.0037, (3, 0.7)), (0.0234, (23, 0.4)), (0.0977, (97, 0.7)),
                                          (0.0985, (98, 0.5)), (0.099, None), (0.25, None)])
def test_slots_of_a_full_ring(latency, want):
    k0, k1, alpha = lr.slots(latency, 0.001, 100)
    if want is None:
        assert (k0, k1, alpha) == (99, 99, 0.0)
    else:
        assert (k0, k1) == (want[0], want[0] + 1) and abs(alpha - want[1]) < 1e-9


def test_slots_at_the_edges():
    assert lr.slots(0, 0.001, 100) == (0, 0, 0.0) and lr.slots(0.0234, 0.001, 1) == (0, 0, 0.0)
    assert lr.slots(0.0013, 0.001, 2) == (1, 1, 0.0) and lr.slots(0.0013, 0.001, 3)[0:2] == (1, 2)
    assert lr.slots(0.0234, 0.001, 24) == (23, 23, 0.0) and lr.slots(0.0234, 0.001, 25)[0:2] == (23, 24)
    # quotients that fall on the other side of an integer: int(0.043 / 0.001) is 42 with alpha 1 - 6e-15; the blend is continuous there
    k0, k1, alpha = lr.slots(0.043, 0.001, 100)
    assert (k0, k1) == (42, 43) and 1.0 - alpha < 1e-12
    k0, k1, alpha = lr.slots(0.005, 0.001, 100)
    assert (k0, k1, alpha) == (5, 6, 0.0) or ((k0, k1) == (4, 5) and 1.0 - alpha < 1e-12)


def test_cursors_cover_every_branch():
    for pd, ctl in lr.PAIRS:
        n_pd, n_c = int(pd / 0.001), int(ctl / 0.001)
        heads, lengths = lr.cursors(67, n_pd, n_c)
        assert set(heads) == {0, 1, 42, 98, 99} and (lengths == 100).sum() * 2 >= 67 and lengths.min() == 1 and lengths.max() == 100
        assert {1, 2, min(n_pd + 1, 100), min(n_pd + 2, 100), min(n_c + 1, 100), min(n_c + 2, 100)} <= set(lengths)
    # a full ring whose two blended slots straddle 99 -> 0
    heads, lengths = lr.cursors(67, 1, 3)
    assert any(h - 1 < 0 for h, l in zip(heads, lengths) if l == 100)


def test_make_ring():
    S0 = lr.tilted_states(10, 1)
    heads, _ = lr.cursors(10, 1, 3)
    R = lr.make_ring(S0, 9, heads)
    assert R.dtype == np.float32 and R.shape == (100, 43, 10)
    rb, sb = lr.blocks(), lr.state_blocks()
    for g in range(10):
        for name in ("q", "qd", "quat", "w"):
            assert np.array_equal(R[heads[g], rb[name], g], S0[sb[name], g])
            step = np.abs(np.diff(R[(heads[g] - np.arange(100)) % 100, rb[name], g].astype(np.float64), axis=0))
            assert step.max() <= lr.STEP[name] * 1.001 and np.median(step) > 0.2 * lr.STEP[name]
    assert np.abs(R[:, rb["tau"]]).max() <= 3.0 and len(np.unique(R[:, rb["tau"], 0])) == 1200
    assert np.array_equal(R, lr.make_ring(S0, 9, heads))


def test_motor_model_is_the_oracles():
    """step_readout_ref.motor_model (numpy) against the float64 C oracle's motor model, actual and observed torque, on delayed readings"""
    rng = np.random.RandomState(0)
    cmd, q, qd, true = rng.uniform(-1, 1, 600), rng.uniform(-1, 1, 600), rng.uniform(-30, 30, 600), rng.uniform(-30, 30, 600)
    act, obs = sr._motor().motor_torque(cmd, q, qd, true, 1.0, 0.02)
    a, o = sr.motor_model(cmd, q, qd, true)
    assert np.abs(a - act).max() <= 1e-12 and np.abs(o - obs).max() <= 1e-12 and np.abs(obs).max() == 5.7 and (np.abs(obs) < 5.7).mean() > 0.2


def test_float32_floor_of_roll_and_pitch():
    floors = []
    for n, seed in lr.TILT_SEEDS.items():
        f = lr.euler_floor(lr.tilted_states(n, seed), lr.RING_SEED)
        print("tilted_states(%d, %d): roll %.3e, pitch %.3e" % (n, seed, f[0], f[1]))
        floors.append(f)
    worst = np.max(floors, axis=0)
    # the recorded floor is never above what this machine's float32 measures (numpy's arcsin / arctan2 may differ in the last place)
    assert np.all(np.array(lr.EULER_FLOOR) <= worst * 1.02) and np.all(np.array(lr.EULER_FLOOR) > 0), (worst, lr.EULER_FLOOR)
