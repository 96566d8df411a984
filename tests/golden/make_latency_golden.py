#!/usr/bin/env python3
"""Golden vectors for the LATENCY MODEL, produced by the reference's own methods.

rex_gym/model/rex.py imports pybullet-flavoured modules at package level, none of which are needed here: Rex._GetDelayedObservation,
_GetPDObservation and _GetControlObservation are plain functions of (the observation deque, a latency, the time step).  This script puts
inert stand-ins for pybullet and gym into sys.modules, builds a Rex object WITHOUT running its constructor, gives it a
collections.deque(maxlen=100) filled with appendleft as ReceiveObservation fills it (rex.py:732), and calls the reference's real methods
for every (deque length, latency) pair.  tests/test_latency_host.py holds tests/latency_ref.py to the records.

The observations are 43-vectors drawn from a seeded generator (the test draws the same ones); the file carries the outputs only: per
(length, latency) the control observation [43] and the PD observation's q and qd [12 + 12].

Run with the reference tree at hand:  REX_REFERENCE=<rex-gym checkout> python tests/golden/make_latency_golden.py
"""
import collections
import json
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.environ.get("REX_REFERENCE", "/root/reference"))
for name in ["pybullet", "pybullet_data", "gym", "gym.spaces", "gym.utils", "gym.utils.seeding"]:
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["pybullet_data"].getDataPath = lambda: "/nonexistent"

from rex_gym.model.rex import Rex                            # noqa: E402

LATENCIES = [0, 0.0003, 0.0013, 0.0037, 0.005, 0.0234, 0.043, 0.0977, 0.0985, 0.099, 0.25]
LENGTHS = [1, 2, 3, 24, 25, 99, 100]
TIME_STEP = 0.001
WORDS, MOTORS, SEED = 43, 12, 20


def observations(length):
    """the `length` most recent observations, oldest first: float32-representable values, as the rings of the product hold"""
    return np.random.RandomState(SEED + length).uniform(-3.0, 3.0, (length, WORDS)).astype(np.float32).astype(np.float64)


def main():
    out = {"time_step": TIME_STEP, "seed": SEED, "latencies": LATENCIES, "lengths": LENGTHS, "records": []}
    for length in LENGTHS:
        rex = object.__new__(Rex)
        rex.time_step, rex.num_motors = TIME_STEP, MOTORS
        rex._observation_history = collections.deque(maxlen=100)
        for row in observations(length):
            rex._observation_history.appendleft(list(row))
        assert len(rex._observation_history) == length
        for latency in LATENCIES:
            rex._pd_latency = rex._control_latency = latency
            q, qd = rex._GetPDObservation()
            control = np.asarray(rex._GetControlObservation(), np.float64)
            assert np.array_equal(control, np.asarray(rex._GetDelayedObservation(latency), np.float64))
            out["records"].append({"length": length, "latency": latency, "control": control.tolist(), "pd_q": np.asarray(q, np.float64).tolist(),
                                   "pd_qd": np.asarray(qd, np.float64).tolist()})
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "latency_golden.json")
    with open(dst, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(out["records"]), "records")


if __name__ == "__main__":
    main()
