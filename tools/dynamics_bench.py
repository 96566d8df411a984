#!/usr/bin/env python3
"""Time the dynamics readout (rex_dynamics) beside the kinematics readout and a control step, in one process on one GPU: 4 096
walk-IK envs (auto-reset) after --steps random steps, on the plane and on the reference's random terrain.

Cases, all through the C ABI into buffers allocated once (a timed call is one launch, nothing else):
  full          every field of RexDynamicsOut
  mass_matrix   mass_matrix alone
  toe_jacobian  toe_jacobian alone
  small         bias, gravity, com, momentum, mass
  kinematics    every field of RexKinematicsOut (rex_kinematics)
  step          rex_step of the same batch (env.step)

Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed
from a calibration run so that a run lasts about --window seconds, then three rounds over all cases in turn, the median of a case's
three runs is reported (device time per call with the launches queued back to back).  Prints one JSON line (and writes it to --out).
REX_LIB_PATH points the run at another build of the library (A/B).

    python tools/dynamics_bench.py [--envs 4096] [--steps 300] [--window 0.3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SMALL = ("bias", "gravity", "com", "momentum", "mass")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rex_gym_amd import RexBatchEnv, _lib, build
    if not torch.cuda.is_available():
        raise SystemExit("dynamics_bench.py measures on the GPU: none found")
    n = args.envs
    res = {"what": "median of three alternating runs, microseconds per call, hipEvents around a run of back-to-back calls",
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(build.LIB_PATH), "envs": n, "steps_before": args.steps,
           "window_s": args.window, "grounds": {}}
    rng = np.random.RandomState(0)
    for ground, kw in (("plane", {}), ("random_terrain", dict(terrain_type="random", terrain_pool=8))):
        env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False, **kw)
        env.reset()
        actions = [torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device) for _ in range(16)]
        for k in range(args.steps):
            env.step(actions[k % 16])
        torch.cuda.synchronize()
        L, h, sp = env._L, env._h, env._stream_ptr()
        results = {name: env.dynamics(fields=fields) for name, fields in (("full", None), ("mass_matrix", ("mass_matrix",)),
                                                                          ("toe_jacobian", ("toe_jacobian",)), ("small", SMALL))}
        cases = {name: (lambda r=r: _lib.check(L.rex_dynamics(h, None, n, ctypes.byref(r.struct), sp), "rex_dynamics")) for name, r in results.items()}
        results["kinematics"] = kin = env.kinematics()
        cases["kinematics"] = lambda: _lib.check(L.rex_kinematics(h, None, n, ctypes.byref(kin.struct), sp), "rex_kinematics")
        cases["step"] = lambda: env.step(actions[0])
        bytes_out = {name: sum(getattr(r, f).numel() * getattr(r, f).element_size() for f in r.fields) for name, r in results.items()}

        def run(fn, calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3 / calls

        calls = {}
        for name, fn in cases.items():       # warm-up and calibration
            run(fn, 20)
            calls[name] = max(100, int(args.window / run(fn, 100)) + 1)
        times = {name: [] for name in cases}
        for _ in range(3):
            for name, fn in cases.items():
                times[name].append(run(fn, calls[name]))
        out = {}
        for name in cases:
            t = sorted(times[name])
            out[name] = {"us_per_call": round(t[1] * 1e6, 2), "min_us": round(t[0] * 1e6, 2), "max_us": round(t[2] * 1e6, 2), "calls_per_run": calls[name]}
        for name in bytes_out:
            out[name]["bytes_written"] = bytes_out[name]
            out[name]["share_of_step"] = round(out[name]["us_per_call"] / out["step"]["us_per_call"], 4)
        out["full_is_cheaper_than_a_step"] = out["full"]["us_per_call"] < out["step"]["us_per_call"]
        res["grounds"][ground] = out
        env.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
