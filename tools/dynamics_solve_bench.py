#!/usr/bin/env python3
"""Time the solves with the mass matrix (rex_dynamics_solve, rex_forward_dynamics, rex_apply_impulse) beside the dynamics readout, a
control step and the dense route through torch, in one process on one GPU: 4 096 walk-IK envs (auto-reset) after --steps random steps,
on the plane and on the reference's random terrain.

Cases, the library's through the C ABI into buffers allocated once (a timed call is one launch, nothing else):
  solve_K1, solve_K6, solve_K24   rex_dynamics_solve with K right-hand sides per env
  forward                         rex_forward_dynamics with joint torques, toe forces and a base wrench
  forward_tau                     ... with joint torques alone (no ground query)
  push                            rex_apply_impulse with a base impulse and toe impulses, dv written; the impulses are zero, so that the
                                  state stays what it is over thousands of calls (the kernel has no branch on their values)
  dynamics_full, mass_matrix      rex_dynamics: every field; mass_matrix alone (what the dense route reads first)
  step                            rex_step of the same batch (env.step)
  dense_solve_K*                  torch.linalg.solve(M, rhs^T) on the mass_matrix tensor already in memory
  dense_cholesky_K*               torch.linalg.cholesky(M) then torch.cholesky_solve
  dense_route_K*                  what a user does without rex_dynamics_solve: the mass_matrix launch, then the faster of the two above
A torch build that cannot run a dense case is reported under "unavailable" with its error; the other cases stand.

Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed
from a calibration run so that a run lasts about --window seconds, then three rounds over all cases in turn, the median of a case's
three runs is reported (device time per call with the launches queued back to back).  Prints one JSON line (and writes it to --out).
REX_LIB_PATH points the run at another build of the library (A/B).

    python tools/dynamics_solve_bench.py [--envs 4096] [--steps 300] [--window 0.3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 6, 24)


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
        raise SystemExit("dynamics_solve_bench.py measures on the GPU: none found")
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
        dev = lambda *shape: torch.as_tensor(rng.standard_normal(shape).astype(np.float32), device=env.device)
        rhs = {K: dev(n, K, 18) for K in KS}
        x = {K: torch.empty_like(rhs[K]) for K in KS}
        tau, toe, wrench, out18 = dev(n, 12), dev(n, 8, 3), dev(n, 6), torch.empty((n, 18), device=env.device)
        zero_toe, zero_wrench = torch.zeros_like(toe), torch.zeros_like(wrench)
        loads = {"forward": _lib.RexDynamicsLoad(joint=tau.data_ptr(), toe=toe.data_ptr(), base=wrench.data_ptr()),
                 "forward_tau": _lib.RexDynamicsLoad(joint=tau.data_ptr()),
                 "push": _lib.RexDynamicsLoad(toe=zero_toe.data_ptr(), base=zero_wrench.data_ptr())}
        full, mm = env.dynamics(), env.dynamics(fields=("mass_matrix",))
        cases = {}
        for K in KS:
            cases["solve_K%d" % K] = lambda K=K: _lib.check(L.rex_dynamics_solve(h, None, n, K, rhs[K].data_ptr(), x[K].data_ptr(), sp), "rex_dynamics_solve")
        for name in ("forward", "forward_tau"):
            cases[name] = lambda name=name: _lib.check(L.rex_forward_dynamics(h, None, n, ctypes.byref(loads[name]), out18.data_ptr(), sp), "rex_forward_dynamics")
        cases["push"] = lambda: _lib.check(L.rex_apply_impulse(h, None, n, ctypes.byref(loads["push"]), out18.data_ptr(), sp), "rex_apply_impulse")
        cases["dynamics_full"] = lambda: _lib.check(L.rex_dynamics(h, None, n, ctypes.byref(full.struct), sp), "rex_dynamics")
        cases["mass_matrix"] = lambda: _lib.check(L.rex_dynamics(h, None, n, ctypes.byref(mm.struct), sp), "rex_dynamics")
        cases["step"] = lambda: env.step(actions[0])
        M = mm.mass_matrix
        dense = {}
        for K in KS:
            bt = rhs[K].transpose(1, 2).contiguous()              # [n, 18, K]
            dense["dense_solve_K%d" % K] = lambda bt=bt: torch.linalg.solve(M, bt)
            dense["dense_cholesky_K%d" % K] = lambda bt=bt: torch.cholesky_solve(bt, torch.linalg.cholesky(M))
        unavailable = {}
        with env._on_stream():
            for name, fn in dense.items():
                try:
                    got = fn()
                    torch.cuda.synchronize()
                    K = int(name.rsplit("K", 1)[1])
                    cases["solve_K%d" % K]()
                    torch.cuda.synchronize()
                    dev_rel = float((got.transpose(1, 2) - x[K]).norm() / x[K].norm())
                    if not dev_rel < 1e-2:
                        raise RuntimeError("differs from rex_dynamics_solve by %.3g (relative, Frobenius)" % dev_rel)
                    cases[name] = fn
                except Exception as e:                             # a torch build without the batched solver: reported, not hidden
                    unavailable[name] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])

        def run(fn, calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3 / calls

        out = {}
        with env._on_stream():
            calls = {}
            for name, fn in cases.items():       # warm-up and calibration
                run(fn, 20)
                calls[name] = max(100, int(args.window / run(fn, 100)) + 1)
            times = {name: [] for name in cases}
            for _ in range(3):
                for name, fn in cases.items():
                    times[name].append(run(fn, calls[name]))
        for name in cases:
            t = sorted(times[name])
            out[name] = {"us_per_call": round(t[1] * 1e6, 2), "min_us": round(t[0] * 1e6, 2), "max_us": round(t[2] * 1e6, 2), "calls_per_run": calls[name],
                         "share_of_step": round(t[1] / sorted(times["step"])[1], 4)}
        for K in KS:
            routes = [out[k]["us_per_call"] for k in ("dense_solve_K%d" % K, "dense_cholesky_K%d" % K) if k in out]
            if routes:
                total = out["mass_matrix"]["us_per_call"] + min(routes)
                out["dense_route_K%d" % K] = {"us_per_call": round(total, 2), "over_solve": round(total / out["solve_K%d" % K]["us_per_call"], 2)}
        out["unavailable"] = unavailable
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
