#!/usr/bin/env python3
"""Time the contact-space readout and inverse dynamics (rex_contact_space, rex_inverse_dynamics) beside the three-call route to the
Delassus matrix that the README kept until now, in one process on one GPU: 4 096 walk-IK envs (auto-reset) after --steps random steps,
on the plane and on the reference's random terrain.

Cases, the library's through the C ABI into buffers allocated once (a timed call is one launch, nothing else):
  delassus, toe_drift, toe_acc_free   rex_contact_space with that output alone (toe_acc_free: joint torques and a base wrench given)
  contact_space_full                  ... with every output
  inverse, inverse_toe                rex_inverse_dynamics with vdot, joint torques and a base wrench; ... and toe forces (a ground query)
  toe_jacobian                        rex_dynamics with toe_jacobian alone            } the existing route to J M^-1 J^T:
  solve_K24                           rex_dynamics_solve, K = 24, rhs = toe_jacobian  } three calls, two intermediate arrays
  einsum                              torch.einsum("kpd,kqd->kpq", J, X)              }
  three_call_route                    the three back to back
  step                                rex_step of the same batch (env.step)
The fused matrix is compared with the three-call one before anything is timed (largest |difference| / largest entry, reported).

Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed
from a calibration run so that a run lasts about --window seconds, then three rounds over all cases in turn, the median of a case's
three runs is reported (device time per call with the launches queued back to back).  Prints one JSON line (and writes it to --out).
REX_LIB_PATH points the run at another build of the library (A/B).

    python tools/contact_space_bench.py [--envs 4096] [--steps 300] [--window 0.3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
        raise SystemExit("contact_space_bench.py measures on the GPU: none found")
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
        tau, toe, wrench, vdot, out18 = dev(n, 12), dev(n, 8, 3), dev(n, 6), dev(n, 18), torch.empty((n, 18), device=env.device)
        with env._on_stream():
            full = env.contact_space(tau=tau, base_wrench=wrench)
            alone = {k: env.contact_space(tau=tau, base_wrench=wrench, fields=(k,)) for k in ("delassus", "toe_drift", "toe_acc_free")}
            jac = env.dynamics(fields=("toe_jacobian",))
        J = jac.toe_jacobian.view(n, 24, 18)
        X = torch.empty_like(J)
        loads = {"inverse": _lib.RexDynamicsLoad(joint=tau.data_ptr(), base=wrench.data_ptr()),
                 "inverse_toe": _lib.RexDynamicsLoad(joint=tau.data_ptr(), toe=toe.data_ptr(), base=wrench.data_ptr())}
        space = lambda o: _lib.check(L.rex_contact_space(h, None, n, tau.data_ptr(), wrench.data_ptr(), ctypes.byref(o.struct), sp), "rex_contact_space")
        cases = {k: (lambda o=o: space(o)) for k, o in alone.items()}
        cases["contact_space_full"] = lambda: space(full)
        for name in loads:
            cases[name] = lambda name=name: _lib.check(L.rex_inverse_dynamics(h, None, n, vdot.data_ptr(), ctypes.byref(loads[name]), out18.data_ptr(), sp),
                                                       "rex_inverse_dynamics")
        cases["toe_jacobian"] = lambda: _lib.check(L.rex_dynamics(h, None, n, ctypes.byref(jac.struct), sp), "rex_dynamics")
        cases["solve_K24"] = lambda: _lib.check(L.rex_dynamics_solve(h, None, n, 24, J.data_ptr(), X.data_ptr(), sp), "rex_dynamics_solve")
        cases["einsum"] = lambda: torch.einsum("kpd,kqd->kpq", J, X)

        def three_calls():
            cases["toe_jacobian"]()
            cases["solve_K24"]()
            return torch.einsum("kpd,kqd->kpq", J, X)
        cases["three_call_route"] = three_calls
        cases["step"] = lambda: env.step(actions[0])
        with env._on_stream():
            space(alone["delassus"])
            theirs = three_calls()
            torch.cuda.synchronize()
            gap = float((alone["delassus"].delassus - theirs).abs().max() / theirs.abs().max())
            if not gap < 1e-4:
                raise SystemExit("rex_contact_space's delassus differs from the three-call route by %.3g of the largest entry" % gap)

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
        out["three_call_route"]["over_delassus"] = round(out["three_call_route"]["us_per_call"] / out["delassus"]["us_per_call"], 2)
        out["two_launches_over_delassus"] = round((out["toe_jacobian"]["us_per_call"] + out["solve_K24"]["us_per_call"]) / out["delassus"]["us_per_call"], 2)
        out["delassus_gap_to_three_call_route"] = gap
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
