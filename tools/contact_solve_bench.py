#!/usr/bin/env python3
"""Time the contact solve (rex_contact_solve) beside a control step and the composition a caller had to write without it, in one process
on one GPU: 4 096 walk-IK envs (auto-reset) after --steps random steps, on the plane and on the reference's random terrain.

Cases, the library's through the C ABI into buffers allocated once (a timed call is one launch, nothing else):
  contact_60          rex_contact_solve, every output, joint torques given, 60 sweeps for every env (residual threshold 0)
  contact_exit        ... with the config's residual threshold: every env leaves on its own residual (`sweeps` gives the counts)
  contact_1           ... one sweep: the front end, the free velocity, the 36 rows and the readout
  contact_60_forces   as contact_60 with toe_force alone
  step                rex_step of the same batch (env.step): action_repeat substeps, controller, observation, reward
  composed_60         what a caller writes today: env.dynamics(toe_jacobian), env.forward_dynamics(tau) for the free velocity,
                      env.dynamics_solve(J) with K = 24 for the responses, kinematics(toe_normal, toe_dist, toe_in_reach), then a torch
                      projected Gauss-Seidel over the 24 toe rows, batched over the envs, 60 sweeps (joint-limit rows and the damping
                      forces left out: a lower bound of that route)
Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed
from a calibration run so that a run lasts about --window seconds, then three rounds over all cases in turn, the median of a case's
three runs is reported (device time per call with the launches queued back to back).  Prints one JSON line (and writes it to --out).

    python tools/contact_solve_bench.py [--envs 4096] [--steps 300] [--window 0.3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWEEPS = 60


def composed(env, tau, dt, mu, sweeps):
    """the torch route over the toe rows (module docstring) -> v_next [n, 18]"""
    import torch
    n = env.num_envs
    kin = env.kinematics(fields=("toe_normal", "toe_dist", "toe_in_reach"))
    J = env.dynamics(fields=("toe_jacobian",)).toe_jacobian.view(n, 8, 3, 18)
    nrm, dist, act = kin.toe_normal.view(n, 8, 3), kin.toe_dist.view(n, 8), kin.toe_in_reach.view(n, 8).bool()
    steep = nrm[..., 2].abs() > 0.7071067811865475244
    a = torch.where(steep, nrm[..., 1] ** 2 + nrm[..., 2] ** 2, nrm[..., 0] ** 2 + nrm[..., 1] ** 2)
    k = torch.rsqrt(a)
    zero = torch.zeros_like(k)
    t1 = torch.where(steep[..., None], torch.stack([zero, -nrm[..., 2] * k, nrm[..., 1] * k], -1), torch.stack([-nrm[..., 1] * k, nrm[..., 0] * k, zero], -1))
    t2 = torch.where(steep[..., None], torch.stack([a * k, -nrm[..., 0] * t1[..., 2], nrm[..., 0] * t1[..., 1]], -1),
                     torch.stack([-nrm[..., 2] * t1[..., 1], nrm[..., 2] * t1[..., 0], a * k], -1))
    rows = torch.cat([torch.einsum("npc,npcd->npd", u, J) for u in (nrm, t1, t2)], 1).contiguous()      # [n, 24, 18]: normals, then t1, t2
    resp = env.dynamics_solve(rows)
    diag = (rows * resp).sum(-1)
    v = torch.cat([env.state[7:13].T, env.state[25:37].T], 1)
    vs = v + dt * env.forward_dynamics(tau=tau)
    vel = torch.einsum("nrd,nd->nr", rows, vs)
    target = torch.where(dist > 0, -dist / dt, -dist * (0.2 / dt))
    rhs = torch.cat([(target - vel[:, 0:8]), -vel[:, 8:24]], 1) / diag
    rhs = rhs * torch.cat([act, act, act], 1)
    top = torch.where(act, 1e10, 0.0)
    lam, dv = torch.zeros((n, 24), device=env.device), torch.zeros((n, 18), device=env.device)
    order = list(range(8)) + [r for p in range(8) for r in (8 + p, 16 + p)]
    for _ in range(sweeps):
        for r in order:
            hi = top[:, r] if r < 8 else mu * lam[:, r % 8]
            lo = torch.zeros_like(hi) if r < 8 else -hi
            new = torch.minimum(torch.maximum(lam[:, r] + rhs[:, r] - (rows[:, r] * dv).sum(-1) / diag[:, r], lo), hi)
            dv = dv + resp[:, r] * (new - lam[:, r])[:, None]
            lam[:, r] = new
    return (vs + dv).clamp(-100.0, 100.0)


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
        raise SystemExit("contact_solve_bench.py measures on the GPU: none found")
    n = args.envs
    res = {"what": "median of three alternating runs, microseconds per call, hipEvents around a run of back-to-back calls",
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(build.LIB_PATH), "envs": n, "steps_before": args.steps,
           "window_s": args.window, "sweeps": SWEEPS, "grounds": {}}
    rng = np.random.RandomState(0)
    for ground, kw in (("plane", {}), ("random_terrain", dict(terrain_type="random", terrain_pool=8))):
        env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False, **kw)
        env.reset()
        actions = [torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device) for _ in range(16)]
        for k in range(args.steps):
            env.step(actions[k % 16])
        torch.cuda.synchronize()
        L, h, sp = env._L, env._h, env._stream_ptr()
        tau = torch.as_tensor(rng.uniform(-3, 3, (n, 12)).astype(np.float32), device=env.device)
        dt = float(env.config.sim_time_step)
        full = env.contact_solve(tau=tau, iterations=SWEEPS, residual_threshold=0.0)
        forces = env.contact_solve(tau=tau, fields=("toe_force",), iterations=SWEEPS, residual_threshold=0.0)
        early = env.contact_solve(tau=tau, iterations=SWEEPS)
        torch.cuda.synchronize()
        sweeps = early.sweeps.cpu().numpy()
        ins = {"contact_60": (_lib.RexContactSolveIn(tau.data_ptr(), 0.0, SWEEPS, 0.0, 1), full), "contact_exit": (_lib.RexContactSolveIn(tau.data_ptr(), 0.0, SWEEPS, -1.0, 1), full),
               "contact_1": (_lib.RexContactSolveIn(tau.data_ptr(), 0.0, 1, 0.0, 1), full), "contact_60_forces": (_lib.RexContactSolveIn(tau.data_ptr(), 0.0, SWEEPS, 0.0, 1), forces)}
        cases = {name: (lambda i=i, o=o: _lib.check(L.rex_contact_solve(h, None, n, ctypes.byref(i), ctypes.byref(o.struct), sp), "rex_contact_solve"))
                 for name, (i, o) in ins.items()}
        cases["step"] = lambda: env.step(actions[0])
        cases["composed_60"] = lambda: composed(env, tau, dt, 0.5, SWEEPS)
        with env._on_stream():                                           # the composed route solves the same problem where no limit row is active
            undamped = env.contact_solve(tau=tau, fields=("v_next", "limit_torque"), iterations=SWEEPS, residual_threshold=0.0, damping=False)
            got = composed(env, tau, dt, 0.5, SWEEPS)
            torch.cuda.synchronize()
            plain = ~(undamped.limit_torque != 0).any(1)
            gap = float((got - undamped.v_next)[plain].abs().max())
            if not gap < 0.1:                                           # (float32 sweeps over clamping rows: a formulation error would be of order 1)
                raise SystemExit("the composed route differs from rex_contact_solve by %.3g in v_next" % gap)

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
                slow = name == "composed_60"
                run(fn, 1 if slow else 20)
                calls[name] = max(2 if slow else 100, int(args.window / run(fn, 2 if slow else 100)) + 1)
            times = {name: [] for name in cases}
            for _ in range(3):
                for name, fn in cases.items():
                    times[name].append(run(fn, calls[name]))
        for name in cases:
            t = sorted(times[name])
            out[name] = {"us_per_call": round(t[1] * 1e6, 2), "min_us": round(t[0] * 1e6, 2), "max_us": round(t[2] * 1e6, 2), "calls_per_run": calls[name],
                         "share_of_step": round(t[1] / sorted(times["step"])[1], 4)}
        out["composed_over_contact_60"] = round(out["composed_60"]["us_per_call"] / out["contact_60"]["us_per_call"], 1)
        out["composed_v_next_gap"] = gap
        out["sweeps_at_the_default_threshold"] = {"mean": round(float(sweeps.mean()), 2), "median": int(np.median(sweeps)), "max": int(sweeps.max()),
                                                  "share_one_sweep": round(float((sweeps == 1).mean()), 4), "share_all_%d" % SWEEPS: round(float((sweeps == SWEEPS).mean()), 4)}
        out["envs_with_a_loaded_foot"] = round(float(full.foot_contact.any(1).float().mean()), 4)
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
