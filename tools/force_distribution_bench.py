#!/usr/bin/env python3
"""Time force distribution (rex_force_distribution) beside the route a caller could write before it existed, in one process on one GPU:
walk-IK envs (auto-reset) after --steps random steps, 4 096 and 32 768 of them, on the plane and on the reference's random terrain, at
100, 300 and the default number of iterations.

Cases per (envs, ground, iterations):
  launch        rex_force_distribution through the C ABI into buffers allocated once, every output, vdot and a base wrench given, the
                stance set the points in reach (a timed call is one launch, nothing else)
  torch_route   env.kinematics (toe_pos, toe_normal, toe_in_reach, link_pos) + env.dynamics (toe_jacobian) + env.inverse_dynamics (the
                wanted base wrench and the joint rows) + the same iteration in batched torch ops on the env's stream + the outputs
and, per (envs, ground), step: rex_step of the same batch (env.step), for the per-iteration cost beside it.
The two routes' forces are compared before anything is timed (largest |difference| / (10 x the nominal mass), reported).

Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed
from a calibration run so that a run lasts about --window seconds (at least two calls), then three rounds over all cases in turn; the
median of a case's three runs is reported.  Prints one JSON line (and writes it to --out).

    python tools/force_distribution_bench.py [--envs 4096,32768] [--steps 300] [--window 0.3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_route(env, vdot, wrench, weights, eps, iterations):
    """the force distribution of rex_force_distribution (stance: the points in reach) from three readouts and batched torch ops"""
    import torch
    n = vdot.shape[0]
    kin = env.kinematics(fields=("link_pos", "toe_pos", "toe_normal", "toe_in_reach"))
    J = env.dynamics(fields=("toe_jacobian",)).toe_jacobian.view(n, 8, 3, 18)
    need = env.inverse_dynamics(vdot=vdot, base_wrench=wrench)
    r, joint = need[:, :6], need[:, 6:]
    d = kin.toe_pos.view(n, 8, 3) - kin.link_pos[:, 0:1]
    nrm = kin.toe_normal.view(n, 8, 3)
    inS = kin.toe_in_reach.view(n, 8, 1) != 0
    mu = env.body_params[2].view(n, 1) if getattr(env, "body_params", None) is not None else torch.full((n, 1), 0.5, device=env.device)
    W = torch.as_tensor(weights, dtype=torch.float32, device=env.device)
    d2 = d * d
    t = W[0] + W[1] + W[2] + W[3] * (d2[..., 1] + d2[..., 2]) + W[4] * (d2[..., 0] + d2[..., 2]) + W[5] * (d2[..., 0] + d2[..., 1])
    L = (eps + (t * inS[..., 0]).sum(-1)).view(n, 1, 1)
    sk = torch.sqrt(L / eps)
    beta = (sk - 1) / (sk + 1)
    inv = 1.0 / (1.0 + mu * mu)
    zero = torch.zeros((), device=env.device)

    def grad(x):
        A = torch.cat([x.sum(1), torch.cross(d, x, dim=-1).sum(1)], -1)
        u = W * (A - r)
        return u[:, None, 0:3] + torch.cross(u[:, None, 3:6].expand(n, 8, 3), d, dim=-1) + eps * x, A

    def project(x):
        s = (nrm * x).sum(-1)
        tv = x - s[..., None] * nrm
        tn = tv.norm(dim=-1)
        sp = (s + mu * tn) * inv
        k = torch.where(tn > 0, mu * sp / tn, zero)
        edge = sp[..., None] * nrm + k[..., None] * tv
        q = torch.where((tn <= mu * s)[..., None], x, torch.where((mu * tn <= -s)[..., None], zero, edge))
        return torch.where(inS, q, zero)

    f = torch.zeros((n, 8, 3), device=env.device)
    y = f
    for _ in range(iterations):
        fn = project(y - grad(y)[0] / L)
        y = fn + beta * (fn - f)
        f = fn
    g, A = grad(f)
    residual = L.view(n) * (project(f - g / L) - f).abs().amax((-1, -2))
    tau = joint - torch.einsum("kpcj,kpc->kj", J[..., 6:], f)
    return f.view(n, 4, 2, 3), tau, r - A, residual


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,32768")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rex_gym_amd import RexBatchEnv, _lib, build, force_distribution as fd
    if not torch.cuda.is_available():
        raise SystemExit("force_distribution_bench.py measures on the GPU: none found")
    counts = (100, 300, fd.ITERATIONS)
    res = {"what": "median of three alternating runs, microseconds per call, hipEvents around a run of back-to-back calls",
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(build.LIB_PATH), "steps_before": args.steps,
           "window_s": args.window, "default_iterations": fd.ITERATIONS, "runs": []}
    rng = np.random.RandomState(0)
    for n in [int(v) for v in args.envs.split(",")]:
        for ground, kw in (("plane", {}), ("random_terrain", dict(terrain_type="random", terrain_pool=8))):
            env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False, **kw)
            env.reset()
            actions = [torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device) for _ in range(16)]
            for k in range(args.steps):
                env.step(actions[k % 16])
            torch.cuda.synchronize()
            L, h, sp = env._L, env._h, env._stream_ptr()
            scale = np.array([1.0] * 3 + [2.0] * 3 + [10.0] * 12, np.float32)
            vdot = torch.as_tensor(rng.standard_normal((n, 18)).astype(np.float32) * scale, device=env.device)
            wrench = torch.as_tensor(rng.standard_normal((n, 6)).astype(np.float32), device=env.device)
            with env._on_stream():
                full = env.force_distribution(vdot=vdot, base_wrench=wrench, iterations=100)
            params = {c: fd.check_params(iterations=c) for c in counts}
            cases = {"step": lambda: env.step(actions[0])}
            for c in counts:
                cases["launch_%d" % c] = lambda c=c: _lib.check(L.rex_force_distribution(h, None, n, vdot.data_ptr(), wrench.data_ptr(), None, ctypes.byref(params[c]),
                                                                                         ctypes.byref(full.struct), sp), "rex_force_distribution")
                cases["torch_route_%d" % c] = lambda c=c: torch_route(env, vdot, wrench, fd.WEIGHTS, fd.EPS, c)
            with env._on_stream():
                cases["launch_300"]()
                theirs = cases["torch_route_300"]()
                torch.cuda.synchronize()
                gap = float((full.toe_force - theirs[0]).abs().max() / 50.0)
                if not gap < 1e-3:
                    raise SystemExit("rex_force_distribution's forces differ from the torch route by %.3g of the weight" % gap)

            def run(fn, calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(calls):
                    fn()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e-3 / calls

            out = {"envs": n, "ground": ground, "force_gap_to_torch_route": gap}
            with env._on_stream():
                calls = {}
                for name, fn in cases.items():       # warm-up and calibration
                    run(fn, 2)
                    calls[name] = max(2, int(args.window / run(fn, 2)) + 1)
                times = {name: [] for name in cases}
                for _ in range(3):
                    for name, fn in cases.items():
                        times[name].append(run(fn, calls[name]))
            for name in cases:
                t = sorted(times[name])
                out[name] = {"us_per_call": round(t[1] * 1e6, 2), "min_us": round(t[0] * 1e6, 2), "max_us": round(t[2] * 1e6, 2), "calls_per_run": calls[name]}
            for c in counts:
                out["torch_route_%d" % c]["over_launch"] = round(out["torch_route_%d" % c]["us_per_call"] / out["launch_%d" % c]["us_per_call"], 1)
            per_it = (out["launch_%d" % counts[2]]["us_per_call"] - out["launch_%d" % counts[0]]["us_per_call"]) / (counts[2] - counts[0])
            out["us_per_iteration"] = round(per_it, 4)
            out["iterations_per_step"] = round(out["step"]["us_per_call"] / per_it, 1)
            res["runs"].append(out)
            env.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
