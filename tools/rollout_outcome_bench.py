#!/usr/bin/env python3
"""Time action-space rollouts with and without the step's epilogue (rex_rollout_actions_outcome beside rex_rollout_actions), at the shapes of
tools/rollout_actions_bench.py: walk-IK envs (auto-reset, the config's 5 substeps, 60 sweeps and residual threshold) after --steps random
steps, on the plane and on the reference's random terrain; K candidates of T = 5 control steps of repeat = 5 substeps, actions uniform in
the Box.

Cases per (ground, K), one process, five alternating rounds (the yardstick and the call under test take turns inside every round), medians:
  plain    rex_rollout_actions, `state`, `trajectory`, `ctrl`, `targets` asked for: the yardstick
  outcome  rex_rollout_actions_outcome with the same four and reward, done, obs, motor_torque
  return   the same with reward and done alone (what scoring by return reads): no torque store, no observation store
Their seven shared fields are compared bit for bit before anything is timed.  Once, at --envs x the largest K rows: env.outcome alone
(rex_outcome on a trajectory slice, its controller words and torques).

Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed from
a calibration run so that a run lasts about --window seconds (at least two calls).  Prints one JSON line, writes it to --out and a markdown
table of it to --md.

    python tools/rollout_outcome_bench.py [--envs 4096] [--candidates 1,8,32] [--steps 300] [--window 0.3] [--out FILE] [--md FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, REPEAT, POOL, ROUNDS = 5, 5, 8, 5
GROUNDS = (("plane", {}), ("random_terrain", dict(terrain_type="random", terrain_pool=POOL)))
SHARED = ("state", "trajectory", "ctrl", "targets")


def timed(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def measure(args):
    import numpy as np
    import torch
    from rex_gym_amd import RexBatchEnv, _lib, build
    n = args.envs
    res = {"what": "median of %d alternating runs, microseconds per call, hipEvents around a run of back-to-back calls" % ROUNDS, "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(build.LIB_PATH), "envs": n, "steps_before": args.steps, "control_steps": T, "repeat": REPEAT, "window_s": args.window, "runs": []}
    rng = np.random.RandomState(0)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    Ks = [int(v) for v in args.candidates.split(",")]
    for ground, kw in GROUNDS:
        env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False, **kw)
        env.reset()
        warm = [torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device) for _ in range(16)]
        for k in range(args.steps):
            env.step(warm[k % 16])
        torch.cuda.synchronize()
        L, h, sp = env._L, env._h, env._stream_ptr()
        for K in Ks:
            actions = torch.as_tensor(rng.uniform(-0.4, 0.4, (T, n, K, 2)).astype(np.float32), device=env.device)
            with env._on_stream():
                plain = env.rollout_actions(actions, repeat=REPEAT, fields=SHARED)
                full = env.rollout_actions(actions, repeat=REPEAT, fields=SHARED + ("reward", "done", "obs", "motor_torque"))
                ret = env.rollout_actions(actions, repeat=REPEAT, fields=SHARED + ("reward", "done"))
                torch.cuda.synchronize()
                for f in SHARED:
                    if not (torch.equal(bits(getattr(plain, f)), bits(getattr(full, f))) and torch.equal(bits(getattr(plain, f)), bits(getattr(ret, f)))):
                        raise SystemExit("rollout_actions with and without the outcome fields differ in " + f)
                if not (torch.equal(bits(ret.reward), bits(full.reward)) and torch.equal(ret.done, full.done)):
                    raise SystemExit("reward and done alone differ from the full call's")
                ws = env._rollout_actions_ws[1]
            inp = _lib.RexRolloutActionsIn(actions.data_ptr(), None, K, T, REPEAT, 0.0, 0, -1.0)
            none = _lib.RexRolloutFrom()
            with_outcome = lambda ro: (lambda: _lib.check(L.rex_rollout_actions_outcome(h, None, n, ctypes.byref(inp), ctypes.byref(none), ctypes.byref(ro.struct),
                                                                                        ctypes.byref(ro.outcome_struct), ws.data_ptr(), ws.numel() * 4, sp), "rex_rollout_actions_outcome"))
            cases = {"plain": lambda: _lib.check(L.rex_rollout_actions(h, None, n, ctypes.byref(inp), ctypes.byref(none), ctypes.byref(plain.struct), ws.data_ptr(),
                                                                       ws.numel() * 4, sp), "rex_rollout_actions"),
                     "outcome": with_outcome(full), "return": with_outcome(ret)}
            out = {"ground": ground, "K": K, "rows": n * K, "done_share_last_step": float(full.done[T - 1].float().mean())}
            with env._on_stream():
                calls = {}
                for name, fn in cases.items():       # warm-up and calibration
                    timed(torch, fn, 2)
                    calls[name] = max(2, int(args.window / timed(torch, fn, 2)) + 1)
                times = {name: [] for name in cases}
                for _ in range(ROUNDS):
                    for name, fn in cases.items():
                        times[name].append(timed(torch, fn, calls[name]))
            for name in cases:
                t = sorted(times[name])
                out[name] = {"us_per_call": round(t[ROUNDS // 2] * 1e6, 2), "min_us": round(t[0] * 1e6, 2), "max_us": round(t[-1] * 1e6, 2), "calls_per_run": calls[name]}
            for name in ("outcome", "return"):
                out[name]["over_plain"] = round(out[name]["us_per_call"] / out["plain"]["us_per_call"], 4)
                out[name]["slowest_over_fastest_plain"] = round(out[name]["max_us"] / out["plain"]["min_us"], 4)
            out["plain"]["spread"] = round(out["plain"]["max_us"] / out["plain"]["min_us"], 4)
            if K == max(Ks):                          # env.outcome alone, on the last slice the full call emitted
                oc = env.outcome(full.trajectory[T - 1], full.ctrl, full.motor_torque[T - 1])
                alone = lambda: env.outcome(full.trajectory[T - 1], full.ctrl, full.motor_torque[T - 1], out=oc)
                with env._on_stream():
                    alone()
                    torch.cuda.synchronize()
                    if not torch.equal(bits(oc.reward), bits(full.reward[T - 1])):
                        raise SystemExit("env.outcome on the last slice and the rollout's reward differ")
                    timed(torch, alone, 2)
                    m = max(2, int(args.window / timed(torch, alone, 2)) + 1)
                    t = sorted(timed(torch, alone, m) for _ in range(ROUNDS))
                out["outcome_alone"] = {"us_per_call": round(t[ROUNDS // 2] * 1e6, 2), "min_us": round(t[0] * 1e6, 2), "max_us": round(t[-1] * 1e6, 2), "calls_per_run": m}
            res["runs"].append(out)
        env.close()
    return res


def markdown(res):
    lines = ["| ground | K | rows | plain ms | spread of plain (max / min) | outcome ms | outcome / plain | reward + done ms | that / plain | `env.outcome` alone us |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        a = r.get("outcome_alone")
        lines.append("| %s | %d | %d | %.3f | %.4f | %.3f | %.4f | %.3f | %.4f | %s |" % (
            r["ground"], r["K"], r["rows"], r["plain"]["us_per_call"] * 1e-3, r["plain"]["spread"], r["outcome"]["us_per_call"] * 1e-3, r["outcome"]["over_plain"],
            r["return"]["us_per_call"] * 1e-3, r["return"]["over_plain"], "%.1f" % a["us_per_call"] if a else "-"))
    lines += ["", "Run to run, (min .. max of the %d rounds) / median: " % ROUNDS + ", ".join(
        "%s K%d %s" % (r["ground"], r["K"], " ".join("(%s) %.3f..%.3f" % (c, r[c]["min_us"] / r[c]["us_per_call"], r[c]["max_us"] / r[c]["us_per_call"])
                                                   for c in ("plain", "outcome", "return"))) for r in res["runs"])]
    lines += ["", "Rows done at the last step (they run on; the caller masks): " + ", ".join("%s K%d %.3f" % (r["ground"], r["K"], r["done_share_last_step"]) for r in res["runs"])]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--candidates", default="1,8,32")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rollout_outcome_bench.py measures on the GPU: none found")
    res = measure(args)
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line + "\n"), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
