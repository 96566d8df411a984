#!/usr/bin/env python3
"""Time action-space rollouts (rex_rollout_actions) at the shapes of tools/rollout_bench.py -- walk-IK envs (auto-reset, the config's 5
substeps, 60 sweeps and residual threshold) after --steps random steps, on the plane and on the reference's random terrain; K candidates
of T = 5 control steps of repeat = 5 substeps, actions uniform in the Box -- beside its floor and beside the routes a caller has without it.

Cases per (ground, K), one process, three alternating rounds, medians:
  rollout_actions  (a) the call: 2 T launches enqueued by one C call (`state`, `trajectory`, `ctrl`, `targets` asked for)
  floor            (b) ONE rex_rollout_from launch fed the targets (a) emitted (`state`, `trajectory`): the physics alone.  (a) - (b) is the
                   T command kernels plus 2 T - 1 launch gaps.  Its `state` is (a)'s bit for bit (asserted here)
  caller_route     (c) per control step one env.command and one env.rollout(T = 1) from Python, chained through state and ctrl: the same
                   kernels and bits (asserted here), the Python calls in between
  scratch_sim      (d) plane only: a scratch RexBatchEnv(N K) loaded with the env's state words repeated K times, stepped by ONE
                   step_segment launch of T steps.  The step kernels pick the terrain by global env index and episode (so on a pool
                   the scratch sim stands on other ground: not run there), write state, and take no per-row wrench or body; they also
                   compute reward, observation and termination.  Its motor commands are compared with (a)'s targets at the first
                   step (the same controller on the same words: the gap is recorded)

Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed from a
calibration run so that a run lasts about --window seconds (at least two calls).  Prints one JSON line, writes it to --out and a markdown
table of it to --md.

    python tools/rollout_actions_bench.py [--envs 4096] [--candidates 1,8,32] [--steps 300] [--window 0.3] [--out FILE] [--md FILE]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, REPEAT, POOL = 5, 5, 8
GROUNDS = (("plane", {}), ("random_terrain", dict(terrain_type="random", terrain_pool=POOL)))


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
    res = {"what": "median of three alternating runs, microseconds per call, hipEvents around a run of back-to-back calls", "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(build.LIB_PATH), "envs": n, "steps_before": args.steps, "control_steps": T, "repeat": REPEAT, "window_s": args.window, "runs": []}
    rng = np.random.RandomState(0)
    bits = lambda t: t.view(torch.int32)
    for ground, kw in GROUNDS:
        env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False, **kw)
        env.reset()
        warm = [torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device) for _ in range(16)]
        for k in range(args.steps):
            env.step(warm[k % 16])
        torch.cuda.synchronize()
        L, h, sp = env._L, env._h, env._stream_ptr()
        for K in [int(v) for v in args.candidates.split(",")]:
            actions = torch.as_tensor(rng.uniform(-0.4, 0.4, (T, n, K, 2)).astype(np.float32), device=env.device)
            with env._on_stream():
                ro = env.rollout_actions(actions, repeat=REPEAT, fields=("state", "trajectory", "ctrl", "targets"))
                targets = ro.targets.permute(1, 2, 0, 3).contiguous()
                floor = env.rollout(targets=targets, repeat=REPEAT, fields=("state", "trajectory"))
                torch.cuda.synchronize()
                if not torch.equal(bits(floor.state), bits(ro.state)):
                    raise SystemExit("one rollout launch fed the emitted targets and rollout_actions differ")
                ws = env._rollout_actions_ws[1]
            inp = _lib.RexRolloutActionsIn(actions.data_ptr(), None, K, T, REPEAT, 0.0, 0, -1.0)
            none = _lib.RexRolloutFrom()
            fin = _lib.RexRolloutIn(targets.data_ptr(), None, K, T, REPEAT, 0.0, 0, -1.0)
            steps = [(torch.empty((n, K, 12), device=env.device), torch.empty((n, K, 8), device=env.device)) for _ in range(T)]
            slices = [None] * T

            def caller_route():
                state = ctrl = None
                for t in range(T):
                    tg, ctrl = env.command(actions[t], state=state, ctrl=ctrl, out=steps[t])
                    slices[t] = env.rollout(targets=tg[:, :, None, :], repeat=REPEAT, init_state=state, fields=("state",), out=slices[t])
                    state = slices[t].state
                return state

            with env._on_stream():
                if not torch.equal(bits(caller_route()), bits(ro.state)):
                    raise SystemExit("the caller's route and rollout_actions differ")
            cases = {"rollout_actions": lambda: _lib.check(L.rex_rollout_actions(h, None, n, ctypes.byref(inp), ctypes.byref(none), ctypes.byref(ro.struct), ws.data_ptr(),
                                                                                 ws.numel() * 4, sp), "rex_rollout_actions"),
                     "floor": lambda: _lib.check(L.rex_rollout_from(h, None, n, ctypes.byref(fin), ctypes.byref(none), ctypes.byref(floor.struct), sp), "rex_rollout_from"),
                     "caller_route": caller_route}
            out = {"ground": ground, "K": K, "rows": n * K}
            sim = None
            if ground == "plane":
                sim = RexBatchEnv(n * K, task="walk", signal_type="ik", seed=0, auto_reset=False, check_actions=False)
                sim.reset()
                flat = actions.reshape(T, n * K, 2)
                seg = (torch.empty((T, n * K, sim.obs_dim), device=env.device), torch.empty((T, n * K), device=env.device),
                       torch.empty((T, n * K), dtype=torch.uint8, device=env.device))
                cmd = torch.empty((T, n * K, 12), device=env.device)

                def scratch_sim():
                    sim.state.copy_(env.state.repeat_interleave(K, dim=1))
                    return sim.step_segment(flat, out=seg, motor_cmd=cmd)

                with env._on_stream():
                    scratch_sim()
                    torch.cuda.synchronize()
                    out["scratch_first_command_gap_rad"] = float((cmd[0].reshape(n, K, 12) - ro.targets[0]).abs().max())
                cases["scratch_sim"] = scratch_sim
            with env._on_stream():
                calls = {}
                for name, fn in cases.items():       # warm-up and calibration
                    timed(torch, fn, 2)
                    calls[name] = max(2, int(args.window / timed(torch, fn, 2)) + 1)
                times = {name: [] for name in cases}
                for _ in range(3):
                    for name, fn in cases.items():
                        times[name].append(timed(torch, fn, calls[name]))
            for name in cases:
                t = sorted(times[name])
                out[name] = {"us_per_call": round(t[1] * 1e6, 2), "min_us": round(t[0] * 1e6, 2), "max_us": round(t[2] * 1e6, 2), "calls_per_run": calls[name]}
            a = out["rollout_actions"]["us_per_call"]
            out["rollout_actions"]["over_floor"] = round(a / out["floor"]["us_per_call"], 4)
            out["rollout_actions"]["minus_floor_us"] = round(a - out["floor"]["us_per_call"], 2)
            out["caller_route"]["over_rollout_actions"] = round(out["caller_route"]["us_per_call"] / a, 4)
            if sim is not None:
                out["scratch_sim"]["over_rollout_actions"] = round(out["scratch_sim"]["us_per_call"] / a, 4)
                sim.close()
            res["runs"].append(out)
        env.close()
    return res


def markdown(res):
    lines = ["| ground | K | rows | (a) `rollout_actions` ms | (b) floor ms | a / b | a - b us | (c) caller's route ms | c / a | (d) scratch sim ms | d / a |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        d = r.get("scratch_sim")
        lines.append("| %s | %d | %d | %.3f | %.3f | %.3f | %.1f | %.3f | %.3f | %s | %s |" % (
            r["ground"], r["K"], r["rows"], r["rollout_actions"]["us_per_call"] * 1e-3, r["floor"]["us_per_call"] * 1e-3, r["rollout_actions"]["over_floor"],
            r["rollout_actions"]["minus_floor_us"], r["caller_route"]["us_per_call"] * 1e-3, r["caller_route"]["over_rollout_actions"],
            "%.3f" % (d["us_per_call"] * 1e-3) if d else "-", "%.3f" % d["over_rollout_actions"] if d else "-"))
    lines += ["", "Run to run, (min .. max of the three rounds) / median: " + ", ".join(
        "%s K%d %s" % (r["ground"], r["K"], " ".join("(%s) %.3f..%.3f" % (tag, r[c]["min_us"] / r[c]["us_per_call"], r[c]["max_us"] / r[c]["us_per_call"])
                                                   for tag, c in zip("abcd", ("rollout_actions", "floor", "caller_route", "scratch_sim")) if c in r)) for r in res["runs"])]
    gaps = [(r["K"], r["scratch_first_command_gap_rad"]) for r in res["runs"] if "scratch_first_command_gap_rad" in r]
    if gaps:
        lines += ["", "Scratch sim against `rollout_actions`, motor commands of the first step, largest difference: " + ", ".join("K%d %.1e rad" % g for g in gaps)]
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
        raise SystemExit("rollout_actions_bench.py measures on the GPU: none found")
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
