#!/usr/bin/env python3
"""Time rollouts from given states, under base pushes and per-candidate bodies (rex_rollout_from) at the shapes of tools/rollout_bench.py --
walk-IK envs (auto-reset, the config's 5 substeps, 60 sweeps and residual threshold) after --steps random steps, on the plane and on the
reference's random terrain; K candidates of T = 5 control steps of repeat = 5 substeps, targets = the env's last motor command +
uniform(-0.1, 0.1) -- beside rex_rollout and beside the route a caller could write without the call.

Inputs of the new call, per row: init_state = the env's own words 0..36 with the joint angles moved by uniform(-0.01, 0.01) rad (perturbed
states, the finite-difference use); base_wrench = force uniform within +-22.6 N per axis, moment within +-2.26 N m, per control step; body =
mass scales 0.8 .. 1.2, toe friction 0.3 .. 1.0.

Cases per (ground, K), one process, three alternating rounds, medians:
  rollout        rex_rollout, as tools/rollout_bench.py times it (`state` and `trajectory` asked for)
  rollout_from   rex_rollout_from with all three inputs, the same outputs
  from_own       rex_rollout_from handed the env's own state and body parameters and a wrench of zeros: rex_rollout's arithmetic bit for
                 bit (asserted here), so its time beside `rollout` is the price of the extra reads alone; `rollout_from` beside it also
                 pays for other physics (with the config's residual threshold the sweep counts follow the states, bodies and pushes:
                 the mean sweeps per row are recorded)
  caller_route   rollout_bench.CallerRoute extended to the same question: per call the scratch sim of N K envs is loaded with the given
                 states (the other words are the env's) and the rows' body parameters (set_body_params); per substep rex_motor_torque on
                 the scratch state, then the wrench as an impulse dt w through push() (rex_apply_impulse), then rex_contact_solve and
                 the integrator in torch
Before anything is timed, rollout_from (T = 1, repeat = 1) and the route are compared after ONE substep and the gap is recorded (largest,
median, rows over 1e-3).  States and bodies alone agree to the bit.  The wrench does not: the route's impulse moves v before the bias and
the damping are evaluated, the call's wrench enters beside them -- a difference of the order dt x the velocity change.  (A route that
pushes BEFORE it draws the motor torque is another model: the motor's stiff damping term sees the pushed joint rates in the same substep,
and the joint rates differ from the call's by the order of the push's own effect.)

--against DIR: a second, built checkout of the project (the parent commit).  rex_rollout is then timed in fresh processes, this tree and
that one in turn, three rounds: the same kernel must sit within the run-to-run spread.  (One process per build: a process loads the library
once.  The driver itself never opens the GPU.)

Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed from a
calibration run so that a run lasts about --window seconds (at least two calls).  Prints one JSON line, writes it to --out and a markdown
table of it to --md.

    python tools/rollout_from_bench.py [--envs 4096] [--candidates 1,8,32] [--steps 300] [--window 0.3] [--against DIR] [--out FILE] [--md FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, REPEAT, POOL = 5, 5, 8
GROUNDS = (("plane", {}), ("random_terrain", dict(terrain_type="random", terrain_pool=POOL)))
FORCE, MOMENT = 22.6, 2.26


def timed(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def batch(args, rng, ground_kw):
    """the batch after --steps random steps and its last motor command"""
    import numpy as np
    import torch
    from rex_gym_amd import RexBatchEnv
    n = args.envs
    env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False, **ground_kw)
    env.reset()
    actions = [torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device) for _ in range(16)]
    for k in range(args.steps):
        _, _, _, info = env.step(actions[k % 16])
    last = info["action"].clone()
    torch.cuda.synchronize()
    return env, last


def commands(env, last, rng, K):
    import numpy as np
    import torch
    return (last[:, None, None, :] + torch.as_tensor(rng.uniform(-0.1, 0.1, (env.num_envs, K, T, 12)).astype(np.float32), device=env.device)).contiguous()


def child_ab(args):
    """one run of rex_rollout per (ground, K) with the library of the tree this process imports"""
    import numpy as np
    import torch
    from rex_gym_amd import _lib
    rng = np.random.RandomState(0)
    runs = []
    for ground, kw in GROUNDS:
        env, last = batch(args, rng, kw)
        for K in [int(v) for v in args.candidates.split(",")]:
            targets = commands(env, last, rng, K)
            with env._on_stream():
                full = env.rollout(targets=targets, repeat=REPEAT, fields=("state", "trajectory"))
                inp = _lib.RexRolloutIn(targets.data_ptr(), None, K, T, REPEAT, 0.0, 0, -1.0)
                fn = lambda: _lib.check(env._L.rex_rollout(env._h, None, env.num_envs, ctypes.byref(inp), ctypes.byref(full.struct), env._stream_ptr()), "rex_rollout")
                timed(torch, fn, 2)
                calls = max(2, int(args.window / timed(torch, fn, 2)) + 1)
                runs.append({"ground": ground, "K": K, "us_per_call": round(timed(torch, fn, calls) * 1e6, 2), "calls": calls})
        env.close()
    print("RESULT " + json.dumps(runs))


def child_from(args):
    import numpy as np
    import torch
    from rex_gym_amd import _lib, build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import rollout_bench as rb

    class FromRoute(rb.CallerRoute):
        """the scratch sim loaded with the given states and bodies; the wrench as an impulse per substep"""

        def load(self, init, body, wrench):
            rows = init.shape[0] * init.shape[1]
            self.init, self.body = init.reshape(rows, 37).t().contiguous(), body.reshape(rows, 3).t().contiguous()
            self.impulse = (float(self.env.config.sim_time_step) * wrench.reshape(rows, -1, 6)).transpose(0, 1).contiguous()      # [T, rows, 6]
            self.dv = None

        def copy_state(self):
            super().copy_state()
            self.sim.state[0:37] = self.init
            self.sim.set_body_params(self.body[0], self.body[1], self.body[2])

        def substep(self, cmd, dt, impulse):
            sim = self.sim
            q, qd = sim.state[13:25].t().contiguous(), sim.state[25:37].t().contiguous()
            _lib.check(sim._L.rex_motor_torque(q.numel(), cmd.data_ptr(), q.data_ptr(), qd.data_ptr(), qd.data_ptr(), float(sim.config.motor_kp),
                                               float(sim.config.motor_kd), self.tau.data_ptr(), self.obs.data_ptr(), sim._stream_ptr()), "rex_motor_torque")
            self.tau *= self.enable
            self.dv = sim.push(base_impulse=impulse, out=self.dv)
            self.con = sim.contact_solve(tau=self.tau, fields=("v_next",), out=self.con)
            rb.integrate(sim.state, self.con.v_next, dt)

        def run(self, targets, steps=T, repeat=REPEAT):
            self.copy_state()
            dt = float(self.env.config.sim_time_step)
            flat = targets.reshape(-1, targets.shape[2], 12)
            for t in range(steps):
                cmd = flat[:, t].contiguous()
                for _ in range(repeat):
                    self.substep(cmd, dt, self.impulse[t])
            return self.sim.state

    n = args.envs
    res = {"what": "median of three alternating runs, microseconds per call, hipEvents around a run of back-to-back calls", "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(build.LIB_PATH), "envs": n, "steps_before": args.steps, "control_steps": T, "repeat": REPEAT, "window_s": args.window, "runs": []}
    rng = np.random.RandomState(0)
    for ground, kw in GROUNDS:
        env, last = batch(args, rng, kw)
        L, h, sp = env._L, env._h, env._stream_ptr()
        for K in [int(v) for v in args.candidates.split(",")]:
            targets = commands(env, last, rng, K)
            dev = lambda a: torch.as_tensor(a.astype(np.float32), device=env.device)
            init = env.state[0:37].t()[:, None, :].repeat(1, K, 1).contiguous()
            init[:, :, 13:25] += dev(rng.uniform(-0.01, 0.01, (n, K, 12)))
            wrench = dev(rng.uniform(-1.0, 1.0, (n, K, T, 6)) * np.array([FORCE] * 3 + [MOMENT] * 3))
            body = dev(np.stack([rng.uniform(0.8, 1.2, (n, K)), rng.uniform(0.8, 1.2, (n, K)), rng.uniform(0.3, 1.0, (n, K))], -1))
            route = FromRoute(env, K, kw)
            route.load(init, body, wrench)
            with env._on_stream():
                full = env.rollout(targets=targets, repeat=REPEAT, fields=("state", "trajectory"))
                full_from = env.rollout(targets=targets, repeat=REPEAT, fields=("state", "trajectory"), init_state=init, base_wrench=wrench, body=body)
                own = (env.state[0:37].t()[:, None, :].repeat(1, K, 1).contiguous(), torch.zeros_like(wrench),
                       (env.body_params.t()[:, None, :].repeat(1, K, 1) if getattr(env, "body_params", None) is not None
                        else torch.tensor([1.0, 1.0, 0.5], device=env.device).repeat(n, K, 1)).contiguous())
                full_own = env.rollout(targets=targets, repeat=REPEAT, fields=("state", "trajectory"), init_state=own[0], base_wrench=own[1], body=own[2])
                if not (torch.equal(full_own.state.view(torch.int32), full.state.view(torch.int32)) and
                        torch.equal(full_own.trajectory.view(torch.int32), full.trajectory.view(torch.int32))):
                    raise SystemExit("rex_rollout_from with the env's own inputs and rex_rollout differ")
                sweeps = [float(env.rollout(targets=targets, repeat=REPEAT, fields=("sweeps",), **kw2).sweeps.float().mean()) / (T * REPEAT)
                          for kw2 in ({}, dict(init_state=init, base_wrench=wrench, body=body))]
                one = env.rollout(targets=targets[:, :, :1].contiguous(), repeat=1, fields=("state",), init_state=init, base_wrench=wrench[:, :, :1].contiguous(),
                                  body=body).state.reshape(n * K, 37)
                theirs = route.run(targets, 1, 1)[0:37].t()
                torch.cuda.synchronize()
                scale = one[:, rb.VEL].abs().amax(-1).clamp_min(1.0)
                gap = (one[:, rb.VEL] - theirs[:, rb.VEL]).abs().amax(-1) / scale
                gap_v, gap_med, gap_rows = float(gap.max()), float(gap.median()), int((gap > 1e-3).sum())
                gap_x = float((one[:, 0:7] - theirs[:, 0:7]).abs().max()), float((one[:, 13:25] - theirs[:, 13:25]).abs().max())
            inp = _lib.RexRolloutIn(targets.data_ptr(), None, K, T, REPEAT, 0.0, 0, -1.0)
            src = _lib.RexRolloutFrom(init.data_ptr(), wrench.data_ptr(), body.data_ptr())
            src_own = _lib.RexRolloutFrom(*(t.data_ptr() for t in own))
            cases = {"rollout": lambda: _lib.check(L.rex_rollout(h, None, n, ctypes.byref(inp), ctypes.byref(full.struct), sp), "rex_rollout"),
                     "rollout_from": lambda: _lib.check(L.rex_rollout_from(h, None, n, ctypes.byref(inp), ctypes.byref(src), ctypes.byref(full_from.struct), sp), "rex_rollout_from"),
                     "from_own": lambda: _lib.check(L.rex_rollout_from(h, None, n, ctypes.byref(inp), ctypes.byref(src_own), ctypes.byref(full_own.struct), sp), "rex_rollout_from"),
                     "caller_route": lambda: route.run(targets)}
            out = {"ground": ground, "K": K, "rows": n * K, "mean_sweeps_per_substep": {"rollout": round(sweeps[0], 2), "rollout_from": round(sweeps[1], 2)},
                   "gap_after_one_substep": {"velocities": gap_v, "velocities_median": gap_med, "rows_over_1e-3": gap_rows, "pose": gap_x[0], "joint_angles": gap_x[1]}}
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
            out["rollout_from"]["over_rollout"] = round(out["rollout_from"]["us_per_call"] / out["rollout"]["us_per_call"], 4)
            out["from_own"]["over_rollout"] = round(out["from_own"]["us_per_call"] / out["rollout"]["us_per_call"], 4)
            out["caller_route"]["over_rollout_from"] = round(out["caller_route"]["us_per_call"] / out["rollout_from"]["us_per_call"], 2)
            res["runs"].append(out)
            route.sim.close()
        env.close()
    print("RESULT " + json.dumps(res))


def spawn(tree, mode, args):
    """a fresh process that imports the package of `tree` -> the JSON behind its RESULT line"""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, "--envs", str(args.envs), "--candidates", args.candidates,
           "--steps", str(args.steps), "--window", str(args.window)]
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout
    return json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])


def markdown(res):
    lines = ["| ground | K | rows | `rollout` ms | `from_own` ms | own / rollout | `rollout_from` ms | from / rollout | mean sweeps a substep: rollout, from | caller's route ms | route / from |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        lines.append("| %s | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f, %.2f | %.3f | %.1f |" % (
            r["ground"], r["K"], r["rows"], r["rollout"]["us_per_call"] * 1e-3, r["from_own"]["us_per_call"] * 1e-3, r["from_own"]["over_rollout"],
            r["rollout_from"]["us_per_call"] * 1e-3, r["rollout_from"]["over_rollout"], r["mean_sweeps_per_substep"]["rollout"],
            r["mean_sweeps_per_substep"]["rollout_from"], r["caller_route"]["us_per_call"] * 1e-3, r["caller_route"]["over_rollout_from"]))
    lines += ["", "| ground | K | route against `rollout_from` after one substep, velocities: largest, median, rows over 1e-3 |", "|---|---|---|"]
    for r in res["runs"]:
        g = r["gap_after_one_substep"]
        lines.append("| %s | %d | %.1e, %.1e, %d of %d |" % (r["ground"], r["K"], g["velocities"], g["velocities_median"], g["rows_over_1e-3"], r["rows"]))
    if res.get("against"):
        lines += ["", "| ground | K | this tree ms: three rounds | the other tree ms: three rounds | medians: this / other |", "|---|---|---|---|---|"]
        for r in res["against"]["runs"]:
            lines.append("| %s | %d | %s | %s | %.4f |" % (r["ground"], r["K"], ", ".join("%.3f" % (v * 1e-3) for v in r["this_us"]),
                                                          ", ".join("%.3f" % (v * 1e-3) for v in r["other_us"]), r["this_over_other"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--candidates", default="1,8,32")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--against", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--child", default=None, choices=("ab", "from"))
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.child:
        sys.path.insert(0, os.path.abspath(args.tree))
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("rollout_from_bench.py measures on the GPU: none found")
        return child_ab(args) if args.child == "ab" else child_from(args)
    res = spawn(ROOT, "from", args)
    if args.against:
        rounds = [(spawn(ROOT, "ab", args), spawn(args.against, "ab", args)) for _ in range(3)]
        runs = []
        for i, first in enumerate(rounds[0][0]):
            this, other = [r[0][i]["us_per_call"] for r in rounds], [r[1][i]["us_per_call"] for r in rounds]
            runs.append({"ground": first["ground"], "K": first["K"], "this_us": this, "other_us": other,
                         "this_over_other": round(sorted(this)[1] / sorted(other)[1], 4)})
        res["against"] = {"what": "rex_rollout, one fresh process per tree and round, this tree and the other in turn; microseconds per call", "runs": runs}
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line + "\n"), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
