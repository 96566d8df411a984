#!/usr/bin/env python3
"""Time candidate rollouts (rex_rollout) beside the route a caller could write before the call existed, in one process on one GPU: walk-IK
envs (auto-reset, the config's 5 substeps, 60 sweeps and residual threshold) after --steps random steps, on the plane and on the reference's
random terrain; K candidates of T = 5 control steps of repeat = 5 substeps, targets = the env's last motor command + uniform(-0.1, 0.1).

Cases per (ground, K):
  rollout        rex_rollout through the C ABI into buffers allocated once, `state` and `trajectory` asked for (a timed call is one launch)
  caller_route   what a caller can write without it: a scratch sim of N K envs holding K copies of every env's state (the episode word moved
                 so that each copy stands on its env's terrain field), and per substep rex_motor_torque on the scratch state's joint words (times the motor enable bits) +
                 rex_contact_solve (v_next alone) + the integrator in batched torch ops writing the scratch state; the copy of the state into
                 the scratch sim is part of a call
  contact_solve  one rex_contact_solve over N K rows: the per-substep yardstick (x T x repeat beside `rollout`)
Before anything is timed the two routes are compared after ONE substep (velocities relative to max(1, |v|), positions and joint angles
absolute; reported, and the tool stops if they disagree by more than 1e-3).

Drift, recorded and not judged: from the batch's state, --drift-steps env.step() calls with random actions record the step's own motor
commands and joint angles; the state is put back; ONE rollout (K = 1, repeat = 5) under those commands.  Median and 99th percentile of the
largest joint-angle difference per env, at the first and the last control step, over the envs that were not reset on the way: round-off
amplified through contact events (and the overheat counters the rollout does not advance).

Timing: hipEvents (torch.cuda.Event) on the env's stream around a run of back-to-back calls; a case is warmed up, its run length fixed from a
calibration run so that a run lasts about --window seconds (at least two calls), then three rounds over all cases in turn; the median of a
case's three runs is reported.  Prints one JSON line, writes it to --out and a markdown table of it to --md.

    python tools/rollout_bench.py [--envs 4096] [--candidates 1,8,32] [--steps 300] [--window 0.3] [--out profiles/rollout.json] [--md FILE]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, REPEAT, POOL = 5, 5, 8
VEL = list(range(7, 13)) + list(range(25, 37))


def integrate(state, v_next, dt):
    """the step's integrator on a [words, rows] state in batched torch ops: the new velocities, then pos += dt lin, q += dt qd, the
    quaternion turned by exp(dt w / 2) and normalised"""
    import torch
    state[VEL] = v_next.t()
    state[0:3] += dt * state[7:10]
    state[13:25] += dt * state[25:37]
    w = state[10:13]
    wn = w.norm(dim=0)
    half = 0.5 * dt * wn
    sc = torch.where(wn < 0.001, 0.5 * dt - dt * dt * dt * 0.020833333333 * wn * wn, torch.sin(half) / wn.clamp_min(1e-30))
    dx, dy, dz, dw = w[0] * sc, w[1] * sc, w[2] * sc, torch.cos(half)
    qx, qy, qz, qw = state[3].clone(), state[4].clone(), state[5].clone(), state[6].clone()
    q = torch.stack([dw * qx + dx * qw + dy * qz - dz * qy, dw * qy - dx * qz + dy * qw + dz * qx, dw * qz + dx * qy - dy * qx + dz * qw,
                     dw * qw - dx * qx - dy * qy - dz * qz])
    state[3:7] = q / q.norm(dim=0)


class CallerRoute:
    """the scratch sim of N K envs and the loop over the substeps"""

    def __init__(self, env, K, kw):
        import torch
        from rex_gym_amd import RexBatchEnv
        self.env, self.K, self.field = env, K, bool(kw)
        n = env.num_envs * K
        self.sim = sim = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False, **kw)
        sim.reset()
        self.src = torch.arange(n, device=env.device) // K
        # terrain_index = (global env index + 977 episode) mod POOL and 977 = 1 mod 8: the copy's episode word puts it on its env's field
        self.shift = ((self.src - torch.arange(n, device=env.device)) % POOL).to(torch.int32)
        self.tau, self.obs = torch.zeros((n, 12), device=env.device), torch.zeros((n, 12), device=env.device)
        self.con = None
        self.ew = 13 + 24 + 8

    def copy_state(self):
        import torch
        sim, env = self.sim, self.env
        sim.state.copy_(env.state[:, self.src])
        if self.field:
            ep = sim.state[self.ew].view(torch.int32)
            ep += self.shift
        # the motors the step has shut down (overheat protection) draw no torque: REX_S_MOTOR_EN, bit j
        self.enable = ((sim.state[self.ew + 1].view(torch.int32)[:, None] >> torch.arange(12, device=env.device, dtype=torch.int32)) & 1).to(torch.float32)

    def substep(self, cmd, dt):
        from rex_gym_amd import _lib
        sim = self.sim
        q, qd = sim.state[13:25].t().contiguous(), sim.state[25:37].t().contiguous()
        _lib.check(sim._L.rex_motor_torque(q.numel(), cmd.data_ptr(), q.data_ptr(), qd.data_ptr(), qd.data_ptr(), float(sim.config.motor_kp),
                                           float(sim.config.motor_kd), self.tau.data_ptr(), self.obs.data_ptr(), sim._stream_ptr()), "rex_motor_torque")
        self.tau *= self.enable
        self.con = sim.contact_solve(tau=self.tau, fields=("v_next",), out=self.con)
        integrate(sim.state, self.con.v_next, dt)

    def run(self, targets, steps=T, repeat=REPEAT):
        """targets [N, K, T, 12] -> the scratch state after steps x repeat substeps"""
        self.copy_state()
        dt = float(self.env.config.sim_time_step)
        flat = targets.reshape(-1, targets.shape[2], 12)
        for t in range(steps):
            cmd = flat[:, t].contiguous()
            for _ in range(repeat):
                self.substep(cmd, dt)
        return self.sim.state


def drift(env, rng, steps):
    """-> dict: joint-angle drift of one rollout under the step's own motor commands from the step's trajectory"""
    import numpy as np
    import torch
    n = env.num_envs
    S0 = env.state.clone()
    ring = getattr(env, "history", None)
    hist = None if ring is None else ring.clone()
    cmds, qs, alive = [], [], torch.ones(n, dtype=torch.bool, device=env.device)
    for _ in range(steps):
        _, _, done, info = env.step(torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device))
        alive &= ~done
        cmds.append(info["action"].clone())
        qs.append(env.state[13:25].t().clone())
    env.state.copy_(S0)
    if hist is not None:
        ring.copy_(hist)
    out = env.rollout(targets=torch.stack(cmds, 1).reshape(n, 1, steps, 12).contiguous(), repeat=int(env.config.action_repeat), fields=("trajectory",))
    torch.cuda.synchronize()
    gap = (out.trajectory[:, 0, :, 13:25] - torch.stack(qs, 1)).abs().amax(-1)[alive].cpu().numpy()          # [envs, steps]
    pct = lambda a: {"median_rad": float(np.median(a)), "p99_rad": float(np.percentile(a, 99)), "max_rad": float(a.max())}
    return {"control_steps": steps, "envs_not_reset": int(alive.sum()), "first_step": pct(gap[:, 0]), "last_step": pct(gap[:, -1])}


def markdown(res):
    lines = ["| ground | K | rows | `rollout` ms | caller's route ms | route / rollout | `contact_solve` us (N K rows) | x 25 ms | rollout / (25 contact solves) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in res["runs"]:
        lines.append("| %s | %d | %d | %.3f | %.3f | %.1f | %.1f | %.3f | %.2f |" % (
            r["ground"], r["K"], r["rows"], r["rollout"]["us_per_call"] * 1e-3, r["caller_route"]["us_per_call"] * 1e-3, r["caller_route"]["over_rollout"],
            r["contact_solve"]["us_per_call"], r["contact_solve"]["us_per_call"] * T * REPEAT * 1e-3, r["rollout"]["over_contact_solves"]))
    lines += ["", "| ground | envs not reset | first control step: median, p99, max (rad) | control step %d: median, p99, max (rad) |" % res["drift"][0]["control_steps"], "|---|---|---|---|"]
    for d in res["drift"]:
        f, l = d["first_step"], d["last_step"]
        lines.append("| %s | %d | %.2e, %.2e, %.2e | %.2e, %.2e, %.2e |" % (d["ground"], d["envs_not_reset"], f["median_rad"], f["p99_rad"], f["max_rad"],
                                                                            l["median_rad"], l["p99_rad"], l["max_rad"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--candidates", default="1,8,32")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--drift-steps", type=int, default=25)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rex_gym_amd import RexBatchEnv, _lib, build
    if not torch.cuda.is_available():
        raise SystemExit("rollout_bench.py measures on the GPU: none found")
    n = args.envs
    res = {"what": "median of three alternating runs, microseconds per call, hipEvents around a run of back-to-back calls",
           "device": torch.cuda.get_device_name(0), "library": os.path.basename(build.LIB_PATH), "envs": n, "steps_before": args.steps,
           "control_steps": T, "repeat": REPEAT, "window_s": args.window, "runs": [], "drift": []}
    rng = np.random.RandomState(0)
    for ground, kw in (("plane", {}), ("random_terrain", dict(terrain_type="random", terrain_pool=POOL))):
        env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False, **kw)
        env.reset()
        actions = [torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device) for _ in range(16)]
        for k in range(args.steps):
            _, _, _, info = env.step(actions[k % 16])
        last_cmd = info["action"].clone()
        torch.cuda.synchronize()
        res["drift"].append(dict(ground=ground, **drift(env, rng, args.drift_steps)))
        L, h, sp = env._L, env._h, env._stream_ptr()
        for K in [int(v) for v in args.candidates.split(",")]:
            targets = (last_cmd[:, None, None, :] + torch.as_tensor(rng.uniform(-0.1, 0.1, (n, K, T, 12)).astype(np.float32), device=env.device)).contiguous()
            route = CallerRoute(env, K, kw)
            with env._on_stream():
                full = env.rollout(targets=targets, repeat=REPEAT, fields=("state", "trajectory"))
                one = env.rollout(targets=targets[:, :, :1].contiguous(), repeat=1, fields=("state",)).state.reshape(n * K, 37)
                theirs = route.run(targets, 1, 1)[0:37].t()
                torch.cuda.synchronize()
                scale = one[:, VEL].abs().amax(-1).clamp_min(1.0)
                gap_v = float(((one[:, VEL] - theirs[:, VEL]).abs().amax(-1) / scale).max())
                gap_x = float((one[:, 0:7] - theirs[:, 0:7]).abs().max()), float((one[:, 13:25] - theirs[:, 13:25]).abs().max())
                if not max(gap_v, *gap_x) < 1e-3:
                    bad = ((one[:, VEL] - theirs[:, VEL]).abs().amax(-1) / scale) >= 1e-3
                    print("rows over 1e-3: %d of %d; of those with a motor shut down: %d" % (int(bad.sum()), bad.numel(), int((route.enable[bad].amin(-1) == 0).sum())))
                    raise SystemExit("rex_rollout and the caller's route differ after one substep: velocities %.3g, pose %.3g, joint angles %.3g" % (gap_v, *gap_x))
            inp = _lib.RexRolloutIn(targets.data_ptr(), None, K, T, REPEAT, 0.0, 0, -1.0)
            tau = route.tau
            cases = {"rollout": lambda: _lib.check(L.rex_rollout(h, None, n, ctypes.byref(inp), ctypes.byref(full.struct), sp), "rex_rollout"),
                     "caller_route": lambda: route.run(targets),
                     "contact_solve": lambda: route.sim.contact_solve(tau=tau, fields=("v_next",), out=route.con)}

            def run(fn, calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(calls):
                    fn()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e-3 / calls

            out = {"ground": ground, "K": K, "rows": n * K, "gap_after_one_substep": {"velocities": gap_v, "pose": gap_x[0], "joint_angles": gap_x[1]}}
            with env._on_stream():
                route.copy_state()
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
            out["caller_route"]["over_rollout"] = round(out["caller_route"]["us_per_call"] / out["rollout"]["us_per_call"], 2)
            out["rollout"]["over_contact_solves"] = round(out["rollout"]["us_per_call"] / (T * REPEAT * out["contact_solve"]["us_per_call"]), 3)
            out["rollout"]["us_per_row_substep"] = round(out["rollout"]["us_per_call"] / (n * K * T * REPEAT), 5)
            res["runs"].append(out)
            route.sim.close()
        env.close()
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line + "\n"), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
