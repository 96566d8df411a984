#!/usr/bin/env python3
"""Time the onboard sensors (rex_sense_depth, rex_height_scan) beside the renderer's kernel and a control step, in one process
on one GPU: 4 096 walk-IK envs (auto-reset) after --steps random steps, so that the batch holds the stationary mix of episode ages.

Cases, all through the C ABI into buffers allocated once (a timed call is one launch, nothing else):
  sense_WxH    rex_sense_depth, the default mount, at 16 x 12, 32 x 24 and 64 x 48
  render_WxH   rex_render with depth on at the same n, W and H: the renderer's launch shape on the sensor's workload
  scan_K       rex_height_scan at K = 25 and K = 187
  step         one env.step of the same batch (rex_step)

Each case is warmed up, then timed in windows of at least --window seconds that end in a device synchronise (the call count of a
window is fixed from a calibration window); three rounds over all cases in turn, the median of a case's three windows is
reported.  Prints one JSON line (and writes it to --out).

    python tools/sense_bench.py [--envs 4096] [--steps 300] [--window 0.5] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(16, 12), (32, 24), (64, 48)]
SCANS = [(5, 5), (17, 11)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from rex_gym_amd import RexBatchEnv, _lib
    if not torch.cuda.is_available():
        raise SystemExit("sense_bench.py measures on the GPU: none found")
    n = args.envs
    env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, auto_reset=True, check_actions=False)
    env.reset()
    rng = np.random.RandomState(0)
    actions = [torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device) for _ in range(16)]
    for k in range(args.steps):
        env.step(actions[k % 16])
    torch.cuda.synchronize()
    L, h, dev = env._L, env._h, env.device
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    cam = env._camera(None)
    sp = env._stream_ptr()
    cases = {}
    keep = []          # the buffers of every case stay alive

    def add(name, fn, work=None):
        cases[name] = (fn, work)

    for W, H in SIZES:
        sensor = env.depth_sensor(width=W, height=H)
        out = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        dep = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        keep += [sensor, out, rgb, dep]
        add(f"sense_{W}x{H}", lambda s=sensor, o=out: _lib.check(
            L.rex_sense_depth(h, ctypes.byref(s.struct), None, n, o.data_ptr(), sp), "rex_sense_depth"), n * W * H)
        add(f"render_{W}x{H}", lambda r=rgb, d=dep, W=W, H=H: _lib.check(
            L.rex_render(h, ctypes.byref(cam), ids.data_ptr(), n, W, H, r.data_ptr(), d.data_ptr(), None, sp), "rex_render"), n * W * H)
    for nx, ny in SCANS:
        grid = np.stack(np.meshgrid(np.linspace(-0.8, 0.8, nx), np.linspace(-0.5, 0.5, ny), indexing="ij"), -1).reshape(-1, 2)
        pts = torch.as_tensor(grid.astype(np.float32), device=dev)
        K = nx * ny
        out = torch.empty((n, K), dtype=torch.float32, device=dev)
        keep += [pts, out]
        add(f"scan_{K}", lambda p=pts, o=out, K=K: _lib.check(
            L.rex_height_scan(h, p.data_ptr(), K, 1, None, n, o.data_ptr(), sp), "rex_height_scan"), n * K)
    add("step", lambda: env.step(actions[0]))

    def window(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls

    calls = {}
    for name, (fn, _) in cases.items():       # warm-up and calibration
        window(fn, 20)
        per = window(fn, 200)
        calls[name] = max(200, int(args.window / per) + 1)
    times = {name: [] for name in cases}
    for _ in range(3):
        for name, (fn, _) in cases.items():
            times[name].append(window(fn, calls[name]))
    res = {"what": "median of three alternating windows, seconds per call, host clock around a window that ends in a device synchronise",
           "device": torch.cuda.get_device_name(0), "envs": n, "steps_before": args.steps, "window_s": args.window, "cases": {}}
    for name, (fn, work) in cases.items():
        t = sorted(times[name])
        med = t[1]
        c = {"us_per_call": round(med * 1e6, 2), "min_us": round(t[0] * 1e6, 2), "max_us": round(t[2] * 1e6, 2), "calls_per_window": calls[name]}
        if work:
            c["mitems_per_s"] = round(work / med / 1e6, 1)      # rays (depth) or points (scan) per second
        res["cases"][name] = c
    step = res["cases"]["step"]["us_per_call"]
    for W, H in SIZES:
        s, r = res["cases"][f"sense_{W}x{H}"], res["cases"][f"render_{W}x{H}"]
        s["render_over_sense"] = round(r["us_per_call"] / s["us_per_call"], 3)
        s["share_of_step"] = round(s["us_per_call"] / step, 4)
    for nx, ny in SCANS:
        c = res["cases"][f"scan_{nx * ny}"]
        c["share_of_step"] = round(c["us_per_call"] / step, 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    env.close()


if __name__ == "__main__":
    main()
