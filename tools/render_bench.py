#!/usr/bin/env python3
"""Time the renderer (RexBatchEnv.render -> rex_render / rex_render_visual): 4 096 walk-IK envs at 64 x 64 and 1 env at
480 x 360.  --geometry visual draws the URDF's visual meshes read under --data-path (the folder holding assets/urdf/);
--geometry both times the two renderers in the same run, collision first.

Every timed call is one render() on the env's stream, bracketed by device events (end to end as a caller sees it on the
device: the Python wrapper issues the output allocations and the one launch; no host sync inside the loop).  Prints one
JSON line: per case the median and p10 / p90 of the per-call times in ms, and the rays per second of the median.
Run it a second time under `rocprofv3 --kernel-trace --stats -- python tools/render_bench.py` for the kernel's own time.

    python tools/render_bench.py [--calls 200] [--warmup 20] [--geometry collision|visual|both] [--data-path DIR]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def time_case(env, torch, calls, warmup, **kw):
    for _ in range(warmup):
        env.render(**kw)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        env.render(**kw)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--geometry", default="collision", choices=["collision", "visual", "both"])
    ap.add_argument("--data-path", default=None, help="rex_gym.util.pybullet_data.getDataPath() (default: an installed rex_gym's)")
    args = ap.parse_args()
    geoms = ["collision", "visual"] if args.geometry == "both" else [args.geometry]
    import numpy as np
    import torch
    from rex_gym_amd import RexBatchEnv
    out = {"what": "RexBatchEnv.render end-to-end per call (device events around the wrapper's allocations + one render launch)",
           "calls": args.calls, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name, n, w, h in (("walk_ik_4096_64x64", 4096, 64, 64), ("single_480x360", 1, 480, 360)):
        env = RexBatchEnv(n, task="walk", signal_type="ik", seed=0, check_actions=False)
        env.reset()
        rng = np.random.RandomState(0)
        for _ in range(10):     # a few steps so that the legs are not all in the reset pose
            env.step(torch.as_tensor(rng.uniform(-0.4, 0.4, (n, 2)).astype(np.float32), device=env.device))
        for geom in geoms:
            if geom == "visual" and getattr(env, "_visuals", None) is None:
                vm = env.load_visual_meshes(args.data_path)
                out["visual_load_s"] = round(vm.seconds, 3)
            ms = time_case(env, torch, args.calls, args.warmup, width=w, height=h, geometry=geom)
            med = ms[len(ms) // 2]
            key = name if geom == "collision" and len(geoms) == 1 else f"{name}_{geom}"
            out[key] = {"envs": n, "width": w, "height": h, "geometry": geom, "median_ms": round(med, 5),
                        "p10_ms": round(ms[len(ms) // 10], 5), "p90_ms": round(ms[(9 * len(ms)) // 10], 5),
                        "mrays_per_s": round(n * w * h / med / 1e3, 1)}
        env.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
