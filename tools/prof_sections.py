#!/usr/bin/env python3
"""Cycle breakdown of one physics substep inside rex_step_kernel (developer tool, needs a GPU).

Builds the library with -DREX_PROF (clock64() stamps around the sections of physics_substep, accumulated per
workgroup by lane 0) into scratch/librexsim_prof.so, runs walk-IK at N envs and prints cycles per substep for:
leg factorisation, base Cholesky, row finishing, PGS sweeps, back-substitution + integration.
  python tools/prof_sections.py [N=4096] [--arm] [--task=standup|poses|...] [--roll=R] [--body=0|1] [--rebuild] [--stagger] [--cert] [--critical[=LAUNCHES]]
--stagger: the pre-roll of bench.py -- a random 1 / 32 of the batch reset every 50 of the first 1 300 pre-roll steps -- instead of a
           synchronised batch: the stationary episode-age mix of the headline, with freshly reset (capped) envs in it
--critical: the critical path of a launch instead of means over workgroups: the counters are read and cleared around every one of LAUNCHES
           (default 100) launches of the steady mix, the wave whose end (start tick + length on the 100 MHz counter) is the launch's latest is
           picked, and ITS section split is averaged over the launches -- the cycles that move a one-launch-per-step figure.  Implies --stagger.
--cert:    which certificate rows for the residual on demand (csrc/rex_device.h REX_CERT_ROW_MASK): a library of its own, built with
           -DREX_PROF_CERT_SETS=<CERT_SETS below> (scratch/librexsim_prof_cert.so, or REX_PROF_LIB=...), counts per candidate set the WAVE
           sweeps in which the out-of-line block would have run -- some running env of the wave left undecided
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# the candidate certificate sets of --cert, bit r = toe row r (rows 0-7: the normals of points 2 L, 2 L + 1 of leg L; rows 8 + 2 k, 9 + 2 k: the
# friction pair of point k); 12 of them (g_prof3[35..46]).  The one list: the library gets it as a define.
CERT_SETS = [0x55, 0xAA, 0x99, 0x66, 0x9D, 0xBD, 0x9F, 0x3F, 0x90, 0x91, 0x4199, 0x410099]
CERT = "--cert" in sys.argv
so = os.environ.get("REX_PROF_LIB") or os.path.join(ROOT, "scratch", "librexsim_prof_cert.so" if CERT else "librexsim_prof.so")   # REX_PROF_LIB: a prebuilt library (A/B)
os.makedirs(os.path.dirname(so), exist_ok=True)
import rex_gym_amd.build as b
if not os.path.exists(so) or "--rebuild" in sys.argv:
    b.build(force=True, lib_path=so, defines=["-DREX_PROF"] + (["-DREX_PROF_CERT_SETS=" + ",".join("%#xu" % m for m in CERT_SETS)] if CERT else []),
            unity=True)   # one translation unit: the counters are one device global
b.LIB_PATH = so
import torch
from rex_gym_amd import RexBatchEnv, _lib

L = _lib.lib()
L.rex_debug_prof.argtypes = [ctypes.c_void_p, ctypes.c_int]
L.rex_debug_prof2.argtypes = [ctypes.c_void_p, ctypes.c_int]
HAVE_PROF3 = hasattr(L, "rex_debug_prof3")      # (a -DREX_PROF library of a commit before the residual on demand has none: A/B runs)
if HAVE_PROF3:
    L.rex_debug_prof3.argtypes = [ctypes.c_void_p, ctypes.c_int]
CRITICAL = next((int(a.split("=")[1]) if "=" in a else 100 for a in sys.argv if a.startswith("--critical")), 0)
STAGGER = "--stagger" in sys.argv or CRITICAL > 0
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 4096
mark = "arm" if "--arm" in sys.argv else "base"
task = next((a.split("=")[1] for a in sys.argv if a.startswith("--task=")), "walk")
extra = {}
for a in sys.argv:
    if a.startswith("--roll="):
        extra["base_roll"] = float(a.split("=")[1])          # poses: every env holds this roll (the self-collision regime at -0.74)
    if a.startswith("--body="):
        extra["body_contacts"] = bool(int(a.split("=")[1]))
env = RexBatchEnv(n, check_actions=False, task=task, signal_type="ol" if task == "standup" else "ik", seed=0, auto_reset=True, max_episode_steps=2000, mark=mark,
                  **extra)
env.reset()
_lo = torch.as_tensor(env.action_space.low, device="cuda").minimum(torch.as_tensor(env.action_space.high, device="cuda"))
acts = [torch.rand((n, env.action_dim), device="cuda") * (-2 * _lo) + _lo for _ in range(8)]


def window(steps, label):
    torch.cuda.synchronize()
    L.rex_debug_prof(None, 1)
    L.rex_debug_prof2(None, 1)
    if HAVE_PROF3:
        L.rex_debug_prof3(None, 1)
    for k in range(steps):
        env.step(acts[k % 8])
    torch.cuda.synchronize()
    out = np.zeros((1024, 10), np.int64)
    L.rex_debug_prof(out.ctypes.data, 0)
    out2 = np.zeros((1024, 16), np.int64)
    L.rex_debug_prof2(out2.ctypes.data, 0)
    out3 = np.zeros((1024, 48), np.int64)
    if HAVE_PROF3:
        L.rex_debug_prof3(out3.ctypes.data, 0)
    keep = out[:, 4] > 0
    out3 = out3[keep].astype(float)
    out2 = out2[out[:, 4] > 0].astype(float)
    out = out[out[:, 4] > 0].astype(float)
    pgs, sw, tot, fin, sub, legs, chol = (out[:, i] for i in (0, 1, 2, 3, 4, 6, 7))
    rest = tot - pgs - fin - legs - chol
    fb = out[:, 5]
    print(f"{label}: {len(out)} workgroups sampled, sweeps/substep mean {np.mean(sw / sub):.1f} (slowest workgroup "
          f"{np.max(sw / sub):.1f}), cycles/sweep {pgs.sum() / sw.sum():.0f}, joint-limit rows in reach in "
          f"{100 * fb.sum() / sub.sum():.2f} % of the substeps")
    print("  cycles/step (whole kernel, per wave): mean %.0f, slowest workgroup %.0f; inside physics_substep %.0f" %
          (np.mean(out[:, 8] / out[:, 9]), np.max(out[:, 8] / out[:, 9]), np.mean(tot / out[:, 9])))
    print("  cycles/substep: total %.0f (slowest workgroup %.0f) = legs %.0f + base chol %.0f + finish rows %.0f + pgs %.0f "
          "+ back-subst/integrate %.0f" % (np.mean(tot / sub), np.max(tot / sub), np.mean(legs / sub), np.mean(chol / sub),
                                           np.mean(fin / sub), np.mean(pgs / sub), np.mean(rest / sub)))
    if out2[:, 7].sum() > 0:     # start times of the blocks of the last launch (10 ns ticks), its own length from the same counter
        st = out2[:, 7] - out2[:, 7].min()
        dur = out2[:, 6] / out[:, 9]
        print("  last launch: block starts spread over %.1f us (median %.1f, p90 %.1f); a block runs %.1f us (mean; max %.1f); "
              "latest end %.1f us after the first start" % (st.max() / 100, np.median(st) / 100, np.percentile(st, 90) / 100,
                                                          dur.mean() / 100, dur.max() / 100, (st + dur).max() / 100))
    if out2[:, 6].sum() > 0:
        print("  clock64() ticks per 10 ns tick of the constant 100 MHz counter over the kernel: %.2f  (a clock64 tick = %.3f ns)" %
              (out[:, 8].sum() / out2[:, 6].sum(), 10.0 * out2[:, 6].sum() / out[:, 8].sum()))
    if out2[:, 4].sum() > 0:
        print("  step = load + command (planner, IK) %.0f + substeps (motors, physics, observation ring) %.0f + reward / done / reset / observation / stores %.0f" %
              tuple(np.mean(out2[:, k] / out[:, 9]) for k in (3, 4, 5)))
    if out2[:, 1].sum() > 0:     # lane-group kernels: inside the pgs section
        su, lp, hb = (np.mean(out2[:, k] / sub) for k in range(3))
        print("  pgs = row couplings %.0f + sweep set-up %.0f + sweep loop %.0f (%.0f per sweep) + hand-back %.0f" %
              (np.mean(pgs / sub) - su - lp - hb, su, lp, out2[:, 1].sum() / sw.sum(), hb))
    # the workgroup that ends the launch: its own sections, and what its sweeps are made of (thread 0's sweeps: an env that has
    # converged no longer counts its wave's rows)
    w = int(np.argmax(tot / sub))
    print("  SLOWEST workgroup, cycles/substep: total %.0f = legs %.0f + base chol %.0f + finish rows %.0f + pgs %.0f + back-subst/integrate %.0f; "
          "%.1f sweeps/substep" % (tot[w] / sub[w], legs[w] / sub[w], chol[w] / sub[w], fin[w] / sub[w], pgs[w] / sub[w], rest[w] / sub[w], sw[w] / sub[w]))
    if out2[w, 10:14].sum() > 0:
        nsw = max(out2[w, 14], 1.0)
        c = out2[w, 10:14] / nsw
        print("    per sweep: %.1f link-box rows + %.1f joint-limit rows + 24 toe rows; cycles: limit rows %.0f, link-box normals %.0f, toe rows %.0f, "
              "link-box friction %.0f (sum %.0f of %.0f per sweep)" % (out2[w, 8] / nsw, out2[w, 9] / nsw, c[0], c[1], c[2], c[3], c.sum(), out2[w, 1] / nsw))
        nsa = max(out2[:, 14].sum(), 1.0)
        ca = out2[:, 10:14].sum(0) / nsa
        print("    all workgroups, per sweep: %.1f link-box rows + %.1f joint-limit rows; cycles: limit rows %.0f, link-box normals %.0f, toe rows %.0f, "
              "link-box friction %.0f" % (out2[:, 8].sum() / nsa, out2[:, 9].sum() / nsa, ca[0], ca[1], ca[2], ca[3]))
    if out3[:, 47].sum() > 0:
        # the sweep boundary of thread 0's env: end of toe row 23 -> start of row 1 of its next sweep (row 0, the exit tests, the loop)
        print("  sweep boundary (row 23 -> row 1 of the next sweep): %.0f cycles, all workgroups (%.0f boundaries); %.0f in the slowest workgroup" %
              (out2[:, 15].sum() / out3[:, 47].sum(), out3[:, 47].sum(), out2[w, 15] / max(out3[w, 47], 1)))
    if out3[:, 17:34].sum() > 0:
        # per WAVE sweep (whatever thread 0's env does), binned by the envs of the wave that still ran when the sweep began: does the
        # `if (running)` lane mask cost a partly stopped wave anything?
        cyc, cnt = out3[:, 0:17].sum(0), out3[:, 17:34].sum(0)
        nsw = cnt.sum()
        print("  wave sweeps %.0f, %.0f cycles each; by envs still running: " % (nsw, cyc.sum() / nsw) +
              ", ".join("%d: %.0f cycles (%.1f %%)" % (k, cyc[k] / cnt[k], 100 * cnt[k] / nsw) for k in range(17) if cnt[k] > 0))
        taken = out3[:, 34]
        wsw = out3[:, 17:34].sum(1)
        print("  out-of-line residual block: taken in %.2f %% of the wave sweeps (all workgroups), %.2f %% in the slowest workgroup "
              "(%.1f wave sweeps/substep there)" % (100 * taken.sum() / nsw, 100 * taken[w] / max(wsw[w], 1), wsw[w] / sub[w]))
        if CERT:
            # mean instructions of the residual per wave sweep = 1.5 per certificate row in the block (fma + half a max3) + taken share x
            # 2.5 per other row out of line (sub + fma + half a max3); 36 with every term in its row.  "long solves": the 5 % of the
            # workgroups with the most sweeps -- the waves that end a launch
            long_wg = wsw >= np.percentile(wsw, 95)
            for c, mask in enumerate(CERT_SETS):
                rows = bin(mask).count("1")
                f_all, f_l, f_w = out3[:, 35 + c].sum() / nsw, out3[long_wg, 35 + c].sum() / wsw[long_wg].sum(), out3[w, 35 + c] / max(wsw[w], 1)
                cost = lambda f: 1.5 * rows + f * 2.5 * (24 - rows)
                print("    set %#08x (%d rows): would be taken in %.2f %% of the wave sweeps (long solves %.2f %%, slowest workgroup %.2f %%); residual "
                      "instructions per sweep %.1f (long solves %.1f, slowest %.1f) of 36" % (mask, rows, 100 * f_all, 100 * f_l, 100 * f_w, cost(f_all), cost(f_l), cost(f_w)))


# sections of one wave, cycles: (label, counters of that wave -> value).  o = g_prof row, o2 = g_prof2 row
CRIT_SECTIONS = [
    ("command: load, planner, IK", lambda o, o2: o2[3]),
    ("substeps outside the physics: motors, observation ring", lambda o, o2: o2[4] - o[2]),
    ("legs", lambda o, o2: o[6]),
    ("base Cholesky, predicted velocity", lambda o, o2: o[7]),
    ("finish rows + couplings (one loop: no stamp between them)", lambda o, o2: o[3]),
    ("pgs outside pgs_dv: votes, parking", lambda o, o2: o[0] - o2[0] - o2[1] - o2[2]),
    ("sweep set-up", lambda o, o2: o2[0]),
    ("sweep loop", lambda o, o2: o2[1]),
    ("hand-back", lambda o, o2: o2[2]),
    ("back-substitution, integration", lambda o, o2: o[2] - o[0] - o[3] - o[6] - o[7]),
    ("epilogue: reward, reset, observation, stores", lambda o, o2: o2[5]),
    ("kernel entry and exit", lambda o, o2: o[8] - o2[3] - o2[4] - o2[5]),
]


PROF_BLOCKS = 1024      # workgroups the library's counters cover (csrc/rex_device.h g_prof: blockIdx.x < 1024)


def critical(launches, cap_sweeps):
    """Per launch: the wave that ended it, and its sections.  Averages over the launches, next to the mean wave of the same launches.
    cap_sweeps: wave sweeps per step of a wave that runs every solve to the cap."""
    epw = env._L.rex_envs_per_wave(env._h)
    blocks = (n + epw - 1) // epw
    # a launch of more workgroups than the counters cover could end with a wave they never saw
    assert blocks <= PROF_BLOCKS, "--critical: %d envs at %d per wave are %d workgroups, the counters cover the first %d" % (n, epw, blocks, PROF_BLOCKS)
    crit = np.zeros((launches, len(CRIT_SECTIONS)))
    mean = np.zeros((launches, len(CRIT_SECTIONS)))
    tot, sweeps, toe, span, lead = (np.zeros(launches) for _ in range(5))
    out, out2 = np.zeros((PROF_BLOCKS, 10), np.int64), np.zeros((PROF_BLOCKS, 16), np.int64)
    for k in range(launches):
        torch.cuda.synchronize()
        L.rex_debug_prof(None, 1)
        L.rex_debug_prof2(None, 1)
        env.step(acts[k % 8])
        torch.cuda.synchronize()
        L.rex_debug_prof(out.ctypes.data, 0)
        L.rex_debug_prof2(out2.ctypes.data, 0)
        ran = out[:, 9] > 0
        o, o2 = out[ran].astype(float), out2[ran].astype(float)
        end = o2[:, 7] + o2[:, 6]                       # 10 ns ticks
        order = np.argsort(end)
        w = order[-1]
        crit[k] = [f(o[w], o2[w]) for _, f in CRIT_SECTIONS]
        mean[k] = [np.mean(f(o.T, o2.T)) for _, f in CRIT_SECTIONS]
        tot[k], sweeps[k], toe[k] = o[w, 8], o[w, 1], o2[w, 12]
        span[k] = (end[w] - o2[:, 7].min()) / 100.0     # us from the first start to the last end
        lead[k] = (end[w] - end[order[-2]]) / 100.0 if len(order) > 1 else 0.0
    print("critical wave of %d launches (%d envs, %s-%s, staggered resets): the wave whose end is the launch's latest" % (launches, n, task, mark))
    print("  its kernel %.0f cycles (mean wave %.0f); launch span first start -> last end %.1f us; it ends %.2f us behind the next-to-last wave; "
          "%.1f wave sweeps per step (%.0f %% of the launches at the full cap of %d)" %
          (tot.mean(), mean.sum(1).mean(), span.mean(), lead.mean(), sweeps.mean(), 100 * np.mean(sweeps >= cap_sweeps), cap_sweeps))
    print("  %-62s %10s %7s   %10s %7s" % ("section (cycles per step, summed over its substeps)", "critical", "share", "mean wave", "share"))
    for j, (label, _) in enumerate(CRIT_SECTIONS):
        print("  %-62s %10.0f %6.1f %%   %10.0f %6.1f %%" % (label, crit[:, j].mean(), 100 * crit[:, j].mean() / tot.mean(), mean[:, j].mean(),
                                                             100 * mean[:, j].mean() / mean.sum(1).mean()))
    print("  of the sweep loop, toe-row blocks of thread 0's env (stamped inside the sweep: the stamps themselves lengthen it): %.0f cycles" % toe.mean())
    return crit, mean


if CRITICAL:
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    for k in range(1500):
        env.step(acts[k % 8])
        if k % 50 == 0 and k < 1300:      # bench.py Rollout.preroll
            env.reset(torch.randperm(n, device="cuda", generator=g)[: max(1, n // 32)].to(torch.int32))
    critical(CRITICAL, 300)      # action_repeat x int(300 / action_repeat) sweeps: 5 x 60 or 6 x 50 (rex_gym_env.py:184)
    sys.exit(0)
window(20, "first 20 steps after reset")
g = torch.Generator(device="cuda"); g.manual_seed(1)
for k in range(1500):
    env.step(acts[k % 8])
    if STAGGER and k % 50 == 0 and k < 1300:      # bench.py Rollout.preroll
        env.reset(torch.randperm(n, device="cuda", generator=g)[: max(1, n // 32)].to(torch.int32))
window(100, "steady state (after 1500 steps%s)" % (", staggered resets" if STAGGER else ""))
