"""Build the HIP extension in-tree: rex_gym_amd/librexsim_hip.so (gfx950, hipcc cross-compiles without a GPU).

The library is compiled variant group by variant group -- one translation unit per group of rex_step_kernel /
rex_settle_kernel instantiations (csrc/rex_step_*.hip, rex_settle_*.hip) next to the C ABI (csrc/rexsim.hip) -- in
parallel, then linked (34 jobs, see variant_jobs(): every step unit once per mode it offers) where the single translation
unit took over 2 minutes.

Developer knobs (never needed for the product build):
  REX_LIB_PATH=<path>     write / load the library somewhere else (A/B builds)
  REX_BUILD_ONLY=base,arm compile only these variant groups' kernels; launching another group's is an error return (REX_EINVAL)
  build(defines=[...], unity=True)  one translation unit (tools/prof_sections.py: -DREX_PROF keeps its counters in one
                          device global)
"""
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.environ.get("REX_LIB_PATH") or os.path.join(PKG_DIR, "librexsim_hip.so")   # REX_LIB_PATH: developer A/B builds
# variant group names in the order of csrc/rex_kernels.h RexStepGroup (REX_BUILD_ONLY; the bit numbers of -DREX_LEFT_OUT_GROUPS)
GROUP_NAMES = ["base", "arm", "mixed_base", "mixed_arm", "body"]
# translation unit -> variant group name; rexsim.hip (the simulator's C ABI, launcher table, reset and controller kernels) and rex_learner.hip
# (the fused PPO learners: their kernels and entry points) are always built
GROUPS = {**{"rex_step_%s.hip" % g: g for g in GROUP_NAMES}, "rex_settle_base.hip": "base", "rex_settle_arm.hip": "arm"}
# (the renderers -- rex_render, rex_render_visual -- are one kernel each, no variants; rexsim.hip last: a unity build includes it behind the
# units whose launchers its table names)
SOURCES = sorted(GROUPS) + ["rex_render.hip", "rex_render_mesh.hip", "rex_sense.hip", "rex_kinematics.hip", "rex_dynamics.hip",
                            "rex_dynamics_solve.hip", "rex_contact_solve.hip", "rex_contact_space.hip", "rex_force_distribution.hip", "rex_rollout.hip", "rex_outcome.hip", "rex_learner.hip",
                            "rexsim.hip"]
# units compiled into another unit's object (that unit includes them at its end): the onboard sensors ride with the collision renderer,
# whose ray functions they cast with, and so do the kinematics and dynamics readouts, the solves with the mass matrix, the contact
# solve, the contact-space readout, the force distribution and the candidate rollouts, which walk the renderer's forward kinematics, and
# the step's epilogue as a readout, whose device function the rollout kernel calls -- dependencies of the library like every source, but no objects of their own
INCLUDED_IN = {"rex_sense.hip": "rex_render.hip", "rex_kinematics.hip": "rex_render.hip", "rex_dynamics.hip": "rex_render.hip",
               "rex_dynamics_solve.hip": "rex_render.hip", "rex_contact_solve.hip": "rex_render.hip", "rex_contact_space.hip": "rex_render.hip",
               "rex_force_distribution.hip": "rex_render.hip", "rex_rollout.hip": "rex_render.hip", "rex_outcome.hip": "rex_render.hip"}
# the modes a step unit is compiled in (csrc/rex_kernels.h RexStepMode, where the reason for each is recorded) and their object-file tags
MODES = {"STEP": "", "TRACE": "_trace", "SEG": "_seg", "POL": "_pol", "RNN": "_rnn"}


def variant_offered(group, mode, motor):
    """csrc/rex_kernels.h rex_step_variant_offered: the fused actor in the single-task toes-only groups, the per-env actuator
    parameters (MOTOR) in the segment-shaped modes."""
    actor = mode in ("POL", "RNN")
    return (not actor or group in ("base", "arm")) and (not motor or mode == "SEG" or actor)


def variant_jobs():
    """(source, object-file tag, defines) of every object of the library: the step units once per offered (mode, MOTOR), then the
    settle units and the sources without variants."""
    jobs = []
    for motor in (False, True):
        for mode, tag in MODES.items():
            for g in GROUP_NAMES:
                if variant_offered(g, mode, motor):
                    defines = ([] if mode == "STEP" else ["-DREX_TU_MODE=REX_MODE_" + mode]) + (["-DREX_TU_MOT=1"] if motor else [])
                    jobs.append(("rex_step_%s.hip" % g, ("_m" + tag[1:]) if motor else tag, defines))
    return jobs + [(s, "", []) for s in SOURCES if not s.startswith("rex_step_") and s not in INCLUDED_IN]


HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))   # every header the sources can include
# -ffp-contract=on: a * b + c inside one expression is one fma and nothing else is fused -- the arithmetic of a kernel is fixed by its
# source and does not depend on what else is compiled into it (hipcc's default lets the backend fuse across statements by heuristics:
# the _trace instantiations then differ from the product kernels in the last bit).  csrc/rex_kernels.h repeats it as a pragma; the
# flag also covers the HIP headers' inline functions.  tools/kres.sh, kstat.sh and check_dpp_masks.py compile with COMPILE_FLAGS too.
COMPILE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on"]
HIPCC_FLAGS = COMPILE_FLAGS + ["-fPIC", "-fvisibility=hidden"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the rexsim HIP extension cannot be built")


def _flags_stamp():
    # the compile flags fix the kernels' arithmetic (-ffp-contract=on): a flags-only edit of this file must rebuild too
    import hashlib
    return hashlib.sha256(repr((HIPCC_FLAGS, variant_jobs())).encode()).hexdigest()[:16]


def needs_build(lib_path=None):
    lib_path = lib_path or LIB_PATH
    if not os.path.exists(lib_path):
        return True
    try:
        with open(lib_path + ".flags") as f:
            if f.read().strip() != _flags_stamp():
                return True
    except OSError:
        return True
    t = os.path.getmtime(lib_path)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.join(PKG_DIR, "..", "include", "rexsim.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def _stamp(lib_path, defines, only):
    if not defines and not only:          # (developer builds with extra defines / left-out groups are never "up to date")
        with open(lib_path + ".flags", "w") as f:
            f.write(_flags_stamp() + "\n")


def build(force=False, verbose=False, lib_path=None, defines=(), unity=False, only=None, jobs=None):
    """Compile csrc/*.hip -> librexsim_hip.so. Returns the library path."""
    lib_path = lib_path or LIB_PATH
    if not force and not needs_build(lib_path):
        return lib_path
    hipcc = _hipcc()
    only = only if only is not None else os.environ.get("REX_BUILD_ONLY")
    left_out = set(GROUP_NAMES) - set(only.split(",")) if only else set()
    flags = HIPCC_FLAGS + list(defines) + ["-I", CSRC]
    if left_out:   # rexsim.hip's launcher table holds nullptr for these groups (step and settle): launching one is an error return
        flags.append("-DREX_LEFT_OUT_GROUPS=%d" % sum(1 << GROUP_NAMES.index(g) for g in left_out))
    todo = [j for j in variant_jobs() if GROUPS.get(j[0]) not in left_out]
    with tempfile.TemporaryDirectory(prefix="rexsim_build_") as tmp:
        if unity:
            uni = os.path.join(tmp, "unity.hip")
            with open(uni, "w") as f:
                for s, _, defs in todo:   # one explicit specialisation of rex_launch_step per inclusion: the template arguments tell them apart
                    macros = {"REX_TU_MODE": "REX_MODE_STEP", "REX_TU_MOT": "0", **dict(d[2:].split("=") for d in defs)}
                    f.write("".join("#undef %s\n#define %s %s\n" % (k, k, v) for k, v in macros.items()) + '#include "%s"\n' % os.path.join(CSRC, s))
            cmd = [hipcc] + flags + ["-shared", uni, "-o", lib_path]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            _stamp(lib_path, defines, only)
            return lib_path
        jobs_list = []
        for s, tag, defs in todo:
            obj = os.path.join(tmp, s[:-4] + tag + ".o")
            jobs_list.append(([hipcc] + flags + defs + ["-c", os.path.join(CSRC, s), "-o", obj], obj))

        def run(job):
            if verbose:
                print(" ".join(job[0]), flush=True)
            subprocess.check_call(job[0])
            return job[1]

        with ThreadPoolExecutor(max_workers=jobs or min(len(jobs_list), os.cpu_count() or 4)) as pool:
            objs = list(pool.map(run, jobs_list))
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", lib_path]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        _stamp(lib_path, defines, only)
    return lib_path


DIAG_LIB_PATH = os.path.join(PKG_DIR, "librexsim_hip_diag.so")
DIAG_INSIDE = "0.3"      # rad; oracle/Makefile DIAG_INSIDE is the same number


def build_diag(force=False, verbose=False):
    """The DIAGNOSTIC twin of the library for one parity test (tests/test_gpu_parity.py::test_mark_arm_window_with_quiet_arm_rows): the mark-arm
    variant groups compiled with -DREX_DIAG_ARM_REST_INSIDE=0.3 (csrc/rex_arm_model_gen.h: the arm's rest targets 0.3 rad inside their
    bounds instead of 0.1 rad beyond them).  Never loaded by the product: rex_gym_amd._lib loads LIB_PATH; the test points REX_LIB_PATH
    at this file in a subprocess."""
    if not force and os.path.exists(DIAG_LIB_PATH) and \
            all(os.path.getmtime(os.path.join(CSRC, f)) <= os.path.getmtime(DIAG_LIB_PATH) for f in SOURCES + HEADERS):
        return DIAG_LIB_PATH
    return build(force=True, verbose=verbose, lib_path=DIAG_LIB_PATH, defines=[f"-DREX_DIAG_ARM_REST_INSIDE={DIAG_INSIDE}"], only="arm,mixed_arm")


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    if "--diag" in __import__("sys").argv:
        print(build_diag(force=True, verbose=True))
