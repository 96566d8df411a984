"""The controller readout and the action-space rollouts, the parts that need no GPU: the C ABI's declarations (include/rexsim.h) and their
ctypes mirror (rex_gym_amd/_lib.py), the struct layouts against the static_asserts of csrc/rexsim.hip, the workspace size, the refusals
the arguments alone decide, and the Python argument checks (tests/test_gpu_rollout_actions.py runs the calls on the MI355X)."""
import ctypes
import inspect
import os
import re

import pytest

from rex_gym_amd import _lib, build, rollout_actions as ra
from rex_gym_amd._lib import RexRolloutActionsIn, RexRolloutActionsOut          # (a tree without the calls fails here: no test of this file passes on it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rexsim.h")).read()
CSRC = os.path.join(ROOT, "rex_gym_amd", "csrc")
CALLS = ("rex_command", "rex_rollout_actions_workspace_bytes", "rex_rollout_actions")


def strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_three_calls_and_the_two_structs_and_keeps_the_abi_version():
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", HEADER))
    assert set(CALLS) <= declared and declared == set(_lib.EXPORTED_SYMBOLS)
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", HEADER) and _lib.ABI_VERSION == 6
    for name, cls in (("RexRolloutActionsIn", RexRolloutActionsIn), ("RexRolloutActionsOut", RexRolloutActionsOut)):
        body = strip(re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1))
        members = re.findall(r"(\w+)\s*;", body)
        assert members == [f[0] for f in cls._fields_], name
    flat = re.sub(r"\s+", " ", strip(HEADER))
    assert ("REX_API int rex_command(RexSim* sim, const int32_t* d_env_ids, int n, int candidates, const float* d_actions, const float* d_state, "
            "const float* d_ctrl, float* d_targets, float* d_ctrl_next, void* stream);") in flat
    assert "REX_API long long rex_rollout_actions_workspace_bytes(int n, int candidates);" in flat
    assert ("REX_API int rex_rollout_actions(RexSim* sim, const int32_t* d_env_ids, int n, const RexRolloutActionsIn* in, const RexRolloutFrom* from, "
            "const RexRolloutActionsOut* out, void* d_workspace, long long workspace_bytes, void* stream);") in flat
    assert len(_lib._SIGS["rex_command"][0]) == 10 and len(_lib._SIGS["rex_rollout_actions"][0]) == 9
    # what the header must say of the readout: noise, the inputs taken as given, the layout, the clock
    low = HEADER.lower()
    assert "sensor noise is not drawn" in low and "garbage in that row only" in HEADER and "no address is formed from an action" in low
    assert "time-major" in low and "the controller's clock stays the env's" in low


def test_struct_layouts_against_the_static_asserts_and_the_pinned_structs():
    src = open(os.path.join(CSRC, "rexsim.hip")).read()
    sizes = re.search(r"static_assert\(sizeof\(RexRolloutActionsIn\) == (\d+) && sizeof\(RexRolloutActionsOut\) == (\d+)", src)
    assert sizes and ctypes.sizeof(RexRolloutActionsIn) == int(sizes.group(1)) == 40 and ctypes.sizeof(RexRolloutActionsOut) == int(sizes.group(2)) == 56
    offsets = dict((("%s.%s" % (s, m)), int(v)) for s, m, v in re.findall(r"offsetof\((RexRolloutActions\w+), (\w+)\) == (\d+)", src))
    assert len(offsets) == 4
    for key, off in offsets.items():
        s, m = key.split(".")
        assert getattr(getattr(_lib, s), m).offset == off, key
    assert [getattr(RexRolloutActionsIn, f[0]).offset for f in RexRolloutActionsIn._fields_] == [0, 8, 16, 20, 24, 28, 32, 36]
    assert [getattr(RexRolloutActionsOut, f[0]).offset for f in RexRolloutActionsOut._fields_] == [0, 8, 16, 24, 32, 40, 48]
    assert [f[0] for f in RexRolloutActionsIn._fields_][2:] == [f[0] for f in _lib.RexRolloutIn._fields_][2:]              # shape and settings as RexRolloutIn's
    assert [f[0] for f in RexRolloutActionsOut._fields_][:4] == [f[0] for f in _lib.RexRolloutOut._fields_]
    assert ctypes.sizeof(_lib.RexRolloutIn) == 40 and ctypes.sizeof(_lib.RexRolloutOut) == 32 and ctypes.sizeof(_lib.RexRolloutFrom) == 24      # pinned
    # the rollout unit keeps its one kernel; the command kernel lives with the ABI's controller kernels and restates no controller code
    assert open(os.path.join(CSRC, "rex_rollout.hip")).read().count("__global__") == 1
    assert '#include "rex_command.h"' in src and "rex_command.h" in build.HEADERS and len(build.variant_jobs()) == 34
    kernel = open(os.path.join(CSRC, "rex_command.h")).read()
    assert kernel.count("__global__") == 1
    for call in ("walk_command<1>(", "gallop_command<1>(", "turn_command<1>(", "standup_command<1>(", "poses_command(", "env_gait_ik<1>("):
        assert kernel.count(call) == 1, call
    assert "gait_loop" not in kernel and "ik_solve" not in kernel and "fp contract" not in kernel
    assert kernel.index("env_gait_ik<1>(") < kernel.index("if (!inrows) return;")          # nobody leaves in front of the ballot


def test_workspace_bytes():
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    for n, K in ((1, 1), (5, 3), (67, 2), (4096, 32), (2 ** 20, 2 ** 10)):
        assert L.rex_rollout_actions_workspace_bytes(n, K) == 4 * n * K * (2 * 37 + 2 * 8 + 12) == 4 * ra.workspace_floats(n, K)
    for n, K in ((0, 1), (1, 0), (-1, 4), (2 ** 16, 2 ** 15), (2 ** 31 - 1, 2)):
        assert L.rex_rollout_actions_workspace_bytes(n, K) == -1


def test_every_refusal_the_arguments_alone_decide_comes_without_a_device():
    assert os.path.exists(build.LIB_PATH) and not build.needs_build(), "the library is missing or older than its sources: build it first"
    L = _lib.lib()
    buf = (ctypes.c_float * 512)()
    p = ctypes.addressof(buf)
    In, out, empty, src = RexRolloutActionsIn, RexRolloutActionsOut(ctrl=p), RexRolloutActionsOut(), _lib.RexRolloutFrom(p, p, p)
    good = In(p, None, 1, 1, 1, 0.0, 0, -1.0)
    nan, inf, big = float("nan"), float("inf"), 1 << 40
    calls = [(None, src, out, p, big, b"null pointer"), (good, None, out, p, big, b"null pointer"), (good, src, None, p, big, b"null pointer"),
             (In(None, p, 1, 1, 1, 0.0, 0, -1.0), src, out, p, big, b"null actions"), (good, src, empty, p, big, b"every output pointer is null"),
             (good, src, out, None, big, b"workspace"), (good, src, out, p, 407, b"workspace"), (In(p, None, 3, 1, 1, 0.0, 0, -1.0), src, out, p, 3 * 408 - 1, b"workspace"),
             (In(p, None, 0, 1, 1, 0.0, 0, -1.0), src, out, p, big, b"candidates 0"), (In(p, None, -3, 1, 1, 0.0, 0, -1.0), src, out, None, 0, b"candidates -3"),
             (In(p, None, 1, 0, 1, 0.0, 0, -1.0), src, out, p, big, b"steps 0"), (In(p, None, 1, 4097, 0, 0.0, 0, -1.0), src, out, p, big, b"at most 4096 substeps"),
             (In(p, None, 1, 1025, 4, 0.0, 0, -1.0), src, out, p, big, b"at most 4096 substeps"), (In(p, None, 1, 1, 1, 0.0, 1001, -1.0), src, out, p, big, b"iterations 1001"),
             (In(p, None, 1, 1, 1, inf, 0, -1.0), src, out, p, big, b"finite"), (In(p, None, 1, 1, 1, 0.0, 0, nan), src, out, p, big, b"finite"),
             (good, src, out, p, 408, b"null sim"), (In(p, p, 3, 1024, 4, 0.001, 1000, 0.0), _lib.RexRolloutFrom(), out, p, big, b"null sim")]
    ref = lambda x: ctypes.byref(x) if x is not None else None
    for inp, s, o, w, wb, msg in calls:
        rc = L.rex_rollout_actions(None, None, 1, ref(inp), ref(s), ref(o), w, wb, None)
        assert rc == -1 and L.rex_last_error().startswith(b"rex_rollout_actions: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    for args, msg in (((1, 1, None, p, p, p, p), b"null actions"), ((1, 1, p, p, p, None, None), b"every output pointer is null"), ((1, 0, p, None, None, p, None), b"candidates 0"),
                      ((1, 1, p, None, None, p, p), b"null sim"), ((1, 7, p, p, p, None, p), b"null sim")):
        rc = L.rex_command(None, None, *args, None)
        assert rc == -1 and L.rex_last_error().startswith(b"rex_command: ") and msg in L.rex_last_error(), (msg, L.rex_last_error())
    assert all(v == 0.0 for v in buf)


def stub_env(**kw):
    import torch
    cfg = _lib.RexConfig()
    cfg.action_repeat = 5
    env = type("StubEnv", (), dict(_torch=torch, device=torch.device("cpu"), action_dim=2, num_envs=5, mark="base", task="walk", config=cfg))()
    for k, v in kw.items():
        setattr(env, k, v)
    return env


def test_python_checks_of_the_arguments():
    import torch
    env, k, K, T = stub_env(), 5, 3, 4
    a, K1, T1 = ra.check_actions(env, torch.zeros((T, k, K, 2)), k, "rollout_actions", True)
    assert (K1, T1) == (K, T) and a.shape == (T, k, K, 2)
    a, K1, T1 = ra.check_actions(env, torch.zeros((T, k, 2)), k, "rollout_actions", True)
    assert (K1, T1) == (1, T) and a.shape == (T, k, 1, 2) and a.is_contiguous()
    a, K1, T1 = ra.check_actions(env, torch.zeros((k, 2)), k, "command", False)
    assert (K1, T1) == (1, 1) and a.shape == (k, 1, 2)
    assert ra.check_actions(env, torch.zeros((k, K, 2)), k, "command", False)[1:] == (K, 1)
    for t, major in ((torch.zeros((T, k, K, 3)), True), (torch.zeros((T, k + 1, K, 2)), True), (torch.zeros((T, k, K, 2)).double(), True), (torch.zeros((T, k, K, 4))[..., ::2], True),
                     (torch.zeros((0, k, K, 2)), True), (torch.zeros((T, k, 0, 2)), True), (torch.zeros((k, 2)), True), (torch.zeros((T, k, K, 2)).numpy(), True),
                     (torch.zeros((T, k, K, 2)), False), (torch.zeros((k, K, 3)), False), (torch.zeros(2), False), ([[0.0, 0.0]] * k, False)):
        with pytest.raises(ValueError) as e:
            ra.check_actions(env, t, k, "who", major)
        assert str(e.value).startswith("who: actions")
    # per-row inputs
    one = torch.arange(k * 8, dtype=torch.float32).reshape(k, 8)
    spread = ra.check_rows(env, one, k, K, 8, "who", "ctrl")
    assert spread.shape == (k, K, 8) and spread.is_contiguous() and all(torch.equal(spread[:, j], one) for j in range(K))
    full = torch.zeros((k, K, 37))
    assert ra.check_rows(env, full, k, K, 37, "who", "state") is full and ra.check_rows(env, None, k, K, 37, "who", "state") is None
    for t in (full[:4], full[..., :36], full.double(), full.numpy(), torch.zeros((k, K, 74))[..., ::2], torch.zeros((k, 36)), torch.zeros((k, 1, 37))):
        with pytest.raises(ValueError) as e:
            ra.check_rows(env, t, k, K, 37, "who", "state")
        assert str(e.value).startswith("who: state")
    # env ids: in range, none twice
    env._row_ids = lambda ids, who: (ids, len(ids))
    assert ra.row_ids(env, [3, 0, 4], "who") == ([3, 0, 4], 3)
    with pytest.raises(ValueError) as e:
        ra.row_ids(env, [3, 0, 3], "who")
    assert "twice" in str(e.value)
    # the envs the calls do not cover, before anything else is looked at
    cfg = _lib.RexConfig(); cfg.pd_latency = 0.003
    rack = _lib.RexConfig(); rack.on_rack = 1
    boxes = _lib.RexConfig(); boxes.body_contacts = 1
    with pytest.raises(NotImplementedError):
        ra.command(stub_env(mark="arm"), None)
    for env_kw in (dict(task="mixed"), dict(config=cfg)):
        for call in (lambda e: ra.command(e, None), lambda e: ra.run(e, None)):
            with pytest.raises(ValueError):
                call(stub_env(**env_kw))
    for c in (rack, boxes):
        with pytest.raises(ValueError):
            ra.run(stub_env(config=c), None)
        ra.check_sim(stub_env(config=c), "command", physics=False)                         # the controller alone reads neither
    # shapes of the result, the public signatures
    assert ra.field_shape("state", k, K, T) == (k, K, 37) and ra.field_shape("ctrl", k, K, T) == (k, K, 8) and ra.field_shape("sweeps", k, K, T) == (T, k, K)
    assert ra.field_shape("trajectory", k, K, T) == (T, k, K, 37) and ra.field_shape("targets", k, K, T) == (T, k, K, 12) and ra.field_shape("foot_contact", k, K, T) == (T, k, K, 4)
    ro = ra.ActionRollout({n: torch.zeros(ra.field_shape(n, k, K, T), dtype=getattr(torch, ra.FIELDS[n][2])) for n in ("state", "ctrl")}, k, K, T)
    ro.ctrl.view(torch.int32)[..., 6] = 7; ro.ctrl.view(torch.int32)[..., 7] = 12
    assert ro.fields == ("state", "ctrl") and len(ro) == 7 and ro[1] is None and ro.base_pos.shape == (k, K, 3) and ro.joint_rates.shape == (k, K, 12)
    assert ro.flags.dtype == torch.int32 and bool((ro.flags == 7).all()) and bool((ro.steps == 12).all()) and (ro.rows, ro.candidates, ro.horizon) == (k, K, T)
    from rex_gym_amd.envs import batch_env
    assert list(inspect.signature(batch_env.RexBatchEnv.command).parameters)[1:] == ["actions", "state", "ctrl", "env_ids", "out"]
    assert list(inspect.signature(batch_env.RexBatchEnv.rollout_actions).parameters)[1:] == [
        "actions", "repeat", "init_state", "ctrl", "base_wrench", "body", "env_ids", "fields", "out", "dt", "iterations", "residual_threshold"]
