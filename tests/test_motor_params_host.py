"""Host-side checks of the per-env actuator parameters (no GPU): the ctypes mirror of RexMotorRandom, the header's declarations,
and the self-consistency of tests/golden/motor_rollout_golden.npz."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rex_set_motor_params", "rex_set_motor_randomization", "rex_get_motor_params", "rex_motor_torque_params")


def test_motor_random_struct_layout():
    from rex_gym_amd import _lib
    assert ctypes.sizeof(_lib.RexMotorRandom) == 11 * 4
    names = [f[0] for f in _lib.RexMotorRandom._fields_]
    assert names == ["strength_lo", "strength_hi", "voltage_lo", "voltage_hi", "damping_lo", "damping_hi", "kp_lo", "kp_hi", "kd_lo", "kd_hi",
                     "strength_per_motor"]
    assert all(getattr(_lib.RexMotorRandom, n).offset == 4 * k for k, n in enumerate(names))
    # ... in the order the header writes them
    hdr = open(os.path.join(ROOT, "include", "rexsim.h")).read()
    body = re.search(r"typedef struct RexMotorRandom \{(.*?)\} RexMotorRandom;", hdr, re.S).group(1)
    assert re.findall(r"\b(\w+_(?:lo|hi)|strength_per_motor)\b", body) == names


def test_header_declares_the_entry_points_and_keeps_the_abi():
    from rex_gym_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rexsim.h")).read()
    declared = set(re.findall(r"REX_API\s+[\w\s\*]+?\b(rex_\w+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS, name
    assert re.search(r"#define\s+REX_ABI_VERSION\s+6\b", hdr) and _lib.ABI_VERSION == 6     # new entry points only
    lib = _lib.lib()                                                                      # (loads without a GPU)
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.rex_set_motor_params(None, None) == -1 and b"null sim" in lib.rex_last_error()


def test_fixture_is_self_consistent():
    z = np.load(os.path.join(ROOT, "tests", "golden", "motor_rollout_golden.npz"))
    meta = json.loads(str(z["meta"]))
    assert [f["name"] for f in meta["families"]] == ["walk_ik", "gallop_ol", "walk_ik_arm"]
    assert [len(f["scenarios"]) for f in meta["families"]] == [6, 7, 2]
    for fam in meta["families"]:
        nm = fam["num_motors"]
        scs = fam["scenarios"]
        assert sum(sc["nominal"] for sc in scs) == 1 and scs[0]["nominal"]
        nominal = z[scs[0]["key"] + "/body"][:, 13:13 + nm]
        for sc in scs:
            body, p = z[sc["key"] + "/body"], sc["params"]
            assert body.shape == (meta["steps"], 13 + 2 * nm) and not z[sc["key"] + "/done"].any()
            assert np.array_equal(z[sc["key"] + "/action"], z[scs[0]["key"] + "/action"])          # one action tape per family
            assert len(p["strength"]) == nm
            if sc["nominal"]:
                assert p == dict(strength=[1.0] * nm, voltage=32.0, damping=0.0, kp=1.0, kd=0.02) and sc["separation"] == 0.0
            else:
                sep = float(np.abs(body[:, 13:13 + nm] - nominal).max())
                assert sc["separation"] == pytest.approx(sep, rel=1e-12) and sep >= meta["min_separation"] == 1e-2
                # the reset motion is the nominal robot's: every scenario starts from the nominal reset state
                assert np.array_equal(z[sc["key"] + "/reset_body"], z[scs[0]["key"] + "/reset_body"])
    par = z["ctl_par"]
    assert par.shape[0] >= 1000 and z["ctl_actual"].shape == z["ctl_observed"].shape == (par.shape[0],)
    for col, (lo, hi) in enumerate(((0.5, 1.5), (0.0, 0.05), (20.0, 36.0), (0.0, 0.1), (0.5, 1.3))):      # kp, kd, voltage, damping, strength
        assert lo <= par[:, col].min() and par[:, col].max() <= hi and np.ptp(par[:, col]) > 0.8 * (hi - lo)
    assert np.abs(z["ctl_actual"]).max() <= 3.5 * 1.3 and np.abs(z["ctl_observed"]).max() <= 5.7
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "motor_rollout_golden.npz")) < 2 ** 20
