"""The toe-row block of the paired-sweep base kernels with the residual formed on demand (csrc/rex_device.h,
REX_RESIDUAL_ON_DEMAND), checked on the compiled kernels; no GPU needed: hipcc cross-compiles gfx950 here (tools/check_dpp_masks.py,
a quarter of a minute for the base group).

A row's residual term is `v_fma_f32 t, -thr, invd, |dl|`: the only fma of the sweep with an absolute-value source.  Inside each of
the two row blocks (one per impulse set) only the certificate rows may form it; the other rows' terms sit in one block behind each
row block, which holds no friction clamp -- it recomputes no row.  And the row block is shorter than the parent commit's by the
terms that left it (PARENT: the parent's rex_step_base.hip compiled with the library's flags; profiles/residual_on_demand.md).
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCROW = 24
PARENT = {4: (313, 315), 8: (317, 318), 16: (318, 318)}      # instructions of the two row blocks before this change, in the kernel's order
pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.fixture(scope="module")
def compiled():
    env = dict(os.environ)
    env["PATH"] = env.get("PATH", "") + ":/opt/rocm/bin"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_masks.py"), "step_base"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    ncert = int(re.search(r"^certificate rows of the toe-row block: (\d+)", r.stdout, re.M).group(1))
    return open(os.path.join(ROOT, "scratch", "isa", "rex_step_base-hip-amdgcn-amd-amdhsa-gfx950.s")).read(), ncert


def _kernel_lines(s, epw):
    m = re.search(r"^(\S*kernel%s\S*):" % re.escape(f"ILi{epw}ELb0ELb0ELb0E"), s, re.M)
    body = s[m.start():s.index(".Lfunc_end", m.start())]
    lines = [l.strip().split(";")[0].strip() for l in body.split("\n")]
    return [l for l in lines if l]


def _clusters(idx, gap):
    out = []
    for i in idx:
        if out and i - out[-1][-1] < gap:
            out[-1].append(i)
        else:
            out.append([i])
    return out


def _row_blocks(lines):
    """(first, last + 1) line of every toe-row block: found by its 16 friction clamps, bounded by the labels around it and the
    first instruction behind it that names a label (the exit to the out-of-line terms: the second block is followed by them directly)."""
    spans = []
    for c in _clusters([i for i, l in enumerate(lines) if l.startswith("v_med3_f32")], 60):
        if len(c) != 16:
            continue
        a = max([i for i in range(c[0] - 170, c[0]) if lines[i].endswith(":")] or [c[0] - 170])
        b = min([i for i in range(c[-1], c[-1] + 80) if lines[i].endswith(":") or re.search(r"\.LBB\d+_\d+", lines[i])] or [c[-1] + 40])
        spans.append((a, b))
    return spans


def _is_residual_term(l):
    return l.startswith("v_fma_f32") and re.search(r"\|v\d+\|", l) is not None


@pytest.mark.parametrize("epw", [4, 8, 16])
def test_row_blocks_form_the_residual_of_the_certificate_rows_only(compiled, epw):
    s, ncert = compiled
    assert 1 <= ncert <= 6
    lines = _kernel_lines(s, epw)
    spans = _row_blocks(lines)
    assert len(spans) == 2, "the base kernels run their sweeps in pairs (two impulse sets): two row blocks"
    for (a, b), parent in zip(spans, PARENT[epw]):
        block = [l for l in lines[a:b] if not l.endswith(":")]
        assert sum(_is_residual_term(l) for l in block) == ncert, (epw, a, b)
        assert sum(l.startswith("v_med3_f32") for l in block) == 16
        assert sum(l.startswith("v_max3_f32") for l in block) <= (ncert + 1) // 2, epw      # the terms fold two at a time
        assert len(block) <= parent - 24, (epw, len(block), parent)


@pytest.mark.parametrize("epw", [4, 8, 16])
def test_the_other_rows_terms_sit_behind_the_row_blocks_and_recompute_no_row(compiled, epw):
    s, ncert = compiled
    lines = _kernel_lines(s, epw)
    spans = _row_blocks(lines)
    lo, hi = spans[0][0], spans[-1][1] + 1200         # the sweep loop: the two row blocks and what follows them
    outside = [i for i in range(lo, hi) if _is_residual_term(lines[i]) and not any(a <= i < b for a, b in spans)]
    tails = [c for c in _clusters(outside, 4) if len(c) == NCROW - ncert]
    assert len(tails) == 2, (epw, [len(c) for c in _clusters(outside, 4)])
    for c in tails:
        assert not any(l.startswith("v_med3_f32") for l in lines[c[0]:c[-1] + 1]), epw
        assert sum(l.startswith("v_max3_f32") for l in lines[c[0]:c[-1] + 8]) <= (NCROW - ncert + 1) // 2 + 1, epw
