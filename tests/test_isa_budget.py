"""Instruction budget guard (no GPU needed: hipcc cross-compiles): the float32 full-band kernel's sample loop.

k_bands<float, 0, 1, false> is VALU-issue bound, so its time follows the number of VALU
instructions a wave issues per sample.  tools/isa_sections.py counts them statically from the ISA: `always` is the
straight-line part every (wave, sample) issues, `cond` the forward-skipped regions (regime branches) a wave issues only
when one of its lanes needs them.  The bounds below are the figures of the instruction diet (EXPERIMENTS.md section B,
round 7: 252 + 70 before it); a change that adds instructions back to the loop fails here before it costs GPU time."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ALWAYS_MAX = 235
TOTAL_MAX = 307          # always + cond
TRANS_MAX = 18


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def test_float32_sample_loop_valu_budget():
    if _hipcc() is None:
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("isa_sections", os.path.join(ROOT, "tools", "isa_sections.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    src = S.build.SOURCES[1]
    frag = "k_bandsIfLi0ELi1ELb0E"
    secmap, k0, k1 = S.section_of_source_lines()
    _, counts, total = S.budget(S.asm_with_lines(src), frag, secmap, k0, k1)
    assert total == S.product_valu_count(src, frag), "-gline-tables-only changed the code"
    valu = sum(c["valu"] + c["trans"] for c in counts.values())
    cond = sum(c["cond"] for c in counts.values())
    trans = sum(c["trans"] for c in counts.values())
    assert valu - cond <= ALWAYS_MAX, {s: dict(c) for s, c in counts.items()}
    assert valu <= TOTAL_MAX, {s: dict(c) for s, c in counts.items()}
    assert trans <= TRANS_MAX, {s: dict(c) for s, c in counts.items()}
