"""Instruction budget guard of both sample-loop bodies of k_bands<float, 0, 1, false> after the third diet (no GPU needed:
hipcc cross-compiles).  A per-stage vote carries one per-sample fact into the loop as a scalar bit (whether a J2 of SAILH can
reach its Taylor side), the film series takes its powers p tw1^k from outside the per-sample part, and the sample's LDS address
lives in one VGPR.  tools/isa_sections.py ranks the innermost loops by VALU count: the general body first, the common-case
body second.  Bounds: round 9 (EXPERIMENTS.md section B; 223 / 218 always before it)."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

GENERAL = dict(always=217, total=284, trans=18)
COMMON = dict(always=207, total=274, trans=17)
VGPRS = 96                    # five waves per SIMD
FRAG = "k_bandsIfLi0ELi1ELb0E"


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def compiled():
    if _hipcc() is None:
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("isa_sections", os.path.join(ROOT, "tools", "isa_sections.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    src = S.build.SOURCES[1]
    secmap, k0, k1 = S.section_of_source_lines()
    lines = S.asm_with_lines(src)
    out = []
    for rank in (0, 1):
        _, counts, total = S.budget(lines, FRAG, secmap, k0, k1, rank)
        assert total == S.product_valu_count(src, FRAG), "-gline-tables-only changed the code"
        valu = sum(c["valu"] + c["trans"] for c in counts.values())
        cond = sum(c["cond"] for c in counts.values())
        trans = sum(c["trans"] for c in counts.values())
        out.append((dict(always=valu - cond, total=valu, trans=trans), {s: dict(c) for s, c in counts.items()}))
    return out, lines


def test_general_body_budget(compiled):
    got, detail = compiled[0][0]
    assert all(got[k] <= GENERAL[k] for k in GENERAL), (got, detail)


def test_common_body_budget(compiled):
    got, detail = compiled[0][1]
    assert all(got[k] <= COMMON[k] for k in COMMON), (got, detail)


def test_the_film_powers_leave_the_common_body(compiled):
    """the common-case body forms p tw1^k once per stage: its soil section issues at least seven instructions fewer than the
    general body's (the film's exp2 and multiply, five power multiplies)"""
    (_, gd), (_, cd) = compiled[0]
    n = lambda d: d["soil"]["valu"] + d["soil"]["trans"]
    assert n(cd) <= n(gd) - 7, (gd["soil"], cd["soil"])


def test_register_budget(compiled):
    """<= 96 VGPRs (five waves per SIMD), nothing spilled"""
    lines = compiled[1]
    i = next(k for k, l in enumerate(lines) if re.match(r"\s+\.name:\s+\S*" + FRAG, l))
    meta = {}
    for l in lines[i:i + 40]:
        m = re.match(r"\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", l)
        if m:
            meta.setdefault(m.group(1), int(m.group(2)))
    assert meta["vgpr_count"] <= VGPRS and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert meta["private_segment_fixed_size"] == 0, meta
