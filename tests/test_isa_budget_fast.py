"""Instruction budget guard of BOTH sample-loop bodies of the float32 full-band kernel k_bands<float, 0, 1, false> (no GPU
needed: hipcc cross-compiles).  A 32-sample stage whose samples all share the film thickness and all have cbc = prot = 0 runs
the common-case body (the benchmark's config 4 and the usual LUT setting: PROSPECT-5D leaf, one film); any other stage runs
the general body.  tools/isa_sections.py ranks the innermost loops by VALU count: the general body first, the common-case body
second.  Bounds: round 8 (EXPERIMENTS.md section B; 235 + 72 before it, one body)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

GENERAL = dict(always=223, total=295, trans=18)
COMMON = dict(always=218, total=290, trans=17)


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def bodies():
    if _hipcc() is None:
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("isa_sections", os.path.join(ROOT, "tools", "isa_sections.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    src = S.build.SOURCES[1]
    frag = "k_bandsIfLi0ELi1ELb0E"
    secmap, k0, k1 = S.section_of_source_lines()
    lines = S.asm_with_lines(src)
    out = []
    for rank in (0, 1):
        _, counts, total = S.budget(lines, frag, secmap, k0, k1, rank)
        assert total == S.product_valu_count(src, frag), "-gline-tables-only changed the code"
        valu = sum(c["valu"] + c["trans"] for c in counts.values())
        cond = sum(c["cond"] for c in counts.values())
        trans = sum(c["trans"] for c in counts.values())
        out.append((dict(always=valu - cond, total=valu, trans=trans), {s: dict(c) for s, c in counts.items()}))
    return out


def test_general_body_budget(bodies):
    got, detail = bodies[0]
    assert all(got[k] <= GENERAL[k] for k in GENERAL), (got, detail)


def test_common_body_budget(bodies):
    got, detail = bodies[1]
    assert all(got[k] <= COMMON[k] for k in COMMON), (got, detail)


def test_common_body_leaves_out_the_film_exponential_and_the_pro_terms(bodies):
    """the common-case body issues one transcendental (the film's exp2) and at least four plain instructions fewer per sample
    (the film multiply, the two PRO FMAs of K)"""
    (g, gd), (c, cd) = bodies
    assert c["trans"] == g["trans"] - 1, (g, c)
    assert c["always"] <= g["always"] - 4, (g, c)
    assert cd["leaf_band"]["valu"] + cd["leaf_band"]["trans"] <= gd["leaf_band"]["valu"] + gd["leaf_band"]["trans"] - 2, (gd, cd)
