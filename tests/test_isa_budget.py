"""Instruction and register budget guard of the float32 full-band kernel k_bands<float, 0, 1, false> (no GPU needed: hipcc
cross-compiles).

The kernel is VALU-issue bound, so its time follows the number of VALU instructions a wave issues per
sample.  tools/isa_sections.py counts them statically from the ISA: `always` is the straight-line part every (wave, sample)
issues, `cond` the forward-skipped regions (regime branches) a wave issues only when one of its lanes needs them.  The kernel
has two sample-loop bodies: a 32-sample stage whose samples all share the film thickness and all have cbc = prot = 0 runs the
common-case body (the benchmark's config 4 and the usual LUT setting: PROSPECT-5D leaf, one film); any other stage runs the
general body.  isa_sections ranks the innermost loops by VALU count: the general body first, the common-case body second.

Where each bound comes from (EXPERIMENTS.md section B):
  round 7  one body: always <= 235, always + cond <= 307, transcendentals <= 18 (252 + 70 before it); the check that
           -gline-tables-only, which the attribution needs, does not change the code
  round 8  two bodies: general 223 / 295 / 18, common 218 / 290 / 17; the three relations between the bodies
           (test_common_body_leaves_out_the_film_exponential_and_the_pro_terms)
  round 9  general 217 / 284 / 18, common 207 / 274 / 17 -- the bounds asserted below, which imply those of rounds 7 and 8;
           the film powers leave the common body's soil section; at most 96 VGPRs, nothing spilled
A change that adds instructions back to a loop fails here before it costs GPU time."""
import importlib.util
import os

import pytest

from conftest import ROOT
from helpers.compiled_meta import compiled
from helpers.kernel_meta import device_asm

GENERAL = dict(always=217, total=284, trans=18)
COMMON = dict(always=207, total=274, trans=17)
VGPRS = 96                    # five waves per SIMD
FRAG = "k_bandsIfLi0ELi1ELb0E"


@pytest.fixture(scope="module")
def bodies():
    """[(figures, counts by section) of the general body, the same of the common-case body].  Two compiles of the float32
    unit in a process: the shared one behind kernel_meta, and one with -gline-tables-only here."""
    compiled()
    spec = importlib.util.spec_from_file_location("isa_sections", os.path.join(ROOT, "tools", "isa_sections.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    src = S.build.SOURCES[1]
    secmap, k0, k1 = S.section_of_source_lines()
    lines = S.asm_with_lines(src)
    product = S.valu_count(device_asm()[os.path.basename(src)].split("\n"), FRAG)
    out = []
    for rank in (0, 1):
        _, counts, total = S.budget(lines, FRAG, secmap, k0, k1, rank)
        assert total == product, "-gline-tables-only changed the code"
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


def test_the_film_powers_leave_the_common_body(bodies):
    """the common-case body forms p tw1^k once per stage: its soil section issues at least seven instructions fewer than the
    general body's (the film's exp2 and multiply, five power multiplies)"""
    (_, gd), (_, cd) = bodies
    n = lambda d: d["soil"]["valu"] + d["soil"]["trans"]
    assert n(cd) <= n(gd) - 7, (gd["soil"], cd["soil"])


def test_register_budget():
    """<= 96 VGPRs (five waves per SIMD), nothing spilled"""
    hits = [k for name, k in compiled().items() if FRAG in name]
    assert hits, FRAG
    for meta in hits:
        assert meta["vgpr_count"] <= VGPRS and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
        assert meta["private_segment_fixed_size"] == 0, meta
