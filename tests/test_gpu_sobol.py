"""spart_sobol on the GPU, Sentinel-2A: the raw C ABI against the definition tools/sobol_defined.py, bit for bit in all six
outputs, with the library's own float64 pruned column path (Engine.run on the table the definition builds) as the definition's
forward model; guard words behind every buffer; a site that crosses the 2^19-row chunk and a middle site that straddles a chunk
boundary among many; NULL outputs; the exact zeros of equal designs and of DOY; the permutation; Engine.sobol / spart_amd.sobol
against the raw call; the example; the refusals that need a context.  If a mismatch shows here and not in
tests/test_sobol_host.py, the cause is in the kernels' index maps or the cross-lane tree, not in the formula."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, torch_mod  # noqa: F401 (fixture)
from helpers.sobol_calls import (FILL, FREE, OUTS, S2, bounds_of, check_sobol, cols_of, design_of, differing, forward_of, same, sd,
                                 sites_of, sobol_call)

pytestmark = pytest.mark.gpu
INDEX_KEYS = ("S1", "ST", "S1_se", "ST_se")


@pytest.fixture(scope="module")
def eng(torch_mod):
    from spart_amd import get_engine
    return get_engine(S2, 0)


@pytest.fixture(scope="module")
def plain(torch_mod, eng):
    """F = 3, N = 192, M = 3 on R_TOC: the case of the NULL, Engine and refusal tests -> (base, names, uA, uB, ref)"""
    base, (uA, uB) = sites_of(3), design_of(192, 3, seed=1)
    ref, _ = check_sobol(torch_mod, eng, base, FREE[3], uA, uB, what="F 3 N 192 M 3")
    return base, FREE[3], uA, uB, ref


@pytest.mark.parametrize("F,N,M,column,band_model", [(1, 128, 1, 0, 0), (3, 128, 2, 0, 0), (3, 128, 2, 1, 0), (3, 128, 2, 2, 0),
                                                     (16, 128, 1, 0, 0), (3, 192, 3, 1, 0), (2, 128, 1, 0, 1)])
def test_definition_bit_for_bit(torch_mod, eng, F, N, M, column, band_model):
    base, (uA, uB) = sites_of(M, seed=F + N), design_of(N, F, seed=F)
    ref, _ = check_sobol(torch_mod, eng, base, FREE[F], uA, uB, column=column, band_model=band_model,
                         what=f"F {F} N {N} M {M} column {column} band_model {band_model}")
    assert np.isfinite(ref["S1"]).all() and (ref["var"] > 0).all()                      # (not vacuous:
    assert (ref["ST"].max(axis=2) > 0.1).all() and (ref["ST_se"].max(axis=2) > 0).all()       # every band has a parameter that moves it)


def test_a_site_across_the_chunk_boundary(torch_mod, eng):
    """F = 1, N = 2^18: 786 432 rows, 4096 blocks of 192 rows in chunks of 2730 blocks"""
    N = 1 << 18
    uA, uB = design_of(N, 1, seed=3)
    check_sobol(torch_mod, eng, sites_of(1), FREE[1], uA, uB, what="F 1 N 2^18 M 1")


def test_a_middle_site_straddles_a_chunk_boundary(torch_mod, eng):
    """F = 2, N = 192: blocks of 256 rows, 2048 per chunk, 3 per site, so site 682 of 684 has blocks 2046, 2047 in the first
    chunk and 2048 in the second; it gives the same bits run alone"""
    F, N, M = 2, 192, 684
    assert ((1 << 19) // (64 * (F + 2))) % (N // 64) != 0 and M * (N // 64) > (1 << 19) // (64 * (F + 2))
    base, (uA, uB) = sites_of(M, seed=8), design_of(N, F, seed=4)
    _, got = check_sobol(torch_mod, eng, base, FREE[F], uA, uB, what="F 2 N 192 M 684")
    free, (lo, hi) = cols_of(FREE[F]), bounds_of(FREE[F])
    m = ((1 << 19) // (64 * (F + 2))) // (N // 64)
    assert m == 682
    rc, alone = sobol_call(torch_mod, eng, base[m:m + 1], free, lo, hi, uA, uB)
    assert rc == 0 and all(same(alone[k][0], got[k][m]) for k in OUTS)
    # the workspace is one chunk's whatever M is
    need = lambda M_: int(eng.lib.spart_sobol_workspace_bytes(eng.ctx, M_, N, F))      # noqa: E731
    assert need(M) == need(10 * M) == need(2000000000) and 0 < need(1) < need(M)


def test_any_subset_of_outputs_may_be_null(torch_mod, eng, plain):
    base, names, uA, uB, ref = plain
    free, (lo, hi) = cols_of(names), bounds_of(names)
    for null in (("S1_se", "ST_se"), ("mean", "var"), ("mean", "var", "S1", "ST", "S1_se"), ("var", "S1", "ST", "S1_se", "ST_se"), ("S1", "ST_se")):
        rc, got = sobol_call(torch_mod, eng, base, free, lo, hi, uA, uB, null=null)
        assert rc == 0, null
        for k in OUTS:
            assert (got[k] == FILL).all() if k in null else same(got[k], ref[k]), (null, k)


def test_equal_designs_doy_and_the_permutation(torch_mod, eng, plain):
    base, names, uA, uB, ref = plain
    free, (lo, hi) = cols_of(names), bounds_of(names)
    rc, got = sobol_call(torch_mod, eng, base, free, lo, hi, uA, uA)
    assert rc == 0 and all((got[k] == 0).all() for k in INDEX_KEYS) and (got["var"] > 0).all()
    # DOY is read by L_TOA alone: exact zeros for it in R_TOC and R_TOA, and the others keep their bits
    rng = np.random.default_rng(6)
    uA4, uB4 = np.column_stack([uA, rng.random(192)]), np.column_stack([uB, rng.random(192)])
    for column in (0, 1):
        rc, with_doy = sobol_call(torch_mod, eng, base, free + [26], np.append(lo, 1.0), np.append(hi, 365.0), uA4, uB4, column=column)
        rc3, without = sobol_call(torch_mod, eng, base, free, lo, hi, uA, uB, column=column)
        assert rc == 0 and rc3 == 0 and all((with_doy[k][:, :, 3] == 0).all() for k in INDEX_KEYS)
        assert same(with_doy["mean"], without["mean"]) and same(with_doy["var"], without["var"])
        assert all(same(with_doy[k][:, :, :3], without[k]) for k in INDEX_KEYS)
    rc, lt = sobol_call(torch_mod, eng, base, free + [26], np.append(lo, 1.0), np.append(hi, 365.0), uA4, uB4, column=2)
    assert rc == 0 and (lt["ST"][:, :, 3] > 0).all()                       # (L_TOA does read it)
    p = [2, 0, 1]
    rc, perm = sobol_call(torch_mod, eng, base, [free[i] for i in p], lo[p], hi[p], uA[:, p], uB[:, p])
    assert rc == 0 and same(perm["mean"], ref["mean"]) and same(perm["var"], ref["var"])
    assert all(same(perm[k], ref[k][:, :, p]) for k in INDEX_KEYS)


def test_engine_and_host_forms_are_the_raw_call(torch_mod, eng, plain):
    import spart_amd
    base, names, uA, uB, ref = plain
    res = eng.sobol(torch_mod.as_tensor(base.T.copy(), device=eng.device), names, design=(uA, uB))
    assert res["names"] == names and not differing({k: res[k].cpu().numpy() for k in OUTS}, ref)
    host = spart_amd.sobol(base.T, S2, names, design=(uA, uB))
    assert host["names"] == names and not differing(host, ref)
    # the default design is sobol_design's, and a scalar site broadcasts
    one = spart_amd.sobol(list(base[0]), S2, names, N=128, seed=5, column="R_TOA")
    want = spart_amd.sobol(base[:1].T, S2, names, design=spart_amd.sobol_design(128, 3, seed=5), column="R_TOA")
    assert one["S1"].shape == (1, eng.nb, 3) and not differing(one, want)
    srf = spart_amd.sobol(base[:1].T, S2, names[:2], design=(uA[:128, :2], uB[:128, :2]), band_model="srf")
    want = sd.sobol_defined(base[:1], cols_of(names[:2]), *bounds_of(names[:2]), uA[:128, :2], uB[:128, :2], forward_of(torch_mod, eng, 0, 1))
    assert not differing(srf, want)


def test_the_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sobol.py"), "256"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("tts = ") == 3 and r.stdout.count("band ") == 3 * 13 and "largest total index" in r.stdout


def test_refusals_that_need_a_context(torch_mod, eng, plain):
    from spart_amd import get_engine
    base, names, uA, uB, _ = plain
    free, (lo, hi) = cols_of(names), bounds_of(names)
    need = int(eng.lib.spart_sobol_workspace_bytes(eng.ctx, 3, 192, 3))
    for kw, code, text in ((dict(ctx=get_engine(None, 0).ctx), -4, "no sensor"), (dict(ws_bytes=need - 1), -3, f"{need} bytes needed"),
                           (dict(null=("ws",)), -3, "bytes needed"), (dict(N=100), -1, "N = 100"), (dict(null=("base[26]",)), -1, "base[26] is null"),
                           (dict(null=OUTS), -1, "every output is null")):
        rc, got = sobol_call(torch_mod, eng, base, free, lo, hi, uA, uB, **kw)
        assert rc == code and text in eng.lib.spart_last_error(eng.ctx).decode(), (kw, rc, eng.lib.spart_last_error(eng.ctx))
        assert all((got[k] == FILL).all() for k in OUTS), kw                # (nothing was written)
    rc, got = sobol_call(torch_mod, eng, base, free, lo, hi, uA, uB, M=0)
    assert rc == 0 and all((got[k] == FILL).all() for k in OUTS)
    for sizes in ((0, 192, 3), (3, 100, 3), (3, 64, 3), (3, 1 << 21, 3), (3, 192, 0), (3, 192, 17), (2000000001, 192, 3)):
        assert eng.lib.spart_sobol_workspace_bytes(eng.ctx, *sizes) == 0, sizes
    assert eng.lib.spart_sobol_workspace_bytes(get_engine(None, 0).ctx, 3, 192, 3) == 0
