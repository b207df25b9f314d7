"""spart_sobol at its own edges, every case bit for bit against the definition tools/sobol_defined.py (check_sobol / sobol_call:
all six outputs of the raw C call, guard words behind every buffer and around the workspace; the definition's forward model is
the engine's float64 pruned column path under the call's own options):
  (a) more sites than workspace slots: a site's block sums and c_j wait in slot m % nslot, and a call with M > nslot reuses
      slots -- many small sites with the bound bc / G + 2 met with equality, few sites longer than a chunk, one site in three
      chunks; each case asserts its own chunk arithmetic (helpers/sobol_calls.layout_of / chunks_of, which
      tests/test_sobol_host.py holds against the header), so a change of SOBOL_ROWS cannot empty it unseen;
  (b) band counts: the wave -> (block, band) map of k_sobol_blocks with a tail workgroup, the entry -> (band, f) map of
      k_sobol_finish below, on and above a multiple of 64, on 1 ... 2162 bands, and the SRF band model on a second sensor;
  (c) fast_prelude and nlayers reach the forward model, raw and through Engine.sobol / spart_amd.sobol, and the forms of
      design, bounds and column that Engine.sobol takes;
  (d) what IEEE gives for a band that does not vary and for a NaN site among finite ones.
If a mismatch shows here and not in tests/test_sobol_host.py, the cause is in the kernels' index maps, the slots or the
cross-lane tree, not in the formula."""
import numpy as np
import pytest

from helpers.lut_calls import hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_srf_calls import L8, S3
from helpers.sobol_calls import (FREE, OUTS, S2, bounds_of, check_sobol, chunk_blocks, chunks_of, cols_of, design_of, differing,
                                 forward_of, layout_of, nan_signs, same, sd, sites_of, sobol_call)

pytestmark = pytest.mark.gpu
INDEX_KEYS = ("S1", "ST", "S1_se", "ST_se")


@pytest.fixture(scope="module")
def eng(torch_mod):
    from spart_amd import get_engine
    return get_engine(S2, 0)


def alone(torch, eng, base, names, uA, uB, got, sites, **kw):
    """each of ``sites`` run in a call of its own gives the bits it has in ``got``"""
    free, (lo, hi) = cols_of(names), bounds_of(names)
    for m in sites:
        rc, one = sobol_call(torch, eng, base[m:m + 1], free, lo, hi, uA, uB, **kw)
        assert rc == 0 and all(same(one[k][0], got[k][m]) for k in OUTS), m


# ---- (a) more sites than slots

def test_many_small_sites_reuse_the_slots(torch_mod, eng):
    """F = 2, N = 192, M = 1400: 3 blocks per site, 2048 per chunk, 684 slots, three launches.  The second launch is blocks
    2048 ... 4095 and touches sites 682 ... 1365: 684 sites, every slot; site 682 came in from the first launch (its c_j out of
    slot 682), sites 684 ... 1365 have slots 0 ... 681 of sites that are finished, and site 1365 goes on into the third launch,
    where its c_j comes out of the reused slot 681.  Site 700 is NaN (a NaN angle) among finite ones in the same launch and
    slot generation.  Sites on both sides of each cut, and the last, give the same bits alone; so does site 682 as site 0 of a
    call that begins with it."""
    F, N, M = 2, 192, 1400
    G, bcap, nslot = layout_of(F, N, M)
    assert (G, bcap, nslot) == (3, 2048, 684) and M > nslot and M * N * (F + 2) == 1075200
    assert chunks_of(F, N, M) == [(0, 2048, 0, 682), (2048, 2048, 682, 1365), (4096, 104, 1365, 1399)]
    assert 1365 - 682 + 1 == nslot == bcap // G + 2 and 1365 % nslot == 681 and 684 % nslot == 0
    base, (uA, uB) = sites_of(M, seed=12), design_of(N, F, seed=7)
    base[700, 20] = np.nan
    ref, got = check_sobol(torch_mod, eng, base, FREE[F], uA, uB, what="F 2 N 192 M 1400, site 700 NaN", nan_sites=[700])
    finite = np.arange(M) != 700
    assert np.isfinite(ref["S1"][finite]).all() and (ref["var"][finite] > 0).all() and (ref["ST"][finite].max(axis=2) > 0.1).all()
    alone(torch_mod, eng, base, FREE[F], uA, uB, got, (682, 683, 684, 700, 1365, 1399))
    # the same site at another phase of the slots: the call that begins with site 682 has it in slot 0 of its first launch
    free, (lo, hi) = cols_of(FREE[F]), bounds_of(FREE[F])
    assert layout_of(F, N, M - 682) == (3, 2048, 684) and chunks_of(F, N, M - 682)[0][2:] == (0, 682)
    rc, tail = sobol_call(torch_mod, eng, base[682:], free, lo, hi, uA, uB)
    assert rc == 0 and all(same(tail[k], got[k][682:]) for k in OUTS)


def test_sites_longer_than_a_chunk_share_two_slots(torch_mod, eng):
    """F = 16, N = 29 440, M = 3: 460 blocks per site and 455 per chunk, so two slots and four launches; every site crosses a
    cut, sites 0 and 1 and then 1 and 2 are in flight in one launch, and site 2 takes slot 0 after site 0 has left it.  The
    first case of several launches at the largest Q = 52.  Site 2 alone gives the same bits."""
    F, N, M = 16, 29440, 3
    G, bcap, nslot = layout_of(F, N, M)
    assert (G, bcap, nslot) == (460, 455, 2) and G > bcap == chunk_blocks(F) and M * N * (F + 2) == 1589760
    assert chunks_of(F, N, M) == [(0, 455, 0, 0), (455, 455, 0, 1), (910, 455, 1, 2), (1365, 15, 2, 2)]
    base, (uA, uB) = sites_of(M, seed=13), design_of(N, F, seed=8)
    ref, got = check_sobol(torch_mod, eng, base, FREE[F], uA, uB, what="F 16 N 29440 M 3")
    assert np.isfinite(ref["S1"]).all() and (ref["var"] > 0).all() and (ref["ST"].max(axis=2) > 0.1).all()
    assert not same(got["S1"][2], got["S1"][0])
    alone(torch_mod, eng, base, FREE[F], uA, uB, got, (2,))


def test_one_site_in_three_chunks(torch_mod, eng):
    """F = 16, N = 64 * 911: G = 2 * 455 + 1 blocks, so the one site is two whole launches and a launch of one block, and c_j
    comes out of cbuf twice"""
    F, M = 16, 1
    N = 64 * (2 * chunk_blocks(F) + 1)
    assert layout_of(F, N, M) == (911, 455, 1) and chunks_of(F, N, M) == [(0, 455, 0, 0), (455, 455, 0, 0), (910, 1, 0, 0)]
    uA, uB = design_of(N, F, seed=9)
    ref, _ = check_sobol(torch_mod, eng, sites_of(M, seed=14), FREE[F], uA, uB, what="F 16 N 58304 M 1")
    assert np.isfinite(ref["S1"]).all() and (ref["var"] > 0).all()


# ---- (b) band counts and sensors

# sensor, F, N, M, column, band_model; the columns in rotation.  Waves of k_sobol_blocks = M (N / 64) nb, four to a workgroup:
# no multiple of 4 on 1, 65, 211 and 2162 bands (6, 390, 1266 / 422 and 6486: a last workgroup of two waves).  Entries of
# k_sobol_finish = nb F, 64 to a block: 1 (one lane), 64 (one block exactly), 65 (one lane past it), 189, 633, 3376, 6486
BAND_CASES = [(L8, 3, 128, 2, 0, 0), (S3, 3, 128, 2, 1, 0), ("hyper211", 3, 128, 3, 2, 0), ("cut1", 1, 128, 3, 0, 0),
              ("cut63", 3, 128, 2, 1, 0), ("cut64", 1, 128, 2, 2, 0), ("cut65", 1, 128, 3, 0, 0), ("hyper211", 16, 128, 1, 1, 0),
              ("model2162", 3, 192, 1, 2, 0), (L8, 2, 128, 2, 1, 1), (S2, 2, 128, 1, 2, 1)]


def engine_of(sensor, hyper_si):
    from spart_amd import get_engine
    if sensor == "model2162":
        from test_gpu_hyperspectral import model_grid, synthetic_sensor
        return get_engine(None, 0, sensor_info=synthetic_sensor(model_grid())), 2162
    if sensor == "hyper211":
        return get_engine(None, 0, sensor_info=hyper_si), 211
    if sensor.startswith("cut"):
        from test_gpu_refine_edges import cut_bands
        return get_engine(None, 0, sensor_info=cut_bands(hyper_si, int(sensor[3:]))), int(sensor[3:])
    return get_engine(sensor, 0), {L8: None, S3: 21, S2: 13}[sensor]


@pytest.mark.parametrize("sensor,F,N,M,column,band_model", BAND_CASES, ids=[f"{c[0]}-F{c[1]}-column{c[4]}-model{c[5]}" for c in BAND_CASES])
def test_band_counts(torch_mod, hyper_si, sensor, F, N, M, column, band_model):
    assert {c[4] for c in BAND_CASES if not c[5]} == {0, 1, 2} and {c[4] for c in BAND_CASES if c[5]} == {1, 2}
    e, nb = engine_of(sensor, hyper_si)
    assert nb in (None, e.nb)
    nb = e.nb
    if sensor in ("cut1", "cut65", "hyper211", "model2162"):
        assert (M * (N // 64) * nb) % 4 != 0                             # (the tail workgroup of k_sobol_blocks)
    assert {"cut1": 1, "cut64": 64, "cut65": 65}.get(sensor, nb * F) == nb * F
    base, (uA, uB) = sites_of(M, seed=F + nb), design_of(N, F, seed=nb)
    ref, _ = check_sobol(torch_mod, e, base, FREE[F], uA, uB, column=column, band_model=band_model,
                         what=f"{sensor} nb {nb} F {F} N {N} M {M} column {column} band_model {band_model}")
    top = ref["ST"].max(axis=2)
    print(f"{sensor}: finite S1 {np.isfinite(ref['S1']).mean():.4f}, var > 0 {(ref['var'] > 0).mean():.4f}, bands whose largest ST > 0.1 "
          f"{(top > 0.1).mean():.4f}, the smallest largest ST {np.nanmin(top):.3e}, ST_se > 0 {(ref['ST_se'].max(axis=2) > 0).mean():.4f}")
    assert np.isfinite(ref["S1"]).all() and (ref["var"] > 0).all()                      # (not vacuous:
    assert (top > 0.1).all() and (ref["ST_se"].max(axis=2) > 0).all()                   # every band has a parameter that moves it)


# ---- (c) the options, and the forms Engine.sobol takes

OPTIONS = [("newton", None), ("literal", 1), ("literal", 30), ("newton", 30)]


@pytest.fixture(scope="module")
def plain(torch_mod, eng):
    """F = 3, N = 192, M = 3 on R_TOA under the default options -> (base, names, uA, uB, the raw call's outputs)"""
    base, (uA, uB) = sites_of(3), design_of(192, 3, seed=1)
    _, got = check_sobol(torch_mod, eng, base, FREE[3], uA, uB, column=1, what="options: the defaults, R_TOA")
    return base, FREE[3], uA, uB, got


@pytest.mark.parametrize("lidf,nlayers", OPTIONS)
def test_options_reach_the_forward_model(torch_mod, eng, plain, lidf, nlayers):
    import spart_amd
    base, names, uA, uB, default = plain
    raw = dict(fast_prelude=1 if lidf == "newton" else 0, nlayers=nlayers or 0)
    _, got = check_sobol(torch_mod, eng, base, names, uA, uB, column=1, what=f"options: lidf {lidf} nlayers {nlayers}", **raw)
    assert not same(got["S1"], default["S1"]) and not same(got["mean"], default["mean"]), (lidf, nlayers)
    if lidf == "newton" and nlayers == 30:
        free, (lo, hi) = cols_of(names), bounds_of(names)
        for only in (dict(nlayers=30), dict(fast_prelude=1)):
            rc, one = sobol_call(torch_mod, eng, base, free, lo, hi, uA, uB, column=1, **only)
            assert rc == 0 and not same(got["S1"], one["S1"]) and not same(got["mean"], one["mean"]), only
    res = eng.sobol(torch_mod.as_tensor(base.T.copy(), device=eng.device), names, design=(uA, uB), column="R_TOA", lidf=lidf, nlayers=nlayers)
    assert res["names"] == names and not differing({k: res[k].cpu().numpy() for k in OUTS}, got)
    host = spart_amd.sobol(base.T, S2, names, design=(uA, uB), column="R_TOA", lidf=lidf, nlayers=nlayers)
    assert host["names"] == names and not differing(host, got)


def test_the_forms_engine_sobol_takes(torch_mod, eng, plain):
    """designs as device tensors, as column-sliced views (numpy and device), in float32; bounds narrower than the default
    ranges; L_TOA: each is the raw call on what the form stands for, and the raw call is the definition"""
    base, names, uA, uB, default = plain
    free, (lo, hi) = cols_of(names), bounds_of(names)
    P = torch_mod.as_tensor(base.T.copy(), device=eng.device)
    run = lambda **kw: {k: v.cpu().numpy() for k, v in eng.sobol(P, names, **kw).items() if k != "names"}     # noqa: E731
    dev = lambda a: torch_mod.as_tensor(a, device=eng.device)     # noqa: E731
    assert not differing(run(design=(dev(uA), dev(uB)), column="R_TOA"), default)
    rng = np.random.default_rng(2)
    wideA, wideB = np.column_stack([rng.random(192), uA, rng.random(192)]), np.column_stack([rng.random(192), uB, rng.random(192)])
    assert not wideA[:, 1:4].flags["C_CONTIGUOUS"] and not dev(wideA)[:, 1:4].is_contiguous()
    assert not differing(run(design=(wideA[:, 1:4], wideB[:, 1:4]), column="R_TOA"), default)
    assert not differing(run(design=(dev(wideA)[:, 1:4], dev(wideB)[:, 1:4]), column="R_TOA"), default)
    # float32 designs are widened, not rounded again: the raw call on the widened values, which differ from uA, uB
    a32, b32 = uA.astype(np.float32), uB.astype(np.float32)
    rc, raw32 = sobol_call(torch_mod, eng, base, free, lo, hi, a32.astype(np.float64), b32.astype(np.float64), column=1)
    assert rc == 0 and not same(raw32["S1"], default["S1"])
    assert not differing(run(design=(a32, b32), column="R_TOA"), raw32)
    assert not differing(run(design=(dev(a32), dev(b32)), column="R_TOA"), raw32)
    # narrower bounds for two of the three names; the third keeps its range
    from spart_amd import workloads
    narrow = {"LAI": (1.0, 5.0), "Cw": (0.01, 0.03)}
    assert all(workloads.RANGES[n][0] < v[0] < v[1] < workloads.RANGES[n][1] for n, v in narrow.items())
    lo2, hi2 = (np.array([narrow.get(n, workloads.RANGES[n])[i] for n in names], dtype=np.float64) for i in (0, 1))
    want = sd.sobol_defined(base, free, lo2, hi2, uA, uB, forward_of(torch_mod, eng, 1))
    rc, raw = sobol_call(torch_mod, eng, base, free, lo2, hi2, uA, uB, column=1)
    print(f"spart_sobol narrower bounds: {sum(differing(raw, want).values())} differing words of {sum(v.size for v in want.values())}")
    assert rc == 0 and not differing(raw, want) and not same(raw["S1"], default["S1"])
    assert not differing(run(design=(uA, uB), column="R_TOA", bounds=narrow), raw)
    _, ltoa = check_sobol(torch_mod, eng, base, names, uA, uB, column=2, what="the forms: L_TOA")
    assert not differing(run(design=(uA, uB), column="L_TOA"), ltoa) and not same(ltoa["mean"], default["mean"])


# ---- (d) what IEEE gives

def test_a_band_that_does_not_vary(torch_mod, eng):
    """F = 1, the free parameter DOY, which R_TOC does not read: every a, b and d is exactly 0, so var == 0, mean == yA[0] and
    S1, ST and both standard errors are 0 / 0 = NaN in every band; nothing is clamped.  NaN matches NaN here whatever its
    sign: the sign of the NaN a 0 / 0 makes is not an IEEE result.  Measured (the test prints it): all 4 * 26 NaN words have
    the sign bit set on gfx950 and in numpy on x86-64 alike, so the two do agree in it today; nothing here relies on that."""
    M, N = 2, 128
    base, (uA, uB) = sites_of(M, seed=15), design_of(N, 1, seed=10)
    lo, hi = np.array([1.0]), np.array([365.0])
    fwd = forward_of(torch_mod, eng, 0)
    ref = sd.sobol_defined(base, [26], lo, hi, uA, uB, fwd)
    rc, got = sobol_call(torch_mod, eng, base, [26], lo, hi, uA, uB)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    counts = differing(got, ref)
    print(f"spart_sobol F 1 (DOY) N 128 M 2: {sum(counts.values())} differing words of {sum(v.size for v in ref.values())}")
    print("(NaN words, with the sign bit): the library's", {k: nan_signs(got[k]) for k in INDEX_KEYS}, "the definition's",
          {k: nan_signs(ref[k]) for k in INDEX_KEYS})
    assert not any(counts.values()), counts
    first = base.copy()
    first[:, 26] = sd.points_defined(uA[0], lo, hi)
    y0 = fwd(first)
    assert np.isfinite(y0).all() and (y0 > 0).all()
    for r in (got, ref):
        assert (r["var"] == 0).all() and not np.signbit(r["var"]).any() and same(r["mean"], y0)
        assert all(np.isnan(r[k]).all() and r[k].shape == (M, eng.nb, 1) for k in INDEX_KEYS)


def test_a_nan_site_among_finite_ones(torch_mod, eng):
    """M = 3, the angle in column 20 of site 1 is NaN: site 1 is NaN in all six outputs (measured: every NaN word with the sign
    bit set, in the library's outputs and the definition's), sites 0 and 2 have the bits of the call without it"""
    base, (uA, uB) = sites_of(3, seed=16), design_of(128, 3, seed=11)
    base[1, 20] = np.nan
    ref, got = check_sobol(torch_mod, eng, base, FREE[3], uA, uB, what="F 3 N 128 M 3, site 1 NaN", nan_sites=[1])
    assert np.isfinite(np.stack([ref[k][[0, 2]].ravel() for k in INDEX_KEYS])).all() and (ref["var"][[0, 2]] > 0).all()
    free, (lo, hi) = cols_of(FREE[3]), bounds_of(FREE[3])
    rc, rest = sobol_call(torch_mod, eng, base[[0, 2]], free, lo, hi, uA, uB)
    assert rc == 0 and all(same(rest[k], got[k][[0, 2]]) for k in OUTS)
