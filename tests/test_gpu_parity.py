"""Parity of the HIP path (through the C ABI, via spart_amd.Engine) with the oracle and with the
reference's golden vectors.  Tolerances: north_star's 1e-6 rel (fp64) / 1e-4 rel (fp32) on the
sensor columns; spectra use the same relative bound with an absolute floor matching the
reference's own unit-test precision (assert_almost_equal: 1.5e-7 leaf, 1.5e-6 canopy)."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

pytestmark = pytest.mark.gpu

TOL = {"float64": 1e-6, "float32": 1e-4}
# |a-b| <= TOL * max(|b|, FLOOR): the floor turns the bound into an absolute one for near-zero
# spectra (1e-7 in fp64 = the reference's own assert_almost_equal precision and its E1-quadrature
# noise; 1e-6 in fp32)
FLOOR = {"float64": 0.1, "float32": 1e-2}
# sensor columns R_TOC / R_TOA / L_TOA: SURVEY.md section 8(d)'s metric |x - ref| / max(|ref|, 1e-6), both dtypes
COLFLOOR = 1e-6


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def test_native_library_is_loaded(torch_mod):
    """the in-tree HIP library is what runs, and it was built from the sources next to it (a stale .so fails here)"""
    from spart_amd import _lib
    lib = _lib.load()
    assert lib is not None
    with open("/proc/self/maps") as f:
        assert "libspart_hip.so" in f.read()
    assert _lib.build_id(lib) == _lib.expected_build_id()
    assert len(_lib.build_id(lib)) == 12


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_prospect_golden(golden, dtype, torch_mod):
    from spart_amd import get_engine
    g = golden["prospect"]
    eng = get_engine(None, 0)
    refl, tran, kchl = eng.prospect(list(g["leaf"].T), dtype)
    tol, fl = TOL[dtype], FLOOR[dtype]
    assert rel_err(refl.cpu().numpy(), g["refl"], fl) < tol
    assert rel_err(tran.cpu().numpy(), g["tran"], fl) < tol
    assert rel_err(kchl.cpu().numpy(), g["kChlrel"], fl) < tol


def test_config2_lhs_workload_all_rows(golden, oracle, tables, torch_mod):
    """BASELINE config 2 AS STATED: workloads.lhs_params(10_000, "leaf") (7-D Latin hypercube, PROT = CBC = 0, SURVEY.md section
    8d) through spart_prospect_batch -- the call bench.py times as configs["2"].  float64: every one of the 3 x 10 000 x 2001
    outputs against the oracle (refl, tran <= 2e-9 absolute, kChlrel <= 1e-9 relative) and the first 32 rows against the REAL
    reference (config2.npz; 1.5e-7 = its own test precision, its QUADPACK E1 carries ~1e-8); float32 at 1e-4.
    Match: prospect_5d.py:117-246."""
    from spart_amd import get_engine, workloads
    leaf = workloads.lhs_params(10_000, "leaf")[:, :9]
    g = golden["config2"]
    assert np.array_equal(leaf[:32], g["leaf"])
    eng = get_engine(None, 0)
    ref = oracle.prospect_5d(leaf, tables)
    n0 = eng.calls["spart_prospect_batch"]
    out = eng.prospect(list(leaf.T), "float64")
    assert eng.calls["spart_prospect_batch"] == n0 + 1
    for got, want, name in zip(out, ref, ("refl", "tran", "kChlrel")):
        a = got.cpu().numpy()
        assert a.shape == (10_000, 2001) and np.isfinite(a).all()
        if name == "kChlrel":
            assert rel_err(a, want, 1e-12) < 1e-9, name
        else:
            assert np.max(np.abs(a - want)) < 2e-9, name
        assert np.max(np.abs(a[:32] - g[name])) < 1.5e-7, (name, "vs the reference")
    out32 = eng.prospect(list(leaf.T), "float32")
    for got, want, name in zip(out32, ref, ("refl", "tran", "kChlrel")):
        assert rel_err(got.double().cpu().numpy(), want, 1e-2) < 1e-4, name
    # any subset of the outputs gives the same numbers (the kernel skips the stores, nothing else)
    only = eng.prospect(list(leaf.T), "float64", outputs=("tran",))
    assert only[0] is None and only[2] is None and torch_mod.equal(only[1], out[1])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_bsm_golden(golden, dtype, torch_mod):
    from spart_amd import get_engine
    g = golden["bsm"]
    eng = get_engine(None, 0)
    refl, dry = eng.bsm(list(g["soil"].T), dtype)
    assert rel_err(refl.cpu().numpy(), g["refl"], FLOOR[dtype]) < TOL[dtype]
    assert rel_err(dry.cpu().numpy(), g["refl_dry"], FLOOR[dtype]) < TOL[dtype]


def test_lidf_golden(golden, torch_mod):
    from spart_amd import get_engine
    g = golden["sailh"]
    eng = get_engine(None, 0)
    lidf = eng.lidf(g["canopy"][:, 1], g["canopy"][:, 2]).cpu().numpy()
    assert np.max(np.abs(lidf - g["lidf"])) < 1e-12


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sailh_golden(golden, dtype, torch_mod):
    from spart_amd import get_engine
    g = golden["sailh"]
    eng = get_engine(None, 0)
    out = eng.sailh(g["leaf_refl"][None], g["leaf_tran"][None], g["soil_refl"][None], list(g["canopy"].T),
                    list(g["angles"].T), dtype)
    for o, k in zip(out, ("rso", "rdo", "rsd", "rdd")):
        assert rel_err(o.cpu().numpy(), g[k], FLOOR[dtype]) < TOL[dtype], k


def test_reference_test_grids_all_rows(golden, oracle, tables, torch_mod):
    """The reference's own unit-test grids IN FULL, refereed by the REFERENCE ITSELF (tests/golden/grids.npz: its
    PROSPECT_5D / SAILH run over every case; 16 probe bands + the all-band mean of each spectrum -- its parquet files with
    the expected values are missing from the snapshot and its tests draw 10 rows unless run with --all): the 6480-case
    PROSPECT grid (tests/unit/test_PROSPECT/build_PROSPECT_tests.py:38-50) and the 8100-case SAILH grid
    (tests/unit/test_SAILH/build_SAILH_tests.py:87-101, default leaf / soil fixtures, dso = 0 hot-spot cases and the
    non-physical |a| + |b| > 1 LIDFs included), HIP float64 through the C ABI with the reference tests' own precision:
    assert_almost_equal (7 decimals = 1.5e-7, test_PROSPECT.py:25-27) on the leaf spectra, assert_array_almost_equal
    (6 decimals = 1.5e-6, test_SAILH.py:33-36) on the canopy spectra -- and float32 at 1e-4 of max(|ref|, 1e-2)."""
    import itertools
    from spart_amd import get_engine
    eng = get_engine(None, 0)
    gg = golden["grids"]
    grid = np.array(list(itertools.product(range(10, 90, 10), (0.005, 0.015), (0.02, 0.06, 0.10), (0.0, 0.5, 1.0), (10, 20, 30),
                                           (10, 20, 30), (1.0, 1.5, 2.0, 2.5, 3.0))), dtype=np.float64)
    assert grid.shape == (6480, 7) and np.allclose(grid, gg["leaf_grid"], rtol=0, atol=1e-12)     # the fixture IS that grid
    leaf = np.concatenate([gg["leaf_grid"], np.zeros((6480, 2))], axis=1)            # LeafBiology(*row): PROT = CBC = 0
    pi = gg["leaf_probe_index"]
    # EVERY band of every case against the oracle (which test_oracle_golden.py pins to the same reference rows): the probes
    # and means above cannot see an error confined to a few bands
    leaf_all = oracle.prospect_5d(leaf, tables)
    for dtype in ("float64", "float32"):
        out = eng.prospect(list(leaf.T), dtype)
        for j, (got, name) in enumerate(zip(out, ("refl", "tran", "kChlrel"))):
            a = got.double().cpu().numpy()
            if dtype == "float64":
                assert np.max(np.abs(a[:, pi] - gg["leaf_probes"][:, j])) < 1.5e-7, name
                assert np.max(np.abs(a.mean(axis=1) - gg["leaf_means"][:, j])) < 1.5e-7, name
                assert np.max(np.abs(a - leaf_all[j])) < 2e-9, (name, "all 2001 bands vs the oracle")
            else:
                assert rel_err(a[:, pi], gg["leaf_probes"][:, j], 1e-2) < 1e-4, name
                assert rel_err(a.mean(axis=1), gg["leaf_means"][:, j], 1e-2) < 1e-4, name
    # SAILH grid over the default leaf / soil fixtures (tests/conftest.py:48-112 of the reference = the golden file's spectra)
    g = golden["sailh"]
    can = np.array(list(itertools.product((1, 4, 7), (-1, -0.6, -0.2, 0.2, 0.6), (-1, -0.6, -0.2, 0.2, 0.6), (0.01, 0.06, 0.11, 0.16),
                                          (0, 30, 60), (0, 30, 60), (0, 80, 160))), dtype=np.float64)
    assert can.shape == (8100, 7) and np.allclose(can, gg["canopy_grid"], rtol=0, atol=1e-12)
    can = gg["canopy_grid"]
    ci = gg["canopy_probe_index"]
    with np.errstate(all="ignore"):
        can_all = oracle.sailh(g["leaf_refl"][None], g["leaf_tran"][None], g["soil_refl"][None], can[:, :4], can[:, 4:], pso="gl")
    for dtype in ("float64", "float32"):
        got = eng.sailh(g["leaf_refl"][None], g["leaf_tran"][None], g["soil_refl"][None], list(can[:, :4].T), list(can[:, 4:].T), dtype)
        for j, (o, k) in enumerate(zip(got, ("rso", "rdo", "rsd", "rdd"))):
            a = o.double().cpu().numpy()
            if dtype == "float64":
                assert rel_err(a, can_all[k], 1e-3) < 1e-7, (k, "all 2162 bands vs the oracle")
                assert np.max(np.abs(a[:, ci] - gg["canopy_probes"][:, j])) < 1.5e-6, k
                assert rel_err(a[:, ci], gg["canopy_probes"][:, j], 1e-3) < 1e-6, k        # (and the north-star tolerance)
                assert np.max(np.abs(a.mean(axis=1) - gg["canopy_means"][:, j])) < 1.5e-6, k
            else:
                assert rel_err(a[:, ci], gg["canopy_probes"][:, j], 1e-2) < 1e-4, k
                assert rel_err(a.mean(axis=1), gg["canopy_means"][:, j], 1e-2) < 1e-4, k


@pytest.mark.parametrize("sensor", ["Sentinel2A-MSI", "Sentinel2B-MSI", "TerraAqua-MODIS", "LANDSAT7-ETM",
                                    "LANDSAT8-OLI", "Sentinel3A-OLCI"])
def test_smac_golden(golden, sensor, torch_mod):
    from spart_amd import get_engine
    from spart_amd.engine import SMAC_FIELDS
    g = golden["smac"]
    eng = get_engine(sensor, 0)
    out = eng.smac(list(g[f"{sensor}/angles"].T), list(g[f"{sensor}/atm"].T))
    # the Sentinel-2 pickles hold float32 coefficients and the reference then computes partly in float32
    tol = 2e-6 if sensor.startswith("Sentinel2") else 1e-9
    for f in SMAC_FIELDS:
        assert rel_err(out[f].cpu().numpy(), g[f"{sensor}/{f}"], 1e-3) < tol, f


def test_bsm_and_smac_random_sweeps(oracle, tables, torch_mod):
    """The two stages the reference never tested on their own: BSM + soilwat on 4000 random soils
    (brightness / latitude / longitude / moisture, incl. SMp <= 5 = dry branch, SMC and film varied) and SMAC on 3000
    random geometries / atmospheres for each of the nine sensors (psi up to 360 deg for the cos(psi * 180/pi) quirk,
    zero gas columns), HIP float64 against the oracle at the north-star tolerance; BSM also in float32."""
    from spart_amd import get_engine, SENSORS
    from spart_amd.engine import SMAC_FIELDS
    rng = np.random.default_rng(2024)
    n = 4000
    soil = np.column_stack([rng.uniform(0.1, 1.0, n), rng.uniform(-40, 40, n), rng.uniform(60, 140, n), rng.uniform(0, 60, n),
                            rng.uniform(10, 50, n), rng.uniform(0.005, 0.03, n)])
    soil[:50, 3] = rng.uniform(0, 5, 50)                                  # mu <= 0: rwet = rdry (bsm.py:101-103)
    ref = oracle.bsm(soil, tables)
    eng = get_engine(None, 0)
    for dtype in ("float64", "float32"):
        out = eng.bsm(list(soil.T), dtype)
        for got, want, name in zip(out, ref, ("refl", "refl_dry")):
            assert rel_err(got.cpu().numpy(), want, FLOOR[dtype]) < TOL[dtype], (dtype, name)
    m = 3000
    ang = np.column_stack([rng.uniform(0, 75, m), rng.uniform(0, 60, m), rng.uniform(0, 360, m)])
    atm = np.column_stack([rng.uniform(0.0, 0.8, m), rng.uniform(0.0, 0.5, m), rng.uniform(0.0, 5.0, m), rng.uniform(600, 1050, m)])
    atm[:20, 1:3] = 0.0
    for sensor in SENSORS:
        want = oracle.smac(ang, atm, oracle.sensor_tables(tables, sensor))
        got = get_engine(sensor, 0).smac(list(ang.T), list(atm.T))
        for f in SMAC_FIELDS:
            assert rel_err(got[f].cpu().numpy(), want[f], 1e-3) < 1e-9, (sensor, f)


def _e2e_groups(golden):
    g = golden["e2e"]
    return sorted(set(k.rsplit("/", 1)[0] for k in g.files))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_full_chain_golden(golden, dtype, torch_mod):
    """Every committed full-chain row of the reference: 9 sensors x defaults, README/MODIS (NaN leaf
    bands), PRO/S2B, the config-4 and config-5 LHS slices."""
    from spart_amd import get_engine
    g = golden["e2e"]
    worst = {}
    for name in _e2e_groups(golden):
        sensor = name.split("/")[1]
        eng = get_engine(sensor, 0)
        P = torch_mod.as_tensor(g[name + "/P"].T.copy(), device="cuda:0")
        out = eng.run(P, dtype, materialize=("rsoil", "La"))
        for k in ("R_TOC", "R_TOA", "L_TOA", "rsoil", "La"):
            e = rel_err(out[k].cpu().numpy(), g[f"{name}/{k}"], COLFLOOR)
            worst[(name, k)] = e
            assert e < TOL[dtype], (name, k, e)
    print({k: f"{v:.1e}" for k, v in worst.items() if v > 0.1 * TOL[dtype]})


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_full_chain_vs_oracle_spectra(oracle, tables, dtype, torch_mod):
    """Materialised leaf / soil / canopy spectra of the fused kernel against the oracle (seeded LHS)."""
    from spart_amd import get_engine, workloads
    P = workloads.lhs_params(96, "full", seed=5)
    ref = oracle.spart_run(P, "Sentinel2A-MSI", tables, pso="gl", full=True)
    eng = get_engine("Sentinel2A-MSI", 0)
    fields = ("leaf_refl", "leaf_tran", "leaf_kchl", "soil_refl", "soil_refl_dry", "rso", "rdo", "rsd", "rdd")
    out = eng.run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), dtype, materialize=fields)
    rho, tau = oracle.pad_leaf(ref["leaf_refl"], ref["leaf_tran"])
    expect = dict(leaf_refl=rho, leaf_tran=tau, leaf_kchl=ref["kChlrel"], soil_refl=oracle.pad_soil(ref["soil_refl"]),
                  soil_refl_dry=ref["soil_refl_dry"], rso=ref["rso"], rdo=ref["rdo"], rsd=ref["rsd"], rdd=ref["rdd"])
    for k in fields:
        assert rel_err(out[k].cpu().numpy(), expect[k], FLOOR[dtype]) < TOL[dtype], k
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert rel_err(out[k].cpu().numpy(), ref[k], COLFLOOR) < TOL[dtype], k


def test_ragged_and_edge_batches(oracle, tables, torch_mod):
    """B = 1, B not a multiple of the chunk / workgroup size, B = 0."""
    from spart_amd import get_engine, workloads
    eng = get_engine("Sentinel2A-MSI", 0)
    for B in (1, 7, 65, 257):
        P = workloads.lhs_params(B, "full", seed=B)
        ref = oracle.spart_run(P, "Sentinel2A-MSI", tables, pso="gl")
        out = eng.run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), "float64")
        for k in ("R_TOC", "R_TOA", "L_TOA"):
            assert rel_err(out[k].cpu().numpy(), ref[k], COLFLOOR) < 1e-6
    out = eng.run(torch_mod.zeros((27, 0), dtype=torch_mod.float64, device="cuda:0"), "float32")
    assert out["R_TOC"].shape == (0, 13)


def test_maximum_batch_size(torch_mod):
    """The largest batch one call takes (60 000 000 spectra: the 32-bit lane offset of the constant staging,
    spart_capi.hip SPART_MAX_BATCH; ~100 GB of workspace, 13 GB of parameters, 9 GB of columns on the 288 GB card):
    every entry finite, and rows from the front, the middle and the far end of the batch equal -- bit for bit -- the
    same rows evaluated on their own (samples are independent; a wrapped offset anywhere would show here).  One more
    sample is refused with the library's message."""
    from spart_amd import get_engine, workloads
    torch = torch_mod
    eng = get_engine("Sentinel2A-MSI", 0)
    B = 60_000_000
    g = torch.Generator(device="cuda:0").manual_seed(5)
    P = torch.empty((27, B), dtype=torch.float64, device="cuda:0")
    d = workloads.default_row()[0]
    for j, name in enumerate(workloads.PARAM_NAMES):
        if name in workloads.RANGES and name not in ("PROT", "CBC"):
            lo, hi = workloads.RANGES[name]
            P[j].uniform_(lo, hi, generator=g)
        else:
            P[j].fill_(workloads.FIXED.get(name, d[j]))
    out = {k: torch.empty((B, 13), dtype=torch.float32, device="cuda:0") for k in ("R_TOC", "R_TOA", "L_TOA")}
    eng.run(P, "float32", out=dict(out))
    torch.cuda.synchronize()
    for k in out:
        assert bool(torch.isfinite(out[k]).all()), k
    for lo in (0, 7_325 * 4_000 - 100, B // 2 + 33, B - 777):       # incl. a chunk boundary of the band kernel and the tail
        sub = eng.run(P[:, lo:lo + 777].contiguous(), "float32")
        for k in out:
            assert torch.equal(sub[k], out[k][lo:lo + 777]), (k, lo)
    assert float(out["R_TOC"].double().mean()) > 0.01
    with pytest.raises(RuntimeError, match="at most 60000000 samples"):
        eng.run(torch.empty((27, B + 1), dtype=torch.float64, device="cuda:0"), "float32")
    del P, out, sub
    eng.release_workspace()
    torch.cuda.empty_cache()


def test_full_size_properties(torch_mod):
    """BASELINE size (1M spectra, config-4 workload): size-independent checks.
    (1) every fp32 column entry against the fp64 evaluation of the SAME 1M rows (fp64 itself is pinned to
        the oracle / reference by the tests above): max |d| / max(|ref|, 1e-6) < 1e-4 over all 13M entries
        (test_float32_tolerance_at_size below does the same for config 5 and for the legacy float32 columns);
    (2) evaluating the batch in two ragged halves gives bit-identical columns (samples are independent);
    (3) batch-mean spectra (all 2162 bands of all samples) agree between fp32 and fp64."""
    from spart_amd import get_engine, workloads
    eng = get_engine("Sentinel2A-MSI", 0)
    B = 1_000_000
    P = torch_mod.as_tensor(workloads.lhs_params(B, "full").T.copy(), device="cuda:0")
    o64 = {k: v.clone() for k, v in eng.run(P, "float64", materialize=("band_mean",)).items()}
    out = {k: v.clone() for k, v in eng.run(P, "float32", materialize=("band_mean",)).items()}
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert torch_mod.isfinite(out[k]).all()
        err = ((out[k].double() - o64[k]).abs() / o64[k].abs().clamp_min(COLFLOOR)).max().item()
        assert err < 1e-4, (k, err)
    bm_err = ((out["band_mean"].double() - o64["band_mean"]).abs() / o64["band_mean"].abs().clamp_min(1e-3)).max().item()
    assert bm_err < 1e-4, bm_err
    h = B // 2 + 13
    o1 = {k: v.clone() for k, v in eng.run(P[:, :h].contiguous(), "float32").items()}
    o2 = eng.run(P[:, h:].contiguous(), "float32")
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert torch_mod.equal(torch_mod.cat([o1[k], o2[k]]), out[k])


@pytest.mark.parametrize("kind,sensor", [("full", "Sentinel2A-MSI"), ("pro", "Sentinel2B-MSI")])
def test_float32_tolerance_at_size(kind, sensor, torch_mod):
    """BASELINE configs 4 (22-D LHS, Sentinel-2A) and 5 (PROSPECT-PRO, Cdm = 0, Sentinel-2B) at B = 1M, float32 mode
    against the float64 mode of the same rows, on SURVEY.md section 8(d)'s metric |x - ref| / max(|ref|, 1e-6):

    * default float32 mode (sensor-slot bands re-evaluated in float64, spart_materialize.f32_columns = 0): EVERY one of
      the 3 x 13M entries is within 1e-4 -- in fact within float32 rounding (1e-7) of the float64 value, physical or not;
    * legacy float32 columns (f32_columns = 1): counted, not hidden -- the entries over 1e-4 are reported by number
      (entries and samples) and bounded: they are the nearly conservative leaves on which the reference's own canopy
      formulas cancel (sailh.py:185-214), which is why that mode is an opt-in."""
    from spart_amd import get_engine, workloads
    eng = get_engine(sensor, 0)
    B = 1_000_000
    P = torch_mod.as_tensor(workloads.lhs_params(B, kind).T.copy(), device="cuda:0")
    o64 = {k: v.clone() for k, v in eng.run(P, "float64").items()}
    o32 = {k: v.clone() for k, v in eng.run(P, "float32").items()}
    leg = eng.run(P, "float32", f32_columns=True)
    report = {}
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        ref = o64[k]
        assert torch_mod.isfinite(ref).all() and torch_mod.isfinite(o32[k]).all()
        den = ref.abs().clamp_min(COLFLOOR)
        err = ((o32[k].double() - ref).abs() / den).max().item()
        assert err < 1e-4, (kind, k, err)
        assert err < 2e-7, (kind, k, err)                  # one float32 rounding of the float64 value
        el = (leg[k].double() - ref).abs() / den
        bad = el > 1e-4
        nbad, nrow = int(bad.sum().item()), int(bad.any(dim=1).sum().item())
        report[k] = (err, float(el.max().item()), nbad, nrow)
        assert nbad < 1000 and nrow < 500, (kind, k, nbad, nrow)     # of 13M entries / 1M samples (measured: 175 in 174 samples)
    print(kind, {k: f"default max {v[0]:.1e} | f32_columns max {v[1]:.1e}, {v[2]} entries in {v[3]} samples > 1e-4"
                 for k, v in report.items()})


def test_float32_columns_are_the_float64_columns_rounded(golden, torch_mod):
    """The default float32 mode takes its sensor columns from a float64 evaluation of the sensor-slot bands over the
    float64 prelude (k_columns<double, float>): on every sensor (integer and fractional band centres), with debug rsoil
    and with user dry-soil spectra, they equal the float64 mode's columns converted to float32."""
    from spart_amd import get_engine, workloads
    for sensor, kind in (("Sentinel2A-MSI", "full"), ("Sentinel2B-MSI", "pro"), ("TerraAqua-MODIS", "full"),
                         ("LANDSAT7-ETM", "pro"), ("Sentinel3A-OLCI", "full")):
        eng = get_engine(sensor, 0)
        P = torch_mod.as_tensor(workloads.lhs_params(3001, kind, seed=77).T.copy(), device="cuda:0")
        o64 = {k: v.clone() for k, v in eng.run(P, "float64", materialize=("rsoil", "La")).items()}
        for kw in (dict(), dict(prune=True), dict(materialize=("rso", "leaf_refl"))):
            mat = tuple(kw.pop("materialize", ())) + ("rsoil", "La")
            o32 = eng.run(P, "float32", materialize=mat, **kw)
            for k in ("R_TOC", "R_TOA", "L_TOA", "rsoil", "La"):
                d = (o32[k].double() - o64[k]).abs() / o64[k].abs().clamp_min(1e-30)
                assert float(d.max()) < 1.2e-7, (sensor, kw, k, float(d.max()))
    eng = get_engine("Sentinel2A-MSI", 0)
    g = golden["rdry"]
    P = workloads.lhs_params(3, "full", seed=1)
    cols = [P[:, j] for j in range(27)]
    cols[9] = cols[10] = cols[11] = None
    a = eng.run(cols, "float64", rdry=g["spectra"])
    b = eng.run(cols, "float32", rdry=g["spectra"].astype(np.float32))
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert float(((b[k].double() - a[k]).abs() / a[k].abs()).max()) < 1e-6, k     # (the spectra themselves were rounded)


def test_float64_columns_over_float32_bands(golden, torch_mod):
    """spart_materialize.f32_bands: float64 columns bit-identical to the float64 mode's (same prelude, same column kernel),
    with the all-band evaluation in float32; against the reference's golden rows; invalid combinations are refused."""
    from spart_amd import get_engine
    g = golden["e2e"]
    for name in ("lhs_full/Sentinel2A-MSI", "lhs_pro/Sentinel2B-MSI", "lhs_small/TerraAqua-MODIS"):
        eng = get_engine(name.split("/")[1], 0)
        P = torch_mod.as_tensor(g[name + "/P"].T.copy(), device="cuda:0")
        a = {k: v.clone() for k, v in eng.run(P, "float64", materialize=("rsoil", "La")).items()}
        b = eng.run(P, "float64", f32_bands=True, materialize=("rsoil", "La"))
        for k in ("R_TOC", "R_TOA", "L_TOA", "rsoil", "La"):
            assert b[k].dtype == torch_mod.float64 and torch_mod.equal(a[k], b[k]), (name, k)
            assert rel_err(b[k].cpu().numpy(), g[f"{name}/{k}"], COLFLOOR) < 1e-6, (name, k)
    with pytest.raises(RuntimeError, match="f32_bands"):
        eng.run(P, "float64", f32_bands=True, materialize=("rso",))


def test_reference_style_api(golden, torch_mod, capsys):
    """import SPART; SPART.SPART(...).run() -> the reference's DataFrame (README quickstart pins)."""
    import SPART
    leafbio = SPART.LeafBiology(40, 10, 0.02, 0.01, 0, 10, 1.5)
    soilpar = SPART.SoilParameters(0.5, 0, 100, 15, 25, 0.015)
    canopy = SPART.CanopyStructure(3, -0.35, -0.15, 0.05)
    angles = SPART.Angles(40, 0, 0)
    atm = SPART.AtmosphericProperties(0.3246, 0.3480, 1.4116, 1013.25)
    df = SPART.SPART(soilpar, leafbio, canopy, atm, angles, "TerraAqua-MODIS", 100).run(debug=True)
    assert list(df.columns) == ["Band", "L_TOA", "R_TOA", "R_TOC", "rsoil"]
    assert abs(df["R_TOC"].iloc[0] / 0.02087402205273674 - 1) < 1e-6
    assert abs(df["R_TOA"].iloc[0] / 0.0497552219811317 - 1) < 1e-6
    assert abs(df["L_TOA"].iloc[0] / 0.022812529362725764 - 1) < 1e-6
    g = golden["e2e"]
    assert rel_err(df["R_TOA"].to_numpy(), g["readme/TerraAqua-MODIS/R_TOA"][0], COLFLOOR) < 1e-6
    # PROSPECT-PRO warning text goes to stdout once (prospect_5d.py:148-155)
    pro = SPART.LeafBiology(40, 0.01, 0.02, 0, 10, 10, 1.5, PROT=0.001, CBC=0.009)
    df2 = SPART.SPART(SPART.SoilParameters(0.5, 0, 100, 20, 25, 0.015), pro, canopy,
                      SPART.AtmosphericProperties(0.325, 0.35, 1.41), angles, "Sentinel2B-MSI", 100).run()
    assert "PROSPECT-PRO was called" in capsys.readouterr().out
    # atmopt (SPART.py:66-81, 226-232; smac.py:209-211) belongs to every run(): golden SMAC row 0 = these defaults
    gs = golden["smac"]
    sp = SPART.SPART(SPART.SoilParameters(0.5, 0, 100, 20, 25, 0.015), SPART.LeafBiology(40, 0.01, 0.02, 0, 10, 10, 1.5), canopy,
                     SPART.AtmosphericProperties(0.325, 0.35, 1.41), angles, "Sentinel2A-MSI", 100)
    from spart_amd import get_engine
    eng = get_engine("Sentinel2A-MSI", None)
    assert not hasattr(sp, "atmopt") and not hasattr(sp, "canopyopt")              # set by run() only (SPART.py:197-229)
    before = dict(eng.calls)
    sp.run()
    # ONE library call per run(); the reference object's atmopt / leafopt / soilopt / canopyopt are evaluated on first access
    assert eng.calls["spart_run_batch"] == before.get("spart_run_batch", 0) + 1
    assert eng.calls["spart_smac_batch"] == before.get("spart_smac_batch", 0)
    assert sp.canopyopt.rso.shape == (2162, 1) and sp.leafopt.refl.shape == (2162, 1) and sp.leafopt.kChlrel.shape == (2001, 1)
    assert sp.soilopt.refl.shape == (2162, 1) and sp.soilopt.refl_dry.shape == (2001, 1)
    assert eng.calls["spart_run_batch"] == before.get("spart_run_batch", 0) + 2         # one materialising call for all three
    assert abs(sp.canopyopt.rso[400, 0] - 0.40396347479496547) < 1e-6 and abs(sp.canopyopt.rdd[2100, 0] - 0.005657296144770152) < 1e-6
    assert abs(sp.leafopt.refl[150, 0] - 0.06375474885800862) < 1e-7 and abs(sp.soilopt.refl[400, 0] - 0.3978653598241099) < 1e-7
    assert abs(sp.R_TOC[0, 5] / 0.3371841542003048 - 1) < 1e-6
    eager = SPART.SPART(sp.soilpar, sp.leafbio, canopy, sp.atm, angles, "Sentinel2A-MSI", 100)
    eager.run(materialize=True)
    assert np.array_equal(eager.canopyopt.rso, sp.canopyopt.rso) and np.array_equal(eager.R_TOA, sp.R_TOA)
    # a batched run: still one call, BatchResult out, lazy (B, 2162) spectra
    many = SPART.SPART(SPART.SoilParameters(0.5, 0, 100, np.array([20.0, 30.0, 4.0]), 25, 0.015), sp.leafbio, canopy, sp.atm, angles,
                       "Sentinel2A-MSI", 100)
    n0 = eng.calls["spart_run_batch"]
    res = many.run()
    assert eng.calls["spart_run_batch"] == n0 + 1 and res["R_TOC"].shape == (3, 13) and many.canopyopt.rdd.shape == (3, 2162)
    assert np.array_equal(res["R_TOC"][0], sp.R_TOC[0])
    assert np.array_equal(gs["Sentinel2A-MSI/angles"][0], [40, 0, 0]) and np.allclose(gs["Sentinel2A-MSI/atm"][0], [0.325, 0.35, 1.41, 1013.25])
    for f in ("Ta_s", "Ta_o", "Tg", "Ra_dd", "Ra_so", "Ta_ss", "Ta_sd", "Ta_oo", "Ta_do"):
        a = getattr(sp.atmopt, f)
        assert a.shape == (1, 13)
        assert rel_err(a[0], gs[f"Sentinel2A-MSI/{f}"][0], 1e-3) < 2e-6, f
    # the reference's calling convention SMAC(angles, atm, sensorinfo["SMAC_coef"]) with a fresh dict per call: two
    # sensors back to back must not share an engine (the dicts may share an id())
    for sensor in ("Sentinel2A-MSI", "TerraAqua-MODIS", "LANDSAT8-OLI"):
        ao = SPART.SMAC(SPART.Angles(*gs[f"{sensor}/angles"][2]), SPART.AtmosphericProperties(*gs[f"{sensor}/atm"][2]),
                        SPART.load_sensor_info(sensor)["SMAC_coef"])
        tol = 2e-6 if sensor.startswith("Sentinel2") else 1e-9
        for f in ("Tg", "Ra_so", "Ta_ss", "Ta_do"):
            assert rel_err(getattr(ao, f)[0], gs[f"{sensor}/{f}"][2], 1e-3) < tol, (sensor, f)
    assert abs(df2["R_TOC"].iloc[0] / 0.016457380856374198 - 1) < 1e-6
    assert abs(df2["R_TOA"].iloc[5] / 0.3058118531440649 - 1) < 1e-6
    # stage functions with reference shapes
    lo = SPART.PROSPECT_5D(SPART.LeafBiology(40, 0.01, 0.02, 0, 10, 10, 1.5), SPART.load_optical_parameters())
    assert lo.refl.shape == (2001, 1)
    assert abs(lo.refl[150, 0] - 0.06375474885800862) < 1e-7 and abs(lo.tran[400, 0] - 0.4700377848758272) < 1e-7
    with pytest.raises(RuntimeError, match="must be of len 2162"):
        SPART.SAILH(SPART.BSM(soilpar), lo, canopy, angles)
    lo = SPART.set_leaf_refl_trans_assumptions(lo, leafbio, SPART.SpectralBands())
    so = SPART.set_soil_refl_trans_assumptions(SPART.BSM(SPART.SoilParameters(0.5, 0, 100, 20, 25, 0.015)),
                                               SPART.SpectralBands())
    rad = SPART.SAILH(so, lo, canopy, angles)
    assert rad.rso.shape == (2162, 1)
    assert abs(rad.rso[400, 0] - 0.40396347479496547) < 1e-6 and abs(rad.rdd[2100, 0] - 0.005657296144770152) < 1e-6
    assert abs(canopy.lidf[0, 0] - 0.037891833294514) < 1e-12


def test_soil_parameters_from_a_jpl_file_through_the_chain(golden):
    """SPART.SPART(SoilParametersFromFile(<path>), ...).run(debug=True) (bsm.py:155-226, 42-43; SPART.py:192-199) against
    the reference's run on the same synthetic JPL-layout file (tests/golden/jpl/, make_golden.py jpl)."""
    import SPART
    g = golden["jpl"]
    d = np.load(os.path.join(ROOT, "tests", "golden", "e2e.npz"))["defaults/Sentinel2A-MSI/P"][0]
    soil = SPART.SoilParametersFromFile(os.path.join(ROOT, "tests", "golden", "jpl", "descending_percent.txt"), 20, 25, 0.015)
    df = SPART.SPART(soil, SPART.LeafBiology(*d[0:7]), SPART.CanopyStructure(*d[15:19]),
                     SPART.AtmosphericProperties(d[22], d[23], d[24], Pa=d[25]), SPART.Angles(*d[19:22]), "Sentinel2A-MSI", 100).run(debug=True)
    for c in ("R_TOC", "R_TOA", "L_TOA", "rsoil"):
        assert rel_err(df[c].to_numpy(), g["run/" + c], COLFLOOR) < 1e-6, c
    so = SPART.BSM(soil)
    assert so.refl_dry.shape == (2001, 1) and np.array_equal(so.refl_dry, g["descending_percent"])


def test_reference_example_and_benchmark_harness(golden):
    """The reference's example script (example/example.py:7-31: every constructor by KEYWORD, SMC / film defaulted) and
    its benchmark fixtures (tests/benchmarks/test_benchmarks.py:27-55: spectra padded by hand through
    SpectralBands().IwlP / IwlT, imported from SPART.SPART) run unchanged against this package."""
    import warnings
    import SPART
    from SPART.SPART import SpectralBands
    from SPART.bsm import BSM, SoilParameters
    from SPART.prospect_5d import PROSPECT_5D, LeafBiology
    from SPART.sailh import SAILH, Angles, CanopyStructure
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        soilpar = SPART.SoilParameters(B=0.5, lat=0, lon=100, SMp=20)
    assert len(w) == 2                                              # bsm.py:274-286: SMC, film
    leafbio = SPART.LeafBiology(Cab=40, Cca=10, Cw=0.02, Cdm=0.01, Cs=0, Cant=10, N=1.5)
    canopy = SPART.CanopyStructure(LAI=3, LIDFa=-0.35, LIDFb=-0.15, q=0.05)
    angles = SPART.Angles(sol_angle=40, obs_angle=0, rel_angle=0)
    atm = SPART.AtmosphericProperties(aot550=0.325, uo3=0.35, uh2o=1.41, Pa=1013.25)
    df = SPART.SPART(soilpar, leafbio, canopy, atm, angles, sensor="Sentinel2A-MSI", DOY=100).run()
    g = golden["e2e"]
    for c in ("R_TOC", "R_TOA", "L_TOA"):
        assert rel_err(df[c].to_numpy(), g[f"defaults/Sentinel2A-MSI/{c}"][0], COLFLOOR) < 1e-6, c
    assert (df[["R_TOC", "R_TOA", "L_TOA"]].to_numpy() > 0).all()    # tests/e2e/test_SPART.py:40-42
    # benchmark fixtures
    op, sb = SPART.load_optical_parameters(), SpectralBands()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        soilopt = BSM(SoilParameters(0.5, 0, 100, 20), op)
    rs = np.zeros((sb.nwlP + sb.nwlT, 1))
    rs[sb.IwlP] = soilopt.refl
    rs[sb.IwlT] = 1 * rs[sb.nwlP - 1]
    soilopt.refl = rs
    lb = LeafBiology(40, 0.01, 0.02, 0, 10, 10, 1.5)
    leafopt = PROSPECT_5D(lb, op)
    rho, tau = np.zeros((sb.nwlP + sb.nwlT, 1)), np.zeros((sb.nwlP + sb.nwlT, 1))
    rho[sb.IwlT], tau[sb.IwlT] = lb.rho_thermal, lb.tau_thermal
    rho[sb.IwlP], tau[sb.IwlP] = leafopt.refl, leafopt.tran
    leafopt.refl, leafopt.tran = rho, tau
    rad = SAILH(soilopt, leafopt, CanopyStructure(3, -0.35, -0.15, 0.05), Angles(40, 0, 0))
    assert rad.rso.shape == (2162, 1)
    assert abs(rad.rso[400, 0] - 0.40396347479496547) < 1e-6 and abs(rad.rdo[2100, 0] - 0.006083228593590332) < 1e-6


def test_example_scripts_run(tmp_path):
    """examples/example.py (quick start, scalar then batched) and examples/lut.py (LUT to disk + inversion) as a user
    runs them: own processes, exit code 0, the expected last lines."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "example.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "R_TOC" in r.stdout and "BatchResult (100000, 13)" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "lut.py"), "20000", str(tmp_path / "lut")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "20000 rows" in r.stdout and "recovered the generating row" in r.stdout


def test_soilwat_entry_point(oracle, tables, golden):
    """SPART.bsm.soilwat(rdry, nw, kw, SMp, SMC, deleff) (bsm.py:62-128) with the context's water tables: against the
    oracle's BSM on the same dry spectrum (wet branch and the mu <= 0 branch), a foreign table, and a malformed one."""
    import SPART
    from SPART.bsm import soilwat
    op = SPART.load_optical_parameters()
    rdry = golden["rdry"]["spectra"][0][:, None]
    for smp in (30.0, 4.0):
        so = soilwat(rdry, op["nw"], op["Kw"], smp, 25, 0.015)
        assert isinstance(so, SPART.bsm.SoilOptics) and so.refl_dry is rdry                 # SoilOptics(rwet, rdry), bsm.py:126-128
        a = so.refl
        b, _ = oracle.bsm(np.array([[0.5, 0, 100, smp, 25, 0.015]]), tables, rdry=rdry[:, 0][None, :])
        assert a.shape == (2001, 1) and rel_err(a[:, 0], b[0], 1e-6) < 1e-9, smp
    assert np.array_equal(soilwat(rdry, op["nw"], op["Kw"], 4.0, 25, 0.015).refl, rdry)    # bsm.py:101-103
    # a foreign water table is HONOURED (round 5; it was refused before): the oracle with the same table agrees
    t2 = dict(tables)
    t2["nw"] = tables["nw"] * 1.01
    a = soilwat(rdry, op["nw"] * 1.01, op["Kw"], 30.0, 25, 0.015).refl
    b, _ = oracle.bsm(np.array([[0.5, 0, 100, 30.0, 25, 0.015]]), t2, rdry=rdry[:, 0][None, :])
    b0, _ = oracle.bsm(np.array([[0.5, 0, 100, 30.0, 25, 0.015]]), tables, rdry=rdry[:, 0][None, :])
    assert rel_err(a[:, 0], b[0], 1e-6) < 1e-9 and rel_err(a[:, 0], b0[0], 1e-6) > 1e-4
    with pytest.raises(ValueError, match="nw"):
        soilwat(rdry, op["nw"][:-1], op["Kw"], 30.0, 25, 0.015)
    from spart_amd import get_engine                   # with rdry only B / lat / lon may be None (they were all read as 0)
    with pytest.raises(ValueError, match="params\\[12\\]"):
        get_engine(None, 0).bsm([None] * 6, "float64", rdry=rdry)


def test_all_bands_are_evaluated_and_prune_is_equivalent(oracle, tables, torch_mod):
    """Default mode: every band of every sample feeds the per-chunk band sums -> batch-mean canopy spectra
    must equal the oracle's means over all 2162 bands.  prune=True must give bit-identical columns."""
    from spart_amd import get_engine, workloads
    B = 300
    P = workloads.lhs_params(B, "full", seed=21)
    ref = oracle.spart_run(P, "Sentinel2A-MSI", tables, pso="gl", full=True)
    eng = get_engine("Sentinel2A-MSI", 0)
    Pd = torch_mod.as_tensor(P.T.copy(), device="cuda:0")
    for dtype in ("float64", "float32"):
        out = eng.run(Pd, dtype, materialize=("band_mean",))
        bm = out["band_mean"].cpu().numpy()
        for q, k in enumerate(("rso", "rdo", "rsd", "rdd")):
            assert rel_err(bm[q], ref[k].mean(axis=0), 1e-3) < (1e-9 if dtype == "float64" else 2e-5), (dtype, k)
        cols = {k: out[k].clone() for k in ("R_TOC", "R_TOA", "L_TOA")}
        pr = eng.run(Pd, dtype, prune=True)
        for k in cols:
            assert torch_mod.equal(cols[k], pr[k]), (dtype, k)


def test_lidf_full_reference_grid(oracle, torch_mod):
    """All 25 (LIDFa, LIDFb) pairs of the reference's SAILH test grid (build_SAILH_tests.py:89-90), which
    includes non-physical |a| + |b| > 1, plus the |a| > 1 branch (sailh.py:371-372)."""
    from spart_amd import get_engine
    a, b = np.meshgrid(np.arange(-1, 1, 0.4), np.arange(-1, 1, 0.4), indexing="ij")
    a = np.concatenate([a.ravel(), [1.5, 0.0, -0.35]])
    b = np.concatenate([b.ravel(), [0.0, 0.0, -0.15]])
    ref = oracle.calculate_leafangles(a, b)
    got = get_engine(None, 0).lidf(a, b).cpu().numpy()
    assert np.max(np.abs(got - ref)) < 1e-12
    assert abs(got[-1, 0] - 0.037891833294514) < 1e-12        # SURVEY.md §8a pin


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_hot_spot_and_geometry_edges(oracle, tables, dtype, torch_mod):
    """hot spot exactly (dso == 0, nadir and off-nadir), tiny and large q, tiny and large LAI, psi folding
    (270, 365 deg), grazing sun, SMp below the 5 % threshold, N = 1 (single plate), PRO leaves."""
    from spart_amd import get_engine
    from helpers.domain_grid import EDGE_ROWS
    P = np.concatenate(EDGE_ROWS)
    ref = oracle.spart_run(P, "Sentinel2A-MSI", tables, pso="quad", full=True)
    eng = get_engine("Sentinel2A-MSI", 0)
    out = eng.run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), dtype, materialize=("rso", "rdd", "leaf_refl", "soil_refl"))
    tol, fl = TOL[dtype], FLOOR[dtype]
    rho, _ = oracle.pad_leaf(ref["leaf_refl"], ref["leaf_tran"])
    # row 16 (Cdm = 0, PROT = 0.001, CBC = 0) is a nearly non-absorbing leaf at 780-870 nm: the reference's SAIL
    # formula is ill-conditioned there and float32 rso is only good to 1e-3 at those bands;
    # its sensor columns still meet 1e-4 (checked below for every row)
    keep = np.ones(P.shape[0], dtype=bool)
    if dtype == "float32":
        keep[16] = False
    for k, e in (("rso", ref["rso"]), ("rdd", ref["rdd"]), ("leaf_refl", rho), ("soil_refl", oracle.pad_soil(ref["soil_refl"]))):
        assert rel_err(out[k].cpu().numpy()[keep], e[keep], fl) < tol, k
        assert rel_err(out[k].cpu().numpy(), e, fl) < 10 * tol, k
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert rel_err(out[k].cpu().numpy(), ref[k], COLFLOOR) < tol, k


def test_nan_and_nonphysical_inputs_do_not_crash(torch_mod):
    """NaN / negative / zero parameters propagate as NaN or inf like in the reference (no clamping, no fault)."""
    from spart_amd import get_engine, workloads
    D = workloads.default_row
    rows = [D(Cab=float("nan")), D(LAI=0.0), D(q=0.0), D(N=0.0), D(tts=90.0), D(SMC=0.0), D(LAI=-1.0), D(Cw=-0.01),
            D(tto=float("nan")), D(Pa=0.0), D(LIDFa=5.0, LIDFb=5.0), D()]
    P = torch_mod.as_tensor(np.concatenate(rows).T.copy(), device="cuda:0")
    eng = get_engine("Sentinel2A-MSI", 0)
    for dtype in ("float64", "float32"):
        out = eng.run(P, dtype)
        torch_mod.cuda.synchronize()
        assert torch_mod.isfinite(out["R_TOC"][-1]).all()          # the clean row is unaffected by its neighbours
        assert not torch_mod.isfinite(out["R_TOC"][0]).all()       # NaN in -> NaN out


def test_nonphysical_rows_nan_parity_float64(oracle, tables, torch_mod):
    """NaN semantics of the float64 band arithmetic: its table-driven exp / log and Newton-step 1/x, sqrt do
    not propagate a NaN ARGUMENT by themselves in every case, so the behaviour is asserted where it matters -- on outputs.
    (a) Full chain: a NaN or singular sample-level input (angle, LAI, soil brightness = NaN; SMC = 0; N = 0) makes every
        column entry NaN in the oracle (= the reference's numpy semantics) and must do so here; rows that stay finite in
        the oracle (LAI = 0 / 1e-9, q = 0, tts = 90, Pa = 0, N = 0.5 / 0.9) stay finite here and agree to the float64 contract
        (a negative LAI stays finite on both sides but only agrees to 6e-5: test_nan_and_nonphysical_inputs_do_not_crash);
        with negative concentrations or a NaN pigment the reference's leaf model turns K <= 0 / NaN bands into NaN or a
        finite value depending on rounding noise (prospect_5d.py:182-235: tau = 1, then 0/0 unless r + t >= 1 happens to
        hold) -- this build returns the finite zero-absorption limit resp. NaN there, so on those
        rows only the entries finite on both sides (and of reflectance size in the reference) are compared.
    (b) SAILH on user spectra with rho + tau > 1 in some bands: m = sqrt(absb (1 + 2 Mn)) (sailh.py:149) is the square
        root of a negative number there -- NaN in numpy, and NaN here (the float64 sqrt used to return finite garbage)."""
    from spart_amd import get_engine, workloads
    D = workloads.default_row
    nan = float("nan")
    all_nan = [D(tto=nan), D(psi=nan), D(tts=nan), D(LAI=nan), D(B=nan), D(SMC=0.0), D(N=0.0)]
    finite = [D(LAI=0.0), D(q=0.0), D(tts=90.0), D(Pa=0.0), D(), D(N=0.5), D(N=0.9), D(LAI=1e-9)]
    mixed = [D(Cab=nan), D(Cw=-0.01), D(Cw=-0.05), D(Cdm=-0.02), D(Cs=-1.0)]
    P = np.concatenate(all_nan + finite + mixed)
    na, nf = len(all_nan), len(finite)
    with np.errstate(all="ignore"):
        ref = oracle.spart_run(P, "Sentinel2A-MSI", tables, pso="gl")
    out = get_engine("Sentinel2A-MSI", 0).run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), "float64")
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        got, want = out[k].cpu().numpy(), ref[k]
        assert np.isnan(want[:na]).all() and not np.isfinite(got[:na]).any(), k
        assert np.isfinite(want[na:na + nf]).all() and np.isfinite(got[na:na + nf]).all(), k
        assert rel_err(got[na:na + nf], want[na:na + nf], COLFLOOR) < 1e-6, k
        both = np.isfinite(got[na + nf:]) & np.isfinite(want[na + nf:]) & (np.abs(want[na + nf:]) < 2.0)   # (not the reference's 1e6-sized noise)
        assert both.sum() > 30
        assert np.max(np.abs(got[na + nf:][both] - want[na + nf:][both]) / np.maximum(np.abs(want[na + nf:][both]), COLFLOOR)) < 1e-6, k
    # (b)
    g = np.load(os.path.join(ROOT, "tests", "golden", "sailh.npz"))
    rho, tau, rs = g["leaf_refl"].copy(), g["leaf_tran"].copy(), g["soil_refl"]
    bad = np.arange(300, 2162, 7)
    tau[bad] = 1.02 - rho[bad]                        # rho + tau = 1.02: negative absorptance
    can, ang = np.array([[3, -0.35, -0.15, 0.05], [1, 0.2, 0.1, 0.1]]), np.array([[40, 0, 0], [30, 20, 100]], dtype=np.float64)
    with np.errstate(all="ignore"):
        want = oracle.sailh(rho[None], tau[None], rs[None], can, ang, pso="gl")
    eng = get_engine(None, 0)
    got = eng.sailh(rho[None], tau[None], rs[None], list(can.T), list(ang.T), "float64")
    for o, k in zip(got, ("rso", "rdo", "rsd", "rdd")):
        a = o.cpu().numpy()
        assert np.isnan(want[k][:, bad]).all() and np.isnan(a[:, bad]).all(), k
        assert np.array_equal(np.isfinite(a), np.isfinite(want[k])), k
        assert rel_err(a, want[k], 1e-3) < 1e-7, k


def test_hip_graph_capture(torch_mod):
    """spart_run_batch allocates nothing and never synchronises: it can be captured into a HIP graph and replayed."""
    from spart_amd import get_engine, workloads
    eng = get_engine("Sentinel2A-MSI", 0)
    B = 4096
    P = torch_mod.as_tensor(workloads.lhs_params(B, "full", seed=4).T.copy(), device="cuda:0")
    out = {k: torch_mod.empty((B, 13), dtype=torch_mod.float32, device="cuda:0") for k in ("R_TOC", "R_TOA", "L_TOA")}
    eng.run(P, "float32", out=out)                 # warm-up: workspace allocation happens here, outside the capture
    ref = {k: v.clone() for k, v in out.items()}
    s = torch_mod.cuda.Stream()
    with torch_mod.cuda.stream(s):
        eng.run(P, "float32", out=out)
        g = torch_mod.cuda.CUDAGraph()
        with torch_mod.cuda.graph(g, stream=s):
            eng.run(P, "float32", out=out)
    for v in out.values():
        v.zero_()
    g.replay()
    torch_mod.cuda.synchronize()
    for k in ref:
        assert torch_mod.equal(out[k], ref[k])


def test_engine_capture_and_output_validation(torch_mod):
    """Engine.capture: one run() recorded into a HIP graph over resident buffers (default float32 mode, i.e. including
    the fork / join onto the context's side stream), replayed after other calls have used the engine in between; and
    the checks on caller-supplied outputs (the kernels only ever see their data_ptr())."""
    from spart_amd import get_engine, workloads
    eng = get_engine("Sentinel2A-MSI", 0)
    B = 20_001
    P = torch_mod.as_tensor(workloads.lhs_params(B, "full", seed=6).T.copy(), device="cuda:0")
    ref = {k: v.clone() for k, v in eng.run(P, "float32").items()}
    out = {k: torch_mod.zeros((B, 13), dtype=torch_mod.float32, device="cuda:0") for k in ("R_TOC", "R_TOA", "L_TOA")}
    replay = eng.capture(P, "float32", out=out)
    eng.run(torch_mod.as_tensor(workloads.lhs_params(50_000, "full", seed=7).T.copy(), device="cuda:0"), "float64")   # larger workspace in between
    for v in out.values():
        v.zero_()
    res = replay()
    torch_mod.cuda.synchronize()
    for k in ref:
        assert torch_mod.equal(out[k], ref[k]) and res[k] is out[k], k
    bad = dict(out)
    bad["R_TOA"] = torch_mod.zeros((B, 13), dtype=torch_mod.float64, device="cuda:0")
    with pytest.raises(ValueError, match="R_TOA"):
        eng.run(P, "float32", out=bad)
    bad["R_TOA"] = torch_mod.zeros((B + 1, 13), dtype=torch_mod.float32, device="cuda:0")
    with pytest.raises(ValueError, match="contiguous"):
        eng.run(P, "float32", out=bad)
    bad["R_TOA"] = torch_mod.zeros((13, B), dtype=torch_mod.float32, device="cuda:0").t()
    with pytest.raises(ValueError):
        eng.run(P, "float32", out=bad)
    keys = set(out)
    eng.run(P, "float32", out=out, materialize=("La",))
    assert set(out) == keys                                      # the caller's dict is not modified
    with pytest.raises(ValueError, match="weights"):
        eng.lut_nearest(out["R_TOA"], out["R_TOA"][:5], weights=np.ones(12))


def test_prepared_call_is_the_same_call(torch_mod):
    """Engine.prepare: run()'s argument marshalling done once; call() issues the same spart_run_batch over the same resident
    buffers -- new inputs written into them are seen, any stream may issue it, results are bit-identical to run()."""
    from spart_amd import get_engine, workloads
    torch = torch_mod
    eng = get_engine("Sentinel2A-MSI", 0)
    B = 4099
    Pa = torch.as_tensor(workloads.lhs_params(B, "full", seed=3).T.copy(), device="cuda:0")
    Pb = torch.as_tensor(workloads.lhs_params(B, "full", seed=4).T.copy(), device="cuda:0")
    lidf = torch.as_tensor(np.random.default_rng(1).dirichlet(np.full(13, 2.0), size=B), device="cuda:0")
    P = Pa.clone()
    out = {k: torch.empty((B, 13), dtype=torch.float64, device="cuda:0") for k in ("R_TOC", "R_TOA", "L_TOA", "La")}
    n0 = eng.calls["spart_run_batch"]
    call = eng.prepare(P, "float64", out=out, materialize=["La"], prune=True, canopy_lidf=lidf, nlayers=24)
    assert eng.calls["spart_run_batch"] == n0                      # nothing issued yet
    for src in (Pa, Pb, Pa):
        P.copy_(src)
        res = call()
        ref = eng.run(src, "float64", materialize=["La"], prune=True, canopy_lidf=lidf, nlayers=24)
        assert res["R_TOC"] is out["R_TOC"]
        for k in out:
            assert torch.equal(out[k], ref[k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        P.copy_(Pb)
        call()
    s.synchronize()
    assert torch.equal(out["R_TOA"], eng.run(Pb, "float64", prune=True, canopy_lidf=lidf, nlayers=24)["R_TOA"])
    with pytest.raises(ValueError):
        eng.prepare(P.cpu(), "float64", out=out)
    with pytest.raises(ValueError):
        eng.prepare(P, "float64", out=out, rho_thermal=0.01)       # host values would be frozen at prepare time: refused
    with pytest.raises(ValueError):
        eng.prepare(P, "float64", out=out, rdry=torch.zeros((B, 2001), dtype=torch.float64, device="cuda:0"))
    # the call owns its engine: an engine nothing else holds stays alive, with its context, as long as the call
    import gc
    import weakref
    from spart_amd.engine import Engine
    own = Engine("Sentinel2A-MSI", 0)
    alive = weakref.ref(own)
    call = own.prepare(P, "float64", out=out)
    del own
    gc.collect()
    assert alive() is not None
    call()
    assert all(torch.equal(out[k], v) for k, v in eng.run(P, "float64").items())


def test_lut_generation_streams_chunks(tmp_path, torch_mod):
    """generate_lut: chunked, double-buffered H2D / kernels / D2H; ragged last chunk; on-disk layout round trip."""
    import spart_amd
    from spart_amd import get_engine, workloads
    B = 25_013
    P = workloads.lhs_params(B, "full", seed=8)
    eng = get_engine("Sentinel2A-MSI", 0)
    ref = eng.run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), "float32")
    ref = {k: v.cpu().numpy() for k, v in ref.items()}
    d = str(tmp_path / "lut")
    out = spart_amd.generate_lut(P, "Sentinel2A-MSI", path=d, dtype="float32", chunk=4096)
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert np.array_equal(np.asarray(out[k]), ref[k]), k
    meta, params, cols = spart_amd.load_lut(d)
    assert meta["rows"] == B and meta["sensor"] == "Sentinel2A-MSI" and len(meta["wavelengths"]) == 13
    assert np.array_equal(np.asarray(params), P)
    assert np.array_equal(np.asarray(cols["R_TOA"]), ref["R_TOA"])
    mem = spart_amd.generate_lut(P[:100], "Sentinel2A-MSI", dtype="float64", chunk=64)
    ref64 = eng.run(torch_mod.as_tensor(P[:100].T.copy(), device="cuda:0"), "float64")
    assert np.array_equal(mem["R_TOC"], ref64["R_TOC"].cpu().numpy())
    # a caller-owned destination (a previous result reused: its pages are resident) is filled in place; a wrong one is refused
    mine = {k: np.full((B, 13), -1.0, dtype=np.float32) for k in ("R_TOC", "R_TOA", "L_TOA")}
    again = spart_amd.generate_lut(P, "Sentinel2A-MSI", chunk=4096, out=mine)
    assert all(again[k] is mine[k] and np.array_equal(mine[k], ref[k]) for k in mine) and again.rows == (0, B)
    with pytest.raises(ValueError, match="R_TOA"):
        spart_amd.generate_lut(P, "Sentinel2A-MSI", out=dict(mine, R_TOA=mine["R_TOA"][:-1]))
    with pytest.raises(ValueError, match="R_TOC"):
        spart_amd.generate_lut(P, "Sentinel2A-MSI", dtype="float64", out=mine)
    # (the parquet export of such a directory is covered without a GPU: tests/test_host_logic.py::test_lut_parquet_export,
    #  and -- where the box has a parquet engine -- end to end in test_lut_on_disk_parquet_leg below)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_lut_on_disk_matches_the_reference_rows(golden, dtype, tmp_path, torch_mod):
    """What generate_lut lands ON DISK against the real reference: the 256 golden rows of the config-4 LHS
    (tests/golden/e2e.npz, lhs_full/Sentinel2A-MSI), streamed in ragged chunks of 100 (3 chunks, the last of 56)
    through the upload / launch / download pipeline and read back from the .npy files."""
    import spart_amd
    g = golden["e2e"]
    P = g["lhs_full/Sentinel2A-MSI/P"]
    d = str(tmp_path / "lut")
    spart_amd.generate_lut(P, "Sentinel2A-MSI", path=d, dtype=dtype, chunk=100)
    meta, params, cols = spart_amd.load_lut(d, mmap=False)
    assert meta["rows"] == 256 and meta["dtype"] == dtype and np.array_equal(params, P)
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        arr = np.load(os.path.join(d, k + ".npy"))                        # the file itself, not the returned memmap
        assert arr.shape == (256, 13) and arr.dtype == (np.float64 if dtype == "float64" else np.float32)
        assert rel_err(arr, g[f"lhs_full/Sentinel2A-MSI/{k}"], COLFLOOR) < TOL[dtype], k
        assert np.array_equal(arr, np.asarray(cols[k]))


def test_lut_on_disk_parquet_leg(golden, tmp_path, torch_mod):
    """generate_lut -> lut_to_parquet -> pandas.read_parquet against the reference's golden rows.  The GPU boxes of this
    pool ship pandas without a parquet engine: that is reported as a SKIP here (never a silent pass); the export itself
    is asserted on the CPU suite (tests/test_host_logic.py::test_lut_parquet_export), where an engine is present."""
    pytest.importorskip("pyarrow", reason="no parquet engine on this box (export covered by tests/test_host_logic.py)")
    import pandas as pd
    import spart_amd
    g = golden["e2e"]
    d = str(tmp_path / "lut")
    spart_amd.generate_lut(g["lhs_full/Sentinel2A-MSI/P"], "Sentinel2A-MSI", path=d, dtype="float64", chunk=100)
    meta, _, _ = spart_amd.load_lut(d)
    df = pd.read_parquet(spart_amd.lut_to_parquet(d, str(tmp_path / "lut.parquet")))
    assert list(df.columns[:27]) == meta["param_names"] and df.shape == (256, 27 + 39)
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        tab = df[[f"{k}_{w:g}" for w in meta["wavelengths"]]].to_numpy()
        assert rel_err(tab, g[f"lhs_full/Sentinel2A-MSI/{k}"], COLFLOOR) < 1e-6, k


def _lut_brute_force():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import lut_brute_force
    return lut_brute_force


@pytest.mark.parametrize("dtype,nb", [("float32", 13), ("float64", 13), ("float32", 6), ("float32", 21), ("float32", 15),
                                      ("float32", 31), ("float32", 1), ("float32", 3), ("float64", 31), ("float64", 1),
                                      ("float64", 3)])
def test_lut_inversion_matches_brute_force(dtype, nb, torch_mod):
    """spart_lut_nearest returns THE argmin: index and cost bit-equal to a numpy brute force that evaluates the cost as the
    header defines it (sequential, in the call's dtype, no FMA; first index on ties -- the reference's np.argmin rule,
    SPART.py:381-387).  Weighted and unweighted, ragged sizes, a NaN row, exact members, every compiled K incl. nb = 1."""
    from spart_amd import get_engine
    bf = _lut_brute_force()
    rng = np.random.default_rng(nb)
    B, M = 20_011, 777
    npdt = np.float32 if dtype == "float32" else np.float64
    lut = rng.uniform(0.0, 0.6, (B, nb)).astype(npdt)
    lut[17] = np.nan                                  # a NaN row must never win
    obs = (lut[rng.integers(18, B, M)] + rng.normal(0, 0.01, (M, nb))).astype(npdt)
    obs[:5] = lut[100:105]                            # exact members: cost 0
    eng = get_engine(None, 0)
    for w in (None, rng.uniform(0.5, 2.0, nb).astype(npdt)):
        idx, cost, st = eng.lut_nearest(lut, obs, w, dtype, stats=True)
        idx, cost = idx.cpu().numpy(), cost.cpu().numpy()
        true_idx, true_cost = bf.brute_force_numpy(lut, obs, w)
        assert np.array_equal(idx, true_idx), (dtype, nb, int(np.sum(idx != true_idx)))
        assert np.array_equal(cost, true_cost)
        assert np.all(cost[:5] == 0.0) and np.all(idx >= 0) and 17 not in idx
        assert 0 <= st["brute_force"] <= M and np.isfinite(st["nmax"])


@pytest.mark.parametrize("dtype,nb", [("float32", 3), ("float32", 6), ("float32", 13), ("float32", 21), ("float64", 6)])
def test_lut_inversion_exact_on_a_correlated_lut(dtype, nb, torch_mod):
    """The hard case for a GEMM-form search: a 400 000-row LUT whose nb bands are smooth functions of 4 latent parameters
    (rows lie on a 4-dimensional sheet, neighbours are close) and observations = rows with 2 % noise.  In float32 the
    cancelling form |x|^2 - 2 x.y alone picks a wrong row for ~1 % of such observations at nb <= 6; the result here must be
    the exact argmin for every one of them (checked against an eager-torch brute force of the defined cost), and the filter
    must have done its job: only a small fraction may have needed the brute-force kernel."""
    from spart_amd import get_engine
    bf = _lut_brute_force()
    torch = torch_mod
    rng = np.random.default_rng(100 + nb)
    B, M = 400_000, 3000
    z = rng.uniform(0, 1, (B, 4))
    A, C = rng.normal(0, 1.5, (4, nb)), rng.normal(0, 1.0, (4, nb))
    npdt = np.float32 if dtype == "float32" else np.float64
    lut = (0.03 + 0.5 / (1.0 + np.exp(-(z @ A + (z * z) @ C - 1.0)))).astype(npdt)
    pick = rng.integers(0, B, M)
    obs = (lut[pick] * (1.0 + rng.normal(0, 0.02, (M, nb)))).astype(npdt)
    obs[:50] = lut[pick[:50]]                         # some exact members
    w = rng.uniform(0.5, 2.0, nb).astype(npdt)
    eng = get_engine(None, 0)
    L, O = torch.as_tensor(lut, device="cuda:0"), torch.as_tensor(obs, device="cuda:0")
    for ww in (None, torch.as_tensor(w, device="cuda:0")):
        idx, cost, st = eng.lut_nearest(L, O, ww, dtype, stats=True)
        true_idx, true_cost = bf.brute_force_torch(L, O, ww)
        assert torch.equal(idx, true_idx), (dtype, nb, int((idx != true_idx).sum()))
        assert torch.equal(cost, true_cost)
        assert float(cost[:50].max()) == 0.0
        if nb >= 6:                                   # (nb = 3: the rows fill a volume densely, many tiles tie within the bound)
            assert st["brute_force"] <= 0.05 * M, st  # the filter leaves the brute force a few per cent at most


def test_caller_owned_spectrum_buffers(torch_mod):
    """Engine.run(out=...) with caller-owned materialise buffers (the C ABI's ownership rule: the caller owns every buffer):
    results land in the given tensors, a second call reuses them, and a buffer with the wrong layout is refused."""
    from spart_amd import get_engine, workloads
    eng = get_engine("Sentinel2A-MSI", 0)
    P = torch_mod.as_tensor(workloads.lhs_params(300, "full", seed=2).T.copy(), device="cuda:0")
    fields = ("rso", "leaf_kchl", "rsoil")
    first = eng.run(P, "float32", materialize=fields)
    keep = {k: first[k].clone() for k in first}
    for v in first.values():
        v.zero_()
    again = eng.run(P, "float32", materialize=fields, out=first)
    for k in keep:
        assert again[k].data_ptr() == first[k].data_ptr() and torch_mod.equal(again[k], keep[k]), k
    with pytest.raises(ValueError, match="row stride"):
        eng.run(P, "float32", materialize=("rso",), out={"rso": torch_mod.empty((300, 2162), dtype=torch_mod.float32, device="cuda:0")})
    with pytest.raises(ValueError):
        eng.run(P, "float32", materialize=("rsoil",), out={"rsoil": torch_mod.empty((300, 12), dtype=torch_mod.float32, device="cuda:0")})


def test_fast_prelude_option_stays_inside_the_contract(golden, torch_mod):
    """Engine.run(lidf="newton") = spart_materialize.fast_prelude: the exact root of the LIDF equation (the reference stops its
    iteration up to ~5e-8 short, sailh.py:378-382) and 8-point hot-spot panels.  Against the REFERENCE's golden rows the
    columns must still meet the 1e-6 contract, and stay within 1e-6 of the default (literal) evaluation."""
    from spart_amd import get_engine
    g = golden["e2e"]
    for name, sensor in (("lhs_full/Sentinel2A-MSI", "Sentinel2A-MSI"), ("lhs_pro/Sentinel2B-MSI", "Sentinel2B-MSI")):
        eng = get_engine(sensor, 0)
        P = torch_mod.as_tensor(g[name + "/P"].T.copy(), device="cuda:0")
        lit, fast = eng.run(P, "float64"), eng.run(P, "float64", lidf="newton")
        for k in ("R_TOC", "R_TOA", "L_TOA"):
            assert rel_err(fast[k].cpu().numpy(), g[f"{name}/{k}"], COLFLOOR) < 1e-6, (name, k)
            d = rel_err(fast[k].cpu().numpy(), lit[k].cpu().numpy(), COLFLOOR)
            assert 0 < d < 1e-6, (name, k, d)             # (it IS a different prelude)
    with pytest.raises(ValueError):
        eng.run(P, "float64", lidf="bisect")


@pytest.mark.parametrize("kind,sensor", [("full", "Sentinel2A-MSI"), ("pro", "Sentinel2B-MSI")])
def test_fast_prelude_at_size(kind, sensor, torch_mod):
    """The numbers include/spart_hip.h states for spart_materialize.fast_prelude, re-measured over ALL 13M float64 column
    entries of the 1M-row config-4 / config-5 table on SURVEY 8(d)'s metric (floor 1e-6): 99.999 % of the entries within
    1.5e-7 (asserted: 3e-7), maximum 1.7e-5 (asserted: 5e-5), and the few entries above 1e-6 (15 / 27; asserted: < 100) all
    have a magnitude below 1e-3."""
    from spart_amd import get_engine, workloads
    eng = get_engine(sensor, 0)
    P = torch_mod.as_tensor(workloads.lhs_params(1_000_000, kind).T.copy(), device="cuda:0")
    a = {k: v.clone() for k, v in eng.run(P, "float64", prune=True).items()}
    b = eng.run(P, "float64", prune=True, lidf="newton")
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        rel = (b[k] - a[k]).abs() / a[k].abs().clamp_min(COLFLOOR)
        over = rel > 1e-6
        assert 0 < float(rel.max()) < 5e-5, (k, float(rel.max()))
        assert float(torch_mod.quantile(rel.flatten()[::7].float(), 0.99999)) < 3e-7, k
        assert int(over.sum()) < 100, (k, int(over.sum()))
        if bool(over.any()):
            assert float(a[k].abs()[over].max()) < 1e-3, (k, float(a[k].abs()[over].max()))


def test_lut_inversion_small_and_tied(torch_mod):
    """Sizes below one MFMA tile / one observation block, duplicate rows (ties go to the lowest row index, also across
    32-row tiles and across slices), mixed-sign weights, an all-NaN LUT and a NaN observation (index -1, cost inf); the
    duplicated rows force the brute-force kernel, which the statistics must show."""
    from spart_amd import get_engine
    bf = _lut_brute_force()
    eng = get_engine(None, 0)
    rng = np.random.default_rng(5)
    for dtype, npdt in (("float32", np.float32), ("float64", np.float64)):
        for B, M in ((1, 1), (20, 3), (33, 130), (4099, 1), (70_000, 5)):
            lut = rng.uniform(0.0, 0.6, (B, 13)).astype(npdt)
            obs = (lut[rng.integers(0, B, M)] + rng.normal(0, 0.01, (M, 13))).astype(npdt)
            for w in (None, rng.uniform(-0.2, 2.0, 13).astype(npdt)):
                idx, cost = eng.lut_nearest(lut, obs, w, dtype)
                ti, tc = bf.brute_force_numpy(lut, obs, w)
                assert np.array_equal(idx.cpu().numpy(), ti) and np.array_equal(cost.cpu().numpy(), tc), (dtype, B, M)
    lut = rng.uniform(0.0, 0.6, (5000, 13)).astype(np.float32)
    lut[[40, 700, 4100]] = lut[7]                     # the same row in three other tiles
    lut[3] = lut[2]
    for dtype in ("float32", "float64"):
        idx, cost, st = eng.lut_nearest(lut, lut[[7, 700, 3, 2]], dtype=dtype, stats=True)
        assert idx.cpu().tolist() == [7, 7, 2, 2] and float(cost.abs().max()) == 0.0, dtype
        obs = lut[:3].copy()
        obs[1, 4] = np.nan
        idx, cost = eng.lut_nearest(lut, obs, dtype=dtype)
        assert idx.cpu().tolist() == [0, -1, 2] and np.isinf(cost.cpu().numpy()[1]), dtype
        idx, cost = eng.lut_nearest(np.full((100, 13), np.nan, dtype=np.float32), lut[:2], dtype=dtype)
        assert idx.cpu().tolist() == [-1, -1] and bool(np.isinf(cost.cpu().numpy()).all()), dtype
        big = lut.copy()
        big[5] = np.inf                               # an infinite row and a huge one never win, nothing overflows the filter
        big[6] = 1e30
        idx, cost = eng.lut_nearest(big, lut[[5, 6, 8]], dtype=dtype)
        ti, tc = bf.brute_force_numpy(big.astype(np.float32 if dtype == "float32" else np.float64),
                                      lut[[5, 6, 8]].astype(np.float32 if dtype == "float32" else np.float64))
        assert np.array_equal(idx.cpu().numpy(), ti) and np.array_equal(cost.cpu().numpy(), tc), dtype
    # a LUT of ONE repeated row (more tiles than slices): every tile ties, every observation takes the brute force, row 0 wins
    same = np.tile(lut[9], (40_000, 1))
    idx, cost, st = eng.lut_nearest(same, lut[:70], stats=True)
    assert idx.cpu().tolist() == [0] * 70 and st["brute_force"] == 70


def test_lut_inversion_recovers_parameters(torch_mod):
    """End to end: build a LUT with the evaluator, invert noisy copies of some of its rows; exact members come back as
    themselves with cost 0 in both dtypes (round 3's float32 search returned a few-ulp-of-|x|^2 neighbour instead)."""
    from spart_amd import get_engine, workloads
    bf = _lut_brute_force()
    eng = get_engine("Sentinel2A-MSI", 0)
    P = workloads.lhs_params(200_000, "full", seed=33)
    out = eng.run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), "float32")
    for name in ("R_TOA", "L_TOA"):                    # reflectance scale and radiance scale
        lut = out[name].clone()
        pick = torch_mod.arange(0, 200_000, 997, device="cuda:0")
        idx, cost = eng.lut_nearest(lut, lut[pick])
        ti, tc = bf.brute_force_torch(lut, lut[pick])
        assert torch_mod.equal(idx, ti) and torch_mod.equal(cost, tc) and float(cost.max()) == 0.0
        assert float((idx == pick).double().mean()) > 0.999          # (duplicate rows aside, a member is its own nearest row)
        noisy = lut[pick] * (1 + 0.03 * torch_mod.randn((pick.numel(), lut.shape[1]), device="cuda:0", generator=torch_mod.Generator("cuda:0").manual_seed(1)))
        idx, cost = eng.lut_nearest(lut, noisy)
        ti, tc = bf.brute_force_torch(lut, noisy)
        assert torch_mod.equal(idx, ti) and torch_mod.equal(cost, tc)
        idx64, cost64 = eng.lut_nearest(lut.double(), noisy.double(), dtype="float64")
        ti, tc = bf.brute_force_torch(lut.double(), noisy.double())
        assert torch_mod.equal(idx64, ti) and torch_mod.equal(cost64, tc)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_user_dry_soil_spectra_full_chain(golden, dtype, torch_mod):
    """SPART.run with SoilParametersFromFile(array): the fused kernel reads the (B,2001) dry spectra from HBM."""
    import SPART
    from spart_amd import get_engine, workloads
    g = golden["rdry"]
    for i in range(4):
        sensor = str(g[f"{i}/sensor"])
        spec = g["spectra"][int(g[f"{i}/spec"])]
        soil = SPART.SoilParametersFromFile(spec[:, None].copy(), float(g[f"{i}/SMp"]), 25, 0.015)
        df = SPART.SPART(soil, SPART.LeafBiology(40, 0.01, 0.02, 0, 10, 10, 1.5), SPART.CanopyStructure(3, -0.35, -0.15, 0.05),
                         SPART.AtmosphericProperties(0.325, 0.35, 1.41, 1013.25), SPART.Angles(40, 0, 0), sensor, 100,
                         dtype=dtype).run(debug=True)
        for k in ("R_TOC", "R_TOA", "L_TOA", "rsoil"):
            assert rel_err(df[k].to_numpy(), g[f"{i}/{k}"], COLFLOOR) < TOL[dtype], (i, k)
    # batched: per-sample spectra, GSV columns absent
    eng = get_engine("Sentinel2A-MSI", 0)
    P = workloads.lhs_params(3, "full", seed=1)
    P[:, 12] = [20.0, 45.0, 4.0]
    cols = [P[:, j] for j in range(27)]
    cols[9] = cols[10] = cols[11] = None
    out = eng.run(cols, dtype, rdry=g["spectra"], materialize=("soil_refl_dry",))
    assert rel_err(out["soil_refl_dry"].cpu().numpy(), g["spectra"], 1e-3) < 1e-6


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_band_mean_with_user_dry_soil_and_no_spectra(dtype, torch_mod):
    """band_mean requested together with user dry-soil spectra but WITHOUT any materialised spectrum: the
    full-band kernel must read the user's spectra (its MAT = 2 variant), not mix a soil from the absent GSV columns --
    band_mean equals the batch mean of the canopy rows of a call that does materialise them, bit for bit, and differs
    from the GSV-soil means."""
    from spart_amd import get_engine, workloads
    eng = get_engine("Sentinel2A-MSI", 0)
    B = 700
    P = workloads.lhs_params(B, "full", seed=21)
    rng = np.random.default_rng(3)
    wl = np.arange(2001)
    rdry = 0.1 + 0.3 * rng.uniform(0, 1, (B, 1)) * (1 + 0.3 * np.sin(wl[None, :] / 150.0 + rng.uniform(0, 6, (B, 1))))
    cols = [P[:, j] for j in range(27)]
    cols[9] = cols[10] = cols[11] = None               # B, lat, lon: legally absent with rdry_in
    only = eng.run(cols, dtype, rdry=rdry, materialize=("band_mean",))
    bm_only = only["band_mean"].clone()
    both = eng.run(cols, dtype, rdry=rdry, materialize=("band_mean", "rso", "rdo", "rsd", "rdd"))
    assert torch_mod.equal(bm_only, both["band_mean"])
    for q, k in enumerate(("rso", "rdo", "rsd", "rdd")):
        m = both[k].double().mean(dim=0)
        assert float(((bm_only[q].double() - m).abs() / m.abs().clamp_min(1e-3)).max()) < (2e-5 if dtype == "float32" else 1e-10), k
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert torch_mod.equal(only[k], both[k])
    gsv = eng.run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), dtype, materialize=("band_mean",))["band_mean"]
    assert float((gsv - bm_only).abs().max()) > 1e-3   # (a different soil gives different means: the check above is not vacuous)


def test_one_engine_from_two_threads_and_streams(torch_mod):
    """SURVEY.md section 8(b) "Threading": a context is thread-safe.  Two host threads, each on its own torch stream,
    issue 20 interleaved run() calls each (different batches, dtypes and modes, full evaluation = side-stream fork / join)
    on ONE engine; every result must be bit-identical to the serial evaluation of the same call.  Then the case the
    engine avoids on purpose: two streams handing the library the SAME workspace -- the library orders the second call
    after the first (include/spart_hip.h), so the results are still the serial ones."""
    import threading
    from spart_amd import get_engine, workloads
    torch = torch_mod
    eng = get_engine("Sentinel2A-MSI", 0)
    jobs = []
    for i in range(40):
        B = 2000 + 997 * (i % 7)
        P = torch.as_tensor(workloads.lhs_params(B, "full", seed=100 + i).T.copy(), device="cuda:0")
        kw = [dict(dtype="float32"), dict(dtype="float64"), dict(dtype="float32", materialize=("rso", "rsoil")),
              dict(dtype="float32", prune=True)][i % 4]
        jobs.append((P, kw))
    serial = []
    for P, kw in jobs:
        serial.append({k: v.clone() for k, v in eng.run(P, **kw).items()})
    torch.cuda.synchronize()
    results, errors = [None] * len(jobs), []

    def worker(tid):
        try:
            st = torch.cuda.Stream("cuda:0")
            with torch.cuda.stream(st):
                for i in range(tid, len(jobs), 2):
                    P, kw = jobs[i]
                    results[i] = {k: v.clone() for k, v in eng.run(P, **kw).items()}
            st.synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, (ref, got) in enumerate(zip(serial, results)):
        for k in ref:
            assert torch.equal(ref[k], got[k]), (i, k)
    # one workspace shared by two streams: ordered by the library, results unchanged
    n = max(int(eng.lib.spart_workspace_bytes(eng.ctx, 1, P.shape[1])) for P, _ in jobs)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    sa, sb = torch.cuda.Stream("cuda:0"), torch.cuda.Stream("cuda:0")
    shared = [None] * 12
    for i in range(12):
        with torch.cuda.stream(sa if i % 2 == 0 else sb):
            P, kw = jobs[i]
            shared[i] = eng.run(P, _workspace=ws, **kw)
    torch.cuda.synchronize()
    for i in range(12):
        for k in serial[i]:
            assert torch.equal(serial[i][k], shared[i][k]), ("shared workspace", i, k)


def test_one_workspace_handed_to_twenty_streams(torch_mod):
    """include/spart_hip.h: two streams passing the same workspace are ordered by the library, "never a race" -- for ANY
    number of (workspace, stream) pairs.  Twenty streams hand ONE workspace to 80 interleaved run() calls on different
    batches (every call rewrites the workspace's per-sample constants, so a call that is not ordered after its predecessor
    reads another batch's constants); a small record list that recycled a live use (round 4: 16 records, least recently
    used out) would lose the order from the 17th pair on.  Every result must be bit-identical to the serial evaluation."""
    from spart_amd import get_engine, workloads
    torch = torch_mod
    eng = get_engine("Sentinel2A-MSI", 0)
    nstream, ncall, B = 20, 80, 30011
    Ps = [torch.as_tensor(workloads.lhs_params(B, "full", seed=500 + i).T.copy(), device="cuda:0") for i in range(8)]
    kws = [dict(dtype="float32", prune=True), dict(dtype="float64", prune=True), dict(dtype="float32")]
    serial = {}
    for i in range(ncall):
        key = (i % len(Ps), i % len(kws))
        if key not in serial:
            serial[key] = {k: v.clone() for k, v in eng.run(Ps[key[0]], **kws[key[1]]).items()}
    torch.cuda.synchronize()
    ws = torch.empty(int(eng.lib.spart_workspace_bytes(eng.ctx, 1, B)), dtype=torch.uint8, device="cuda:0")
    streams = [torch.cuda.Stream("cuda:0") for _ in range(nstream)]
    assert len({s.cuda_stream for s in streams}) == nstream
    got = [None] * ncall
    for i in range(ncall):
        with torch.cuda.stream(streams[(7 * i) % nstream]):
            got[i] = eng.run(Ps[i % len(Ps)], _workspace=ws, **kws[i % len(kws)])
    torch.cuda.synchronize()
    for i in range(ncall):
        ref = serial[(i % len(Ps), i % len(kws))]
        for k in ref:
            assert torch.equal(ref[k], got[i][k]), (i, k)
    # and a second workspace on the same twenty streams (40 live pairs), interleaved with the first
    ws2 = torch.empty_like(ws)
    for i in range(ncall):
        with torch.cuda.stream(streams[(3 * i) % nstream]):
            got[i] = eng.run(Ps[i % len(Ps)], _workspace=(ws if i % 2 else ws2), **kws[i % len(kws)])
    torch.cuda.synchronize()
    for i in range(ncall):
        ref = serial[(i % len(Ps), i % len(kws))]
        for k in ref:
            assert torch.equal(ref[k], got[i][k]), ("two workspaces", i, k)


def test_row_pitch_dense_and_padded_agree(torch_mod):
    """spart_ctx_set_row_pitch: the padded default (rows on the 128 B line grid) and the dense layout give
    bit-identical spectra through every entry point that reads or writes (B,2162) / (B,2001) arrays, including
    spectra handed back in as inputs (strided views and dense copies)."""
    from spart_amd import workloads
    from spart_amd.engine import Engine, ROW_PITCH
    pad, dense = Engine("Sentinel2A-MSI", 0), Engine("Sentinel2A-MSI", 0, row_pitch=None)
    B = 333
    P = torch_mod.as_tensor(workloads.lhs_params(B, "full", seed=11).T.copy(), device="cuda:0")
    fields = ("leaf_refl", "leaf_tran", "leaf_kchl", "soil_refl", "soil_refl_dry", "rso", "rdo", "rsd", "rdd")
    for dtype in ("float32", "float64"):
        a, b = pad.run(P, dtype, materialize=fields), dense.run(P, dtype, materialize=fields)
        assert a["rso"].stride() == (ROW_PITCH[0], 1) and a["leaf_kchl"].stride() == (ROW_PITCH[1], 1)
        assert b["rso"].is_contiguous()
        for k in fields + ("R_TOC", "R_TOA", "L_TOA"):
            assert torch_mod.equal(a[k], b[k]), (dtype, k)
        la, lb = pad.prospect([P[i] for i in range(9)], dtype), dense.prospect([P[i] for i in range(9)], dtype)
        sa, sb = pad.bsm([P[i] for i in range(9, 15)], dtype), dense.bsm([P[i] for i in range(9, 15)], dtype)
        assert all(torch_mod.equal(x, y) for x, y in zip(la + sa, lb + sb))
        # spectra back in: the padded engine takes its own strided outputs as they are, the dense engine's
        # contiguous ones through a re-pitching copy; user dry-soil spectra likewise
        can, ang = [P[i] for i in range(15, 19)], [P[i] for i in range(19, 22)]
        ca = pad.sailh(a["leaf_refl"], a["leaf_tran"], a["soil_refl"], can, ang, dtype)
        cb = dense.sailh(b["leaf_refl"], b["leaf_tran"], b["soil_refl"], can, ang, dtype)
        cc = pad.sailh(b["leaf_refl"], b["leaf_tran"], b["soil_refl"], can, ang, dtype)
        for x, y, z in zip(ca, cb, cc):
            assert torch_mod.equal(x, y) and torch_mod.equal(x, z)
        ra = pad.run(P, dtype, rdry=sa[1], materialize=("soil_refl",))
        rb = dense.run(P, dtype, rdry=sb[1], materialize=("soil_refl",))
        for k in ("soil_refl", "R_TOC", "R_TOA", "L_TOA"):
            assert torch_mod.equal(ra[k], rb[k]), (dtype, k)


def test_edge_rows_golden(golden, torch_mod):
    """The widened-range / edge-value rows of tests/golden/edge.npz (real reference outputs) through the C ABI.  float64:
    every row whose leaf has water or dry matter (without either, refl + tran = 1 exactly in the infrared and the
    reference divides by zero); float32: rows whose reference reflectances are still physical (0 <= R_TOC <= 1)."""
    from spart_amd import get_engine
    g = golden["edge"]
    P = g["P"]
    eng = get_engine(str(g["sensor"]), 0)
    Pd = torch_mod.as_tensor(P.T.copy(), device="cuda:0")
    o64, o32 = eng.run(Pd, "float64"), eng.run(Pd, "float32")
    keep = (P[:, 1] + P[:, 2]) > 0
    assert keep.sum() > 100
    for k, floor, tol in (("R_TOC", 1e-6, 1e-6), ("R_TOA", 1e-2, 2e-6), ("L_TOA", 1e-2, 2e-6)):
        assert rel_err(o64[k].cpu().numpy()[keep], g[k][keep], floor) < tol, k
    phys = keep & np.all((g["R_TOC"] >= 0) & (g["R_TOC"] <= 1), axis=1)
    assert phys.sum() > 60
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert rel_err(o32[k].cpu().numpy()[phys], g[k][phys], COLFLOOR) < 1e-4, k


def test_sentinel2_float64_coefficient_pins(golden, torch_mod):
    """Sentinel-2A/B against the reference run with its float32 SMAC coefficients up-cast to float64 in the harness
    (tests/golden/s2_f64.npz, make_golden.py gen_s2f64; SPART.py:228, smac.py:44-92): the float32-storage noise that forces
    2e-6 / 5e-7 on every other Sentinel-2 comparison is gone, so the HIP float64 path is held to 1e-9 on the nine SMAC
    outputs and 1e-8 on the columns (survey metric, floor 1e-6) for the defaults, PRO, the 256 config-4 rows and the 64
    config-5 rows, and to north_star's 1e-6 on a 1e-6 floor for R_TOA / L_TOA of the 128 edge rows (edge.npz needs floor 1e-2)."""
    from spart_amd import get_engine
    from spart_amd.engine import SMAC_FIELDS
    g = golden["s2_f64"]
    worst = {}
    for sensor in ("Sentinel2A-MSI", "Sentinel2B-MSI"):
        eng = get_engine(sensor, 0)
        out = eng.smac(list(g[f"smac/{sensor}/angles"].T), list(g[f"smac/{sensor}/atm"].T))
        for f in SMAC_FIELDS:
            e = rel_err(out[f].cpu().numpy(), g[f"smac/{sensor}/{f}"], COLFLOOR)
            worst[("smac", sensor)] = max(worst.get(("smac", sensor), 0.0), e)
            assert e < 1e-9, (sensor, f, e)
    for name in ("defaults/Sentinel2A-MSI", "defaults/Sentinel2B-MSI", "pro/Sentinel2B-MSI", "lhs_full/Sentinel2A-MSI",
                 "lhs_pro/Sentinel2B-MSI"):
        eng = get_engine(name.split("/")[1], 0)
        out = eng.run(torch_mod.as_tensor(g[name + "/P"].T.copy(), device="cuda:0"), "float64", materialize=("rsoil", "La"))
        for k in ("R_TOC", "R_TOA", "L_TOA", "rsoil", "La"):
            e = rel_err(out[k].cpu().numpy(), g[f"{name}/{k}"], COLFLOOR)
            worst[name] = max(worst.get(name, 0.0), e)
            assert e < 1e-8, (name, k, e)
    P = g["edge/Sentinel2A-MSI/P"]
    keep = (P[:, 1] + P[:, 2]) > 0                     # (test_edge_rows_golden: without water or dry matter the reference divides by zero)
    out = get_engine("Sentinel2A-MSI", 0).run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), "float64")
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        e = rel_err(out[k].cpu().numpy()[keep], g[f"edge/Sentinel2A-MSI/{k}"][keep], COLFLOOR)
        worst["edge/" + k] = e
        assert e < 1e-6, (k, e)
    print({str(k): f"{v:.1e}" for k, v in worst.items()})


MAT_FIELDS = ("leaf_refl", "leaf_tran", "leaf_kchl", "soil_refl", "soil_refl_dry", "rso", "rdo", "rsd", "rdd")


def _probe_rows(B, chunk, rng):
    """64 rows of a batch whose band kernel walks `chunk` samples per workgroup (spart_capi.hip pick_chunk): the front,
    two workgroup (chunk) boundaries, the 32-sample constant-staging boundary inside two chunks, the ragged tail, and
    random rows."""
    nchunk = -(-B // chunk)
    rows = list(range(0, 8))
    for c in (3, nchunk // 2):
        rows += list(range(c * chunk - 4, c * chunk + 4))
    if chunk > 32:
        for c in (5, nchunk - 2):
            rows += list(range(c * chunk + 32 - 4, min(c * chunk + 32 + 4, (c + 1) * chunk)))
    rows += list(range(B - 8, B))
    rows = sorted(set(r for r in rows if 0 <= r < B))
    extra = [int(r) for r in rng.choice(B, size=200, replace=False) if int(r) not in rows]
    rows = sorted(rows + extra[:64 - len(rows)])
    assert len(rows) == 64
    return rows


@pytest.mark.parametrize("dtype,B", [("float32", 300_001), ("float64", 270_001)])
def test_materialised_and_user_soil_paths_at_size(oracle, tables, dtype, B, torch_mod):
    """The store path of the fused kernel at a size where every part of its sample walk is exercised -- chunks of 37
    (float32) / 33 (float64) samples per workgroup, i.e. a full 32-sample staging block + a short one, a ragged last chunk,
    the per-sample row advance (off += pitch), the thermal-pad broadcast, the column kernel's support points -- with all nine
    spectrum arrays + rsoil + La + band_mean requested, for the padded and the dense row pitch, without (MAT = 1) and with
    per-sample user dry-soil spectra read from HBM (MAT = 2; SoilParametersFromFile, bsm.py:42-43).  64 probe rows are
    compared (a) with the oracle (leaf / soil / canopy spectra SPART.py:427-470, bsm.py:42-43, sailh.py:222-233 + the
    columns) at the stage tests' tolerances and (b) BIT FOR BIT with the same rows evaluated as 64 one-sample batches;
    the two pitches must agree bit for bit on everything, and band_mean must be the mean of the materialised rows."""
    import spart_amd.engine as E
    from spart_amd import workloads
    torch = torch_mod
    td = torch.float32 if dtype == "float32" else torch.float64
    chunk = -(-B // 8192)
    assert chunk > 32, "the batch must be large enough for more than one constant-staging block per workgroup"
    rng = np.random.default_rng(31)
    rows = _probe_rows(B, chunk, rng)
    Ph = workloads.lhs_params(B, "full", seed=77)
    P = torch.as_tensor(Ph.T.copy(), device="cuda:0")
    ridx = torch.as_tensor(rows, device="cuda:0")
    # per-sample dry-soil spectra: smooth, in (0.05, 0.6), different for every sample
    gen = torch.Generator(device="cuda:0").manual_seed(9)
    abc = torch.rand((B, 3), generator=gen, device="cuda:0", dtype=torch.float64)
    x = torch.arange(2001, device="cuda:0", dtype=torch.float64)[None, :]
    fields = MAT_FIELDS + ("rsoil", "La", "band_mean")
    tol, fl = TOL[dtype], FLOOR[dtype]
    pad = E.Engine("Sentinel2A-MSI", 0)
    dense = E.Engine("Sentinel2A-MSI", 0, row_pitch=None)
    for use_rdry in (False, True):
        rd = None
        if use_rdry:
            rd = (0.08 + 0.25 * abc[:, 0:1] + 0.2 * abc[:, 1:2] * (x / 2000.0) + 0.03 * abc[:, 2:3] * torch.sin(x / 90.0)).to(td)
        ref = oracle.spart_run(Ph[rows], "Sentinel2A-MSI", tables, pso="gl", full=True,
                               rdry=None if rd is None else rd[ridx].double().cpu().numpy())
        rho, tau = oracle.pad_leaf(ref["leaf_refl"], ref["leaf_tran"])
        expect = dict(leaf_refl=rho, leaf_tran=tau, leaf_kchl=ref["kChlrel"], soil_refl=oracle.pad_soil(ref["soil_refl"]),
                      soil_refl_dry=ref["soil_refl_dry"], rso=ref["rso"], rdo=ref["rdo"], rsd=ref["rsd"], rdd=ref["rdd"],
                      rsoil=ref["rsoil"], La=ref["La"], R_TOC=ref["R_TOC"], R_TOA=ref["R_TOA"], L_TOA=ref["L_TOA"])
        got = {}
        for name, eng in (("padded", pad), ("dense", dense)):
            out = eng.run(P, dtype, materialize=fields, rdry=rd)
            torch.cuda.synchronize()
            assert out["rso"].stride(0) == (E.ROW_PITCH[0] if name == "padded" else 2162)
            # band_mean (4, 2162) = mean over ALL samples of the materialised canopy rows (every row took part)
            for q, k in enumerate(("rso", "rdo", "rsd", "rdd")):
                m = out[k].double().mean(0)
                assert float(((out["band_mean"][q].double() - m).abs() / m.abs().clamp_min(1e-3)).max()) < (2e-5 if dtype == "float32" else 1e-10), (name, k)
            assert all(bool(torch.isfinite(out[k]).all()) for k in MAT_FIELDS), name
            got[name] = {k: out[k][ridx].cpu().numpy() for k in expect}
            del out
            torch.cuda.empty_cache()
        for k in expect:
            assert np.array_equal(got["padded"][k], got["dense"][k]), (use_rdry, k)
            floor = COLFLOOR if k in ("R_TOC", "R_TOA", "L_TOA", "rsoil", "La") else fl
            assert rel_err(got["padded"][k], expect[k], floor) < tol, (use_rdry, k)
        # the same rows as one-sample batches (chunk = 1: no walk at all)
        for j, r in enumerate(rows):
            one = pad.run(P[:, r:r + 1].contiguous(), dtype, materialize=fields, rdry=None if rd is None else rd[r:r + 1])   # (same kernel variant)
            for k in expect:
                assert np.array_equal(one[k].cpu().numpy()[0], got["padded"][k][j]), (use_rdry, r, k)
        del rd
    pad.release_workspace()
    dense.release_workspace()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind,sensor", [("full", "Sentinel2A-MSI"), ("pro", "Sentinel2B-MSI")])
def test_parity_at_scale_against_the_oracle(torch_mod, tmp_path, kind, sensor):
    """The tolerance claim of the headline, where the driver sees it: 65 536 FRESH Latin-hypercube rows (a seed nothing else
    uses) of BASELINE config 4 (Sentinel-2A) resp. config 5 (PROSPECT-PRO, Sentinel-2B) through the ORACLE -- a child
    process with a pool of host processes (tests/helpers/oracle_rows.py; this process has initialised HIP and must not
    fork) -- against the HIP float64 mode, the default float32 mode and float64 columns over float32 bands (f32_bands), on
    SURVEY section 8(d)'s metric |x - ref| / max(|ref|, 1e-6).  The reference samples its own grids the same way
    (tests/conftest.py:17-45); this is 64x the rows the golden fixtures hold.  Bounds: float64 <= 5e-8 (the oracle's closed-form E1
    against the kernels' own series; 1.6e-8 measured over 2 x 1M rows), float32 <= 1e-4 (north_star)."""
    import subprocess
    from spart_amd import get_engine, workloads
    rows, seed = 65536, 20251004
    out = str(tmp_path / "oracle.npz")
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "oracle_rows.py"), kind, sensor, str(rows), str(seed), out],
                   check=True, env=env, timeout=900)
    ref = np.load(out)
    Pn = workloads.lhs_params(rows, kind, seed=seed)
    P = torch_mod.as_tensor(Pn.T.copy(), device="cuda:0")
    eng = get_engine(sensor, 0)
    modes = {"float64": (dict(dtype="float64"), 5e-8), "float32": (dict(dtype="float32"), 1e-4),
             "f32_bands": (dict(dtype="float64", f32_bands=True), 5e-8)}
    cols = {}
    for name, (kw, tol) in modes.items():
        o = eng.run(P, **kw)
        cols[name] = o
        for k in ("R_TOC", "R_TOA", "L_TOA"):
            x, r = o[k].double().cpu().numpy(), ref[k]
            assert np.isfinite(r).all() and np.isfinite(x).all()
            rel = np.abs(x - r) / np.maximum(np.abs(r), COLFLOOR)
            i, j = np.unravel_index(np.argmax(rel), rel.shape)
            print(f"[at scale] {kind}/{sensor} {name} {k}: max {rel.max():.3e} p99.9 {np.quantile(rel, 0.999):.3e} over {rel.size} entries; "
                  f"worst row {i} band {j} ref {r[i, j]:.6e} got {x[i, j]:.6e} params {np.array2string(Pn[i], precision=5, separator=',')}"
                  f" (oracle: {float(ref['seconds']):.1f} s on {int(ref['processes'])} processes)")
            assert rel.max() <= tol, (name, k, float(rel.max()), int(i), int(j), Pn[i].tolist())
    for k in ("R_TOC", "R_TOA", "L_TOA"):      # f32_bands: the float64 columns themselves, not an approximation of them
        assert torch_mod.equal(cols["float64"][k], cols["f32_bands"][k])


def test_results_do_not_depend_on_wave_mates(torch_mod):
    """A sample's columns are a function of its own 27 parameters: the same batch twice, the batch reversed, and every
    2048th row evaluated alone give bit-identical float64 columns.  (The prelude deals its samples to waves by a counting sort
    whose order inside a bucket is not fixed, and several routines branch on wave-level votes -- all of them may only SKIP work
    no lane needs, never pick the arithmetic of one lane from the data of another; round 5 had a version of the LIDF iteration
    that did, and whose results changed from call to call in the last bits.)"""
    from spart_amd import get_engine, workloads
    eng = get_engine("Sentinel2A-MSI", 0)
    B = 100_003
    Pn = workloads.lhs_params(B, "full", seed=77)
    P = torch_mod.as_tensor(Pn.T.copy(), device="cuda:0")
    a = {k: v.clone() for k, v in eng.run(P, "float64").items()}
    b = eng.run(P, "float64")
    Pr = torch_mod.as_tensor(Pn[::-1].T.copy(), device="cuda:0")
    c = eng.run(Pr, "float64", prune=True)
    rows = list(range(0, B, 2048))
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        assert torch_mod.equal(a[k], b[k]), k
        assert torch_mod.equal(a[k], c[k].flip(0)), k
    for r in rows[:24]:
        one = eng.run(torch_mod.as_tensor(Pn[r:r + 1].T.copy(), device="cuda:0"), "float64")
        for k in ("R_TOC", "R_TOA", "L_TOA"):
            assert torch_mod.equal(one[k][0], a[k][r]), (r, k)


def test_event_queries_do_not_break_a_capture_in_progress(torch_mod):
    """The library looks for completed workspace records with hipEventQuery when a new (workspace, stream) pair shows up and
    16 are remembered.  An event query is a "potentially unsafe" call under a GLOBAL-mode stream capture (torch.cuda.graph's
    default) anywhere in the process: the library switches the calling thread to relaxed capture interaction around its
    queries and never queries on a capturing stream.  Here: a capture is open on one stream while 20 other streams make
    ordinary calls with new pairs (every one of them runs the query loop); the capture must survive, its replay and the
    ordinary calls must give the serial results."""
    from spart_amd import get_engine, workloads
    torch = torch_mod
    eng = get_engine("Sentinel2A-MSI", 0)
    B = 8192
    P = torch.as_tensor(workloads.lhs_params(B, "full", seed=31).T.copy(), device="cuda:0")
    P2 = torch.as_tensor(workloads.lhs_params(B, "full", seed=32).T.copy(), device="cuda:0")
    ref = {k: v.clone() for k, v in eng.run(P, "float32").items()}
    ref2 = {k: v.clone() for k, v in eng.run(P2, "float32", prune=True).items()}
    n = int(eng.lib.spart_workspace_bytes(eng.ctx, 1, B))
    ws, ws2, wsg = (torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in range(3))
    mk = lambda: {k: torch.empty((B, eng.nb), dtype=torch.float32, device="cuda:0") for k in ("R_TOC", "R_TOA", "L_TOA")}   # noqa: E731
    out, outs2 = mk(), [mk() for _ in range(20)]
    streams = [torch.cuda.Stream("cuda:0") for _ in range(20)]
    for st in streams:                                   # more than 16 live records before the capture starts
        with torch.cuda.stream(st):
            eng.run(P2, "float32", prune=True, _workspace=ws, out=outs2[0])
    cap = torch.cuda.Stream("cuda:0")
    with torch.cuda.stream(cap):
        eng.run(P, "float32", out=out, _workspace=wsg)    # (first use of the stream and of the workspace: outside the capture)
    torch.cuda.synchronize()
    for t in out.values():
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        eng.run(P, "float32", out=out, _workspace=wsg)
        for i, st in enumerate(streams):                 # ordinary work on other streams while the capture is open
            with torch.cuda.stream(st):
                eng.run(P2, "float32", prune=True, _workspace=ws2, out=outs2[i])
    torch.cuda.synchronize()
    for i in range(20):
        for k in ref2:
            assert torch.equal(outs2[i][k], ref2[k]), (i, k)
    assert not any(bool(t.any()) for t in out.values())   # (captured, not run)
    g.replay()
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    # the same from ANOTHER host thread while this one holds a capture open (each thread has its own capture-interaction mode)
    import threading
    ws3 = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    streams3 = [torch.cuda.Stream("cuda:0") for _ in range(20)]
    go, done, errors = threading.Event(), threading.Event(), []

    def worker():
        try:
            go.wait(30)
            for i, st in enumerate(streams3):
                with torch.cuda.stream(st):
                    eng.run(P2, "float32", prune=True, _workspace=ws3, out=outs2[i])
        except Exception as e:      # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    for o in outs2:
        for t in o.values():
            t.zero_()
    th = threading.Thread(target=worker)
    th.start()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=cap):
        eng.run(P, "float32", out=out, _workspace=wsg)
        go.set()
        assert done.wait(60)
    th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(20):
        for k in ref2:
            assert torch.equal(outs2[i][k], ref2[k]), ("worker thread", i, k)
    for t in out.values():
        t.zero_()
    g2.replay()
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(out[k], ref[k]), ("second graph", k)


def test_c_abi_argument_checks(torch_mod):
    """The C ABI's own argument checks, called directly on a real context (the engine replaces None before the library sees
    it): each rejected call returns its code and message before any launch -- the caller's outputs stay untouched -- and
    the NULL columns the rule allows (params 9-11 with rdry_in, 16-17 with lidf_in) give the engine's columns bit for bit."""
    import ctypes
    from spart_amd import _lib, get_engine, workloads
    torch = torch_mod
    INVALID, WORKSPACE, NOSENSOR = -1, -3, -4
    eng = get_engine("Sentinel2A-MSI", 0)
    lib, ctx, st = eng.lib, eng.ctx, eng._stream()
    B = 257
    P = torch.as_tensor(workloads.lhs_params(B, "full", seed=91).T.copy(), device="cuda:0")
    cols = list(P)

    ws_t = torch.empty(int(lib.spart_workspace_bytes(ctx, 1, B)), dtype=torch.uint8, device="cuda:0")
    ws, wsn = ctypes.c_void_p(ws_t.data_ptr()), ctypes.c_size_t(ws_t.numel())

    def rejected(rc, code, fragment, c=ctx):
        msg = lib.spart_last_error(c).decode()
        assert rc == code and fragment in msg, (rc, msg)

    def with_null(ts, *idx):
        return eng._ptrs([None if i in idx else t for i, t in enumerate(ts)])

    spec = {w: torch.full((B, w), -7.0, dtype=torch.float64, device="cuda:0") for w in (_lib.NWL, _lib.NWLS)}
    outs = [torch.full((B, eng.nb), -7.0, dtype=torch.float64, device="cuda:0") for _ in range(3)]
    optr = [o.data_ptr() for o in outs]
    s1, s2 = spec[_lib.NWL].data_ptr(), spec[_lib.NWLS].data_ptr()

    # spart_prospect_batch / spart_bsm_batch / spart_sailh_batch / spart_smac_batch
    rejected(lib.spart_prospect_batch(ctx, 1, B, with_null(cols[:9], 3), s1, s1, s1, ws, wsn, st), INVALID, "leaf[3] is null")
    rejected(lib.spart_bsm_batch(ctx, 1, B, with_null(cols[9:15], 1), None, s1, s1, ws, wsn, st), INVALID, "soil[1] is null")
    rejected(lib.spart_bsm_batch(ctx, 1, B, with_null(cols[9:15], 0, 3), s1, s1, s1, ws, wsn, st), INVALID, "soil[3] is null")
    out4 = eng._ptrs([spec[_lib.NWLS]] * 4)
    rejected(lib.spart_sailh_batch(ctx, 1, B, s2, s2, s2, with_null(cols[15:19], 1), eng._ptrs(cols[19:22]), None, 0, out4,
                                   ws, wsn, st), INVALID, "canopy/out4[1] is null")
    rejected(lib.spart_sailh_batch(ctx, 1, B, s2, s2, s2, eng._ptrs(cols[15:19]), with_null(cols[19:22], 2), None, 0, out4,
                                   ws, wsn, st), INVALID, "angles[2] is null")
    for nl in (-1, 1000001):
        rejected(lib.spart_sailh_batch(ctx, 1, B, s2, s2, s2, eng._ptrs(cols[15:19]), eng._ptrs(cols[19:22]), None, nl, out4,
                                       ws, wsn, st), INVALID, f"nlayers = {nl}")
    out9 = eng._ptrs([outs[0]] * 9)
    rejected(lib.spart_smac_batch(ctx, B, with_null(cols[19:22], 0), eng._ptrs(cols[22:26]), out9, ws, wsn, st), INVALID,
             "angles[0] is null")
    rejected(lib.spart_smac_batch(ctx, B, eng._ptrs(cols[19:22]), with_null(cols[22:26], 2), out9, ws, wsn, st), INVALID,
             "atm[2] is null")
    # spart_run_batch
    mat = _lib.SpartMaterialize()
    run = lambda ptrs, dt=1, b=B, m=None, w=ws, n=wsn: lib.spart_run_batch(ctx, dt, b, ptrs, None, None, *optr,  # noqa: E731
                                                                            ctypes.byref(m) if m is not None else None, w, n, st)
    rd = eng._rows(torch.linspace(0.05, 0.4, _lib.NWL, dtype=torch.float64, device="cuda:0"), B, _lib.NWL, torch.float64)
    lidf = eng.lidf(P[16], P[17])
    mat.rdry_in, mat.lidf_in = rd.data_ptr(), lidf.data_ptr()
    rejected(run(with_null(cols, 9, 10, 11, 12, 16, 17), m=mat), INVALID, "params[12] is null")
    rejected(run(with_null(cols, 9)), INVALID, "params[9] is null")
    for nl in (-1, 1000001):
        m = _lib.SpartMaterialize()
        m.nlayers = nl
        rejected(run(eng._ptrs(cols), m=m), INVALID, f"nlayers = {nl}")
    rejected(run(eng._ptrs(cols), dt=2), INVALID, "bad dtype 2")
    rejected(run(eng._ptrs(cols), b=-1), INVALID, "negative batch")
    rejected(run(None, b=60_000_001), INVALID, "at most 60000000 samples")
    rejected(lib.spart_run_batch(None, 1, B, eng._ptrs(cols), None, None, *optr, None, ws, wsn, st), INVALID, "null context")
    rejected(run(eng._ptrs(cols), n=ctypes.c_size_t(wsn.value - 1)), WORKSPACE,
             f"workspace of {wsn.value} bytes needed, {wsn.value - 1} given")
    m = _lib.SpartMaterialize()
    m.f32_bands, m.leaf_refl = 1, spec[_lib.NWLS].data_ptr()
    rejected(run(eng._ptrs(cols), m=m), INVALID, "f32_bands")
    m = _lib.SpartMaterialize()
    bm = torch.full((4, _lib.NWLS), -7.0, dtype=torch.float64, device="cuda:0")
    m.prune_unused_bands, m.band_mean = 1, bm.data_ptr()
    rejected(run(eng._ptrs(cols), m=m), INVALID, "band_mean needs prune_unused_bands = 0")
    # B = 0: nothing to check, nothing to do, whatever the pointers
    assert lib.spart_run_batch(ctx, 1, 0, None, None, None, None, None, None, None, None, 0, st) == 0
    assert lib.spart_prospect_batch(ctx, 1, 0, None, None, None, None, None, 0, st) == 0
    assert lib.spart_bsm_batch(ctx, 1, 0, None, None, None, None, None, 0, st) == 0
    assert lib.spart_sailh_batch(ctx, 1, 0, None, None, None, None, None, None, 0, None, None, 0, st) == 0
    assert lib.spart_smac_batch(ctx, 0, None, None, None, None, 0, st) == 0
    # a context without a sensor
    e0 = get_engine(None, 0)
    ws0 = torch.empty(int(lib.spart_workspace_bytes(e0.ctx, 1, B)), dtype=torch.uint8, device="cuda:0")
    rejected(lib.spart_smac_batch(e0.ctx, B, eng._ptrs(cols[19:22]), eng._ptrs(cols[22:26]), out9, ws0.data_ptr(),
                                  ws0.numel(), st), NOSENSOR, "no sensor", e0.ctx)
    # spart_lut_nearest: its own size rules
    rejected(lib.spart_lut_nearest(ctx, 0, B, 32, None, 5, None, None, None, None, None, 0, st), INVALID, "bad sizes")
    rejected(lib.spart_lut_nearest(ctx, 0, 0, 4, None, 5, None, None, None, None, None, 0, st), INVALID, "empty LUT")
    torch.cuda.synchronize()
    for t in list(spec.values()) + outs + [bm]:                  # no rejected call launched anything
        assert bool((t == -7.0).all())
    # accepted NULLs: B / lat / lon with rdry_in, LIDFa / LIDFb with lidf_in -- the engine's columns, bit for bit
    for dtype, dt in (("float64", 1), ("float32", 0)):
        td = torch.float64 if dt else torch.float32
        ref = eng.run(P, dtype, rdry=rd, canopy_lidf=lidf)
        got = {k: torch.full((B, eng.nb), -7.0, dtype=td, device="cuda:0") for k in ("R_TOC", "R_TOA", "L_TOA")}
        rdt = eng._rows(rd, B, _lib.NWL, td)
        m = _lib.SpartMaterialize()
        m.rdry_in, m.lidf_in = rdt.data_ptr(), lidf.data_ptr()
        rc = lib.spart_run_batch(ctx, dt, B, with_null(cols, 9, 10, 11, 16, 17), None, None, *[got[k].data_ptr() for k in got],
                                 ctypes.byref(m), ws, wsn, st)
        _lib.check(lib, ctx, rc)
        torch.cuda.synchronize()
        for k in got:
            assert torch.equal(got[k], ref[k]), (dtype, k)
