"""SRF-convolved sensor columns (spart_materialize.R_TOC_srf ... rdd_srf, kernel k_columns_srf) on the MI355X: against the
oracle's spectra convolved by helpers/srf_numpy.py, against the real reference (tests/golden/srf.npz), against the engine's
own materialised spectra, across batch sizes, band counts and modes, and through the Python surface (band_model="srf").

Metric everywhere: max |x - ref| / max(|ref|, 1e-6), NaN-aware (srf_numpy.rel_err); 1e-8 is the project's float64 contract."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from helpers import srf_numpy as S

pytestmark = pytest.mark.gpu

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SENSORS = ["TerraAqua-MODIS", "LANDSAT4-TM", "LANDSAT5-TM", "LANDSAT7-ETM", "LANDSAT8-OLI", "Sentinel2A-MSI", "Sentinel2B-MSI",
           "Sentinel3A-OLCI", "Sentinel3B-OLCI"]
CANOPY = ("rso", "rdo", "rsd", "rdd")
SRF7 = ["R_TOC_srf", "R_TOA_srf", "L_TOA_srf", "rso_srf", "rdo_srf", "rsd_srf", "rdd_srf"]
COLS = ("R_TOC", "R_TOA", "L_TOA")
F64, F32 = 1e-8, 1e-4


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def rows():
    """64 Latin-hypercube rows + the default row"""
    from spart_amd import workloads
    return np.concatenate([workloads.lhs_params(64, "full", seed=1358), workloads.default_row()], axis=0)


@pytest.fixture(scope="module")
def canopy(oracle, tables, rows):
    """the oracle's full run of the 65 rows, once: the canopy spectra do not depend on the sensor"""
    with np.errstate(all="ignore"):
        return oracle.spart_run(rows, "Sentinel2A-MSI", tables, pso="gl", full=True)


def sensor_tables_of(si):
    """the oracle's sensor block (sensor_tables) of a reference-style sensorinfo dict"""
    from spart_amd import tables as tb
    return {"wl_smac": np.asarray(si["wl_smac"], dtype=np.float64).reshape(-1),
            "coef": np.stack([np.asarray(si["SMAC_coef"][n], dtype=np.float64).reshape(-1) for n in tb.COEF_NAMES]),
            "wl_srf": np.asarray(si["wl_srf_smac"], dtype=np.float64), "p_srf": np.asarray(si["p_srf_smac"], dtype=np.float64)}


def expected(oracle, tables, P, spectra, sens):
    """the seven outputs by the definition: srf_numpy's convolution of the four canopy spectra, then the oracle's SMAC, its
    convolved irradiance and TOC -> TOA"""
    P = np.atleast_2d(P)
    conv = {x: S.convolve(spectra[x], sens["wl_srf"], sens["p_srf"]) for x in CANOPY}
    with np.errstate(all="ignore"):
        at = oracle.smac(P[:, 19:22], P[:, 22:26], sens)
        La = (oracle.et_correction(P[:, 26]) * np.cos(P[:, 19] * np.pi / 180) / np.pi)[:, None] * oracle.et_convolution(tables, sens)[None, :]
    rtoc, rtoa, ltoa = S.toc_to_toa(at, conv["rso"], conv["rdo"], conv["rsd"], conv["rdd"], La)
    return dict(R_TOC_srf=rtoc, R_TOA_srf=rtoa, L_TOA_srf=ltoa, **{x + "_srf": conv[x] for x in CANOPY})


def run(eng, P, dtype="float64", fields=SRF7, **kw):
    import torch
    res = eng.run(torch.as_tensor(np.atleast_2d(P).T.copy(), device=eng.device), dtype, materialize=fields, **kw)
    torch.cuda.synchronize()
    return res


def host(res, keys):
    return {k: res[k].double().cpu().numpy() for k in keys}


def worst(got, want, keys=SRF7):
    return {k: S.rel_err(got[k], want[k]) for k in keys}


# ------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("sensor", SENSORS)
def test_against_the_oracle_on_every_packaged_sensor(torch_mod, oracle, tables, rows, canopy, sensor):
    """literal tables (MODIS and OLCI with their SRF columns in the packaged order: the engine does what the tables say)"""
    from spart_amd import get_engine
    want = expected(oracle, tables, rows, canopy, oracle.sensor_tables(tables, sensor))
    eng = get_engine(sensor, 0)
    for dtype, tol in (("float64", F64), ("float32", F32)):
        err = worst(host(run(eng, rows, dtype), SRF7), want)
        print(sensor, dtype, {k: f"{v:.2e}" for k, v in err.items()})
        assert max(err.values()) <= tol, (sensor, dtype, err)


# ------------------------------------------------------------------ 2. against the real reference
@pytest.mark.parametrize("sensor", ["Sentinel2A-MSI", "LANDSAT7-ETM", "LANDSAT8-OLI", "TerraAqua-MODIS"])
def test_against_the_reference_fixture(torch_mod, sensor):
    """tests/golden/srf.npz: the reference's own calculate_spectral_convolution on its own canopy spectra, its atmopt and _La.
    Sentinel-2 carries float32 SMAC coefficients upstream: 1e-7 on the atmosphere-dependent columns, as for e2e.npz"""
    from spart_amd import get_engine
    z = np.load(os.path.join(ROOT, "tests", "golden", "srf.npz"))
    got = host(run(get_engine(sensor, 0), z["P"]), SRF7)
    err = worst(got, {k: z[f"{sensor}/{k}"] for k in SRF7})
    print(sensor, {k: f"{v:.2e}" for k, v in err.items()})
    assert max(err[x + "_srf"] for x in CANOPY) <= F64, err
    assert max(err[k + "_srf"] for k in COLS) <= (1e-7 if sensor.startswith("Sentinel2") else F64), err


# ------------------------------------------------------------------ 3. self-consistency
def test_convolution_of_the_engines_own_spectra(torch_mod, rows):
    """one float64 call materialises rso ... rdd (B, 2162) together with rso_srf ... rdd_srf"""
    from spart_amd import get_engine, tables as tb
    for sensor in ("Sentinel2A-MSI", "LANDSAT8-OLI", "TerraAqua-MODIS"):
        si = tb.load_sensor_info(sensor)
        res = run(get_engine(sensor, 0), rows, fields=list(CANOPY) + SRF7)
        spectra = host(res, CANOPY)
        got = host(res, SRF7)
        err = {x: S.rel_err(got[x + "_srf"], S.convolve(spectra[x], si["wl_srf_smac"], si["p_srf_smac"])) for x in CANOPY}
        print(sensor, {k: f"{v:.2e}" for k, v in err.items()})
        assert max(err.values()) <= F64, (sensor, err)


def test_one_unit_sample_at_the_centre_gives_the_centre_columns(torch_mod, rows):
    """a synthetic sensor whose SRF is ONE sample of weight 1 at each (integer) band centre: the convolution is the sample --
    the four canopy columns, R_TOA and L_TOA bit for bit; R_TOC within the float64 contract (a
    quotient in one kernel against a reciprocal product in the other)"""
    from spart_amd import get_engine, tables as tb
    si = dict(tb.load_sensor_info("Sentinel2A-MSI"))
    centres = np.asarray(si["wl_smac"], dtype=np.float64).reshape(-1)
    assert np.array_equal(centres, np.round(centres))
    si["wl_srf_smac"], si["p_srf_smac"] = centres[None, :].copy(), np.ones((1, centres.size))
    eng = get_engine(None, 0, sensor_info=si)
    res = run(eng, rows, fields=list(CANOPY) + SRF7)
    got = host(res, list(COLS) + SRF7)
    spectra = host(res, CANOPY)
    at = (centres - 400).astype(int)
    err = {k: S.rel_err(got[k + "_srf"], got[k]) for k in COLS}
    err.update({x: S.rel_err(got[x + "_srf"], spectra[x][:, at]) for x in CANOPY})
    print({k: f"{v:.2e}" for k, v in err.items()})
    assert max(err.values()) <= F64, err
    for x in CANOPY:
        assert np.array_equal(got[x + "_srf"], spectra[x][:, at], equal_nan=True), x
    for k in ("R_TOA", "L_TOA"):
        assert np.array_equal(got[k + "_srf"], got[k], equal_nan=True), k


# ------------------------------------------------------------------ 4. shapes and modes
@pytest.fixture(scope="module")
def s2_base(torch_mod, rows):
    """130 rows (the 65 twice, the second half reversed) on Sentinel-2A, float64, pruned: the batch every slice is compared with"""
    from spart_amd import get_engine
    P = np.concatenate([rows, rows[::-1]], axis=0)
    eng = get_engine("Sentinel2A-MSI", 0)
    return eng, P, host(run(eng, P, prune=True), list(COLS) + SRF7)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_batch_sizes_are_bit_identical_slices(s2_base, B):
    eng, P, base = s2_base
    got = host(run(eng, P[:B], prune=True), list(COLS) + SRF7)
    for k in got:
        assert got[k].shape == (B, 13) and np.array_equal(got[k], base[k][:B], equal_nan=True), (B, k)


def test_a_batch_equals_its_one_sample_calls(s2_base):
    eng, P, base = s2_base
    for i in range(P.shape[0]):
        one = host(run(eng, P[i:i + 1], prune=True), SRF7)
        for k in SRF7:
            assert np.array_equal(one[k][0], base[k][i], equal_nan=True), (i, k)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_modes_give_the_same_bits_and_leave_the_existing_outputs_alone(s2_base, dtype):
    """pruned == unpruned == f32_bands, and a call with *_srf requested returns the existing outputs of a call without"""
    eng, P, _ = s2_base
    P = P[:65]
    old = ["rsoil", "La", "rso", "leaf_refl"]
    with_srf = host(run(eng, P, dtype, fields=old + SRF7), list(COLS) + old + SRF7)
    without = host(run(eng, P, dtype, fields=old), list(COLS) + old)
    for k in without:
        assert np.array_equal(with_srf[k], without[k], equal_nan=True), (dtype, k)
    pruned = host(run(eng, P, dtype, prune=True), list(COLS) + SRF7)
    for k in pruned:
        assert np.array_equal(pruned[k], with_srf[k], equal_nan=True), (dtype, k)
    if dtype == "float64":
        mixed = host(run(eng, P, dtype, f32_bands=True), list(COLS) + SRF7)
        for k in mixed:
            assert np.array_equal(mixed[k], pruned[k], equal_nan=True), k
    else:                                                  # float32: the float64 column path rounded once
        f64 = host(run(eng, P, "float64", prune=True), SRF7)
        for k in SRF7:
            assert np.array_equal(pruned[k], f64[k].astype(np.float32).astype(np.float64), equal_nan=True), k


def one_band(si, j):
    out = dict(si)
    out["wl_smac"] = np.asarray(si["wl_smac"], dtype=np.float64).reshape(-1, 1)[j:j + 1]
    out["band_id_smac"] = [list(si["band_id_smac"])[j]]
    out["SMAC_coef"] = {n: np.asarray(v, dtype=np.float64).reshape(1, -1)[:, j:j + 1].copy() for n, v in si["SMAC_coef"].items()}
    out["wl_srf_smac"] = np.ascontiguousarray(np.asarray(si["wl_srf_smac"], dtype=np.float64)[:, j:j + 1])
    out["p_srf_smac"] = np.ascontiguousarray(np.asarray(si["p_srf_smac"], dtype=np.float64)[:, j:j + 1])
    return out


@pytest.mark.parametrize("nb", [1, 6, 13, 20, 211])
def test_band_counts(torch_mod, oracle, tables, rows, canopy, nb):
    """one wave of a workgroup, whole groups, a last group of one band, 53 groups; 211: SRF samples in the thermal pad"""
    from spart_amd import get_engine, tables as tb
    if nb == 211:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        from make_hyperspectral import sensorinfo_from_npz
        si = sensorinfo_from_npz(dict(np.load(os.path.join(ROOT, "tests", "golden", "hyperspectral.npz"))))
    elif nb == 1:
        si = one_band(tb.load_sensor_info("LANDSAT8-OLI"), 4)
    else:
        si = tb.load_sensor_info({6: "LANDSAT7-ETM", 13: "Sentinel2B-MSI", 20: "TerraAqua-MODIS"}[nb])
    eng = get_engine(None, 0, sensor_info=si)
    assert eng.nb == nb
    P = rows[-17:]                                          # (the default row among them)
    sub = {x: canopy[x][-17:] for x in CANOPY}
    got = host(run(eng, P, prune=True), SRF7)
    err = worst(got, expected(oracle, tables, P, sub, sensor_tables_of(si)))
    print(nb, {k: f"{v:.2e}" for k, v in err.items()})
    assert all(v.shape == (17, nb) for v in got.values()) and max(err.values()) <= F64, (nb, err)


def test_user_dry_soil_spectra(torch_mod, oracle, tables, rows):
    from spart_amd import get_engine
    P = rows[-9:]
    rng = np.random.default_rng(5)
    rdry = np.linspace(0.05, 0.45, 2001)[None, :] * rng.uniform(0.6, 1.4, (9, 1))
    with np.errstate(all="ignore"):
        full = oracle.spart_run(P, "LANDSAT8-OLI", tables, pso="gl", full=True, rdry=rdry)
    want = expected(oracle, tables, P, full, oracle.sensor_tables(tables, "LANDSAT8-OLI"))
    err = worst(host(run(get_engine("LANDSAT8-OLI", 0), P, rdry=rdry, prune=True), SRF7), want)
    print({k: f"{v:.2e}" for k, v in err.items()})
    assert max(err.values()) <= F64, err


def test_canopy_state_of_the_caller(torch_mod, oracle, tables, rows):
    from spart_amd import get_engine
    P = rows[-9:]
    lidf = oracle.calculate_leafangles(P[:, 16] * 0.5, -P[:, 17])
    with np.errstate(all="ignore"):
        full = oracle.spart_run(P, "Sentinel2A-MSI", tables, pso="gl", full=True, lidf=lidf, nlayers=30)
    want = expected(oracle, tables, P, full, oracle.sensor_tables(tables, "Sentinel2A-MSI"))
    err = worst(host(run(get_engine("Sentinel2A-MSI", 0), P, canopy_lidf=lidf, nlayers=30, prune=True), SRF7), want)
    print({k: f"{v:.2e}" for k, v in err.items()})
    assert max(err.values()) <= F64, err


def test_per_row_thermal_leaf_optics_on_modis(torch_mod, oracle, tables, rows):
    """MODIS has weighted SRF samples in the thermal pad: the thermal evaluation with per-row rho / tau carries weight"""
    from spart_amd import get_engine
    P = rows[-9:]
    rng = np.random.default_rng(6)
    rho, tau = rng.uniform(0.005, 0.1, 9), rng.uniform(0.005, 0.1, 9)
    with np.errstate(all="ignore"):
        full = oracle.spart_run(P, "TerraAqua-MODIS", tables, pso="gl", full=True, rho_thermal=rho, tau_thermal=tau)
        plain = oracle.spart_run(P, "TerraAqua-MODIS", tables, pso="gl", full=True)
    sens = oracle.sensor_tables(tables, "TerraAqua-MODIS")
    want = expected(oracle, tables, P, full, sens)
    assert S.rel_err(want["rso_srf"], expected(oracle, tables, P, plain, sens)["rso_srf"]) > 1e-4     # the case bites
    err = worst(host(run(get_engine("TerraAqua-MODIS", 0), P, rho_thermal=rho, tau_thermal=tau, prune=True), SRF7), want)
    print({k: f"{v:.2e}" for k, v in err.items()})
    assert max(err.values()) <= F64, err


def test_graph_capture_replays_the_srf_columns(torch_mod, s2_base):
    torch = torch_mod
    eng, P, base = s2_base
    Pd = torch.as_tensor(P.T.copy(), device=eng.device)
    out = {k: torch.zeros((P.shape[0], 13), dtype=torch.float64, device=eng.device) for k in list(COLS) + SRF7}
    replay = eng.capture(Pd, "float64", out=out, materialize=SRF7)
    for t in out.values():
        t.zero_()
    replay()
    torch.cuda.synchronize()
    for k in out:
        assert np.array_equal(out[k].cpu().numpy(), base[k], equal_nan=True), k


# ------------------------------------------------------------------ 5. refusals and the Python surface
def raw_call(eng, torch, B, dt, setup):
    from spart_amd import _lib
    td = torch.float64 if dt else torch.float32
    P = torch.ones((27, B), dtype=torch.float64, device=eng.device)
    nb = max(eng.nb, 1)
    outs = [torch.full((B, nb), -7.0, dtype=td, device=eng.device) for _ in range(4)]
    m = _lib.SpartMaterialize()
    setup(m, outs[3])
    n = int(eng.lib.spart_workspace_bytes(eng.ctx, dt, B))
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=eng.device)
    cols = (_lib.vp * 27)(*[P[i].data_ptr() for i in range(27)])
    rc = eng.lib.spart_run_batch(eng.ctx, dt, B, cols, None, None, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                 ctypes.byref(m), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return rc, outs, eng.lib.spart_last_error(eng.ctx).decode()


def test_refusals(torch_mod):
    from spart_amd import get_engine
    torch = torch_mod
    eng = get_engine("Sentinel2A-MSI", 0)

    def f32_columns(m, t):
        m.f32_columns, m.rdd_srf = 1, t.data_ptr()
    rc, outs, msg = raw_call(eng, torch, 5, 0, f32_columns)
    assert rc == -1 and "f32_columns" in msg, (rc, msg)             # SPART_ERR_INVALID
    assert all(bool((t == -7.0).all()) for t in outs)               # nothing was launched
    with pytest.raises(RuntimeError, match="f32_columns"):
        eng.run(torch.ones((27, 5), dtype=torch.float64, device=eng.device), "float32", materialize=["R_TOC_srf"], f32_columns=True)

    def srf_only(m, t):
        m.R_TOC_srf = t.data_ptr()
    rc, outs, msg = raw_call(get_engine(None, 0), torch, 5, 1, srf_only)
    assert rc == -4 and "no sensor" in msg, (rc, msg)               # SPART_ERR_NOSENSOR
    with pytest.raises(ValueError, match="unknown materialize field"):
        eng.run(torch.ones((27, 5), dtype=torch.float64, device=eng.device), "float64", materialize=["R_TOC_SRF"])


def test_band_model_srf_dataframe_and_batch(torch_mod, rows):
    import spart_amd
    from spart_amd import get_engine, workloads
    row = workloads.default_row()[0]
    raw = host(run(get_engine("LANDSAT8-OLI", 0), row), list(COLS) + SRF7)

    def model(r, sensor="LANDSAT8-OLI"):
        leaf, soil, can, ang, atm, doy = r[0:9], r[9:15], r[15:19], r[19:22], r[22:26], r[26]
        return spart_amd.SPART(spart_amd.SoilParameters(*soil), spart_amd.LeafBiology(*leaf[:7], PROT=leaf[7], CBC=leaf[8]),
                               spart_amd.CanopyStructure(*can), spart_amd.AtmosphericProperties(atm[0], atm[1], atm[2], Pa=atm[3]),
                               spart_amd.Angles(*ang), sensor, doy)
    sp = model(row)
    df = sp.run(band_model="srf")
    centre = sp.run()
    for k in COLS:
        assert np.array_equal(df[k].to_numpy(), raw[k + "_srf"][0]) and np.array_equal(centre[k].to_numpy(), raw[k][0]), k
        assert np.array_equal(getattr(sp, k), raw[k][None, 0])                       # (the last run was the centre model)
    assert list(df.columns) == list(centre.columns) and df.index.equals(centre.index)
    with pytest.raises(ValueError, match="band_model"):
        sp.run(band_model="SRF")
    # a batch: arrays in, BatchResult out
    P = rows[:7]
    rawb = host(run(get_engine("LANDSAT8-OLI", 0), P), SRF7)
    res = model(P.T).run(band_model="srf")
    assert set(res) >= set(COLS) and not any(k.endswith("_srf") for k in res)
    for k in COLS:
        assert np.array_equal(np.asarray(res[k]), rawb[k + "_srf"]), k


def test_band_model_srf_on_a_misaligned_sensor(torch_mod):
    import spart_amd
    from spart_amd import get_engine, workloads
    r = workloads.default_row()[0]
    sp = spart_amd.SPART(spart_amd.SoilParameters(*r[9:15]), spart_amd.LeafBiology(*r[0:7], PROT=r[7], CBC=r[8]),
                         spart_amd.CanopyStructure(*r[15:19]), spart_amd.AtmosphericProperties(r[22], r[23], r[24], Pa=r[25]),
                         spart_amd.Angles(*r[19:22]), "TerraAqua-MODIS", r[26])
    eng = get_engine("TerraAqua-MODIS", 0)
    assert eng.srf_aligned.dtype == bool and int(eng.srf_aligned.sum()) == 12 and eng.srf_aligned.shape == (20,)
    assert get_engine("LANDSAT8-OLI", 0).srf_aligned.all()
    with pytest.raises(ValueError, match="align_srf"):
        sp.run(band_model="srf")
    with pytest.raises(ValueError, match="align_srf"):
        spart_amd.generate_lut(r[None, :], "TerraAqua-MODIS", band_model="srf")
    sp.run()                                               # the centre model does not look at the SRFs' order
    mended = spart_amd.align_srf(sp.sensorinfo)
    sp.sensorinfo = mended
    df = sp.run(band_model="srf")
    raw = host(run(get_engine(None, 0, sensor_info=mended), r), SRF7)
    for k in COLS:
        assert np.isfinite(df[k].to_numpy()).all() and np.array_equal(df[k].to_numpy(), raw[k + "_srf"][0]), k


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_generate_lut_band_model_srf(torch_mod, rows, tmp_path, dtype):
    import spart_amd
    from spart_amd import get_engine
    raw = run(get_engine("Sentinel2A-MSI", 0), rows, dtype, prune=True)
    path = str(tmp_path / "lut")
    res = spart_amd.generate_lut(rows, "Sentinel2A-MSI", path=path, dtype=dtype, chunk=32, band_model="srf")    # three chunks
    meta, params, cols = spart_amd.load_lut(path)
    assert meta["band_model"] == "srf" and json.load(open(os.path.join(path, "meta.json")))["columns"] == list(COLS)
    assert np.array_equal(params, rows)
    for k in COLS:
        want = raw[k + "_srf"].cpu().numpy()
        assert cols[k].dtype == want.dtype and np.array_equal(np.asarray(cols[k]), want) and np.array_equal(np.asarray(res[k]), want), k
    centre = spart_amd.generate_lut(rows, "Sentinel2A-MSI", dtype=dtype, chunk=32)
    for k in COLS:
        assert np.array_equal(centre[k], raw[k].cpu().numpy()), k
    spart_amd.generate_lut(rows[:3], "Sentinel2A-MSI", path=str(tmp_path / "c"), dtype=dtype)
    assert spart_amd.load_lut(str(tmp_path / "c"))[0]["band_model"] == "centre"
