"""Hyperspectral sensors (up to SPART_NWLS = 2162 bands) through the forward model on the MI355X: the 211-band sensor of
tests/golden/hyperspectral.npz against the real reference, 2001- and 2162-band sensors against the oracle, the band limit,
and 64-bit (B, nb) offsets."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "hyperspectral.npz")
COLS = ("R_TOC", "R_TOA", "L_TOA")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def hyper():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_hyperspectral import sensorinfo_from_npz
    z = dict(np.load(FIXTURE))
    return z, sensorinfo_from_npz(z)


def synthetic_sensor(centres, fwhm=10.0):
    """a reference-style sensorinfo dict: Gaussian SRFs, SMAC coefficients of the nearest Sentinel-2A band"""
    from spart_amd import tables
    s2 = tables.load_sensor_info("Sentinel2A-MSI")
    c = np.asarray(centres, dtype=np.float64)
    s2c = np.asarray(s2["wl_smac"], dtype=np.float64).reshape(-1)
    near = np.argmin(np.abs(np.minimum(c, 2500.0)[:, None] - s2c[None, :]), axis=1)
    offs = np.arange(-15.0, 16.0, 1.0)
    sig = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
    p = np.exp(-0.5 * (offs[:, None] / sig) ** 2) * np.ones((1, c.size))
    return {"wl_smac": c[:, None], "band_id_smac": [f"H{j}" for j in range(c.size)],
            "SMAC_coef": {n: np.asarray(v, dtype=np.float64).reshape(1, -1)[:, near].copy() for n, v in s2["SMAC_coef"].items()},
            "wl_srf_smac": c[None, :] + offs[:, None], "p_srf_smac": p / p.sum(axis=0, keepdims=True)}


def oracle_tables(tables, name, si):
    from spart_amd import tables as tb
    t = dict(tables)
    t[f"{name}/wl_smac"] = np.asarray(si["wl_smac"], dtype=np.float64).reshape(-1)
    t[f"{name}/coef"] = np.stack([np.asarray(si["SMAC_coef"][n], dtype=np.float64).reshape(-1) for n in tb.COEF_NAMES])
    t[f"{name}/wl_srf"] = np.asarray(si["wl_srf_smac"], dtype=np.float64)
    t[f"{name}/p_srf"] = np.asarray(si["p_srf_smac"], dtype=np.float64)
    return t


def model_grid():
    """the 2162 evaluation wavelengths of the model (SPART.py:303-310): 400..2400 nm, then the thermal grid"""
    return np.concatenate([np.arange(400.0, 2401.0), np.arange(2500.0, 15001.0, 100.0), np.arange(16000.0, 50001.0, 1000.0)])


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-7), ("float32", 1e-4)])
def test_engine_matches_reference_on_211_bands(hyper, torch_mod, dtype, tol):
    from spart_amd import get_engine
    z, si = hyper
    eng = get_engine(None, 0, sensor_info=si)
    assert eng.nb == 211
    out = eng.run(torch_mod.as_tensor(z["P"].T.copy(), device="cuda:0"), dtype)
    for k in COLS:
        assert rel_err(out[k].cpu().numpy(), z[k], 1e-6) <= tol, (k, dtype)


def test_reference_api_with_hyperspectral_sensorinfo(hyper, torch_mod):
    """SPART.SPART(...) with sp.sensorinfo replaced before run(), as a user of the reference does (SPART.py:184, 216, 228, 254)"""
    import SPART
    z, si = hyper
    for i, row in enumerate(z["P"][:4]):
        leaf, soil, can, ang, atm, doy = row[0:9], row[9:15], row[15:19], row[19:22], row[22:26], row[26]
        sp = SPART.SPART(SPART.SoilParameters(*soil), SPART.LeafBiology(*leaf[:7], PROT=leaf[7], CBC=leaf[8]),
                         SPART.CanopyStructure(*can), SPART.AtmosphericProperties(atm[0], atm[1], atm[2], Pa=atm[3]),
                         SPART.Angles(*ang), "Sentinel2A-MSI", int(doy))
        sp.sensorinfo = si
        df = sp.run()
        assert len(df) == 211 and list(df["Band"])[:2] == ["H400", "H410"]
        for k in COLS:
            assert rel_err(df[k].to_numpy(), z[k][i], 1e-6) <= 1e-7, (i, k)


@pytest.mark.parametrize("which", ["nm2001", "grid2162"])
def test_engine_matches_oracle_on_wide_sensors(oracle, tables, torch_mod, which):
    from spart_amd import get_engine, workloads
    centres = np.arange(400.0, 2401.0) if which == "nm2001" else model_grid()
    si = synthetic_sensor(centres)
    P = workloads.lhs_params(512, "full", seed=77)
    ref = oracle.spart_run(P, which, oracle_tables(tables, which, si), pso="gl")
    eng = get_engine(None, 0, sensor_info=si)
    assert eng.nb == centres.size
    out = eng.run(torch_mod.as_tensor(P.T.copy(), device="cuda:0"), "float64")
    for k in COLS:
        assert rel_err(out[k].cpu().numpy(), ref[k], 1e-6) <= 1e-8, (which, k)


def test_context_refuses_2163_bands(torch_mod):
    from spart_amd import _lib
    from spart_amd.engine import Engine
    si = synthetic_sensor(np.concatenate([model_grid(), [50000.0]]))
    with pytest.raises(Exception, match="nb=2163 out of range"):
        Engine(None, 0, sensor_info=si)
    eng = Engine(None, 0, sensor_info=synthetic_sensor(model_grid()))
    assert eng.nb == _lib.NWLS


def test_64bit_offsets_at_2162_bands(torch_mod):
    """B = 1 000 000 rows of 2162 bands (B nb = 2.16e9 > 2^31): the last 64 rows equal the same rows run as a batch of 64"""
    from spart_amd import get_engine, workloads
    torch = torch_mod
    eng = get_engine(None, 0, sensor_info=synthetic_sensor(model_grid()))
    B = 1_000_000
    P = workloads.lhs_params(B, "full", seed=9)
    big = eng.run(torch.as_tensor(P.T.copy(), device="cuda:0"), "float32", prune=True)
    tail = {k: big[k][-64:].clone() for k in COLS}
    del big
    torch.cuda.empty_cache()
    small = eng.run(torch.as_tensor(P[-64:].T.copy(), device="cuda:0"), "float32", prune=True)
    for k in COLS:
        assert torch.equal(torch.nan_to_num(tail[k], nan=7.0), torch.nan_to_num(small[k], nan=7.0)), k
