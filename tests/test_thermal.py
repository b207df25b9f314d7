"""The thermal leaf optics LeafBiology.rho_thermal / tau_thermal (prospect_5d.py:82-83; padded over bands 2001..2161 by
set_leaf_refl_trans_assumptions, SPART.py:445-470) and sensor band centres outside 400-2400 nm (np.interp over the 2162-point
grid, SPART.py:219-223), against the REAL reference (tests/golden/thermal.npz, make_golden.py gen_thermal).

CPU: the oracle reproduces the fixture, with per-row thermal values in one call, and with edited band centres; it is then the
reference of the larger GPU tests (tests/test_gpu_thermal.py).  The host logic that turns band centres into support points is
checked in tests/test_hostmath.py.
"""
import os

import numpy as np
import pytest

from conftest import ROOT, rel_err

SENSORS = ("Sentinel2A-MSI", "TerraAqua-MODIS")
GROUPS = ("0", "1", "2", "3", "mixed")
SPECTRA = ("rso", "rdo", "rsd", "rdd")
COLUMNS = ("R_TOC", "R_TOA", "L_TOA", "rsoil")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(ROOT, "tests", "golden", "thermal.npz"))


def edited_tables(tables, fx):
    """the oracle's tables with MODIS' band centres as the fixture's generator set them"""
    t = dict(tables)
    t["TerraAqua-MODIS/wl_smac"] = fx["centres/wl_smac"][:, 0].copy()
    return t


def nan_same(a, b):
    """non-finite exactly where the reference is (rho = tau = 0: the reference's SAILH gives NaN in the thermal bands)"""
    return np.array_equal(~np.isfinite(np.asarray(a, dtype=np.float64)), ~np.isfinite(np.asarray(b, dtype=np.float64)))


def test_fixture_states_what_the_reference_does(fx):
    """what the generator recorded, in its own terms: thermal values reach bands 2001..2161 only, and change no solar band"""
    pi = list(fx["probe_index"])
    th = [pi.index(b) for b in (2001, 2002, 2100, 2161)]
    solar = [pi.index(b) for b in (0, 150, 400, 1000, 1600, 2000)]
    for s in SENSORS:
        for g in GROUPS:
            n = f"run/{g}/{s}"
            rho, tau = fx[n + "/rho_thermal"], fx[n + "/tau_thermal"]
            assert np.array_equal(fx[n + "/leaf_refl"][:, th], np.repeat(rho[:, None], 4, axis=1))
            assert np.array_equal(fx[n + "/leaf_tran"][:, th], np.repeat(tau[:, None], 4, axis=1))
            full = fx[n + "/leafopt_refl_row1"]
            assert full.shape == (2162,) and np.all(full[2001:] == rho[1])
            for k in SPECTRA:
                a = fx[n + "/" + k]
                assert np.array_equal(a[:, solar], fx[f"run/0/{s}/{k}"][:, solar]), (g, k)     # solar bands: untouched
                assert np.array_equal(a[:, th], np.repeat(a[:, th[:1]], 4, axis=1), equal_nan=True)   # the pad is one value
                if g != "0":
                    assert not np.array_equal(a[:, th], fx[f"run/0/{s}/{k}"][:, th], equal_nan=True), (g, k)
    assert np.all(np.isnan(fx["run/1/TerraAqua-MODIS/rso"][:, th]))          # rho = tau = 0
    assert len(set(map(tuple, np.column_stack([fx["run/mixed/Sentinel2A-MSI/rho_thermal"],
                                               fx["run/mixed/Sentinel2A-MSI/tau_thermal"]])))) == 4
    # edited band centres: the first 11 of MODIS' 20, every branch of np.interp
    assert np.array_equal(fx["centres/wl_smac"][:11, 0], fx["edited_centres"])
    assert not np.array_equal(fx["centres/default/R_TOC"], fx["centres/2/R_TOC"])


def _check(o, fx, n, pi):
    for k in COLUMNS:
        assert rel_err(o[k], fx[f"{n}/{k}"], 1e-6) < 1e-8, (n, k)
    for k in SPECTRA:
        assert rel_err(o[k][:, pi], fx[f"{n}/{k}"], 1e-6) < 1e-9, (n, k)
        assert nan_same(o[k][:, pi], fx[f"{n}/{k}"]), (n, k)


def test_oracle_reproduces_thermal_runs(oracle, tables, fx):
    """spart_run(..., rho_thermal=, tau_thermal=, full=True) per group (defaults + 8 LHS rows per (rho, tau) pair; `mixed`: every
    row its own pair) on both sensors: columns <= 1e-8, SAILH spectra <= 1e-9 at the probe bands (2000, 2001, 2002, 2100, 2161 and
    solar ones), NaN exactly where the reference has NaN; the padded leaf optics equal the pair in the thermal bands."""
    P, pi = fx["P"], fx["probe_index"]
    for s in SENSORS:
        for g in GROUPS:
            n = f"run/{g}/{s}"
            rho, tau = fx[n + "/rho_thermal"], fx[n + "/tau_thermal"]
            args = (rho, tau) if g == "mixed" else (float(rho[0]), float(tau[0]))       # per-row arrays / one scalar
            with np.errstate(all="ignore"):
                o = oracle.spart_run(P, s, tables, rho_thermal=args[0], tau_thermal=args[1], full=True)
            _check(o, fx, n, pi)
            r, t = oracle.pad_leaf(o["leaf_refl"], o["leaf_tran"], rho, tau)
            th = pi >= 2001
            assert np.array_equal(r[:, pi][:, th], fx[n + "/leaf_refl"][:, th]) and np.array_equal(t[:, pi][:, th], fx[n + "/leaf_tran"][:, th])
            # solar leaf bands: the reference's QUADPACK E1 carries ~1e-9 (test_full_chain's probe bound)
            assert rel_err(r[:, pi][:, ~th], fx[n + "/leaf_refl"][:, ~th], 0.1) < 1e-6
            assert rel_err(r[1], fx[n + "/leafopt_refl_row1"], 0.1) < 1e-6 and rel_err(t[1], fx[n + "/leafopt_tran_row1"], 0.1) < 1e-6


def test_oracle_per_row_thermal_in_one_call(oracle, tables, fx):
    """every group of the fixture stacked into ONE call with per-row (B,) thermal arrays: the rows do not see each other's
    values (what the GPU tests compare the batched kernels with)"""
    P = fx["P"]
    for s in SENSORS:
        rho = np.concatenate([fx[f"run/{g}/{s}/rho_thermal"] for g in GROUPS])
        tau = np.concatenate([fx[f"run/{g}/{s}/tau_thermal"] for g in GROUPS])
        with np.errstate(all="ignore"):
            o = oracle.spart_run(np.tile(P, (len(GROUPS), 1)), s, tables, rho_thermal=rho, tau_thermal=tau, full=True)
        for j, g in enumerate(GROUPS):
            sl = slice(j * len(P), (j + 1) * len(P))
            _check({k: o[k][sl] for k in COLUMNS + SPECTRA}, fx, f"run/{g}/{s}", fx["probe_index"])


def test_oracle_reproduces_edited_band_centres(oracle, tables, fx):
    """MODIS with centres at 390, 400, 2399.5, 2400, 2450, 2500, 2550, 3000, 20 000, 50 000 and 60 000 nm: below the grid, the
    solar/thermal lerp, thermal points and beyond the grid, with the default and a non-default thermal pair"""
    P = fx["P"][:5]
    t = edited_tables(tables, fx)
    for g in ("default", "2"):
        n = f"centres/{g}"
        with np.errstate(all="ignore"):
            o = oracle.spart_run(P, "TerraAqua-MODIS", t, rho_thermal=fx[n + "/rho_thermal"], tau_thermal=fx[n + "/tau_thermal"],
                                 full=True)
        for k in COLUMNS:
            assert rel_err(o[k], fx[f"{n}/{k}"], 1e-6) < 1e-8, (n, k)
    # the thermal pair moves exactly the bands whose support reaches past 2400 nm
    i0, i1, fr = oracle.interp_weights(fx["centres/wl_smac"][:, 0])
    moved = (i0 >= 2001) | ((i1 >= 2001) & (fr > 0))
    assert list(np.nonzero(moved)[0]) == [4, 5, 6, 7, 8, 9, 10]
    diff = np.any(fx["centres/default/R_TOC"] != fx["centres/2/R_TOC"], axis=0)
    assert np.array_equal(diff, moved)


def test_oracle_black_leaves_limit(oracle, tables, fx):
    """rho = tau = 0: the reference's rinf = (a - m) / sigb is 0/0 (sailh.py:151), NaN in every thermal band of the fixture.  The
    oracle at rho = tau = 1e-200 (sigb^2 underflows: rinf = 0 exactly) is the limit the kernels return there; it is finite and
    continuous with the fixture's own values as rho, tau -> 0 (checked at 1e-7)."""
    P, pi = fx["P"], fx["probe_index"]
    with np.errstate(all="ignore"):
        lim = oracle.spart_run(P, "Sentinel2A-MSI", tables, rho_thermal=1e-200, tau_thermal=1e-200, full=True)
        near = oracle.spart_run(P, "Sentinel2A-MSI", tables, rho_thermal=1e-7, tau_thermal=1e-7, full=True)
    ref = fx["run/1/Sentinel2A-MSI/rso"]
    assert np.isnan(ref[:, pi >= 2001]).all() and np.isfinite(ref[:, pi < 2001]).all()
    for k in SPECTRA:
        assert np.isfinite(lim[k]).all(), k
        assert np.max(np.abs(lim[k][:, 2001:] - near[k][:, 2001:])) < 1e-6, k
        assert rel_err(lim[k][:, pi][:, pi < 2001], fx[f"run/1/Sentinel2A-MSI/{k}"][:, pi < 2001], 1e-6) < 1e-9, k
