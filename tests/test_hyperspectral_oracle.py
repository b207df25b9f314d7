"""The 211-band synthetic hyperspectral sensor of tests/golden/hyperspectral.npz (make_hyperspectral.py): the CPU oracle with
that sensorinfo added to its tables reproduces the reference's SPART(...).run() (sp.sensorinfo replaced at call time,
SPART.py:184, 216, 228, 254), thermal-pad centres above 2400 nm included.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import spart_oracle as oracle  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "hyperspectral.npz")


def hyper_tables(z, name="Hyper211"):
    t = dict(oracle.load_tables())
    t[f"{name}/wl_smac"] = np.asarray(z["si/wl_smac"], dtype=np.float64)
    t[f"{name}/coef"] = np.asarray(z["si/coef"], dtype=np.float64)
    t[f"{name}/wl_srf"] = np.asarray(z["si/wl_srf"], dtype=np.float64)
    t[f"{name}/p_srf"] = np.asarray(z["si/p_srf"], dtype=np.float64)
    return t


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(FIXTURE))


def test_fixture_sensor_shape(fixture):
    wl = fixture["si/wl_smac"]
    assert wl.shape == (211,) and wl[0] == 400.0 and wl[-1] == 2500.0
    assert (wl > 2400.0).sum() == 10                   # centres in the thermal padding of the model grid
    assert fixture["si/coef"].shape == (48, 211)
    assert fixture["P"].shape == (16, 27) and fixture["R_TOC"].shape == (16, 211)


def test_oracle_matches_reference_on_211_bands(fixture):
    out = oracle.spart_run(fixture["P"], "Hyper211", tables=hyper_tables(fixture))
    for k in ("R_TOC", "R_TOA", "L_TOA"):
        want, got = fixture[k], out[k]
        assert got.shape == want.shape
        # (the README row's NaN leaf optics at 400-410 nm: at an integer centre next to a NaN grid value np.interp itself
        #  returns NaN -- numpy retries the other interval -- where the oracle, like the engine, reads the one grid point)
        assert not (np.isnan(got) & ~np.isnan(want)).any(), k
        assert np.isnan(want).sum() <= 2 and (np.isnan(want) & ~np.isnan(got)).sum() <= 1, k
        ok = ~np.isnan(want)
        err = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-6)
        assert err.max() <= 1e-7, (k, float(err.max()))
