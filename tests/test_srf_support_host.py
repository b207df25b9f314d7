"""spart_srf_support (the compressed SRF support behind the *_srf columns; a host function: no context, no GPU) against the
literal numpy restatement of calculate_spectral_convolution's index search (helpers/srf_numpy.py), and check_srf / align_srf
on the packaged sensors."""
import ctypes
import os

import numpy as np
import pytest

from helpers import srf_numpy
from helpers.srf_exact import hostile_table

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
# sum_j |E_j| (and the largest |E_j|) of the packaged tables.  Sentinel-2B: 962 with the literal argmin; the definition's exact
# arithmetic sends one wavelength of +9.1e306 (weight 6.9e-310) to the thermal evaluation instead of index 0: one entry more
SUPPORT_SIZES = {"Sentinel2A-MSI": (968, 243), "Sentinel2B-MSI": (963, None), "LANDSAT8-OLI": (1149, 319),
                 "LANDSAT7-ETM": (905, None), "TerraAqua-MODIS": (2014, None), "Sentinel3A-OLCI": (434, None)}
ALIGNED = {"TerraAqua-MODIS": (12, 20), "Sentinel3A-OLCI": (0, 21), "Sentinel3B-OLCI": (0, 21), "LANDSAT4-TM": (6, 6),
           "LANDSAT5-TM": (6, 6), "LANDSAT7-ETM": (6, 6), "LANDSAT8-OLI": (9, 9), "Sentinel2A-MSI": (13, 13),
           "Sentinel2B-MSI": (13, 13)}


@pytest.fixture(scope="module")
def lib():
    from spart_amd import _lib
    return _lib.load()


def library_support(lib, wl_srf, p_srf):
    """the two-call protocol: size query (ev = q = NULL), then the lists"""
    w = np.ascontiguousarray(wl_srf, dtype=np.float64)
    p = np.ascontiguousarray(p_srf, dtype=np.float64)
    nsrf, nb = w.shape
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda a, t: a.ctypes.data_as(t)
    start = np.full(nb + 1, -7, dtype=np.int32)
    assert lib.spart_srf_support(ptr(w, dp), ptr(p, dp), nsrf, nb, ptr(start, ip), None, None, None) == 0
    n = int(start[nb])
    sizes = start.copy()
    ev, q, Q = np.full(n, -7, dtype=np.int32), np.full(n, np.nan), np.full(nb, np.nan)
    assert lib.spart_srf_support(ptr(w, dp), ptr(p, dp), nsrf, nb, ptr(start, ip), ptr(ev, ip), ptr(q, dp), ptr(Q, dp)) == 0
    assert np.array_equal(start, sizes)
    return start, ev, q, Q


def assert_support_equal(got, want):
    for name, g, w in zip(("start", "ev", "q", "Q"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), name               # bit-equal: NaN payloads and signed zeros included


@pytest.mark.parametrize("sensor", ["TerraAqua-MODIS", "LANDSAT4-TM", "LANDSAT5-TM", "LANDSAT7-ETM", "LANDSAT8-OLI",
                                    "Sentinel2A-MSI", "Sentinel2B-MSI", "Sentinel3A-OLCI", "Sentinel3B-OLCI"])
def test_packaged_sensor_support(lib, sensor):
    from spart_amd import tables
    assert sorted(tables.SENSORS) == sorted(ALIGNED)       # every packaged sensor is a case here and below
    si = tables.load_sensor_info(sensor)
    got = library_support(lib, si["wl_srf_smac"], si["p_srf_smac"])
    assert_support_equal(got, srf_numpy.support(si["wl_srf_smac"], si["p_srf_smac"]))
    start, ev = got[0], got[1]
    assert all(np.all(np.diff(ev[a:b]) > 0) and b > a for a, b in zip(start[:-1], start[1:]))     # ascending, distinct, non-empty
    assert ev.min() >= 0 and ev.max() <= srf_numpy.NWL
    if sensor in SUPPORT_SIZES:
        total, largest = SUPPORT_SIZES[sensor]
        assert int(start[-1]) == total
        if largest is not None:
            assert int(np.diff(start).max()) == largest
    literal = np.minimum(srf_numpy.nearest_index_literal(si["wl_srf_smac"]), srf_numpy.NWL)
    n_literal = sum(len(np.unique(literal[:, j])) for j in range(literal.shape[1]))
    assert n_literal == (962 if sensor == "Sentinel2B-MSI" else int(start[-1]))       # the only packaged table where the two differ
    if sensor == "TerraAqua-MODIS":                        # weighted samples in the thermal pad
        w, p = np.asarray(si["wl_srf_smac"], dtype=np.float64), np.asarray(si["p_srf_smac"], dtype=np.float64)
        assert int(((srf_numpy.nearest_index(w) >= srf_numpy.NWL) & (p != 0)).sum()) == 101
        assert (ev == srf_numpy.NWL).any()


def test_hyperspectral_fixture_support(lib):
    z = np.load(os.path.join(ROOT, "tests", "golden", "hyperspectral.npz"))
    got = library_support(lib, z["si/wl_srf"], z["si/p_srf"])
    assert_support_equal(got, srf_numpy.support(z["si/wl_srf"], z["si/p_srf"]))
    assert got[0].shape == (212,) and (got[1] == srf_numpy.NWL).any()      # centres up to 2500 nm reach the thermal pad


def test_hostile_table_support(lib):
    w, p = hostile_table()
    assert np.nanmax(np.abs(w)) < 1e15
    got = library_support(lib, w, p)
    want = srf_numpy.support(w, p)
    assert_support_equal(got, want)
    idx = srf_numpy.nearest_index(w)
    assert np.array_equal(idx, srf_numpy.nearest_index_literal(w))
    assert idx[0, 0] == 0 and idx[16, 0] == 2000 and idx[17, 0] == 2001 and idx[18, 0] == 2001 and idx[19, 0] == 2000   # NaN, 2450 tie
    assert idx[7, 0] == 0 and idx[8, 0] == 1 and idx[10, 0] == 600                     # x.5 ties go down
    assert idx[0, 1] == 2001 and idx[1, 1] == 2002 and idx[13, 1] == 2161 and idx[15, 1] == 0
    start, ev, q, Q = got
    assert list(ev[start[2]:start[3]]) == [0, 465] and q[start[2]] == 0.0               # the zero-weight entry stays
    assert Q[2] == p[21, 2]


def test_exact_arithmetic_beyond_the_literal_argmin(lib):
    """|w| >= 1e15: the library keeps the nearest grid point (documented difference: the literal argmin returns 0)"""
    assert srf_numpy.nearest_index_literal(np.array([[1e300]]))[0, 0] == 0
    w = np.array([[1e15, -1e15, 1e300, np.inf, -np.inf, 3e16]], dtype=np.float64).T.reshape(6, 1)
    start, ev, q, Q = library_support(lib, w, np.ones_like(w))
    assert list(ev) == [0, srf_numpy.NWL] and list(q) == [2.0, 4.0] and Q[0] == 6.0


def test_bad_arguments_are_refused(lib):
    w = np.zeros((2, 2))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    start, ev = np.zeros(3, np.int32), np.zeros(4, np.int32)
    wp = w.ctypes.data_as(dp)
    assert lib.spart_srf_support(None, wp, 2, 2, start.ctypes.data_as(ip), None, None, None) == -1
    assert lib.spart_srf_support(wp, wp, 0, 2, start.ctypes.data_as(ip), None, None, None) == -1
    assert lib.spart_srf_support(wp, wp, 2, 2, None, None, None, None) == -1
    assert lib.spart_srf_support(wp, wp, 2, 2, start.ctypes.data_as(ip), ev.ctypes.data_as(ip), None, None) == -1   # ev without q


def test_convolution_through_the_support_equals_the_literal_form(lib):
    """the re-ordered sum over spart_srf_support's lists (q_e per evaluation, ascending) against gather * p summed over the
    samples, the reference's form: rounding only"""
    from spart_amd import tables
    rng = np.random.default_rng(3)
    x = rng.uniform(0.0, 0.6, (5, srf_numpy.NWLS))
    x[:, srf_numpy.NWL:] = x[:, srf_numpy.NWL:srf_numpy.NWL + 1]          # the thermal pad holds one value
    for sensor in ("Sentinel2A-MSI", "LANDSAT8-OLI", "TerraAqua-MODIS"):
        si = tables.load_sensor_info(sensor)
        lists = library_support(lib, si["wl_srf_smac"], si["p_srf_smac"])
        a = srf_numpy.convolve(x, si["wl_srf_smac"], si["p_srf_smac"], lists=lists)
        b = srf_numpy.convolve_literal(x, si["wl_srf_smac"], si["p_srf_smac"])
        assert srf_numpy.rel_err(a, b) < 1e-12, sensor


@pytest.mark.parametrize("sensor", sorted(ALIGNED))
def test_check_and_align_srf(sensor):
    import spart_amd
    si = spart_amd.load_sensor_info(sensor)
    inside, nb = ALIGNED[sensor]
    ok = spart_amd.check_srf(si)
    assert ok.dtype == bool and ok.shape == (nb,) and int(ok.sum()) == inside
    mended = spart_amd.align_srf(si)
    assert spart_amd.check_srf(mended).all()
    assert mended is not si and mended["SMAC_coef"] is si["SMAC_coef"] and np.array_equal(mended["wl_smac"], si["wl_smac"])
    same = np.array_equal(mended["wl_srf_smac"], np.asarray(si["wl_srf_smac"], dtype=np.float64), equal_nan=True) and \
        np.array_equal(mended["p_srf_smac"], np.asarray(si["p_srf_smac"], dtype=np.float64), equal_nan=True)
    assert same == (inside == nb)                          # the identity exactly on the aligned sensors
    # a permutation of the columns, nothing else
    key = lambda a: sorted(np.nan_to_num(np.asarray(a, dtype=np.float64), nan=-1.0).T.tolist())
    assert key(mended["wl_srf_smac"]) == key(si["wl_srf_smac"])


def test_align_srf_refuses_tables_of_other_bands():
    import spart_amd
    si = dict(spart_amd.load_sensor_info("LANDSAT8-OLI"))
    si["wl_smac"] = np.asarray(si["wl_smac"], dtype=np.float64) + 400.0
    with pytest.raises(ValueError, match="outside"):
        spart_amd.align_srf(si)
