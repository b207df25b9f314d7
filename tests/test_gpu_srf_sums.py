"""k_columns_srf sum by sum on the MI355X (helpers/srf_exact.py holds the construction; tests/test_srf_exact_host.py proves its
host half without a GPU).

1. A probe sensor of 2002 bands, band e one SRF sample of weight 1 at evaluation e, reads out what the kernel evaluates:
   fma(1, x, 0) / 1 == x, so its rso_srf ... rdd_srf are the kernel's own per-evaluation values X[s, e].  X is held against
   the oracle per sample and per band on the domain grid (helpers/domain_grid.py, 543 rows at and past the domain's edges,
   per-row thermal rho / tau) at the float64 band kernels' tolerance, and against k_bands<double>'s spectra of the same call.
2. Every sensor's band sum must then be srf_chain(X, support): the chain of correctly rounded FMAs from 0 over the band's
   entries in ascending order and one IEEE division that include/spart_hip.h defines -- BIT FOR BIT, every row, every band:
   the nine packaged sensors with their literal tables, the 211-band fixture sensor, and a 7-band sensor built for the
   dealing and for hostile weights (helpers/srf_exact.dealing_sensor).
3. The tail: R_TOC_srf / R_TOA_srf / L_TOA_srf against the oracle's SMAC and TOC -> TOA of the kernel's own four *_srf columns.

Rows: the grid and one appended row with Cab = NaN (544: nine sample blocks, the last of 32 rows).  The NaN pigment makes
every optical evaluation 0..2000 NaN; the thermal evaluation takes the row's rho_thermal / tau_thermal in place of the leaf
model (SPART.py:463-466), does not read Cab and stays finite, here as in the oracle.

Dealing: srf_deal sorts the bands by support size, so the dealing sensor's workgroups are [long (2002 entries), hostile,
plus_minus, zero_weight] and [one_700, one_thermal, one_1650, idle wave]; the probe's 2002 bands are 501 workgroups in
grid.y, the last with two idle waves.  No column of the dealing sensor's table is refused by context creation.
"""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import domain_grid as G
from helpers import srf_exact as E
from helpers import srf_numpy as S

pytestmark = pytest.mark.gpu

SENSORS = ["TerraAqua-MODIS", "LANDSAT4-TM", "LANDSAT5-TM", "LANDSAT7-ETM", "LANDSAT8-OLI", "Sentinel2A-MSI", "Sentinel2B-MSI",
           "Sentinel3A-OLCI", "Sentinel3B-OLCI"]
CANOPY = ("rso", "rdo", "rsd", "rdd")
CANOPY_SRF = tuple(x + "_srf" for x in CANOPY)
TAIL = ("R_TOC_srf", "R_TOA_srf", "L_TOA_srf")
ORACLE = (1e-7, 1e-3)           # test_gpu_band_sums.F64: bound and floor of the float64 band kernels against the oracle
F64 = 1e-8                      # test_gpu_srf_columns.F64, metric srf_numpy.rel_err


@pytest.fixture(scope="module")
def grid(oracle, tables):
    return G.build_grid(oracle, tables)


@pytest.fixture(scope="module")
def rows(grid):
    """(P (544, 27), rho (544,), tau (544,)): the grid and the Cab = NaN row"""
    from spart_amd_workloads import default_row
    P = np.concatenate([grid["P"], default_row(Cab=float("nan"))], axis=0)
    assert P.shape == (544, 27) and len(grid["P"]) == 543
    return P, np.append(grid["rho"], 0.1), np.append(grid["tau"], 0.05)


def call(si, rows, fields, dtype="float64"):
    """one pruned call of the sensor on the 544 rows -> {field: numpy}"""
    import torch
    from spart_amd import get_engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    P, rho, tau = rows
    eng = get_engine(si, 0) if isinstance(si, str) else get_engine(None, 0, sensor_info=si)
    res = eng.run(torch.as_tensor(P.T.copy(), device=eng.device), dtype, rho_thermal=rho, tau_thermal=tau, materialize=list(fields),
                  prune=True)
    torch.cuda.synchronize()
    return {k: res[k].cpu().numpy() for k in fields}


@pytest.fixture(scope="module")
def probe(rows):
    """the probe once: X = {rso ... rdd: (544, 2002)} and, from the same call, k_bands<double>'s spectra (544, 2162)"""
    got = call(E.probe_sensor(), rows, CANOPY_SRF + CANOPY)
    X = {x: got[x + "_srf"] for x in CANOPY}
    assert all(v.shape == (544, E.NEV) and v.dtype == np.float64 for v in X.values())
    return X, {x: got[x] for x in CANOPY}


_RUNS = {}


def sensor_run(name, rows):
    """the seven *_srf outputs of a packaged sensor on the 544 rows (literal tables), float64, once per module"""
    if name not in _RUNS:
        _RUNS[name] = call(name, rows, CANOPY_SRF + TAIL)
    return _RUNS[name]


def ulp_distance(a, b):
    """|a - b| in units in the last place, on the finite elements of both (ordered-integer view of the doubles)"""
    def ordered(x):
        i = x.view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    ok = np.isfinite(a) & np.isfinite(b) & (a != b)        # (Python integers: no overflow between values of opposite sign)
    return [abs(int(u) - int(v)) for u, v in zip(ordered(a[ok]), ordered(b[ok]))]


def assert_sums_equal_chain(tag, got, X, lists):
    """got[x_srf] == srf_chain(X[x], lists) in bits (NaN where the chain has NaN, infinities with their sign)"""
    for x in CANOPY:
        want, _, n = E.srf_chain(X[x], lists)
        g = got[x + "_srf"]
        assert g.shape == want.shape and g.dtype == np.float64, (tag, x, g.shape, g.dtype)
        if not np.array_equal(g, want, equal_nan=True):
            bad = np.argwhere(~((g == want) | (np.isnan(g) & np.isnan(want))))
            r, j = bad[0]
            print(tag, x, "elements differing:", len(bad), "of", g.size)
            pytest.fail(f"{tag} {x}_srf: row {r} band {j}: kernel {g[r, j]!r} chain {want[r, j]!r} n_j {n[j]} ({len(bad)} elements differ)")


# ------------------------------------------------------------------ a. the evaluations against the oracle
def test_evaluations_per_sample_vs_oracle(grid, probe):
    """X[:543] against the oracle's rso, rdo, rsd, rdd at evaluations 0..2001: 1e-7 on a 1e-3 floor, the bound of
    test_gpu_band_sums.test_float64_per_sample_vs_oracle for the same arithmetic in k_bands<double>.
    Measured worst error on one MI355X: see DESIGN.md section 14."""
    X, _ = probe
    tol, fl = ORACLE
    worst = {}
    for k in CANOPY:
        got = X[k][:543]
        assert np.isfinite(got).all(), (k, np.argwhere(~np.isfinite(got))[:3])
        err = np.abs(got - grid[k]) / np.maximum(np.abs(grid[k]), fl)
        r, b = np.unravel_index(np.argmax(err), err.shape)
        worst[k] = (float(err[r, b]), int(r), str(grid["kind"][r]), "band", int(b))
    print("worst |X - oracle| / max(|oracle|, 1e-3):", {k: "%.3g" % v[0] for k, v in worst.items()})
    for k in CANOPY:
        assert worst[k][0] < tol, (k,) + worst[k]


def test_nan_pigment_row(oracle, tables, rows, probe):
    """Cab = NaN: every optical evaluation 0..2000 is NaN; the thermal evaluation reads rho_thermal / tau_thermal instead of
    the leaf model and equals the oracle's"""
    X, _ = probe
    P, rho, tau = rows
    with np.errstate(all="ignore"):
        o = oracle.spart_run(P[543:], "Sentinel2A-MSI", tables, pso="gl", full=True, rho_thermal=rho[543:], tau_thermal=tau[543:])
    for k in CANOPY:
        assert np.isnan(X[k][543, :S.NWL]).all(), (k, np.flatnonzero(~np.isnan(X[k][543, :S.NWL]))[:5])
        ref = o[k][0, S.NWL]
        assert np.isfinite(ref) and abs(X[k][543, S.NWL] - ref) / max(abs(ref), ORACLE[1]) < ORACLE[0], (k, X[k][543, S.NWL], ref)


# ------------------------------------------------------------------ b. the evaluations against k_bands<double>
def test_evaluations_vs_materialised_spectra(probe):
    """X[:, e] against rso ... rdd[:, e] of the same call (k_bands<double, 1, 1>), all 544 rows, at the float64 contract.
    Recorded, not asserted: how many elements differ in bits and by how many ulp."""
    X, spectra = probe
    for k in CANOPY:
        a, b = X[k], spectra[k][:, :E.NEV]
        assert spectra[k].shape == (544, S.NWLS)
        assert np.array_equal(spectra[k][:, E.NEV:], np.repeat(b[:, -1:], S.NWLS - E.NEV, axis=1), equal_nan=True), k
        d = ulp_distance(a, b)
        differ = int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))
        err = S.rel_err(a, b)
        print(k, "elements differing in bits: %d of %d, worst distance %s ulp, rel_err %.3g" % (differ, a.size, max(d, default=0), err))
        assert err <= F64, (k, err)


# ------------------------------------------------------------------ c. sum by sum, the packaged sensors
@pytest.mark.parametrize("sensor", SENSORS)
def test_band_sums_equal_the_fma_chain(rows, probe, sensor):
    """literal tables (MODIS and OLCI in the packaged order)"""
    from spart_amd import tables as tb
    si = tb.load_sensor_info(sensor)
    w, p = np.asarray(si["wl_srf_smac"], dtype=np.float64), np.asarray(si["p_srf_smac"], dtype=np.float64)
    lists = S.support(w, p)
    start, ev, q, Q = lists
    if sensor in ("LANDSAT7-ETM", "LANDSAT8-OLI"):
        assert (p < 0).any() and (q < 0).any()                                    # negative weights
    if sensor == "TerraAqua-MODIS":
        assert ((ev == S.NWL) & (q != 0)).any()                                   # weight in the thermal pad
    if sensor == "Sentinel2B-MSI":
        assert (w > 9e306).sum() == 1 and ev[start[5] - 1] == S.NWL and 0 < q[start[5] - 1] < 1e-309    # the +9.1e306 nm sample, band 4
    assert_sums_equal_chain(sensor, sensor_run(sensor, rows), probe[0], lists)


# ------------------------------------------------------------------ d. the 211-band fixture sensor
def test_band_sums_of_the_hyperspectral_fixture(rows, probe):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_hyperspectral import sensorinfo_from_npz
    si = sensorinfo_from_npz(dict(np.load(os.path.join(ROOT, "tests", "golden", "hyperspectral.npz"))))
    lists = S.support(si["wl_srf_smac"], si["p_srf_smac"])
    assert len(lists[3]) == 211 and (lists[1] == S.NWL).any()
    assert_sums_equal_chain("hyperspectral", call(si, rows, CANOPY_SRF), probe[0], lists)


# ------------------------------------------------------------------ e. dealing and hostile weights
def test_dealing_and_hostile_weights(rows, probe):
    """helpers/srf_exact.dealing_sensor: 2002 entries beside 2 in one workgroup, one-entry bands (one of them the thermal
    evaluation alone) in a group with an idle wave, Q = 0, a zero-weight entry, NaN and infinite weights.  Only the canopy
    columns: this sensor's econv may be 0 / 0.  (tests/test_srf_exact_host.py asserts the supports.)"""
    si = E.dealing_sensor()
    lists = S.support(si["wl_srf_smac"], si["p_srf_smac"])
    got = call(si, rows, CANOPY_SRF)
    X = probe[0]
    assert_sums_equal_chain("dealing", got, X, lists)
    j = {name: i for i, name in enumerate(E.DEAL_BANDS)}
    for x in CANOPY:
        g = got[x + "_srf"]
        assert np.array_equal(g[:, j["one_700"]], X[x][:, 300], equal_nan=True) and np.array_equal(g[:, j["one_thermal"]], X[x][:, S.NWL])
        assert np.isfinite(g[:543, j["long"]]).all() and np.isnan(g[543, j["long"]])
        z = g[:, j["zero_weight"]]
        assert np.isnan(z[543]) and np.isfinite(z[:543]).all() and np.array_equal(z[:543], X[x][:543, 465])   # 0 * NaN is NaN
        pm = g[:543, j["plus_minus"]]                       # (x[600 nm] - x[601 nm]) / 0: signed infinities, NaN where equal
        d = X[x][:543, 200] - X[x][:543, 201]
        assert np.array_equal(np.isnan(pm), d == 0) and np.array_equal(pm[d != 0], np.where(d[d != 0] > 0, np.inf, -np.inf))
        assert (d > 0).any() and (d < 0).any() and np.isnan(g[:, j["hostile"]]).all()


# ------------------------------------------------------------------ f. the tail
@pytest.mark.parametrize("sensor", SENSORS)
def test_tail_vs_oracle_smac_of_the_kernels_own_columns(oracle, tables, rows, sensor):
    """R_TOC_srf, R_TOA_srf, L_TOA_srf of the 543 finite rows against srf_numpy.toc_to_toa(oracle.smac, the kernel's own
    rso_srf ... rdd_srf, La): only SMAC and TOC -> TOA are in the difference -- the aot550 = 0, uh2o = uo3 = 0 and Pa = 500
    rows of the grid among them"""
    P = rows[0][:543]
    assert (P[:, 22] == 0).any() and ((P[:, 23] == 0) & (P[:, 24] == 0)).any() and (P[:, 25] == 500).any()
    got = {k: v[:543] for k, v in sensor_run(sensor, rows).items()}
    sens = oracle.sensor_tables(tables, sensor)
    with np.errstate(all="ignore"):
        at = oracle.smac(P[:, 19:22], P[:, 22:26], sens)
        La = (oracle.et_correction(P[:, 26]) * np.cos(P[:, 19] * np.pi / 180) / np.pi)[:, None] * oracle.et_convolution(tables, sens)[None, :]
    want = dict(zip(TAIL, S.toc_to_toa(at, got["rso_srf"], got["rdo_srf"], got["rsd_srf"], got["rdd_srf"], La)))
    err = {k: S.rel_err(got[k], want[k]) for k in TAIL}
    print(sensor, {k: "%.2e" % v for k, v in err.items()})
    assert max(err.values()) <= F64, (sensor, err)


# ------------------------------------------------------------------ g. float32 outputs
def test_float32_outputs_are_the_float64_ones_rounded_once(rows):
    f64 = sensor_run("Sentinel2A-MSI", rows)
    f32 = call("Sentinel2A-MSI", rows, CANOPY_SRF + TAIL, "float32")
    for k in CANOPY_SRF + TAIL:
        assert f32[k].dtype == np.float32 and np.array_equal(f32[k], f64[k].astype(np.float32), equal_nan=True), k
