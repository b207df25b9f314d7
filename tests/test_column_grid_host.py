"""The reference side of tests/test_gpu_column_grid.py, on a machine without a GPU: the rows of helpers/column_grid.py, the
oracle's columns on them for all nine packaged sensors, and the conditions the GPU tests rely on -- every oracle column is
finite on every row, both sides of k_columns' `b1 == b0` are exercised, columns() is oracle.spart_run, and the g++ build of
csrc/spart_math.h (tests/hostmath, test_hostmath.chain_bands / chain_sensor) holds the 5e-8 float64 contract per sample on
these rows (1.8e-10 measured) and the f32_columns condition of the GPU module (at most 3 entries of a sensor's column above
the bound, the worst at 1.97 x)."""
import numpy as np
import pytest

from helpers import column_grid as C
from helpers import domain_grid as G
from helpers import srf_numpy as S
from test_hostmath import chain_bands, chain_sensor, hm, tab  # noqa: F401  (hm, tab: the fixtures that build and load tests/hostmath)

F64 = 5e-8


@pytest.fixture(scope="module")
def grid(oracle, tables):
    P, kind = C.rows()
    can = C.canopy(oracle, tables, P)
    return P, kind, can


@pytest.fixture(scope="module")
def chains(hm, tab, oracle, tables, grid):  # noqa: F811
    """{(sensor, dtype): (B, nb, 3) R_TOC, R_TOA, L_TOA of the g++ chain}, dtype 1 = float64, 0 = float32; the bands are
    evaluated once per dtype, the sensor step once per sensor"""
    out = {}
    for d in (1, 0):
        bands, atm, _ = chain_bands(hm, tab, grid[0], d)
        out.update({(s, d): chain_sensor(hm, oracle, tables, bands, atm, s)[1] for s in C.SENSORS})
    return out


def test_rows_and_kinds():
    P, kind = C.rows()
    Pg, kg = G.grid_params()
    assert P.shape == (557, 27) and np.array_equal(P[:len(Pg)], Pg) and np.array_equal(kind[:len(kg)], kg)
    assert {k: int((kind == k).sum()) for k in np.unique(kind)} == C.KIND_COUNTS
    assert np.all(kind[-14:] == "atm") and len(np.unique(P[-14:], axis=0)) == 14


def test_every_oracle_column_is_finite_on_every_row(oracle, tables, grid):
    P, kind, can = grid
    for k, v in can.items():
        assert v.shape == (557, 2162) and np.isfinite(v).all(), k
    for sensor in C.SENSORS:
        col = C.columns(oracle, tables, P, can, sensor)
        nb = oracle.sensor_tables(tables, sensor)["coef"].shape[1]
        for k in C.COLS:
            assert col[k].shape == (557, nb) and np.isfinite(col[k]).all(), (sensor, k)


def test_both_sides_of_the_support_point_branch_are_exercised(oracle, tables):
    """k_columns evaluates one support point where the band centre sits on a grid point and two elsewhere"""
    two = {s: int(C.two_support(oracle, tables, s).sum()) for s in C.SENSORS}
    assert two == C.TWO_SUPPORT, two
    nb = {s: oracle.sensor_tables(tables, s)["coef"].shape[1] for s in C.SENSORS}
    assert sorted(set(nb.values())) == [6, 9, 13, 20, 21], nb
    assert any(0 < two[s] < nb[s] for s in C.SENSORS)          # a sensor whose waves meet both kinds of band


def test_columns_are_spart_run(oracle, tables, grid):
    """columns() on the shared canopy against oracle.spart_run itself: 1e-15 on the default sensor, and on one sensor with
    two support points; with the caller's lidf, nlayers, rdry and thermal leaf optics passed through canopy()"""
    P, kind, can = grid
    for sensor in ("Sentinel2A-MSI", "TerraAqua-MODIS"):
        with np.errstate(all="ignore"):
            ref = oracle.spart_run(P, sensor, tables, pso="gl", full=True)
        col = C.columns(oracle, tables, P, can, sensor)
        for k in C.COLS:
            assert S.rel_err(col[k], ref[k]) <= 1e-15, (sensor, k)
    m = np.flatnonzero(kind == "atm")
    rho, tau = G.thermal_draw(len(m), 5)
    kw = dict(lidf=oracle.calculate_leafangles(P[m, 16] * 0.5, -P[m, 17]), nlayers=30, rho_thermal=rho, tau_thermal=tau,
              rdry=np.linspace(0.05, 0.45, 2001)[None, :] * np.linspace(0.6, 1.4, len(m))[:, None])
    with np.errstate(all="ignore"):
        ref = oracle.spart_run(P[m], "TerraAqua-MODIS", tables, pso="gl", full=True, **kw)
    col = C.columns(oracle, tables, P[m], C.canopy(oracle, tables, P[m], block=5, **kw), "TerraAqua-MODIS")
    for k in C.COLS:
        assert S.rel_err(col[k], ref[k]) <= 1e-15, k
    plain = C.columns(oracle, tables, P[m], {k: v[m] for k, v in can.items()}, "TerraAqua-MODIS")
    assert S.rel_err(col["R_TOC"], plain["R_TOC"]) > 1e-3                                             # (the kwargs move the result)


def test_band_subset(oracle, tables):
    """band_subset keeps the named bands, in the order asked for"""
    si = {"wl_smac": np.arange(5.0).reshape(-1, 1), "band_id_smac": list("abcde"),
          "SMAC_coef": {n: np.arange(5.0).reshape(1, -1) + i for i, n in enumerate(oracle.COEF_NAMES)},
          "wl_srf_smac": np.arange(15.0).reshape(3, 5), "p_srf_smac": np.arange(15.0).reshape(3, 5) + 100, "other": 7}
    sub = C.band_subset(si, [4, 1, 2])
    assert sub["band_id_smac"] == ["e", "b", "c"] and sub["other"] == 7 and sub["wl_smac"].shape == (3, 1)
    t, full = C.sensor_tables_of(oracle, sub), C.sensor_tables_of(oracle, si)
    for k in ("wl_smac", "coef", "wl_srf", "p_srf"):
        assert np.array_equal(t[k], full[k][..., [4, 1, 2]]), k
    assert si["wl_smac"].shape == (5, 1) and si["SMAC_coef"][oracle.COEF_NAMES[0]].shape == (1, 5)      # (the input is untouched)


@pytest.mark.parametrize("sensor", C.SENSORS)
def test_float64_chain_per_sample(oracle, tables, grid, chains, sensor):
    """the g++ float64 build of the kernels' arithmetic: <= 5e-8 on |x - ref| / max(|ref|, 1e-6), every row and band"""
    P, kind, can = grid
    col = C.columns(oracle, tables, P, can, sensor)
    toa = chains[sensor, 1]
    for q, k in enumerate(("R_TOC", "R_TOA", "L_TOA")):
        e = C.err(toa[:, :, q], col[k])
        print(C.worst(e, P, kind, f"[host f64] {sensor} {k}:"))
        assert e.max() <= F64, (sensor, k, float(e.max()))


@pytest.fixture(scope="module")
def can32(oracle, grid):
    P, kind, can = grid
    return C.canopy32(oracle, P, can)


@pytest.mark.parametrize("sensor", C.SENSORS)
def test_float32_chain_meets_the_f32_columns_condition(oracle, tables, grid, can32, chains, sensor):
    """the g++ float32 build against max(1e-4, C32 * delta32) on a 1e-2 floor: no entry above 10 x its bound and at most
    0.1 % of a sensor's entries per column above it (measured: at most 3 entries, the worst at 1.97 x)"""
    P, kind, can = grid
    col = C.columns(oracle, tables, P, can, sensor)
    d = C.delta32(oracle, tables, P, can, can32, sensor)
    toa = chains[sensor, 0]
    for q, k in enumerate(("R_TOC", "R_TOA", "L_TOA")):
        x = C.err(toa[:, :, q], col[k], C.FLOOR32) / np.maximum(1e-4, G.C32 * d[k])
        over = np.argwhere(x > 1.0)
        print(C.worst(x, P, kind, f"[host f32, error / bound] {sensor} {k}: {len(over)} over;"))
        assert x.max() <= 10.0 and len(over) <= 1e-3 * x.size, (sensor, k, float(x.max()), over.tolist())
