"""The sensor columns per sample: R_TOC, R_TOA, L_TOA and the materialised rsoil and La of k_prelude -> k_columns on the 557
rows of tests/helpers/column_grid.py (the domain grid of the band tests plus 14 atmosphere / geometry / date rows), for all
nine packaged sensors, against the float64 oracle's columns assembled by column_grid.columns from ONE oracle canopy run.
tests/test_column_grid_host.py pins that reference and holds the g++ build of the same arithmetic to the same bounds.

Metric: |x - ref| / max(|ref|, 1e-6) per entry (floor 1e-2 in the f32_columns leg); a non-finite GPU value counts as inf.

  a  float64 per sample against the oracle, five columns, nine sensors                          bound 5e-8
  b  prune, f32_bands, float32 (= float64 rounded once), reversed batch, rows alone             bit for bit
  c  sub-sensors of 1, 2, 3, 5 bands (Landsat 8, MODIS) against the full sensor's columns       bit for bit
  d  the caller's canopy.lidf (LIDFa / LIDFb NULL) and nlayers = 30 against the oracle          bound 5e-8
  e  fast_prelude against the default float64 columns: include/spart_hip.h's statement          1e-4, 1e-6 where |ref| >= 1e-3
  f  f32_columns against the oracle: max(1e-4, C32 * delta32), floor 1e-2                       <= 10 x, <= 0.1 % above 1 x
  g  user dry-soil spectra and per-row thermal leaf optics, Landsat 7 and MODIS                 bound 5e-8

No packaged sensor has a band centre past 2400 nm, so leg g adds MODIS with the centres of tests/golden/thermal.npz: the
only case here whose columns see the thermal leaf optics (k_columns' `thermal ?` selects).

Measured on one MI355X (the 50 cases run in 5.0 s, their oracle included), worst entry per leg against its bound:
  a  1.7e-10 / 5e-8 (R_TOA and L_TOA, Sentinel-2A band 8, an ota_pro row); R_TOC 3.6e-11, rsoil 2.8e-11, La 2.5e-15
  b, c  every comparison bit-identical
  d  lidf_in with NULL LIDFa / LIDFb 1.8e-11 / 5e-8 (OLCI band 14, a corner_pro row); nlayers = 30 1.3e-10 / 5e-8
  e  inside the LHS ranges and atm rows 7.5e-7 / 1e-4 (Sentinel-2A R_TOA band 8) and, where |ref| >= 1e-3, 1.1e-7 / 1e-6;
     outside (past, golden) 5.2e-7 / 1e-4 (MODIS R_TOC band 10, a past row); against the oracle 7.5e-7
  f  error / bound at most 0.85 for R_TOA and L_TOA with no entry above its bound; R_TOC 2.67 x at the worst (limit 10 x) with
     4 of Sentinel-2B's 7241 entries above their bound (limit 7), all in band 7 on ota_pro rows, errors 1.0e-4 ... 5.5e-4;
     the eight other sensors have none.  The g++ build of the same arithmetic (tests/test_column_grid_host.py): 3, 1.97 x
  g  8.6e-12 / 5e-8 (MODIS R_TOC), the moved centres included
"""
import numpy as np
import pytest

from helpers import column_grid as C
from helpers import domain_grid as G

pytestmark = pytest.mark.gpu

F64 = 5e-8
MAIN = ("R_TOC", "R_TOA", "L_TOA")
SUBSETS = {"LANDSAT8-OLI": ([4], [8, 1], [0, 3, 7], [8, 6, 5, 2, 1]),
           "TerraAqua-MODIS": ([17], [19, 6], [2, 9, 16], [18, 12, 7, 3, 0])}


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def grid(oracle, tables):
    """(P, kind, the oracle's canopy) of the 557 rows"""
    P, kind = C.rows()
    return P, kind, C.canopy(oracle, tables, P)


def run(eng, P, dtype="float64", **kw):
    """the five columns of one call, as float64 numpy (exact for float32 outputs); P (B, 27) or a list of 27 columns"""
    import torch
    params = P if isinstance(P, list) else torch.as_tensor(np.atleast_2d(P).T.copy(), device=eng.device)
    res = eng.run(params, dtype, materialize=("rsoil", "La"), **kw)
    torch.cuda.synchronize()
    return {k: res[k].double().cpu().numpy() for k in C.COLS}


@pytest.fixture(scope="module")
def base(torch_mod, oracle, tables, grid):
    """base(sensor) -> (engine, the oracle's columns, the float64 columns of the 557 rows, their error against the oracle),
    computed once per sensor"""
    from spart_amd import get_engine
    P, kind, can = grid
    cache = {}

    def get(sensor):
        if sensor not in cache:
            eng = get_engine(sensor, 0)
            want = C.columns(oracle, tables, P, can, sensor)
            got = run(eng, P)
            cache[sensor] = eng, want, got, {k: C.err(got[k], want[k]) for k in C.COLS}
        return cache[sensor]
    return get


def check(got, want, P, kind, tol, tag, keys=C.COLS):
    for k in keys:
        e = C.err(got[k], want[k])
        print(C.worst(e, P, kind, f"[{tag}] {k}:"))
        assert got[k].shape == want[k].shape and e.max() <= tol, (tag, k, C.worst(e, P, kind))


def same(a, b, tag, keys=C.COLS):
    for k in keys:
        bad = np.argwhere(~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))))
        assert a[k].shape == b[k].shape and len(bad) == 0, (tag, k, len(bad), "entries differ; first (row, band)", bad[:4].tolist())


# ------------------------------------------------------------------ a. float64 per sample against the oracle
@pytest.mark.parametrize("sensor", C.SENSORS)
def test_float64_columns_per_sample(base, grid, sensor):
    """every entry of the five columns <= 5e-8 (the gap between the oracle's closed-form E1 and the kernels' series, the bound
    test_parity_at_scale_against_the_oracle holds); finite wherever the oracle is, which is everywhere"""
    P, kind, _ = grid
    eng, want, got, err = base(sensor)
    assert all(np.isfinite(want[k]).all() for k in C.COLS)
    for k in C.COLS:
        print(C.worst(err[k], P, kind, f"[a float64] {sensor} {k}:"))
    for k in C.COLS:
        assert got[k].shape == want[k].shape == (len(P), eng.nb) and np.isfinite(got[k]).all(), (sensor, k)
        assert err[k].max() <= F64, (sensor, k, C.worst(err[k], P, kind))


# ------------------------------------------------------------------ b. the modes are the same numbers
@pytest.mark.parametrize("sensor", C.SENSORS)
def test_modes_are_the_same_numbers(base, grid, sensor):
    """prune, f32_bands, the default float32 mode (the float64 columns rounded once), the reversed batch, and the 8 rows with
    the largest error of (a) evaluated alone: bit for bit"""
    P, kind, _ = grid
    eng, want, got, err = base(sensor)
    same(run(eng, P, prune=True), got, (sensor, "prune"))
    same(run(eng, P, f32_bands=True), got, (sensor, "f32_bands"))
    rounded = {k: got[k].astype(np.float32).astype(np.float64) for k in C.COLS}
    same(run(eng, P, "float32"), rounded, (sensor, "float32"))
    same(run(eng, P, "float32", prune=True), rounded, (sensor, "float32 pruned"))
    same(run(eng, P[::-1]), {k: got[k][::-1] for k in C.COLS}, (sensor, "reversed"))
    row_err = np.max([err[k].max(axis=1) for k in C.COLS], axis=0)
    for r in np.argsort(-row_err, kind="stable")[:8]:
        same(run(eng, P[r:r + 1]), {k: got[k][r:r + 1] for k in C.COLS}, (sensor, "row alone", int(r), str(kind[r])))


# ------------------------------------------------------------------ c. fewer bands than waves, band independence
@pytest.mark.parametrize("sensor", sorted(SUBSETS))
def test_sub_sensors_give_the_full_sensors_columns(base, grid, sensor):
    """sensors of 1, 2, 3 and 5 bands (k_columns has four waves; a non-contiguous and a descending index set among them):
    each column is bit-identical to that band's column of the full sensor, on the first and the last 70 rows"""
    from spart_amd import get_engine, tables as tb
    P, kind, _ = grid
    _, _, got, _ = base(sensor)
    rows = np.r_[0:70, len(P) - 70:len(P)]
    si = tb.load_sensor_info(sensor)
    assert [len(i) for i in SUBSETS[sensor]] == [1, 2, 3, 5]
    for idx in SUBSETS[sensor]:
        eng = get_engine(None, 0, sensor_info=C.band_subset(si, idx))
        assert eng.nb == len(idx)
        same(run(eng, P[rows]), {k: got[k][rows][:, idx] for k in C.COLS}, (sensor, idx))


# ------------------------------------------------------------------ d. the caller's canopy state
@pytest.fixture(scope="module")
def state_refs(oracle, tables, grid):
    """the oracle's canopy (1) with lidf = calculate_leafangles of each row's own LIDFa / LIDFb on the corner, past and atm
    rows, (2) with nlayers = 30 on every row"""
    P, kind, _ = grid
    m = np.flatnonzero(np.isin(kind, ("corner_full", "corner_pro", "past", "atm")))
    lidf = oracle.calculate_leafangles(P[m, 16], P[m, 17])
    return m, lidf, C.canopy(oracle, tables, P[m], lidf=lidf), C.canopy(oracle, tables, P, nlayers=30)


def run_with_lidf_only(eng, P, lidf):
    """spart_run_batch itself, float64, with lidf_in given and the LIDFa / LIDFb column pointers NULL (Engine.run would hand
    the library columns of zeros in their place).  The call is marshalled as Engine.run does it (spart_amd/engine.py, the end
    of run(): workspace, SpartMaterialize, argument order); a change of spart_run_batch's signature is mirrored here."""
    import ctypes
    import torch
    from spart_amd import _lib
    B = len(P)
    Pd = torch.as_tensor(P.T.copy(), device=eng.device)
    li = torch.as_tensor(np.ascontiguousarray(lidf, dtype=np.float64), device=eng.device)
    assert tuple(li.shape) == (B, 13)
    out = {k: torch.full((B, eng.nb), float("nan"), dtype=torch.float64, device=eng.device) for k in C.COLS}
    m = _lib.SpartMaterialize()
    m.lidf_in, m.rsoil, m.La = li.data_ptr(), out["rsoil"].data_ptr(), out["La"].data_ptr()
    n = int(eng.lib.spart_workspace_bytes(eng.ctx, _lib.SPART_F64, B))
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=eng.device)
    cols = (_lib.vp * 27)(*[None if i in (16, 17) else Pd[i].data_ptr() for i in range(27)])
    rc = eng.lib.spart_run_batch(eng.ctx, _lib.SPART_F64, B, cols, None, None, out["R_TOC"].data_ptr(), out["R_TOA"].data_ptr(),
                                 out["L_TOA"].data_ptr(), ctypes.byref(m), ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, eng.lib.spart_last_error(eng.ctx).decode())
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("sensor", C.SENSORS)
def test_callers_lidf_and_nlayers(base, grid, state_refs, oracle, tables, sensor):
    """k_prelude<false, true> without its LIDF iteration (lidf_in given, the LIDFa / LIDFb pointers NULL) and with it
    (nlayers = 30), each against the oracle given the same state"""
    P, kind, can = grid
    eng = base(sensor)[0]
    m, lidf, can_lidf, can_nl = state_refs
    assert len(m) == 128 + 128 + 72 + 14
    check(run_with_lidf_only(eng, P[m], lidf), C.columns(oracle, tables, P[m], can_lidf, sensor), P[m], kind[m], F64, f"d lidf_in {sensor}")
    want = C.columns(oracle, tables, P, can_nl, sensor)
    assert C.err(want["R_TOC"], C.columns(oracle, tables, P, can, sensor)["R_TOC"]).max() > 1e-5      # (nlayers moves the result)
    check(run(eng, P, nlayers=30), want, P, kind, F64, f"d nlayers=30 {sensor}")


# ------------------------------------------------------------------ e. fast_prelude
@pytest.mark.parametrize("sensor", C.SENSORS)
def test_fast_prelude_keeps_the_headers_statement(base, grid, sensor):
    """lidf="newton" (k_prelude<true>) against the default float64 columns, as include/spart_hip.h states it: within 1e-4
    everywhere and within 1e-6 wherever the value is at least 1e-3 -- held exactly on the rows inside the LHS ranges and the
    atm rows; the rows outside them (past, golden) are held to 1e-4"""
    P, kind, _ = grid
    eng, want, got, _ = base(sensor)
    new = run(eng, P, lidf="newton")
    inside = np.isin(kind, G.INSIDE + ("atm",))
    assert inside.sum() == 128 + 128 + 44 + 46 + 14
    for k in MAIN:
        e = C.err(new[k], got[k])
        big = np.abs(got[k]) >= 1e-3
        print(C.worst(e[inside], P[inside], kind[inside], f"[e fast_prelude, inside] {sensor} {k}:"))
        print(C.worst(np.where(big, e, 0.0)[inside], P[inside], kind[inside], f"[e fast_prelude, inside, |ref| >= 1e-3] {sensor} {k}:"))
        print(C.worst(e[~inside], P[~inside], kind[~inside], f"[e fast_prelude, outside] {sensor} {k}:"))
        print(C.worst(C.err(new[k], want[k]), P, kind, f"[e fast_prelude, against the oracle] {sensor} {k}:"))
        assert e[inside].max() <= 1e-4, (sensor, k, C.worst(e[inside], P[inside], kind[inside]))
        assert np.where(big, e, 0.0)[inside].max() <= 1e-6, (sensor, k, C.worst(np.where(big, e, 0.0)[inside], P[inside], kind[inside]))
        assert e[~inside].max() <= 1e-4, (sensor, k, C.worst(e[~inside], P[~inside], kind[~inside]))


# ------------------------------------------------------------------ f. f32_columns
@pytest.fixture(scope="module")
def can32(oracle, grid):
    P, _, can = grid
    return C.canopy32(oracle, P, can)


@pytest.mark.parametrize("sensor", C.SENSORS)
def test_f32_columns_within_the_conditioning_bound(base, grid, can32, oracle, tables, sensor):
    """k_columns<float, float, float> against the oracle on a 1e-2 floor; per-entry bound max(1e-4, C32 * delta32), from the
    oracle alone.  No entry above 10 x its bound, at most 0.1 % of a sensor's entries per column above it; every offending
    entry is printed (the g++ build of the same arithmetic: at most 3, the worst at 1.97 x)"""
    P, kind, can = grid
    eng, want, _, _ = base(sensor)
    d = C.delta32(oracle, tables, P, can, can32, sensor)
    got = run(eng, P, "float32", f32_columns=True)
    for k in MAIN:
        bound = np.maximum(1e-4, G.C32 * d[k])
        e = C.err(got[k], want[k], C.FLOOR32)
        x = e / bound
        over = np.argwhere(x > 1.0)
        print(C.worst(x, P, kind, f"[f f32_columns, error / bound] {sensor} {k}: {len(over)} of {x.size} over;"))
        print(C.worst(e, P, kind, f"[f f32_columns, error] {sensor} {k}:"))
        for r, b in over:
            print(f"    over: row {r} kind {kind[r]} band {b} err {e[r, b]:.3e} bound {bound[r, b]:.3e} ref {want[k][r, b]:.6e}")
        assert x.max() <= 10.0, (sensor, k, C.worst(x, P, kind))
        assert len(over) <= 1e-3 * x.size, (sensor, k, len(over), x.size)


# ------------------------------------------------------------------ g. user dry-soil spectra, per-row thermal leaf optics
MOVED = "TerraAqua-MODIS, centres moved"


@pytest.mark.parametrize("sensor", ["LANDSAT7-ETM", "TerraAqua-MODIS", MOVED])
def test_user_dry_soil_and_thermal_leaf_optics(torch_mod, grid, oracle, tables, sensor):
    """the 256 corner rows with rdry (the rdry_in read inside k_columns) and per-row rho_thermal / tau_thermal.  No packaged
    sensor has a band centre past 2400 nm, so their columns do not see the thermal leaf optics; the third case is MODIS with
    the centres of tests/golden/thermal.npz (390 ... 60 000 nm: 7 bands whose support reaches the thermal evaluation, the
    `thermal ?` selects of k_columns), which tests/test_gpu_thermal.py runs on Latin-hypercube rows"""
    import os
    from conftest import ROOT
    from spart_amd import get_engine, tables as tb
    P, kind, can = grid
    if sensor == MOVED:
        si = dict(tb.load_sensor_info("TerraAqua-MODIS"))
        si["wl_smac"] = np.load(os.path.join(ROOT, "tests", "golden", "thermal.npz"))["centres/wl_smac"].copy()
        eng, sens = get_engine(None, 0, sensor_info=si), C.sensor_tables_of(oracle, si)
    else:
        eng, sens = get_engine(sensor, 0), oracle.sensor_tables(tables, sensor)
    m = np.flatnonzero(np.isin(kind, ("corner_full", "corner_pro")))
    assert len(m) == 256
    rdry = np.linspace(0.05, 0.45, 2001)[None, :] * np.random.default_rng(5).uniform(0.6, 1.4, (len(m), 1))
    rho, tau = G.thermal_draw(len(m), 74)
    want = C.columns(oracle, tables, P[m], C.canopy(oracle, tables, P[m], rdry=rdry, rho_thermal=rho, tau_thermal=tau), sens)
    plain = C.columns(oracle, tables, P[m], {k: v[m] for k, v in can.items()}, sens)
    assert C.err(want["rsoil"], plain["rsoil"]).max() > 1e-2                                           # (the case bites)
    only_rdry = C.columns(oracle, tables, P[m], C.canopy(oracle, tables, P[m], rdry=rdry), sens)
    moved = np.any(C.err(want["R_TOC"], only_rdry["R_TOC"]) > 1e-2, axis=0)                            # bands the thermal optics move
    assert moved.sum() == (7 if sensor == MOVED else 0), moved
    check(run(eng, P[m], rdry=rdry, rho_thermal=rho, tau_thermal=tau), want, P[m], kind[m], F64, f"g rdry + thermal {sensor}")
