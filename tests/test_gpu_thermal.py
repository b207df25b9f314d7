"""GPU side of tests/test_thermal.py: LeafBiology.rho_thermal / tau_thermal (prospect_5d.py:82-83, padded over bands 2001..2161,
SPART.py:445-470), band centres outside 400-2400 nm (SPART.py:219-223), and the per-chunk band sums of the headline kernel
k_bands<T, 0, 1, false>, whose only output is a workspace block (spart_workspace_bandsum says where it lies).

The thermal values reach the kernels in three places: the prelude (NULL pointer = 0.01), k_bands at its last tile (the
evaluation at index 2001 and the padding stores of bands 2002..2161) and k_columns (support points past 2400 nm).  Every test
below gives non-default values, most of them different per row.  References: the REAL reference through thermal.npz, and the
oracle, which tests/test_thermal.py pins to that fixture.  fp64 <= 1e-8 against the reference, fp32 <= 1e-4.
"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT, rel_err
from helpers.domain_grid import thermal_draw as _thermal_draw
from test_thermal import COLUMNS, GROUPS, SENSORS, SPECTRA, edited_tables

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import table_edits  # noqa: E402

pytestmark = pytest.mark.gpu

COLTOL = {"float64": 1e-8, "float32": 1e-4}                         # columns, |x - ref| / max(|ref|, 1e-6)
SPECTOL = {"float64": (1e-3, 1e-8), "float32": (1e-2, 1e-4)}        # spectra: (floor, bound), test_canopy_state's metric
TINY = 1e-200     # the oracle's stand-in for rho = tau = 0 (see test_black_leaves_limit)
MAT7 = ("leaf_refl", "leaf_tran", "soil_refl", "rso", "rdo", "rsd", "rdd")   # the arrays k_bands pads over bands 2002..2161


@pytest.fixture(scope="module")
def fx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return np.load(os.path.join(ROOT, "tests", "golden", "thermal.npz"))


def finite_limit(a):
    """rho = tau = 0 makes the reference's rinf = (a - m) / sigb a 0/0 (sailh.py:151), NaN in every thermal band; the kernels
    use rinf = sigb / (a + m) and return the finite limit, which test_black_leaves_limit pins against the
    oracle.  Everywhere else rel_err has already asserted finiteness where the reference is finite."""
    return bool(np.isfinite(np.asarray(a, dtype=np.float64)).all())


def _sp(S, P, rho, tau, sensor, dtype, wl_smac=None):
    """a SPART object of this package as the generator built the reference's: row-wise scalars for a 1-D row, arrays otherwise"""
    col = (lambda i: P[i]) if P.ndim == 1 else (lambda i: P[:, i])
    with redirect_stdout(io.StringIO()):
        sp = S.SPART(S.SoilParameters(*[col(i) for i in range(9, 15)]),
                     S.LeafBiology(*[col(i) for i in range(7)], PROT=col(7), CBC=col(8), rho_thermal=rho, tau_thermal=tau),
                     S.CanopyStructure(*[col(i) for i in range(15, 19)]),
                     S.AtmosphericProperties(col(22), col(23), col(24), Pa=col(25)), S.Angles(col(19), col(20), col(21)),
                     sensor, int(P[26]) if P.ndim == 1 else P[:, 26], dtype=dtype)
    table_edits.upcast_coefs(sp.sensorinfo)
    if wl_smac is not None:
        sp.sensorinfo["wl_smac"] = wl_smac.copy()
    return sp


def _check_cols(got, fx, n, dtype, rows=slice(None)):
    for k in COLUMNS:
        assert rel_err(np.asarray(got[k]), fx[f"{n}/{k}"][rows], 1e-6) < COLTOL[dtype], (n, dtype, k)


def _check_spectra(sp, fx, n, dtype, rows=slice(None)):
    """canopyopt / leafopt of a batched run(materialize=True) at the fixture's probe bands"""
    pi = fx["probe_index"]
    fl, tol = SPECTOL[dtype]
    for k in SPECTRA:
        a, ref = np.asarray(getattr(sp.canopyopt, k))[:, pi], fx[f"{n}/{k}"][rows]
        assert rel_err(a, ref, fl) < tol, (n, dtype, k)
        assert finite_limit(a), (n, dtype, k)
    th = pi >= 2001
    for k, f in (("refl", "leaf_refl"), ("tran", "leaf_tran")):
        a = np.asarray(getattr(sp.leafopt, k))[:, pi]
        assert np.array_equal(a[:, th], fx[f"{n}/{f}"][rows][:, th].astype(np.float32 if dtype == "float32" else np.float64)), (n, k)
        assert rel_err(a[:, ~th], fx[f"{n}/{f}"][rows][:, ~th], 0.1) < (1e-6 if dtype == "float64" else 1e-4), (n, k)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_scalar_run_vs_reference(fx, dtype):
    """SPART(...).run(debug=True), one scalar object per row: the fast path (_run_scalar), thermal values through its staging
    block (din[27:29]).  Every pair of the fixture, both sensors; fp32 on the first 3 rows of each group."""
    import SPART as S
    P = fx["P"]
    for s in SENSORS:
        for g in GROUPS:
            n = f"run/{g}/{s}"
            rho, tau = fx[n + "/rho_thermal"], fx[n + "/tau_thermal"]
            m = len(P) if dtype == "float64" else 3
            got = {k: [] for k in COLUMNS}
            for i in range(m):
                sp = _sp(S, P[i], float(rho[i]), float(tau[i]), s, dtype)
                with redirect_stdout(io.StringIO()):
                    df = sp.run(debug=True)
                for k in COLUMNS:
                    got[k].append(df[k].to_numpy())
            _check_cols({k: np.array(v) for k, v in got.items()}, fx, n, dtype, slice(0, m))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_batched_run_vs_reference(fx, dtype):
    """the same rows as ONE batched object: every LeafBiology field a length-B array (thermal values per row in `mixed`), columns
    and the materialised spectra at the probe bands (thermal bands 2001, 2002, 2100, 2161 and solar ones)"""
    import SPART as S
    P = fx["P"]
    for s in SENSORS:
        for g in GROUPS:
            n = f"run/{g}/{s}"
            sp = _sp(S, P, fx[n + "/rho_thermal"], fx[n + "/tau_thermal"], s, dtype)
            with redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                res = sp.run(debug=True)
                full = sp.run(debug=True, materialize=True)
            _check_cols(res, fx, n, dtype)
            for k in COLUMNS:
                assert np.array_equal(res[k], full[k]), (n, dtype, k)           # pruned and full runs: identical columns
            _check_spectra(sp, fx, n, dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_scalar_fields_with_thermal_arrays(fx, dtype):
    """README: every constructor field accepts a length-B array.  Scalar parameters with (B,) rho_thermal / tau_thermal: B is
    the thermal arrays' length (the batch used to be sized from the parameter columns alone, B = 1, and the run raised)."""
    import SPART as S
    pairs = fx["pairs"]
    d = fx["P"][0]
    for s in SENSORS:
        sp = _sp(S, d, pairs[:, 0].copy(), pairs[:, 1].copy(), s, dtype)
        with redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            res = sp.run(debug=True)
            sp.run(debug=True, materialize=True)
        assert res["R_TOC"].shape[0] == len(pairs)
        for j in range(len(pairs)):
            n = f"run/{j}/{s}"
            _check_cols({k: res[k][j:j + 1] for k in COLUMNS}, fx, n, dtype, slice(0, 1))
            for k in SPECTRA:
                a, ref = np.asarray(getattr(sp.canopyopt, k))[j:j + 1, fx["probe_index"]], fx[f"{n}/{k}"][:1]
                assert rel_err(a, ref, SPECTOL[dtype][0]) < SPECTOL[dtype][1] and finite_limit(a), (n, k)
        # the lazy spectra of a pruned run are evaluated from the same (B,) thermal values
        sp2 = _sp(S, d, pairs[:, 0].copy(), pairs[:, 1].copy(), s, dtype)
        with redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            sp2.run()
            assert np.array_equal(np.asarray(sp2.canopyopt.rso), np.asarray(sp.canopyopt.rso), equal_nan=True)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_edited_band_centres_vs_reference(fx, dtype):
    """MODIS with centres moved to 390 ... 60 000 nm (sensorinfo['wl_smac'] edited on the object), default and non-default
    thermal pair, scalar objects (fast path) and one batched object"""
    import SPART as S
    P = fx["P"][:5]
    wl = fx["centres/wl_smac"]
    for g in ("default", "2"):
        n = f"centres/{g}"
        rho, tau = fx[n + "/rho_thermal"], fx[n + "/tau_thermal"]
        got = {k: [] for k in COLUMNS}
        for i in range(len(P)):
            with redirect_stdout(io.StringIO()):
                df = _sp(S, P[i], float(rho[i]), float(tau[i]), "TerraAqua-MODIS", dtype, wl).run(debug=True)
            assert np.array_equal(df.index.to_numpy(dtype=np.float64), wl[:, 0])
            for k in COLUMNS:
                got[k].append(df[k].to_numpy())
        _check_cols({k: np.array(v) for k, v in got.items()}, fx, n, dtype)
        with redirect_stdout(io.StringIO()):
            res = _sp(S, P, rho, tau, "TerraAqua-MODIS", dtype, wl).run(debug=True)
        _check_cols(res, fx, n, dtype)


def test_sailh_with_thermal_leafopt_vs_reference(fx):
    """SAILH(soil, leafopt, canopy, angles) at the API level with leafopt padded to non-default thermal values by
    set_leaf_refl_trans_assumptions: the reference's probe bands of the default-parameter row, every pair"""
    import SPART as S
    d = fx["P"][0]
    op = S.load_optical_parameters()
    so = S.set_soil_refl_trans_assumptions(S.BSM(S.SoilParameters(*d[9:15]), op), S.SpectralBands())
    pi = fx["probe_index"]
    for j, (rho, tau) in enumerate(fx["pairs"]):
        lb = S.LeafBiology(*d[:7], PROT=d[7], CBC=d[8], rho_thermal=float(rho), tau_thermal=float(tau))
        lo = S.set_leaf_refl_trans_assumptions(S.PROSPECT_5D(lb, op), lb, S.SpectralBands())
        assert np.all(np.asarray(lo.refl)[2001:] == rho) and np.all(np.asarray(lo.tran)[2001:] == tau)
        for dtype in ("float64", "float32"):
            with np.errstate(all="ignore"):
                rad = S.SAILH(so, lo, S.CanopyStructure(*d[15:19]), S.Angles(*d[19:22]), dtype=dtype)
            for k in SPECTRA:
                a, ref = np.asarray(getattr(rad, k))[pi, 0], fx[f"run/{j}/Sentinel2A-MSI/{k}"][0]
                assert rel_err(a, ref, SPECTOL[dtype][0]) < SPECTOL[dtype][1], (j, dtype, k)
                assert finite_limit(a), (j, dtype, k)


# ------------------------------------------------------------------------------------------------ engine level, vs the oracle
def _oracle_rows(oracle, tables, P, sensor, rho, tau, block=1000):
    out = None
    for a in range(0, len(P), block):
        with np.errstate(all="ignore"):
            o = oracle.spart_run(P[a:a + block], sensor, tables, pso="gl", full=True, rho_thermal=rho[a:a + block],
                                 tau_thermal=tau[a:a + block])
        o["leaf_refl"], o["leaf_tran"] = oracle.pad_leaf(o["leaf_refl"], o["leaf_tran"], rho[a:a + block], tau[a:a + block])
        o["soil_refl"] = oracle.pad_soil(o["soil_refl"])
        o = {k: o[k] for k in MAT7 + ("R_TOC", "R_TOA", "L_TOA", "rsoil")}
        out = o if out is None else {k: np.concatenate([out[k], o[k]]) for k in o}
    return out


def _check_mat(res, ref, dtype, tag):
    """materialised (B, 2162) spectra: solar bands at the spectra bound; the thermal evaluation (band 2001) at the columns' bound;
    the padding 2002..2161 of EVERY row bit-equal to band 2001; leaf thermal bands equal to the row's own value"""
    fl, tol = SPECTOL[dtype]
    for k in MAT7:
        a = res[k].double().cpu().numpy()
        assert a.shape == ref[k].shape, (tag, k)
        assert np.array_equal(a[:, 2001:], np.repeat(a[:, 2001:2002], 161, axis=1)), (tag, dtype, k, "padding")
        if k.startswith("leaf"):
            if dtype == "float64":          # test_config2_lhs_workload_all_rows' bound on the leaf model against the oracle
                assert np.max(np.abs(a[:, :2001] - ref[k][:, :2001])) < 2e-9, (tag, dtype, k)
            else:
                assert rel_err(a[:, :2001], ref[k][:, :2001], fl) < tol, (tag, dtype, k)
            want = ref[k][:, 2001].astype(np.float32) if dtype == "float32" else ref[k][:, 2001]
            assert np.array_equal(a[:, 2001], want), (tag, dtype, k)
        else:
            assert rel_err(a[:, :2001], ref[k][:, :2001], fl) < (1e-7 if dtype == "float64" else tol), (tag, dtype, k)
            assert rel_err(a[:, 2001], ref[k][:, 2001], 1e-6) < COLTOL[dtype], (tag, dtype, k, "thermal")


def test_engine_per_row_thermal_all_bands(oracle, tables, fx):
    """Engine.run on 2 048 LHS rows, each with its own rho_thermal / tau_thermal, against the oracle with the same (B,) arrays:
    the seven padded spectra in both dtypes over every band of every row (a padding store taking another lane's or another
    row's value, or a value that reaches row 0 only, fails here), and the columns of an engine whose band centres lie past
    2400 nm (k_columns' thermal support points)."""
    import torch
    from spart_amd import get_engine, workloads
    B = 2048
    P = workloads.lhs_params(B, "full", seed=43)
    rho, tau = _thermal_draw(B, 44)
    for sensor, tabs, si in (("Sentinel2A-MSI", tables, None), ("TerraAqua-MODIS", edited_tables(tables, fx), "edited")):
        ref = _oracle_rows(oracle, tabs, P, sensor, rho, tau)
        if si is None:
            eng = get_engine(sensor, 0)
        else:
            import SPART as S
            info = S.load_sensor_info(sensor)
            info["wl_smac"] = fx["centres/wl_smac"].copy()
            eng = get_engine(sensor_info=info, device=0)
            assert np.array_equal(eng.wl_smac, fx["centres/wl_smac"][:, 0])
        Pd = torch.as_tensor(P.T.copy(), device="cuda:0")
        for dtype in ("float64", "float32"):
            res = eng.run(Pd, dtype, rho_thermal=rho, tau_thermal=tau, materialize=MAT7 + ("rsoil",))
            for k in ("R_TOC", "R_TOA", "L_TOA", "rsoil"):
                assert rel_err(res[k].double().cpu().numpy(), ref[k], 1e-6) < COLTOL[dtype], (sensor, dtype, k)
            if si is None:
                _check_mat(res, ref, dtype, sensor)
            del res


def test_null_and_default_thermal_pointers(oracle, tables, fx):
    """spart_run_batch with NULL thermal pointers == explicit (B,) arrays of 0.01, bit for bit (columns and the seven spectra);
    non-default arrays change the thermal bands 2001..2161 of every row and NOTHING else -- no solar band, no soil, and only the
    columns whose np.interp support reaches past 2400 nm"""
    import torch
    import SPART as S
    from spart_amd import get_engine, workloads
    B = 300
    P = workloads.lhs_params(B, "full", seed=45)
    rho, tau = _thermal_draw(B, 46)
    info = S.load_sensor_info("TerraAqua-MODIS")
    info["wl_smac"] = fx["centres/wl_smac"].copy()
    i0, i1, fr = oracle.interp_weights(fx["centres/wl_smac"][:, 0])
    moved = (i0 >= 2001) | ((i1 >= 2001) & (fr > 0))
    Pd = torch.as_tensor(P.T.copy(), device="cuda:0")
    for eng in (get_engine("Sentinel2A-MSI", 0), get_engine(sensor_info=info, device=0)):
        for dtype in ("float64", "float32"):
            run = lambda r, t: {k: v.clone() for k, v in eng.run(Pd, dtype, rho_thermal=r, tau_thermal=t,  # noqa: E731
                                                                  materialize=MAT7 + ("leaf_kchl", "soil_refl_dry", "rsoil")).items()}
            a, b = run(None, None), run(np.full(B, 0.01), np.full(B, 0.01))
            for k in a:
                assert torch.equal(a[k], b[k]), (dtype, k)
            c = run(rho, tau)
            for k in a:
                x, y = a[k].cpu().numpy(), c[k].cpu().numpy()
                if k in ("R_TOC", "R_TOA", "L_TOA", "rsoil"):
                    diff = np.any(x != y, axis=0)
                    want = moved if (eng.nb == len(moved) and k != "rsoil") else np.zeros(eng.nb, bool)   # (soil: no leaf)
                    assert np.array_equal(diff, want), (dtype, k, diff)
                elif k in ("leaf_kchl", "soil_refl_dry", "soil_refl"):
                    assert np.array_equal(x, y), (dtype, k)
                else:
                    assert np.array_equal(x[:, :2001], y[:, :2001]), (dtype, k)
                    assert np.all(x[:, 2001:] != y[:, 2001:]), (dtype, k)


def test_black_leaves_limit(oracle, tables, fx):
    """rho_thermal = tau_thermal = 0 (a pair of the fixture): where the reference divides 0 by 0 the kernels return the limit
    rho, tau -> 0, which the oracle reaches at rho = tau = 1e-200 (sigb^2 underflows, rinf = 0 exactly).  The seven padded spectra
    over every band and the columns of the edited-centre engine, both dtypes."""
    import torch
    import SPART as S
    from spart_amd import get_engine
    P = fx["P"]
    B = len(P)
    info = S.load_sensor_info("TerraAqua-MODIS")
    info["wl_smac"] = fx["centres/wl_smac"].copy()
    ref = _oracle_rows(oracle, edited_tables(tables, fx), P, "TerraAqua-MODIS", np.full(B, TINY), np.full(B, TINY))
    for k in ("leaf_refl", "leaf_tran"):
        ref[k][:, 2001:] = 0.0
    with np.errstate(all="ignore"):
        lit = oracle.spart_run(P, "TerraAqua-MODIS", edited_tables(tables, fx), pso="gl", full=True, rho_thermal=0.0, tau_thermal=0.0)
    assert np.isnan(lit["rso"][:, 2001:]).all() and np.isfinite(ref["rso"]).all()        # (what the limit stands in for)
    for k in SPECTRA:
        assert np.array_equal(ref[k][:, :2001], lit[k][:, :2001]), k
    eng = get_engine(sensor_info=info, device=0)
    Pd = torch.as_tensor(P.T.copy(), device="cuda:0")
    for dtype in ("float64", "float32"):
        res = eng.run(Pd, dtype, rho_thermal=np.zeros(B), tau_thermal=np.zeros(B), materialize=MAT7 + ("rsoil",))
        for k in ("R_TOC", "R_TOA", "L_TOA", "rsoil"):
            assert rel_err(res[k].double().cpu().numpy(), ref[k], 1e-6) < COLTOL[dtype], (dtype, k)
        _check_mat(res, ref, dtype, "black")


# ------------------------------------------------------------------------------------------------ the headline kernel's output
def _band_sums(eng, P, dtype, rho, tau):
    """Engine.run(materialize=(), prune=False) -- the launch of k_bands<T, 0, 1, false> -- into a workspace of our own, filled
    with NaN bytes first; then the per-chunk band sums read where spart_workspace_bandsum says, summed over the chunks (fp64)"""
    import torch
    B = P.shape[1]
    n = int(eng.lib.spart_workspace_bytes(eng.ctx, 1 if dtype == "float64" else 0, B))
    ws = torch.full((n,), 255, dtype=torch.uint8, device=eng.device)
    eng.run(P, dtype, rho_thermal=rho, tau_thermal=tau, materialize=(), prune=False, _workspace=ws)
    off, nchunk, stride = eng.bandsum_layout(dtype, B)
    td = torch.float64 if dtype == "float64" else torch.float32
    es = 8 if dtype == "float64" else 4
    assert stride >= 2002 and off % es == 0 and off + nchunk * stride * es <= n
    blk = ws[off:off + nchunk * stride * es].view(td).reshape(nchunk, stride)[:, :2002]
    torch.cuda.synchronize()
    return blk.double().sum(dim=0).cpu().numpy(), nchunk


# B -> chunks: 1 row; chunk 2; chunk 9 with a last chunk of 6 rows; chunk 32 with a last chunk of 8 rows
BANDSUM_B = {1: 1, 300: 150, 2049: 228, 9000: 282}


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 2e-5)])
@pytest.mark.parametrize("B", sorted(BANDSUM_B))
def test_headline_band_sums_vs_oracle(oracle, tables, B, dtype, tol):
    """the per-chunk band sums of the benchmark's dominant kernel (k_bands<float, 0, 1, false>, and <double, ...> in fp64),
    which no other output exposes, summed over the chunks = sum over rows of rso + rdo + rsd + rdd from the oracle at bands
    0..2001 (2001 = the thermal evaluation, per-row thermal values); the band_mean tests' metric and bounds"""
    import torch
    from spart_amd import get_engine, workloads
    P = workloads.lhs_params(B, "full", seed=47)
    rho, tau = _thermal_draw(B, 48)
    ref = np.zeros(2002)
    for a in range(0, B, 1000):
        with np.errstate(all="ignore"):
            o = oracle.spart_run(P[a:a + 1000], "Sentinel2A-MSI", tables, pso="gl", full=True, rho_thermal=rho[a:a + 1000],
                                 tau_thermal=tau[a:a + 1000])
        ref += sum(o[k][:, :2002].sum(axis=0) for k in SPECTRA)
    eng = get_engine("Sentinel2A-MSI", 0)
    Pd = torch.as_tensor(P.T.copy(), device="cuda:0")
    got, nchunk = _band_sums(eng, Pd, dtype, rho, tau)
    assert nchunk == BANDSUM_B[B]
    assert rel_err(got / B, ref / B, 1e-3) < tol, dtype


@pytest.fixture(scope="module")
def at_scale(oracle, tables):
    """B = 300 001 rows with per-row thermal values and the sum over all rows of their float64 materialised rso + rdo + rsd + rdd"""
    import torch
    from spart_amd import get_engine, workloads
    B = 300_001
    P = workloads.lhs_params(B, "full", seed=49)
    rho, tau = _thermal_draw(B, 50)
    eng = get_engine("Sentinel2A-MSI", 0)
    Pd = torch.as_tensor(P.T.copy(), device="cuda:0")
    res = eng.run(Pd, "float64", rho_thermal=rho, tau_thermal=tau, materialize=SPECTRA)
    rows = np.sort(np.random.default_rng(51).choice(B, 512, replace=False))
    rows[-1] = B - 1
    with np.errstate(all="ignore"):
        o = oracle.spart_run(P[rows], "Sentinel2A-MSI", tables, pso="gl", full=True, rho_thermal=rho[rows], tau_thermal=tau[rows])
    idx = torch.as_tensor(rows, device="cuda:0")
    ref = torch.zeros(2002, dtype=torch.float64, device="cuda:0")
    for k in SPECTRA:
        a = res[k][idx].cpu().numpy()
        assert rel_err(a[:, :2001], o[k][:, :2001], 1e-3) < 1e-7, k
        assert rel_err(a[:, 2001:], o[k][:, 2001:], 1e-6) < 1e-8, k
        ref += res[k][:, :2002].sum(dim=0)
    ref = ref.cpu().numpy()
    del res, o
    torch.cuda.empty_cache()
    return eng, Pd, rho, tau, ref


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-9), ("float32", 2e-5)])
def test_headline_band_sums_at_scale(at_scale, dtype, tol):
    """B = 300 001 (chunk 37, a ragged last chunk of 5 rows): the float64 materialised spectra (the MAT = 1 path, spot-checked on
    512 sampled rows against the oracle, every band) summed on the GPU are the reference of the band sums of the MAT = 0 kernel"""
    eng, Pd, rho, tau, ref = at_scale
    B = Pd.shape[1]
    got, nchunk = _band_sums(eng, Pd, dtype, rho, tau)
    assert nchunk == 8109
    assert rel_err(got / B, ref / B, 1e-3) < tol, dtype
