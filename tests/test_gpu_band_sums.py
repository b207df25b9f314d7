"""The band kernels per sample: k_bands<T, MAT, FULL> read out sample by sample and band by band, and their reductions bit for bit.

Per sample.  pick_chunk(B) is 1 for B <= 256, so a run of at most 256 rows leaves one row of per-chunk band sums per sample in
its workspace (spart_workspace_bandsum): rso + rdo + rsd + rdd at bands 0..2001 (FULL = 1; 2001 = the thermal evaluation) or
the four separately (FULL = 2, the band_mean launch).  per_sample() reads them in slices of <= 256 rows.  At chunk 1 a stage
is one sample, so a row with cbc = prot = 0 runs the float32 headline kernel's common-case body and any other the general one.
The rows are the domain grid of tests/helpers/domain_grid.py; the float32 bound is its conditioning-aware bound32 (factor
C32 = 4 on the relative change of the oracle's SAILH when given float32-rounded leaf and soil spectra; floor 1e-2; the
bare-soil rows of edge.npz at 4e-4 for the sum).  tests/test_band_sum_f32.py holds the same expression, built with g++, to the
same bound.

Exact reductions.  The kernels add each sample's value to a running sum in T, in sample order, from 0.  Every value that
enters such a sum is the result of an add or an FMA, never a bare product -- canopy_soil_sum and the four outputs of
canopy_soil all have the form x + y z, the materialised FULL = 1 value is (rso + rdo) + (rsd + rdd) -- so clang's
contraction cannot fuse it into the running sum, and the per-chunk sums of any chunk equal the sequential sum (numpy, in T,
from 0, one add per sample) of the chunk-1 values of the same rows.  A kernel change that lets a product reach the running
sum breaks that, and these tests say so.  A failure only where a stage's body differs from the rows' own chunk-1 body means
the GPU's two bodies do not give the same bits.

Measured on one MI355X: the module runs in about 20 s (its oracle included).  The float32 kernels stay within 0.79 of
bound32 on the grid; the worst relative error of the headline sum is 1.7e-3 inside the LHS ranges and 6.7e-4 outside them,
both where delta is large.  canopy_soil_sum against (rso + rdo) + (rsd + rdd) of the materialising kernel: at most 3.5e-6
of |rso| + |rdo| + |rsd| + |rdd| (1.2e-6 inside the LHS ranges), held to EXPR.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import domain_grid as G

pytestmark = pytest.mark.gpu

SENSOR = "Sentinel2A-MSI"
SLICE = 256                               # pick_chunk(B) == 1 up to here
TD = {"float32": np.float32, "float64": np.float64}
MAT8 = ("leaf_refl", "leaf_tran", "leaf_kchl", "soil_refl") + G.SPECTRA
F64 = (1e-7, 1e-3)                        # float64 band kernels: bound, floor (test_gpu_thermal's at_scale fixture)
LEAFTOL = (1e-4, 1e-2)                    # float32 leaf / soil fields (test_gpu_parity TOL / FLOOR)
EXPR = 5e-6                               # headline expression vs materialised expression (relative to |rso| + |rdo| + |rsd| + |rdd|)
IN_PROCESS = {300: 2, 2049: 9, 9000: 32, 8193: 32, 8191: 32}   # B -> pick_chunk(B); last chunk 2, 6, 8, 1, 31 rows
CHILD = {33: 33 * 269 + 1, 37: 37 * 240 + 31, 80: 80 * 111 + 1, 123: 123 * 72 + 31}   # SPART_CHUNK -> B (ragged 1 / 31)
NMIX = 9000


def chunk_block(eng, P, dtype, rho, tau, four=False, materialize=()):
    """one run(prune=False) into a workspace of our own filled with NaN bytes first; returns the per-chunk band sums
    (nchunk, 2002) -- (nchunk, 2002, 4) with four -- in T, the run's outputs and nchunk"""
    import torch
    B = P.shape[1]
    n = int(eng.lib.spart_workspace_bytes(eng.ctx, 1 if dtype == "float64" else 0, B))
    ws = torch.full((n,), 255, dtype=torch.uint8, device=eng.device)
    mat = tuple(materialize) + (("band_mean",) if four else ())
    res = eng.run(P, dtype, rho_thermal=rho, tau_thermal=tau, materialize=mat, prune=False, _workspace=ws)
    off, nchunk, stride = eng.bandsum_layout(dtype, B)
    es, w = (8 if dtype == "float64" else 4), (4 if four else 1)
    assert stride >= G.NEV and off % es == 0 and off + nchunk * stride * w * es <= n
    td = torch.float64 if dtype == "float64" else torch.float32
    blk = ws[off:off + nchunk * stride * w * es].view(td).reshape(nchunk, stride, w)[:, :G.NEV]
    torch.cuda.synchronize()
    blk = blk.cpu().numpy()
    return (blk if four else blk[..., 0]), res, nchunk


def per_sample(eng, P, dtype, rho, tau, four=False, materialize=()):
    """(B, 2002[, 4]) values of every sample, in slices of <= 256 rows (one chunk per sample: asserted, so that a SPART_CHUNK
    left in the environment cannot pass silently); with materialize also the named outputs, (B, width) numpy float64"""
    import torch
    out, mats = [], {k: [] for k in materialize}
    for a in range(0, len(P), SLICE):
        Pd = torch.as_tensor(P[a:a + SLICE].T.copy(), device="cuda:0")
        blk, res, nchunk = chunk_block(eng, Pd, dtype, rho[a:a + SLICE], tau[a:a + SLICE], four, materialize)
        assert nchunk == Pd.shape[1], (nchunk, Pd.shape[1])
        out.append(blk)
        for k in materialize:
            mats[k].append(res[k].double().cpu().numpy())
    return np.concatenate(out), {k: np.concatenate(v) for k, v in mats.items()}


def seq_chunk_sums(vals, chunk):
    """sequential sums in vals' dtype over consecutive chunks of `chunk` rows (sample order, from 0, one add per sample)"""
    B = vals.shape[0]
    nchunk = -(-B // chunk)
    pad = np.zeros((nchunk * chunk,) + vals.shape[1:], dtype=vals.dtype)   # (x + 0 == x: the ragged tail adds zeros)
    pad[:B] = vals
    v = pad.reshape((nchunk, chunk) + vals.shape[1:])
    acc = np.zeros((nchunk,) + vals.shape[1:], dtype=vals.dtype)
    for j in range(chunk):
        acc = acc + v[:, j]
    return acc


def mixed_batch(n=NMIX):
    """LHS 'full' rows (cbc = prot = 0, film 0.015: the common case) with 1.5 % of them replaced by grid rows (PRO leaves,
    other films, edge values) and 0.5 % given another film -- at every chunk some stages run the common-case body, some the
    general one, some have a film that changes inside the stage (float64 film_same), and a workgroup's stages switch bodies"""
    from spart_amd_workloads import lhs_params
    P = lhs_params(n, "full", seed=81)
    Pg, _ = G.grid_params()
    rng = np.random.default_rng(82)
    u = rng.random(n)
    gi = np.flatnonzero(u < 0.015)
    P[gi] = Pg[rng.integers(0, len(Pg), len(gi))]
    P[(u >= 0.015) & (u < 0.02), G.COL["film"]] = 0.004
    rho, tau = G.thermal_draw(n, 83)
    return P, rho, tau


def _mix_stats(P, chunk):
    """(stages of 32 samples within chunks of `chunk` that run the common-case body, stages that do not, stages whose film changes)"""
    common = G.common_body(P)
    film = P[:, G.COL["film"]]
    nc = nd = nf = 0
    for s0 in range(0, len(P), chunk):
        for a in range(s0, min(s0 + chunk, len(P)), 32):
            b = min(a + 32, s0 + chunk, len(P))
            same = np.all(film[a:b] == film[a])
            nf += not same
            if same and common[a:b].all():
                nc += 1
            else:
                nd += 1
    return nc, nd, nf


@pytest.fixture(scope="module")
def eng():
    import torch
    from spart_amd import get_engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_engine(SENSOR, 0)


@pytest.fixture(scope="module")
def grid(oracle, tables):
    return G.build_grid(oracle, tables)


@pytest.fixture(scope="module")
def grid_runs(eng, grid):
    """the grid through k_bands<float, 0, 1>, <float, 0, 2>, <double, 0, 1>, <double, 0, 2> and the materialising
    <float, 1, 1> / <double, 1, 1> (all eight fields), one chunk per sample"""
    P, rho, tau = grid["P"], grid["rho"], grid["tau"]
    out = {}
    for dtype in ("float32", "float64"):
        out[dtype, 1] = per_sample(eng, P, dtype, rho, tau)[0]
        out[dtype, 2] = per_sample(eng, P, dtype, rho, tau, four=True)[0]
        out[dtype, "mat"] = per_sample(eng, P, dtype, rho, tau, materialize=MAT8)
    return out


def _worst(err, bound, g):
    x = err / bound
    r, b = np.unravel_index(np.argmax(x), x.shape)
    return float(x[r, b]), (int(r), str(g["kind"][r]), "band", int(b), "err %.3g bound %.3g" % (err[r, b], bound[r, b]))


def test_grid_has_both_bodies(grid):
    """both sample-loop bodies are measured on every kind of edge"""
    n = {k: ((grid["kind"] == k) & grid["common"]).sum() for k in np.unique(grid["kind"])}
    g = {k: ((grid["kind"] == k) & ~grid["common"]).sum() for k in np.unique(grid["kind"])}
    assert n == {"ota_full": 44, "ota_pro": 44, "past": 70, "corner_full": 128, "corner_pro": 30, "golden": 94}, n
    assert g == {"ota_full": 0, "ota_pro": 2, "past": 2, "corner_full": 0, "corner_pro": 98, "golden": 31}, g
    assert G.bare_soil(grid["P"]).sum() == G.BARE_SOIL_ROWS


def test_headline_per_sample_vs_oracle(grid, grid_runs):
    """k_bands<float, 0, 1> (the benchmark's kernel): rso + rdo + rsd + rdd of every grid row and band within bound32 of the
    oracle, both bodies"""
    got = grid_runs["float32", 1]
    assert got.dtype == np.float32 and np.isfinite(got).all()
    for body in (True, False):
        m = grid["common"] == body
        w, where = _worst(G.rel(got[m], grid["sum"][m]), G.bound32(grid)[m], {"kind": grid["kind"][m]})
        assert w <= 1.0, ("common" if body else "general", where)


def test_four_sums_per_sample_vs_oracle(grid, grid_runs):
    """k_bands<float, 0, 2> (the band_mean launch): each of rso, rdo, rsd, rdd within its own bound32"""
    got = grid_runs["float32", 2]
    assert np.isfinite(got).all()
    for q, k in enumerate(G.SPECTRA):
        w, where = _worst(G.rel(got[..., q], grid[k]), G.bound32(grid, k), grid)
        assert w <= 1.0, (k, where)


def test_float64_per_sample_vs_oracle(grid, grid_runs):
    """k_bands<double, 0, 1>, <double, 0, 2> and <double, 1, 1>: 1e-7 against the oracle on a 1e-3 floor"""
    tol, fl = F64
    err = np.abs(grid_runs["float64", 1] - grid["sum"]) / np.maximum(np.abs(grid["sum"]), fl)
    assert err.max() < tol, _worst(err, np.full_like(err, tol), grid)
    for q, k in enumerate(G.SPECTRA):
        for got in (grid_runs["float64", 2][..., q], grid_runs["float64", "mat"][1][k][:, :G.NEV]):
            err = np.abs(got - grid[k]) / np.maximum(np.abs(grid[k]), fl)
            assert err.max() < tol, (k, _worst(err, np.full_like(err, tol), grid))


def test_materialised_per_sample_vs_oracle(grid, grid_runs):
    """k_bands<float, 1, 1>: the leaf, soil and leaf_kchl fields at 1e-4 (floor 1e-2: they do not pass through SAIL), rso, rdo,
    rsd, rdd at bound32"""
    m = grid_runs["float32", "mat"][1]
    tol, fl = LEAFTOL
    for k in ("leaf_refl", "leaf_tran", "soil_refl"):
        err = np.abs(m[k][:, :G.NEV] - grid[k]) / np.maximum(np.abs(grid[k]), fl)
        assert err.max() < tol, (k, _worst(err, np.full_like(err, tol), grid))
    err = np.abs(m["leaf_kchl"] - grid["leaf_kchl"]) / np.maximum(np.abs(grid["leaf_kchl"]), fl)
    assert err.max() < tol, ("leaf_kchl", _worst(err, np.full_like(err, tol), grid))
    for k in G.SPECTRA:
        w, where = _worst(G.rel(m[k][:, :G.NEV], grid[k]), G.bound32(grid, k), grid)
        assert w <= 1.0, (k, where)


def test_headline_expression_vs_materialised_expression(grid, grid_runs):
    """canopy_soil_sum (k_bands<float, 0, 1>) against (rso + rdo) + (rsd + rdd) of k_bands<float, 1, 1> for the same rows: the
    two share canopy_core_l and differ in the soil coupling and the final sum only.  The difference is measured against
    |rso| + |rdo| + |rsd| + |rdd| (floor 1e-2), the scale of a float32 rounding of the sum: where the four cancel -- the
    nearly non-absorbing PRO leaf at LAI 7, rso = -6.2 against rdo + rsd + rdd = +6.2, sum 0.005 -- the two float32 forms
    differ by 3.4e-5 of the sum and 3e-8 of that scale.  Worst over the grid: 3.5e-6 of the scale (an edge.npz row)."""
    a = grid_runs["float32", 1].astype(np.float64)
    m = grid_runs["float32", "mat"][1]
    b = (m["rso"] + m["rdo"] + m["rsd"] + m["rdd"])[:, :G.NEV]
    scale = sum(np.abs(m[k][:, :G.NEV]) for k in G.SPECTRA)
    err = np.abs(a - b) / np.maximum(scale, G.FLOOR)
    assert err.max() < EXPR, _worst(err, np.full_like(err, EXPR), grid)


def test_materialised_band_sums_equal_stored_rows(grid, grid_runs):
    """MAT = 1, FULL = 1 at chunk 1: the band sum of a sample is fl((rso + rdo) + (rsd + rdd)) of its stored rows, in T"""
    for dtype in ("float32", "float64"):
        blk, m = grid_runs[dtype, "mat"]
        t = TD[dtype]
        want = (m["rso"].astype(t) + m["rdo"].astype(t)) + (m["rsd"].astype(t) + m["rdd"].astype(t))
        assert np.array_equal(blk, want[:, :G.NEV]), dtype


# ------------------------------------------------------------------------------------------------ exact reductions
@pytest.fixture(scope="module")
def mixed(eng):
    """the mixed batch and its chunk-1 values: {(dtype, four): (NMIX, 2002[, 4]) in T}"""
    P, rho, tau = mixed_batch()
    vals = {(d, f): per_sample(eng, P, d, rho, tau, four=f)[0] for d in ("float32", "float64") for f in (False, True)}
    return P, rho, tau, vals


def _check_chunks(got, vals, chunk, tag):
    want = seq_chunk_sums(vals, chunk)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.flatnonzero(np.any((got != want).reshape(len(got), -1), axis=1))
    assert bad.size == 0, (tag, "chunks differing", bad.size, "first", int(bad[0]))


@pytest.mark.parametrize("B", sorted(IN_PROCESS))
def test_stage_invariance_in_process(eng, mixed, B):
    """per-chunk sums at pick_chunk(B) = 2, 9, 32 (ragged last chunks of 2, 6, 8, 1, 31 rows) == the sequential sums of the
    chunk-1 values, FULL = 1 and 2, float32 and float64"""
    import torch
    P, rho, tau, vals = mixed
    chunk = IN_PROCESS[B]
    nc, nd, nf = _mix_stats(P[:B], chunk)
    assert nc >= 1 and nd >= 1, (nc, nd)
    if chunk >= 9:
        assert nf >= 1
    Pd = torch.as_tensor(P[:B].T.copy(), device="cuda:0")
    for (dtype, four), v in vals.items():
        got, _, nchunk = chunk_block(eng, Pd, dtype, rho[:B], tau[:B], four)
        assert nchunk == -(-B // chunk)
        _check_chunks(got, v[:B], chunk, (dtype, four, B))


@pytest.mark.parametrize("chunk", sorted(CHILD))
def test_stage_invariance_across_stages(mixed, chunk, tmp_path):
    """SPART_CHUNK = 33, 37, 80, 123 in a child process (123: the chunk of the headline's B = 1 000 000 -- three full stages and
    one of 27): every workgroup walks several stages, which switch between the two bodies; the same equality"""
    P, rho, tau, vals = mixed
    B = CHILD[chunk]
    nc, nd, nf = _mix_stats(P[:B], chunk)
    assert nc >= 10 and nd >= 10 and nf >= 1, (nc, nd, nf)
    out = str(tmp_path / "sums.npz")
    env = dict(os.environ, SPART_CHUNK=str(chunk))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), str(B), out], env=env,
                       timeout=330)
    assert r.returncode == 0, r.returncode
    got = np.load(out)
    for (dtype, four), v in vals.items():
        g = got[f"{dtype}/{int(four)}"]
        assert g.shape[0] == -(-B // chunk)
        _check_chunks(g, v[:B], chunk, (dtype, four, chunk))


@pytest.fixture(scope="module")
def mat_runs(eng, mixed):
    """B = 2049 (chunk 9, last chunk 6) with materialised spectra: MAT = 1 with FULL = 1 and with FULL = 2 (band_mean)"""
    import torch
    P, rho, tau, _ = mixed
    B = 2049
    Pd = torch.as_tensor(P[:B].T.copy(), device="cuda:0")
    out = {}
    for dtype in ("float32", "float64"):
        for four in (False, True):
            blk, res, nchunk = chunk_block(eng, Pd, dtype, rho[:B], tau[:B], four, materialize=G.SPECTRA)
            assert nchunk == 228
            out[dtype, four] = blk, {k: v.cpu().numpy() for k, v in res.items() if k in G.SPECTRA + ("band_mean",)}
    return out


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_materialised_chunk_sums_equal_stored_rows(mat_runs, dtype):
    """MAT = 1: per-chunk sums == sequential sums in T of fl((rso + rdo) + (rsd + rdd)) of the stored rows (FULL = 1), and of
    each stored spectrum (FULL = 2)"""
    blk, m = mat_runs[dtype, False]
    r = {k: m[k][:, :G.NEV] for k in G.SPECTRA}
    _check_chunks(blk, (r["rso"] + r["rdo"]) + (r["rsd"] + r["rdd"]), 9, (dtype, "FULL = 1"))
    blk, m = mat_runs[dtype, True]
    _check_chunks(blk, np.stack([m[k][:, :G.NEV] for k in G.SPECTRA], axis=-1), 9, (dtype, "FULL = 2"))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_band_mean_is_the_float64_sum_of_chunk_sums(eng, mixed, mat_runs, dtype):
    """k_bandmean: (T)(float64 sequential sum of the per-chunk sums in chunk order / B); bands 2002..2161 == band 2001.  Both
    with materialised spectra (MAT = 1) and without (MAT = 0, B = 9000, chunk 32)"""
    import torch
    P, rho, tau, _ = mixed
    B = 9000
    blk, res, _ = chunk_block(eng, torch.as_tensor(P[:B].T.copy(), device="cuda:0"), dtype, rho[:B], tau[:B], four=True)
    runs = [(blk, res["band_mean"].cpu().numpy(), B), (mat_runs[dtype, True][0], mat_runs[dtype, True][1]["band_mean"], 2049)]
    for blk, bm, n in runs:
        assert bm.shape == (4, 2162) and bm.dtype == TD[dtype]
        acc = np.add.accumulate(blk.astype(np.float64), axis=0)[-1]          # (2002, 4), chunk order
        want = (acc / float(n)).astype(TD[dtype]).T
        assert np.array_equal(bm[:, :G.NEV], want), (dtype, n)
        assert np.array_equal(bm[:, G.NEV:], np.repeat(bm[:, G.NEV - 1:G.NEV], 2162 - G.NEV, axis=1)), (dtype, n)


if __name__ == "__main__":          # the child of test_stage_invariance_across_stages (SPART_CHUNK set): per-chunk sums -> .npz
    for p in (os.path.join(ROOT, "spart-python_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    from spart_amd import get_engine
    B, path = int(sys.argv[1]), sys.argv[2]
    chunk = int(os.environ["SPART_CHUNK"])
    P, rho, tau = mixed_batch()
    e = get_engine(SENSOR, 0)
    Pd = torch.as_tensor(P[:B].T.copy(), device="cuda:0")
    res = {}
    for dtype in ("float32", "float64"):
        for four in (False, True):
            blk, _, nchunk = chunk_block(e, Pd, dtype, rho[:B], tau[:B], four)
            assert nchunk == -(-B // chunk), nchunk
            res[f"{dtype}/{int(four)}"] = blk
    np.savez(path, **res)
