"""The float32 band kernel's per-stage vote (k_bands<float, 0, 1, false>: the J2 bit of sail_j2_possible) on stages that MIX
its outcomes, and the soil's wet / dry select beside it: inside every 32-sample stage ks LAI lies below 0.06, inside the
guard band 0.06..0.07 and far above it, and dry soils (SMp = 3) alternate with wet ones.  A sample's numbers must not depend
on its stage mates.

Rows.  STAGES x 32 LHS 'full' rows (cbc = prot = 0, one film: every stage runs the common-case body); LAI of positions
0..11 of a stage is set from the oracle's own extinction coefficient k so that k LAI is 0.02..0.055 (positions 0..7) or
0.061..0.069 (8..11); even positions are dry.  The oracle alone shows each stage on both sides of both thresholds.  The
"general" run gives the last sample of every stage another film, which sends the whole stage through the general body.

Checks.  (1) every row at chunk 1 (a stage of one sample) against the oracle at the bound of
test_gpu_band_sums.test_headline_per_sample_vs_oracle (domain_grid.bound32).  (2) in a child process with SPART_CHUNK = 32
the per-chunk sums of both runs equal the sequential float32 sums of the chunk-1 values of their rows
(test_gpu_band_sums._check_chunks): mixing changes no bit.  (3) directly: stages of ONE row of (1) among 31 "null" rows (LAI = 0,
soil brightness 0, dry: every band sums to exactly 0, asserted), so that the chunk's sum IS that row's value; with one null
given another film the general body computes it -- the two runs are bit-equal, and equal to the chunk-1 value.  (A sum of 32
values hides a last-bit difference of one of them in a share of the cases; (3) does not.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import domain_grid as G

STAGES, SUB = 16, 32
B = STAGES * SUB
OTHER_FILM = 0.004
J2_THRESH, J2_GUARD = 0.06, 0.07          # SailJ<float>::THRESH, SAIL_J2_GUARD_F32 (csrc/spart_math.h)


def mixed_rows(oracle, tables):
    """(P (B, 27), k (B,)): the rows described above and the oracle's extinction coefficient in the sun's direction"""
    from spart_amd_workloads import lhs_params
    P = lhs_params(B, "full", seed=91)
    with np.errstate(all="ignore"):
        k = oracle.spart_run(P, "Sentinel2A-MSI", tables, pso="gl", full=True)["aux"]["k"][:, 0]      # (does not depend on LAI)
    rng = np.random.default_rng(92)
    pos = np.arange(B) % SUB
    target = np.where(pos < 8, rng.uniform(0.02, 0.055, B), rng.uniform(0.061, 0.069, B))
    low = pos < 12
    P[low, G.COL["LAI"]] = (target / k)[low]
    P[pos % 2 == 0, G.COL["SMp"]] = 3.0
    return P, k


def general_rows(P):
    Q = P.copy()
    Q[SUB - 1::SUB, G.COL["film"]] = OTHER_FILM
    return Q


def null_row(film):
    from spart_amd_workloads import default_row
    return default_row(LAI=0.0, B=0.0, SMp=3.0, film=film)


def direct_rows(P):
    """stage i: row i of P at position i, 31 null rows around it; (common, general: the null at position (i + 1) % 32 has
    another film)"""
    film = P[0, G.COL["film"]]
    C = np.repeat(null_row(film), SUB * SUB, axis=0)
    for i in range(SUB):
        C[i * SUB + i] = P[i]
    Gn = C.copy()
    for i in range(SUB):
        Gn[i * SUB + (i + 1) % SUB, G.COL["film"]] = OTHER_FILM
    return C, Gn


@pytest.fixture(scope="module")
def rows(oracle, tables):
    P, k = mixed_rows(oracle, tables)
    assert np.all(P[:, G.COL["film"]] == P[0, G.COL["film"]]) and G.common_body(P).all()
    return P, k


def test_oracle_shows_every_stage_on_both_sides(rows):
    """from the oracle's quantities alone: k LAI below the threshold, inside the guard band and above it, and wet and dry
    soils (mu = (SMp - 5) / SMC, bsm.py:101), in every stage"""
    P, k = rows
    kl = (k * P[:, G.COL["LAI"]]).reshape(STAGES, SUB)
    mu = ((P[:, G.COL["SMp"]] - 5.0) / P[:, G.COL["SMC"]]).reshape(STAGES, SUB)
    assert ((kl < J2_THRESH).sum(axis=1) >= 1).all()
    assert (((kl > J2_THRESH) & (kl < J2_GUARD)).sum(axis=1) >= 1).all()
    assert ((kl > J2_GUARD).sum(axis=1) >= 1).all()
    assert ((mu > 0).sum(axis=1) >= 1).all() and ((mu <= 0).sum(axis=1) >= 1).all()


@pytest.fixture(scope="module")
def eng():
    import torch
    from spart_amd import get_engine
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return get_engine("Sentinel2A-MSI", 0)


@pytest.fixture(scope="module")
def chunk1(eng, rows):
    """chunk-1 values (a stage of one sample) of the mixed rows, of the rows the general run replaces, and of the null rows"""
    from test_gpu_band_sums import per_sample
    P, _ = rows
    rho, tau = G.thermal_draw(B, 93)
    Q = general_rows(P)
    rep = np.arange(SUB - 1, B, SUB)
    nul = np.concatenate([null_row(P[0, G.COL["film"]]), null_row(OTHER_FILM)])
    v = per_sample(eng, P, "float32", rho, tau)[0]
    vr = per_sample(eng, Q[rep], "float32", rho[rep], tau[rep])[0]
    vn = per_sample(eng, nul, "float32", rho[:2], tau[:2])[0]
    return dict(P=P, Q=Q, rep=rep, rho=rho, tau=tau, v=v, vr=vr, vn=vn)


@pytest.mark.gpu
def test_per_sample_vs_oracle(oracle, tables, chunk1):
    """both thresholds' two sides, wet and dry, at the headline kernel's per-sample bound"""
    c = chunk1
    P = np.concatenate([c["P"], c["Q"][c["rep"]]])
    rho, tau = np.concatenate([c["rho"], c["rho"][c["rep"]]]), np.concatenate([c["tau"], c["tau"][c["rep"]]])
    g = G.oracle_grid(oracle, tables, P, rho, tau)
    g["P"] = P
    got = np.concatenate([c["v"], c["vr"]])
    assert got.dtype == np.float32 and np.isfinite(got).all() and np.isfinite(g["sum"]).all()
    x = G.rel(got, g["sum"]) / G.bound32(g)
    r, b = np.unravel_index(np.argmax(x), x.shape)
    print("worst error / bound %.3f at row %d band %d" % (x[r, b], r, b))
    assert x.max() <= 1.0, (int(r), int(b), float(G.rel(got, g["sum"])[r, b]), float(G.bound32(g)[r, b]))


@pytest.fixture(scope="module")
def staged(chunk1, tmp_path_factory):
    """the four SPART_CHUNK = 32 launches of the child process: per-chunk sums of the mixed rows (common, general) and of the
    one-row-among-nulls stages (common, general)"""
    c = chunk1
    d = tmp_path_factory.mktemp("diet3")
    inp, out = str(d / "rows.npz"), str(d / "sums.npz")
    DC, DG = direct_rows(c["P"])
    rho_d, tau_d = np.tile(c["rho"][:SUB], SUB), np.tile(c["tau"][:SUB], SUB)      # (position i: row i's thermal pair)
    np.savez(inp, mixed_common=c["P"], mixed_general=c["Q"], direct_common=DC, direct_general=DG, rho=c["rho"], tau=c["tau"],
             rho_d=rho_d, tau_d=tau_d)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), inp, out],
                       env=dict(os.environ, SPART_CHUNK=str(SUB)), timeout=330)
    assert r.returncode == 0, r.returncode
    return dict(np.load(out))


@pytest.mark.gpu
def test_mixed_stages_equal_their_samples(chunk1, staged):
    """per-chunk sums of mixed stages == sequential sums of the rows' own chunk-1 values, in the common-case body and --
    one sample of each stage with another film -- in the general body"""
    from test_gpu_band_sums import _check_chunks
    c = chunk1
    assert staged["mixed_common"].shape == (STAGES, G.NEV)
    _check_chunks(staged["mixed_common"], c["v"], SUB, "common")
    vg = c["v"].copy()
    vg[c["rep"]] = c["vr"]
    _check_chunks(staged["mixed_general"], vg, SUB, "general")


@pytest.mark.gpu
def test_two_bodies_bit_equal_on_shared_samples(chunk1, staged):
    """a stage of one row among 31 rows that sum to exactly zero: the chunk's sum is the row's value.  The common-case body,
    the general body (one null row has another film) and the row's own chunk-1 run give the same bits in all 2002 bands"""
    c = chunk1
    assert np.all(c["vn"] == 0.0), "the null rows must sum to exactly 0"
    a, b = staged["direct_common"], staged["direct_general"]
    assert a.shape == b.shape == (SUB, G.NEV)
    assert np.array_equal(a, b)
    assert np.array_equal(a, c["v"][:SUB])


if __name__ == "__main__":                        # the child of `staged` (SPART_CHUNK = 32)
    for p in (os.path.join(ROOT, "spart-python_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    from spart_amd import get_engine
    from test_gpu_band_sums import chunk_block
    z = np.load(sys.argv[1])
    e = get_engine("Sentinel2A-MSI", 0)
    res = {}
    for name in ("mixed_common", "mixed_general", "direct_common", "direct_general"):
        P = z[name]
        rho, tau = (z["rho_d"], z["tau_d"]) if name.startswith("direct") else (z["rho"], z["tau"])
        blk, _, nchunk = chunk_block(e, torch.as_tensor(P.T.copy(), device="cuda:0"), "float32", rho, tau)
        assert nchunk == len(P) // SUB, nchunk
        res[name] = blk
    np.savez(sys.argv[2], **res)
