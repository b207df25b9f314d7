"""The float32 band kernel's two sample-loop bodies (k_bands<float, 0, 1, false>): a 32-sample stage whose samples all share
the film thickness and all have cbc = prot = 0 runs the common-case body, any other stage the general one.  A batch whose
stages mix both -- film varying in one sample of a stage, cbc or prot non-zero in one sample, PROT / CBC varying throughout --
must give the band sums of the oracle at the bound of test_gpu_thermal.test_headline_band_sums_vs_oracle.

In-process the band kernel's chunk is <= 32 samples (one stage per workgroup); a child process with SPART_CHUNK = 80 makes
every workgroup walk three stages (32, 32, 16 samples) that switch between the bodies."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_err

SPECTRA = ("rso", "rdo", "rsd", "rdd")
B = 4000
FILM, PROT, CBC, CDM = 14, 7, 8, 1


def mixed_params(B, stage_len, chunk):
    """(B, 27) rows; stage = 32-sample block of a chunk; stage kind cycles over common / one sample with another film / one
    sample with cbc, prot > 0 / PROT and CBC varying in every sample (config 5's leaf)"""
    from spart_amd import workloads
    P = workloads.lhs_params(B, "full", seed=61)
    Q = workloads.lhs_params(B, "pro", seed=62)
    r = np.arange(B)
    stage = (r // chunk) * -(-chunk // stage_len) + (r % chunk) // stage_len      # running index of the stage
    kinds = {}
    for st in np.unique(stage):
        rows = r[stage == st]
        kind = st % 4
        kinds[kind] = kinds.get(kind, 0) + 1
        if kind == 1:
            P[rows[-1], FILM] = 0.004
        elif kind == 2:
            P[rows[0], [PROT, CBC]] = Q[rows[0], [PROT, CBC]]
        elif kind == 3:
            P[rows] = Q[rows]
    assert all(kinds.get(k, 0) >= 4 for k in range(4)), kinds
    return P


def _rho_tau(B):
    rng = np.random.default_rng(63)
    return rng.uniform(0.005, 0.45, B), rng.uniform(0.005, 0.45, B)


def _reference(oracle, tables, P, rho, tau):
    ref = np.zeros(2002)
    for a in range(0, len(P), 1000):
        with np.errstate(all="ignore"):
            o = oracle.spart_run(P[a:a + 1000], "Sentinel2A-MSI", tables, pso="gl", full=True, rho_thermal=rho[a:a + 1000],
                                 tau_thermal=tau[a:a + 1000])
        ref += sum(o[k][:, :2002].sum(axis=0) for k in SPECTRA)
    return ref


def _gpu_band_sums(P, rho, tau):
    import torch
    from spart_amd import get_engine
    from test_gpu_thermal import _band_sums
    eng = get_engine("Sentinel2A-MSI", 0)
    got, nchunk = _band_sums(eng, torch.as_tensor(P.T.copy(), device="cuda:0"), "float32", rho, tau)
    return got, nchunk


@pytest.mark.gpu
def test_mixed_stages_one_stage_per_workgroup(oracle, tables):
    chunk = min(32, (B + 255) // 256)              # pick_chunk at this B
    P = mixed_params(B, min(32, chunk), chunk)
    rho, tau = _rho_tau(B)
    got, nchunk = _gpu_band_sums(P, rho, tau)
    assert nchunk == (B + chunk - 1) // chunk
    assert rel_err(got / B, _reference(oracle, tables, P, rho, tau) / B, 1e-3) < 2e-5


@pytest.mark.gpu
def test_mixed_stages_three_stages_per_workgroup(oracle, tables, tmp_path):
    P = mixed_params(B, 32, 80)
    rho, tau = _rho_tau(B)
    out = str(tmp_path / "sums.npy")
    env = dict(os.environ, SPART_CHUNK="80")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, check=True, timeout=300)
    got = np.load(out)
    assert rel_err(got / B, _reference(oracle, tables, P, rho, tau) / B, 1e-3) < 2e-5


if __name__ == "__main__":                        # the child of test_mixed_stages_three_stages_per_workgroup (SPART_CHUNK = 80)
    for p in (os.path.join(ROOT, "spart-python_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    P = mixed_params(B, 32, 80)
    rho, tau = _rho_tau(B)
    got, nchunk = _gpu_band_sums(P, rho, tau)
    assert nchunk == B // 80, nchunk
    np.save(sys.argv[1], got)
