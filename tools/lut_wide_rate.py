"""Rate of spart_lut_topk_wide (Engine.lut_topk / lut_nearest above 31 bands) on a LUT of real hyperspectral spectra.

    python tools/lut_wide_rate.py [--rows 1048576] [--obs 16384] [--wide-rows 262144] [--wide-obs 4096] [--reps 3]

Workloads: the 211-band sensor of tests/golden/hyperspectral.npz (10 nm, 400-2500 nm) and a 2001-band sensor at every integer
nm (Gaussian SRFs, Sentinel-2A SMAC coefficients of the nearest band).  The LUT is R_TOC of LHS parameters (NaN entries set to
0.5), the observations are LUT rows x (1 + 0.02 N(0, 1)).  Per (nb, dtype, k): the median call time over --reps calls, the
filter's stats (brute-forced observations, candidate tiles: mean and maximum per observation), and 2 (nb + 1) B M / call time.
The scan kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of this script (k_lutw_gemm<.., false>);
profiles/lut_wide_rate.txt holds both.  Prints one JSON line per case.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

F32_MATRIX_PEAK_TF = 157.3


def sensor_1nm():
    from spart_amd import tables
    s2 = tables.load_sensor_info("Sentinel2A-MSI")
    c = np.arange(400.0, 2401.0)
    s2c = np.asarray(s2["wl_smac"], dtype=np.float64).reshape(-1)
    near = np.argmin(np.abs(c[:, None] - s2c[None, :]), axis=1)
    offs = np.arange(-15.0, 16.0, 1.0)
    p = np.exp(-0.5 * (offs[:, None] / (10.0 / 2.3548200450309493)) ** 2) * np.ones((1, c.size))
    return {"wl_smac": c[:, None], "band_id_smac": [f"N{int(x)}" for x in c],
            "SMAC_coef": {n: np.asarray(v, dtype=np.float64).reshape(1, -1)[:, near].copy() for n, v in s2["SMAC_coef"].items()},
            "wl_srf_smac": c[None, :] + offs[:, None], "p_srf_smac": p / p.sum(axis=0, keepdims=True)}


def workload(torch, si, B, M, seed):
    from spart_amd import get_engine, workloads
    eng = get_engine(None, 0, sensor_info=si)
    P = workloads.lhs_params(B, "full", seed=seed)
    lut = torch.empty((B, eng.nb), dtype=torch.float64, device="cuda:0")
    step = 1 << 17
    for r0 in range(0, B, step):
        Pd = torch.as_tensor(P[r0:r0 + step].T.copy(), device="cuda:0")
        lut[r0:r0 + step] = eng.run(Pd, "float64", prune=True)["R_TOC"]
    lut = torch.nan_to_num(lut, nan=0.5)
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    pick = torch.randint(0, B, (M,), generator=g, device="cuda:0")
    obs = lut[pick] * (1 + 0.02 * torch.randn((M, eng.nb), generator=g, device="cuda:0", dtype=torch.float64))
    return lut, obs


def run_case(torch, eng, lut, obs, dtype, k, reps):
    td = torch.float32 if dtype == "float32" else torch.float64
    L, O = lut.to(td).contiguous(), obs.to(td).contiguous()
    B, nb = L.shape
    M = O.shape[0]
    _, _, st = eng.lut_topk(L, O, k, dtype=dtype, stats=True)            # warm-up + stats
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.lut_topk(L, O, k, dtype=dtype)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = float(np.median(ts))
    tf = 2.0 * (nb + 1) * B * M / (ms * 1e-3) / 1e12
    return {"nb": nb, "dtype": dtype, "k": k, "B": B, "M": M, "call_ms": round(ms, 3), "call_ms_all": [round(t, 3) for t in ts],
            "tflops_per_call": round(tf, 2), "share_of_f32_matrix_peak": round(tf / F32_MATRIX_PEAK_TF, 4),
            "n_brute_force": st["brute_force"], "brute_force_share": round(st["brute_force"] / M, 5),
            "mean_candidate_tiles": round(st["candidate_tiles"] / M, 2), "max_candidate_tiles": st["max_candidate_tiles"],
            "nmax": st["nmax"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--obs", type=int, default=16384)
    ap.add_argument("--wide-rows", type=int, default=1 << 18)
    ap.add_argument("--wide-obs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-2001", action="store_true")
    a = ap.parse_args()
    import torch
    from make_hyperspectral import sensorinfo_from_npz
    from spart_amd import get_engine
    eng = get_engine(None, 0)
    si211 = sensorinfo_from_npz(dict(np.load(os.path.join(ROOT, "tests", "golden", "hyperspectral.npz"))))
    cases = [(si211, a.rows, a.obs)] + ([] if a.skip_2001 else [(sensor_1nm(), a.wide_rows, a.wide_obs)])
    for si, B, M in cases:
        lut, obs = workload(torch, si, B, M, seed=2024)
        for dtype in ("float32", "float64"):
            for k in (1, 10):
                print(json.dumps(run_case(torch, eng, lut, obs, dtype, k, a.reps)), flush=True)
        del lut, obs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
