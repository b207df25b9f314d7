"""Rate of spart_lut_topk_obs_weights (Engine.lut_topk with (M, nb) weights) on a LUT of real hyperspectral spectra, next to
the shared-weights wide call (spart_lut_topk_wide) on the same data.

    python tools/lut_obs_weights_rate.py [--rows 1048576] [--obs 16384] [--wide-rows 262144] [--wide-obs 4096] [--reps 3]

Workloads: those of tools/lut_wide_rate.py (211-band sensor: 1M rows x 16 384 observations; 2001-band sensor: 262 144 x 4 096),
observations = LUT rows x (1 + 0.02 N(0, 1)).  Weights: noise_weights(obs, rel_sigma=0.02) with about 5 % of the entries masked
at random (the observation set to NaN there); the shared-weights call gets the column means of those weights and the
unmasked observations.  Per (nb, dtype, k): median call time over --reps calls of both, and the obs-weights call's stats
(brute-forced observations, candidate tiles: mean and maximum per observation, the largest Nbound_m).  One JSON line per case.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(torch, f, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 3) for t in ts]


def run_case(torch, eng, lut, obs, obs_masked, W, w_shared, dtype, k, reps):
    td = torch.float32 if dtype == "float32" else torch.float64
    L, O, Om = lut.to(td).contiguous(), obs.to(td).contiguous(), obs_masked.to(td).contiguous()
    Wt, ws = W.to(td).contiguous(), w_shared.to(td).contiguous()
    B, nb = L.shape
    M = O.shape[0]
    _, _, st = eng.lut_topk(L, Om, k, weights=Wt, dtype=dtype, stats=True)            # warm-up + stats
    ms, all_ms = timed(torch, lambda: eng.lut_topk(L, Om, k, weights=Wt, dtype=dtype), reps)
    _, _, sw = eng.lut_topk(L, O, k, weights=ws, dtype=dtype, stats=True)
    ms_w, _ = timed(torch, lambda: eng.lut_topk(L, O, k, weights=ws, dtype=dtype), reps)
    return {"nb": nb, "dtype": dtype, "k": k, "B": B, "M": M, "call_ms": round(ms, 3), "call_ms_all": all_ms,
            "tflops_per_call": round(2.0 * (2 * nb + 1) * B * M / (ms * 1e-3) / 1e12, 2),
            "n_brute_force": st["brute_force"], "mean_candidate_tiles": round(st["candidate_tiles"] / M, 2),
            "max_candidate_tiles": st["max_candidate_tiles"], "nbound": st["nbound"],
            "shared_weights_call_ms": round(ms_w, 3), "ratio_to_shared": round(ms / ms_w, 3),
            "shared_n_brute_force": sw["brute_force"], "shared_mean_candidate_tiles": round(sw["candidate_tiles"] / M, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--obs", type=int, default=16384)
    ap.add_argument("--wide-rows", type=int, default=1 << 18)
    ap.add_argument("--wide-obs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mask", type=float, default=0.05)
    ap.add_argument("--skip-2001", action="store_true")
    a = ap.parse_args()
    import torch
    from lut_wide_rate import sensor_1nm, workload
    from make_hyperspectral import sensorinfo_from_npz
    from spart_amd import get_engine, noise_weights
    eng = get_engine(None, 0)
    si211 = sensorinfo_from_npz(dict(np.load(os.path.join(ROOT, "tests", "golden", "hyperspectral.npz"))))
    cases = [(si211, a.rows, a.obs)] + ([] if a.skip_2001 else [(sensor_1nm(), a.wide_rows, a.wide_obs)])
    for si, B, M in cases:
        lut, obs = workload(torch, si, B, M, seed=2024)
        rng = np.random.default_rng(7)
        o = obs.cpu().numpy()
        o[rng.random(o.shape) < a.mask] = np.nan
        W = torch.as_tensor(noise_weights(o, rel_sigma=0.02), device="cuda:0")
        obs_masked = torch.as_tensor(o, device="cuda:0")
        w_shared = W.mean(dim=0)
        for dtype in ("float32", "float64"):
            for k in (1, 10):
                print(json.dumps(run_case(torch, eng, lut, obs, obs_masked, W, w_shared, dtype, k, a.reps)), flush=True)
        del lut, obs, obs_masked, W
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
