"""PROSPECT inversion: 256 simulated leaves with 1 % noise, 400 - 449 nm masked, fitted for Cab, Cca, Cw, Cdm and N, once from
reflectance and transmittance and once from reflectance alone.  Needs an MI355X.

    python examples/refine_leaf.py [leaves]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import get_engine, refine_leaf, workloads  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 256
free = ["Cab", "Cca", "Cw", "Cdm", "N"]
rng = np.random.default_rng(0)
truth = workloads.lhs_params(M, "leaf")[:, :9]                   # BASELINE config 2's leaves: Cab, Cdm, Cw, Cs, Cca, Cant, N, PROT, CBC
refl, tran, _ = (None if t is None else t.cpu().numpy() for t in get_engine(None).prospect(list(truth.T), outputs=("refl", "tran")))
sigma = 0.01
obs_r = refl * (1 + sigma * rng.standard_normal(refl.shape))
obs_t = tran * (1 + sigma * rng.standard_normal(tran.shape))
# weights 1 / sigma^2 make `std` the linearised 1-sigma; weight 0 masks a band, and the measurement may be NaN there
w_r, w_t = 1.0 / (sigma * refl) ** 2, 1.0 / (sigma * tran) ** 2
for w, obs in ((w_r, obs_r), (w_t, obs_t)):
    w[:, :50] = 0.0
    obs[:, :50] = np.nan

start = truth.copy()                                             # what is not fitted is known; what is fitted starts mid-range
cols = [workloads.PARAM_NAMES.index(n) for n in free]
lo, hi = (np.array([workloads.RANGES[n][k] for n in free], dtype=np.float64) for k in (0, 1))
start[:, cols] = 0.5 * (lo + hi)
for title, t, wt in (("reflectance and transmittance", obs_t, w_t), ("reflectance alone", None, None)):
    res = refine_leaf(start.T, obs_r, t, free=free, weights_refl=w_r, weights_tran=wt, n_iter=20)
    rmse = np.sqrt(np.mean((res["x"] - truth[:, cols]) ** 2, axis=0))
    print(f"{title}: {int((res['n_accept'] >= 0).sum())} of {M} leaves fitted, median cost / cost0 "
          f"{np.median(res['cost'] / res['cost0']):.2e}")
    for j, n in enumerate(res["names"]):
        print(f"  {n:4s} RMSE {rmse[j]:.4g}   median std {np.median(res['std'][:, j]):.4g}   (range {lo[j]:g} ... {hi[j]:g})")
