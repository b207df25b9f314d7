"""A LUT inversion followed by the refinement every LUT user runs next: the best row of each observation starts a bounded
Levenberg-Marquardt fit of a few parameters, the others held at the row's values -- one device-resident call.  Needs an MI355X.

    python examples/refine.py [rows] [directory]
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import generate_lut, noise_weights, refine, retrieve, workloads  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(tempfile.gettempdir(), "spart_lut_f64")
sensor, names = "Sentinel2A-MSI", ["LAI", "Cab", "Cw", "Cdm"]
cols = [workloads.PARAM_NAMES.index(n) for n in names]

# a canopy whose other parameters are known (the fixture defaults): the LUT varies the four retrieved ones only
rng = np.random.default_rng(1)
lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
P = np.repeat(workloads.default_row(), rows, axis=0)
P[:, cols] = rng.uniform(lo, hi, (rows, len(names)))
generate_lut(P, sensor, out, dtype="float64")

# 2048 "observed" spectra: the model at parameters that are NOT LUT rows, 0.5 % noise
truth = np.repeat(workloads.default_row(), 2048, axis=0)
truth[:, cols] = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (2048, len(names)))
clean = refine(truth.T, np.zeros((2048, 13)), sensor, names, n_iter=0)["y"]        # n_iter = 0: one forward evaluation
obs = clean * (1 + 0.005 * rng.standard_normal(clean.shape))

res = retrieve(out, obs, 10, refine=names, refine_opts={"n_iter": 8})
span = hi - lo
err_lut = np.median(np.abs(P[res["idx"][:, 0]][:, cols] - truth[:, cols]) / span, axis=0)
err_fit = np.median(np.abs(res["refined"] - truth[:, cols]) / span, axis=0)
print(rows, "rows; median |error| / range of", names)
print("  nearest LUT row:", np.round(err_lut, 4))
print("  refined        :", np.round(err_fit, 4), " median 1-sigma / range:", np.round(np.nanmedian(res["refined_std"], axis=0) / span, 4))
print("cost went down for", float((res["refined_cost"] < res["refined_cost0"]).mean()) * 100, "% of the spectra; median cost ratio",
      float(np.median(res["refined_cost"] / res["refined_cost0"])))
assert (res["refined_cost"] <= res["refined_cost0"]).all()

# the same fit as optimal estimation: the mean and spread of the k rows found become a Gaussian prior on the four parameters
# (knn_prior), the cost gains its term and refined_std is the linearised posterior 1-sigma
oe = retrieve(out, obs, 10, refine=names, refine_opts={"n_iter": 8, "prior": "knn"})
err_oe = np.median(np.abs(oe["refined"] - truth[:, cols]) / span, axis=0)
print("  with knn prior :", np.round(err_oe, 4), " median 1-sigma / range:", np.round(np.nanmedian(oe["refined_std"], axis=0) / span, 4))
assert (oe["refined_cost"] <= oe["refined_cost0"]).all()

# what the fit knows beyond one sigma per parameter: with the noise model as weights (1 / sigma^2 of the 0.5 % noise),
# "posterior": True adds the full posterior covariance, the averaging kernel and its trace, the degrees of freedom for signal
w = noise_weights(obs, 1e-4, 0.005)
a, b = names.index("LAI"), names.index("Cdm")
for label, prior in (("no prior ", None), ("knn prior", "knn")):
    opts = {"n_iter": 8, "posterior": True, **({"prior": prior} if prior else {})}
    r = retrieve(out, obs, 10, weights=w, refine=names, refine_opts=opts)
    cov, ok = r["refined_cov"], np.isfinite(r["refined_dfs"])
    corr = cov[ok, a, b] / np.sqrt(cov[ok, a, a] * cov[ok, b, b])
    print(f"  {label}: median LAI / Cdm correlation {np.median(corr):+.3f}, degrees of freedom for signal: median "
          f"{np.median(r['refined_dfs'][ok]):.3f} of {len(names)} (min {r['refined_dfs'][ok].min():.3f})")
    assert ok.mean() > 0.9 and (np.abs(corr) <= 1 + 1e-9).all() and (r["refined_dfs"][ok] <= len(names) + 1e-6).all()
print("refined", len(names), "parameters of", obs.shape[0], "spectra")
