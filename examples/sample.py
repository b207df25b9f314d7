"""The shape of a retrieval's posterior, not just a point and a sigma: Sentinel-2A R_TOC of a dense canopy (LAI near its upper
bound, where the signal saturates) and of a sparse one, 2 % noise, LAI / Cab / Cw / Cdm free.  spart_amd.refine gives x +- std, a
symmetric Gaussian that knows nothing of the bounds; spart_amd.sample walks an ensemble through the posterior itself and gives
the median and the 5 - 95 % interval (spart_sample; chain_summary for the quantiles, R^ and the effective sample size).
Needs an MI355X.

    python examples/sample.py [n_steps]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
import spart_amd  # noqa: E402
from spart_amd import workloads  # noqa: E402

n_steps = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
sensor, free = "Sentinel2A-MSI", ["LAI", "Cab", "Cw", "Cdm"]
truth = np.repeat(workloads.default_row(), 2, axis=0)
truth[:, workloads.PARAM_NAMES.index("LAI")] = [6.5, 0.8]
rng = np.random.default_rng(0)
eng = spart_amd.get_engine(sensor, 0)
clean = eng.run(eng.torch.as_tensor(truth.T.copy(), device=eng.device), "float64")["R_TOC"].cpu().numpy()
sigma = 0.02 * np.maximum(clean, 0.01)
obs = clean + sigma * rng.normal(size=sigma.shape)
w = 1.0 / sigma ** 2
start = truth.copy()
start[:, workloads.PARAM_NAMES.index("LAI")] = [5.0, 1.5]
fit = spart_amd.refine(start.T, obs, sensor, free, weights=w, n_iter=20)
rows = start.copy()
rows[:, [workloads.PARAM_NAMES.index(n) for n in free]] = fit["x"]
res = spart_amd.sample(rows.T, obs, sensor, free, weights=w, n_steps=n_steps, walkers=16, chain=True, seed=1)
s = spart_amd.chain_summary(res["chain"])
print(f"{n_steps} steps of 16 walkers, the second half kept; acceptance {res['accept_fraction'].round(2)}")
for m, what in enumerate(("dense canopy", "sparse canopy")):
    print(f"\n{what}" + " " * 9 + "truth      refine x, its std        sample median [5 %, 95 %]      R^   ess")
    for f, n in enumerate(free):
        t = truth[m, workloads.PARAM_NAMES.index(n)]
        q = s["quantiles"][m, :, f]
        print(f"  {n:>4s} {t:14.4g}   {fit['x'][m, f]:9.4g} +- {fit['std'][m, f]:<9.3g}   {q[1]:9.4g} [{q[0]:.4g}, {q[2]:.4g}]"
              f"   {s['rhat'][m, f]:5.2f} {s['ess'][m, f]:6.0f}")
hi = workloads.RANGES["LAI"][1]
print(f"\nLAI of the dense canopy: refine's 90 % interval reaches {fit['x'][0, 0] + 1.645 * fit['std'][0, 0]:.2f}, the bound is {hi:g}; "
      f"the sampled one ends at {s['quantiles'][0, 2, 0]:.2f}")
