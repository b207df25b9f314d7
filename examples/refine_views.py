"""Three looks at the same canopies -- three sun / view geometries, as the cameras of a multi-angle instrument or the overpasses
of a few days give them -- fitted one by one and then jointly: refine_views fits ONE LAI / LIDFa / Cab per pixel against all
three observations, which is what takes LAI against leaf angle out of its ill-posedness.  Needs an MI355X.

    python examples/refine_views.py [pixels]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import refine, refine_views, workloads  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
sensor, names = "Sentinel2A-MSI", ["LAI", "LIDFa", "Cab"]
cols = [workloads.PARAM_NAMES.index(n) for n in names]
geometry = [dict(tts=30.0, tto=0.0, psi=0.0), dict(tts=45.0, tto=25.0, psi=20.0), dict(tts=55.0, tto=28.0, psi=160.0)]
V = len(geometry)

# the same canopies under every geometry; the start is the middle of the box
rng = np.random.default_rng(2)
lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
truth = np.repeat(workloads.default_row(), M, axis=0)
truth[:, cols] = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), (M, len(names)))
views = np.repeat(truth[None], V, axis=0)                                   # (V, M, 27)
for v, g in enumerate(geometry):
    for k, val in g.items():
        views[v, :, workloads.PARAM_NAMES.index(k)] = val
start = views.copy()
start[:, :, cols] = 0.5 * (lo + hi)

# noisy observations (M, V, nb): the model at the truth (n_iter = 0 is one forward evaluation), 2 % noise
clean = refine_views(np.moveaxis(views, 2, 0), np.zeros((M, V, 13)), sensor, names, n_iter=0)["y"]
obs = clean * (1 + 0.02 * rng.standard_normal(clean.shape))

alone = np.stack([refine(start[v].T, obs[:, v], sensor, names, n_iter=10)["x"] for v in range(V)])      # (V, M, 3)
joint = refine_views(np.moveaxis(start, 2, 0), obs, sensor, names, n_iter=10)
print(M, "pixels,", V, "views; median |error| of", names[:2])
for v in range(V):
    print(f"  view {v} alone   :", np.round(np.median(np.abs(alone[v] - truth[:, cols]), axis=0)[:2], 4))
print("  mean of the fits:", np.round(np.median(np.abs(alone.mean(axis=0) - truth[:, cols]), axis=0)[:2], 4))
print("  joint fit       :", np.round(np.median(np.abs(joint["shared"] - truth[:, cols]), axis=0)[:2], 4),
      " median 1-sigma:", np.round(np.nanmedian(joint["shared_std"], axis=0)[:2], 4))
print("fitted", len(names), "shared parameters of", M, "pixels from", V, "views")
