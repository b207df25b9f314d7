"""A season of 24 Sentinel-2A dates of a handful of pixels, three consecutive dates under cloud: LAI and Cab follow a smooth
curve, the leaf angle parameter LIDFa is one value per pixel.  Fitted date by date (refine), as a tile without a tie between the
dates (refine_series with no smoothing, which is refine_tiles) and as a series with a first-difference smoothness prior.  The
date-by-date and the untied fit leave the cloudy dates at their start; the series fills the gap from its neighbours.  Needs an
MI355X.

    python examples/refine_series.py [pixels]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import date_links, refine, refine_series, workloads  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = 24
sensor, shared, local = "Sentinel2A-MSI", ["LIDFa"], ["LAI", "Cab"]
idx = {n: workloads.PARAM_NAMES.index(n) for n in shared + local + ["DOY"]}
M = N * T
rng = np.random.default_rng(7)
series_start = np.arange(0, M + 1, T)
days = np.tile(100.0 + 5.0 * np.arange(T), N) + rng.uniform(-1, 1, M)              # a five-day revisit, jittered
phase = (np.tile(np.arange(T), N) + 0.5) / T

# the truth: a season's bell in LAI, Cab following it, one leaf angle per pixel, the acquisition day of every date
truth = np.repeat(workloads.default_row(), M, axis=0)
peak = np.repeat(rng.uniform(3.0, 6.0, N), T)
truth[:, idx["LAI"]] = 0.5 + peak * np.sin(np.pi * phase) ** 2
truth[:, idx["Cab"]] = 25.0 + 30.0 * np.sin(np.pi * phase) ** 2
truth[:, idx["LIDFa"]] = np.repeat(rng.uniform(-0.3, 0.3, N), T)
truth[:, idx["DOY"]] = days
start = truth.copy()
start[:, idx["LAI"]], start[:, idx["Cab"]], start[:, idx["LIDFa"]] = 2.0, 40.0, 0.0

clean = refine(truth.T, np.zeros((M, 13)), sensor, local, n_iter=0)["y"]            # (n_iter = 0 is one forward evaluation)
obs = clean * (1 + 0.02 * rng.standard_normal(clean.shape))
cloud = np.tile((np.arange(T) >= 10) & (np.arange(T) < 13), N)                        # three consecutive dates
weights = np.where(cloud[:, None], 0.0, 1.0 / (0.02 * np.maximum(clean, 0.01)) ** 2)
obs[cloud] = np.nan

by_date = refine(start.T, np.where(cloud[:, None], 0.0, obs), sensor, local, weights=weights, n_iter=10)["x"][:, 0]
kw = dict(series_start=series_start, weights=weights, n_iter=10)
untied = refine_series(start.T, obs, sensor, shared, local, **kw)["local"][:, 0]
series = refine_series(start.T, obs, sensor, shared, local, smooth={"LAI": 0.15, "Cab": 1.5}, link=date_links(days, series_start),
                       **kw)["local"][:, 0]
lai = truth[:, idx["LAI"]]
rms = lambda a, pick: float(np.sqrt(np.mean((a[pick] - lai[pick]) ** 2)))     # noqa: E731
print(f"{N} pixels x {T} dates, dates 10 ... 12 masked; RMS LAI error over the gap / over the clear dates")
for name, x in (("date by date", by_date), ("tile, no tie", untied), ("series", series)):
    print(f"  {name:13s}: {rms(x, cloud):.3f}  {rms(x, ~cloud):.3f}")
print("fitted", T, "dates of", N, "pixels three ways")
