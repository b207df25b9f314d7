"""One aerosol load per 8 x 8 window of a scene, one LAI and Cab per pixel: the per-pixel fit with aot550 free trades aerosol
against canopy, refine_tiles fits ONE aot550 per window against all of its pixels' top-of-atmosphere reflectances.  Needs an
MI355X.

    python examples/refine_tiles.py [height] [width]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import refine, refine_tiles, window_tiles, workloads  # noqa: E402

H = int(sys.argv[1]) if len(sys.argv) > 1 else 64
W = int(sys.argv[2]) if len(sys.argv) > 2 else H
sensor, shared, local = "Sentinel2A-MSI", ["aot550"], ["LAI", "Cab"]
ia = workloads.PARAM_NAMES.index("aot550")
il = [workloads.PARAM_NAMES.index(n) for n in local]
M = H * W

# the scene in window order, every window's pixels contiguous: pixel k of the arrays below is raster pixel order[k]
order, tile_start = window_tiles(H, W, 8)
T = tile_start.size - 1
tile_of = np.repeat(np.arange(T), np.diff(tile_start))
rng = np.random.default_rng(4)
lo, hi = (np.array([workloads.RANGES[n][i] for n in local]) for i in (0, 1))
truth = np.repeat(workloads.default_row(), M, axis=0)
truth[:, il] = rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (M, 2))
truth[:, ia] = rng.uniform(0.05, 0.5, T)[tile_of]
start = truth.copy()
start[:, il] = 0.5 * (lo + hi)
start[:, ia] = 0.25

# noisy R_TOA: the model at the truth (n_iter = 0 is one forward evaluation), 1 % noise
clean = refine(truth.T, np.zeros((M, 13)), sensor, local, column="R_TOA", n_iter=0)["y"]
obs = clean * (1 + 0.01 * rng.standard_normal(clean.shape))

alone = refine(start.T, obs, sensor, local + shared, column="R_TOA", n_iter=10)["x"]                     # (M, 3)
joint = refine_tiles(start.T, obs, sensor, shared, local, tile_start=tile_start, column="R_TOA", n_iter=10)
rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))     # noqa: E731
print(f"{H} x {W} pixels in {T} windows; RMS error of LAI and aot550")
print(f"  per pixel, aot550 free : {rms(alone[:, 0], truth[:, il[0]]):.4f}  {rms(alone[:, 2], truth[:, ia]):.4f}")
print(f"  aot550 per window      : {rms(joint['local'][:, 0], truth[:, il[0]]):.4f}  {rms(joint['shared'][tile_of, 0], truth[:, ia]):.4f}")
print("fitted 1 shared parameter of", T, "tiles and 2 local parameters of", M, "pixels")
