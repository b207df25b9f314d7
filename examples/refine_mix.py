"""Mixed pixels -- a crop and the bare soil between its rows -- fitted once as ONE homogeneous canopy (refine, which can only
answer with too small an LAI) and once as a linear mixture of two components with the cover fraction as an unknown
(refine_mix): the soil brightness B is shared by both components, LAI and Cab belong to the crop alone.  Needs an MI355X.

    python examples/refine_mix.py [pixels] [sensor]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import workloads  # noqa: E402

SHARED, LOCAL = ["B"], ["LAI", "Cab"]
ACTIVE = {"LAI": [0], "Cab": [0]}                 # component 0 is the crop, component 1 the bare soil
SOIL_LAI = 0.01


def twin(M, seed=4):
    """-> (truth (2, M, 27), fraction (M,) of the crop, start (2, M, 27), start fraction (M,)): crops of LAI 1 ... 5 and
    Cab 20 ... 60 over soils of brightness 0.3 ... 0.8, cover 0.2 ... 0.8; the start is within 10 % of each range of the truth
    and within 0.15 of the fraction"""
    rng = np.random.default_rng(seed)
    names = SHARED + LOCAL
    cols = [workloads.PARAM_NAMES.index(n) for n in names]
    lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
    truth = np.repeat(np.repeat(workloads.default_row(), M, axis=0)[None], 2, axis=0)
    truth[:, :, cols[0]] = rng.uniform(0.3, 0.8, M)[None]
    truth[0, :, cols[1]] = rng.uniform(1.0, 5.0, M)
    truth[0, :, cols[2]] = rng.uniform(20.0, 60.0, M)
    truth[1, :, cols[1]] = SOIL_LAI
    frac = rng.uniform(0.2, 0.8, M)
    start = truth.copy()
    move = rng.uniform(-0.1, 0.1, (M, 3)) * (hi - lo)
    start[:, :, cols[0]] = np.clip(truth[0, :, cols[0]] + move[:, 0], lo[0], hi[0])[None]
    for k in (1, 2):
        start[0, :, cols[k]] = np.clip(truth[0, :, cols[k]] + move[:, k], lo[k], hi[k])
    return truth, frac, start, np.clip(frac + rng.uniform(-0.15, 0.15, M), 0.0, 1.0)


def observe(truth, frac, sensor, noise=0.005, seed=5):
    """the mixed column at the truth (given fractions, n_iter = 0 is one forward evaluation) with relative noise"""
    from spart_amd import get_engine, refine_mix
    M, nb = frac.size, get_engine(sensor, None).nb
    clean = refine_mix(np.moveaxis(truth, 2, 0), np.zeros((M, nb)), sensor, SHARED, LOCAL, active=ACTIVE, n_iter=0,
                       fractions=np.stack([frac, 1.0 - frac], axis=1), fit_fractions=False)["y"]
    return clean * (1 + noise * np.random.default_rng(seed).standard_normal(clean.shape))


def main(M, sensor):
    from spart_amd import refine, refine_mix
    truth, frac, start, frac0 = twin(M)
    obs = observe(truth, frac, sensor)
    single = refine(start[0].T, obs, sensor, SHARED + LOCAL, n_iter=10)
    mix = refine_mix(np.moveaxis(start, 2, 0), obs, sensor, SHARED, LOCAL, active=ACTIVE,
                     fractions=np.stack([frac0, 1.0 - frac0], axis=1), n_iter=10)
    lai = workloads.PARAM_NAMES.index("LAI")
    print(M, "mixed crop / bare-soil pixels on", sensor)
    print(f"  one canopy : median cost {np.median(single['cost']):.3e}   median LAI error "
          f"{np.median(np.abs(single['x'][:, 1] - truth[0, :, lai])):.3f}")
    print(f"  mixture    : median cost {np.median(mix['cost']):.3e}   median LAI error "
          f"{np.median(np.abs(mix['local'][:, 0, 0] - truth[0, :, lai])):.3f}")
    print(f"  cover fraction: median |error| {np.median(np.abs(frac0 - frac)):.4f} at the start, "
          f"{np.median(np.abs(mix['fractions'][:, 0] - frac)):.4f} after the fit "
          f"(median 1-sigma {np.nanmedian(mix['fractions_std'][:, 0]):.4f})")
    print("fitted", M, "pixels as a mixture of 2 components")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2048, sys.argv[2] if len(sys.argv) > 2 else "Sentinel2A-MSI")
