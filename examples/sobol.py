"""Which parameters can a retrieval free?  Sobol' first-order and total sensitivity indices of the Sentinel-2A R_TOC bands to
LAI, Cab, Cw, Cdm, N and LIDFa over their ranges, at three sun zenith angles, with their jackknife standard errors
(spart_amd.sobol; the three angles are three sites of ONE call).  Needs an MI355X.

    python examples/sobol.py [N]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import sobol, workloads  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
free = ["LAI", "Cab", "Cw", "Cdm", "N", "LIDFa"]
tts = [20.0, 40.0, 60.0]
sites = np.repeat(workloads.default_row(), len(tts), axis=0)
sites[:, workloads.PARAM_NAMES.index("tts")] = tts
res = sobol(sites.T, "Sentinel2A-MSI", free, N=N, column="R_TOC")
print(f"N = {N} base samples, {N * (len(free) + 2)} forward rows per site; total index ST +- its standard error (first-order S1)")
for m, angle in enumerate(tts):
    print(f"\ntts = {angle:g} deg" + " " * 6 + "".join(f"{n:>22s}" for n in res["names"]))
    for j in range(res["ST"].shape[1]):
        cells = "".join(f"  {res['ST'][m, j, f]:6.3f} +-{res['ST_se'][m, j, f]:6.3f} ({res['S1'][m, j, f]:5.2f})" for f in range(len(free)))
        print(f"band {j:2d}  sd {np.sqrt(res['var'][m, j]):7.4f}{cells}")
top = np.argmax(res["ST"], axis=2)
print("\nthe parameter with the largest total index per band:", [[res["names"][f] for f in row] for row in top])
