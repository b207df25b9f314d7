"""Generate tests/golden/srf.npz from the REAL reference (run in the build container only).

    python tests/golden/make_srf.py

The SRF-convolved sensor columns as the reference's own pieces give them: for the default row and 8 Latin-hypercube rows, and
for Sentinel-2A, Landsat 7, Landsat 8 and MODIS with their tables as packaged, SPART(...).run() is evaluated, the four canopy
spectra it leaves in ``canopyopt`` are taken through the reference's own
``calculate_spectral_convolution(spectral.wlS[:, None], rad.x, sensorinfo)`` (SPART.py:358-396), and the TOC -> TOA formulas
(SPART.py:243-252, restated in tests/helpers/srf_numpy.py) are applied with the object's own ``atmopt`` and ``_La``.

Stored (data only; nothing of the reference's source): P (9, 27) and, per sensor,
  <sensor>/rso_srf, rdo_srf, rsd_srf, rdd_srf, R_TOC_srf, R_TOA_srf, L_TOA_srf  (9, nb) float64.
Every stored value is finite (asserted).
"""
import io
import os
import sys
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
OUT = os.path.join(HERE, "srf.npz")
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd", "spart_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import workloads  # noqa: E402  (a plain module import: it does not pull in the package / HIP lib)
from helpers import srf_numpy  # noqa: E402

SENSORS = ("Sentinel2A-MSI", "LANDSAT7-ETM", "LANDSAT8-OLI", "TerraAqua-MODIS")
SMAC_FIELDS = ("Ta_s", "Ta_o", "Tg", "Ra_dd", "Ra_so", "Ta_ss", "Ta_sd", "Ta_oo", "Ta_do")


def main():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from _ref_import import import_reference
    SPART = import_reference()
    from SPART.SPART import calculate_spectral_convolution
    from SPART.bsm import SoilParameters
    from SPART.prospect_5d import LeafBiology
    from SPART.sailh import Angles, CanopyStructure
    from SPART.smac import AtmosphericProperties
    P = np.concatenate([workloads.default_row(), workloads.lhs_params(8, "full", seed=358)], axis=0)
    out = {"P": P}
    for sensor in SENSORS:
        res = {k: [] for k in ("rso_srf", "rdo_srf", "rsd_srf", "rdd_srf", "R_TOC_srf", "R_TOA_srf", "L_TOA_srf")}
        for row in P:
            leaf, soil, can, ang, atm, doy = row[0:9], row[9:15], row[15:19], row[19:22], row[22:26], row[26]
            with redirect_stdout(io.StringIO()):
                sp = SPART.SPART(SoilParameters(*soil), LeafBiology(*leaf[:7], PROT=leaf[7], CBC=leaf[8]),
                                 CanopyStructure(*can), AtmosphericProperties(atm[0], atm[1], atm[2], Pa=atm[3]),
                                 Angles(*ang), sensor, int(doy))
                sp.run()
            rad = sp.canopyopt
            conv = {x: np.asarray(calculate_spectral_convolution(sp.spectral.wlS[:, None], getattr(rad, x), sp.sensorinfo),
                                  dtype=np.float64).reshape(1, -1) for x in ("rso", "rdo", "rsd", "rdd")}
            at = {f: np.asarray(getattr(sp.atmopt, f), dtype=np.float64).reshape(1, -1) for f in SMAC_FIELDS}
            La = np.asarray(sp._La, dtype=np.float64).reshape(1, -1)
            rtoc, rtoa, ltoa = srf_numpy.toc_to_toa(at, conv["rso"], conv["rdo"], conv["rsd"], conv["rdd"], La)
            for x in ("rso", "rdo", "rsd", "rdd"):
                res[x + "_srf"].append(conv[x][0])
            for k, v in (("R_TOC_srf", rtoc), ("R_TOA_srf", rtoa), ("L_TOA_srf", ltoa)):
                res[k].append(v[0])
        for k, v in res.items():
            a = np.array(v, dtype=np.float64)
            assert np.isfinite(a).all(), (sensor, k)
            out[f"{sensor}/{k}"] = a
    np.savez_compressed(OUT, **out)
    print(OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
