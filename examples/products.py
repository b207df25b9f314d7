"""fAPAR, albedo and fCover as LUT columns: a small Sentinel-2A look-up table, its product columns (lut_products), and a
retrieval that averages the products themselves over the k nearest rows and over the likelihood-weighted posterior.
Needs an MI355X.

    python examples/products.py [rows] [directory]
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spart-python_amd"))
from spart_amd import PRODUCT_NAMES, generate_lut, load_lut, lut_products, noise_weights, products, retrieve, workloads  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(tempfile.gettempdir(), "spart_lut_products")
P = workloads.lhs_params(rows, "full")
generate_lut(P, "Sentinel2A-MSI", out, dtype="float64")
table = lut_products(out)                                       # writes products.npy (rows, 5) beside params.npy
meta, params, cols = load_lut(out)
print(meta["rows"], "rows;", dict(zip(meta["product_names"], np.round(table.mean(axis=0), 3))))

# the products of single rows, host arrays in and out (no sensor involved): the same bits as the LUT's columns
one = products(P[:4].T)
assert all(np.array_equal(one[n], table[:4, j]) for j, n in enumerate(PRODUCT_NAMES))

# 256 "observed" canopy spectra = LUT rows + 2 % noise; LAI, fAPAR and fCover from the 10 nearest rows and from the posterior
rng = np.random.default_rng(1)
pick = rng.integers(0, rows, 256)
obs = cols["R_TOC"][pick] * (1 + 0.02 * rng.standard_normal((256, cols["R_TOC"].shape[1])))
res = retrieve(out, obs, 10, column="R_TOC", weights=noise_weights(obs, rel_sigma=0.02), summary="device",
               params_cols=["LAI", "fAPAR_bs", "fCover"], bayes={"cut": 50.0, "quantiles": [0.05, 0.5, 0.95]})
truth = np.stack([params[pick, 15], table[pick, 0], table[pick, 4]], axis=1)
for j, n in enumerate(res["names"]):
    print(f"{n:9s} median |error|: k = 10 mean {np.median(np.abs(res['mean'][:, j] - truth[:, j])):.4f}, posterior mean "
          f"{np.nanmedian(np.abs(res['bayes_mean'][:, j] - truth[:, j])):.4f}; median 90 % interval width "
          f"{np.nanmedian(res['bayes_quantiles'][:, j, 2] - res['bayes_quantiles'][:, j, 0]):.4f}")
