"""What retrieve(refine=...) and retrieve_stream(refine=...) are DEFINED to return, composed in numpy of the four definitions
tools/ already holds -- nothing else: the search (tools/lut_brute_force.py: brute_force_topk_numpy, or
brute_force_topk_obs_weights_numpy for (M, nb) weights), the summary (summarise_defined), the "knn" prior (knn_prior on that
summary, numpy form) and the fit (tools/refine_defined.py).  Each of them is the bit-exact oracle of its kernel, so their
composition is an answer for the whole call that does not come from spart_amd/lut.py.

Of the package under test this file uses knn_prior and engine.prior_arrays in their numpy forms (neither touches a device) and
the list of column names; the forward model is handed in (helpers.refine_calls.forward_of on the GPU, a toy on the CPU)."""
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lut_brute_force as bf  # noqa: E402
import refine_defined as rd  # noqa: E402

NARROW_NB = 31          # above it the library takes its wide search; its checker is the eager-torch form of the same loop
REFINED = ("refined", "refined_std", "refined_cost", "refined_cost0", "refined_accepts")
_FIT = {"refined": "x", "refined_std": "std", "refined_cost": "cost", "refined_cost0": "cost0", "refined_accepts": "n_accept"}


def same(a, b):
    """equal bit for bit as numbers: shape, dtype and every element, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def weights_kind(weights, M, nb):
    if weights is None:
        return "none"
    shape = np.shape(weights)
    if shape == (M, nb):
        return "per_observation"
    assert shape == (nb,), (shape, M, nb)
    return "shared"


def search_defined(table, obs, k, weights, torch_device=None):
    """obs and weights cast to the table's dtype; the brute force of the defined cost.  ``torch_device``: above NARROW_NB bands
    the eager-torch forms of the same loops on that device (the checker of tests/test_gpu_lut_wide.py) -> numpy (idx, cost)"""
    table = np.ascontiguousarray(table)
    dt = table.dtype
    M, nb = np.shape(obs)
    o = np.ascontiguousarray(obs, dtype=dt)
    kind = weights_kind(weights, M, nb)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=dt)
    if torch_device is not None and nb > NARROW_NB and table.shape[0] > 0 and M > 0:
        import torch
        up = lambda a: torch.as_tensor(a, device=torch_device)      # noqa: E731
        if kind == "per_observation":
            idx, cost = bf.brute_force_topk_obs_weights_torch(up(table), up(o), k, up(w))
        else:
            idx, cost = bf.brute_force_topk_torch(up(table), up(o), k, None if w is None else up(w))
        return idx.cpu().numpy(), cost.cpu().numpy()
    if kind == "per_observation":
        return bf.brute_force_topk_obs_weights_numpy(table, o, k, w)
    return bf.brute_force_topk_numpy(table, o, k, w)


def prior_plan_of(names, prior):
    """{name: (mean, sigma)} -> what engine.prior_arrays takes: per free name the mean and 1.0 / (sigma * sigma), each a scalar
    or an (M,) array; a name that is not listed has weight 0"""
    mean, weight, rows = [np.float64(0.0)] * len(names), [np.float64(0.0)] * len(names), None
    for n, (mu, sigma) in prior.items():
        mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        for v in (mu, sigma):
            if v.ndim == 1:
                rows = int(v.shape[0])
        mean[names.index(n)], weight[names.index(n)] = mu, 1.0 / (sigma * sigma)
    return {"mean": mean, "weight": weight, "rows": rows}


def retrieve_defined(params, table, obs, k, weights, names, lo, hi, forward, n_iter=10, rel_step=1e-3, lambda0=1e-2, prior=None,
                     prior_floor=0.05, params_cols=None, torch_device=None):
    """params (B, 27) float64; table (B, nb) the LUT column in the LUT's dtype; obs (M, nb) and weights (None, (nb,) or (M, nb))
    as the CALLER holds them; names: the free parameters, lo / hi (F,) their bounds; forward(rows (R, 27)) -> (R, nb) float64;
    prior None, "knn" (with prior_floor) or {name: (mean, sigma)}; params_cols: the names the summary is taken over (None: all).
    -> dict idx (M, k) int64, cost (M, k) table dtype, mean / median / std (M, P) float64, count (M,) int32, refined and
    refined_std (M, F), refined_cost and refined_cost0 (M,) float64, refined_accepts (M,) int32; and start (M, F), the free
    columns of the start rows (NaN without a row), for the tests that ask whether the fit moved."""
    from spart_amd.engine import knn_prior, prior_arrays
    from spart_amd.workloads import PARAM_NAMES
    params = np.ascontiguousarray(params, dtype=np.float64)
    names = list(names)
    M, nb = np.shape(obs)
    F = len(names)
    free = [PARAM_NAMES.index(n) for n in names]
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    # the search, in the table's dtype
    idx, cost = search_defined(table, obs, k, weights, torch_device)
    # the summary of the k rows found
    cols = list(range(len(PARAM_NAMES))) if params_cols is None else [PARAM_NAMES.index(n) for n in params_cols]
    mean, median, std, count = bf.summarise_defined(params[:, cols], idx)
    out = {"idx": idx, "cost": cost, "mean": mean, "median": median, "std": std, "count": count,
           "refined": np.full((M, F), np.nan), "refined_std": np.full((M, F), np.nan), "refined_cost": np.full(M, np.nan),
           "refined_cost0": np.full(M, np.nan), "refined_accepts": np.full(M, -1, dtype=np.int32), "start": np.full((M, F), np.nan)}
    ok = np.flatnonzero(idx[:, 0] >= 0) if M else np.zeros(0, dtype=np.int64)
    if ok.size == 0:
        return out
    # the start, and the fit's inputs: float64 of the caller's arrays, not of the LUT-dtype copies
    start = params[idx[ok, 0]]
    obs64 = np.asarray(obs, dtype=np.float64)[ok]
    w64 = None if weights is None else np.asarray(weights, dtype=np.float64)
    if w64 is not None and w64.ndim == 2:
        w64 = w64[ok]
    pm = pw = None
    if isinstance(prior, str):
        assert prior == "knn"
        near = bf.summarise_defined(params[:, free], idx[ok])
        pm, pw = knn_prior(near[0], near[2], lo, hi, floor=prior_floor)
    elif prior is not None:
        pm, pw = (a[ok] if a.ndim == 2 else a for a in prior_arrays(prior_plan_of(names, prior), M))
    fit = rd.refine_defined(start, free, lo, hi, obs64, forward, weights=w64, n_iter=n_iter, rel_step=rel_step, lambda0=lambda0,
                            prior_mean=pm, prior_weight=pw)
    for key, name in _FIT.items():
        out[key][ok] = fit[name]
    out["start"][ok] = start[:, free]
    return out
