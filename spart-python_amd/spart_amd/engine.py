"""Host-side driver of the HIP kernels: one Engine = one libspart_hip context = one
(device, sensor) pair.  torch tensors are used for device memory and streams only; every
compute call goes through the C ABI (include/spart_hip.h)."""
import collections
import ctypes
import math
import threading

import numpy as np

from . import _lib, tables, workloads
from .srf import check_srf

DTYPES = {"float32": _lib.SPART_F32, "fp32": _lib.SPART_F32, "f32": _lib.SPART_F32,
          "float64": _lib.SPART_F64, "fp64": _lib.SPART_F64, "f64": _lib.SPART_F64}
SMAC_FIELDS = ["Ta_s", "Ta_o", "Tg", "Ra_dd", "Ra_so", "Ta_ss", "Ta_sd", "Ta_oo", "Ta_do"]   # smac.py:209-211
MATERIALIZE_FIELDS = ["leaf_refl", "leaf_tran", "leaf_kchl", "soil_refl", "soil_refl_dry", "rso", "rdo", "rsd",
                      "rdd", "rsoil", "La", "band_mean", "R_TOC_srf", "R_TOA_srf", "L_TOA_srf", "rso_srf", "rdo_srf", "rsd_srf",
                      "rdd_srf"]
_SRF_COLUMNS = ["R_TOC_srf", "R_TOA_srf", "L_TOA_srf"]      # what band_model="srf" returns as R_TOC / R_TOA / L_TOA
_MAT_WIDTH = dict(leaf_refl=_lib.NWLS, leaf_tran=_lib.NWLS, leaf_kchl=_lib.NWL, soil_refl=_lib.NWLS,
                  soil_refl_dry=_lib.NWL, rso=_lib.NWLS, rdo=_lib.NWLS, rsd=_lib.NWLS, rdd=_lib.NWLS)


def _require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("spart_amd needs an AMD GPU (HIP device): the evaluator has no CPU path")
    return torch


def _dp(a):
    return a.ctypes.data_as(_lib.c_dp)


def _on_rows(t, row_stride):
    """a 2-D tensor steps ``row_stride`` elements from row to row and 1 along a row (a dimension of size 1 is never stepped:
    the kernels index element [b, j] at b * row_stride + j)"""
    return all(n == 1 or s == want for n, s, want in zip(t.shape, t.stride(), (row_stride, 1)))


def _nrows(x, width):
    """the row count of a row-set: (width,) and the reference's (width, 1) column are one row, (..., width) are rows"""
    s = tuple(np.shape(x))
    if s == (width, 1):
        return 1
    if not s or s[-1] != width:
        raise ValueError(f"an input of shape {s}: expected ({width},), ({width}, 1) or (B, {width})")
    return math.prod(s[:-1])


def batch_size(cols=(), rows=(), B=None):
    """The batch size of one call, from shapes alone.  ``cols``: per-sample values, each a scalar or B values (None = not
    given); ``rows``: (x, width) pairs of row-sets -- spectra (width 2001 / 2162) or lidf (13) -- each (width,),
    (width, 1) or (B, width) (x None = not given); ``B``: fixed by a (27, B) params block, else the largest count.
    Every input broadcasts: its count is 1 or B, anything else is a ValueError."""
    counts = [math.prod(np.shape(c)) for c in cols if c is not None] + [_nrows(x, w) for x, w in rows if x is not None]
    if B is None:
        B = max(counts, default=1)
    for n in counts:
        if n != 1 and n != B:
            raise ValueError(f"an input of {n} samples does not broadcast to a batch of {B}")
    return B


# the params rows (workloads.PARAM_NAMES) the C ABI lets be NULL, and the input that must then be given: soil B / lat / lon
# with user dry-soil spectra (spart_materialize.rdry_in), LIDFa / LIDFb with a given lidf (lidf_in)
NULLABLE = {9: "rdry", 10: "rdry", 11: "rdry", 16: "canopy_lidf", 17: "canopy_lidf"}


def fill_nulls(vals, first=0, **given):
    """``vals`` = params[first:first + len(vals)] with each None that NULLABLE allows for the inputs ``given`` (rdry=...,
    canopy_lidf=...) replaced by 0.0; any other None is a ValueError."""
    out = list(vals)
    for k, v in enumerate(out):
        if v is None:
            if given.get(NULLABLE.get(first + k)) is None:
                raise ValueError(f"params[{first + k}] is None (only B / lat / lon with rdry= and LIDFa / LIDFb with "
                                 "canopy_lidf= may be)")
            out[k] = 0.0
    return out


# Row pitch (elements) of the (B,2162) / (B,2001) spectrum arrays: rows padded to a multiple of 64 elements start
# on the 128 B line grid, which nearly doubles the HBM store rate of the materialised spectra on MI355X
# (include/spart_hip.h: spart_ctx_set_row_pitch).  Spectra are returned as [:, :width] views of padded storage.
ROW_PITCH = (2176, 2048)
LUT_NARROW_NB = 31     # spart_lut_nearest / spart_lut_topk take nb <= 31; above it lut_nearest / lut_topk call spart_lut_topk_wide


# LUT search -> (its *_workspace_bytes, its *_stats, the key of the float64 word of its stats)
_LUT_SEARCHES = {
    "spart_lut_nearest": ("spart_lut_workspace_bytes", "spart_lut_stats", "nmax"),
    "spart_lut_topk": ("spart_lut_topk_workspace_bytes", "spart_lut_topk_stats", "nmax"),
    "spart_lut_topk_wide": ("spart_lut_topk_wide_workspace_bytes", "spart_lut_topk_wide_stats", "nmax"),
    "spart_lut_topk_obs_weights": ("spart_lut_topk_obs_weights_workspace_bytes", "spart_lut_topk_obs_weights_stats", "nbound")}


def lut_weights_kind(shape, M, nb):
    """Which LUT search a ``weights`` argument of Engine.lut_nearest / lut_topk selects: shape None -> "none"; (nb,) ->
    "shared" (one weight per band for every observation: spart_lut_nearest / _topk / _topk_wide); (M, nb) -> "per_observation"
    (one weight row per observation, zero = masked band: spart_lut_topk_obs_weights).  Any other shape: ValueError."""
    if shape is None:
        return "none"
    shape = tuple(int(n) for n in shape)
    if shape == (nb,):
        return "shared"
    if shape == (M, nb):
        return "per_observation"
    raise ValueError(f"weights has shape {shape}, expected (nb,) = ({nb},) or (M, nb) = ({M}, {nb})")


def _prior_plan(names, prior):
    """refine_plan's prior checks: {name: (mean, sigma)} -> {"mean", "weight": F arrays, each () or (n,); "rows": n or None}"""
    if not isinstance(prior, dict):
        raise ValueError(f"prior = {prior!r}, expected a dict {{name: (mean, sigma)}}")
    stray = [n for n in prior if n not in names]
    if stray:
        raise ValueError(f"prior: {stray} not free")
    mean, weight, rows = [np.float64(0.0)] * len(names), [np.float64(0.0)] * len(names), None
    for n, entry in prior.items():
        if not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise ValueError(f"prior[{n!r}]: expected (mean, sigma)")
        mu, sigma = (np.asarray(v, dtype=np.float64) for v in entry)
        if not (np.all(sigma > 0) and not np.isnan(sigma).any()):
            raise ValueError(f"prior[{n!r}]: sigma must be > 0 (finite, or inf for no prior), got {entry[1]!r}")
        for what, v in (("mean", mu), ("sigma", sigma)):
            if v.ndim > 1 or (v.ndim == 1 and rows not in (None, v.shape[0])):
                raise ValueError(f"prior[{n!r}]: {what} has shape {v.shape}, expected a scalar or (M,)" +
                                 (f" = ({rows},)" if rows is not None else ""))
            if v.ndim == 1:
                rows = int(v.shape[0])
        with np.errstate(over="ignore"):
            w = 1.0 / (sigma * sigma)
        i = names.index(n)
        mean[i], weight[i] = mu, w
    return {"mean": mean, "weight": weight, "rows": rows}


def prior_arrays(plan_prior, M):
    """the prior of a refine_plan for M observations -> (mean, weight) float64, (F,) or, with any array-valued entry, (M, F)"""
    rows = plan_prior["rows"]
    if rows is None:
        return np.array(plan_prior["mean"], dtype=np.float64), np.array(plan_prior["weight"], dtype=np.float64)
    if rows != M:
        raise ValueError(f"prior: arrays of {rows} values for {M} observations; expected scalars or (M,) = ({M},)")
    return tuple(np.ascontiguousarray(np.stack([np.broadcast_to(v, (M,)) for v in plan_prior[k]], axis=1), dtype=np.float64)
                 for k in ("mean", "weight"))


def _prior_tensor_shapes(prior_mean, prior_weight, M, F):
    """the ready-made form of a prior: both given, both (F,) or both (M, F) -> 1 for (M, F), else 0"""
    if prior_mean is None or prior_weight is None:
        raise ValueError("prior_mean and prior_weight come together")
    sm, sw = (tuple(int(n) for n in (v.shape if hasattr(v, "shape") else np.shape(v))) for v in (prior_mean, prior_weight))
    if sm != sw or sm not in ((F,), (M, F)):
        raise ValueError(f"prior_mean {sm} and prior_weight {sw}: expected both (F,) = ({F},) or both (M, F) = ({M}, {F})")
    return int(len(sm) == 2)


def knn_prior(mean, std, lo, hi, floor=0.05):
    """A Gaussian prior for Engine.refine from the summary of the k nearest LUT rows (Engine.lut_summarise / retrieve's mean and
    std of the free columns): sigma = maximum(std, floor * (hi - lo)), weight = 1.0 / (sigma * sigma), each one rounded
    operation in float64, so numpy arrays and torch tensors give the same bits.  ``mean``, ``std`` (M, F) (numpy or torch);
    ``lo``, ``hi`` (F,) the bounds of the free parameters.  ``floor`` (default 0.05: a twentieth of the range) is an option, not
    a tolerance: it keeps a set of k identical rows (std = 0) from pinning the parameter.  An observation without rows (a NaN
    mean or std) gets weight 0 and mean 0: no prior.  -> (prior_mean, prior_weight), like the inputs."""
    floor = float(floor)
    if not (np.isfinite(floor) and floor >= 0):
        raise ValueError(f"floor = {floor!r}, expected a finite value >= 0")
    width = floor * (np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))
    if hasattr(mean, "device") and not isinstance(mean, np.ndarray):            # torch tensors
        import torch
        mean, std = mean.to(torch.float64), torch.as_tensor(std).to(device=mean.device, dtype=torch.float64)
        sigma = torch.maximum(std, torch.as_tensor(width, device=mean.device).expand_as(std))
        weight = 1.0 / (sigma * sigma)
        none = torch.isnan(mean) | torch.isnan(std)
        zero = torch.zeros((), dtype=torch.float64, device=mean.device)
        return torch.where(none, zero, mean), torch.where(none, zero, weight)
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    with np.errstate(all="ignore"):
        sigma = np.maximum(std, width)
        weight = 1.0 / (sigma * sigma)
    none = np.isnan(mean) | np.isnan(std)
    return np.where(none, 0.0, mean), np.where(none, 0.0, weight)


def refine_plan(free, bounds, n_iter, column, rel_step, lambda0, default_ranges=None, prior=None):
    """The host-side argument checks of Engine.refine / spart_refine, none of which needs a device.  ``free``: names from
    workloads.PARAM_NAMES, 1 ... 16 of them, each once; ``bounds``: {name: (lo, hi)} for free names only, finite with lo < hi,
    the others from ``default_ranges`` (None = workloads.RANGES; a name with neither is a ValueError).  ``prior``:
    {name: (mean, sigma)} for free names only, each a scalar or an (M,) array (any array makes the prior per-observation);
    sigma > 0, finite or np.inf (no prior on that name, like a name that is not listed); the weight is 1.0 / (sigma * sigma).
    -> dict: names, cols (int32), lo, hi (float64), column (0 / 1 / 2), n_iter, rel_step, lambda0, prior (None, or what
    prior_arrays turns into (mean, weight) once M is known)."""
    names = [str(n) for n in free]
    unknown = [n for n in names if n not in workloads.PARAM_NAMES]
    if unknown:
        raise ValueError(f"free: unknown parameter name(s) {unknown}; expected names from {list(workloads.PARAM_NAMES)}")
    if not 1 <= len(names) <= _lib.REFINE_MAXF:
        raise ValueError(f"free: {len(names)} names, expected 1 ... {_lib.REFINE_MAXF}")
    twice = sorted({n for n in names if names.count(n) > 1})
    if twice:
        raise ValueError(f"free: {twice} named twice")
    bounds = dict(bounds or {})
    stray = [n for n in bounds if n not in names]
    if stray:
        raise ValueError(f"bounds: {stray} not free")
    ranges = workloads.RANGES if default_ranges is None else default_ranges
    lo, hi = np.empty(len(names)), np.empty(len(names))
    for i, n in enumerate(names):
        if n not in bounds and n not in ranges:
            raise ValueError(f"free: {n!r} has no range and no bound was given for it (bounds={{{n!r}: (lo, hi)}})")
        lo[i], hi[i] = (float(v) for v in (bounds[n] if n in bounds else ranges[n]))
        if not (np.isfinite(lo[i]) and np.isfinite(hi[i]) and lo[i] < hi[i]):
            raise ValueError(f"bounds of {n!r}: ({lo[i]}, {hi[i]}); finite lo < hi expected")
    if column not in _lib.REFINE_COLUMNS:
        raise ValueError(f"column = {column!r}, expected one of {_lib.REFINE_COLUMNS}")
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or not 0 <= int(n_iter) <= _lib.REFINE_MAX_ITER:
        raise ValueError(f"n_iter = {n_iter!r}, expected an integer 0 ... {_lib.REFINE_MAX_ITER}")
    for what, v in (("rel_step", rel_step), ("lambda0", lambda0)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{what} = {v!r}, expected a finite value > 0")
    return {"names": names, "cols": np.array([workloads.PARAM_NAMES.index(n) for n in names], dtype=np.int32), "lo": lo, "hi": hi,
            "column": _lib.REFINE_COLUMNS.index(column), "n_iter": int(n_iter), "rel_step": float(rel_step),
            "lambda0": float(lambda0), "prior": None if prior is None else _prior_plan(names, prior)}


def _refine_head(make_plan, lidf, prior, prior_mean, prior_weight, band_model):
    """How refine_args and refine_views_args begin: prior exclusivity, the band model's name, the plan ``make_plan()`` gives,
    lidf -> the plan"""
    ready = prior_mean is not None or prior_weight is not None
    if prior is not None and ready:
        raise ValueError("prior and prior_mean / prior_weight exclude each other")
    _band_model(band_model)
    plan = make_plan()
    if plan.get("prior") is not None and ready:
        raise ValueError("prior and prior_mean / prior_weight exclude each other")
    if lidf not in ("literal", "newton"):
        raise ValueError("lidf must be 'literal' or 'newton'")
    return plan


def _refine_prior(prior_mean, prior_weight, M, n, made):
    """How they end: the ready-made prior with its shapes checked for n unknowns, else ``made``, the (mean, weight) arrays of
    the dict prior or None -> (prior_mean, prior_weight, prior per observation 0 / 1)"""
    if prior_mean is not None or prior_weight is not None:
        return prior_mean, prior_weight, _prior_tensor_shapes(prior_mean, prior_weight, M, n)
    if made is None:
        return None, None, 0
    return made[0], made[1], int(made[0].ndim == 2)


def refine_args(params, obs, free, bounds, weights, column, n_iter, rel_step, lambda0, lidf, prior, prior_mean, prior_weight,
                band_model, nb=None, _plan=None):
    """Every argument check of spart_amd.refine and Engine.refine that needs no device: prior exclusivity, the band model's
    name, refine_plan (unless ``_plan`` is one), lidf, and the shapes of obs ((M, nb); ``nb`` given: that nb), params (a (27, M)
    block or 27 columns of 1 or M values), weights and the prior.
    -> (plan, params, M, weights kind, prior_mean, prior_weight, prior per observation 0 / 1); ``params`` comes back as the
    2-D tensor it was, else as a list of 27 columns; a plan's prior comes back as its prior_arrays."""
    import torch
    plan = _refine_head(lambda: _plan if _plan is not None else refine_plan(free, bounds, n_iter, column, rel_step, lambda0, prior=prior),
                        lidf, prior, prior_mean, prior_weight, band_model)
    oshape = tuple(int(n) for n in np.shape(obs))
    if len(oshape) != 2 or (nb is not None and oshape[1] != nb):
        raise ValueError(f"obs has shape {oshape}, expected (M, nb)" + ("" if nb is None else f" = (M, {nb})"))
    M = oshape[0]
    if not isinstance(params, (list, tuple)):
        if not torch.is_tensor(params):
            params = np.asarray(params, dtype=np.float64)
        if len(params.shape) != 2 or params.shape[0] != _lib.NPARAM:
            raise ValueError(f"params must be (27, M) or a list of 27 columns, got shape {tuple(params.shape)}")
        counts = [int(params.shape[1])]
        if not torch.is_tensor(params):
            params = list(params)
    else:
        if len(params) != _lib.NPARAM:
            raise ValueError(f"params must have {_lib.NPARAM} entries, got {len(params)}")
        params = fill_nulls(params)
        counts = [math.prod(np.shape(c)) for c in params]
    for n in counts:
        if n not in (1, M):
            raise ValueError(f"a params column of {n} values does not broadcast to the {M} rows of obs")
    kind = lut_weights_kind(None if weights is None else np.shape(weights), M, oshape[1])
    return (plan, params, M, kind) + _refine_prior(prior_mean, prior_weight, M, len(plan["names"]),
                                                   None if plan.get("prior") is None else prior_arrays(plan["prior"], M))


LEAF_NAMES = tuple(workloads.PARAM_NAMES[:_lib.LEAF_NPAR])      # spart_refine_leaf's leaf[9], spart_prospect_batch's order


def refine_leaf_args(leaf, refl, tran, free, bounds, weights_refl, weights_tran, n_iter, rel_step, lambda0, prior, prior_mean,
                     prior_weight):
    """Every argument check of spart_amd.refine_leaf and Engine.refine_leaf that needs no device: prior exclusivity; ``free``
    1 ... 9 distinct names of LEAF_NAMES with refine_plan's checks of bounds, n_iter, rel_step, lambda0 and the prior; refl and
    tran (M, 2001), at least one of them; weights only for a given array, (2001,) or (M, 2001); leaf a (9, M) block or nine
    columns of 1 or M values; the prior's shapes.
    -> (plan, leaf, M, weights per observation 0 / 1, prior_mean, prior_weight, prior per observation 0 / 1); ``leaf`` comes
    back as the 2-D tensor it was, else as a list of nine columns; a plan's prior comes back as its prior_arrays."""
    import torch
    ready = prior_mean is not None or prior_weight is not None
    if prior is not None and ready:
        raise ValueError("prior and prior_mean / prior_weight exclude each other")
    names = [str(n) for n in free]
    stray = [n for n in names if n not in LEAF_NAMES]
    if stray:
        raise ValueError(f"free: {stray} are no leaf parameters; expected names from {list(LEAF_NAMES)}")
    if not 1 <= len(names) <= _lib.LEAF_MAXF:
        raise ValueError(f"free: {len(names)} names, expected 1 ... {_lib.LEAF_MAXF}")
    plan = refine_plan(names, bounds, n_iter, _lib.REFINE_COLUMNS[0], rel_step, lambda0, prior=prior)
    if refl is None and tran is None:
        raise ValueError("refl and tran are both None: at least one spectrum per leaf is needed")
    shapes = {k: tuple(int(n) for n in np.shape(v)) for k, v in (("refl", refl), ("tran", tran)) if v is not None}
    for k, sh in shapes.items():
        if len(sh) != 2 or sh[1] != _lib.NWL:
            raise ValueError(f"{k} has shape {sh}, expected (M, {_lib.NWL})")
    if len({sh[0] for sh in shapes.values()}) != 1:
        raise ValueError(f"refl {shapes['refl']} and tran {shapes['tran']} differ in their number of leaves")
    M = next(iter(shapes.values()))[0]
    wper = 0
    for k, w, obs in (("weights_refl", weights_refl, refl), ("weights_tran", weights_tran, tran)):
        if w is None:
            continue
        if obs is None:
            raise ValueError(f"{k} given without its spectra")
        if lut_weights_kind(np.shape(w), M, _lib.NWL) == "per_observation":
            wper = 1
    if not isinstance(leaf, (list, tuple)):
        if not torch.is_tensor(leaf):
            leaf = np.asarray(leaf, dtype=np.float64)
        if len(leaf.shape) != 2 or leaf.shape[0] != _lib.LEAF_NPAR:
            raise ValueError(f"leaf must be ({_lib.LEAF_NPAR}, M) or a list of {_lib.LEAF_NPAR} columns, got shape {tuple(leaf.shape)}")
        counts = [int(leaf.shape[1])]
        if not torch.is_tensor(leaf):
            leaf = list(leaf)
    else:
        if len(leaf) != _lib.LEAF_NPAR:
            raise ValueError(f"leaf must have {_lib.LEAF_NPAR} entries, got {len(leaf)}")
        if any(c is None for c in leaf):
            raise ValueError("leaf: no entry may be None")
        leaf = list(leaf)
        counts = [math.prod(np.shape(c)) for c in leaf]
    for n in counts:
        if n not in (1, M):
            raise ValueError(f"a leaf column of {n} values does not broadcast to the {M} rows of the spectra")
    return (plan, leaf, M, wper) + _refine_prior(prior_mean, prior_weight, M, len(names),
                                                 None if plan.get("prior") is None else prior_arrays(plan["prior"], M))


def _views_prior(names, Fs, V, prior):
    """refine_views' prior: {name: (mean, sigma)} -> (mean, weight) per UNKNOWN, (n,) or -- when any value has a pixel axis --
    (M, n), with M read from the values.  A shared name takes a scalar or (M,); a local name a scalar, (V,) or (M, V)."""
    if not isinstance(prior, dict):
        raise ValueError(f"prior = {prior!r}, expected a dict {{name: (mean, sigma)}}")
    stray = [k for k in prior if k not in names]
    if stray:
        raise ValueError(f"prior: {stray} not free")
    Fl = len(names) - Fs
    n, rows = Fs + V * Fl, None
    parts = {}
    for name, entry in prior.items():
        if not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise ValueError(f"prior[{name!r}]: expected (mean, sigma)")
        mu, sigma = (np.asarray(v, dtype=np.float64) for v in entry)
        if not (np.all(sigma > 0) and not np.isnan(sigma).any()):
            raise ValueError(f"prior[{name!r}]: sigma must be > 0 (finite, or inf for no prior), got {entry[1]!r}")
        local = names.index(name) >= Fs
        for what, v in (("mean", mu), ("sigma", sigma)):
            ok = v.ndim == 0 or (v.ndim == 1 and (not local or v.shape[0] == V)) or (local and v.ndim == 2 and v.shape[1] == V)
            m = v.shape[0] if (v.ndim == 2 or (v.ndim == 1 and not local)) else None
            if not ok or (m is not None and rows not in (None, m)):
                raise ValueError(f"prior[{name!r}]: {what} has shape {v.shape}, expected a scalar, " +
                                 (f"(V,) = ({V},) or (M, V)" if local else "or (M,)"))
            rows = m if m is not None else rows
        with np.errstate(over="ignore"):
            parts[name] = (mu, 1.0 / (sigma * sigma))
    R = 1 if rows is None else rows
    mean, weight = np.zeros((R, n)), np.zeros((R, n))
    for name, (mu, w) in parts.items():
        f = names.index(name)
        for out, v in ((mean, mu), (weight, w)):
            if f < Fs:
                out[:, f] = v
            else:
                out[:, Fs + (f - Fs):n:Fl] = np.broadcast_to(v, (R, V))
    return (mean[0], weight[0]) if rows is None else (mean, weight)


def refine_views_args(params, obs, shared, local, bounds, weights, column, n_iter, rel_step, lambda0, lidf, prior, prior_mean,
                      prior_weight, band_model, nb=None):
    """Every argument check of spart_amd.refine_views and Engine.refine_views that needs no device: refine_plan on the names
    shared + local, then the shapes -- obs (M, V, nb) with 1 <= V <= 64, n = Fs + V Fl in 1 ... 16, params a (27, V, M) block or
    27 entries each broadcastable to (V, M), weights None / (nb,) / (M, V, nb), the prior per unknown.
    -> (plan, params, (M, V, Fs, n), weights per observation 0 / 1, prior_mean, prior_weight, prior per observation 0 / 1)"""
    import torch

    def make_plan():
        nonlocal shared, local
        shared, local = [str(s) for s in shared], [str(s) for s in local]
        return refine_plan(shared + local, bounds, n_iter, column, rel_step, lambda0)
    plan = _refine_head(make_plan, lidf, prior, prior_mean, prior_weight, band_model)
    oshape = tuple(int(k) for k in np.shape(obs))
    if len(oshape) != 3 or (nb is not None and oshape[2] != nb):
        raise ValueError(f"obs has shape {oshape}, expected (M, V, nb)" + ("" if nb is None else f" = (M, V, {nb})"))
    M, V, Fs = oshape[0], oshape[1], len(shared)
    if not 1 <= V <= _lib.REFINE_MAXV:
        raise ValueError(f"obs has V = {V} views, expected 1 ... {_lib.REFINE_MAXV}")
    n = Fs + V * len(local)
    if not 1 <= n <= _lib.REFINE_MAXF:
        raise ValueError(f"{Fs} shared + {V} views x {len(local)} local = {n} unknowns per pixel, expected 1 ... {_lib.REFINE_MAXF}")
    if not isinstance(params, (list, tuple)):
        if not torch.is_tensor(params):
            params = np.asarray(params, dtype=np.float64)
        if len(params.shape) != 3 or tuple(params.shape) != (_lib.NPARAM, V, M):
            raise ValueError(f"params must be (27, V, M) = (27, {V}, {M}) or a list of 27 entries, got shape {tuple(params.shape)}")
    else:
        if len(params) != _lib.NPARAM:
            raise ValueError(f"params must have {_lib.NPARAM} entries, got {len(params)}")
        for i, c in enumerate(fill_nulls(params)):
            try:
                np.broadcast_shapes(tuple(np.shape(c)), (V, M))
            except ValueError:
                raise ValueError(f"params[{i}] of shape {tuple(np.shape(c))} does not broadcast to (V, M) = ({V}, {M})") from None
            if len(np.shape(c)) > 2:
                raise ValueError(f"params[{i}] of shape {tuple(np.shape(c))} does not broadcast to (V, M) = ({V}, {M})")
        params = fill_nulls(params)
    wper = 0
    if weights is not None:
        ws = tuple(int(k) for k in np.shape(weights))
        if ws not in ((oshape[2],), oshape):
            raise ValueError(f"weights has shape {ws}, expected (nb,) = ({oshape[2]},) or (M, V, nb) = {oshape}")
        wper = int(len(ws) == 3)
    prior_mean, prior_weight, per_obs = _refine_prior(prior_mean, prior_weight, M, n,
                                                      None if prior is None else _views_prior(plan["names"], Fs, V, prior))
    if prior is not None and per_obs and prior_mean.shape[0] != M:
        raise ValueError(f"prior: arrays of {prior_mean.shape[0]} pixels for the {M} of obs")
    return plan, params, (M, V, Fs, n), wper, prior_mean, prior_weight, per_obs


def mix_maps(V, Fs, Fl, active, fit_fractions):
    """The unknowns of refine_mix in their order -- the Fs shared names, the ACTIVE locals (component v ascending, l ascending
    within it), with fitted fractions q_0 ... q_{V-2} -> (unknown (V, Fl) int: the unknown of local l in component v or -1, nm
    the number of model unknowns, n)"""
    unknown = np.full((V, Fl), -1, dtype=np.int64)
    nm = Fs
    for v in range(V):
        for l in range(Fl):
            if active[v, l]:
                unknown[v, l] = nm
                nm += 1
    return unknown, nm, nm + (V - 1 if fit_fractions else 0)


def _mix_prior(names, Fs, V, unknown, nm, n, prior):
    """refine_mix's prior: {name: (mean, sigma)} -> (mean, weight) per UNKNOWN, (n,) or -- when any value has a pixel axis --
    (M, n).  A shared name takes a scalar or (M,); a local name a scalar, (V,) or (M, V) (the entries of components where it is
    inactive are not read); the key "fractions" a scalar, (V - 1,) or (M, V - 1), one entry per fitted fraction."""
    if not isinstance(prior, dict):
        raise ValueError(f"prior = {prior!r}, expected a dict {{name: (mean, sigma)}}")
    stray = [k for k in prior if k not in names and k != "fractions"]
    if stray:
        raise ValueError(f"prior: {stray} not free")
    if "fractions" in prior and n == nm:
        raise ValueError("prior: 'fractions' without a fitted fraction")
    rows, parts = None, {}
    for name, entry in prior.items():
        if not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise ValueError(f"prior[{name!r}]: expected (mean, sigma)")
        mu, sigma = (np.asarray(v, dtype=np.float64) for v in entry)
        if not (np.all(sigma > 0) and not np.isnan(sigma).any()):
            raise ValueError(f"prior[{name!r}]: sigma must be > 0 (finite, or inf for no prior), got {entry[1]!r}")
        width = None if name != "fractions" and names.index(name) < Fs else (n - nm if name == "fractions" else V)
        for what, v in (("mean", mu), ("sigma", sigma)):
            ok = v.ndim == 0 or (v.ndim == 1 and (width is None or v.shape[0] == width)) or (width is not None and v.ndim == 2 and
                                                                                             v.shape[1] == width)
            m = v.shape[0] if (v.ndim == 2 or (v.ndim == 1 and width is None)) else None
            if not ok or (m is not None and rows not in (None, m)):
                raise ValueError(f"prior[{name!r}]: {what} has shape {v.shape}, expected a scalar, " +
                                 ("or (M,)" if width is None else f"({width},) or (M, {width})"))
            rows = m if m is not None else rows
        with np.errstate(over="ignore"):
            parts[name] = (mu, 1.0 / (sigma * sigma))
    R = 1 if rows is None else rows
    mean, weight = np.zeros((R, n)), np.zeros((R, n))
    for name, (mu, w) in parts.items():
        for out, v in ((mean, mu), (weight, w)):
            if name == "fractions":
                out[:, nm:] = np.broadcast_to(v, (R, n - nm))
            elif names.index(name) < Fs:
                out[:, names.index(name)] = v
            else:
                l, full = names.index(name) - Fs, np.broadcast_to(v, (R, V))
                for c in range(V):
                    if unknown[c, l] >= 0:
                        out[:, unknown[c, l]] = full[:, c]
    return (mean[0], weight[0]) if rows is None else (mean, weight)


def refine_mix_args(params, obs, shared, local, active, fractions, fit_fractions, fraction_bounds, bounds, weights, column, n_iter,
                    rel_step, lambda0, lidf, prior, band_model, nb=None):
    """Every argument check of spart_amd.refine_mix and Engine.refine_mix that needs no device: refine_plan on the names
    shared + local, then the shapes -- obs (M, nb), params a (27, V, M) block or 27 entries each broadcastable to (V, M) (V is then
    read from ``fractions``, from an ``active`` array or from the entries), 1 <= V <= 8, ``active`` a dict {local name:
    components} or a (V, Fl) array of 0 / 1 with every local active somewhere, ``fractions`` None / (V,) / (M, V), the fraction
    box, n in 1 ... 16, weights None / (nb,) / (M, nb), the prior per unknown.
    -> (plan, params, (M, V, Fs, nm, n), active (V, Fl) int32, fractions (M, V) float64, (frac_lo, frac_hi), weights per
    observation 0 / 1, prior_mean, prior_weight, prior per observation 0 / 1)"""
    import torch

    def make_plan():
        nonlocal shared, local
        shared, local = [str(s) for s in shared], [str(s) for s in local]
        return refine_plan(shared + local, bounds, n_iter, column, rel_step, lambda0)
    plan = _refine_head(make_plan, lidf, prior, None, None, band_model)
    oshape = tuple(int(k) for k in np.shape(obs))
    if len(oshape) != 2 or (nb is not None and oshape[1] != nb):
        raise ValueError(f"obs has shape {oshape}, expected (M, nb)" + ("" if nb is None else f" = (M, {nb})"))
    M, Fs, Fl = oshape[0], len(shared), len(local)
    if isinstance(fit_fractions, (bool, np.bool_)):
        fit_fractions = bool(fit_fractions)
    else:
        raise ValueError(f"fit_fractions = {fit_fractions!r}, expected True or False")
    fr = None if fractions is None else np.asarray(fractions, dtype=np.float64)
    if fr is not None and fr.ndim not in (1, 2):
        raise ValueError(f"fractions has shape {fr.shape}, expected (V,) or (M, V)")
    act = None if active is None or isinstance(active, dict) else np.asarray(active)
    if act is not None and act.ndim != 2:
        raise ValueError(f"active has shape {act.shape}, expected (V, Fl) = (V, {Fl}), or a dict {{local name: components}}")
    if not isinstance(params, (list, tuple)):
        if not torch.is_tensor(params):
            params = np.asarray(params, dtype=np.float64)
        if len(params.shape) != 3 or params.shape[0] != _lib.NPARAM or params.shape[2] != M:
            raise ValueError(f"params must be (27, V, M) = (27, V, {M}) or a list of 27 entries, got shape {tuple(params.shape)}")
        V = int(params.shape[1])
    else:
        if len(params) != _lib.NPARAM:
            raise ValueError(f"params must have {_lib.NPARAM} entries, got {len(params)}")
        params = fill_nulls(params)
        V = fr.shape[-1] if fr is not None else act.shape[0] if act is not None else max(
            [1] + [int(np.shape(c)[0]) for c in params if len(np.shape(c)) == 2])
    if not 1 <= V <= _lib.MIX_MAXV:
        raise ValueError(f"V = {V} components, expected 1 ... {_lib.MIX_MAXV}")
    if isinstance(params, list):
        for i, c in enumerate(params):
            try:
                bad = len(np.shape(c)) > 2
                np.broadcast_shapes(tuple(np.shape(c)), (V, M))
            except ValueError:
                bad = True
            if bad:
                raise ValueError(f"params[{i}] of shape {tuple(np.shape(c))} does not broadcast to (V, M) = ({V}, {M})")
    if isinstance(active, dict):
        stray = [k for k in active if k not in local]
        if stray:
            raise ValueError(f"active: {stray} not local")
        act = np.ones((V, Fl), dtype=np.int32)
        for name, comps in active.items():
            comps = [comps] if np.ndim(comps) == 0 else list(comps)
            if any(isinstance(c, bool) or int(c) != c or not 0 <= int(c) < V for c in comps):
                raise ValueError(f"active[{name!r}] = {comps!r}, expected components 0 ... {V - 1}")
            act[:, local.index(name)] = 0
            act[[int(c) for c in comps], local.index(name)] = 1
    elif act is None:
        act = np.ones((V, Fl), dtype=np.int32)
    else:
        if act.shape != (V, Fl) or not np.isin(act, (0, 1)).all():
            raise ValueError(f"active has shape {act.shape}, expected (V, Fl) = ({V}, {Fl}) of 0 / 1")
        act = act.astype(np.int32)
    nowhere = [local[l] for l in range(Fl) if not act[:, l].any()]
    if nowhere:
        raise ValueError(f"active: {nowhere} active in no component")
    act = np.ascontiguousarray(act, dtype=np.int32)
    if fr is None:
        fr = np.full((M, V), 1.0 / V)
    elif fr.shape not in ((V,), (M, V)):
        raise ValueError(f"fractions has shape {fr.shape}, expected (V,) = ({V},) or (M, V) = ({M}, {V})")
    fr = np.array(np.broadcast_to(fr, (M, V)), order="C")
    try:
        flo, fhi = (float(v) for v in fraction_bounds)
    except (TypeError, ValueError):
        raise ValueError(f"fraction_bounds = {fraction_bounds!r}, expected (lo, hi)") from None
    if not 0.0 <= flo < fhi <= 1.0:
        raise ValueError(f"fraction_bounds = ({flo}, {fhi}), expected 0 <= lo < hi <= 1")
    unknown, nm, n = mix_maps(V, Fs, Fl, act, fit_fractions)
    if not 1 <= n <= _lib.REFINE_MAXF:
        raise ValueError(f"{Fs} shared + {nm - Fs} active local + {n - nm} fractions = {n} unknowns per pixel, expected 1 ... "
                         f"{_lib.REFINE_MAXF}")
    kind = lut_weights_kind(None if weights is None else np.shape(weights), M, oshape[1])
    prior_mean, prior_weight, per_obs = _refine_prior(None, None, M, n, None if prior is None else _mix_prior(
        plan["names"], Fs, V, unknown, nm, n, prior))
    if prior is not None and per_obs and prior_mean.shape[0] != M:
        raise ValueError(f"prior: arrays of {prior_mean.shape[0]} pixels for the {M} of obs")
    return (plan, params, (M, V, Fs, nm, n), act, fr, (flo, fhi), 1 if kind == "per_observation" else 0, prior_mean, prior_weight,
            per_obs)


def tile_starts(M, tile_size, tile_start):
    """refine_tiles' partition: exactly one of ``tile_size`` (uniform runs of G pixels, a shorter last one) and ``tile_start``
    ((T + 1,) integers, 0 = s_0 < s_1 < ... < s_T = M) -> tile_start as int64; no tile above 4096 pixels"""
    if (tile_size is None) == (tile_start is None):
        raise ValueError("exactly one of tile_size and tile_start is expected")
    if tile_size is not None:
        if isinstance(tile_size, bool) or int(tile_size) != tile_size or not 1 <= int(tile_size) <= _lib.TILES_MAXG:
            raise ValueError(f"tile_size = {tile_size!r}, expected an integer 1 ... {_lib.TILES_MAXG}")
        G = int(tile_size)
        return np.minimum(np.arange(0, M + G, G, dtype=np.int64)[:(M + G - 1) // G + 1], M)
    ts = np.asarray(tile_start)
    if ts.ndim != 1 or ts.size < 1 or not np.issubdtype(ts.dtype, np.integer):
        raise ValueError(f"tile_start: expected a (T + 1,) integer array, got shape {ts.shape} of {ts.dtype}")
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    if ts[0] != 0 or ts[-1] != M:
        raise ValueError(f"tile_start runs from {int(ts[0])} to {int(ts[-1])}, expected 0 ... M = {M}")
    size = np.diff(ts)
    if ((size < 1) | (size > _lib.TILES_MAXG)).any():
        t = int(np.flatnonzero((size < 1) | (size > _lib.TILES_MAXG))[0])
        raise ValueError(f"tile_start: tile {t} has {int(size[t])} pixels, expected 1 ... {_lib.TILES_MAXG}")
    return ts


def refine_tiles_args(params, obs, shared, local, tile_size, tile_start, bounds, weights, column, n_iter, rel_step, lambda0, lidf,
                      prior, band_model, nb=None, partition=None, units=("pixels", "tiles")):
    """Every argument check of spart_amd.refine_tiles and Engine.refine_tiles that needs no device: refine_args on the names
    shared + local (the plan, obs (M, nb), params, weights), the partition (tile_starts), and the prior dict split by name --
    a shared name takes scalars or (T,) arrays, a local name scalars or (M,) arrays.
    -> (plan, params, M, Fs, weights per observation 0 / 1, tile_start, local prior, shared prior), a prior being
    (mean, weight, per row 0 / 1) with (None, None, 0) for none.  ``partition`` (M -> tile_start) and ``units`` are
    refine_series_args' way in: its rows and series in place of pixels and tiles"""
    shared, local = [str(s) for s in shared], [str(s) for s in local]
    plan, params, M, kind = refine_args(params, obs, shared + local, bounds, weights, column, n_iter, rel_step, lambda0, lidf, None,
                                        None, None, band_model, nb=nb)[:4]
    ts = tile_starts(M, tile_size, tile_start) if partition is None else partition(M)
    priors = []
    if prior is not None and not isinstance(prior, dict):
        raise ValueError(f"prior = {prior!r}, expected a dict {{name: (mean, sigma)}}")
    stray = [k for k in (prior or {}) if k not in plan["names"]]
    if stray:
        raise ValueError(f"prior: {stray} not free")
    for names, rows, what in ((local, M, units[0]), (shared, ts.size - 1, units[1])):
        part = {k: v for k, v in (prior or {}).items() if k in names}
        if not part:
            priors.append((None, None, 0))
            continue
        pp = _prior_plan(names, part)
        if pp["rows"] not in (None, rows):
            raise ValueError(f"prior: arrays of {pp['rows']} values for the {rows} {what} of {names}")
        mean, weight = prior_arrays(pp, rows)
        priors.append((mean, weight, int(mean.ndim == 2)))
    return plan, params, M, len(shared), int(kind == "per_observation"), ts, priors[0], priors[1]


def series_starts(M, n_dates, series_start):
    """refine_series' partition: exactly one of ``n_dates`` (uniform series of T rows; M must be a multiple) and
    ``series_start`` ((S + 1,) integers, 0 = s_0 < s_1 < ... < s_S = M) -> series_start as int64; no series above 256 rows"""
    if (n_dates is None) == (series_start is None):
        raise ValueError("exactly one of n_dates and series_start is expected")
    if n_dates is not None:
        if isinstance(n_dates, bool) or int(n_dates) != n_dates or not 1 <= int(n_dates) <= _lib.SERIES_MAXT:
            raise ValueError(f"n_dates = {n_dates!r}, expected an integer 1 ... {_lib.SERIES_MAXT}")
        T = int(n_dates)
        if M % T:
            raise ValueError(f"n_dates = {T} does not divide the {M} rows of obs")
        return np.arange(0, M + 1, T, dtype=np.int64)
    ts = np.asarray(series_start)
    if ts.ndim != 1 or ts.size < 1 or not np.issubdtype(ts.dtype, np.integer):
        raise ValueError(f"series_start: expected a (S + 1,) integer array, got shape {ts.shape} of {ts.dtype}")
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    if ts[0] != 0 or ts[-1] != M:
        raise ValueError(f"series_start runs from {int(ts[0])} to {int(ts[-1])}, expected 0 ... M = {M}")
    size = np.diff(ts)
    if ((size < 1) | (size > _lib.SERIES_MAXT)).any():
        t = int(np.flatnonzero((size < 1) | (size > _lib.SERIES_MAXT))[0])
        raise ValueError(f"series_start: series {t} has {int(size[t])} rows, expected 1 ... {_lib.SERIES_MAXT}")
    return ts


def refine_series_args(params, obs, shared, local, n_dates, series_start, smooth, link, bounds, weights, column, n_iter, rel_step,
                       lambda0, lidf, prior, band_model, nb=None):
    """Every argument check of spart_amd.refine_series and Engine.refine_series that needs no device: refine_tiles_args with
    the series partition, at least one local name, ``smooth`` = {local name: sigma > 0} (gamma = 1 / sigma^2; a local that
    is not named gets gamma = 0) and ``link`` (None, or (M,) values; a tensor is left for the device to judge).
    -> refine_tiles_args' tuple, then gamma (Fl,) float64"""
    local = [str(s) for s in local]
    if not local:
        raise ValueError("local: at least one local name is expected (nothing to link: use refine_tiles)")
    out = refine_tiles_args(params, obs, shared, local, None, None, bounds, weights, column, n_iter, rel_step, lambda0, lidf, prior,
                            band_model, nb=nb, partition=lambda M: series_starts(M, n_dates, series_start), units=("rows", "series"))
    if smooth is not None and not isinstance(smooth, dict):
        raise ValueError(f"smooth = {smooth!r}, expected a dict {{local name: sigma}}")
    stray = [k for k in (smooth or {}) if k not in local]
    if stray:
        raise ValueError(f"smooth: {stray} not local")
    gamma = np.zeros(len(local))
    for k, sigma in (smooth or {}).items():
        try:
            sg = float(sigma)
        except (TypeError, ValueError):
            raise ValueError(f"smooth[{k!r}] = {sigma!r}, expected one sigma > 0") from None
        if not (sg > 0.0 and np.isfinite(sg) and sg * sg > 0.0 and np.isfinite(1.0 / (sg * sg))):
            raise ValueError(f"smooth[{k!r}]: sigma = {sigma!r}, expected a finite number > 0 with a finite 1 / sigma^2")
        gamma[local.index(k)] = 1.0 / (sg * sg)
    M = out[2]
    if link is not None and not hasattr(link, "data_ptr"):
        ln = np.asarray(link, dtype=np.float64)
        if ln.shape != (M,):
            raise ValueError(f"link has shape {ln.shape}, expected ({M},)")
    elif link is not None and tuple(link.shape) != (M,):
        raise ValueError(f"link has shape {tuple(link.shape)}, expected ({M},)")
    return out + (gamma,)


def sobol_design(N, F, seed=0):
    """The two designs of sobol(): -> (uA, uB), float64 (N, F) in [0, 1): the first and the last F columns of ONE scrambled
    torch.quasirandom.SobolEngine(2 F, scramble=True, seed=seed) draw of N points in float64 (Saltelli's scheme wants A and B
    as the two halves of one 2 F-dimensional sequence).  Needs no device."""
    import torch
    if isinstance(N, bool) or int(N) != N or int(N) < 1:
        raise ValueError(f"N = {N!r}, expected an integer >= 1")
    if isinstance(F, bool) or int(F) != F or not 1 <= int(F) <= _lib.REFINE_MAXF:
        raise ValueError(f"F = {F!r}, expected an integer 1 ... {_lib.REFINE_MAXF}")
    N, F = int(N), int(F)
    u = torch.quasirandom.SobolEngine(2 * F, scramble=True, seed=int(seed)).draw(N, dtype=torch.float64).numpy()
    return np.ascontiguousarray(u[:, :F]), np.ascontiguousarray(u[:, F:])


def sobol_args(params, free, N, bounds, design, seed, column, band_model, lidf):
    """Every argument check of spart_amd.sobol and Engine.sobol that needs no device: refine_plan on ``free`` / ``bounds`` /
    ``column``, the band model's name, lidf, params (a (27, M) block or 27 entries of 1 or M values; M sites), and the design:
    ``design`` = (uA, uB), two (N, F) arrays or tensors used as given (their N counts), or None for sobol_design(N, F, seed).
    N: a multiple of 64 in 128 ... 2^20.  -> (plan, params, M, N, uA, uB); params as refine_args returns it"""
    import torch
    plan = refine_plan(free, bounds, 0, column, 1e-3, 1e-2)
    _band_model(band_model)
    if lidf not in ("literal", "newton"):
        raise ValueError("lidf must be 'literal' or 'newton'")
    F = len(plan["names"])
    if design is not None:
        if not isinstance(design, (tuple, list)) or len(design) != 2:
            raise ValueError("design: expected (uA, uB), two (N, F) arrays")
        uA, uB = (d if torch.is_tensor(d) else np.ascontiguousarray(d, dtype=np.float64) for d in design)
        for name, u in (("uA", uA), ("uB", uB)):
            if len(u.shape) != 2 or int(u.shape[1]) != F:
                raise ValueError(f"design: {name} has shape {tuple(u.shape)}, expected (N, {F})")
        if tuple(uA.shape) != tuple(uB.shape):
            raise ValueError(f"design: uA {tuple(uA.shape)} and uB {tuple(uB.shape)} differ in shape")
        N = int(uA.shape[0])
    if isinstance(N, bool) or int(N) != N or int(N) % _lib.SOBOL_BLOCK or not _lib.SOBOL_MIN_N <= int(N) <= _lib.SOBOL_MAX_N:
        raise ValueError(f"N = {N!r}, expected a multiple of {_lib.SOBOL_BLOCK} in {_lib.SOBOL_MIN_N} ... {_lib.SOBOL_MAX_N}")
    N = int(N)
    M = params_rows(params)
    params = refine_args(params, np.broadcast_to(np.float64(0.0), (M, 1)), free, bounds, None, column, 0, 1e-3, 1e-2, lidf, None,
                         None, None, band_model, _plan=plan)[1]
    if design is None:
        uA, uB = sobol_design(N, F, seed)
    return plan, params, M, N, uA, uB


def vjp_columns(columns, band_model):
    """The sensor columns a vjp() call or a SpartLayer is about: names from R_TOC / R_TOA / L_TOA, at least one, each once, and
    exactly one with band_model "srf" (the SRF forward call writes one column) -> tuple of names, in the caller's order"""
    if isinstance(columns, str):
        columns = (columns,)
    cols = tuple(str(c) for c in columns)
    unknown = [c for c in cols if c not in _lib.REFINE_COLUMNS]
    if unknown:
        raise ValueError(f"columns: unknown column name(s) {unknown}; expected names from {list(_lib.REFINE_COLUMNS)}")
    if not cols:
        raise ValueError("columns: 0 names, expected 1 ... 3")
    twice = sorted({c for c in cols if cols.count(c) > 1})
    if twice:
        raise ValueError(f"columns: {twice} named twice")
    if _band_model(band_model) and len(cols) != 1:
        raise ValueError(f"band_model='srf' takes one column per call, {len(cols)} given: {list(cols)}")
    return cols


def vjp_rel_step(rel_step):
    """rel_step of vjp() / SpartLayer: finite, in (0, 0.5] -> float"""
    if isinstance(rel_step, bool) or not (np.ndim(rel_step) == 0 and np.isfinite(rel_step) and 0 < rel_step <= _lib.VJP_MAX_REL_STEP):
        raise ValueError(f"rel_step = {rel_step!r}, expected a finite value in (0, {_lib.VJP_MAX_REL_STEP}]")
    return float(rel_step)


def vjp_args(params, grad_outputs, free, bounds, rel_step, lidf, band_model, nb=None):
    """Every argument check of spart_amd.vjp and Engine.vjp that needs no device: refine_plan on ``free`` / ``bounds``,
    rel_step in (0, 0.5], the band model's name, lidf, ``grad_outputs`` -- a dict {column name: (M, nb) array or tensor, or
    None for a column that takes no part}, at least one given, all of one shape (``nb`` given: that nb), one only with
    band_model "srf" -- and params (a (27, M) block or 27 entries of 1 or M values).
    -> (plan, params, M, [gy of R_TOC, R_TOA, L_TOA; None where not given]); params as refine_args returns it"""
    plan = refine_plan(free, bounds, 0, "R_TOC", 1e-3, 1e-2)
    rel_step = vjp_rel_step(rel_step)
    if not isinstance(grad_outputs, dict):
        raise ValueError("grad_outputs: expected a dict {column name: (M, nb) tensor}")
    given = {k: v for k, v in grad_outputs.items() if v is not None}
    vjp_columns(tuple(grad_outputs), "centre")
    if not given:
        raise ValueError("grad_outputs: every entry is None")
    vjp_columns(tuple(given), band_model)
    shapes = {k: tuple(int(n) for n in v.shape) if hasattr(v, "shape") else np.shape(v) for k, v in given.items()}
    first = next(iter(shapes.values()))
    for k, s in shapes.items():
        if len(s) != 2 or s != first or (nb is not None and s[1] != nb):
            raise ValueError(f"grad_outputs[{k!r}] has shape {s}, expected (M, nb)" + ("" if nb is None else f" = (M, {nb})") +
                             ("" if s == first else f" like the others, {first}"))
    M = first[0]
    params = refine_args(params, np.broadcast_to(np.float64(0.0), first), free, bounds, None, "R_TOC", 0, 1e-3, 1e-2, lidf, None,
                         None, None, band_model, _plan=plan)[1]
    return dict(plan, rel_step=rel_step), params, M, [given.get(c) for c in _lib.REFINE_COLUMNS]


def sample_args(params, obs, free, bounds, weights, prior, prior_mean, prior_weight, walkers, n_steps, burn, thin, a, temperature,
                rel_init, init, init_radius, step0, obs_offset, seed, column, band_model, lidf, nb=None):
    """Every argument check of spart_amd.sample and Engine.sample that needs no device: refine_args (refine_plan on ``free`` /
    ``bounds`` / ``column``, the prior, the shapes of obs, params and weights), then the sampler's own options: ``walkers`` one
    of 8, 16, 32, 64 with W >= 2 F (None: the smallest such), n_steps 1 ... 2^20, burn 0 ... n_steps - 1 (None: n_steps // 2),
    thin >= 1 with (n_steps - burn) // thin >= 1, a > 1, temperature > 0, rel_init > 0, step0, obs_offset >= 0, seed in
    0 ... 2^64 - 1, init (M, W, F) and init_radius (M, F) or None.
    -> (plan, params, M, weights kind, prior_mean, prior_weight, prior per observation, opt): ``opt`` a dict W, n_steps, burn,
    thin, n_keep, a, temperature, rel_init, step0, obs_offset, seed"""
    head = refine_args(params, obs, free, bounds, weights, column, 0, 1e-3, 1e-2, lidf, prior, prior_mean, prior_weight, band_model, nb=nb)
    plan, M = head[0], head[2]
    F = len(plan["names"])

    def whole(name, v, lo, hi=None):
        if isinstance(v, bool) or int(v) != v or int(v) < lo or (hi is not None and int(v) > hi):
            raise ValueError(f"{name} = {v!r}, expected an integer >= {lo}" + ("" if hi is None else f" and <= {hi}"))
        return int(v)
    if walkers is None:
        walkers = min(w for w in _lib.SAMPLE_WALKERS if w >= 2 * F)
    if isinstance(walkers, bool) or walkers not in _lib.SAMPLE_WALKERS or walkers < 2 * F:
        raise ValueError(f"walkers = {walkers!r}, expected one of {_lib.SAMPLE_WALKERS} and >= 2 F = {2 * F}")
    W = int(walkers)
    n_steps = whole("n_steps", n_steps, 1, _lib.SAMPLE_MAX_STEPS)
    burn = n_steps // 2 if burn is None else whole("burn", burn, 0, n_steps - 1)
    thin = whole("thin", thin, 1)
    if (n_steps - burn) // thin < 1:
        raise ValueError(f"thin = {thin} keeps no step of the {n_steps - burn} after the burn-in")
    for name, v, lo in (("a", a, 1.0), ("temperature", temperature, 0.0), ("rel_init", rel_init, 0.0)):
        if not (np.isfinite(v) and v > lo):
            raise ValueError(f"{name} = {v!r}, expected a finite value > {lo:g}")
    for name, v, shape in (("init", init, (M, W, F)), ("init_radius", init_radius, (M, F))):
        if v is not None and tuple(int(n) for n in v.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(v.shape)}, expected {shape}")
    opt = {"W": W, "n_steps": n_steps, "burn": burn, "thin": thin, "n_keep": (n_steps - burn) // thin, "a": float(a),
           "temperature": float(temperature), "rel_init": float(rel_init), "step0": whole("step0", step0, 0),
           "obs_offset": whole("obs_offset", obs_offset, 0), "seed": whole("seed", seed, 0, 2 ** 64 - 1)}
    return head + (opt,)


def chain_summary(chain, q=(0.05, 0.5, 0.95)):
    """What a chain of sample(chain=True) says about itself, per observation and parameter, on the host.  chain: (M, n_keep, W, F)
    or (n_keep, W, F), a numpy array or a tensor.  -> dict of numpy arrays
      quantiles (M, len(q), F)  over kept steps x walkers
      rhat (M, F)               split-R^: the first and the second half of the kept steps as the two groups (Gelman et al. 2013)
      tau (M, F)                integrated autocorrelation time, in kept steps, of the ensemble-mean series: 1 + 2 sum of the
                                autocorrelations from lag 1 up to (not including) the first negative one
      ess (M, F)                n_keep W / tau
    (the leading axis is dropped for a 3-D chain).  A parameter that does not move has NaN rhat, tau and ess."""
    x = chain.detach().cpu().numpy() if hasattr(chain, "detach") else np.asarray(chain)
    x = np.asarray(x, dtype=np.float64)
    single = x.ndim == 3
    if single:
        x = x[None]
    if x.ndim != 4 or x.shape[1] < 4:
        raise ValueError(f"chain has shape {tuple(np.shape(chain))}, expected (M, n_keep, W, F) or (n_keep, W, F) with n_keep >= 4")
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or not ((q >= 0.0) & (q <= 1.0)).all():
        raise ValueError("q: levels in 0 ... 1")
    M, T, W, F = x.shape
    quant = np.quantile(x.reshape(M, T * W, F), q, axis=1).transpose(1, 0, 2)
    half = T // 2
    with np.errstate(all="ignore"):
        groups = np.stack([x[:, :half].reshape(M, half * W, F), x[:, T - half:].reshape(M, half * W, F)])      # (2, M, n, F)
        n = half * W
        within = groups.var(axis=2, ddof=1).mean(axis=0)
        between = n * groups.mean(axis=2).var(axis=0, ddof=1)
        rhat = np.sqrt(((n - 1) / n * within + between / n) / within)
        series = x.mean(axis=2)                                               # (M, T, F)
        d = series - series.mean(axis=1, keepdims=True)
        size = 1 << int(2 * T - 1).bit_length()
        f = np.fft.rfft(d, n=size, axis=1)
        acov = np.fft.irfft(f * np.conj(f), n=size, axis=1)[:, :T]
        rho = acov / acov[:, :1]
        neg = rho < 0.0
        first = np.where(neg.any(axis=1), neg.argmax(axis=1), T)              # (M, F): the first negative lag
        lag = np.arange(T)[None, :, None]
        tau = 1.0 + 2.0 * np.where((lag >= 1) & (lag < first[:, None, :]), rho, 0.0).sum(axis=1)
        tau = np.where(np.isfinite(rho[:, 0]), tau, np.nan)
        ess = T * W / tau
    res = {"quantiles": quant, "rhat": rhat, "tau": tau, "ess": ess}
    return {k: v[0] for k, v in res.items()} if single else res


BAND_MODELS = ("centre", "srf")
_FIT_OUTS = ("x", "cost", "cost0", "std", "n_accept", "y")     # of spart_refine / _srf / _views, in the order of their argument lists


PRODUCT_NAMES = _lib.PRODUCT_NAMES


def product_names(names=None):
    """``names`` of Engine.products (None = all five, in PRODUCT_NAMES order) -> the tuple asked for, in the caller's order;
    an unknown, repeated or missing name is a ValueError"""
    if names is None:
        return tuple(PRODUCT_NAMES)
    if isinstance(names, str):
        raise ValueError(f"names must be a list of names from {list(PRODUCT_NAMES)}, got the string {names!r}")
    names = tuple(names)
    unknown = [n for n in names if n not in PRODUCT_NAMES]
    if unknown or not names or len(set(names)) != len(names):
        raise ValueError(f"names = {list(names)}: expected distinct names from {list(PRODUCT_NAMES)}"
                         + (f"; unknown {unknown}" if unknown else ""))
    return names


def products_columns(params):
    """The parameter columns spart_products reads, checked without a device: a (27, B) block passes through; a list of 27
    gives its first 22 entries (Cab ... psi; none may be None), the atmosphere and DOY entries are not read and may be None"""
    if isinstance(params, (list, tuple)):
        if len(params) != _lib.NPARAM:
            raise ValueError(f"params must have {_lib.NPARAM} entries, got {len(params)}")
        read = list(params[:_lib.PRODUCTS_NREAD])
        missing = [i for i, c in enumerate(read) if c is None]
        if missing:
            raise ValueError(f"params[{missing[0]}] is None: products read params[0 ... {_lib.PRODUCTS_NREAD - 1}] "
                             f"(only the atmosphere and DOY entries may be None)")
        batch_size(read)
        return read
    shape = tuple(np.shape(params))
    if len(shape) != 2 or shape[0] != _lib.NPARAM:
        raise ValueError(f"params must be (27, B) or a list of 27 columns, got shape {shape}")
    return params


def params_rows(params):
    """the number of rows a params argument of refine() / posterior() stands for when no obs says it: the second axis of a
    (27, M) block, else the largest entry of the list"""
    if isinstance(params, (list, tuple)):
        return max([1] + [math.prod(np.shape(c)) for c in params if c is not None])
    shape = tuple(np.shape(params))
    if len(shape) != 2:
        raise ValueError(f"params must be (27, M) or a list of 27 columns, got shape {shape}")
    return int(shape[1])


def _band_model(band_model, eng=None):
    """band_model= of SPART.run / generate_lut / refine -> True for "srf"; ValueError for anything but "centre" / "srf", and,
    given the engine, for "srf" on one whose SRF columns do not belong to its band centres"""
    if band_model not in BAND_MODELS:
        raise ValueError(f"band_model must be 'centre' or 'srf', got {band_model!r}")
    if eng is None:
        return band_model == "srf"
    if band_model == "srf" and eng.nb == 0:
        raise ValueError("band_model='srf' needs a sensor: this engine was made without one")
    if band_model == "srf" and not np.all(eng.srf_aligned):
        off = np.flatnonzero(~np.asarray(eng.srf_aligned)).tolist()
        raise ValueError(f"band_model='srf': the centres of bands {off} lie outside the wavelength extent of their SRF columns -- "
                         "this sensor's wl_srf_smac / p_srf_smac are in another band order than wl_smac / SMAC_coef; pass "
                         "a sensorinfo mended by spart_amd.align_srf")
    return band_model == "srf"


# ---- the static tables a context is built from (spart_tables): the reference reads them from the dicts it is HANDED at call
# time -- PROSPECT_5D(leafbio, optical_params) prospect_5d.py:158-167, BSM(soilpar, optical_params) bsm.py:45, 54-55,
# SPART.run() self.optipar / self.ETpar / self.sensorinfo SPART.py:93-95, 181-184, 192, 202, 228 -- so an engine is keyed on
# their CONTENT, never on a name or on the identity of a dict.
LEAF_KEYS = ("nr", "Kdm", "Kab", "Kca", "Kw", "Ks", "Kant", "cbc", "prot")       # prospect_5d.py:158-167
SOIL_KEYS = ("GSV", "Kw", "nw")                                                     # bsm.py:45, 54-55
OPTICAL_KEYS = ("nr", "Kab", "Kca", "Kdm", "Kw", "Ks", "Kant", "cbc", "prot", "GSV", "nw")
SENSOR_KEYS = ("wl_smac", "SMAC_coef", "wl_srf_smac", "p_srf_smac")               # SPART.py:216, 228, 376-377

try:                                         # (the digest is a cache key, not a security boundary)
    import xxhash as _xx                     # optional dependency: ~20 us per 230 KB of tables

    def _hasher():
        return _xx.xxh3_128()
    HASHER = "xxhash.xxh3_128"
except ImportError:                          # pragma: no cover
    import hashlib as _hl                    # without xxhash: blake2b, ~0.2 ms per call of a scalar SPART.run() (README states both)

    def _hasher():
        return _hl.blake2b(digest_size=16)
    HASHER = "hashlib.blake2b"


def _digest(arrays):
    h = _hasher()
    for a in arrays:
        h.update(np.asarray(a.shape, dtype=np.int64).tobytes())
        h.update(a.data)
    return h.hexdigest()


def _raw_update(h, v):
    """feed one table value into the hasher WITHOUT converting it: dtype + shape + raw bytes (float64 C-contiguous arrays -- the
    packaged tables -- are hashed in place; anything else through one contiguous copy)"""
    a = v if isinstance(v, np.ndarray) else np.asarray(v)
    if a.dtype == object:
        h.update(repr(a.tolist()).encode())
        return
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    h.update(a.dtype.str.encode())
    h.update(np.asarray(a.shape, dtype=np.int64).tobytes())
    h.update(a.data if a.ndim else a.tobytes())


def raw_digest(optical_params, et_params, sensor_info):
    """Digest of the three reference-style dicts AS THEY ARE (no float64 conversion, no validation): the keys the context is
    built from, in a fixed order.  Equal raw content -> equal converted tables -> the same engine, so a caller (SPART.run) may
    key a small cache on it and skip optical_block / sensor_block on the hot path; any edit of a dict or of an array in place
    changes it.  A missing key hashes as such (the slow path then raises the reference's KeyError).
    C-contiguous arrays go to the hasher through the buffer protocol as they are (~0.4 us each + 20 us for the 230 KB); their
    dtypes and sizes are hashed once at the end."""
    h = _hasher()
    up = h.update
    meta = []
    add = meta.append
    nd = np.ndarray

    def feed(d, k):
        v = d.get(k) if d is not None else None
        if v is None:
            up(b"\0missing:" + k.encode())
        elif type(v) is nd and v.flags.c_contiguous and v.dtype != object:
            up(v)
            add(v.dtype.num)
            add(v.size)
        else:
            _raw_update(h, v)

    for k in OPTICAL_KEYS:
        feed(optical_params, k)
    feed(et_params, "Ea")
    feed(et_params, "wl_Ea")
    for k in ("wl_smac", "wl_srf_smac", "p_srf_smac", "band_id_smac"):
        feed(sensor_info, k)
    coefs = sensor_info.get("SMAC_coef") if sensor_info is not None else None
    if coefs is None:
        up(b"\0nocoef")
    else:
        for n in tables.COEF_NAMES:
            feed(coefs, n)
    up(np.array(meta, dtype=np.int64))
    return h.digest()


def optical_block(optical_params=None, et_params=None, need=OPTICAL_KEYS):
    """The twelve float64 host tables of spart_tables from the reference's dicts.  ``optical_params`` /
    ``et_params`` = None means the packaged tables (load_optical_parameters / load_ET_parameters).  A key of ``need`` that
    the dict lacks is the reference's own KeyError; keys the calling entry point never reads fall back to the packaged
    table.  Anything that is not a 2001-point spectrum (GSV: (2001, 3)) -- or an ET wavelength axis that is not the
    400..2400 nm grid the SRF convolution indexes -- is refused with a ValueError: never a silently different answer."""
    z = tables._npz()
    out = {}
    for k in OPTICAL_KEYS:
        if optical_params is None or (k not in optical_params and k not in need):
            v = z[k]
        else:
            v = optical_params[k]            # KeyError like the reference's optical_params["..."]
        a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
        if k == "GSV":
            if a.shape != (_lib.NWL, 3):
                raise ValueError(f"optical_params['GSV'] has shape {a.shape}, expected ({_lib.NWL}, 3) (bsm.py:45-52)")
        else:
            if a.size != _lib.NWL:
                raise ValueError(f"optical_params[{k!r}] has {a.size} entries, expected the {_lib.NWL} bands 400..2400 nm")
            a = a.reshape(-1)
        out[k] = a
    if et_params is None:
        out["Ea"] = np.ascontiguousarray(z["Ea"], dtype=np.float64)
    else:
        ea = np.ascontiguousarray(np.asarray(et_params["Ea"], dtype=np.float64)).reshape(-1)
        if ea.size != _lib.NWL:
            raise ValueError(f"ETpar['Ea'] has {ea.size} entries, expected {_lib.NWL}")
        wl = np.asarray(et_params["wl_Ea"], dtype=np.float64).reshape(-1) if "wl_Ea" in et_params else None
        if wl is None:
            raise KeyError("wl_Ea")          # SPART.py:184
        if wl.size != _lib.NWL or not np.array_equal(wl, np.arange(400, 2401, dtype=np.float64)):
            raise ValueError("ETpar['wl_Ea'] must be the 1 nm grid 400..2400 nm: the SRF convolution of the device context "
                             "(SPART.py:381-387) indexes that grid")
        out["Ea"] = ea
    return out


def sensor_block(sensor_info):
    """The sensor part of spart_tables from a sensorinfo dict (SPART.py:419-424): float64, validated shapes."""
    for k in SENSOR_KEYS:
        if k not in sensor_info:
            raise KeyError(k)
    wl = np.ascontiguousarray(np.asarray(sensor_info["wl_smac"], dtype=np.float64).reshape(-1))
    nb = wl.shape[0]
    coefs = sensor_info["SMAC_coef"]
    rows = []
    for n in tables.COEF_NAMES:
        r = np.asarray(coefs[n], dtype=np.float64).reshape(-1)       # KeyError like smac.py:44-92
        if r.size != nb:
            raise ValueError(f"SMAC_coef[{n!r}] has {r.size} entries for {nb} sensor bands")
        rows.append(r)
    coef = np.ascontiguousarray(np.stack(rows))
    wsrf = np.ascontiguousarray(np.asarray(sensor_info["wl_srf_smac"], dtype=np.float64))
    psrf = np.ascontiguousarray(np.asarray(sensor_info["p_srf_smac"], dtype=np.float64))
    if wsrf.ndim != 2 or wsrf.shape[1] != nb or psrf.shape != wsrf.shape:
        raise ValueError(f"wl_srf_smac {wsrf.shape} / p_srf_smac {psrf.shape} must both be (nsrf, {nb})")
    return dict(wl=wl, coef=coef, wsrf=wsrf, psrf=psrf)



def quantile_levels(quantiles):
    """Engine.lut_bayes(quantiles=...): a sequence of 1 ... 8 floats in [0, 1] -> a list of floats; anything else is a ValueError"""
    try:
        levels = [float(q) for q in quantiles]
    except (TypeError, ValueError):
        raise ValueError(f"quantiles = {quantiles!r}, expected a sequence of 1 ... {_lib.LUT_BAYES_MAXQ} levels in [0, 1]") from None
    if not 1 <= len(levels) <= _lib.LUT_BAYES_MAXQ or not all(0.0 <= q <= 1.0 for q in levels):
        raise ValueError(f"quantiles = {quantiles!r}, expected 1 ... {_lib.LUT_BAYES_MAXQ} levels, each in [0, 1]")
    return levels


class Engine:
    def __init__(self, sensor=None, device=0, sensor_info=None, lib_path=None, row_pitch=ROW_PITCH, optical_params=None,
                 et_params=None, need=OPTICAL_KEYS):
        """sensor: a packaged sensor name, or None with ``sensor_info`` = a sensorinfo dict (both None: no sensor).
        optical_params / et_params: the reference's table dicts (None = packaged); the context is built from THEIR content.
        row_pitch: (pitch of 2162-wide rows, pitch of 2001-wide rows) or None for dense arrays."""
        torch = _require_gpu()
        self.lib = _lib.load(lib_path)
        self.torch = torch
        self.device = torch.device("cuda", device)
        self.sensor = sensor
        keep = optical_block(optical_params, et_params, need)
        t = _lib.SpartTables()
        for k, v in keep.items():
            setattr(t, k, _dp(v))
        self.nb = 0
        self.srf_aligned = np.zeros(0, dtype=bool)        # no sensor: no bands
        if sensor is not None or sensor_info is not None:
            si = sensor_info if sensor_info is not None else tables.load_sensor_info(sensor)
            self.sensor_info = si
            sb = sensor_block(si)
            keep.update(sb)
            wl, coef, wsrf, psrf = sb["wl"], sb["coef"], sb["wsrf"], sb["psrf"]
            t.nb, t.wl_smac, t.coef = wl.shape[0], _dp(wl), _dp(coef)
            t.nsrf, t.wl_srf, t.p_srf = wsrf.shape[0], _dp(wsrf), _dp(psrf)
            self.nb = int(wl.shape[0])
            self.wl_smac = np.asarray(si["wl_smac"]).reshape(-1)
            self.band_id = list(si["band_id_smac"]) if "band_id_smac" in si else [""] * self.nb
            # per band: the centre lies inside the extent of its SRF column's weighted samples (srf.check_srf).  The *_srf
            # outputs are what the tables say either way; api.SPART.run / generate_lut(band_model="srf") insist on all true
            self.srf_aligned = check_srf(si)
        self._keep = keep
        ctx = _lib.vp()
        rc = self.lib.spart_ctx_create(ctypes.byref(ctx), device, ctypes.byref(t))
        _lib.check(self.lib, None, rc)
        self.ctx = ctx
        self._ws_buf = {}                         # scratch per torch stream (see _workspace)
        self.calls = collections.Counter()        # C-ABI compute calls issued through this engine, by entry point
        self.row_pitch = {_lib.NWLS: _lib.NWLS, _lib.NWL: _lib.NWL}
        if row_pitch is not None:
            pf, po = int(row_pitch[0]), int(row_pitch[1])
            _lib.check(self.lib, self.ctx, self.lib.spart_ctx_set_row_pitch(self.ctx, pf, po))
            self.row_pitch = {_lib.NWLS: pf, _lib.NWL: po}

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.spart_ctx_destroy(self.ctx)
                self.ctx = None
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, dt, B):
        """The scratch buffer of the CURRENT torch stream: calls issued on different streams (from one or several host
        threads) run concurrently on the GPU, so each stream gets its own.  (The library would also accept one buffer for
        all of them -- it orders a call after the previous user of its workspace -- but that serialises the streams.)"""
        n = int(self.lib.spart_workspace_bytes(self.ctx, dt, B))
        key = self.torch.cuda.current_stream(self.device).cuda_stream
        buf = self._ws_buf.get(key)
        if buf is None or buf.numel() < n:
            buf = self._ws_buf[key] = self.torch.empty(max(n, 256), dtype=self.torch.uint8, device=self.device)
        return ctypes.c_void_p(buf.data_ptr()), ctypes.c_size_t(buf.numel())

    def bandsum_layout(self, dtype, B):
        """(byte offset, chunks, row stride in elements) of the per-chunk band sums an unpruned run(dtype, B) leaves in its
        workspace (spart_workspace_bandsum)"""
        off, nchunk, stride = ctypes.c_size_t(), ctypes.c_int64(), ctypes.c_int()
        rc = self.lib.spart_workspace_bandsum(self.ctx, DTYPES[dtype], B, ctypes.byref(off), ctypes.byref(nchunk), ctypes.byref(stride))
        _lib.check(self.lib, self.ctx, rc)
        return int(off.value), int(nchunk.value), int(stride.value)

    def release_workspace(self):
        """Drop the scratch buffers the engine keeps between calls (one per stream used; each grows to the largest batch
        seen: ~0.9 KB per sample); the next call allocates what it needs."""
        self._ws_buf = {}

    def to_f64(self, x, B):
        """scalar / sequence / numpy / tensor of 1 or B values (batch_size) -> contiguous float64 device tensor of length B."""
        torch = self.torch
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x, dtype=np.float64))
        return x.to(device=self.device, dtype=torch.float64).reshape(-1).expand(B).contiguous()

    def columns(self, cols, B=None):
        """list of per-parameter values -> (list of (B,) tensors, B); B = batch_size(cols) unless given.  Host values (scalars,
        sequences, numpy arrays) travel in ONE host-to-device copy of an (n, B) block (a scalar SPART.run() used to issue 29
        one-element copies: half its 0.9 ms); device tensors are used where they are."""
        torch = self.torch
        if B is None:
            B = batch_size(cols)
        host = [i for i, c in enumerate(cols) if not torch.is_tensor(c)]
        out = [None] * len(cols)
        if host:
            blk = np.empty((len(host), B), dtype=np.float64)
            for k, i in enumerate(host):
                blk[k] = np.asarray(cols[i], dtype=np.float64).reshape(-1)
            dev = torch.as_tensor(blk).to(self.device)
            for k, i in enumerate(host):
                out[i] = dev[k]
        for i, c in enumerate(cols):
            if out[i] is None:
                out[i] = self.to_f64(c, B)
        return out, B

    @staticmethod
    def _nlayers(n):
        """canopy.nlayers -> the C ABI's int (0 = default).  The reference slices Pso[0:nl] (sailh.py:216): integers only."""
        if n is None:
            return 0
        import numbers
        if isinstance(n, bool) or not isinstance(n, (numbers.Integral, np.integer)):
            if np.ndim(n) != 0:
                raise ValueError("canopy.nlayers must be ONE integer per call (sailh.py:48)")
            raise TypeError(f"canopy.nlayers must be an integer, got {type(n).__name__} (the reference slices Pso[0:nl], sailh.py:216)")
        n = int(n)
        if n < 1 or n > 1000000:
            raise ValueError(f"canopy.nlayers = {n}: expected 1 ... 1000000")
        return n

    def _ptrs(self, tensors):
        arr = (_lib.vp * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])
        return arr

    def _tdtype(self, dt):
        return self.torch.float32 if dt == _lib.SPART_F32 else self.torch.float64

    def _alloc_spec(self, B, width, td):
        """(B, width) array on this context's row pitch (a view of padded storage when pitch > width; lidf rows are dense)."""
        pitch = self.row_pitch.get(width, width)
        return self.torch.empty((B, pitch), dtype=td, device=self.device)[:, :width]

    def _rows(self, x, B, width, td):
        """an input row-set (spectra, or canopy.lidf as the caller set it) whose row count batch_size() has checked against B
        -> (B, width) device tensor of dtype td laid out as _alloc_spec lays it out (the input itself when it already is)"""
        torch = self.torch
        if not torch.is_tensor(x):
            x = torch.as_tensor(np.asarray(x))
        x = x.to(device=self.device, dtype=td).reshape(-1, width).expand(B, width)
        if _on_rows(x, self.row_pitch.get(width, width)):
            return x
        buf = self._alloc_spec(B, width, td)
        buf.copy_(x)
        return buf

    # ------------------------------------------------------------------ operators
    def prospect(self, leaf9, dtype="float64", outputs=("refl", "tran", "kChlrel")):
        """PROSPECT_5D for a batch (prospect_5d.py:117-246): leaf9 = [Cab,Cdm,Cw,Cs,Cca,Cant,N,PROT,CBC].
        -> [refl, tran, kChlrel], each (B, 2001); entries not named in ``outputs`` are None (not computed / stored)."""
        dt = DTYPES[dtype]
        cols, B = self.columns(leaf9)
        td = self._tdtype(dt)
        out = [self._alloc_spec(B, _lib.NWL, td) if n in outputs else None for n in ("refl", "tran", "kChlrel")]
        ws, wsn = self._workspace(dt, B)
        self.calls["spart_prospect_batch"] += 1
        rc = self.lib.spart_prospect_batch(self.ctx, dt, B, self._ptrs(cols), *[o.data_ptr() if o is not None else None for o in out],
                                           ws, wsn, self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return out

    def bsm(self, soil6, dtype="float64", rdry=None):
        """BSM (bsm.py:17-128): soil6 = [B,lat,lon,SMp,SMC,film]; rdry = optional (B,2001) dry spectra."""
        dt = DTYPES[dtype]
        soil6 = fill_nulls(soil6, 9, rdry=rdry)
        cols, B = self.columns(soil6, batch_size(soil6, [(rdry, _lib.NWL)]))
        td = self._tdtype(dt)
        rd = self._rows(rdry, B, _lib.NWL, td) if rdry is not None else None
        out = [self._alloc_spec(B, _lib.NWL, td) for _ in range(2)]
        ws, wsn = self._workspace(dt, B)
        self.calls["spart_bsm_batch"] += 1
        rc = self.lib.spart_bsm_batch(self.ctx, dt, B, self._ptrs(cols), rd.data_ptr() if rd is not None else None,
                                      out[0].data_ptr(), out[1].data_ptr(), ws, wsn, self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return out

    def lidf(self, LIDFa, LIDFb):
        cols, B = self.columns([LIDFa, LIDFb])
        out = self.torch.empty((B, _lib.NLINCL), dtype=self.torch.float64, device=self.device)
        self.calls["spart_lidf_batch"] += 1
        rc = self.lib.spart_lidf_batch(self.ctx, B, cols[0].data_ptr(), cols[1].data_ptr(), out.data_ptr(),
                                       self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return out

    def sailh(self, rho, tau, rs, canopy4, angles3, dtype="float64", canopy_lidf=None, nlayers=None):
        """SAILH (sailh.py:14-237) on (B,2162) spectra.  canopy_lidf / nlayers: canopy.lidf ((13,), (13,1) or (B,13)) and
        canopy.nlayers as the reference reads them from the object at call time (sailh.py:48, 51); None = derived from
        LIDFa / LIDFb, 60."""
        dt = DTYPES[dtype]
        nl = self._nlayers(nlayers)
        vals = fill_nulls(list(canopy4) + list(angles3), 15, canopy_lidf=canopy_lidf)
        B = batch_size(vals, [(rho, _lib.NWLS), (tau, _lib.NWLS), (rs, _lib.NWLS), (canopy_lidf, _lib.NLINCL)])
        cols, _ = self.columns(vals, B)
        td = self._tdtype(dt)
        li = self._rows(canopy_lidf, B, _lib.NLINCL, self.torch.float64) if canopy_lidf is not None else None
        rho, tau, rs = (self._rows(x, B, _lib.NWLS, td) for x in (rho, tau, rs))
        out = [self._alloc_spec(B, _lib.NWLS, td) for _ in range(4)]
        ws, wsn = self._workspace(dt, B)
        self.calls["spart_sailh_batch"] += 1
        rc = self.lib.spart_sailh_batch(self.ctx, dt, B, rho.data_ptr(), tau.data_ptr(), rs.data_ptr(),
                                        self._ptrs(cols[:4]), self._ptrs(cols[4:]), li.data_ptr() if li is not None else None,
                                        nl, self._ptrs(out), ws, wsn, self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return out

    def smac(self, angles3, atm4):
        """SMAC (smac.py:14-213): nine (B,nb) float64 tensors in AtmosphericOptics order."""
        cols, B = self.columns(list(angles3) + list(atm4))
        out = [self.torch.empty((B, self.nb), dtype=self.torch.float64, device=self.device) for _ in range(9)]
        ws, wsn = self._workspace(_lib.SPART_F64, B)
        self.calls["spart_smac_batch"] += 1
        rc = self.lib.spart_smac_batch(self.ctx, B, self._ptrs(cols[:3]), self._ptrs(cols[3:]), self._ptrs(out), ws, wsn,
                                       self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return dict(zip(SMAC_FIELDS, out))

    def run(self, params, dtype="float32", rho_thermal=None, tau_thermal=None, materialize=(), out=None,
            prune=False, rdry=None, f32_columns=False, f32_bands=False, lidf="literal", _workspace=None,
            canopy_lidf=None, nlayers=None, _defer=False):
        """SPART(...).run() for every column of ``params`` (SPART.py:162-269).

        params : (27, B) float64 device tensor (rows = spart_amd.workloads.PARAM_NAMES) or a list of 27
                 scalars / arrays.
        materialize : iterable of names from MATERIALIZE_FIELDS to also return (full spectra etc.; the seven ``*_srf`` names
              are the SRF-convolved sensor columns, (B, nb): the band's spectral response function applied to the canopy
              spectra instead of a sample at the band centre -- float64 column path in every mode, not with f32_columns)
        out : optional dict with preallocated 'R_TOC','R_TOA','L_TOA' (B,nb) tensors and / or preallocated tensors for
              names in ``materialize`` (spectrum arrays on this engine's row pitch, e.g. a previous call's results)
        prune : False (default) evaluates all 2162 bands of every sample; True lets the kernel skip bands
                that no requested output needs (identical columns, much less work)
        rdry : optional (B, 2001) / (2001,) user dry-soil spectra replacing the GSV mixing (bsm.py:42-43);
               the B / lat / lon entries of ``params`` are then ignored (may be None in a list)
        f32_bands : float64 only.  True: float64 columns identical to the float64 mode's over a float32 evaluation of
               the 2162 bands (spart_materialize.f32_bands): reference precision at the float32 mode's speed
        lidf : "literal" (default) = the reference's LIDF fixed-point iteration with its stopping rule and 10-point hot-spot
               panels; "newton" = spart_materialize.fast_prelude: the exact root + 8-point panels, columns within 1e-7
               relative of the default, the prelude kernel twice as fast
        f32_columns : float32 only.  False (default): the bands the sensor columns depend on are re-evaluated in
               float64, the columns are the float64 mode's values rounded to float32; True: columns straight from
               the float32 band arithmetic (spart_materialize.f32_columns)
        canopy_lidf : optional canopy.lidf as the caller set it, (13,), (13,1) or (B,13) (spart_materialize.lidf_in; the
               reference's SAILH reads it from the object, sailh.py:51); the LIDFa / LIDFb entries of ``params`` are then
               ignored (may be None in a list)
        nlayers : optional canopy.nlayers, one integer per call (spart_materialize.nlayers; sailh.py:48); None = 60
        """
        torch = self.torch
        dt = DTYPES[dtype]
        td = self._tdtype(dt)
        rows = [(rdry, _lib.NWL), (canopy_lidf, _lib.NLINCL)]
        col_ptrs = cols = None
        if torch.is_tensor(params) and params.dim() == 2:
            if params.shape[0] != _lib.NPARAM:
                raise ValueError("params must be (27, B)")
            P = params.to(device=self.device, dtype=torch.float64).contiguous()
            B = batch_size((rho_thermal, tau_thermal), rows, P.shape[1])
            base = P.data_ptr()                     # row i of the contiguous block: no 27 tensor views, no 27 data_ptr() calls
            col_ptrs = (_lib.vp * _lib.NPARAM)(*[base + 8 * B * i for i in range(_lib.NPARAM)])
        else:
            if len(params) != _lib.NPARAM:
                raise ValueError(f"params must have {_lib.NPARAM} entries, got {len(params)}")
            plist = fill_nulls(params, rdry=rdry, canopy_lidf=canopy_lidf)
            B = batch_size(plist + [rho_thermal, tau_thermal], rows)
            cols, _ = self.columns(plist, B)
        nl = self._nlayers(nlayers)
        li = self._rows(canopy_lidf, B, _lib.NLINCL, torch.float64) if canopy_lidf is not None else None
        th = [None if x is None else self.to_f64(x, B) for x in (rho_thermal, tau_thermal)]
        res = dict(out) if out is not None else {}       # (the caller's dict is not modified)
        for k in ("R_TOC", "R_TOA", "L_TOA"):
            if k not in res:
                res[k] = torch.empty((B, self.nb), dtype=td, device=self.device)
            else:
                self._check_out(k, res[k], (B, self.nb), td, self.nb)
        mat = None
        rd = None
        if lidf not in ("literal", "newton"):
            raise ValueError("lidf must be 'literal' or 'newton'")
        if materialize or prune or rdry is not None or f32_columns or f32_bands or lidf == "newton" or li is not None or nl:
            mat = _lib.SpartMaterialize()
            mat.lidf_in = li.data_ptr() if li is not None else None
            mat.nlayers = nl
            mat.fast_prelude = 1 if lidf == "newton" else 0
            mat.prune_unused_bands = 1 if prune else 0
            mat.f32_columns = 1 if f32_columns else 0
            mat.f32_bands = 1 if f32_bands else 0
            if rdry is not None:
                rd = self._rows(rdry, B, _lib.NWL, td)
                mat.rdry_in = rd.data_ptr()
            for name in materialize:
                if name not in MATERIALIZE_FIELDS:
                    raise ValueError(f"unknown materialize field {name}")
                w = _MAT_WIDTH.get(name)
                shape = (B, w) if w else ((4, _lib.NWLS) if name == "band_mean" else (B, self.nb))
                if name in res:                     # caller-owned buffer (out=): must already have this context's layout
                    self._check_out(name, res[name], shape, td, self.row_pitch[w] if w else shape[1])
                elif w:
                    res[name] = self._alloc_spec(B, w, td)
                else:
                    res[name] = torch.empty(shape, dtype=td, device=self.device)
                setattr(mat, name, res[name].data_ptr())
        if _defer and _workspace is None:                  # a prepared call owns its scratch (other calls on the engine do not disturb it)
            n = int(self.lib.spart_workspace_bytes(self.ctx, dt, B))
            _workspace = torch.empty(max(n, 256), dtype=torch.uint8, device=self.device)
        if _workspace is not None:
            ws, wsn = ctypes.c_void_p(_workspace.data_ptr()), ctypes.c_size_t(_workspace.numel())
        else:
            ws, wsn = self._workspace(dt, B)
        args = (self.ctx, dt, B, col_ptrs if col_ptrs is not None else self._ptrs(cols),
                th[0].data_ptr() if th[0] is not None else None, th[1].data_ptr() if th[1] is not None else None,
                res["R_TOC"].data_ptr(), res["R_TOA"].data_ptr(), res["L_TOA"].data_ptr(),
                ctypes.byref(mat) if mat is not None else None, ws, wsn)
        if not _defer:
            self.calls["spart_run_batch"] += 1
            rc = self.lib.spart_run_batch(*args, self._stream())
            _lib.check(self.lib, self.ctx, rc)
            return res
        # everything the argument pointers point into, and the engine: its __del__ destroys the context the call uses
        keep = (params, cols, th, li, rd, mat, res, _workspace, self)
        lib, ctx, calls, stream_of, device = self.lib, self.ctx, self.calls, self.torch.cuda.current_stream, self.device

        def call():
            calls["spart_run_batch"] += 1
            rc = lib.spart_run_batch(*args, ctypes.c_void_p(stream_of(device).cuda_stream))
            if rc:
                _lib.check(lib, ctx, rc)
            return keep[6]
        return call

    def products(self, params, names=None, out=None):
        """fAPAR and albedo, black- and white-sky, and fCover of every column of ``params`` (include/spart_hip.h: spart_products,
        which defines them; float64; no sensor needed).  ``params`` as for run(): a (27, B) float64 block or a list of 27
        scalars / arrays, of which the atmosphere and DOY entries (22 ... 26) are not read and may be None.  ``names``: which of
        PRODUCT_NAMES to compute, in the order wanted (None = all five); only those are asked of the kernel.  ``out``: optional
        dict of preallocated (B,) float64 tensors on the engine's device for some of the names.
        -> dict {name: (B,) float64 device tensor} in the order of ``names``."""
        torch = self.torch
        names = product_names(names)
        params = products_columns(params)
        if out is not None and set(out) - set(names):
            raise ValueError(f"out has entries {sorted(set(out) - set(names))} that names = {list(names)} does not ask for")
        if isinstance(params, list):
            cols, B = self.columns(params)
            col_ptrs = self._ptrs(cols + [None] * (_lib.NPARAM - len(cols)))
        else:
            P = cols = torch.as_tensor(params).to(device=self.device, dtype=torch.float64).contiguous()
            B = P.shape[1]
            col_ptrs = (_lib.vp * _lib.NPARAM)(*[P.data_ptr() + 8 * B * i for i in range(_lib.NPARAM)])
        res = {}
        for n in names:
            if out is not None and n in out:
                self._check_out(n, out[n], (B,), torch.float64, 1)
                res[n] = out[n]
            else:
                res[n] = torch.empty((B,), dtype=torch.float64, device=self.device)
        po = _lib.SpartProductsOut()
        for n, (field, _) in zip(PRODUCT_NAMES, _lib.SpartProductsOut._fields_):
            setattr(po, field, res[n].data_ptr() if n in res and B > 0 else None)
        ws, wsn = self._workspace(_lib.SPART_F64, B)
        self.calls["spart_products"] += 1
        rc = self.lib.spart_products(self.ctx, B, col_ptrs, ctypes.byref(po), ws, wsn, self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return res

    def prepare(self, params, dtype="float32", out=None, **kw):
        """run() with its argument marshalling done ONCE: returns ``call()`` which issues the same spart_run_batch on the current
        stream over the SAME resident buffers (``params`` a (27, B) float64 device tensor, ``out`` the preallocated results, any
        thermal / lidf tensors), with nothing but the ctypes call on the hot path -- what a loop over small batches wants when
        a HIP-graph capture is too rigid (the stream may change from call to call).  The call owns its workspace."""
        torch = self.torch
        self._check_resident("prepare", params, out)
        if kw.get("rdry") is not None:
            raise ValueError("prepare(): user dry-soil spectra are re-laid out per call (row pitch): use run()")
        for k in ("rho_thermal", "tau_thermal", "canopy_lidf"):
            v = kw.get(k)
            if v is not None and not (torch.is_tensor(v) and v.device == self.device):
                raise ValueError(f"prepare(): {k} must be a tensor on the engine's device (its storage is reused by every call)")
        return self.run(params, dtype, out=out, _defer=True, **kw)

    def _check_out(self, name, t, shape, td, row_stride):
        """a caller-supplied output must be exactly what the kernels write: they get its data_ptr() and ``row_stride``"""
        if not self.torch.is_tensor(t):
            got = type(t)
        elif tuple(t.shape) == tuple(shape) and t.dtype == td and t.device == self.device and _on_rows(t, row_stride):
            return
        else:
            got = f"{tuple(t.shape)} {t.dtype} on {t.device} with strides {t.stride()}"
        raise ValueError(f"out[{name!r}] must be a {tuple(shape)} {td} tensor on {self.device} with contiguous rows at row "
                         f"stride {row_stride}, got {got}")

    def _check_resident(self, what, params, out):
        """prepare() / capture(): the call reuses the storage of ``params`` and of the three result tensors every time"""
        torch = self.torch
        if not (torch.is_tensor(params) and params.dim() == 2 and params.dtype == torch.float64 and params.is_contiguous()
                and params.device == self.device):
            raise ValueError(f"{what}() needs a contiguous (27, B) float64 tensor on the engine's device")
        if out is None or any(k not in out for k in ("R_TOC", "R_TOA", "L_TOA")):
            raise ValueError(f"{what}() needs preallocated out['R_TOC'|'R_TOA'|'L_TOA']")

    def capture(self, params, dtype="float32", out=None, **kw):
        """Record one run() over RESIDENT buffers into a HIP graph and return its replay function (no arguments;
        results land in ``out``).  For steps of a few kernels on small batches (100k spectra: 1.3 ms) the replay
        removes the per-launch host work and the gaps between the dependent kernels.  ``params`` must be a (27, B)
        float64 device tensor and ``out`` the three (B, nb) result tensors; the graph owns its workspace, so other
        calls on this engine do not disturb it.  spart_run_batch allocates nothing and never synchronises, which is
        what makes it capturable."""
        torch = self.torch
        self._check_resident("capture", params, out)
        dt = DTYPES[dtype]
        n = int(self.lib.spart_workspace_bytes(self.ctx, dt, params.shape[1]))
        ws = torch.empty(max(n, 256), dtype=torch.uint8, device=self.device)
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self.run(params, dtype, out=out, _workspace=ws, **kw)         # warm-up outside the capture
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                res = self.run(params, dtype, out=out, _workspace=ws, **kw)
        torch.cuda.current_stream(self.device).wait_stream(s)
        keep = (ws, params, res, self)                                     # buffers the graph points into, and their context

        def replay():
            g.replay()
            return keep[2]
        replay.graph = g
        return replay

    def lut_nearest(self, lut, obs, weights=None, dtype="float32", stats=False):
        """LUT inversion: for each row of obs (M, nb) the index of THE closest row of lut (B, nb) under the weighted squared
        distance ``c = sum_j (w_j * d_j) * d_j``, ``d = lut - obs`` (sequential, rounded to ``dtype``, no FMA), lowest index on
        ties, and that distance -- bit-exact against a brute-force loop (include/spart_hip.h: spart_lut_nearest).
        -> (idx (M,) int64 tensor, cost (M,) tensor); with ``stats=True`` also a dict with the number of observations that
        took the brute-force path and the scale Nmax of the rounding bound (spart_lut_stats; synchronises).
        ``weights`` (M, nb): one weight row per observation, a zero weight masking its band (lut_topk with k = 1)."""
        return self._lut_search(lut, obs, weights, None, dtype, stats)

    def lut_topk(self, lut, obs, k, weights=None, dtype="float32", stats=False):
        """The k nearest LUT rows per observation (include/spart_hip.h: spart_lut_topk): the same cost as lut_nearest, rows
        ordered by (cost, row index) -- np.argsort(cost, kind="stable")[:k] with non-finite costs set to +inf -- bit-exact,
        padded with (-1, +inf) when fewer than k rows have a finite cost.  1 <= k <= 256.
        -> (idx (M, k) int64 tensor, cost (M, k) tensor); with ``stats=True`` also a dict with the number of observations that
        took the brute-force path, the candidate tiles (sum and maximum per observation) and Nmax (spart_lut_topk_stats;
        synchronises).  ``weights`` is None, (nb,) -- one weight per band for every observation -- or (M, nb): one weight row
        per observation (spart_lut_topk_obs_weights, any nb): a band of weight zero is skipped, so the observation may be NaN
        there; the stats then report "nbound" (the largest per-observation bound scale) in place of "nmax"."""
        return self._lut_search(lut, obs, weights, k, dtype, stats)

    def _lut_search(self, lut, obs, weights, k, dtype, stats):
        """lut_nearest (``k`` None) and lut_topk: the tensors on the device, in ``dtype`` and contiguous; the choice of the
        search; its outputs and workspace; the counted and checked call; with ``stats`` a synchronise and the search's *_stats.
        The search: (M, nb) weights -> spart_lut_topk_obs_weights; else above LUT_NARROW_NB bands -> spart_lut_topk_wide;
        else spart_lut_nearest / spart_lut_topk.  Only spart_lut_nearest has no k ((M,) outputs, no candidate counters): the
        other two serve lut_nearest with k = 1 and column 0 of their answer."""
        torch = self.torch
        dt = DTYPES[dtype]
        td = self._tdtype(dt)
        if k is not None:
            k = int(k)
        lut = torch.as_tensor(lut).to(device=self.device, dtype=td).contiguous()
        obs = torch.as_tensor(obs).to(device=self.device, dtype=td).contiguous()
        if lut.dim() != 2 or obs.dim() != 2 or lut.shape[1] != obs.shape[1]:
            raise ValueError("lut (B, nb) and obs (M, nb) must share nb")
        w = None if weights is None else torch.as_tensor(weights).to(device=self.device, dtype=td).contiguous()
        B, nb = lut.shape
        M = obs.shape[0]
        if lut_weights_kind(None if w is None else w.shape, M, nb) == "per_observation":
            entry = "spart_lut_topk_obs_weights"
        elif nb > LUT_NARROW_NB:
            entry = "spart_lut_topk_wide"
        else:
            entry = "spart_lut_nearest" if k is None else "spart_lut_topk"
        workspace_bytes, read_stats, scale = _LUT_SEARCHES[entry]
        kk = () if entry == "spart_lut_nearest" else (1 if k is None else k,)
        shape = (M, max(kk[0], 0)) if kk else (M,)
        idx = torch.empty(shape, dtype=torch.int64, device=self.device)
        cost = torch.empty(shape, dtype=td, device=self.device)
        nbytes = max(getattr(self.lib, workspace_bytes)(dt, B, nb, M, *kk), 256)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.calls[entry] += 1
        rc = getattr(self.lib, entry)(self.ctx, dt, B, nb, lut.data_ptr(), M, obs.data_ptr(),
                                      w.data_ptr() if w is not None else None, *kk, idx.data_ptr(), cost.data_ptr(),
                                      ws.data_ptr(), nbytes, self._stream())
        _lib.check(self.lib, self.ctx, rc)
        res = (idx[:, 0], cost[:, 0]) if kk and k is None else (idx, cost)
        if not stats:
            return res
        names = ("brute_force", "candidate_tiles", "max_candidate_tiles") if kk else ("brute_force",)
        counts, word = [ctypes.c_int64(0) for _ in names], ctypes.c_double(0.0)
        if M > 0:
            torch.cuda.current_stream(self.device).synchronize()
            _lib.check(self.lib, self.ctx, getattr(self.lib, read_stats)(
                self.ctx, dt, B, nb, M, *kk, ws.data_ptr(), *[ctypes.byref(c) for c in counts], ctypes.byref(word)))
        return res + ({**{n: int(c.value) for n, c in zip(names, counts)}, scale: float(word.value)},)

    def lut_summarise(self, params, idx):
        """count, mean, median and standard deviation (ddof = 0) of the parameter rows ``params[idx[m]]`` per observation,
        on the device (include/spart_hip.h: spart_lut_summarise, which pins the order of every sum): entries of ``idx`` outside
        0 ... B-1 -- the -1 padding of lut_topk -- are skipped, duplicated rows count as often as they appear, an observation
        without rows gets count 0 and NaN.  Unlike spart_amd.summarise_rows on a padded observation (numpy's nan* forms), NaN
        parameter VALUES propagate; LUT parameter tables hold none, so the two agree on every real table.
        ``params`` (B, P): anything torch.as_tensor takes, moved to the engine's device as contiguous float64 (a tensor already
        there is used as it is, no copy); ``idx`` (M, k) int64, e.g. lut_topk's.  1 <= P <= 64, 1 <= k <= 256.
        -> dict of device tensors: mean, median, std (M, P) float64 and count (M,) int32."""
        torch = self.torch
        params = torch.as_tensor(params).to(device=self.device, dtype=torch.float64).contiguous()
        idx = torch.as_tensor(idx).to(device=self.device, dtype=torch.int64).contiguous()
        if params.dim() != 2 or idx.dim() != 2:
            raise ValueError("params must be (B, P) and idx (M, k)")
        B, P = params.shape
        M, k = idx.shape
        res = {n: torch.empty((M, P), dtype=torch.float64, device=self.device) for n in ("mean", "median", "std")}
        res["count"] = torch.empty((M,), dtype=torch.int32, device=self.device)
        self.calls["spart_lut_summarise"] += 1
        rc = self.lib.spart_lut_summarise(self.ctx, B, P, params.data_ptr(), M, k, idx.data_ptr(), res["mean"].data_ptr(),
                                          res["median"].data_ptr(), res["std"].data_ptr(), res["count"].data_ptr(),
                                          self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return res

    def lut_bayes(self, lut, params, obs, weights=None, cut=50.0, temperature=1.0, dtype="float32", stats=False, brute_force=False,
                  quantiles=None):
        """The likelihood-weighted LUT estimate (include/spart_hip.h: spart_lut_bayes, which pins every sum): every accepted row b
        of lut (B, nb) whose cost lies within ``cut`` of the best one, e_b = c(b) - c* <= cut, gets the weight
        exp(-e_b / (2 temperature)); the cost is lut_topk's with (M, nb) weights (chi^2 when the weights are 1 / sigma^2).
        ``params`` (B, P) float64, 1 <= P <= 64; ``weights`` None (ones), (nb,) (expanded to (M, nb) on the device: the C call
        knows one layout) or (M, nb), a zero weight masking its band.  ``cut`` >= 0 or inf (every accepted row).
        -> dict of device tensors: mean, std (M, P) float64 -- the weighted mean and spread of the parameter rows --, sum_w, ess
        (M,) float64 -- the effective sample size (sum w)^2 / sum w^2 --, count, best_idx (M,) int64 and best_cost (M,) in
        ``dtype`` (lut_topk(k=1)'s, bit for bit); an observation that matches nothing gets count 0, best_idx -1, best_cost inf,
        sum_w 0 and NaN.  ``brute_force=True`` sends every observation through the brute-force kernel (the same result bit for
        bit).  With ``stats=True`` -> (dict, stats): brute-forced observations, candidate tiles (sum and maximum) and "nbound"
        (spart_lut_bayes_stats; synchronises).
        ``quantiles``: None, or 1 ... 8 levels in [0, 1] (ValueError otherwise, before any GPU work): the call is then
        spart_lut_bayes_quantiles and the dict gains "quantiles", (M, P, Q) float64 -- per parameter and level the smallest
        value of the column whose omega-weighted share of the set reaches the level (the inverted-CDF quantile: a table value,
        0.5 the lower median; NaN where the column holds a NaN over the set or nothing matched); every other entry is the same
        bits as without."""
        levels = None if quantiles is None else quantile_levels(quantiles)
        torch = self.torch
        dt = DTYPES[dtype]
        td = self._tdtype(dt)
        lut = torch.as_tensor(lut).to(device=self.device, dtype=td).contiguous()
        obs = torch.as_tensor(obs).to(device=self.device, dtype=td).contiguous()
        params = torch.as_tensor(params).to(device=self.device, dtype=torch.float64).contiguous()
        if lut.dim() != 2 or obs.dim() != 2 or lut.shape[1] != obs.shape[1]:
            raise ValueError("lut (B, nb) and obs (M, nb) must share nb")
        B, nb = lut.shape
        M = obs.shape[0]
        if params.dim() != 2 or params.shape[0] != B:
            raise ValueError(f"params must be (B, P) = ({B}, P), got shape {tuple(params.shape)}")
        P = params.shape[1]
        if weights is None:
            w = torch.ones((M, nb), dtype=td, device=self.device)
        else:
            w = torch.as_tensor(weights).to(device=self.device, dtype=td)
            if lut_weights_kind(w.shape, M, nb) == "shared":
                w = w.expand(M, nb)
            w = w.contiguous()
        res = {n: torch.empty((M, P), dtype=torch.float64, device=self.device) for n in ("mean", "std")}
        res.update({n: torch.empty((M,), dtype=torch.float64, device=self.device) for n in ("sum_w", "ess")})
        res.update({n: torch.empty((M,), dtype=torch.int64, device=self.device) for n in ("count", "best_idx")})
        res["best_cost"] = torch.empty((M,), dtype=td, device=self.device)
        opt = _lib.SpartLutBayesOpt(float(cut), float(temperature), int(bool(brute_force)))
        out = _lib.SpartLutBayesOut(*[res[n].data_ptr() for n in _lib.LUT_BAYES_OUTS])
        nbytes = max(self.lib.spart_lut_bayes_workspace_bytes(dt, B, nb, M), 256)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if levels is None:
            self.calls["spart_lut_bayes"] += 1
            rc = self.lib.spart_lut_bayes(self.ctx, dt, B, nb, lut.data_ptr(), P, params.data_ptr(), M, obs.data_ptr(), w.data_ptr(),
                                          ctypes.byref(opt), ctypes.byref(out), ws.data_ptr(), nbytes, self._stream())
        else:
            res["quantiles"] = torch.empty((M, P, len(levels)), dtype=torch.float64, device=self.device)
            qopt = _lib.SpartLutBayesQOpt(opt, len(levels), (ctypes.c_double * len(levels))(*levels))
            qout = _lib.SpartLutBayesQOut(out, res["quantiles"].data_ptr())
            self.calls["spart_lut_bayes_quantiles"] += 1
            rc = self.lib.spart_lut_bayes_quantiles(self.ctx, dt, B, nb, lut.data_ptr(), P, params.data_ptr(), M, obs.data_ptr(),
                                                    w.data_ptr(), ctypes.byref(qopt), ctypes.byref(qout), ws.data_ptr(), nbytes,
                                                    self._stream())
        _lib.check(self.lib, self.ctx, rc)
        if not stats:
            return res
        names = ("brute_force", "candidate_tiles", "max_candidate_tiles")
        counts, word = [ctypes.c_int64(0) for _ in names], ctypes.c_double(0.0)
        if M > 0 and B > 0:
            torch.cuda.current_stream(self.device).synchronize()
            _lib.check(self.lib, self.ctx, self.lib.spart_lut_bayes_stats(
                self.ctx, dt, B, nb, M, ws.data_ptr(), *[ctypes.byref(c) for c in counts], ctypes.byref(word)))
        return res, {**{n: int(c.value) for n, c in zip(names, counts)}, "nbound": float(word.value)}

    def _refine_columns(self, params, M):
        """the start rows of refine() / posterior() as 27 float64 device columns of M values"""
        if self.torch.is_tensor(params):
            P = params.to(device=self.device, dtype=self.torch.float64)
            return list(P.expand(_lib.NPARAM, M).contiguous()) if M else list(P)
        return self.columns(params, M)[0]

    def _fit_outputs(self, M, n, yshape):
        """the six outputs of a fit of n unknowns per observation, in the order of the C argument list (_FIT_OUTS)"""
        torch = self.torch
        shapes = {"x": (M, n), "cost": (M,), "cost0": (M,), "std": (M, n), "n_accept": (M,), "y": yshape}
        return {k: torch.empty(shapes[k], dtype=torch.int32 if k == "n_accept" else torch.float64, device=self.device) for k in _FIT_OUTS}

    def _refine_device(self, entry, plan, M, cols, obs, weights, wper, lidf, nl, prior, outs, views=None, tiles=None, series=None,
                       mix=None):
        """What every entry point of the refinement family does once its parameter columns ``cols`` and its outputs are on the
        device: obs and weights as float64 device tensors, spart_refine_opt from the plan, the prior (mean, weight, per
        observation 0 / 1) hooked up, the workspace, the call count, the C call and its check.  ``outs``: the C arguments between
        the options and the workspace; ``views`` = (V, Fs, srf) wraps the options in spart_refine_views_opt;
        ``tiles`` = (Fs, srf, tile_start, shared prior) wraps them in spart_refine_tiles_opt and passes the partition;
        ``series`` = (gamma, link) with ``tiles`` wraps those in spart_refine_series_opt; ``mix`` = (V, Fs, srf, fit_fractions,
        active, frac_lo, frac_hi, n, fractions) wraps them in spart_refine_mix_opt and passes the fractions after the weights.
        -> (obs, weights) as the call got them"""
        torch = self.torch
        f64 = dict(dtype=torch.float64, device=self.device)
        o = None if obs is None else torch.as_tensor(obs).to(**f64).contiguous()
        w = None if weights is None else torch.as_tensor(weights).to(**f64).contiguous()
        opt = _lib.SpartRefineOpt(column=plan["column"], n_iter=plan["n_iter"], weights_per_obs=wper,
                                  fast_prelude=1 if lidf == "newton" else 0, nlayers=nl, rel_step=plan["rel_step"],
                                  lambda0=plan["lambda0"])
        if prior[0] is not None:
            pm, pw = (torch.as_tensor(v).to(**f64).contiguous() for v in prior[:2])
            opt.prior_per_obs, opt.prior_mean, opt.prior_weight = prior[2], pm.data_ptr(), pw.data_ptr()
        F = len(plan["names"])
        part, after = [], []
        if tiles is not None:
            Fs, srf, ts, sprior = tiles
            nbytes = int(self.lib.spart_tiles_workspace_bytes(self.ctx, M, F, Fs))
            opt = _lib.SpartRefineTilesOpt(fit=opt, n_shared=Fs, band_model=int(srf))
            if sprior[0] is not None:
                sm, sw = (torch.as_tensor(v).to(**f64).contiguous() for v in sprior[:2])
                opt.shared_prior_per_tile, opt.shared_prior_mean, opt.shared_prior_weight = sprior[2], sm.data_ptr(), sw.data_ptr()
            part = [ts.size - 1, ts.ctypes.data_as(_lib.c_i64p)]
            if series is not None:
                gamma, link = series
                ln = None if link is None else torch.as_tensor(link).to(**f64).contiguous()
                nbytes = int(self.lib.spart_series_workspace_bytes(self.ctx, M, F, Fs))
                opt = _lib.SpartRefineSeriesOpt(tiles=opt, smooth=_dp(gamma), link=None if ln is None else ln.data_ptr())
        elif mix is not None:
            V, Fs, srf, fit, act, flo, fhi, n, frd = mix
            nbytes = int(self.lib.spart_mix_workspace_bytes(self.ctx, M, V, F, n))
            opt = _lib.SpartRefineMixOpt(fit=opt, V=V, n_shared=Fs, band_model=int(srf), fit_fractions=int(fit),
                                         local_active=act.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), frac_lo=flo, frac_hi=fhi)
            after = [frd.data_ptr()]
        elif views is None:
            nbytes = int(self.lib.spart_refine_workspace_bytes(self.ctx, M, F))
        else:
            V, Fs, srf = views
            nbytes = int(self.lib.spart_views_workspace_bytes(self.ctx, M, V, F, Fs))
            opt = _lib.SpartRefineViewsOpt(fit=opt, V=V, n_shared=Fs, band_model=int(srf))
        nbytes = max(nbytes, 256)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.calls[entry] += 1
        rc = getattr(self.lib, entry)(self.ctx, M, self._ptrs(cols), F, plan["cols"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      _dp(plan["lo"]), _dp(plan["hi"]), *part, o.data_ptr() if o is not None else None,
                                      w.data_ptr() if w is not None else None, *after, ctypes.byref(opt), *outs, ws.data_ptr(), nbytes,
                                      self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return o, w

    def refine(self, params, obs, free, bounds=None, weights=None, column="R_TOC", n_iter=10, rel_step=1e-3, lambda0=1e-2,
               lidf="literal", nlayers=None, prior=None, prior_mean=None, prior_weight=None, band_model="centre", _plan=None,
               posterior=False):
        """Bounded Levenberg-Marquardt refinement of the ``free`` parameters of every start row against its observation, on the
        device (include/spart_hip.h: spart_refine, which defines every sum and solve; tools/refine_defined.py is the numpy form).
        params : the start rows, as for run(): a (27, M) float64 device tensor or a list of 27 scalars / arrays (each 1 or M values)
        obs : (M, nb) observed ``column`` (R_TOC / R_TOA / L_TOA) of this engine's sensor
        free : names from workloads.PARAM_NAMES (1 ... 16); the other parameters stay at their start values
        bounds : {name: (lo, hi)} for some or all free names; the default is workloads.RANGES[name]
        weights : None, (nb,) or (M, nb); a weight of exactly 0 skips the band (obs may be NaN there); 1 / sigma^2 makes
                  ``std`` the linearised 1-sigma uncertainty
        n_iter : proposals (0 ... 100): n_iter + 1 forward evaluations of (F + 1) M rows; there is no early exit
        lidf, nlayers : as for run()
        prior : {name: (mean, sigma)} for some free names, scalars or (M,) arrays: a Gaussian prior (optimal estimation); the cost
                gains sum_f (t_f - mean_f)^2 / sigma_f^2, and ``std`` becomes the linearised posterior 1-sigma
        prior_mean, prior_weight : the same prior ready-made, (F,) or (M, F) float64 (weight = 1 / sigma^2, exactly 0 = none;
                e.g. knn_prior's); tensors already on the device are used where they are.  Not together with ``prior``
        band_model : "centre" (default: the model sampled at the band centres, spart_refine) or "srf": ``obs`` and the fitted model
                are the SRF-convolved column (run()'s R_TOC_srf / R_TOA_srf / L_TOA_srf; spart_refine_srf) -- what a sensor measures
                and what generate_lut(band_model="srf") stores.  An iteration then evaluates the whole SRF support of every band
                (968 model bands per row for Sentinel-2A against 13).  ValueError for a sensor whose SRF columns are not in
                the order of its band centres (align_srf mends it)
        -> dict of device tensors x (M, F), cost, cost0 (M,), std (M, F), n_accept (M,) int32 (-1: the start could not be
        evaluated, x is then the clipped start) and y (M, nb), the model at x; and ``names``, the F names.
        posterior=True adds cov, corr, ak (M, F, F) and dfs (M,) of posterior() at the fitted rows (one more forward call); every
        other entry keeps its bits."""
        plan, params, M, kind, prior_mean, prior_weight, per_obs = refine_args(
            params, obs, free, bounds, weights, column, n_iter, rel_step, lambda0, lidf, prior, prior_mean, prior_weight, band_model,
            nb=self.nb, _plan=_plan)
        entry = "spart_refine_srf" if _band_model(band_model, self) else "spart_refine"
        nl = self._nlayers(nlayers)
        # ---- the device from here on
        cols = self._refine_columns(params, M)
        res = self._fit_outputs(M, len(plan["names"]), (M, self.nb))
        o, w = self._refine_device(entry, plan, M, cols, obs, weights, 1 if kind == "per_observation" else 0, lidf, nl,
                                   (prior_mean, prior_weight, per_obs), [res[k].data_ptr() for k in _FIT_OUTS])
        res["names"] = list(plan["names"])
        if posterior:
            # the fitted rows: the start rows with the free columns at x; std, y and cost of that call are the fit's bit for bit
            fitted = list(cols)
            for f, c in enumerate(plan["cols"]):
                fitted[int(c)] = res["x"][:, f].contiguous()
            post = self.posterior(fitted, o, free, weights=w, lidf=lidf, nlayers=nlayers, prior_mean=prior_mean,
                                  prior_weight=prior_weight, band_model=band_model, _plan=dict(plan, prior=None))
            res.update({k: post[k] for k in ("cov", "corr", "ak", "dfs")})
        return res

    def refine_leaf(self, leaf, refl=None, tran=None, free=("Cab", "Cw", "Cdm", "N"), bounds=None, weights_refl=None,
                    weights_tran=None, n_iter=20, rel_step=1e-3, lambda0=1e-2, prior=None, prior_mean=None, prior_weight=None,
                    spectra=False):
        """PROSPECT inversion: bounded Levenberg-Marquardt fits of the ``free`` leaf parameters of every start row against
        its measured leaf reflectance and / or transmittance on the 400 ... 2400 nm grid, on the device in ONE launch
        (include/spart_hip.h: spart_refine_leaf, which defines every sum and solve; tools/refine_leaf_defined.py is the numpy
        form).  No sensor is involved: any engine serves.
        leaf : the start rows, a (9, M) float64 tensor or a list of nine scalars / arrays (each 1 or M values), in LEAF_NAMES
               order (Cab, Cdm, Cw, Cs, Cca, Cant, N, PROT, CBC); the parameters not in ``free`` stay at these values
        refl, tran : (M, 2001) measured spectra; either may be None (reflectance-only fits are common), not both
        free : names from LEAF_NAMES (1 ... 9); bounds : {name: (lo, hi)}, the default is workloads.RANGES[name]
        weights_refl, weights_tran : None (weight 1), (2001,) or (M, 2001), only for spectra that are given; a weight of exactly
               0 skips the band (the measurement may be NaN there); 1 / sigma^2 makes ``std`` the linearised 1-sigma
        n_iter : proposals (0 ... 100), n_iter + 1 evaluations of F + 1 leaves each; there is no early exit
        prior, prior_mean, prior_weight : as for refine()
        -> dict of device tensors x (M, F), std (M, F), cost, cost0 (M,), n_accept (M,) int32 (-1: the start could not be
        evaluated, x is then the clipped start) and ``names``; with ``spectra`` also y_refl, y_tran (M, 2001), the model at x."""
        plan, leaf, M, wper, prior_mean, prior_weight, per_obs = refine_leaf_args(
            leaf, refl, tran, free, bounds, weights_refl, weights_tran, n_iter, rel_step, lambda0, prior, prior_mean, prior_weight)
        # ---- the device from here on
        torch = self.torch
        f64 = dict(dtype=torch.float64, device=self.device)
        F = len(plan["names"])
        if torch.is_tensor(leaf):
            L = leaf.to(**f64)
            cols = list(L.expand(_lib.LEAF_NPAR, M).contiguous()) if M else list(L)
        else:
            cols = self.columns(leaf, M)[0]

        def dense(v, rows):
            if v is None:
                return None
            v = torch.as_tensor(v).to(**f64)
            return (v.expand(M, _lib.NWL) if rows and v.dim() == 1 else v).contiguous()
        obs = [dense(refl, False), dense(tran, False)]
        wts = [dense(weights_refl, bool(wper)), dense(weights_tran, bool(wper))]
        opt = _lib.SpartLeafFitOpt(n_iter=plan["n_iter"], weights_per_obs=wper, rel_step=plan["rel_step"], lambda0=plan["lambda0"])
        if prior_mean is not None:
            pm, pw = (torch.as_tensor(v).to(**f64).contiguous() for v in (prior_mean, prior_weight))
            opt.prior_per_obs, opt.prior_mean, opt.prior_weight = per_obs, pm.data_ptr(), pw.data_ptr()
        shapes = {"x": (M, F), "cost": (M,), "cost0": (M,), "std": (M, F), "n_accept": (M,)}
        if spectra:
            shapes.update(y_refl=(M, _lib.NWL), y_tran=(M, _lib.NWL))
        res = {k: torch.empty(sh, dtype=torch.int32 if k == "n_accept" else torch.float64, device=self.device)
               for k, sh in shapes.items()}
        out = _lib.SpartLeafFitOut(**{k: res[k].data_ptr() if k in res else None for k in _lib.LEAF_FIT_OUTS})
        self.calls["spart_refine_leaf"] += 1
        ptr = [None if t is None else t.data_ptr() for t in obs + wts]
        rc = self.lib.spart_refine_leaf(self.ctx, M, self._ptrs(cols), F, plan["cols"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        _dp(plan["lo"]), _dp(plan["hi"]), *ptr, ctypes.byref(opt), ctypes.byref(out), self._stream())
        _lib.check(self.lib, self.ctx, rc)
        res["names"] = list(plan["names"])
        return res

    def posterior(self, params, obs, free, bounds=None, weights=None, column="R_TOC", rel_step=1e-3, lidf="literal", nlayers=None,
                  prior=None, prior_mean=None, prior_weight=None, band_model="centre", _plan=None, _outputs=None):
        """What refine()'s optimal-estimation fit knows about a point, on the device in one call (include/spart_hip.h:
        spart_refine_posterior, which defines every sum; tools/refine_posterior_defined.py is the numpy form): the Jacobian of the
        sensor column, the posterior covariance (J^T W J + S_a^-1)^-1, the averaging kernel and the degrees of freedom for signal.
        params, free, bounds, weights, column, rel_step, lidf, nlayers, prior / prior_mean / prior_weight, band_model : as for
        refine(); the point is ``params`` with its free columns clipped to the bounds.  With weights = 1 / sigma^2 of the
        measurement ``cov`` is the linearised posterior covariance
        obs : (M, nb), or None: no measurement -- ``cost`` is then the prior's term alone, everything else is unchanged
        -> dict of device tensors x (M, F), y (M, nb), jac (M, nb, F) (every band, weight-0 bands included), cov, ak (M, F, F),
        std (M, F), dfs, cost (M,), nband (M,) int32 (bands with a weight != 0), status (M,) int32 (0 ok; 1: A is not positive
        definite, cov / ak / std / dfs are NaN; -1: the point could not be evaluated or a weight is negative or not finite, jac
        is NaN too), corr (M, F, F) = cov_ab / (std_a std_b); and ``names``.  On the rows a fit returned, with the fit's
        arguments, std, y and cost are the fit's bit for bit (refine(posterior=True) does that)."""
        shape_of = obs if obs is not None else np.broadcast_to(np.float64(0.0), (params_rows(params), self.nb))
        plan, params, M, kind, prior_mean, prior_weight, per_obs = refine_args(
            params, shape_of, free, bounds, weights, column, 0, rel_step, 1e-2, lidf, prior, prior_mean, prior_weight, band_model,
            nb=self.nb, _plan=_plan)
        srf = _band_model(band_model, self)
        nl = self._nlayers(nlayers)
        nb, F = self.nb, len(plan["names"])
        # ---- the device from here on
        torch = self.torch
        cols = self._refine_columns(params, M)
        shapes = {"x": (M, F), "y": (M, nb), "jac": (M, nb, F), "cov": (M, F, F), "ak": (M, F, F), "std": (M, F), "dfs": (M,),
                  "cost": (M,), "nband": (M,), "status": (M,)}
        want = _lib.POSTERIOR_OUTS if _outputs is None else tuple(_outputs)
        res = {k: torch.empty(shapes[k], dtype=torch.int32 if k in ("nband", "status") else torch.float64, device=self.device)
               for k in _lib.POSTERIOR_OUTS if k in want}
        out = _lib.SpartPosteriorOut(**{k: v.data_ptr() for k, v in res.items()})
        self._refine_device("spart_refine_posterior", dict(plan, n_iter=0, lambda0=0.0), M, cols, obs, weights,
                            1 if kind == "per_observation" else 0, lidf, nl, (prior_mean, prior_weight, per_obs),
                            [1 if srf else 0, ctypes.byref(out)])
        if "cov" in res and "std" in res:
            res["corr"] = res["cov"] / (res["std"][:, :, None] * res["std"][:, None, :])
            d = res["corr"].diagonal(dim1=1, dim2=2)      # sqrt(v) * sqrt(v) need not be v: the diagonal is 1 by definition
            d.copy_(torch.where(torch.isnan(d), d, torch.ones_like(d)))
        res["names"] = list(plan["names"])
        return res

    def jacobian(self, params, free, bounds=None, column="R_TOC", rel_step=1e-3, lidf="literal", nlayers=None, band_model="centre"):
        """The thin form of posterior(): no observation, no weights, no prior.  -> dict of device tensors y (M, nb), the sensor
        column at ``params`` (free columns clipped to the bounds), and jac (M, nb, F), its one-sided finite-difference Jacobian
        with respect to the ``free`` parameters (step rel_step (hi - lo), forward unless that leaves the bounds); and ``names``.
        A row that cannot be evaluated has a NaN jac."""
        res = self.posterior(params, None, free, bounds=bounds, column=column, rel_step=rel_step, lidf=lidf, nlayers=nlayers,
                             band_model=band_model, _outputs=("y", "jac"))
        return {k: res[k] for k in ("y", "jac", "names")}

    def refine_views(self, params, obs, shared, local=(), bounds=None, weights=None, column="R_TOC", n_iter=10, rel_step=1e-3,
                     lambda0=1e-2, lidf="literal", nlayers=None, prior=None, prior_mean=None, prior_weight=None,
                     band_model="centre"):
        """refine() for V observations ("views") of the same pixels at once: per pixel ONE unknown vector -- the ``shared``
        parameters, one value for all views, and the ``local`` ones, one value per view -- is fitted against all V observations
        (include/spart_hip.h: spart_refine_views; tools/refine_views_defined.py is the numpy form).  Every view has its own fixed
        parameters (geometry, atmosphere, DOY ...).
        params : a (27, V, M) float64 device tensor, or 27 entries each broadcastable to (V, M) (scalar, (M,), (V, 1), (V, M)).
                 A shared parameter starts from view 0's value
        obs : (M, V, nb);  weights : None, (nb,) for every view, or (M, V, nb) (exactly 0 skips the band; a view of zeros is masked:
              its locals stay at their start, and without a prior on them the pixel's ``std`` is NaN)
        shared, local : names from workloads.PARAM_NAMES; n = len(shared) + V len(local) unknowns per pixel, 1 ... 16
        bounds : {name: (lo, hi)}, one pair per name; the default is workloads.RANGES[name]
        prior : {name: (mean, sigma)}: a shared name takes scalars or (M,) arrays, a local name scalars, (V,) or (M, V)
        prior_mean, prior_weight : the same ready-made per unknown, (n,) or (M, n); not together with ``prior``
        column, n_iter, rel_step, lambda0, lidf, nlayers, band_model : as for refine()
        -> dict of device tensors x, std (M, n) -- unknown a < Fs is shared[a], unknown Fs + v Fl + l is local[l] in view v --
        cost, cost0 (M,), n_accept (M,) int32 (-1: a dead pixel), y (M, V, nb); the slices shared / shared_std (M, Fs) and
        local / local_std (M, V, Fl) of x / std; and ``names`` = shared + local.
        A LUT search across views is another feature: retrieve / retrieve_stream do not call this."""
        plan, params, (M, V, Fs, n), wper, prior_mean, prior_weight, per_obs = refine_views_args(
            params, obs, shared, local, bounds, weights, column, n_iter, rel_step, lambda0, lidf, prior, prior_mean, prior_weight,
            band_model, nb=self.nb)
        srf = _band_model(band_model, self)
        nl = self._nlayers(nlayers)
        nb, F = self.nb, len(plan["names"])
        # ---- the device from here on
        torch = self.torch
        if torch.is_tensor(params):
            cols = list(params.to(dtype=torch.float64, device=self.device).contiguous())
        else:
            host = np.stack([np.broadcast_to(np.asarray(c.cpu() if torch.is_tensor(c) else c, dtype=np.float64), (V, M)) for c in params])
            cols = list(torch.as_tensor(host).to(self.device))
        res = self._fit_outputs(M, n, (M, V, nb))
        self._refine_device("spart_refine_views", plan, M, cols, obs, weights, wper, lidf, nl, (prior_mean, prior_weight, per_obs),
                            [res[k].data_ptr() for k in _FIT_OUTS], views=(V, Fs, srf))
        for k, src in (("shared", "x"), ("shared_std", "std")):
            res[k] = res[src][:, :Fs]
        for k, src in (("local", "x"), ("local_std", "std")):
            res[k] = res[src][:, Fs:].reshape(M, V, F - Fs)
        res["names"] = list(plan["names"])
        return res

    def refine_mix(self, params, obs, shared=(), local=(), active=None, fractions=None, fit_fractions=True, fraction_bounds=(0, 1),
                   bounds=None, weights=None, column="R_TOC", n_iter=10, rel_step=1e-3, lambda0=1e-2, lidf="literal", nlayers=None,
                   prior=None, band_model="centre"):
        """refine() with a LINEAR MIXTURE of V canopies per pixel: the observed column is sum_v a_v Y_v over V components, each
        with its own 27 parameters -- crop plus bare soil with the cover fraction as an unknown, a coarse pixel over several land
        covers (include/spart_hip.h: spart_refine_mix; tools/refine_mix_defined.py is the numpy form).  The chosen column itself is
        mixed: for R_TOA / L_TOA that neglects the coupling of neighbouring surfaces through the atmosphere.
        params : a (27, V, M) float64 device tensor, or 27 entries each broadcastable to (V, M).  A shared parameter starts from
                 component 0's value
        obs : (M, nb);  weights : None, (nb,) or (M, nb) (exactly 0 skips the band)
        shared, local : names from workloads.PARAM_NAMES: a shared name has one value for all components, a local name one per
                 component where it is active
        active : None (every local in every component), a dict {local name: components} or a (V, Fl) array of 0 / 1; an inactive
                 local of a component stays at that component's start value and is no unknown
        fractions : None (1 / V each), (V,) or (M, V): the given fractions (fit_fractions=False; no sum rule, a negative or
                 non-finite entry makes the pixel dead) or the start of the fitted ones (the last column is then not read)
        fit_fractions : the first V - 1 fractions are unknowns in ``fraction_bounds``, the last is 1 minus their sum; a trial whose
                 last fraction is negative is rejected
        bounds : {name: (lo, hi)}, one pair per name; the default is workloads.RANGES[name]
        prior : {name: (mean, sigma)}: a shared name takes scalars or (M,) arrays, a local name scalars, (V,) or (M, V); the key
                 "fractions" a scalar, (V - 1,) or (M, V - 1) per fitted fraction
        column, n_iter, rel_step, lambda0, lidf, nlayers, band_model : as for refine()
        -> dict of device tensors x, std (M, n) -- the shared names, the active locals (component by component), the fitted
        fractions --, cost, cost0 (M,), n_accept (M,) int32 (-1: a dead pixel), y (M, nb) the mixed column at x, y_comp (M, V, nb)
        the components' own columns, fractions (M, V) and fractions_std (M, V - 1; NaN when the fractions are given), shared /
        shared_std (M, Fs), local / local_std (M, V, Fl) where an inactive entry is the start value with std NaN; and ``names``
        = shared + local."""
        plan, params, (M, V, Fs, nm, n), act, fr, (flo, fhi), wper, prior_mean, prior_weight, per_obs = refine_mix_args(
            params, obs, shared, local, active, fractions, fit_fractions, fraction_bounds, bounds, weights, column, n_iter, rel_step,
            lambda0, lidf, prior, band_model, nb=self.nb)
        srf = _band_model(band_model, self)
        nl = self._nlayers(nlayers)
        nb, F = self.nb, len(plan["names"])
        Fl = F - Fs
        # ---- the device from here on
        torch = self.torch
        f64 = dict(dtype=torch.float64, device=self.device)
        if torch.is_tensor(params):
            P = params.to(**f64).contiguous()
        else:
            host = np.stack([np.broadcast_to(np.asarray(c.cpu() if torch.is_tensor(c) else c, dtype=np.float64), (V, M)) for c in params])
            P = torch.as_tensor(host).to(self.device)
        cols = list(P)
        shapes = {"x": (M, n), "cost": (M,), "cost0": (M,), "std": (M, n), "n_accept": (M,), "y": (M, nb), "frac": (M, V),
                  "y_comp": (M, V, nb)}
        res = {k: torch.empty(shapes[k], dtype=torch.int32 if k == "n_accept" else torch.float64, device=self.device)
               for k in _lib.MIX_OUTS}
        out = _lib.SpartRefineMixOut(**{k: v.data_ptr() for k, v in res.items()})
        frd = torch.as_tensor(fr).to(**f64).contiguous()
        self._refine_device("spart_refine_mix", plan, M, cols, obs, weights, wper, lidf, nl, (prior_mean, prior_weight, per_obs),
                            [ctypes.byref(out)], mix=(V, Fs, srf, bool(fit_fractions), act, flo, fhi, n, frd))
        res["fractions"] = res.pop("frac")
        res["fractions_std"] = res["std"][:, nm:] if n > nm else torch.full((M, V - 1), float("nan"), **f64)
        res["shared"], res["shared_std"] = res["x"][:, :Fs], res["std"][:, :Fs]
        unknown = mix_maps(V, Fs, Fl, act, False)[0]
        loc = P[plan["cols"][Fs:].tolist()].permute(2, 1, 0).clone() if Fl else torch.empty((M, V, 0), **f64)
        loc_std = torch.full((M, V, Fl), float("nan"), **f64)
        for v in range(V):
            for l in range(Fl):
                if unknown[v, l] >= 0:
                    loc[:, v, l] = res["x"][:, unknown[v, l]]
                    loc_std[:, v, l] = res["std"][:, unknown[v, l]]
        res["local"], res["local_std"] = loc, loc_std
        res["names"] = list(plan["names"])
        return res

    def refine_tiles(self, params, obs, shared, local=(), tile_size=None, tile_start=None, bounds=None, weights=None,
                     column="R_TOC", n_iter=10, rel_step=1e-3, lambda0=1e-2, lidf="literal", nlayers=None, prior=None,
                     band_model="centre"):
        """refine() with parameters shared by a TILE of pixels: the ``shared`` names are ONE unknown per tile -- one atmosphere
        per window, one leaf-angle parameter per field -- and the ``local`` names one unknown per pixel; one Levenberg-Marquardt
        decision is taken per tile on the summed cost (include/spart_hip.h: spart_refine_tiles; tools/refine_tiles_defined.py
        is the numpy form).
        params, obs, weights, bounds, column, n_iter, rel_step, lambda0, lidf, nlayers, band_model : as for refine(); a shared
                 parameter starts from its tile's first pixel
        tile_size : G: uniform runs of G pixels, the last one shorter;  or  tile_start : (T + 1,) integers, tile t being the
                 pixels tile_start[t] ... tile_start[t + 1] - 1 (tiles_from_labels / window_tiles make them); 1 ... 4096 pixels
        prior : {name: (mean, sigma)}: a shared name takes scalars or (T,) arrays, a local name scalars or (M,) arrays
        -> dict of device tensors shared, shared_std (T, Fs), local, local_std (M, Fl), cost, cost0 (T,), n_accept (T,) int32
        (-1: a dead tile), pixel_cost (M,), status (M,) int32 (0 live, -1 a dead pixel, which takes no part in its tile, 1 a live
        pixel of a dead tile), y (M, nb); and ``names`` = shared + local, ``tile_start`` (numpy int64).
        retrieve / retrieve_stream do not call this."""
        plan, params, M, Fs, wper, ts, lprior, sprior = refine_tiles_args(
            params, obs, shared, local, tile_size, tile_start, bounds, weights, column, n_iter, rel_step, lambda0, lidf, prior,
            band_model, nb=self.nb)
        srf = _band_model(band_model, self)
        nl = self._nlayers(nlayers)
        T, Fl = ts.size - 1, len(plan["names"]) - Fs
        # ---- the device from here on
        torch = self.torch
        cols = self._refine_columns(params, M)
        shapes = {"shared": (T, Fs), "shared_std": (T, Fs), "local": (M, Fl), "local_std": (M, Fl), "cost": (T,), "cost0": (T,),
                  "n_accept": (T,), "pixel_cost": (M,), "status": (M,), "y": (M, self.nb)}
        res = {k: torch.empty(shapes[k], dtype=torch.int32 if k in ("n_accept", "status") else torch.float64, device=self.device)
               for k in _lib.TILES_OUTS}
        out = _lib.SpartTilesOut(**{k: v.data_ptr() for k, v in res.items()})
        self._refine_device("spart_refine_tiles", plan, M, cols, obs, weights, wper, lidf, nl, lprior, [ctypes.byref(out)],
                            tiles=(Fs, srf, ts, sprior))
        res["names"], res["tile_start"] = list(plan["names"]), ts
        return res

    def refine_series(self, params, obs, shared=(), local=(), n_dates=None, series_start=None, smooth=None, link=None, bounds=None,
                      weights=None, column="R_TOC", n_iter=10, rel_step=1e-3, lambda0=1e-2, lidf="literal", nlayers=None, prior=None,
                      band_model="centre"):
        """refine_tiles() with the tile read as a TIME SERIES of one pixel and a smoothness prior between consecutive dates: a
        row is one date with its own geometry, atmosphere, observation and weights; the ``shared`` names are ONE unknown per
        series (leaf angle, soil brightness), the ``local`` names (at least one) one unknown per date, tied to the next date by
        a first-difference penalty (include/spart_hip.h: spart_refine_series; tools/refine_series_defined.py is the numpy form).
        A date whose weights are all zero is a masked (cloudy) date: its locals are filled by its neighbours.
        n_dates : T: uniform series of T rows (M a multiple of T);  or  series_start : (S + 1,) integers; 1 ... 256 rows each
        smooth : {local name: sigma}: the tie of that parameter between consecutive dates has weight 1 / sigma^2 (times link);
                 a local that is not named is not tied
        link   : None, or (M,) values >= 0: link[m] scales the tie between rows m and m + 1 (date_links makes 1 / dt); the
                 entry of a series' last row is not read
        everything else as for refine_tiles(); prior: a shared name takes scalars or (S,) arrays, a local name scalars or (M,)
        -> refine_tiles()'s dict with ``series_start`` in place of ``tile_start``: cost, cost0, n_accept per series (-1: a dead
        series -- a bad row kills its whole series: status -1 on the bad rows, 1 on the others).
        retrieve / retrieve_stream do not call this."""
        plan, params, M, Fs, wper, ts, lprior, sprior, gamma = refine_series_args(
            params, obs, shared, local, n_dates, series_start, smooth, link, bounds, weights, column, n_iter, rel_step, lambda0, lidf,
            prior, band_model, nb=self.nb)
        srf = _band_model(band_model, self)
        nl = self._nlayers(nlayers)
        T, Fl = ts.size - 1, len(plan["names"]) - Fs
        # ---- the device from here on
        torch = self.torch
        cols = self._refine_columns(params, M)
        shapes = {"shared": (T, Fs), "shared_std": (T, Fs), "local": (M, Fl), "local_std": (M, Fl), "cost": (T,), "cost0": (T,),
                  "n_accept": (T,), "pixel_cost": (M,), "status": (M,), "y": (M, self.nb)}
        res = {k: torch.empty(shapes[k], dtype=torch.int32 if k in ("n_accept", "status") else torch.float64, device=self.device)
               for k in _lib.TILES_OUTS}
        out = _lib.SpartTilesOut(**{k: v.data_ptr() for k, v in res.items()})
        self._refine_device("spart_refine_series", plan, M, cols, obs, weights, wper, lidf, nl, lprior, [ctypes.byref(out)],
                            tiles=(Fs, srf, ts, sprior), series=(gamma, link))
        res["names"], res["series_start"] = list(plan["names"]), ts
        return res

    def sobol(self, params, free, N=4096, bounds=None, design=None, seed=0, column="R_TOC", band_model="centre", lidf="literal",
              nlayers=None):
        """GLOBAL sensitivity of a sensor column to the ``free`` parameters over their ranges, on the device in one call
        (include/spart_hip.h: spart_sobol, which defines every sum; tools/sobol_defined.py is the numpy form): Sobol' first-order
        and total indices of every band with jackknife standard errors -- what tells which parameters a retrieval can free.
        params : the SITES: a (27, M) block or 27 entries of 1 or M values; a site fixes geometry, atmosphere and every
                 parameter that is not free
        free, bounds : as for refine(): names, and {name: (lo, hi)} with workloads.RANGES as the default
        N : base samples, a multiple of 64 in 128 ... 2^20: N (F + 2) forward rows per site
        design : None (sobol_design(N, F, seed)) or (uA, uB), two (N, F) arrays in the unit cube, used as given
        column, band_model, lidf, nlayers : as for refine()
        -> dict of device tensors mean, var (M, nb) (over the 2 N rows of A and B), S1, ST, S1_se, ST_se (M, nb, F); and ``names``.
        A band that does not vary has var 0 and NaN indices; nothing is clamped."""
        plan, params, M, N, uA, uB = sobol_args(params, free, N, bounds, design, seed, column, band_model, lidf)
        srf = _band_model(band_model, self)
        nl = self._nlayers(nlayers)
        F, nb = len(plan["names"]), self.nb
        # ---- the device from here on
        torch = self.torch
        f64 = dict(dtype=torch.float64, device=self.device)
        cols = self._refine_columns(params, M)
        uA, uB = (torch.as_tensor(u).to(**f64).contiguous() for u in (uA, uB))
        res = {k: torch.empty((M, nb) if k in ("mean", "var") else (M, nb, F), **f64) for k in _lib.SOBOL_OUTS}
        out = _lib.SpartSobolOut(**{k: v.data_ptr() for k, v in res.items()})
        opt = _lib.SpartSobolOpt(column=plan["column"], band_model=int(srf), fast_prelude=1 if lidf == "newton" else 0, nlayers=nl)
        nbytes = max(int(self.lib.spart_sobol_workspace_bytes(self.ctx, M, N, F)), 256)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.calls["spart_sobol"] += 1
        rc = self.lib.spart_sobol(self.ctx, M, self._ptrs(cols), F, plan["cols"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                  _dp(plan["lo"]), _dp(plan["hi"]), N, uA.data_ptr(), uB.data_ptr(), ctypes.byref(opt),
                                  ctypes.byref(out), ws.data_ptr(), nbytes, self._stream())
        _lib.check(self.lib, self.ctx, rc)
        res["names"] = list(plan["names"])
        return res

    def vjp(self, params, grad_outputs, free, bounds=None, rel_step=1e-3, lidf="literal", nlayers=None, band_model="centre"):
        """The vector-Jacobian product of the sensor columns with respect to the ``free`` parameters, on the device in one call
        (include/spart_hip.h: spart_vjp, which defines every sum; tools/vjp_defined.py is the numpy form): what a backward pass
        needs, by bounded central differences, with no Jacobian stored.
        params, free, bounds, lidf, nlayers, band_model : as for refine(); the point is ``params`` with its free columns clipped
                 to the bounds
        grad_outputs : {column name: (M, nb) tensor or array}, dLoss / d column for R_TOC / R_TOA / L_TOA; a column that is
                 missing or None takes no part; band_model "srf" takes one column
        rel_step : the step is rel_step (hi - lo) to either side, cut at the bounds; in (0, 0.5]
        -> {"grad": (M, F) float64 device tensor, dLoss / d free parameter, "names": [...]}.  A NaN parameter or gradient makes
        that row's grad NaN and no other."""
        plan, params, M, gys = vjp_args(params, grad_outputs, free, bounds, rel_step, lidf, band_model, nb=self.nb or None)
        srf = _band_model(band_model, self)
        nl = self._nlayers(nlayers)
        F = len(plan["names"])
        # ---- the device from here on
        torch = self.torch
        f64 = dict(dtype=torch.float64, device=self.device)
        cols = self._refine_columns(params, M)
        gys = [None if g is None else torch.as_tensor(g).to(**f64).contiguous() for g in gys]
        grad = torch.empty((M, F), **f64)
        opt = _lib.SpartVjpOpt(band_model=int(srf), fast_prelude=1 if lidf == "newton" else 0, nlayers=nl, rel_step=plan["rel_step"])
        nbytes = max(int(self.lib.spart_vjp_workspace_bytes(self.ctx, M, F)), 256)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.calls["spart_vjp"] += 1
        rc = self.lib.spart_vjp(self.ctx, M, self._ptrs(cols), F, plan["cols"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                _dp(plan["lo"]), _dp(plan["hi"]), self._ptrs(gys), ctypes.byref(opt), grad.data_ptr(), ws.data_ptr(),
                                nbytes, self._stream())
        _lib.check(self.lib, self.ctx, rc)
        return {"grad": grad, "names": list(plan["names"])}

    def sample(self, params, obs, free, bounds=None, weights=None, prior=None, walkers=None, n_steps=1000, burn=None, thin=1, seed=0,
               init=None, init_radius=None, step0=0, obs_offset=0, column="R_TOC", band_model="centre", chain=False, a=2.0,
               temperature=1.0, rel_init=0.01, prior_mean=None, prior_weight=None, lidf="literal", nlayers=None):
        """The SHAPE of the posterior around a fit, sampled with the forward model itself, on the device in one call
        (include/spart_hip.h: spart_sample, which defines every operation; tools/sample_defined.py is the numpy form): the
        affine-invariant ensemble sampler (Goodman & Weare; emcee's stretch move) with ``walkers`` walkers per observation inside
        the bounds.  The density is exp(-cost / (2 temperature)), cost being refine()'s: with weights = 1 / sigma^2 and
        temperature 1 it is the posterior of the retrieval.
        params, obs, free, bounds, weights, prior / prior_mean / prior_weight, column, band_model, lidf, nlayers : as for
                 refine(); the walkers start in a box of +- rel_init (hi - lo) (or +- init_radius (M, F)) around ``params``
                 clipped to the bounds, so ``params`` is best the fitted point
        walkers : 8, 16, 32 or 64 and >= 2 F; None: the smallest such
        n_steps, burn, thin : steps, of which the first ``burn`` (None: n_steps // 2) are dropped and then every thin-th kept
        seed, obs_offset, step0 : the random numbers are a pure function of (seed, obs_offset + row, step0 + step, walker): rows
                 [a, b) sampled with obs_offset = a give the rows of the whole call
        init : (M, W, F), a given ensemble (with step0 = the steps already taken, the ``last`` of an earlier call resumes it)
        chain : True adds chain (M, n_keep, W, F) and chain_cost (M, n_keep, W); chain_summary() reads them
        -> dict of device tensors mean, std (M, F), cov (M, F, F) over the kept states, best (M, F), best_cost (M,) the lowest cost
        seen, accept_fraction (M,), status (M,) int32 (0; -1: a dead observation, everything of it is NaN), last (M, W, F),
        last_cost (M, W); and ``names``."""
        plan, params, M, kind, prior_mean, prior_weight, per_obs, so = sample_args(
            params, obs, free, bounds, weights, prior, prior_mean, prior_weight, walkers, n_steps, burn, thin, a, temperature,
            rel_init, init, init_radius, step0, obs_offset, seed, column, band_model, lidf, nb=self.nb)
        srf = _band_model(band_model, self)
        nl = self._nlayers(nlayers)
        F, W, nk = len(plan["names"]), so["W"], so["n_keep"]
        # ---- the device from here on
        torch = self.torch
        f64 = dict(dtype=torch.float64, device=self.device)
        cols = self._refine_columns(params, M)
        dev = lambda v: None if v is None else torch.as_tensor(v).to(**f64).contiguous()     # noqa: E731
        o, w, pm, pw, x_init, radius = (dev(v) for v in (obs, weights, prior_mean, prior_weight, init, init_radius))
        shapes = {"mean": (M, F), "cov": (M, F, F), "std": (M, F), "best_x": (M, F), "best_cost": (M,), "n_accept": (M,),
                  "status": (M,), "chain": (M, nk, W, F), "chain_cost": (M, nk, W), "last": (M, W, F), "last_cost": (M, W)}
        kinds = {"n_accept": torch.int64, "status": torch.int32}
        raw = {k: torch.empty(shapes[k], dtype=kinds.get(k, torch.float64), device=self.device) for k in _lib.SAMPLE_OUTS
               if chain or k not in ("chain", "chain_cost")}
        out = _lib.SpartSampleOut(**{k: v.data_ptr() for k, v in raw.items()})
        ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
        opt = _lib.SpartSampleOpt(column=plan["column"], band_model=int(srf), fast_prelude=1 if lidf == "newton" else 0, nlayers=nl,
                                  weights_per_obs=1 if kind == "per_observation" else 0, prior_per_obs=per_obs, prior_mean=ptr(pm),
                                  prior_weight=ptr(pw), W=W, n_steps=so["n_steps"], burn=so["burn"], thin=so["thin"], a=so["a"],
                                  temperature=so["temperature"], rel_init=so["rel_init"], init_radius=ptr(radius), init=ptr(x_init),
                                  step0=so["step0"], obs_offset=so["obs_offset"], seed=so["seed"])
        nbytes = max(int(self.lib.spart_sample_workspace_bytes(self.ctx, M, F, W)), 256)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.calls["spart_sample"] += 1
        rc = self.lib.spart_sample(self.ctx, M, self._ptrs(cols), F, plan["cols"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   _dp(plan["lo"]), _dp(plan["hi"]), ptr(o), ptr(w), ctypes.byref(opt), ctypes.byref(out),
                                   ws.data_ptr(), nbytes, self._stream())
        _lib.check(self.lib, self.ctx, rc)
        res = {k: raw[k] for k in ("mean", "std", "cov", "best_cost", "status", "last", "last_cost")}
        res["best"] = raw["best_x"]
        na = raw["n_accept"]
        res["accept_fraction"] = torch.where(na < 0, torch.full_like(res["best_cost"], float("nan")),
                                             na.to(torch.float64) / float(W * so["n_steps"]))
        if chain:
            res["chain"], res["chain_cost"] = raw["chain"], raw["chain_cost"]
        res["names"] = list(plan["names"])
        return res

    def profile(self, max_calls):
        """bracket the band kernel of the next ``max_calls`` run() calls with HIP events (0 = off)."""
        _lib.check(self.lib, self.ctx, self.lib.spart_profile_enable(self.ctx, int(max_calls)))

    def profile_read(self):
        """-> (summed band-kernel milliseconds, number of timed calls)"""
        ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
        _lib.check(self.lib, self.ctx, self.lib.spart_profile_read(self.ctx, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def profile_read_stages(self):
        """-> ({'prelude': ms, 'bands': ms, 'columns': ms} summed over the timed calls, number of calls)"""
        ms, n = (ctypes.c_double * 8)(), ctypes.c_int(0)      # (room for builds of earlier rounds that report four stages)
        _lib.check(self.lib, self.ctx, self.lib.spart_profile_read_stages(self.ctx, ms, ctypes.byref(n)))
        return dict(zip(_lib.STAGES, [float(x) for x in ms])), n.value

    def econv(self):
        out = np.zeros(self.nb)
        _lib.check(self.lib, self.ctx, self.lib.spart_ctx_econv(self.ctx, _dp(out)))
        return out


_cache_lock = threading.RLock()   # guards the three caches below (contexts are thread-safe; so is finding one)
_engines = {}            # (sensor name, device) -> Engine built from the packaged tables: no hashing on this path
_by_content = {}         # (table digest, sensor digest | None, device) -> Engine, least recently used last out
_packaged_digest = {}    # memo: digests of the packaged tables ("optical") and sensors (name)
MAX_CONTENT_ENGINES = 16  # a context is ~0.6 MB of device tables; a handful of table sets at most is expected


def get_engine(sensor=None, device=None, optical_params=None, et_params=None, sensor_info=None, need=OPTICAL_KEYS):
    """The engine (device context) for a sensor and a set of tables.

    get_engine(sensor, device): the packaged tables and the packaged sensor ``sensor`` (or no sensor), one engine per
    (name, device), found without looking at any table.
    With ``optical_params`` / ``et_params`` / ``sensor_info`` (the reference's dicts: SPART.optipar, SPART.ETpar,
    SPART.sensorinfo; PROSPECT_5D's and BSM's second argument): the engine whose device tables have exactly THAT content
    -- the key is a digest of the arrays, re-computed on every call (~20 us with xxhash, 0.2 ms with sha1), so editing
    a dict or one of its arrays in place between two calls gives the second call the edited tables, as in the
    reference, and handing in the unmodified packaged dicts gives the very engine of the name-keyed path.
    ``need``: the keys of optical_params the calling entry point reads (see optical_block)."""
    torch = _require_gpu()
    if device is None:
        device = torch.cuda.current_device()
    device = int(device)
    with _cache_lock:
        return _get_engine_locked(sensor, device, optical_params, et_params, sensor_info, need)


def _get_engine_locked(sensor, device, optical_params, et_params, sensor_info, need):
    if optical_params is None and et_params is None and sensor_info is None:
        key = (sensor, device)
        if key not in _engines:
            _engines[key] = Engine(sensor, device)
        return _engines[key]
    if "optical" not in _packaged_digest:
        _packaged_digest["optical"] = _digest(optical_block().values())
    ob = optical_block(optical_params, et_params, need)
    dt = _digest(ob.values())
    ds = None
    if sensor_info is not None:
        ds = _digest(sensor_block(sensor_info).values())
    elif sensor is not None:
        ds = _packaged_digest.get(sensor)
        if ds is None:
            ds = _packaged_digest[sensor] = _digest(sensor_block(tables.load_sensor_info(sensor)).values())
    # the packaged content under whatever dict it arrives in IS the name-keyed engine
    if dt == _packaged_digest["optical"]:
        if ds is None:
            return get_engine(None, device)
        for name in ([sensor] if isinstance(sensor, str) else []) + list(tables.SENSORS):
            if name not in _packaged_digest:
                try:
                    _packaged_digest[name] = _digest(sensor_block(tables.load_sensor_info(name)).values())
                except FileNotFoundError:
                    continue
            if _packaged_digest[name] == ds:
                return get_engine(name, device)
    key = (dt, ds, device)
    eng = _by_content.pop(key, None)
    if eng is None:
        while len(_by_content) >= MAX_CONTENT_ENGINES:
            _by_content.pop(next(iter(_by_content)))
        eng = Engine(sensor if sensor_info is None else None, device, sensor_info=sensor_info, optical_params=optical_params,
                     et_params=et_params, need=need)
    _by_content[key] = eng                    # (re-inserted at the end: most recently used)
    return eng
