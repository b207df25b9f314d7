"""What the GPU tests of spart_refine_posterior share beside helpers/refine_calls.py: the raw C-ABI caller (every output in a
buffer of its own with guard elements behind it), the case builder with its planted rows, the definition configured like the
call, and what retrieve(refine_opts={"posterior": True}) is DEFINED to add, composed of helpers/retrieve_defined.py and
tools/refine_posterior_defined.py."""
import ctypes
import os
import sys

import numpy as np

from helpers.refine_calls import COLUMNS, FILL, GUARD, forward_of, make_case, same
from helpers.refine_srf_calls import srf_forward_of
from helpers.lut_calls import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_posterior_defined as rpd  # noqa: E402

OUTS = rpd.OUTS
INT_OUTS = ("nband", "status")
TAIL = GUARD // 8           # guard elements behind every output


def out_shapes(M, F, nb):
    return {"x": (M, F), "y": (M, nb), "jac": (M, nb, F), "cov": (M, F, F), "ak": (M, F, F), "std": (M, F), "dfs": (M,), "cost": (M,),
            "nband": (M,), "status": (M,)}


def posterior_call(torch, eng, base, free, lo, hi, obs, w=None, mean=None, weight=None, column=0, band_model=0, outputs=OUTS,
                   rel_step=0.0, n_iter=0, lambda0=0.0, nlayers=0, fast_prelude=0, per_obs=None, weights_per_obs=None, null=(),
                   ws_bytes=None, M=None, F=None, ctx="own", nb=None):
    """One spart_refine_posterior through ctypes -> (rc, dict of numpy outputs).  Every output in ``outputs`` gets a buffer of
    its own, pre-filled with FILL, with TAIL more elements behind it that must still hold FILL afterwards; the others are NULL.
    The workspace has GUARD bytes of 0xFF behind it that must survive.  ``null``: names of base / free / lo / hi / opt / out / ws
    to pass as NULL; ``M`` / ``F`` / ``ws_bytes``: sizes to pass in place of the arrays' own; ``obs`` may be None (NULL)."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, f = base.shape[0], len(free)
    nb = eng.nb if nb is None else nb
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt, ot, wt, mt, pt = up(base.T), up(obs), up(w), up(mean), up(weight)
    bufs = {}
    for k, shape in out_shapes(m, f, nb).items():
        if k in outputs:
            dt = torch.int32 if k in INT_OUTS else torch.float64
            bufs[k] = torch.full((int(np.prod(shape)) + TAIL,), int(FILL) if k in INT_OUTS else FILL, dtype=dt, device=dev)
    out = _lib.SpartPosteriorOut(**{k: v.data_ptr() for k, v in bufs.items()})
    if per_obs is None:
        per_obs = int(any(a is not None and np.ndim(a) == 2 for a in (mean, weight)))
    if weights_per_obs is None:
        weights_per_obs = 1 if (w is not None and np.ndim(w) == 2) else 0
    opt = _lib.SpartRefineOpt(column=column, n_iter=n_iter, weights_per_obs=weights_per_obs, fast_prelude=fast_prelude, nlayers=nlayers,
                              rel_step=rel_step, lambda0=lambda0, prior_per_obs=per_obs,
                              prior_mean=None if mt is None else mt.data_ptr(), prior_weight=None if pt is None else pt.data_ptr())
    need = int(eng.lib.spart_refine_workspace_bytes(eng.ctx, m, f))
    n = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(need, 256) + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    ptr = lambda name, v: None if name in null else v     # noqa: E731
    rc = eng.lib.spart_refine_posterior(
        eng.ctx if ctx == "own" else ctx, m if M is None else M, ptr("base", (_lib.vp * 27)(*[Bt[i].data_ptr() for i in range(27)])),
        f if F is None else F, ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), ptr("lo", lo.ctypes.data_as(_lib.c_dp)),
        ptr("hi", hi.ctypes.data_as(_lib.c_dp)), None if ot is None else ot.data_ptr(), None if wt is None else wt.data_ptr(),
        ptr("opt", ctypes.byref(opt)), band_model, ptr("out", ctypes.byref(out)), ptr("ws", ws.data_ptr()), ctypes.c_size_t(n),
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert bool((ws[max(need, 256):] == 0xFF).all()), "bytes behind the workspace were written"
    got = {}
    for k, shape in out_shapes(m, f, nb).items():
        if k in bufs:
            a = bufs[k].cpu().numpy()
            assert (a[int(np.prod(shape)):] == (int(FILL) if k in INT_OUTS else FILL)).all(), f"elements behind {k} were written"
            got[k] = a[:int(np.prod(shape))].reshape(shape)
    return rc, got


def untouched(got):
    return all((v == (int(FILL) if k in INT_OUTS else FILL)).all() for k, v in got.items())


def make_posterior_case(torch, eng, names, M, column, kind, prior, seed, srf=False, constant=False):
    """refine_calls.make_case (its planted rows: 0 a start outside the bounds, 1 a start on hi, 3 an unmasked NaN observation
    (dead), 4 a NaN fixed parameter (dead), and with per-observation weights 2 an all-zero weight row, 5 a negative band weight
    (dead), 6 a NaN observation under a zero weight (alive)) with a prior: "none", "shared" ((F,), sigma = 10 % of the range on
    every name) or "per_observation" ((M, F), about 20 % zero weights over NaN means).  Planted on top, M >= 63:
      7  (per-observation prior) a negative prior weight: dead
      8  (per-observation weights) all band weights zero; with a prior, its full weight on every name: a row whose only
         information is the prior (K = 0: ak and dfs exactly 0); without a prior A = 0: status 1
      2  (per-observation weights and prior) all band weights zero AND all prior weights zero: A = 0, status 1
      9  (``constant``; needs a per-observation prior and a column other than L_TOA) the LAST free column is replaced by DOY,
         bounds (1, 365), which enters L_TOA alone: a constant free column.  Every row has a prior on it but row 9: status 1
    -> (base, free, lo, hi, obs, w, mean, weight)"""
    from spart_amd import workloads
    base, free, lo, hi, obs, w = make_case(torch, eng, names, M, column, kind, seed)
    if srf:
        with np.errstate(all="ignore"):
            truth = workloads.lhs_params(M, "full", seed=seed)
            clean = srf_forward_of(torch, eng, column)(truth)
        rng0 = np.random.default_rng(seed + 7)
        fresh = np.where(np.isfinite(clean), clean, 0.3) * (1.0 + 0.01 * rng0.normal(size=clean.shape))
        obs = np.where(np.isnan(obs), np.nan, fresh)                  # (the planted NaN stay where they are)
    rng = np.random.default_rng(seed + 99)
    F = len(free)
    if constant:
        assert prior == "per_observation" and column != "L_TOA" and M >= 63
        free, lo, hi = list(free[:-1]) + [workloads.PARAM_NAMES.index("DOY")], lo.copy(), hi.copy()
        lo[-1], hi[-1] = 1.0, 365.0
    mean = weight = None
    if prior != "none":
        truth = workloads.lhs_params(M, "full", seed=seed)[:, free]
        shape = (M, F) if prior == "per_observation" else (F,)
        mean = (truth if prior == "per_observation" else truth[0]) + 0.1 * rng.normal(size=shape) * (hi - lo)
        weight = np.array(np.broadcast_to(1.0 / (0.1 * (hi - lo)) ** 2, shape))
        if prior == "per_observation":
            zero = rng.random(shape) < 0.2
            mean, weight = np.where(zero, np.nan, mean), np.where(zero, 0.0, weight)
    if M >= 63:
        full = 1.0 / (0.1 * (hi - lo)) ** 2
        if prior == "per_observation":
            if constant:
                weight[:, F - 1], mean[:, F - 1] = full[F - 1], 100.0
                weight[9], mean[9] = full, 0.5 * (lo + hi)
                weight[9, F - 1] = 0.0
            weight[7, F - 1], mean[7, F - 1] = -1.0, 0.5 * (lo[F - 1] + hi[F - 1])
        if kind == "per_observation":
            w[8] = 0.0
            if prior == "per_observation":
                weight[8], mean[8] = full, 0.5 * (lo + hi)
                weight[2], mean[2] = 0.0, np.nan
    return base, free, lo, hi, obs, w, mean, weight


def defined(torch, eng, case, column, srf=False, with_obs=True, **kw):
    """the definition configured like posterior_call(case, column, band_model=srf)"""
    base, free, lo, hi, obs, w, mean, weight = case
    fwd = (srf_forward_of if srf else forward_of)(torch, eng, COLUMNS[column])
    return rpd.posterior_defined(base, free, lo, hi, obs if with_obs else None, fwd, weights=w, prior_mean=mean, prior_weight=weight, **kw)


def call(torch, eng, case, column, srf=False, with_obs=True, **kw):
    base, free, lo, hi, obs, w, mean, weight = case
    rc, got = posterior_call(torch, eng, base, free, lo, hi, obs if with_obs else None, w, mean, weight, column=column,
                             band_model=1 if srf else 0, **kw)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    return got


def mismatches(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return "shape" if a.shape != b.shape else int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def assert_same(got, ref, what, keys=OUTS):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and same(got[k], ref[k]), (what, k, mismatches(got[k], ref[k]))


# ---- retrieve(refine_opts={"posterior": True})
POSTERIOR = ("refined_cov", "refined_ak", "refined_dfs")


def retrieve_posterior_defined(params, table, obs, k, weights, names, lo, hi, forward, **fit):
    """helpers.retrieve_defined.retrieve_defined, then the definition of spart_refine_posterior on the fitted rows of the matched
    observations with the fit's own weights and prior -> its dict plus refined_cov, refined_ak (M, F, F) and refined_dfs (M,)
    (NaN without a row); the definition's std, cost at those rows must be the fit's."""
    from helpers.retrieve_defined import prior_plan_of, retrieve_defined
    from spart_amd.engine import knn_prior, prior_arrays
    from spart_amd.workloads import PARAM_NAMES
    import lut_brute_force as bf
    out = retrieve_defined(params, table, obs, k, weights, names, lo, hi, forward, **fit)
    M, F = np.shape(obs)[0], len(names)
    free = [PARAM_NAMES.index(n) for n in names]
    out.update(refined_cov=np.full((M, F, F), np.nan), refined_ak=np.full((M, F, F), np.nan), refined_dfs=np.full(M, np.nan))
    ok = np.flatnonzero(out["idx"][:, 0] >= 0)
    if ok.size == 0:
        return out
    rows = np.ascontiguousarray(params, dtype=np.float64)[out["idx"][ok, 0]]
    rows[:, free] = out["refined"][ok]
    w64 = None if weights is None else np.asarray(weights, dtype=np.float64)
    if w64 is not None and w64.ndim == 2:
        w64 = w64[ok]
    prior, pm, pw = fit.get("prior"), None, None
    if isinstance(prior, str):
        near = bf.summarise_defined(np.ascontiguousarray(params, dtype=np.float64)[:, free], out["idx"][ok])
        pm, pw = knn_prior(near[0], near[2], np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64),
                           floor=fit.get("prior_floor", 0.05))
    elif prior is not None:
        pm, pw = (a[ok] if a.ndim == 2 else a for a in prior_arrays(prior_plan_of(list(names), prior), M))
    post = rpd.posterior_defined(rows, free, lo, hi, np.asarray(obs, dtype=np.float64)[ok], forward, weights=w64,
                                 rel_step=fit.get("rel_step", 1e-3), prior_mean=pm, prior_weight=pw)
    assert same(post["std"], out["refined_std"][ok]) and same(post["cost"], out["refined_cost"][ok])
    out["refined_cov"][ok], out["refined_ak"][ok], out["refined_dfs"][ok] = post["cov"], post["ak"], post["dfs"]
    return out
