"""What the tests of spart_refine_tiles share beside helpers/refine_calls.py: the raw C-ABI caller, the case builder with its
special pixels, and the comparison with the definition tools/refine_tiles_defined.py.  The case builder takes the forward
model as an argument, so that a case can be pre-checked without a GPU, with the oracle as the forward model."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import ROOT
from helpers.refine_calls import COLUMNS, FILL, GUARD, bounds_of, cols_of, forward_of, rd, same
from helpers.refine_srf_calls import srf_forward_of

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_tiles_defined as rtd  # noqa: E402

PARTITION = [1, 1, 2, 7, 8, 9, 39]          # M = 67: tile boundaries inside and across the groups of 4 and 8 pixels
TILE_KEYS = ("shared", "shared_std", "cost", "cost0", "n_accept")
PIXEL_KEYS = ("local", "local_std", "pixel_cost", "status", "y")
OUTS = ("shared", "shared_std", "local", "local_std", "cost", "cost0", "n_accept", "pixel_cost", "status", "y")


def starts_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def tiles_call(torch, eng, base, shared, local, lo, hi, tile_start, obs, w=None, mean=None, weight=None, smean=None, sweight=None,
               column=0, n_iter=2, lambda0=0.0, band_model=0, guard=False, null=(), ws_bytes=None, n_shared=None, F=None, M=None, T=None,
               ctx="own", sper=None):
    """One spart_refine_tiles through ctypes -> (rc, dict of numpy outputs), every output pre-filled with FILL.  base (M, 27);
    shared, local: column numbers; w None, (nb,) or (M, nb); mean / weight: the local prior, (Fl,) or (M, Fl); smean / sweight:
    the shared prior, (Fs,) or (T, Fs); lambda0 = 0 is the default 1e-2.  ``n_shared`` / ``F`` / ``M`` / ``T`` / ``sper``: values
    to pass in place of the arrays' own; ``null``: names to pass as NULL ("base[i]" for one column); ``guard``: GUARD bytes of 0xFF on BOTH sides of a correctly sized workspace
    must survive."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, nb, free = base.shape[0], obs.shape[1], list(shared) + list(local)
    f, fs = len(free), len(shared)
    ts = np.ascontiguousarray(tile_start, dtype=np.int64)
    t = ts.size - 1
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt = up(base.T)
    ot, wt, mt, pt, smt, spt = up(obs), up(w), up(mean), up(weight), up(smean), up(sweight)
    full = lambda shape, dt=torch.float64: torch.full(shape, int(FILL) if dt is torch.int32 else FILL, dtype=dt, device=dev)  # noqa: E731
    out = {"shared": full((t, fs)), "shared_std": full((t, fs)), "local": full((m, f - fs)), "local_std": full((m, f - fs)),
           "cost": full((t,)), "cost0": full((t,)), "n_accept": full((t,), torch.int32), "pixel_cost": full((m,)),
           "status": full((m,), torch.int32), "y": full((m, nb))}
    opt = _lib.SpartRefineTilesOpt(n_shared=fs if n_shared is None else n_shared, band_model=band_model,
                                   shared_prior_per_tile=int(smean is not None and np.ndim(smean) == 2) if sper is None else sper,
                                   shared_prior_mean=None if smt is None or "smean" in null else smt.data_ptr(),
                                   shared_prior_weight=None if spt is None or "sweight" in null else spt.data_ptr())
    opt.fit = _lib.SpartRefineOpt(column=column, n_iter=n_iter, lambda0=lambda0, weights_per_obs=int(w is not None and np.ndim(w) == 2),
                                  prior_per_obs=int(mean is not None and np.ndim(mean) == 2),
                                  prior_mean=None if mt is None else mt.data_ptr(), prior_weight=None if pt is None else pt.data_ptr())
    so = _lib.SpartTilesOut(**{k: (None if k in null else v.data_ptr()) for k, v in out.items()})
    need = int(eng.lib.spart_tiles_workspace_bytes(eng.ctx, m, f, fs))
    size = need if ws_bytes is None else ws_bytes
    if guard:
        assert ws_bytes is None and need > 0
        ws = torch.full((need + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
        wsp = ws.data_ptr() + GUARD
    else:
        ws = torch.empty(max(size, 256), dtype=torch.uint8, device=dev)
        wsp = ws.data_ptr()
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    ptr = lambda name, val: None if name in null else val     # noqa: E731
    rc = eng.lib.spart_refine_tiles(eng.ctx if ctx == "own" else ctx, m if M is None else M,
                                    ptr("base", (_lib.vp * 27)(*[ptr(f"base[{i}]", Bt[i].data_ptr()) for i in range(27)])), f if F is None else F,
                                    ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), ptr("lo", lo.ctypes.data_as(_lib.c_dp)),
                                    ptr("hi", hi.ctypes.data_as(_lib.c_dp)), t if T is None else T,
                                    ptr("tile_start", ts.ctypes.data_as(_lib.c_i64p)), ptr("obs", ot.data_ptr()),
                                    None if wt is None else wt.data_ptr(), ptr("opt", ctypes.byref(opt)), ptr("out", ctypes.byref(so)),
                                    ptr("ws", wsp), ctypes.c_size_t(size), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert bool((ws[:GUARD] == 0xFF).all()) and bool((ws[GUARD + need:] == 0xFF).all()), "bytes around the workspace were written"
    return rc, {k: val.cpu().numpy() for k, val in out.items()}


def make_tiles_case(fwd, shared, local, sizes, kind, lprior, sprior, seed, special=None, dead_tile=None, lambda0=None, move=0.1):
    """truth = LHS rows with every shared name constant over a tile (its first pixel's draw); obs = ``fwd`` at the truth, 1 %
    noise; starts moved up to ``move`` = 10 % of the range.  ``kind``: "none" / "shared" ((nb,)) / "per_pixel" ((M, nb), 15 % zeros over NaN
    observations) weights; ``lprior`` / ``sprior``: "none" / "shared" ((Fl,) / (Fs,)) / "per_row" ((M, Fl) with 20 % zero
    weights over NaN means / (T, Fs)).
    Special pixels from ``special`` (a pixel index, M >= special + 4): +0 a start outside the bounds; +1 a NaN fixed parameter
    (a dead pixel); +2 a fully masked pixel over NaN observations (per-pixel weights); +3 a NaN in the shared column unless it
    is its tile's first pixel (never read).  ``dead_tile``: a pixel that is a tile of its own and gets a NaN fixed parameter.
    ``lambda0``: the first damping of the case (None = the default; a small one makes the first steps long enough to be rejected).
    -> dict of tiles_call's / refine_tiles_defined's arguments (names -> column numbers) and ``truth``"""
    from spart_amd import workloads
    rng = np.random.default_rng(seed)
    names = list(shared) + list(local)
    free, (lo, hi) = cols_of(names), bounds_of(names)
    Fs, Fl = len(shared), len(local)
    F = Fs + Fl
    ts = starts_of(sizes)
    M, T = int(ts[-1]), len(sizes)
    tile_of = np.repeat(np.arange(T), sizes)
    truth = workloads.lhs_params(M, "full", seed=seed)
    truth[:, free[:Fs]] = truth[ts[:-1]][tile_of][:, free[:Fs]]
    with np.errstate(all="ignore"):
        obs = fwd(truth)
    obs = np.where(np.isfinite(obs), obs, 0.3) * (1.0 + 0.01 * rng.normal(size=obs.shape))
    nb = obs.shape[1]
    base = truth.copy()
    base[:, free] = rd.clip_defined(truth[:, free] + rng.uniform(-move, move, (M, F)) * (hi - lo), lo, hi)
    w = None
    if kind == "shared":
        w = 10.0 ** rng.uniform(-1, 2, nb)
        w[rng.random(nb) < 0.2] = 0.0
        w[0] = w[0] or 1.0
    elif kind == "per_pixel":
        w = 10.0 ** rng.uniform(-1, 2, (M, nb))
        w[rng.random((M, nb)) < 0.15] = 0.0
        w[:, 1] = np.where(w[:, 1] == 0.0, 1.0, w[:, 1])
    fixed = 20 if 20 not in free else 26
    if special is not None:
        at = special
        base[at, free[0]] = hi[0] + 0.5 * (hi[0] - lo[0])
        base[at + 1, fixed] = np.nan
        if kind == "per_pixel":
            w[at + 2] = 0.0
        if Fs and at + 3 not in ts[:-1]:
            base[at + 3, free[0]] = np.nan
    if dead_tile is not None:
        assert dead_tile in ts[:-1] and dead_tile + 1 in ts
        base[dead_tile, fixed] = np.nan
    if kind == "per_pixel":
        obs[w == 0.0] = np.nan
    mean = weight = smean = sweight = None
    if lprior != "none" and Fl:
        shape = (M, Fl) if lprior == "per_row" else (Fl,)
        t0 = truth[:, free[Fs:]]
        mean = (t0 if lprior == "per_row" else t0[0]) + 0.1 * rng.normal(size=shape) * (hi - lo)[Fs:]
        weight = np.array(np.broadcast_to(1.0 / (0.1 * (hi - lo)[Fs:]) ** 2, shape))
        if lprior == "per_row":
            zero = rng.random(shape) < 0.2
            mean, weight = np.where(zero, np.nan, mean), np.where(zero, 0.0, weight)
    if sprior != "none" and Fs:
        shape = (T, Fs) if sprior == "per_row" else (Fs,)
        t0 = truth[ts[:-1]][:, free[:Fs]]
        smean = (t0 if sprior == "per_row" else t0[0]) + 0.1 * rng.normal(size=shape) * (hi - lo)[:Fs]
        sweight = np.array(np.broadcast_to(1.0 / (0.1 * (hi - lo)[:Fs]) ** 2, shape))
    return dict(base=base, shared=free[:Fs], local=free[Fs:], lo=lo, hi=hi, tile_start=ts, obs=obs, w=w, mean=mean, weight=weight,
                smean=smean, sweight=sweight, truth=truth, lambda0=lambda0)


def defined_tiles(fwd, case, n_iter, history=None):
    return rtd.refine_tiles_defined(case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["tile_start"],
                                    case["obs"], fwd, weights=case["w"], n_iter=n_iter, prior_mean=case["mean"],
                                    prior_weight=case["weight"], shared_prior_mean=case["smean"],
                                    shared_prior_weight=case["sweight"], history=history,
                                    **({} if case.get("lambda0") is None else {"lambda0": case["lambda0"]}))


def call_tiles(torch, eng, case, column, n_iter, **kw):
    rc, got = tiles_call(torch, eng, case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["tile_start"],
                         case["obs"], case["w"], case["mean"], case["weight"], case["smean"], case["sweight"], column=column,
                         n_iter=n_iter, lambda0=case.get("lambda0") or 0.0, **kw)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    return got


def not_vacuous(ref, n_iter, what):
    """the conditions on the DEFINITION's output that keep a random case from being vacuous: at least half of the live tiles
    accept a step and at least one tile rejects one"""
    live = ref["n_accept"] >= 0
    assert live.any(), what
    assert (ref["cost"][live] <= ref["cost0"][live]).all(), what
    if n_iter >= 1:
        assert (ref["n_accept"][live] >= 1).mean() >= 0.5, (what, ref["n_accept"])
        assert (ref["n_accept"][live] < n_iter).any(), (what, ref["n_accept"])


def differing(got, ref):
    return {k: int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()) for k in OUTS if not same(got[k], ref[k])}


def fwd_of(torch, eng, column, srf=False):
    return (srf_forward_of if srf else forward_of)(torch, eng, COLUMNS[column])


def check_tiles(torch, eng, case, column, n_iter, what, **kw):
    """the library against the definition, bit for bit, and the definition not vacuous -> (ref, got)"""
    ref = defined_tiles(fwd_of(torch, eng, column, kw.get("band_model", 0) == 1), case, n_iter)
    got = call_tiles(torch, eng, case, column, n_iter, **kw)
    assert not differing(got, ref), (what, differing(got, ref))
    not_vacuous(ref, n_iter, what)
    return ref, got
