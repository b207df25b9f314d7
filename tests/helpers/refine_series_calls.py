"""What the tests of spart_refine_series share beside helpers/refine_tiles_calls.py: the raw C-ABI caller, the case builder
(a tiles case read as series, with the smoothing weights, the link array and the special rows), and the comparison with the
definition tools/refine_series_defined.py.  The case builder takes the forward model as an argument, so that a case can be
pre-checked without a GPU, with the oracle as the forward model."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import ROOT
from helpers.refine_calls import FILL, GUARD, same
from helpers.refine_tiles_calls import OUTS, fwd_of, make_tiles_case

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_series_defined as rsd  # noqa: E402

LENGTHS = [1, 2, 7, 8, 9, 39, 1]            # M = 67: series boundaries inside and across the groups of 4 and 8 series' rows
SERIES_KEYS = ("shared", "shared_std", "cost", "cost0", "n_accept")
ROW_KEYS = ("local", "local_std", "pixel_cost", "status", "y")


def series_call(torch, eng, base, shared, local, lo, hi, series_start, obs, smooth, link=None, w=None, mean=None, weight=None,
                smean=None, sweight=None, column=0, n_iter=2, lambda0=0.0, band_model=0, guard=False, null=(), ws_bytes=None,
                n_shared=None, F=None, M=None, S=None, ctx="own", **_):
    """One spart_refine_series through ctypes -> (rc, dict of numpy outputs), every output pre-filled with FILL.  Arguments as
    helpers.refine_tiles_calls.tiles_call; smooth (Fl,) on the host, link None or (M,).  ``null``: names to pass as NULL;
    ``guard``: GUARD bytes of 0xFF on BOTH sides of a correctly sized workspace must survive."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, nb, free = base.shape[0], obs.shape[1], list(shared) + list(local)
    f, fs = len(free), len(shared)
    ts = np.ascontiguousarray(series_start, dtype=np.int64)
    t = ts.size - 1
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt = up(base.T)
    ot, wt, mt, pt, smt, spt, lt = up(obs), up(w), up(mean), up(weight), up(smean), up(sweight), up(link)
    full = lambda shape, dt=torch.float64: torch.full(shape, int(FILL) if dt is torch.int32 else FILL, dtype=dt, device=dev)  # noqa: E731
    out = {"shared": full((t, fs)), "shared_std": full((t, fs)), "local": full((m, f - fs)), "local_std": full((m, f - fs)),
           "cost": full((t,)), "cost0": full((t,)), "n_accept": full((t,), torch.int32), "pixel_cost": full((m,)),
           "status": full((m,), torch.int32), "y": full((m, nb))}
    gam = None if smooth is None else np.ascontiguousarray(smooth, dtype=np.float64)
    opt = _lib.SpartRefineSeriesOpt(smooth=None if gam is None else gam.ctypes.data_as(_lib.c_dp), link=None if lt is None else lt.data_ptr())
    opt.tiles = _lib.SpartRefineTilesOpt(n_shared=fs if n_shared is None else n_shared, band_model=band_model,
                                         shared_prior_per_tile=int(smean is not None and np.ndim(smean) == 2),
                                         shared_prior_mean=None if smt is None else smt.data_ptr(),
                                         shared_prior_weight=None if spt is None else spt.data_ptr())
    opt.tiles.fit = _lib.SpartRefineOpt(column=column, n_iter=n_iter, lambda0=lambda0, weights_per_obs=int(w is not None and np.ndim(w) == 2),
                                        prior_per_obs=int(mean is not None and np.ndim(mean) == 2),
                                        prior_mean=None if mt is None else mt.data_ptr(), prior_weight=None if pt is None else pt.data_ptr())
    so = _lib.SpartTilesOut(**{k: (None if k in null else v.data_ptr()) for k, v in out.items()})
    need = int(eng.lib.spart_series_workspace_bytes(eng.ctx, m, f, fs))
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
    rc = eng.lib.spart_refine_series(eng.ctx if ctx == "own" else ctx, m if M is None else M,
                                     ptr("base", (_lib.vp * 27)(*[Bt[i].data_ptr() for i in range(27)])), f if F is None else F,
                                     ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), ptr("lo", lo.ctypes.data_as(_lib.c_dp)),
                                     ptr("hi", hi.ctypes.data_as(_lib.c_dp)), t if S is None else S,
                                     ptr("series_start", ts.ctypes.data_as(_lib.c_i64p)), ptr("obs", ot.data_ptr()),
                                     None if wt is None else wt.data_ptr(), ptr("opt", ctypes.byref(opt)), ptr("out", ctypes.byref(so)),
                                     ptr("ws", wsp), ctypes.c_size_t(size), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert bool((ws[:GUARD] == 0xFF).all()) and bool((ws[GUARD + need:] == 0xFF).all()), "bytes around the workspace were written"
    return rc, {k: val.cpu().numpy() for k, val in out.items()}


def make_series_case(fwd, shared, local, sizes, kind, lprior, sprior, linkkind, seed, sigma=0.05, special=None, lambda0=None,
                     move=0.1):
    """helpers.refine_tiles_calls.make_tiles_case without its dead pixels, read as series, plus: smooth = 1 / (sigma range)^2
    for every local but the last of three or more (gamma = 0 there); link by ``linkkind``: "none" (NULL), "varied" (0.25 ... 4)
    or "zero" (varied, with a zero in the middle of every series of 7 or more rows: a broken chain).  A link is given a NaN at
    every series' last row (never read).  Special rows from ``special`` (a row index inside a series, M >= special + 3):
    +0 a start outside the bounds; +1 a fully masked date over NaN observations (per-pixel weights); +2 a NaN in the shared
    column unless it is its series' first row (never read)."""
    case = make_tiles_case(fwd, shared, local, sizes, kind, lprior, sprior, seed, special=None, dead_tile=None, lambda0=lambda0,
                           move=move)
    rng = np.random.default_rng(seed + 1000)
    Fs, Fl = len(shared), len(local)
    lo, hi, ts = case["lo"], case["hi"], case["tile_start"]
    M = int(ts[-1])
    smooth = 1.0 / (sigma * (hi - lo)[Fs:]) ** 2
    if Fl >= 3:
        smooth[-1] = 0.0
    link = None
    if linkkind != "none":
        link = 2.0 ** rng.uniform(-2, 2, M)
        if linkkind == "zero":
            for t in range(ts.size - 1):
                if ts[t + 1] - ts[t] >= 7:
                    link[(ts[t] + ts[t + 1]) // 2] = 0.0
        link[ts[1:] - 1] = np.nan
    if special is not None:
        at = special
        free = case["shared"] + case["local"]
        case["base"][at, free[0]] = hi[0] + 0.5 * (hi[0] - lo[0])
        if kind == "per_pixel":
            case["w"][at + 1] = 0.0
            case["obs"][at + 1] = np.nan
        if Fs and at + 2 not in ts[:-1]:
            case["base"][at + 2, free[0]] = np.nan
    case["series_start"] = case.pop("tile_start")
    case["smooth"], case["link"] = smooth, link
    return case


def defined_series(fwd, case, n_iter, history=None, smooth=None, **kw):
    return rsd.refine_series_defined(case["base"], case["shared"], case["local"], case["lo"], case["hi"], case["series_start"],
                                     case["obs"], fwd, case["smooth"] if smooth is None else smooth, link=case["link"],
                                     weights=case["w"], n_iter=n_iter, prior_mean=case["mean"], prior_weight=case["weight"],
                                     shared_prior_mean=case["smean"], shared_prior_weight=case["sweight"], history=history,
                                     **({} if case.get("lambda0") is None else {"lambda0": case["lambda0"]}), **kw)


def call_series(torch, eng, case, column, n_iter, **kw):
    args = {k: v for k, v in case.items() if k not in ("truth", "lambda0")}
    rc, got = series_call(torch, eng, column=column, n_iter=n_iter, lambda0=case.get("lambda0") or 0.0, **{**args, **kw})
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    return got


def not_vacuous(fwd, case, ref, n_iter, what):
    """the conditions on the DEFINITION's output that keep a random case with gamma > 0 from being vacuous: at least half of the
    live series accept a step, at least one rejects one, and in at least half of them ``local`` differs from the gamma = 0
    result of the same inputs (otherwise the chain was never exercised)"""
    live = ref["n_accept"] >= 0
    assert live.any(), what
    assert (ref["cost"][live] <= ref["cost0"][live]).all(), what
    if n_iter >= 1:
        assert (ref["n_accept"][live] >= 1).mean() >= 0.5, (what, ref["n_accept"])
        assert (ref["n_accept"][live] < n_iter).any(), (what, ref["n_accept"])
        flat = defined_series(fwd, case, n_iter, smooth=np.zeros_like(case["smooth"]), want_std=False)
        ts = case["series_start"]
        moved = np.array([not same(ref["local"][ts[t]:ts[t + 1]], flat["local"][ts[t]:ts[t + 1]]) for t in range(ts.size - 1)])
        assert moved[live].mean() >= 0.5, (what, moved)


def differing(got, ref):
    return {k: int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()) for k in OUTS if not same(got[k], ref[k])}


def check_series(torch, eng, case, column, n_iter, what, **kw):
    """the library against the definition, bit for bit, and the definition not vacuous -> (ref, got)"""
    fwd = fwd_of(torch, eng, column, kw.get("band_model", 0) == 1)
    ref = defined_series(fwd, case, n_iter)
    got = call_series(torch, eng, case, column, n_iter, **kw)
    assert not differing(got, ref), (what, differing(got, ref))
    not_vacuous(fwd, case, ref, n_iter, what)
    return ref, got
