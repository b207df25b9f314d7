"""What the GPU tests of spart_refine share: the raw C-ABI caller, the forward model the definition tools/refine_defined.py is
given (the library's own float64 pruned column path, configured like the call), the case builder with its special rows, and
the bit-for-bit comparison."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_defined as rd  # noqa: E402

FILL = -7.0        # what refine_call writes into every output before the call: a refused call leaves it there
GUARD = 4096
S2 = "Sentinel2A-MSI"
OUTS = ("x", "cost", "cost0", "std", "n_accept", "y")
F16 = ["Cab", "Cdm", "Cw", "Cs", "Cca", "Cant", "N", "B", "SMp", "LAI", "LIDFa", "LIDFb", "q", "aot550", "uo3", "uh2o"]
FREE = {1: ["LAI"], 2: ["LAI", "Cab"], 6: ["LAI", "Cab", "Cw", "Cdm", "N", "B"], 16: F16}
COLUMNS = ("R_TOC", "R_TOA", "L_TOA")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def forward_of(torch, eng, column, lidf="literal", nlayers=None):
    def forward(rows):
        P = torch.as_tensor(np.ascontiguousarray(rows.T), device=eng.device)
        return eng.run(P, "float64", prune=True, lidf=lidf, nlayers=nlayers)[column].cpu().numpy()
    return forward


def bounds_of(names):
    from spart_amd import workloads
    return (np.array([workloads.RANGES[n][0] for n in names], dtype=np.float64),
            np.array([workloads.RANGES[n][1] for n in names], dtype=np.float64))


def cols_of(names):
    from spart_amd import workloads
    return [workloads.PARAM_NAMES.index(n) for n in names]


def refine_call(torch, eng, base, free, lo, hi, obs, w=None, column=0, n_iter=3, rel_step=0.0, lambda0=0.0, null=(), ws_bytes=None,
                guard=False, M=None, F=None, ctx="own", nlayers=0, fast_prelude=0, entry="spart_refine"):
    """One ``entry`` (spart_refine / spart_refine_srf) through ctypes -> (rc, dict of numpy outputs).  Every output is pre-filled
    with FILL; ``null``: names of base / free / lo / hi / obs / opt / ws / the outputs to pass as NULL, "base[i]" for one NULL
    column; ``M`` / ``F``: sizes to pass in place of the arrays' own;
    ``ws_bytes``: the workspace size handed in; ``guard``: GUARD bytes of 0xFF behind a correctly sized workspace must survive."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, f, nb = base.shape[0], len(free), obs.shape[1]
    Bt = torch.as_tensor(np.ascontiguousarray(base.T), device=dev)
    ot = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float64), device=dev)
    wt = None if w is None else torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64), device=dev)
    out = {"x": torch.full((m, f), FILL, dtype=torch.float64, device=dev), "cost": torch.full((m,), FILL, dtype=torch.float64, device=dev),
           "cost0": torch.full((m,), FILL, dtype=torch.float64, device=dev), "std": torch.full((m, f), FILL, dtype=torch.float64, device=dev),
           "n_accept": torch.full((m,), int(FILL), dtype=torch.int32, device=dev),
           "y": torch.full((m, nb), FILL, dtype=torch.float64, device=dev)}
    opt = _lib.SpartRefineOpt(column=column, n_iter=n_iter, weights_per_obs=1 if (w is not None and np.ndim(w) == 2) else 0,
                              fast_prelude=fast_prelude, nlayers=nlayers, rel_step=rel_step, lambda0=lambda0)
    Mx, Fx = (m if M is None else M), (f if F is None else F)
    c = eng.ctx if ctx == "own" else ctx
    need = int(eng.lib.spart_refine_workspace_bytes(eng.ctx, m, f))
    n = need if ws_bytes is None else ws_bytes
    if guard:
        assert ws_bytes is None and need > 0
        ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    else:
        ws = torch.empty(max(n, 256), dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    ptr = lambda name, v: None if name in null else v     # noqa: E731
    rc = getattr(eng.lib, entry)(c, Mx, ptr("base", (_lib.vp * 27)(*[ptr(f"base[{i}]", Bt[i].data_ptr()) for i in range(27)])), Fx,
                                 ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                                 ptr("lo", lo.ctypes.data_as(_lib.c_dp)), ptr("hi", hi.ctypes.data_as(_lib.c_dp)),
                                 ptr("obs", ot.data_ptr()), None if wt is None else wt.data_ptr(), ptr("opt", ctypes.byref(opt)),
                                 *[ptr(k, out[k].data_ptr()) for k in OUTS], ptr("ws", ws.data_ptr()), ctypes.c_size_t(n),
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert bool((ws[need:] == 0xFF).all()), "bytes behind the workspace were written"
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def make_case(torch, eng, names, M, column, kind, seed):
    """truth = LHS rows; obs = the model at the truth, 1 % noise; starts moved up to 10 % of the range.  Special rows (M >= 63):
    0 a start outside the bounds, 1 a start exactly on hi (s = -1), 2 an all-zero weight row (per-observation weights),
    3 a NaN observation in a weighted band (dead), 4 a NaN parameter that is not free (dead), 5 a negative weight
    (per-observation weights; dead), 6 a NaN observation under a zero weight"""
    from spart_amd import workloads
    rng = np.random.default_rng(seed)
    free, (lo, hi) = cols_of(names), bounds_of(names)
    truth = workloads.lhs_params(M, "full", seed=seed)
    with np.errstate(all="ignore"):
        obs = forward_of(torch, eng, column)(truth)
    obs = np.where(np.isfinite(obs), obs, 0.3) * (1.0 + 0.01 * rng.normal(size=obs.shape))
    nb = obs.shape[1]
    base = truth.copy()
    base[:, free] = rd.clip_defined(truth[:, free] + rng.uniform(-0.1, 0.1, (M, len(free))) * (hi - lo), lo, hi)
    w = None
    if kind == "shared":
        w = 10.0 ** rng.uniform(-1, 2, nb)
        w[rng.random(nb) < 0.2] = 0.0
    elif kind == "per_observation":
        w = 10.0 ** rng.uniform(-1, 2, (M, nb))
        w[rng.random((M, nb)) < 0.15] = 0.0
        obs[w == 0.0] = np.nan                                     # zero weights over NaN observations
    if M >= 63:
        base[0, free[0]] = hi[0] + 0.5 * (hi[0] - lo[0])
        base[1, free[-1]] = hi[-1]
        base[4, 20 if 20 not in free else 26] = np.nan
        if kind == "per_observation":
            w[2] = 0.0
            w[3, nb // 2] = 1.0
            w[5, 0] = -1.0
            w[6, nb - 1], obs[6, nb - 1] = 0.0, np.nan
        obs[3, nb // 2] = np.nan if kind != "shared" or w[nb // 2] != 0 else obs[3, nb // 2]
        if kind == "shared" and w[nb // 2] == 0:
            j = int(np.flatnonzero(w)[0])
            obs[3, j] = np.nan
    return base, free, lo, hi, obs, w


def check_against_definition(torch, eng, case, column, n_iter, what):
    base, free, lo, hi, obs, w = case
    ref = rd.refine_defined(base, free, lo, hi, obs, forward_of(torch, eng, COLUMNS[column]), weights=w, n_iter=n_iter)
    rc, got = refine_call(torch, eng, base, free, lo, hi, obs, w, column=column, n_iter=n_iter)
    assert rc == 0, (what, eng.lib.spart_last_error(eng.ctx))
    for k in OUTS:
        assert same(got[k], ref[k]), (what, k, int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()))
    return ref, got
