"""What the tests of spart_vjp share: the raw C-ABI caller (a poisoned gradient buffer with guard words behind it, a poisoned
workspace with guard bytes around it), the forward model the definition tools/vjp_defined.py is given (the library's own float64
pruned column path, configured like the call), the case builder with its planted rows and the bit-for-bit comparison.  The
host test passes a loaded library and fake pointers for the refusals that come before anything is read."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import vjp_defined as vd  # noqa: E402

FILL = -7.0
GUARD = 512            # doubles of FILL behind grad, bytes x 8 of 0xFF around the workspace
S2, S3, HYPER = "Sentinel2A-MSI", "Sentinel3A-OLCI", "hyper211"
COLUMNS = ("R_TOC", "R_TOA", "L_TOA")
F16 = ["Cab", "Cdm", "Cw", "Cs", "Cca", "Cant", "N", "B", "SMp", "LAI", "LIDFa", "LIDFb", "q", "aot550", "uo3", "uh2o"]
FREE = {1: ["LAI"], 2: ["LAI", "Cab"], 6: ["LAI", "Cab", "Cw", "Cdm", "N", "B"], 16: F16}
SUBSETS = ((0,), (1,), (2,), (0, 1), (0, 1, 2))        # of the three columns: each alone, two, all
NAN_FIXED = 20         # tto: never free here, read by every column


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def cols_of(names):
    from spart_amd import workloads
    return [workloads.PARAM_NAMES.index(n) for n in names]


def bounds_of(names):
    from spart_amd import workloads
    return (np.array([workloads.RANGES[n][0] for n in names], dtype=np.float64),
            np.array([workloads.RANGES[n][1] for n in names], dtype=np.float64))


def vjp_call(torch, eng, base, free, lo, hi, gy, band_model=0, rel_step=0.0, nlayers=0, fast_prelude=0, null=(), ws_bytes=None,
             M=None, F=None, ctx="own"):
    """One spart_vjp through ctypes on the current torch stream -> (rc, grad (m, f) numpy, untouched): grad pre-filled with
    FILL, the workspace with 0xFF; ``untouched``: neither was written at all.  base (m, 27); free: column numbers; gy: three
    entries None or (m, nb); ``null``: names of base / base[i] / free / lo / hi / gy / opt / grad / ws to pass as NULL; ``M`` /
    ``F``: sizes to pass in place of the arrays' own; ``ws_bytes``: the workspace size handed in.  The GUARD words behind grad and
    the bytes around the workspace must survive every call."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, f = base.shape[0], len(free)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt = up(base.T)
    gt = [None if g is None else up(g) for g in gy]
    buf = torch.full((m * f + GUARD,), FILL, dtype=torch.float64, device=dev)
    opt = _lib.SpartVjpOpt(band_model=band_model, fast_prelude=fast_prelude, nlayers=nlayers, rel_step=rel_step)
    need = int(eng.lib.spart_vjp_workspace_bytes(eng.ctx, m, f))
    given = need if ws_bytes is None else ws_bytes
    pad = GUARD * 8
    ws = torch.full((max(need, given, 256) + 2 * pad,), 0xFF, dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    ptr = lambda name, v: None if name in null else v     # noqa: E731
    rc = eng.lib.spart_vjp(eng.ctx if ctx == "own" else ctx, m if M is None else M,
                           ptr("base", (_lib.vp * 27)(*[ptr(f"base[{i}]", Bt[i].data_ptr()) for i in range(27)])),
                           f if F is None else F, ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                           ptr("lo", lo.ctypes.data_as(_lib.c_dp)), ptr("hi", hi.ctypes.data_as(_lib.c_dp)),
                           ptr("gy", (_lib.vp * 3)(*[None if g is None else g.data_ptr() for g in gt])), ptr("opt", ctypes.byref(opt)),
                           ptr("grad", buf.data_ptr()), ptr("ws", ws.data_ptr() + pad), ctypes.c_size_t(given),
                           ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert bool((ws[:pad] == 0xFF).all()) and bool((ws[pad + max(need, given):] == 0xFF).all()), "bytes around the workspace were written"
    assert bool((buf[m * f:] == FILL).all()), "words behind grad were written"
    untouched = bool((ws == 0xFF).all()) and bool((buf == FILL).all())
    return rc, buf[:m * f].reshape(m, f).cpu().numpy(), untouched


def forward_of(torch, eng, band_model=0, srf_column=0, nlayers=None, lidf="literal", chunk=1 << 19):
    """rows (R, 27) -> three (R, nb) arrays: Engine.run (float64, pruned; ``lidf`` and ``nlayers`` as the call's) on the table
    the definition builds; with band_model 1 only entry ``srf_column`` is there, the *_srf column; in pieces of ``chunk`` rows (a
    row's column does not depend on its batch)"""
    keys = [COLUMNS[srf_column] + "_srf"] if band_model else list(COLUMNS)

    def forward(rows):
        out = {k: [] for k in keys}
        for r0 in range(0, rows.shape[0], chunk):
            P = torch.as_tensor(np.ascontiguousarray(rows[r0:r0 + chunk].T), device=eng.device)
            res = eng.run(P, "float64", prune=True, lidf=lidf, nlayers=nlayers, **({"materialize": keys} if band_model else {}))
            for k in keys:
                out[k].append(res[k].cpu().numpy())
        got = {k: np.concatenate(v) for k, v in out.items()}
        return [got.get(c + "_srf") for c in COLUMNS] if band_model else [got[c] for c in COLUMNS]
    return forward


def make_case(nb, names, M, subset, seed):
    """base = LHS rows, gy = normal draws for the columns of ``subset`` -> (base, free, lo, hi, gy, zero band).  The band
    ``zero band`` has g exactly 0 in every row and column.  Planted rows (M >= 63): 0 a free parameter exactly on lo, 1 one exactly
    on hi, 2 one outside the bounds, 3 a NaN parameter that is not free, 4 a NaN g"""
    from spart_amd import workloads
    rng = np.random.default_rng(seed)
    free, (lo, hi) = cols_of(names), bounds_of(names)
    base = workloads.lhs_params(max(M, 2), "full", seed=seed)[:M].copy()
    gy = [rng.normal(size=(M, nb)) if c in subset else None for c in range(3)]
    jz = int(rng.integers(nb))
    for g in gy:
        if g is not None:
            g[:, jz] = 0.0
    if M >= 63:
        base[0, free[0]] = lo[0]
        base[1, free[-1]] = hi[-1]
        base[2, free[0]] = hi[0] + 0.5 * (hi[0] - lo[0])
        base[3, NAN_FIXED] = np.nan
        gy[subset[0]][4, (jz + 1) % nb if nb > 1 else 0] = np.nan
    return base, free, lo, hi, gy, jz


def check_case_can_fail(ref, case, M):
    """the properties of the reference that make the comparison worth something, asserted before the library is called"""
    base, free, lo, hi, gy, jz = case
    assert ref.shape == (M, len(free))
    if M < 63:
        assert np.isfinite(ref).all() and (ref != 0).any()
        return
    assert np.isnan(ref[3]).all() and np.isnan(ref[4]).all(), ref[:6]
    assert np.isfinite(ref[[0, 1, 2, 5]]).all() and np.isfinite(ref).all(axis=1).mean() > 0.5
    assert (ref[np.isfinite(ref).all(axis=1)][:, 0] != 0).all()                      # the first free parameter moves every row
    x = vd.clip_defined(base[:, free], lo, hi)
    a, b = vd.steps_defined(x, lo, hi)
    assert b[0, 0] == lo[0] == x[0, 0] and a[1, -1] == hi[-1] == x[1, -1] and a[2, 0] == hi[0] == x[2, 0]      # one-sided there
    assert a[5, 0] - x[5, 0] > 0 and x[5, 0] - b[5, 0] > 0                                                    # central elsewhere


def check_against_definition(torch, eng, case, band_model=0, rel_step=0.0, what="", **kw):
    base, free, lo, hi, gy, _ = case
    column = next(c for c in range(3) if gy[c] is not None)
    fwd = forward_of(torch, eng, band_model, column, nlayers=kw.get("nlayers") or None, lidf="newton" if kw.get("fast_prelude") else "literal")
    ref = vd.vjp_defined(base, free, lo, hi, gy, fwd, rel_step=rel_step or vd.REL_STEP)
    check_case_can_fail(ref, case, base.shape[0])
    rc, got, _ = vjp_call(torch, eng, base, free, lo, hi, gy, band_model=band_model, rel_step=rel_step, **kw)
    assert rc == 0, (what, eng.lib.spart_last_error(eng.ctx))
    bad = int((~((got == ref) | (np.isnan(got) & np.isnan(ref)))).sum())
    print(f"spart_vjp {what}: {bad} differing words of {ref.size}")
    assert same(got, ref), (what, bad)
    return ref, got
