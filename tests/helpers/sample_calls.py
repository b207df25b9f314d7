"""What the tests of spart_sample share: the raw C-ABI caller (every buffer with guard words behind it), the definition
tools/sample_defined.py configured like the call, and the bit-for-bit comparison under the margin condition."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import ROOT
from helpers.refine_calls import COLUMNS, forward_of, same
from helpers.refine_srf_calls import srf_forward_of

sys.path.insert(0, os.path.join(ROOT, "tools"))
import sample_defined as sd  # noqa: E402

FILL = -7.0
GUARD = 512            # words of FILL behind every output, bytes x 8 of 0xFF around the workspace
OUTS = sd.OUTS
MARGIN = 1e-12         # every decision of a compared run is further than this from its threshold (exp is not pinned to the bit)
KINDS = {"n_accept": np.int64, "status": np.int32}


def out_shapes(M, F, W, n_keep):
    return {"mean": (M, F), "cov": (M, F, F), "std": (M, F), "best_x": (M, F), "best_cost": (M,), "n_accept": (M,), "status": (M,),
            "chain": (M, n_keep, W, F), "chain_cost": (M, n_keep, W), "last": (M, W, F), "last_cost": (M, W)}


def sample_call(torch, eng, base, free, lo, hi, obs, weights=None, prior_mean=None, prior_weight=None, column=0, band_model=0, W=8,
                n_steps=6, burn=2, thin=2, a=0.0, temperature=0.0, rel_init=0.0, init_radius=None, init=None, step0=0, obs_offset=0,
                seed=0, nlayers=0, fast_prelude=0, outputs=OUTS, null=(), ws_bytes=None, M=None, F=None, ctx="own",
                weights_per_obs=None, prior_per_obs=None):
    """One spart_sample through ctypes -> (rc, dict of numpy outputs).  Every output of ``outputs`` gets a buffer pre-filled with
    FILL, GUARD words of FILL behind it; the others are passed as NULL.  ``null``: names of base / base[i] / free / lo / hi / obs
    / opt / out / ws to pass as NULL; ``M`` / ``F``: sizes to pass in place of the arrays' own; ``ws_bytes``: the workspace size
    handed in.  The guards are asserted."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, f, nb = base.shape[0], len(free), eng.nb
    up = lambda v: None if v is None else torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=dev)     # noqa: E731
    Bt, ot, wt, pmt, pwt, rt, it = (up(v) for v in (base.T, obs, weights, prior_mean, prior_weight, init_radius, init))
    n_keep = max((n_steps - burn) // max(thin, 1), 1)
    shapes = out_shapes(m, f, W if W > 0 else 8, n_keep)
    size = {k: int(np.prod(shapes[k])) for k in OUTS}
    tdt = {"n_accept": torch.int64, "status": torch.int32}
    buf = {k: torch.full((size[k] + GUARD,), int(FILL) if k in tdt else FILL, dtype=tdt.get(k, torch.float64), device=dev) for k in outputs}
    so = _lib.SpartSampleOut(**{k: buf[k].data_ptr() for k in outputs})
    ptr = lambda t: None if t is None else t.data_ptr()     # noqa: E731
    wper = int(weights is not None and np.ndim(weights) == 2) if weights_per_obs is None else weights_per_obs
    pper = int(prior_weight is not None and np.ndim(prior_weight) == 2) if prior_per_obs is None else prior_per_obs
    opt = _lib.SpartSampleOpt(column=column, band_model=band_model, fast_prelude=fast_prelude, nlayers=nlayers, weights_per_obs=wper,
                              prior_per_obs=pper, prior_mean=ptr(pmt), prior_weight=ptr(pwt), W=W, n_steps=n_steps, burn=burn,
                              thin=thin, a=a, temperature=temperature, rel_init=rel_init, init_radius=ptr(rt), init=ptr(it),
                              step0=step0, obs_offset=obs_offset, seed=seed)
    need = int(eng.lib.spart_sample_workspace_bytes(eng.ctx, m, f, W))
    given = need if ws_bytes is None else ws_bytes
    pad = GUARD * 8
    ws = torch.full((max(need, given, 256) + 2 * pad,), 0xFF, dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    pick = lambda name, v: None if name in null else v     # noqa: E731
    rc = eng.lib.spart_sample(eng.ctx if ctx == "own" else ctx, m if M is None else M,
                              pick("base", (_lib.vp * 27)(*[pick(f"base[{i}]", Bt[i].data_ptr()) for i in range(27)])),
                              f if F is None else F, pick("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                              pick("lo", lo.ctypes.data_as(_lib.c_dp)), pick("hi", hi.ctypes.data_as(_lib.c_dp)), pick("obs", ptr(ot)),
                              ptr(wt), pick("opt", ctypes.byref(opt)), pick("out", ctypes.byref(so)), pick("ws", ws.data_ptr() + pad),
                              ctypes.c_size_t(given), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert bool((ws[:pad] == 0xFF).all()) and bool((ws[pad + max(need, given):] == 0xFF).all()), "bytes around the workspace were written"
    for k in outputs:
        assert bool((buf[k][size[k]:] == (int(FILL) if k in tdt else FILL)).all()), f"words behind {k} were written"
    return rc, {k: buf[k][:size[k]].reshape(shapes[k]).cpu().numpy() for k in outputs}


def untouched(got):
    return all((v == (int(FILL) if k in KINDS else FILL)).all() for k, v in got.items())


def defined(torch, eng, base, free, lo, hi, obs, column=0, band_model=0, nlayers=0, fast_prelude=0, **kw):
    """the definition configured like sample_call, with the engine's own float64 column as forward model"""
    fwd = (srf_forward_of if band_model else forward_of)(torch, eng, COLUMNS[column], lidf="newton" if fast_prelude else "literal",
                                                         nlayers=nlayers or None)
    kw.setdefault("n_steps", 6), kw.setdefault("burn", 2), kw.setdefault("thin", 2)
    with np.errstate(all="ignore"):
        return sd.sample_defined(base, free, lo, hi, obs, fwd, **kw)


def differing(got, ref, keys=OUTS):
    """{output: count of differing words}"""
    return {k: ("shape / dtype" if got[k].shape != ref[k].shape or got[k].dtype != ref[k].dtype else
                int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()))
            for k in keys if not (got[k].dtype == ref[k].dtype and same(got[k], ref[k]))}


def check_sample(torch, eng, base, free, lo, hi, obs, what="", **kw):
    """the library against the definition in all eleven outputs, bit for bit, under the margin condition -> (ref, got)"""
    ref = defined(torch, eng, base, free, lo, hi, obs, **kw)
    assert ref["margin"] > MARGIN, (what, ref["margin"])
    rc, got = sample_call(torch, eng, base, free, lo, hi, obs, **kw)
    assert rc == 0, (what, eng.lib.spart_last_error(eng.ctx))
    diff = differing(got, ref)
    print(f"spart_sample {what}: {sum(v if isinstance(v, int) else 1 for v in diff.values())} differing words, margin {ref['margin']:.2e}, "
          f"accepted {ref['n_accepted']}, rejected {ref['n_rejected']}, outside {ref['n_outside']}")
    assert not diff, (what, diff)
    return ref, got
