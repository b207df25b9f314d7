"""What the tests of spart_sobol share: the raw C-ABI caller (every buffer with guard words behind it), a case builder, the
definition tools/sobol_defined.py and the bit-for-bit comparison.  The host test passes a loaded library and fake pointers
for the refusals that come before anything is read."""
import ctypes
import os
import sys

import numpy as np

from helpers.lut_calls import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import sobol_defined as sd  # noqa: E402

FILL = -7.0
GUARD = 512            # doubles of 0xFF.. behind every output, bytes x 8 around the workspace
OUTS = sd.OUTS
S2 = "Sentinel2A-MSI"
COLUMNS = ("R_TOC", "R_TOA", "L_TOA")
F16 = ["Cab", "Cdm", "Cw", "Cs", "Cca", "Cant", "N", "B", "SMp", "LAI", "LIDFa", "LIDFb", "q", "aot550", "uo3", "uh2o"]
FREE = {1: ["LAI"], 2: ["LAI", "Cab"], 3: ["LAI", "Cab", "Cw"], 16: F16}


def same(a, b):
    """equal bit for bit, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def differing(got, ref, keys=OUTS):
    """{output: count of differing words}"""
    return {k: int((~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))).sum()) + int(got[k].shape != ref[k].shape)
            for k in keys if not same(got[k], ref[k])}


def cols_of(names):
    from spart_amd import workloads
    return [workloads.PARAM_NAMES.index(n) for n in names]


def bounds_of(names):
    from spart_amd import workloads
    return (np.array([workloads.RANGES[n][0] for n in names], dtype=np.float64),
            np.array([workloads.RANGES[n][1] for n in names], dtype=np.float64))


def design_of(N, F, seed=0):
    """two independent (N, F) designs in [0, 1) (numpy's generator: the tests of the kernels need no low discrepancy)"""
    rng = np.random.default_rng(seed)
    return rng.random((N, F)), rng.random((N, F))


def sites_of(M, seed=5):
    """(M, 27) base rows from the Latin hypercube of the benchmark"""
    from spart_amd import workloads
    return workloads.lhs_params(max(M, 2), "full", seed=seed)[:M].copy()


def sobol_call(torch, eng, base, free, lo, hi, uA, uB, column=0, band_model=0, nlayers=0, fast_prelude=0, null=(), ws_bytes=None,
               guard=True, M=None, F=None, N=None, ctx="own"):
    """One spart_sobol through ctypes -> (rc, dict of numpy outputs), every output pre-filled with FILL.  base (M, 27); free:
    column numbers; ``null``: names of base / base[i] / free / lo / hi / uA / uB / opt / out / ws / the six outputs to pass as
    NULL; ``M`` / ``F`` / ``N``: sizes to pass in place of the arrays' own; ``ws_bytes``: the workspace size handed in;
    ``guard``: GUARD doubles of FILL behind every output and GUARD x 8 bytes of 0xFF on both sides of the workspace survive."""
    from spart_amd import _lib
    dev = eng.device
    base = np.ascontiguousarray(base, dtype=np.float64)
    m, f, nb, n = base.shape[0], len(free), eng.nb, uA.shape[0]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)     # noqa: E731
    Bt, At, Bu = up(base.T), up(uA), up(uB)
    shapes = {k: (m, nb) if k in ("mean", "var") else (m, nb, f) for k in OUTS}
    size = {k: int(np.prod(shapes[k])) for k in OUTS}
    buf = {k: torch.full((size[k] + GUARD,), FILL, dtype=torch.float64, device=dev) for k in OUTS}
    so = _lib.SpartSobolOut(**{k: (None if k in null else buf[k].data_ptr()) for k in OUTS})
    opt = _lib.SpartSobolOpt(column=column, band_model=band_model, fast_prelude=fast_prelude, nlayers=nlayers)
    need = int(eng.lib.spart_sobol_workspace_bytes(eng.ctx, m, n, f))
    given = need if ws_bytes is None else ws_bytes
    pad = GUARD * 8
    ws = torch.full((max(need, given, 256) + 2 * pad,), 0xFF, dtype=torch.uint8, device=dev)
    fc = np.array(free, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    ptr = lambda name, v: None if name in null else v     # noqa: E731
    rc = eng.lib.spart_sobol(eng.ctx if ctx == "own" else ctx, m if M is None else M,
                             ptr("base", (_lib.vp * 27)(*[ptr(f"base[{i}]", Bt[i].data_ptr()) for i in range(27)])),
                             f if F is None else F, ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))),
                             ptr("lo", lo.ctypes.data_as(_lib.c_dp)), ptr("hi", hi.ctypes.data_as(_lib.c_dp)), n if N is None else N,
                             ptr("uA", At.data_ptr()), ptr("uB", Bu.data_ptr()), ptr("opt", ctypes.byref(opt)),
                             ptr("out", ctypes.byref(so)), ptr("ws", ws.data_ptr() + pad), ctypes.c_size_t(given),
                             ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if guard:
        assert bool((ws[:pad] == 0xFF).all()) and bool((ws[pad + max(need, given):] == 0xFF).all()), "bytes around the workspace were written"
        for k in OUTS:
            assert bool((buf[k][size[k]:] == FILL).all()), f"words behind {k} were written"
    return rc, {k: buf[k][:size[k]].reshape(shapes[k]).cpu().numpy() for k in OUTS}


def forward_of(torch, eng, column, band_model=0, nlayers=None, chunk=1 << 19, lidf="literal"):
    """rows (R, 27) -> (R, nb): Engine.run (float64, pruned; ``lidf`` and ``nlayers`` as the call's) on the table the
    definition builds, the *_srf column with band_model 1; in pieces of ``chunk`` rows (a row's column does not depend on its
    batch)"""
    name = COLUMNS[column] + ("_srf" if band_model else "")

    def forward(rows):
        out = []
        for r0 in range(0, rows.shape[0], chunk):
            P = torch.as_tensor(np.ascontiguousarray(rows[r0:r0 + chunk].T), device=eng.device)
            res = eng.run(P, "float64", prune=True, lidf=lidf, nlayers=nlayers, **({"materialize": [name]} if band_model else {}))
            out.append(res[name].cpu().numpy())
        return np.concatenate(out)
    return forward


def nan_signs(v):
    """(NaN words, those of them with the sign bit set)"""
    nan = np.isnan(v)
    return int(nan.sum()), int(np.signbit(v[nan]).sum())


def check_sobol(torch, eng, base, names, uA, uB, column=0, band_model=0, what="", nlayers=0, fast_prelude=0, nan_sites=(), **kw):
    """the library against the definition in all six outputs, bit for bit -> (ref, got); prints the count of differing words.
    ``nlayers`` / ``fast_prelude``: the raw call's (0: the default), and the definition's forward model is configured alike.
    ``nan_sites``: sites whose every word must be NaN on both sides; what sign a NaN carries is left open for them alone (a
    subtraction hands a NaN operand on with the sign its instruction set gives it) and printed."""
    free, (lo, hi) = cols_of(names), bounds_of(names)
    fwd = forward_of(torch, eng, column, band_model, nlayers=nlayers or None, lidf="newton" if fast_prelude else "literal")
    ref = sd.sobol_defined(base, free, lo, hi, uA, uB, fwd)
    rc, got = sobol_call(torch, eng, base, free, lo, hi, uA, uB, column=column, band_model=band_model, nlayers=nlayers,
                         fast_prelude=fast_prelude, **kw)
    assert rc == 0, (what, eng.lib.spart_last_error(eng.ctx))
    counts = differing(got, ref)
    keep = np.setdiff1d(np.arange(base.shape[0]), np.asarray(nan_sites, dtype=np.int64))
    diff = differing({k: got[k][keep] for k in OUTS}, {k: ref[k][keep] for k in OUTS})
    print(f"spart_sobol {what}: {sum(counts.values())} differing words of {sum(v.size for v in ref.values())}")
    assert not diff and not any(counts.values()), (what, diff, counts)
    for m in nan_sites:
        print(f"spart_sobol {what}: site {m}, (NaN words, with the sign bit): the library's",
              {k: nan_signs(got[k][m]) for k in OUTS}, "the definition's", {k: nan_signs(ref[k][m]) for k in OUTS})
        assert all(np.isnan(got[k][m]).all() and np.isnan(ref[k][m]).all() for k in OUTS), (what, m)
    return ref, got


# ---- the chunk arithmetic of sobol_layout / sobol_impl (csrc/spart_capi.hip), restated: tests/test_sobol_host.py holds ROWS
# against the header's sobol_chunk_blocks, so a test that asserts its case with these cannot go vacuous unseen
ROWS = 1 << 19         # SOBOL_ROWS: rows of one forward call at most


def chunk_blocks(F):
    """blocks per chunk: whole blocks of 64 (F + 2) rows within ROWS"""
    return ROWS // (sd.BLOCK * (F + 2))


def layout_of(F, N, M):
    """-> (G, bcap, nslot): blocks per site, blocks per chunk of this call, slots of the workspace"""
    G = N // sd.BLOCK
    bcap = min(M * G, chunk_blocks(F))
    return G, bcap, min(M, bcap // G + 2)


def chunks_of(F, N, M):
    """the launches of a call -> [(b0, bc, first site touched, last site touched)]"""
    G, bcap, _ = layout_of(F, N, M)
    return [(b0, min(bcap, M * G - b0), b0 // G, (b0 + min(bcap, M * G - b0) - 1) // G) for b0 in range(0, M * G, bcap)]
