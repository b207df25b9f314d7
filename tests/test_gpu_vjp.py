"""spart_vjp on the GPU: the raw C ABI against the definition tools/vjp_defined.py, bit for bit, with the library's own float64
pruned column path (Engine.run on the table the definition builds) as the definition's forward model, over three sensors, four
F and four M with the column subset and the band model dealt round; the chunk edge at F = 16; batch independence; NULL against
zeros; every refusal with poisoned buffers; a non-default stream; Engine.vjp / spart_amd.vjp against the raw call.  If a
mismatch shows here and not in tests/test_vjp_host.py, the cause is in the kernels' index maps, not in the formula."""
import itertools

import numpy as np
import pytest

from helpers.lut_calls import hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.vjp_calls import FILL, FREE, HYPER, S2, S3, SUBSETS, check_against_definition, make_case, same, vd, vjp_call

pytestmark = pytest.mark.gpu
FS, MS = (1, 2, 6, 16), (1, 63, 65, 70)


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {S2: get_engine(S2, 0), S3: get_engine(S3, 0), HYPER: get_engine(None, 0, sensor_info=hyper_si)}


def grid():
    """sensor x F x M with the column subset and the band model dealt round: every subset meets every sensor and every F, and
    the SRF band model (single columns only) meets every sensor and every F too"""
    out = []
    for g, (sensor, F, M) in enumerate(itertools.product((S2, S3, HYPER), FS, MS)):
        subset = SUBSETS[g % len(SUBSETS)]
        out.append((sensor, F, M, subset, 1 if len(subset) == 1 and (g + g // 4) % 2 == 0 else 0))
    return out


def test_the_grid_deals_everything_everywhere():
    cases = grid()
    assert len(cases) == 48
    for key in (0, 1):                                                        # by sensor, by F
        for v in {c[key] for c in cases}:
            mine = [c for c in cases if c[key] == v]
            assert {c[3] for c in mine} == set(SUBSETS) and {c[4] for c in mine} == {0, 1}, (key, v)
    assert {c[3] for c in cases if c[4] == 1} == {(0,), (1,), (2,)} and any(c[4] == 1 and c[2] >= 63 for c in cases)


@pytest.mark.parametrize("sensor,F,M,subset,band_model", grid())
def test_raw_call_against_the_definition(torch_mod, engines, sensor, F, M, subset, band_model):
    eng = engines[sensor]
    case = make_case(eng.nb, FREE[F], M, subset, seed=2000 + 37 * F + M + 5 * len(subset) + subset[0])
    ref, got = check_against_definition(torch_mod, eng, case, band_model=band_model, what=(sensor, F, M, subset, band_model))
    if M >= 63:
        assert np.isnan(got[3]).all() and np.isnan(got[4]).all() and np.isfinite(got[[2, 5]]).all()


def test_options_reach_the_forward_call(torch_mod, engines):
    """nlayers, the Newton prelude and a rel_step of the caller's, each against the definition configured alike, and each
    different from the default's result"""
    eng = engines[S2]
    case = make_case(eng.nb, FREE[2], 5, (0, 1), seed=7)
    plain, _ = check_against_definition(torch_mod, eng, case, what="defaults")
    for kw in (dict(nlayers=20), dict(fast_prelude=1), dict(rel_step=0.05), dict(rel_step=0.5)):
        ref, _ = check_against_definition(torch_mod, eng, case, what=kw, **kw)
        assert not same(ref, plain), kw


def test_the_chunk_edge(torch_mod, engines):
    """F = 16: chunks of 2^19 / 32 = 16384 observations, so M = 16385 is a full chunk and a chunk of one row; the first and the
    last row and 64 rows across the boundary are the bits of the same rows evaluated alone"""
    eng = engines[S2]
    F, M = 16, (1 << 19) // 32 + 1
    assert vd.chunk_of(F) == M - 1
    base, free, lo, hi, gy, _ = make_case(eng.nb, FREE[F], M, (0,), seed=3)
    rc, whole, _ = vjp_call(torch_mod, eng, base, free, lo, hi, gy)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    rows = np.r_[0, np.arange(M - 64, M)]                                     # the first row, then 63 rows of chunk 0 and chunk 1's one
    assert rows.size == 65 and rows[-1] == M - 1 == vd.chunk_of(F) and rows[-2] == vd.chunk_of(F) - 1
    rc, alone, _ = vjp_call(torch_mod, eng, base[rows], free, lo, hi, [gy[0][rows], None, None])
    assert rc == 0 and same(alone, whole[rows])
    finite = np.isfinite(whole).all(axis=1)
    assert finite.mean() > 0.99 and np.isnan(whole[3]).all() and np.isnan(whole[4]).all() and finite[M - 1] and finite[M - 2]
    need = lambda M_: int(eng.lib.spart_vjp_workspace_bytes(eng.ctx, M_, F))      # noqa: E731
    assert need(M - 1) == need(M) == need(2000000000) and 0 < need(1) < need(M)    # one chunk's, whatever M is


def test_a_permuted_batch_gives_permuted_bits_and_null_is_a_zero_block(torch_mod, engines):
    eng = engines[S3]
    base, free, lo, hi, gy, _ = make_case(eng.nb, FREE[6], 70, (0, 1, 2), seed=12)
    rc, ref, _ = vjp_call(torch_mod, eng, base, free, lo, hi, gy)
    assert rc == 0 and np.isfinite(ref).all(axis=1).mean() > 0.5
    p = np.random.default_rng(1).permutation(70)
    rc, perm, _ = vjp_call(torch_mod, eng, base[p], free, lo, hi, [g[p] for g in gy])
    assert rc == 0 and same(perm, ref[p])
    for keep in ((0,), (1, 2), (2,)):
        rc, null, _ = vjp_call(torch_mod, eng, base, free, lo, hi, [g if c in keep else None for c, g in enumerate(gy)])
        rc2, zero, _ = vjp_call(torch_mod, eng, base, free, lo, hi, [g if c in keep else np.zeros_like(g) for c, g in enumerate(gy)])
        assert rc == 0 and rc2 == 0 and same(null, zero) and not same(null, ref), keep
    q = [3, 0, 5, 1, 4, 2]                                                   # the free columns permuted: the gradient's columns
    rc, fperm, _ = vjp_call(torch_mod, eng, base, [free[i] for i in q], lo[q], hi[q], gy)
    assert rc == 0 and same(fperm, ref[:, q])


def test_a_non_default_stream(torch_mod, engines):
    eng = engines[S2]
    base, free, lo, hi, gy, _ = make_case(eng.nb, FREE[6], 65, (0, 2), seed=4)
    rc, ref, _ = vjp_call(torch_mod, eng, base, free, lo, hi, gy)
    side = torch_mod.cuda.Stream(eng.device)
    with torch_mod.cuda.stream(side):
        rc2, got, _ = vjp_call(torch_mod, eng, base, free, lo, hi, gy)
    assert rc == 0 and rc2 == 0 and same(got, ref) and np.isfinite(ref).any()


def test_refusals_leave_every_buffer_untouched(torch_mod, engines):
    from spart_amd import get_engine
    eng = engines[S2]
    base, free, lo, hi, gy, _ = make_case(eng.nb, FREE[2], 3, (0,), seed=5)
    two = [gy[0], None, gy[0]]
    need = int(eng.lib.spart_vjp_workspace_bytes(eng.ctx, 3, 2))
    # each entry: what is wrong -> the refusal met; an entry is wrong in what it names AND in everything listed after it that a
    # call can be wrong in at once, so each refusal is met ahead of all later ones
    ladder = [(dict(F=0), -1, "F = 0"), (dict(null=("free",)), -1, "null argument"), (dict(nlayers=-1), -1, "nlayers = -1"),
              (dict(free=[15, 15]), -1, "free twice"), (dict(lo=[0.1, 80.0]), -1, "bounds of free_cols[1]"),
              (dict(null=("opt",)), -1, "opt is null"), (dict(band_model=2), -1, "band_model = 2"), (dict(rel_step=0.6), -1, "rel_step = 0.6"),
              (dict(rel_step=-1e-3), -1, "rel_step = -0.001"), (dict(null=("gy",)), -1, "gy is null"), (dict(gy=[None] * 3), -1, "every entry of gy"),
              (dict(gy=two, band_model=1), -1, "exactly one entry"), (dict(null=("grad",)), -1, "grad is null"), (dict(M=-1), -1, "M = -1"),
              (dict(M=2000000001), -1, "M = 2000000001"), (dict(null=("base",)), -1, "base is null"), (dict(null=("base[26]",)), -1, "base[26] is null"),
              (dict(ctx=get_engine(None, 0).ctx), -4, "no sensor"), (dict(ws_bytes=need - 1), -3, f"{need} bytes needed"),
              (dict(null=("ws",)), -3, "bytes needed")]

    def call(kw):
        kw = dict(kw)
        args = dict(free=free, lo=lo, hi=hi, gy=gy)
        args.update({k: kw.pop(k) for k in ("free", "lo", "hi", "gy") if k in kw})
        rc, grad, untouched = vjp_call(torch_mod, eng, base, args["free"], args["lo"], args["hi"], args["gy"], **kw)
        return rc, eng.lib.spart_last_error(eng.ctx).decode(), grad, untouched

    for i, (kw, code, text) in enumerate(ladder):
        rc, msg, grad, untouched = call(kw)
        assert rc == code and text in msg and untouched and (grad == FILL).all(), (kw, rc, msg)
        for later, _, _ in ladder[i + 1:]:
            both = dict(later, **kw)
            if set(later) & set(kw) and not ("null" in later and "null" in kw and len(set(later) & set(kw)) == 1):
                continue                                                     # (one argument cannot be wrong in two ways)
            if "opt" in later.get("null", ()) and {"nlayers", "band_model", "rel_step"} & set(kw):
                continue                                                     # (nor can the options be both absent and wrong)
            if "null" in later and "null" in kw:
                both["null"] = tuple(kw["null"]) + tuple(later["null"])
            rc, msg, grad, untouched = call(both)
            assert rc == code and text in msg and untouched, (kw, later, rc, msg)
    rc, msg, grad, untouched = call(dict(M=0))
    assert rc == 0 and untouched                                             # M = 0 launches nothing
    rc, msg, grad, untouched = call(dict(M=0, null=("base", "ws")))
    assert rc == 0 and untouched
    for sizes in ((0, 2), (-1, 2), (3, 0), (3, 17), (2000000001, 2)):
        assert eng.lib.spart_vjp_workspace_bytes(eng.ctx, *sizes) == 0, sizes
    assert eng.lib.spart_vjp_workspace_bytes(get_engine(None, 0).ctx, 3, 2) == 0
    rc, msg, grad, untouched = call({})
    assert rc == 0 and not untouched and np.isfinite(grad).all()


def test_engine_and_host_forms_are_the_raw_call(torch_mod, engines):
    import spart_amd
    eng = engines[S2]
    names = FREE[6]
    base, free, lo, hi, gy, _ = make_case(eng.nb, names, 9, (0, 2), seed=6)
    rc, ref, _ = vjp_call(torch_mod, eng, base, free, lo, hi, gy)
    assert rc == 0
    n0 = eng.calls["spart_vjp"]
    P = torch_mod.as_tensor(base.T.copy(), device=eng.device)
    res = eng.vjp(P, {"R_TOC": torch_mod.as_tensor(gy[0], device=eng.device), "L_TOA": gy[2], "R_TOA": None}, names)
    assert res["names"] == names and res["grad"].dtype == torch_mod.float64 and same(res["grad"].cpu().numpy(), ref)
    assert eng.calls["spart_vjp"] == n0 + 1
    host = spart_amd.vjp(base.T, {"L_TOA": gy[2], "R_TOC": gy[0]}, S2, names)
    assert host["names"] == names and same(host["grad"], ref)
    # a scalar row broadcasts; bounds, rel_step, lidf, nlayers and the band model travel
    kw = dict(bounds={"LAI": (0.5, 6.0)}, rel_step=0.01, lidf="newton", nlayers=30, band_model="srf")
    one = spart_amd.vjp(list(base[0]), {"R_TOA": gy[0][:2]}, S2, names, **kw)
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[0], hi2[0] = 0.5, 6.0
    rc, want, _ = vjp_call(torch_mod, eng, np.repeat(base[:1], 2, axis=0), free, lo2, hi2, [None, gy[0][:2], None], band_model=1, rel_step=0.01,
                           nlayers=30, fast_prelude=1)
    assert rc == 0 and same(one["grad"], want) and np.isfinite(want).all()
