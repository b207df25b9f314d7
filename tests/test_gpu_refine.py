"""spart_refine on the GPU: the raw C ABI against the definition tools/refine_defined.py, bit for bit, with the library's own
float64 column path (eng.run(..., "float64", prune=True)) as the definition's forward model; the chunk boundary; the twin
experiment; retrieve(refine=...); and the refusals, which must leave every output and the bytes behind the workspace alone.
If a mismatch shows here and not in tests/test_refine_host.py, the cause is contraction or a fast-math form in the kernel, not
the formula."""
import ctypes
import os
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, hyper_si, torch_mod  # noqa: F401 (fixtures)

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_defined as rd  # noqa: E402

pytestmark = pytest.mark.gpu

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


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {"s2": get_engine(S2, 0), "hyper": get_engine(None, 0, sensor_info=hyper_si)}


def forward_of(torch, eng, column):
    def forward(rows):
        P = torch.as_tensor(np.ascontiguousarray(rows.T), device=eng.device)
        return eng.run(P, "float64", prune=True)[column].cpu().numpy()
    return forward


def bounds_of(names):
    from spart_amd import workloads
    return (np.array([workloads.RANGES[n][0] for n in names], dtype=np.float64),
            np.array([workloads.RANGES[n][1] for n in names], dtype=np.float64))


def cols_of(names):
    from spart_amd import workloads
    return [workloads.PARAM_NAMES.index(n) for n in names]


def refine_call(torch, eng, base, free, lo, hi, obs, w=None, column=0, n_iter=3, rel_step=0.0, lambda0=0.0, null=(), ws_bytes=None,
                guard=False, M=None, F=None, ctx="own", nlayers=0):
    """One spart_refine through ctypes -> (rc, dict of numpy outputs).  Every output is pre-filled with FILL; ``null``: names
    of base / free / lo / hi / obs / opt / the outputs to pass as NULL; ``M`` / ``F``: sizes to pass in place of the arrays' own;
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
                              fast_prelude=0, nlayers=nlayers, rel_step=rel_step, lambda0=lambda0)
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
    rc = eng.lib.spart_refine(c, Mx, ptr("base", (_lib.vp * 27)(*[Bt[i].data_ptr() for i in range(27)])), Fx,
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


@pytest.mark.parametrize("F", [1, 2, 6, 16])
@pytest.mark.parametrize("sensor", ["s2", "hyper"])
def test_definition_bit_for_bit(torch_mod, engines, sensor, F):
    eng = engines[sensor]
    kinds = ("none", "shared", "per_observation")
    seen = set()
    for i, M in enumerate((1, 63, 65, 1000)):
        for j, n_iter in enumerate((0, 1, 3)):
            column, kind = (i + j + F) % 3, kinds[(i + 2 * j + F) % 3]
            seen.add((column, kind))
            case = make_case(torch_mod, eng, FREE[F], M, COLUMNS[column], kind, 100 * F + 10 * i + j)
            ref, _ = check_against_definition(torch_mod, eng, case, column, n_iter, (sensor, F, M, n_iter, kind, column))
            if M >= 63:
                dead = [3, 4] + ([5] if kind == "per_observation" else [])
                assert (ref["n_accept"][dead] == -1).all() and np.isnan(ref["std"][dead]).all(), (sensor, F, M, kind)
                assert ref["n_accept"][0] >= 0 and ref["n_accept"][1] >= 0 and (ref["x"][0] <= case[3]).all()
                if kind == "per_observation":
                    assert ref["cost0"][2] == 0 and ref["n_accept"][2] == 0 and ref["n_accept"][6] >= 0
                alive = ref["n_accept"] >= 0
                assert alive.mean() > 0.5 and (ref["cost"][alive] <= ref["cost0"][alive]).all()
                if n_iter == 3 and kind == "none":
                    assert np.median(ref["cost"][alive] / ref["cost0"][alive]) < 0.9       # the fit does move
    assert len({c for c, _ in seen}) == 3 and len({k for _, k in seen}) == 3


def test_null_optional_outputs_leave_the_others_correct(torch_mod, engines):
    eng = engines["s2"]
    case = make_case(torch_mod, eng, FREE[6], 65, "R_TOA", "per_observation", 77)
    ref, _ = check_against_definition(torch_mod, eng, case, 1, 2, "all outputs")
    base, free, lo, hi, obs, w = case
    for null in (("cost0", "std", "n_accept", "y"), ("y",), ("std", "cost0")):
        rc, got = refine_call(torch_mod, eng, base, free, lo, hi, obs, w, column=1, n_iter=2, null=null)
        assert rc == 0
        for k in OUTS:
            assert (got[k] == FILL).all() if k in null else same(got[k], ref[k]), (null, k)
    # rel_step / lambda0 given explicitly equal the defaults that 0 stands for; other values follow the definition
    rc, got = refine_call(torch_mod, eng, base, free, lo, hi, obs, w, column=1, n_iter=2, rel_step=1e-3, lambda0=1e-2)
    assert rc == 0 and all(same(got[k], ref[k]) for k in OUTS)
    ref2 = rd.refine_defined(base, free, lo, hi, obs, forward_of(torch_mod, eng, "R_TOA"), weights=w, n_iter=2, rel_step=3e-3, lambda0=1.0)
    rc, got = refine_call(torch_mod, eng, base, free, lo, hi, obs, w, column=1, n_iter=2, rel_step=3e-3, lambda0=1.0)
    assert rc == 0 and all(same(got[k], ref2[k]) for k in OUTS) and not same(ref2["x"], ref["x"])


def test_chunk_boundary(torch_mod, engines):
    """M = 31 000 with F = 16: the chunk is (1 << 19) // 17 = 30 840 observations, so the call runs two chunks"""
    eng = engines["s2"]
    M = 31000
    assert (1 << 19) // 17 == 30840 < M
    case = make_case(torch_mod, eng, F16, M, "R_TOC", "none", 5)
    ref, got = check_against_definition(torch_mod, eng, case, 0, 2, "two chunks")
    base, free, lo, hi, obs, _ = case
    h = M // 2
    for sl in (slice(0, h), slice(h, M)):
        rc, part = refine_call(torch_mod, eng, base[sl], free, lo, hi, obs[sl], None, column=0, n_iter=2)
        assert rc == 0 and all(same(part[k], got[k][sl]) for k in OUTS)
    one = int(eng.lib.spart_refine_workspace_bytes(eng.ctx, 30840, 16))
    assert one == int(eng.lib.spart_refine_workspace_bytes(eng.ctx, 2_000_000_000, 16)) > int(eng.lib.spart_refine_workspace_bytes(eng.ctx, 1000, 16)) > 0


def twin_case(torch, eng):
    from spart_amd import workloads
    names = ["LAI", "Cab", "Cw", "Cdm"]
    lo, hi = bounds_of(names)
    free = cols_of(names)
    truth = workloads.lhs_params(48, "full", seed=5)
    obs = forward_of(torch, eng, "R_TOC")(truth)
    start = truth.copy()
    start[:, free] = truth[:, free] + 0.15 * (hi - lo) * np.sign(0.5 * (lo + hi) - truth[:, free])
    return names, truth, start, free, lo, hi, obs


def test_twin_experiment(torch_mod, engines):
    """the conditions of tests/test_refine_host.py::test_twin_experiment_with_the_oracle, the GPU as the forward model"""
    eng = engines["s2"]
    names, truth, start, free, lo, hi, obs = twin_case(torch_mod, eng)
    res = eng.refine(torch_mod.as_tensor(np.ascontiguousarray(start.T), device=eng.device), obs, names, n_iter=10)
    x, cost, cost0 = (res[k].cpu().numpy() for k in ("x", "cost", "cost0"))
    print("twin: max cost / cost0 =", float((cost / cost0).max()), " max |x - truth| / range =", float((np.abs(x - truth[:, free]) / (hi - lo)).max()))
    assert res["names"] == names and (res["n_accept"].cpu().numpy() >= 1).all()
    assert (cost <= cost0).all() and (cost <= 1e-8 * cost0).all(), float((cost / cost0).max())
    assert (np.abs(x - truth[:, free]) <= 1e-6 * (hi - lo)).all()
    r3 = eng.refine(list(start.T), obs, names, n_iter=3)
    r5 = eng.refine(list(start.T), obs, names, n_iter=5)
    assert (r5["cost"] <= r3["cost"]).all() and (res["cost"] <= r5["cost"]).all()
    # a non-default stream: the same bits
    s = torch_mod.cuda.Stream(eng.device)
    s.wait_stream(torch_mod.cuda.current_stream(eng.device))
    with torch_mod.cuda.stream(s):
        other = eng.refine(list(start.T), obs, names, n_iter=10)
    s.synchronize()
    for k in OUTS:
        assert same(other[k].cpu().numpy(), res[k].cpu().numpy()), k
    # the host form
    import spart_amd
    host = spart_amd.refine(start.T, obs, S2, names, n_iter=10)
    assert all(same(host[k], res[k].cpu().numpy()) for k in OUTS) and host["names"] == names


def test_retrieve_with_refine(torch_mod, tmp_path):
    import spart_amd
    from spart_amd import workloads
    P = workloads.lhs_params(4000, "full", seed=12)
    d = str(tmp_path / "lut")
    spart_amd.generate_lut(P, S2, path=d, dtype="float64")
    truth = workloads.lhs_params(48, "full", seed=13)
    obs = spart_amd.get_engine(S2, 0).run(torch_mod.as_tensor(np.ascontiguousarray(truth.T), device="cuda:0"), "float64", prune=True)["R_TOC"].cpu().numpy()
    names = ["LAI", "Cab", "Cw", "Cdm"]
    for summary in ("host", "device"):
        plain = spart_amd.retrieve(d, obs, 5, summary=summary)
        got = spart_amd.retrieve(d, obs, 5, summary=summary, refine=names, refine_opts={"n_iter": 5})
        for k, v in plain.items():
            assert (got[k] == v) if k == "names" else same(got[k], v), k
        assert got["refined_names"] == names and got["refined"].shape == (48, 4)
        assert (got["refined_cost"] <= got["refined_cost0"]).all() and (got["refined_accepts"] >= 0).all()
        assert same(got["refined_cost0"], got["cost"][:, 0])
        lo, hi = P[:, cols_of(names)].min(axis=0), P[:, cols_of(names)].max(axis=0)
        assert ((got["refined"] >= lo) & (got["refined"] <= hi)).all() and np.isfinite(got["refined_std"]).any()
        assert (got["refined_cost"] < got["refined_cost0"]).mean() > 0.9
    # observations without a row: NaN and -1
    bad = obs.copy()
    bad[1] = np.nan
    got = spart_amd.retrieve(d, bad, 3, refine=["LAI"])
    assert got["idx"][1, 0] == -1 and np.isnan(got["refined"][1]).all() and got["refined_accepts"][1] == -1
    assert np.isnan(got["refined_cost"][1]) and np.isfinite(got["refined"][0]).all()


def test_refusals_leave_outputs_and_guard_untouched(torch_mod, engines):
    from spart_amd import get_engine
    eng = engines["s2"]
    names = ["LAI", "Cab", "Cw"]
    case = make_case(torch_mod, eng, names, 65, "R_TOC", "per_observation", 3)
    base, free, lo, hi, obs, w = case
    need = int(eng.lib.spart_refine_workspace_bytes(eng.ctx, 65, 3))
    assert need > 0
    INVALID, WORKSPACE, NOSENSOR = -1, -3, -4
    inf, nan = np.inf, np.nan
    cases = [(dict(F=0), INVALID), (dict(F=17), INVALID), (dict(free=[15, 0, 27]), INVALID), (dict(free=[15, 0, -1]), INVALID),
             (dict(free=[15, 0, 15]), INVALID), (dict(lo=[0.1, 10, 0.05]), INVALID), (dict(hi=[7, 80, inf]), INVALID),
             (dict(lo=[nan, 10, 0.005]), INVALID), (dict(lo=[7.5, 10, 0.005]), INVALID), (dict(n_iter=-1), INVALID),
             (dict(n_iter=101), INVALID), (dict(column=3), INVALID), (dict(column=-1), INVALID), (dict(rel_step=-1e-3), INVALID),
             (dict(rel_step=inf), INVALID), (dict(lambda0=nan), INVALID), (dict(lambda0=-1.0), INVALID), (dict(M=-1), INVALID),
             (dict(M=2_000_000_001), INVALID), (dict(nlayers=-2), INVALID),
             *[(dict(null=(n,)), INVALID) for n in ("base", "free", "lo", "hi", "obs", "opt", "x", "cost")],
             (dict(ctx=None), INVALID), (dict(null=("ws",)), WORKSPACE), (dict(ws_bytes=need - 1), WORKSPACE), (dict(ws_bytes=0), WORKSPACE),
             (dict(ctx=get_engine(None, 0).ctx), NOSENSOR)]
    for kw, want in cases:
        kw = dict(kw)
        a = dict(base=base, free=kw.pop("free", free), lo=kw.pop("lo", lo), hi=kw.pop("hi", hi), obs=obs, w=w)
        rc, got = refine_call(torch_mod, eng, a["base"], a["free"], a["lo"], a["hi"], a["obs"], a["w"], **kw)
        assert rc == want, (kw, rc, eng.lib.spart_last_error(eng.ctx))
        assert all((got[k] == FILL).all() for k in OUTS), kw
    assert int(eng.lib.spart_refine_workspace_bytes(eng.ctx, 65, 0)) == 0 == int(eng.lib.spart_refine_workspace_bytes(eng.ctx, 0, 3))
    assert int(eng.lib.spart_refine_workspace_bytes(get_engine(None, 0).ctx, 65, 3)) == 0
    # M = 0: ok, nothing launched, nothing written
    rc, got = refine_call(torch_mod, eng, base, free, lo, hi, obs, w, M=0)
    assert rc == 0 and all((got[k] == FILL).all() for k in OUTS)
    # a correctly sized workspace with a guard region behind it
    ref = rd.refine_defined(base, free, lo, hi, obs, forward_of(torch_mod, eng, "R_TOC"), weights=w, n_iter=2)
    rc, got = refine_call(torch_mod, eng, base, free, lo, hi, obs, w, n_iter=2, guard=True)
    assert rc == 0 and all(same(got[k], ref[k]) for k in OUTS)


def test_refine_example_runs(tmp_path):
    """examples/refine.py as a user runs it: its own process, exit code 0, the expected last line"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine.py"), "20000", str(tmp_path / "lut")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "20000 rows" in r.stdout and "refined 4 parameters of 2048 spectra" in r.stdout
