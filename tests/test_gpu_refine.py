"""spart_refine on the GPU: the raw C ABI against the definition tools/refine_defined.py, bit for bit, with the library's own
float64 column path (eng.run(..., "float64", prune=True)) as the definition's forward model; the chunk boundary; the twin
experiment; retrieve(refine=...); and the refusals, which must leave every output and the bytes behind the workspace alone.
If a mismatch shows here and not in tests/test_refine_host.py, the cause is contraction or a fast-math form in the kernel, not
the formula."""
import os
import sys

import numpy as np
import pytest

from helpers.lut_calls import ROOT, hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import (COLUMNS, F16, FILL, FREE, OUTS, S2, bounds_of, check_against_definition, cols_of, forward_of,  # noqa: F401
                                  make_case, rd, refine_call, same)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {"s2": get_engine(S2, 0), "hyper": get_engine(None, 0, sensor_info=hyper_si)}


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


@pytest.mark.parametrize("entry", ["spart_refine", "spart_refine_srf"])
def test_the_first_refusal_wins(torch_mod, engines, entry):
    """calls with two faults: the one that is checked first is the one reported, and nothing is written"""
    from spart_amd import get_engine
    eng = engines["s2"]
    base, free, lo, hi, obs, w = make_case(torch_mod, eng, ["LAI", "Cab", "Cw"], 9, "R_TOC", "per_observation", 4)
    INVALID = -1
    bare = get_engine(None, 0).ctx
    for kw, want, text in [(dict(F=17, null=("free",)), INVALID, "F = 17, expected"),
                           (dict(M=-1, F=0), INVALID, "M = -1, expected"),
                           (dict(column=3, ctx=bare), INVALID, "column = 3"),
                           (dict(n_iter=101, null=("obs",)), INVALID, "n_iter = 101"),
                           (dict(M=0, null=("obs", "x", "cost", "ws")), 0, None),
                           (dict(null=("base[3]", "obs")), INVALID, "base[3] is null"),
                           (dict(null=("obs", "ws")), INVALID, "null argument (obs, x and cost are required)")]:
        rc, got = refine_call(torch_mod, eng, base, free, lo, hi, obs, w, entry=entry, **kw)
        msg = eng.lib.spart_last_error(eng.ctx).decode()
        assert rc == want and (text is None or msg.startswith(f"{entry}: {text}")), (kw, rc, msg)
        assert all((got[k] == FILL).all() for k in OUTS), kw


def test_refine_example_runs(tmp_path):
    """examples/refine.py as a user runs it: its own process, exit code 0, the expected last line"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine.py"), "20000", str(tmp_path / "lut")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "20000 rows" in r.stdout and "refined 4 parameters of 2048 spectra" in r.stdout
