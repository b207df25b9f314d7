"""spart_refine_leaf / Engine.refine_leaf / spart_amd.refine_leaf on the MI355X: PROSPECT inversion of leaf spectra.

The kernel evaluates the leaf model with the device's float64 arithmetic, so its fits are not the bits of a numpy run of the
definition (tools/refine_leaf_defined.py); part 1 of the kernel's header is pinned to the definition bit for bit on the CPU
(tests/test_refine_leaf_host.py).  Here the spectra are held to the oracle at the project's float64 bar, the sums to the
definition at tolerances derived where they are used, and everything that is a property of the call -- position
independence, masks, dead leaves, refusals -- is bit for bit.

Measured on one MI355X (the tests print the figures again):
test_std_at_the_start_within_the_references_own_gap and test_recovery_within_four_times_the_references_error."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers import refine_leaf_calls as rl
from helpers.lut_calls import eng, torch_mod  # noqa: F401  (fixtures; eng is a context WITHOUT a sensor)
from helpers.refine_leaf_calls import rld

pytestmark = pytest.mark.gpu
NWL = rl.NWL
TOL64 = 4e-9              # the project's float64 bar on |x - ref| / max(|ref|, 1e-6)
KEYS = ("x", "cost", "cost0", "std", "n_accept", "y_refl", "y_tran")
FILL = -7.0


def host(res):
    return {k: (v if k == "names" else v.cpu().numpy()) for k, v in res.items()}


def fit(eng, leaf, refl, tran, F, **kw):
    """Engine.refine_leaf on (M, 9) rows with the cases' free names and bounds -> numpy dict, spectra included"""
    return host(eng.refine_leaf(np.ascontiguousarray(leaf.T), refl, tran, free=rl.FREE[F], spectra=True, **kw))


def same(a, b, keys=KEYS, rows=slice(None)):
    return all(rl.same_bits(a[k][rows], b[k]) for k in keys)


@pytest.fixture(scope="module")
def fwd_engine(eng):
    def forward(rows):
        r = eng.prospect(list(np.ascontiguousarray(np.asarray(rows, dtype=np.float64).T)), outputs=("refl", "tran"))
        return r[0].cpu().numpy(), r[1].cpu().numpy()
    return forward


@pytest.fixture(scope="module")
def fwd_oracle(oracle, tables):
    return lambda rows: oracle.prospect_5d(rows, tables)[:2]


@pytest.fixture(scope="module")
def batch(fwd_engine):
    """130 leaves; their observations are the spectra of OTHER leaves with 1 % noise (a fit has somewhere to go and
    the residual is large); starts at the middle of the ranges of the seven PROSPECT-5D parameters"""
    rng = np.random.default_rng(7)
    truth = rl.leaves(130, seed=21)
    refl, tran = fwd_engine(truth[::-1])
    obs_r = refl * (1 + 0.01 * rng.standard_normal(refl.shape))
    obs_t = tran * (1 + 0.01 * rng.standard_normal(tran.shape))
    return truth, obs_r, obs_t


# ---- 3
def test_spectra_at_x_against_the_oracle(eng, batch, oracle, tables):
    leaf, obs_r, obs_t = (a[:33] for a in batch)
    res = fit(eng, leaf, obs_r, obs_t, 4, n_iter=5)
    rows = leaf.copy()
    rows[:, rl.free_cols(4)] = res["x"]
    refl, tran, _ = oracle.prospect_5d(rows, tables)
    for got, ref in ((res["y_refl"], refl), (res["y_tran"], tran)):
        err = np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6))
        print("y against the oracle:", err)
        assert np.isfinite(got).all() and err <= TOL64


# ---- 4
def test_start_cost_against_the_definition_driven_by_the_oracle(eng, batch, fwd_oracle):
    """Spectra within 4e-9 (relative, of values below 1) move c = sum w d^2 by |dc| / c <= 2 * 4e-9 / rms(d): with
    rms(d) >= 0.01, asserted here on the test's own inputs, that is 8e-7 < 1e-6."""
    leaf, obs_r, obs_t = (a[:40] for a in batch)
    for F in (1, 4, 7, 9):
        lo, hi = rl.bounds(F)
        res = fit(eng, leaf, obs_r, obs_t, F, n_iter=0)
        want = rld.refine_leaf_defined(leaf, rl.free_cols(F), lo, hi, obs_r, obs_t, fwd_oracle, n_iter=0)
        rms = np.sqrt(np.mean(np.concatenate([want["y_refl"] - obs_r, want["y_tran"] - obs_t], axis=1) ** 2, axis=1))
        assert rms.min() >= 0.01, rms.min()
        err = np.max(np.abs(res["cost0"] - want["cost0"]) / want["cost0"])
        print(f"F = {F}: cost0 against the definition, relative {err:.2e}; smallest rms residual {rms.min():.3f}")
        assert err <= 1e-6
        assert np.array_equal(res["cost"], res["cost0"]) and (res["n_accept"] == 0).all()


# ---- 5
def test_std_at_the_start_within_the_references_own_gap(eng, batch, fwd_engine, fwd_oracle):
    """std comes from difference quotients, which amplify the forward model's error.  Its tolerance is the gap between two
    references, neither of them under test: the definition driven by Engine.prospect and the definition driven by the
    oracle.  The kernel must lie within that gap of the Engine.prospect-driven result, per parameter, with no further margin.
    Measured on one MI355X, F = 4 (Cab, Cw, Cdm, N): see DESIGN.md section 21."""
    leaf, obs_r, obs_t = (a[:24] for a in batch)
    F = 4
    lo, hi = rl.bounds(F)
    res = fit(eng, leaf, obs_r, obs_t, F, n_iter=0)
    ref_e = rld.refine_leaf_defined(leaf, rl.free_cols(F), lo, hi, obs_r, obs_t, fwd_engine, n_iter=0, spectra=False)
    ref_o = rld.refine_leaf_defined(leaf, rl.free_cols(F), lo, hi, obs_r, obs_t, fwd_oracle, n_iter=0, spectra=False)
    assert np.isfinite(res["std"]).all() and np.isfinite(ref_e["std"]).all() and np.isfinite(ref_o["std"]).all()
    gap = np.max(np.abs(ref_e["std"] - ref_o["std"]) / ref_e["std"], axis=0)
    got = np.max(np.abs(res["std"] - ref_e["std"]) / ref_e["std"], axis=0)
    print("std, references' mutual difference per parameter:", gap)
    print("std, kernel against the Engine.prospect-driven definition:", got)
    assert (got <= gap).all(), (got, gap)


# ---- 6
@pytest.mark.parametrize("F", [4, 7])
def test_recovery_within_four_times_the_references_error(eng, fwd_engine, fwd_oracle, F):
    """64 leaves, observations from Engine.prospect, starts at the middle of the ranges, n_iter = 30.  The bar, per
    parameter, is 4 x the larger error of the two reference runs of the definition on the same observations (forward =
    Engine.prospect and forward = the oracle); the factor allows for another accept / reject path.  Every leaf counts.
    Measured on one MI355X: see DESIGN.md section 21."""
    truth = rl.leaves(64, seed=3)
    obs_r, obs_t = fwd_engine(truth)
    free, (lo, hi) = rl.free_cols(F), rl.bounds(F)
    start = truth.copy()
    start[:, free] = 0.5 * (lo + hi)
    res = fit(eng, start, obs_r, obs_t, F, n_iter=30)
    refs = [rld.refine_leaf_defined(start, free, lo, hi, obs_r, obs_t, fwd, n_iter=30, spectra=False) for fwd in (fwd_engine, fwd_oracle)]
    err = np.abs(res["x"] - truth[:, free]) / (hi - lo)
    err_e, err_o = (np.abs(r["x"] - truth[:, free]) / (hi - lo) for r in refs)
    print(f"F = {F}: largest error / range per parameter, kernel:", err.max(axis=0))
    print(f"F = {F}: definition driven by Engine.prospect:", err_e.max(axis=0))
    print(f"F = {F}: definition driven by the oracle:", err_o.max(axis=0))
    bar = 4.0 * np.maximum(err_e.max(axis=0), err_o.max(axis=0))
    assert (res["n_accept"] >= 1).all()
    assert (err <= bar[None, :]).all(), (err.max(axis=0), bar)


# ---- 7
def test_position_independence_bit_for_bit(eng, batch):
    leaf, obs_r, obs_t = batch
    rng = np.random.default_rng(1)
    w_r = rng.uniform(0.5, 2.0, obs_r.shape)
    kw = dict(n_iter=6, weights_refl=w_r)
    full = fit(eng, leaf, obs_r, obs_t, 4, **kw)
    assert same(fit(eng, leaf, obs_r, obs_t, 4, **kw), full)                               # two runs
    for p in (0, 63, 64, 129):
        one = fit(eng, leaf[p:p + 1], obs_r[p:p + 1], obs_t[p:p + 1], 4, n_iter=6, weights_refl=w_r[p:p + 1])
        assert same(full, one, rows=slice(p, p + 1)), p
    for M in (63, 64, 65):
        part = fit(eng, leaf[:M], obs_r[:M], obs_t[:M], 4, n_iter=6, weights_refl=w_r[:M])
        assert same(full, part, rows=slice(0, M)), M
    assert (full["n_accept"] >= 1).all() and np.isfinite(full["x"]).all()


# ---- 8
def test_masks_and_absent_arrays(eng, batch):
    leaf, obs_r, obs_t = (a[:20] for a in batch)
    rng = np.random.default_rng(2)
    w_r, w_t = rng.uniform(0.5, 2.0, obs_r.shape), rng.uniform(0.5, 2.0, obs_t.shape)
    w_r[:, :50] = 0.0
    w_t[::2, 1000:1200] = 0.0
    nan_r, nan_t = obs_r.copy(), obs_t.copy()
    nan_r[w_r == 0.0] = np.nan
    nan_t[w_t == 0.0] = np.nan
    kw = dict(n_iter=5, weights_refl=w_r, weights_tran=w_t)
    ref = fit(eng, leaf, obs_r, obs_t, 4, **kw)
    assert same(fit(eng, leaf, nan_r, nan_t, 4, **kw), ref)                                # NaN under weight 0
    assert np.isfinite(ref["x"]).all() and (ref["n_accept"] >= 1).all()
    # no transmittance at all == every transmittance weight zero
    a = fit(eng, leaf, obs_r, None, 4, n_iter=5, weights_refl=w_r)
    b = fit(eng, leaf, obs_r, obs_t, 4, n_iter=5, weights_refl=w_r, weights_tran=np.zeros_like(w_t))
    assert same(a, b)
    c = fit(eng, leaf, None, obs_t, 4, n_iter=5, weights_tran=w_t[0])                      # ... and the other way, shared weights
    d = fit(eng, leaf, obs_r, obs_t, 4, n_iter=5, weights_refl=np.zeros(NWL), weights_tran=w_t[0])
    assert same(c, d)
    # one band only: the tail pass (2000: lane 16 of pass 31) and its first lane (1984).  In-loop Y_0 and the closing y are two
    # evaluations of one row, each within 4e-9 of the model: |d cost0| / cost0 <= 2 * 8e-9 * |y| / |d| <= 3.2e-7 at |d| = 0.05
    for band in (2000, 1984):
        w1 = np.zeros(NWL)
        w1[band] = 3.0
        at0 = fit(eng, leaf, obs_r, None, 4, n_iter=0, weights_refl=w1)
        shifted = nan_r.copy()
        shifted[:, band] = at0["y_refl"][:, band] + 0.05
        one = fit(eng, leaf, shifted, None, 4, n_iter=4, weights_refl=w1)
        assert np.isfinite(one["x"]).all() and np.isfinite(one["cost"]).all() and np.isfinite(one["y_refl"]).all()
        start = fit(eng, leaf, shifted, None, 4, n_iter=0, weights_refl=w1)
        d0 = start["y_refl"][:, band] - shifted[:, band]
        assert np.allclose(start["cost0"], (3.0 * d0) * d0, rtol=3.2e-7, atol=0.0), band
        assert np.array_equal(one["cost0"], start["cost0"])
        assert (one["cost"] <= one["cost0"]).all()


# ---- 9
def test_dead_and_degenerate_leaves(eng, batch):
    leaf, obs_r, obs_t = (a[:12].copy() for a in batch)
    F, free = 4, rl.free_cols(4)
    lo, hi = rl.bounds(F)
    leaf[1, free[0]] = hi[0] + 5.0                                                         # a start outside the box
    w_r, w_t = np.ones_like(obs_r), np.ones_like(obs_t)
    ref = fit(eng, leaf, obs_r, obs_t, F, n_iter=4, weights_refl=w_r, weights_tran=w_t)
    w_r2, w_t2 = w_r.copy(), w_t.copy()
    w_r2[1, 300], w_t2[4, 2000], w_r2[7, 0] = -1.0, np.nan, np.inf
    res = fit(eng, leaf, obs_r, obs_t, F, n_iter=4, weights_refl=w_r2, weights_tran=w_t2)
    dead = [1, 4, 7]
    alive = [m for m in range(12) if m not in dead]
    assert (res["n_accept"][dead] == -1).all() and np.isnan(res["std"][dead]).all()
    clipped = np.minimum(np.maximum(leaf[dead][:, free], lo), hi)
    assert np.array_equal(res["x"][dead], clipped)
    for k in KEYS:
        assert rl.same_bits(res[k][alive], ref[k][alive]), k                               # the neighbours are untouched
    # nothing observed and no prior: nowhere to go
    none = fit(eng, leaf, obs_r, obs_t, F, n_iter=3, weights_refl=np.zeros(NWL), weights_tran=np.zeros(NWL))
    assert np.isnan(none["std"]).all() and np.array_equal(none["x"], np.minimum(np.maximum(leaf[:, free], lo), hi))
    assert (none["cost"] == 0.0).all() and (none["n_accept"] == 0).all()
    # ... with a prior there is
    mu, pw = 0.5 * (lo + hi), 1.0 / (0.1 * (hi - lo)) ** 2
    pri = fit(eng, leaf, obs_r, obs_t, F, n_iter=6, weights_refl=np.zeros(NWL), weights_tran=np.zeros(NWL), prior_mean=mu, prior_weight=pw)
    assert np.isfinite(pri["std"]).all() and np.allclose(pri["x"], mu[None, :], rtol=1e-9)
    # a NaN parameter makes only its own row NaN
    bad = leaf.copy()
    bad[3, free[1]] = np.nan
    bad[5, 3] = np.nan                                                                     # (Cs: not free)
    nanres = fit(eng, bad, obs_r, obs_t, F, n_iter=4, weights_refl=w_r, weights_tran=w_t)
    assert (nanres["n_accept"][[3, 5]] == -1).all() and np.isnan(nanres["cost"][[3, 5]]).all() and np.isnan(nanres["x"][3, 1])
    keep = [m for m in range(12) if m not in (3, 5)]
    for k in KEYS:
        assert rl.same_bits(nanres[k][keep], ref[k][keep]), k


# ---- 10
def test_cost_never_rises(eng, batch):
    leaf, obs_r, obs_t = (a[:32] for a in batch)
    for F in (1, 9):
        last = None
        for n in (0, 1, 2, 5, 12):
            r = fit(eng, leaf, obs_r, obs_t, F, n_iter=n)
            assert (r["cost"] <= r["cost0"]).all() and np.isfinite(r["x"]).all() and r["x"].shape == (32, F)
            assert last is None or ((r["cost"] <= last["cost"]).all() and np.array_equal(r["cost0"], last["cost0"]))
            last = r
        assert (last["n_accept"] >= 1).all() and (last["cost"] < last["cost0"]).all()
        lo, hi = rl.bounds(F)
        assert ((last["x"] >= lo) & (last["x"] <= hi)).all()


def test_host_form_and_leafbiology(eng, batch):
    import spart_amd
    leaf, obs_r, obs_t = (a[:9] for a in batch)
    want = fit(eng, leaf, obs_r, obs_t, 4, n_iter=3)
    got = spart_amd.refine_leaf(spart_amd.LeafBiology(*[leaf[:, k] for k in range(9)]), obs_r, obs_t, free=rl.FREE[4], n_iter=3,
                                spectra=True)
    assert got["names"] == rl.FREE[4] and same(got, want)
    assert set(spart_amd.refine_leaf(leaf.T, obs_r, None, n_iter=1)) == {"x", "std", "cost", "cost0", "n_accept", "names"}


def raw_call(torch, eng, M=5, F=2, **over):
    """One spart_refine_leaf through ctypes with every argument valid unless ``over`` replaces it; the arrays hold 5 rows
    whatever M is passed -> (rc, message, buffers)"""
    from spart_amd import _lib
    dev, n = "cuda:0", 5
    leaf = torch.as_tensor(rl.leaves(n, seed=4).T.copy(), device=dev)
    spec = torch.full((n, NWL), 0.3, dtype=torch.float64, device=dev)
    bufs = {k: torch.full((n * (NWL if k.startswith("y") else F if k in ("x", "std") else 1) + 8,), FILL,
                          dtype=torch.float64, device=dev) for k in _lib.LEAF_FIT_OUTS}
    a = dict(ctx=eng.ctx, M=M, leaf=[leaf[k].data_ptr() for k in range(9)], F=F, free=[0, 2, 6, 1, 3, 4, 5, 7, 8][:F], lo=[1.0] * F,
             hi=[2.0] * F, obs_r=spec.data_ptr(), obs_t=spec.data_ptr(), w_r=None, w_t=None,
             opt=dict(n_iter=2, weights_per_obs=0, rel_step=0.0, lambda0=0.0, prior_per_obs=0, prior_mean=None, prior_weight=None),
             out={k: bufs[k].data_ptr() for k in _lib.LEAF_FIT_OUTS})
    for k, v in over.items():
        if k in ("opt", "out") and isinstance(v, dict):
            a[k] = dict(a[k], **v)
        else:
            a[k] = v

    def arr(v, ct):
        return None if v is None else (ct * len(v))(*v)
    opt = None if a["opt"] is None else _lib.SpartLeafFitOpt(**a["opt"])
    out = None if a["out"] is None else _lib.SpartLeafFitOut(**a["out"])
    rc = eng.lib.spart_refine_leaf(a["ctx"], a["M"], None if a["leaf"] is None else (_lib.vp * 9)(*a["leaf"]), a["F"],
                                   arr(a["free"], ctypes.c_int32), arr(a["lo"], ctypes.c_double), arr(a["hi"], ctypes.c_double),
                                   a["obs_r"], a["obs_t"], a["w_r"], a["w_t"], None if opt is None else ctypes.byref(opt),
                                   None if out is None else ctypes.byref(out), None)
    torch.cuda.synchronize()
    msg = eng.lib.spart_last_error(eng.ctx)
    return rc, (msg or b"").decode(), bufs, spec


def test_the_c_call_refuses_with_nothing_written(torch_mod, eng):
    torch = torch_mod
    rc, _, bufs, _ = raw_call(torch, eng)
    assert rc == 0 and (bufs["x"][:10] != FILL).all() and (bufs["x"][10:] == FILL).all() and (bufs["y_tran"][5 * NWL:] == FILL).all()
    rc, _, bufs, _ = raw_call(torch, eng, M=0, leaf=None)                                  # M = 0 launches nothing
    assert rc == 0 and all((b == FILL).all() for b in bufs.values())
    w = torch.ones(NWL, dtype=torch.float64, device="cuda:0").data_ptr()
    refusals = [dict(ctx=None), dict(F=0), dict(F=10, free=list(range(9)) + [0], lo=[1.0] * 10, hi=[2.0] * 10), dict(free=None),
                dict(lo=None), dict(hi=None), dict(free=[0, 9]), dict(free=[-1, 2]), dict(free=[2, 2]), dict(lo=[1.0, 2.0]),
                dict(hi=[2.0, float("inf")]), dict(lo=[float("nan"), 1.0]), dict(opt=None), dict(opt=dict(n_iter=-1)),
                dict(opt=dict(n_iter=101)), dict(opt=dict(rel_step=-1e-3)), dict(opt=dict(rel_step=float("inf"))),
                dict(opt=dict(lambda0=float("nan"))), dict(opt=dict(weights_per_obs=2)), dict(opt=dict(prior_mean=w)),
                dict(opt=dict(prior_weight=w)), dict(opt=dict(prior_per_obs=2)), dict(obs_r=None, obs_t=None),
                dict(obs_r=None, w_r=w), dict(obs_t=None, w_t=w), dict(out=None), dict(out=dict(x=None)), dict(out=dict(cost=None)),
                dict(M=-1), dict(M=3_000_000_000), dict(leaf=None)]
    for over in refusals:
        rc, msg, bufs, _ = raw_call(torch, eng, **over)
        assert rc == -1 and "spart_refine_leaf" in msg, (over, rc, msg)
        assert all((b == FILL).all() for b in bufs.values()), over
    leaf = torch.as_tensor(rl.leaves(5, seed=4).T.copy(), device="cuda:0")
    ptrs = [leaf[k].data_ptr() for k in range(9)]
    ptrs[3] = None
    ptrs[6] = None                                                                         # a NULL leaf column: the first is named
    rc, msg, bufs, _ = raw_call(torch, eng, leaf=ptrs)
    assert rc == -1 and "leaf[3]" in msg and all((b == FILL).all() for b in bufs.values())
    # the order of the list: of two faults the earlier one is reported
    rc, msg, _, _ = raw_call(torch, eng, F=0, opt=None)
    assert rc == -1 and "F = 0" in msg
    rc, msg, _, _ = raw_call(torch, eng, opt=dict(n_iter=200), obs_r=None, obs_t=None)
    assert rc == -1 and "n_iter" in msg
    rc, msg, _, _ = raw_call(torch, eng, out=None, M=-5)
    assert rc == -1 and "out" in msg


# ---- 11
def test_example_runs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "refine_leaf.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "Cab" in p.stdout and "reflectance alone" in p.stdout
