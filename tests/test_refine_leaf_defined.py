"""tools/refine_leaf_defined.py with the oracle's PROSPECT as its forward model recovers leaves from their own noise-free
spectra, and every refusal of engine.refine_leaf_args is raised before a device is touched.  No GPU."""
import numpy as np
import pytest

from helpers import refine_leaf_calls as rl
from helpers.refine_leaf_calls import rld

M = 24


@pytest.fixture(scope="module")
def twin(oracle, tables):
    truth = rl.leaves(M, seed=11)
    forward = lambda rows: oracle.prospect_5d(rows, tables)[:2]      # noqa: E731
    refl, tran = forward(truth)
    return truth, forward, refl, tran


@pytest.mark.parametrize("F,both", [(4, True), (4, False), (7, True)])
def test_definition_recovers_leaves_from_their_own_spectra(twin, F, both):
    """Noise-free spectra have their minimum, cost 0, at the truth.  A fit counts as recovered when every parameter is within
    one finite-difference step of it, rel_step = 1e-3 of its range: the scale below which the difference quotient no longer
    tells two points apart, a bound set by the method and not by what this run gives."""
    truth, forward, refl, tran = twin
    free, (lo, hi) = rl.free_cols(F), rl.bounds(F)
    start = truth.copy()
    start[:, free] = 0.5 * (lo + hi)
    res = rld.refine_leaf_defined(start, free, lo, hi, refl, tran if both else None, forward, n_iter=30, spectra=True)
    err = np.abs(res["x"] - truth[:, free]) / (hi - lo)
    print("largest error / range per parameter:", err.max(axis=0), "accepted steps:", res["n_accept"].min(), "...", res["n_accept"].max())
    assert (res["n_accept"] >= 1).all() and (res["cost"] <= res["cost0"]).all()
    assert err.max() < 1e-3, err.max(axis=0)
    assert np.isfinite(res["std"]).all()
    assert np.abs(res["y_refl"] - refl).max() < 1e-3


def test_join_and_lane_layout():
    """by_pass puts band 64 k + l at [k, l]; join_defined is the tree d = 32 ... 1, not a running sum"""
    a = np.arange(2 * rld.NWL, dtype=np.float64).reshape(2, rld.NWL)
    p = rld.by_pass(a, -1.0)
    assert p.shape == (2, 32, 64) and p[1, 31, 16] == a[1, 2000] and p[0, 1, 0] == a[0, 64] and (p[:, 31, 17:] == -1.0).all()
    rng = np.random.default_rng(0)
    v = rng.standard_normal((3, 64)) * 10.0 ** rng.integers(-8, 8, (3, 64))
    want = v.copy()
    for d in (32, 16, 8, 4, 2, 1):
        for l in range(d):
            want[:, l] = want[:, l] + want[:, l + d]
    assert np.array_equal(rld.join_defined(v), want[:, 0])


def test_every_refusal_needs_no_device(monkeypatch):
    import spart_amd
    from spart_amd import engine

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(engine, "get_engine", no_device)
    monkeypatch.setattr(spart_amd.lut, "get_engine", no_device)
    leaf = rl.leaves(5, seed=2).T.copy()
    spec = np.full((5, 2001), 0.3)
    ok = dict(leaf=leaf, refl=spec, tran=spec, free=("Cab", "Cw"), bounds=None, weights_refl=None, weights_tran=None, n_iter=5,
              rel_step=1e-3, lambda0=1e-2, prior=None, prior_mean=None, prior_weight=None)
    plan, _, M_, wper, pm, pw, per = engine.refine_leaf_args(**ok)
    assert M_ == 5 and wper == 0 and pm is None and plan["names"] == ["Cab", "Cw"] and list(plan["cols"]) == [0, 2]
    assert engine.refine_leaf_args(**dict(ok, weights_refl=spec))[3] == 1
    assert engine.refine_leaf_args(**dict(ok, tran=None, weights_refl=spec[0]))[3] == 0
    bad = [dict(free=("Cab", "LAI")), dict(free=()), dict(free=("Cab", "Cab")), dict(free=("Cab",), bounds={"Cw": (0, 1)}),
           dict(bounds={"Cab": (5.0, 5.0)}), dict(bounds={"Cab": (0.0, np.inf)}), dict(n_iter=101), dict(n_iter=-1), dict(n_iter=2.5),
           dict(rel_step=0.0), dict(rel_step=np.nan), dict(lambda0=-1.0), dict(lambda0=np.inf),
           dict(refl=None, tran=None), dict(refl=spec[:, :2000]), dict(refl=spec[0]), dict(tran=spec[:4]),
           dict(tran=None, weights_tran=spec), dict(refl=None, weights_refl=spec[0]), dict(weights_refl=spec[:4]),
           dict(weights_tran=spec[:, :13]), dict(leaf=leaf[:8]), dict(leaf=list(leaf[:8])), dict(leaf=leaf[:, :4]),
           dict(leaf=[None] + list(leaf[1:])), dict(prior={"N": (1.5, 0.2)}), dict(prior={"Cab": (40.0, -1.0)}),
           dict(prior={"Cab": (40.0, 5.0)}, prior_mean=np.zeros(2), prior_weight=np.ones(2)),
           dict(prior_mean=np.zeros(2)), dict(prior_mean=np.zeros(3), prior_weight=np.ones(3)),
           dict(prior_mean=np.zeros((4, 2)), prior_weight=np.ones((4, 2)))]
    for change in bad:
        with pytest.raises(ValueError):
            engine.refine_leaf_args(**dict(ok, **change))
        with pytest.raises(ValueError):                    # ... and the host form stops at the same check
            kw = dict(ok, **change)
            spart_amd.refine_leaf(kw.pop("leaf"), kw.pop("refl"), kw.pop("tran"), **kw)
