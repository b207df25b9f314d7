"""Part 1 of csrc/spart_refine_leaf.h, built by g++ with -ffp-contract=off as the stand-alone program
tests/hostmath/refine_leaf_host.cpp, against the definition tools/refine_leaf_defined.py driven by the same build's leaf model
(the program's `spectra` mode): x, cost, cost0, std and n_accept must be the SAME BITS.  No GPU.  The cases run a second time
on a build under AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded)."""
import numpy as np
import pytest

from helpers import refine_leaf_calls as rl
from helpers.refine_leaf_calls import rld

M = 24
KEYS = ("x", "cost", "cost0", "std", "n_accept")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return str(tmp_path_factory.mktemp("refine_leaf_host"))


@pytest.fixture(scope="module")
def exe(work):
    path = work + "/refine_leaf_host"
    assert rl.build_harness(path) is None
    return path


@pytest.fixture(scope="module")
def exe_san(work):
    path = work + "/refine_leaf_host_san"
    why = rl.build_harness(path, sanitize=True)
    if why is not None:
        pytest.skip(f"g++ has no sanitizer runtime here: {why}")
    return path


@pytest.fixture(scope="module")
def raw(tables):
    return rl.raw_tables(tables)


@pytest.fixture(scope="module")
def forward(exe, work, raw):
    return lambda rows: rl.host_spectra(exe, work, raw, rows)


def make_case(F, kind, forward):
    """24 leaves, their noisy spectra as observations, starts away from the truth, and the edges of ``kind``"""
    rng = np.random.default_rng(100 * F + len(kind))
    truth = rl.leaves(M, seed=11)
    free, (lo, hi) = rl.free_cols(F), rl.bounds(F)
    refl, tran = forward(truth)
    obs_r = refl * (1 + 0.01 * rng.standard_normal(refl.shape))
    obs_t = tran * (1 + 0.01 * rng.standard_normal(tran.shape))
    start = truth.copy()
    start[:, free] = lo + (hi - lo) * rng.uniform(0.2, 0.8, (M, F))
    start[0, free[0]] = hi[0]                               # on the upper bound: a backward finite-difference step
    start[1, free[-1]] = lo[-1]                             # on the lower bound (N = 1 exactly where N is free)
    start[2, 6] = 1.0                                       # N = 1 exactly (a fixed N stays there; a free one starts there)
    start[3, free[0]] = hi[0] + 1.0                         # outside the box: the start is clipped
    case = dict(leaf=start, free=free, lo=lo, hi=hi, obs_refl=obs_r, obs_tran=obs_t, w_refl=None, w_tran=None)
    if kind == "edges":
        w_r, w_t = rng.uniform(0.5, 2.0, (M, rl.NWL)), rng.uniform(0.5, 2.0, (M, rl.NWL))
        obs_r, obs_t = obs_r.copy(), obs_t.copy()
        w_r[4, :50] = 0.0                                   # masks, the observations NaN under them
        obs_r[4, :50] = np.nan
        w_t[5, 1000:1100] = 0.0
        obs_t[5, 1000:1100] = np.nan
        w_r[6, 700] = -1.0                                  # a negative weight kills the leaf
        w_t[7, 2000] = np.nan
        w_r[8, 0] = np.inf
        for m, band in ((9, 2000), (10, 1984), (11, 63), (12, 64)):       # the tail pass and the lane wrap
            w_r[m], w_t[m] = 0.0, 0.0
            w_r[m, band] = 1.0
            obs_r[m, np.arange(rl.NWL) != band] = np.nan
        w_r[13], w_t[13] = 0.0, 0.0                         # nothing observed
        start[14, free[0]] = np.nan                         # a NaN parameter
        case.update(obs_refl=obs_r, obs_tran=obs_t, w_refl=w_r, w_tran=w_t)
    elif kind == "refl_only":
        w = rng.uniform(0.5, 2.0, rl.NWL)
        w[:50] = 0.0
        case.update(obs_tran=None, w_refl=w)
    elif kind == "tran_only":
        case.update(obs_refl=None)
    elif kind == "prior":
        mu = lo + (hi - lo) * rng.uniform(0.3, 0.7, (M, F))
        pw = 1.0 / (0.2 * (hi - lo)) ** 2 * np.ones((M, F))
        pw[:, 0] = 0.0                                      # no prior on the first name; its mean may be NaN
        mu[:, 0] = np.nan
        pw[5, F - 1] = -1.0                                 # a bad prior weight kills the leaf
        case.update(prior_mean=mu, prior_weight=pw)
    elif kind == "prior_shared":
        case.update(prior_mean=0.5 * (lo + hi), prior_weight=1.0 / (0.3 * (hi - lo)) ** 2)
    else:
        assert kind == "plain"
    return case


CASES = [("edges", 0), ("edges", 1), ("edges", 12), ("plain", 3), ("refl_only", 3), ("tran_only", 2), ("prior", 3), ("prior_shared", 2)]
_defined = {}


def defined_of(F, kind, n_iter, forward):
    """the definition's result of a case and its history, computed once for both builds"""
    key = (F, kind, n_iter)
    if key not in _defined:
        case, hist = make_case(F, kind, forward), []
        _defined[key] = (case, rld.refine_leaf_defined(forward=forward, n_iter=n_iter, history=hist, spectra=False, **case), hist)
    return _defined[key]


def check_case(binary, work, raw, forward, F, kind, n_iter):
    case, want, _ = defined_of(F, kind, n_iter, forward)
    got = rl.host_fit(binary, work, raw, n_iter=n_iter, **case)
    for k in KEYS:
        assert rl.same_bits(got[k], want[k]), (F, kind, n_iter, k, got[k], want[k])
    return case, want


@pytest.mark.parametrize("kind,n_iter", CASES)
@pytest.mark.parametrize("F", [1, 4, 7, 9])
def test_fit_is_the_definition_bit_for_bit(exe, work, raw, forward, F, kind, n_iter):
    case, want = check_case(exe, work, raw, forward, F, kind, n_iter)
    assert (want["cost"] <= want["cost0"])[want["n_accept"] >= 0].all()
    if kind == "edges":
        na = want["n_accept"]
        assert (na[[6, 7, 8, 14]] == -1).all() and np.isnan(want["std"][[6, 7, 8, 14]]).all()
        assert (na[[0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13]] >= 0).all()
        lo, hi = case["lo"], case["hi"]
        clipped = np.minimum(np.maximum(case["leaf"][[6, 7, 8]][:, case["free"]], lo), hi)
        assert np.array_equal(want["x"][[6, 7, 8]], clipped)
        assert np.isnan(want["std"][13]).all() and want["cost"][13] == 0.0                 # nothing observed, no prior
        if n_iter == 12:
            assert (na[:6] >= 1).all()                                                     # the fits do move


@pytest.mark.parametrize("F", [1, 4, 7, 9])
def test_prefix_property(exe, work, raw, forward, F):
    """n_iter = k is the state of a longer run after k decisions"""
    case, _, hist = defined_of(F, "edges", 12, forward)
    assert len(hist) == 13
    for k in (0, 1, 11):
        got = rl.host_fit(exe, work, raw, n_iter=k, **case)
        assert rl.same_bits(got["x"], hist[k][0]) and rl.same_bits(got["cost"], hist[k][1]), (F, k)


def test_spectra_mode_is_the_same_under_the_sanitizers(exe_san, work, raw, forward):
    rows = rl.leaves(7, seed=5)
    for a, b in zip(rl.host_spectra(exe_san, work, raw, rows), forward(rows)):
        assert rl.same_bits(a, b)


@pytest.mark.parametrize("kind,n_iter", CASES)
@pytest.mark.parametrize("F", [1, 4, 7, 9])
def test_fit_under_address_and_undefined_behaviour_sanitizers(exe_san, work, raw, forward, F, kind, n_iter):
    check_case(exe_san, work, raw, forward, F, kind, n_iter)
