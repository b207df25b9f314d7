"""The numpy definition of spart_lut_bayes_quantiles (tools/lut_bayes_defined.py) on its own, no GPU: the bracket property
against the exactly rounded sums, the exact rank values at omega = 1, monotony in q, the NaN rule, independence of the order
of the levels -- and the device kernel's search written out in numpy (quantile_search), which must return the same values."""
import math

import numpy as np
import pytest

from helpers.lut_bayes_calls import defined
from helpers.lut_bayes_quantile_calls import bracket_violations

B, NB, P, M, CUT = 3001, 7, 4, 24, 50.0
LEVELS = (0.05, 0.5, 0.95)


@pytest.fixture(scope="module")
def inputs():
    """float32 LUT of B rows, observations near rows of it, relative-noise weights whose noise level runs over the
    observations so that the sets within CUT run from a few rows to nearly all of them; the members, computed once"""
    rng = np.random.default_rng(11)
    lut = rng.uniform(0.0, 0.6, (B, NB)).astype(np.float32)
    params = rng.uniform(0.0, 8.0, (B, P))
    params[:, 3] = np.round(params[:, 3] * 2.0) / 2.0                       # a column of 17 distinct values: duplicates
    obs = (lut[rng.integers(0, B, M)] * (1 + 0.02 * rng.standard_normal((M, NB)))).astype(np.float32)
    rel = np.geomspace(0.03, 3.0, M)[:, None]
    w = (1.0 / (rel * np.abs(obs.astype(np.float64)) + 0.01) ** 2).astype(np.float32)
    members = defined.members_defined(lut, obs, w, CUT)
    sizes = [r.size for r, _, _, _ in members]
    print("set sizes", min(sizes), "...", max(sizes))
    assert min(sizes) <= 8 and max(sizes) >= 2500 and len({s for s in sizes if 8 < s < 2500}) >= 5       # (of the inputs)
    return lut, params, obs, w, members


def test_bracket_property_against_the_exact_sums(inputs):
    """(a) every (m, p, i): a value of the set, F_ex(v) >= q W (1 - g) and F_ex(u) < q W (1 + g) for the next smaller value u"""
    lut, params, obs, w, members = inputs
    got = defined.lut_bayes_quantiles_defined(lut, params, obs, w, LEVELS + (0.0, 1.0), CUT, members=members)
    assert got.shape == (M, P, 5) and not np.isnan(got).any()
    assert bracket_violations(members, params, got, LEVELS + (0.0, 1.0), CUT, 1.0) == []
    for m, (rows, _, _, _) in enumerate(members):                          # q = 0 and q = 1: minimum and maximum over S
        assert np.array_equal(got[m, :, 3], params[rows].min(axis=0)) and np.array_equal(got[m, :, 4], params[rows].max(axis=0))


def test_rank_values_at_unit_weights(inputs):
    """(b) all weights zero: omega = 1, every sum an exact integer, and a dyadic q gives sort(x)[max(ceil(q n) - 1, 0)]"""
    lut, params, obs, _, _ = inputs
    levels = (0.0, 0.25, 0.5, 0.75, 1.0)
    for rows in (slice(0, B), slice(0, 1), slice(0, 2), slice(5, 70), slice(100, 165)):      # n = 3001, 1, 2, 65, 65
        got = defined.lut_bayes_quantiles_defined(lut[rows], params[rows], obs[:2], np.zeros_like(obs[:2]), levels, CUT)
        x = np.sort(params[rows], axis=0)
        n = x.shape[0]
        want = np.stack([x[max(math.ceil(q * n) - 1, 0)] for q in levels], axis=1)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), n


def test_monotone_in_q(inputs):
    """(c) quantiles do not decrease with the level"""
    lut, params, obs, w, members = inputs
    levels = np.linspace(0.0, 1.0, 33)
    got = defined.lut_bayes_quantiles_defined(lut, params, obs, w, levels, CUT, members=members)
    assert (np.diff(got, axis=2) >= 0).all()


def test_nan_rule(inputs):
    """(d) a NaN in a column over S: every level of that (m, p) is NaN, nothing else changes; +-inf are ordinary values"""
    lut, params, obs, w, members = inputs
    clean = defined.lut_bayes_quantiles_defined(lut, params, obs, w, LEVELS, CUT, members=members)
    big = max(range(M), key=lambda m: members[m][0].size)
    par = params.copy()
    par[members[big][0][3], 1] = np.nan                                    # a row of the largest set, column 1
    par[members[big][0][5], 2] = np.inf
    par[members[big][0][6], 2] = -np.inf
    got = defined.lut_bayes_quantiles_defined(lut, par, obs, w, LEVELS + (0.0, 1.0), CUT, members=members)
    hit = np.array([np.isin(members[big][0][3], members[m][0]) for m in range(M)])
    assert hit[big] and np.isnan(got[hit, 1]).all() and not np.isnan(got[~hit]).any() and not np.isnan(got[:, [0, 2, 3]]).any()
    assert np.array_equal(got[:, 0, :3], clean[:, 0]) and np.array_equal(got[:, 3, :3], clean[:, 3])
    assert got[big, 2, 3] == -np.inf and got[big, 2, 4] == np.inf
    assert bracket_violations(members, par, got, LEVELS + (0.0, 1.0), CUT, 1.0) == []


def test_order_of_levels_does_not_matter(inputs):
    """(e) a level's result is the same wherever it stands in the list, and when it is repeated"""
    lut, params, obs, w, members = inputs
    a = defined.lut_bayes_quantiles_defined(lut, params, obs, w, (0.05, 0.5, 0.95), CUT, members=members)
    b = defined.lut_bayes_quantiles_defined(lut, params, obs, w, (0.95, 0.5, 0.5, 0.05), CUT, members=members)
    assert np.array_equal(a, b[:, :, [3, 1, 0]]) and np.array_equal(b[:, :, 1], b[:, :, 2])


def test_the_kernel_search_in_numpy_returns_the_definition(inputs):
    """quantile_search (pivot on the integer image, interval ends snapped to data values) = the definition, value for value,
    in at most 64 passes: on the random columns, on duplicates, constants, +-inf, denormals and signed zeros"""
    lut, params, obs, w, members = inputs
    levels = np.array(LEVELS + (0.0, 1.0, 0.25))
    worst = 0
    for m, (rows, e, _, _) in enumerate(members):
        om = np.exp(-(e / 2.0))
        got, passes = defined.quantile_search(params[rows], om, levels)
        assert np.array_equal(got, defined.quantiles_of_members(params[rows], om, levels)), m
        assert passes <= 64
        worst = max(worst, passes)
    print("passes over S: at most", worst)
    rng = np.random.default_rng(5)
    n = 300
    x = np.stack([np.full(n, 2.5), rng.integers(0, 3, n).astype(np.float64), rng.choice([-np.inf, -1.0, 0.0, -0.0, 5e-324, np.inf], n),
                  rng.standard_normal(n) * 1e-310, rng.standard_normal(n) * 1e300, np.where(rng.random(n) < 0.5, -0.0, 0.0)], axis=1)
    om = np.exp(-rng.uniform(0.0, 25.0, n))
    got, passes = defined.quantile_search(x, om, levels)
    want = defined.quantiles_of_members(x, om, levels)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)) and passes <= 64
    x[7, 4] = np.nan
    got, _ = defined.quantile_search(x, om, levels)
    assert np.isnan(got[4]).all() and np.array_equal(got[:4], want[:4]) and np.array_equal(got[5], want[5])
