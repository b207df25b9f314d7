"""helpers/srf_exact.py without a GPU: srf_chain (std::fma chains, tests/hostmath/srf_chain.cpp) against exact rational
arithmetic, against srf_numpy.convolve on the packaged sensors, and the supports of the probe and dealing sensors that
tests/test_gpu_srf_sums.py runs."""
from fractions import Fraction
import math

import numpy as np
import pytest

from helpers import srf_exact as E
from helpers import srf_numpy
from test_srf_support_host import assert_support_equal, library_support, lib  # noqa: F401  (lib: the fixture)

SENSORS = ["TerraAqua-MODIS", "LANDSAT4-TM", "LANDSAT5-TM", "LANDSAT7-ETM", "LANDSAT8-OLI", "Sentinel2A-MSI", "Sentinel2B-MSI",
           "Sentinel3A-OLCI", "Sentinel3B-OLCI"]


def exact_fma(q, x, acc):
    """fma(q, x, acc) correctly rounded: Fraction arithmetic, float() of a Fraction rounds to nearest even; the IEEE rules
    for non-finite operands, overflow and the sign of an exact zero written out"""
    if math.isnan(q) or math.isnan(x) or math.isnan(acc):
        return math.nan
    if math.isinf(q) or math.isinf(x):
        if q == 0 or x == 0:
            return math.nan
        prod = math.copysign(math.inf, q) * math.copysign(1.0, x)
        return math.nan if (math.isinf(acc) and acc != prod) else prod
    if math.isinf(acc):
        return acc                                         # (a finite exact product, however large)
    r = Fraction(q) * Fraction(x) + Fraction(acc)
    if r == 0:
        if (q == 0 or x == 0) and acc == 0:                # zero + zero: the common sign, else +0
            sp = math.copysign(1.0, q) * math.copysign(1.0, x)
            return acc if math.copysign(1.0, acc) == sp else 0.0
        return 0.0                                         # exact cancellation rounds to +0
    try:
        return float(r)
    except OverflowError:
        return math.inf if r > 0 else -math.inf


def exact_chain(q, x, Q):
    acc = 0.0
    for qe, xe in zip(q, x):
        acc = exact_fma(float(qe), float(xe), acc)
    with np.errstate(all="ignore"):
        return float(np.float64(acc) / np.float64(Q))      # one IEEE division (numpy's: x / 0 and 0 / 0 included)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def one_band(q, x, Q):
    n = len(q)
    lists = (np.array([0, n], np.int32), np.arange(n, dtype=np.int32), np.asarray(q, np.float64), np.array([Q], np.float64))
    return E.srf_chain(np.asarray(x, np.float64)[None, :], lists)


def test_exact_fma_reference_is_not_the_unfused_form():
    """the rational reference tells a fused accumulate from a rounded product: 3 * (1/3) - 1"""
    third = 1.0 / 3.0
    assert exact_fma(3.0, third, -1.0) == -2.0 ** -54 and 3.0 * third - 1.0 == 0.0
    assert math.copysign(1.0, exact_fma(-1.0, 0.0, 0.0)) == 1.0 and math.copysign(1.0, exact_fma(-1.0, 0.0, -0.0)) == -1.0


def test_random_chains_equal_exact_arithmetic():
    """3000 chains (1000 supports of length 1 ... 400 on three rows), mixed signs and magnitudes over six decades"""
    rng = np.random.default_rng(21)
    nb, B = 1000, 3
    n = rng.integers(1, 401, nb)
    n[:4] = [1, 2, 399, 400]
    start = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    ev = np.concatenate([np.sort(rng.choice(E.NEV, k, replace=False)) for k in n]).astype(np.int32)
    mag = lambda size: rng.uniform(-1.0, 1.0, size) * 10.0 ** rng.uniform(-3.0, 3.0, size)
    q, X = mag(ev.size), mag((B, E.NEV))
    Q = np.array([q[a:b].sum() for a, b in zip(start[:-1], start[1:])])
    out, S, nn = E.srf_chain(X, (start, ev, q, Q))
    assert np.array_equal(nn, n) and out.shape == S.shape == (B, nb)
    want = np.array([[exact_chain(q[a:b], X[s, ev[a:b]], Q[j]) for j, (a, b) in enumerate(zip(start[:-1], start[1:]))]
                     for s in range(B)])
    assert same_bits(out, want), np.argwhere(out != want)[:5]
    Sw = np.array([[np.sum(np.abs(q[a:b]) * np.abs(X[s, ev[a:b]])) / abs(Q[j]) for j, (a, b) in enumerate(zip(start[:-1], start[1:]))]
                   for s in range(B)])
    assert np.allclose(S, Sw, rtol=1e-12, atol=0.0)
    # (the chains are not trivially equal to a rounded multiply-add: a fair share differs in bits)
    plain = np.array([[np.add.accumulate(np.concatenate([[0.0], q[a:b] * X[s, ev[a:b]]]))[-1] / Q[j]
                       for j, (a, b) in enumerate(zip(start[:-1], start[1:]))] for s in range(B)])
    assert (plain != out).mean() > 0.3


HOSTILE = {
    "cancelling": ([1.0, -1.0, 1e-30], [1 / 3, 1 / 3, 1.0], 1e-30),
    "cancelling_residual": ([-1.0, 3.0], [1.0, 1 / 3], 2.0),               # -2^-54 / 2 fused, 0 unfused
    "cancelling_long": ([1e16, 1.0, -1e16, 1.0] * 25, [0.1, 0.3, 0.1, 0.7] * 25, 50.0),
    "subnormal_q": ([5e-324, 2.5e-308, -5e-324], [0.7, 0.3, 0.2], 1e-308),
    "subnormal_result": ([1e-200], [1e-120], 4.0),
    "overflow": ([1e200], [1e200], 1.0),
    "overflow_both_ways": ([1e200, -1e200], [1e200, 1e200], 1.0),          # inf - 1e400 = inf: a fused product does not overflow
    "overflow_negative": ([-1e308, 1.0], [10.0, 1.0], 3.0),
    "huge_but_finite": ([-1e308, 1e308], [1.0, 1.9], 1e300),               # 9e307: the rounded product 1.9e308 would overflow
    "zero_against_inf": ([0.0, 1.0], [np.inf, 1.0], 1.0),
    "zero_against_nan": ([0.0, 1.0], [np.nan, 1.0], 1.0),
    "negative_zero_against_inf": ([-0.0, 1.0], [-np.inf, 1.0], 1.0),
    "inf_value": ([0.5, 0.5], [np.inf, 1.0], 1.0),
    "inf_values_cancel": ([0.5, 0.5], [np.inf, -np.inf], 1.0),
    "inf_weight": ([np.inf, 1.0], [0.5, 1.0], np.inf),
    "nan_weight": ([np.nan, 1.0], [0.5, 1.0], np.nan),
    "Q_zero_plus": ([1.0, -1.0], [0.3, 0.2], 0.0),
    "Q_zero_minus": ([1.0, -1.0], [0.2, 0.3], 0.0),
    "Q_zero_nan": ([1.0, -1.0], [0.3, 0.3], 0.0),
    "Q_negative_zero": ([1.0, -1.0], [0.3, 0.2], -0.0),
    "Q_negative": ([-1.0, -2.0], [0.25, 0.4], -3.0),
    "signed_zero": ([-1.0], [0.0], 1.0),
    "signed_zero_pair": ([1.0, -1.0], [-0.0, 0.0], -1.0),
}


@pytest.mark.parametrize("name", sorted(HOSTILE))
def test_hostile_chains_equal_exact_arithmetic(name):
    q, x, Q = HOSTILE[name]
    out, S, n = one_band(q, x, Q)
    want = exact_chain(q, x, Q)
    assert out.shape == (1, 1) and n[0] == len(q)
    assert same_bits(out[0, 0], want), (name, out[0, 0], want)


def test_hostile_chains_have_the_values_they_are_named_for():
    v = {k: one_band(*HOSTILE[k])[0][0, 0] for k in HOSTILE}
    assert v["cancelling_residual"] == -2.0 ** -55 and v["overflow"] == np.inf and v["overflow_negative"] == -np.inf
    assert abs(v["huge_but_finite"] / 9e7 - 1.0) < 1e-15 and np.isfinite(v["subnormal_q"]) and 0 < v["subnormal_result"] < 2.3e-308
    for k in ("zero_against_inf", "zero_against_nan", "negative_zero_against_inf", "inf_values_cancel",
              "inf_weight", "nan_weight", "Q_zero_nan"):
        assert np.isnan(v[k]), k
    assert v["overflow_both_ways"] == np.inf and v["inf_value"] == np.inf and v["Q_zero_plus"] == np.inf and v["Q_zero_minus"] == -np.inf and v["Q_negative_zero"] == -np.inf
    assert v["Q_negative"] == (-0.25 - 0.8) / -3.0 and v["cancelling"] == 1.0
    assert v["signed_zero"] == 0.0 and not np.signbit(v["signed_zero"]) and np.signbit(v["signed_zero_pair"])


@pytest.mark.parametrize("sensor", SENSORS)
def test_chain_against_numpy_convolution(sensor):
    """the FMA chain over srf_numpy.support against srf_numpy.convolve (numpy's multiply, then add, in the same order):
    |difference| <= (n_j + 1) 2^-53 S per element"""
    from spart_amd import tables
    si = tables.load_sensor_info(sensor)
    rng = np.random.default_rng(31)
    x = rng.uniform(0.0, 0.6, (5, srf_numpy.NWLS))
    x[:, srf_numpy.NWL:] = x[:, srf_numpy.NWL:srf_numpy.NWL + 1]          # the thermal pad holds one value
    lists = srf_numpy.support(si["wl_srf_smac"], si["p_srf_smac"])
    out, S, n = E.srf_chain(x[:, :E.NEV], lists)
    ref = srf_numpy.convolve(x, si["wl_srf_smac"], si["p_srf_smac"], lists=lists)
    assert np.isfinite(out).all() and np.isfinite(ref).all()
    excess = np.abs(out - ref) / E.chain_bound(S, n)
    print(sensor, "worst |chain - numpy| / bound: %.3f" % excess.max(), "n_j", int(n.min()), "...", int(n.max()))
    assert excess.max() <= 1.0, (sensor, np.unravel_index(np.argmax(excess), excess.shape))


def test_probe_support_is_the_identity(lib):
    si = E.probe_sensor()
    start, ev, q, Q = lists = srf_numpy.support(si["wl_srf_smac"], si["p_srf_smac"])
    assert np.array_equal(start, np.arange(E.NEV + 1)) and np.array_equal(ev, np.arange(E.NEV))
    assert np.array_equal(q, np.ones(E.NEV)) and np.array_equal(Q, np.ones(E.NEV))
    assert_support_equal(library_support(lib, si["wl_srf_smac"], si["p_srf_smac"]), lists)
    X = np.random.default_rng(5).standard_normal((3, E.NEV))
    X[0, 7], X[1, 9] = np.nan, -np.inf
    out, S, n = E.srf_chain(X, lists)
    assert same_bits(out, X) and np.array_equal(n, np.ones(E.NEV))


def test_dealing_sensor_support(lib):
    """the seven bands have the supports their names say, in the library as in srf_numpy"""
    si = E.dealing_sensor()
    w, p = si["wl_srf_smac"], si["p_srf_smac"]
    assert w.shape == p.shape == (E.NEV, 7) and len(E.DEAL_BANDS) == 7
    start, ev, q, Q = lists = srf_numpy.support(w, p)
    assert_support_equal(library_support(lib, w, p), lists)
    band = {name: (ev[start[j]:start[j + 1]], q[start[j]:start[j + 1]], Q[j]) for j, name in enumerate(E.DEAL_BANDS)}
    assert np.array_equal(band["long"][0], np.arange(E.NEV)) and np.array_equal(band["long"][1], p[:, 0])
    for name, e, wt in (("one_700", 300, 1.0), ("one_thermal", srf_numpy.NWL, 1.0), ("one_1650", 1250, 0.75)):
        assert list(band[name][0]) == [e] and list(band[name][1]) == [wt] and band[name][2] == wt, name
    assert list(band["plus_minus"][0]) == [200, 201] and list(band["plus_minus"][1]) == [1.0, -1.0] and band["plus_minus"][2] == 0.0
    assert list(band["zero_weight"][0]) == [50, 465] and list(band["zero_weight"][1]) == [0.0, 1.0] and band["zero_weight"][2] == 1.0
    he, hq, hQ = band["hostile"]
    hostile_only = srf_numpy.support(*[a[:, :1] for a in E.hostile_table()])
    assert np.array_equal(he, hostile_only[1]) and he[0] == 0 and he[-1] == srf_numpy.NWL       # (the padding adds no entry)
    assert np.isnan(hq).sum() == 1 and np.isinf(hq).sum() == 1 and np.isnan(hQ)
    # sorted by support size the deal is [long, hostile, plus_minus, zero_weight | one_700, one_thermal, one_1650, idle]
    assert len(he) > 2 and sorted(np.diff(start))[:3] == [1, 1, 1]
