"""The device-only math of csrc/spart_math.h, element by element on the GPU against long double (float64 functions) and
float64 (float32 functions).

tests/hostmath compiles the header with g++, where Mx<T> is libm and plate_tau reads plain literals.  The product (hipcc,
SPART_FAST_MATH) runs other code: table-driven exp / exp2 / log on two tables staged into LDS, a Taylor exp_poly with
coefficients in constant memory, v_rsq_f64 / v_rcp_f64 with one Newton step, the float32 hardware transcendentals, Taylor
sides behind a wave vote, and plate_tau<double> on constant-memory tables through an inline-asm FMA.  tests/devmath/
devmath_probe.hip maps each of those functions over an array, one lane per element, compiled with the product's flags
(tests/helpers/devmath_probe.py); nothing here goes through libspart_hip.so.

References.  np.longdouble of the exact float64 input (64 mantissa bits asserted; tests/test_devmath_probe_host.py holds
these forms to 1e-18 of mpmath), float64 numpy of the exact float32 input, scipy's expn / exp1 for plate_tau.

Bounds.  EPS = 2^-53, U = 2^-24 (half an ulp of 1.0f).
  float64, from csrc/spart_math.h: exp / exp2 / exp_poly 3e-16 relative for normal results (below that: 3e-16 of the value
  plus half a spacing of the subnormal result, the rounding of ldexp); log max(3e-16, 2e-15 |ln x|) absolute; log1p 2.5e-15
  (tests/test_hostmath.py).  The header's 2e-15 for rcp and 1e-15 for sqrt did not hold and are corrected there: both rest
  on the accuracy of v_rcp_f64 / v_rsq_f64, which the probe also runs alone (SEED64: measured, rounded up to two digits);
  one Newton step leaves d^2 + EPS of the reciprocal (2.23e-15) and
  3 d^2 / 2 + 1.5 EPS of the root (4.22e-15); divx = a * rcp(b) adds the product's rounding.
  1 - e^-z (three float64 forms): |z| < 0.02 is the Taylor side, 3 EPS (the last Horner step and the product z p round
  once each, everything before is scaled by |z| <= 0.02; truncation z^8 / 9! < 1e-19); beyond it 1 - E with E = e^-z good to
  3e-16 relative and one rounding of the difference: (3e-16 + EPS) / (1 - e^-|z|) relative, 2.1e-14 at |z| = 0.02.
  float32 primitives: the project states no figure.  F32_STEPS holds, per function, the worst error measured on one MI355X
  rounded up to the next multiple of U; every entry is under the cap 4 U relative that the float32 forms are held to
  (exp: (1 + |x|) 2 U, since x log2(e) is rounded before v_exp_f32 and ln2 |t| U = |x| U; log / log2 on [0.5, 2): 2 U
  ABSOLUTE, the result passes through 0).
  float32 forms: log1p and log2_1p 4 U (tests/test_hostmath.py); 1 - e^-z and 1 - 2^-z: 4 U on the Taylor side, beyond
  it err(E) E / (1 - E) + U with err(E) the bound asserted here for exp resp. exp2 (plus 2^-126 absolute where E is flushed).

Independence from wave mates.  Every function with a SPART_WAVE_ANY branch (one_minus_exp_neg(z, ez) and
one_minus_exp2_neg(z, e) in float32; sail_j1_d, sail_j1_a, sail_j2_d in both types) and the other float32 forms run the same
16384 inputs in three arrangements: sorted (whole waves on one side of the threshold), interleaved (half a wave each), one
Taylor-side lane per wave.  Each input's result is the same bits in all three.

Block sizes.  Every float64 launch is repeated with 64 threads per workgroup, where stage_f64_tables() needs 4 + 8 passes;
the bits equal those of the 256-thread launch.  (The probe fills both LDS tables with NaN before it calls
stage_f64_tables(): LDS keeps what the previous workgroup staged, which would hide an entry that is never written.)

Table entries.  One wrong unit in the last place of a table entry stays inside every bound above; the mean signed error over
the arguments that read the entry shows it (assert_exp_entries, test_log_f64).

Measured on one MI355X (worst over the inputs of each test; bound beside it):
  the module runs in about 7 s (2 s of it the first use of the GPU); no case takes more than 0.7 s.
  float64  exp 2.39e-16 (3e-16), exp2 2.39e-16, exp_poly 1.5e-16; exp below the normal range: half a spacing; mean signed
           error per table entry off the entry's own rounding by 0.015 units in the last place (0.25)
           log 1.32e-16 absolute on [0.5, 2], 1.88e-16 relative beyond (3e-16 / 2e-15); per table entry 0.086 (0.25)
           v_rcp_f64 alone 4.56e-8 (4.6e-8), v_rsq_f64 alone 5.16e-8 (5.2e-8)
           rcp 2.18e-15 (2.23e-15; the header said 2e-15), every power of two exact; divx 2.14e-15 (2.34e-15)
           sqrt 4.06e-15 (4.22e-15; the header said < 1e-15, taking the residual e = 2 d for the seed's error d);
           11485 of 21281 exact squares give the exact root; sqrt(-1e-300) is -inf, not NaN
           log1p 1.2e-15 (2.5e-15)
           1 - e^-z: Taylor side 2.2e-16 (3.3e-16); direct side 9.1e-15 with exp, 5.6e-15 with exp_poly, both at |z| = 0.02
           (2.1e-14); the header's 1e-16 / 0.02 = 5e-15 left out exp's own error
           plate_tau: tau 6.0e-11 relative (2e-10), 1.5e-12 absolute (5e-11); 1 - tau 1.8e-12 (1e-7)
  float32  (U = 2^-24)  exp 1.21 U per (1 + |x|) (2 U); exp2 1.42 U (2 U); log 1.21 U absolute on [0.5, 2) (2 U), 2.72 U
           relative beyond (3 U); log2 0.998 U absolute (1 U), 1.99 U relative (2 U); sqrt 1.56 U (2 U); rcp 1.54 U (2 U);
           divx 2.44 U (3 U)
           log1p 3.70 U series side, 3.75 U direct side (4 U) -- with v_rcp_f32 in the series: 4.24 U, which is why it divides now
           log2_1p 4.93 U at x = 0.464, series side (8.2 U); 1.77 U direct side (its bound, 1.77 U, is reached at x = 0.968)
           1 - e^-z 1.04e-7 at z = 1.0 (1.99e-7), both forms; 1 - 2^-z 6.6e-8 at z = 1.9 (1.02e-7)
           plate_tau: tau 6.7e-7 relative (1e-6), 1.4e-7 absolute (2.5e-7); 1 - tau 1.9e-7 (1e-6)
  Broken on purpose (scratch builds of the probe, not in the tree), each turned the module red: the last hex digit of
  SPART_F64_EXP_TABLE[100] (test_exp_f64, test_exp2_f64: the per-entry mean) and of one L[i] of SPART_F64_LOG_TABLE
  (test_log_f64, likewise); c_E3_P_F64[3] doubled (test_plate_tau[1]); rcp without its Newton step (rcp, divx, log1p,
  plate_tau); stage_f64_tables() as a single pass (eight float64 tests at block 64, through the NaN the probe leaves in LDS).
"""
import numpy as np
import pytest

from helpers import devmath_probe as D

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -53
U = 2.0 ** -24
N64 = 1 << 20                  # points of a float64 sweep (every launch stays under 2^21)
C_EXP = 369.32993046757463     # 256 / ln 2, the constant of Mx<double>::exp
# v_rcp_f64 / v_rsq_f64 alone: the worst relative error measured on one MI355X, rounded up to two digits
SEED64 = {"rcp": 4.6e-8, "rsq": 5.2e-8}
RCP64 = SEED64["rcp"] ** 2 + EPS                   # r (2 - x r): the seed's error squared, and the rounding of the last FMA: 2.23e-15


def sqrt64_bound(eta):
    """y0 = (1 + eta) / sqrt(x): g = x y0 and e = 1 - g y0 = -2 eta - eta^2 give g (1 + e / 2) = sqrt(x) (1 - 3 eta^2 / 2 - eta^3 / 2);
    the last FMA rounds once and g's own rounding enters halved"""
    return 1.5 * eta * eta + 1.5 * EPS


SQRT64 = sqrt64_bound(SEED64["rsq"])               # 4.2e-15
CAP = 4                        # float32: 4 U relative, the float32 forms' bound
# worst measured error in multiples of U, rounded up (see the module docstring for the unit of each)
F32_STEPS = {"exp": 2, "exp2": 2, "log": 3, "log_near_1": 2, "log2": 2, "log2_near_1": 1, "sqrt": 2, "rcp": 2, "divx": 3}
F32_CAPS = {"exp": 2, "log_near_1": 2, "log2_near_1": 2}      # (every other: CAP)


class Probe:
    """the probe library and a device to run it on: numpy in, numpy out, one launch per call"""

    def __init__(self):
        import torch
        assert torch.cuda.is_available(), "the device math tests need a GPU"
        self.torch = torch
        self.lib = {t: D.load(t) for t in (0, 1)}
        for lib in self.lib.values():
            assert lib.dm_fast_math() == 1, "the probe was not compiled with SPART_FAST_MATH"

    def _dev(self, x, dtype):
        x = np.ascontiguousarray(x, dtype=np.float64 if dtype else np.float32)
        return self.torch.as_tensor(x, device="cuda:0")

    def _out(self, t):
        return self.torch.full_like(t, float("nan"))

    def unary(self, name, x, dtype, block=256):
        t = self._dev(x, dtype)
        y = self._out(t)
        rc = self.lib[dtype].dm_unary(dtype, D.UNARY[name], t.data_ptr(), y.data_ptr(), t.numel(), block)
        assert rc == 0, (name, rc)
        return y.cpu().numpy()

    def binary(self, name, a, b, dtype, block=256):
        ta, tb = self._dev(a, dtype), self._dev(b, dtype)
        assert ta.shape == tb.shape
        y = self._out(ta)
        rc = self.lib[dtype].dm_binary(dtype, D.BINARY[name], ta.data_ptr(), tb.data_ptr(), y.data_ptr(), ta.numel(), block)
        assert rc == 0, (name, rc)
        return y.cpu().numpy()

    def plate(self, x, dtype, block=256):
        t = self._dev(x, dtype)
        tau, u = self._out(t), self._out(t)
        rc = self.lib[dtype].dm_plate_tau(dtype, t.data_ptr(), tau.data_ptr(), u.data_ptr(), t.numel(), block)
        assert rc == 0, rc
        return tau.cpu().numpy(), u.cpu().numpy()


@pytest.fixture(scope="module")
def probe():
    assert np.finfo(LD).nmant >= 63, "np.longdouble has no more bits than float64 here: there is no reference to compare with"
    return Probe()


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                                                 b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


def both_blocks(run, *args):
    """a float64 launch at 256 threads per workgroup and again at 64: the same bits"""
    y = run(*args, 1, 256)
    y64 = run(*args, 1, 64)
    if isinstance(y, tuple):
        assert all(same_bits(p, q) for p, q in zip(y, y64)), "block 64 and block 256 differ"
    else:
        assert same_bits(y, y64), "block 64 and block 256 differ"
    return y


def held(what, worst, bound):
    """print the figure, then hold it (worst and bound may be arrays: the worst ratio decides)"""
    worst, bound = np.asarray(worst, dtype=LD), np.asarray(bound, dtype=LD)
    assert np.isfinite(worst).all(), what
    ratio = worst / bound
    i = int(np.argmax(ratio)) if ratio.ndim else 0
    w, b = (float(worst.flat[i]), float(np.broadcast_to(bound, worst.shape).flat[i])) if ratio.ndim else (float(worst), float(bound))
    print(f"[devmath] {what}: {w:.3g} (bound {b:.3g})")
    assert w <= b, what


def rel(y, ref):
    return np.abs((y.astype(LD) - ref) / ref)


# ------------------------------------------------------------------------------------------ float64 inputs
def table_points(scale):
    """arguments x = (k + s) / scale of the table-driven exp (k = rint(x scale), entry k & 255): every entry, eight times over and
    at far exponents, at the middle of its interval, next to both ends and a few units in the last place around them"""
    k = np.concatenate([np.arange(-1024, 1024), np.arange(-180000, -180000 + 256), np.arange(150000, 150000 + 256)]).astype(np.float64)
    pts = [(k + s) / scale for s in (-0.4999, -0.25, 0.0, 0.25, 0.4999)]
    half = (k + 0.5) / scale
    for _ in range(3):
        half = np.nextafter(half, -np.inf)
    for _ in range(6):
        pts.append(half.copy())
        half = np.nextafter(half, np.inf)
    return np.concatenate(pts)


def assert_all_entries(x, scale):
    k = np.rint(x * scale)                   # (the device's own first two instructions; IEEE in numpy too)
    idx = k.astype(np.int64) & 255
    frac = x * scale - k
    assert np.array_equal(np.unique(idx), np.arange(256))
    lo, hi = np.full(256, np.inf), np.full(256, -np.inf)
    np.minimum.at(lo, idx, frac)
    np.maximum.at(hi, idx, frac)
    assert lo.max() < -0.49 and hi.min() > 0.49, "an entry of the exp table is not reached next to both ends of its interval"


def per_entry_mean(idx, signed):
    return np.bincount(idx, weights=np.asarray(signed, dtype=np.float64), minlength=256) / np.maximum(np.bincount(idx, minlength=256), 1)


def assert_exp_entries(x, y, ref, scale, what):
    """The worst error cannot see one wrong unit in the last place of a table entry (2.2e-16 relative, inside the bound), the mean
    can: over the few thousand arguments that read entry j, the signed relative error averages to the entry's own rounding
    error, (T[j] - 2^(j/256)) / 2^(j/256) with T[j] the correctly rounded value -- every other rounding of the sequence is
    unbiased and the remainder r^5 / 120 is odd in r.  A wrong last digit moves the mean by a whole unit in the last place of
    T[j]; the mean of a few thousand roundings is good to a few hundredths of one: held to a quarter."""
    idx = np.rint(x * scale).astype(np.int64) & 255
    assert np.bincount(idx, minlength=256).min() >= 2000
    exact = np.exp2(np.arange(256, dtype=LD) / 256)
    want = ((exact.astype(np.float64).astype(LD) - exact) / exact).astype(np.float64)
    off = (per_entry_mean(idx, (y.astype(LD) - ref) / ref) - want) * exact.astype(np.float64) / 2.0 ** -52
    held(f"{what}: mean signed error per table entry against the entry's own rounding, units in the last place of T[j]", np.abs(off).max(), 0.25)


def exp_sweep(lo, hi, scale, seed):
    rng = np.random.default_rng(seed)
    tiny = 10.0 ** rng.uniform(-300, 0, 1 << 14)
    x = np.concatenate([rng.uniform(lo, hi, N64 - (1 << 17)), tiny, -tiny, table_points(scale), [0.0, -0.0, lo, hi]])
    x = x[(x >= lo) & (x <= hi)]
    assert x.size <= 1 << 21
    return x


def log_table_points():
    """every entry of the log table (the top 8 mantissa bits) at the first, second, middle and last mantissa of its interval, in
    the binades next to 1, a few others and the two outermost normal ones"""
    i = np.arange(256, dtype=np.uint64)[None, :, None]
    low = np.array([0, 1, 1 << 43, (1 << 44) - 1], dtype=np.uint64)[None, None, :]
    e = (np.array([-1022, -500, -2, -1, 0, 1, 2, 10, 700, 1023], dtype=np.int64) + 1023).astype(np.uint64)[:, None, None]
    return ((e << np.uint64(52)) | (i << np.uint64(44)) | low).ravel().view(np.float64)


def log_inputs():
    rng = np.random.default_rng(2)
    d = 10.0 ** rng.uniform(-16, -1, 1 << 16)
    return np.concatenate([2.0 ** rng.uniform(-1022, 1023.999, 1 << 19), rng.uniform(0.5, 2.0, 1 << 20), 1.0 + d, 1.0 - d,
                           log_table_points(), [1.0, 0.5, 2.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), np.finfo(np.float64).tiny,
                                                np.finfo(np.float64).max]])


def around(t, dtype):
    """both sides of a switch point t: t itself, its neighbours, and points up to 10 % away on either side"""
    T = np.float64 if dtype else np.float32
    t = T(t)
    d = (10.0 ** np.random.default_rng(3).uniform(-15 if dtype else -7, -1, 4096)).astype(T)
    return np.concatenate([[np.nextafter(t, T(0)), t, np.nextafter(t, T(2) * t)], t * (T(1) + d), t * (T(1) - d)]).astype(T)


# ------------------------------------------------------------------------------------------ float64 primitives
def test_compiled_branch_is_the_device_one(probe):
    """the probe reports SPART_FAST_MATH (Probe()), and Mx<double>::exp(NaN) is 0 as csrc/spart_math.h documents for the
    table-driven exp; libm's exp, the host branch, returns NaN"""
    y = both_blocks(probe.unary, "exp", np.array([np.nan, 0.0, 1.0]))
    assert y[0] == 0.0 and y[1] == 1.0 and abs(y[2] - np.e) < 1e-15


def test_exp_f64(probe):
    x = exp_sweep(-708.0, 700.0, C_EXP, 1)
    assert_all_entries(x, C_EXP)
    y = both_blocks(probe.unary, "exp", x)
    ref = np.exp(x.astype(LD))
    held("Mx<double>::exp, [-708, 700], relative", rel(y, ref).max(), 3e-16)
    assert_exp_entries(x, y, ref, C_EXP, "Mx<double>::exp")
    edge = np.array([0.0, -0.0, -745.2, -800.0, -1e9, -np.inf])
    ye = both_blocks(probe.unary, "exp", edge)
    assert ye[0] == 1.0 and ye[1] == 1.0 and np.array_equal(ye[2:], np.zeros(4)) and not np.signbit(ye[2:]).any()
    # results below the normal range: the value's 3e-16 and the rounding of ldexp to a multiple of 2^-1074
    xs = np.random.default_rng(4).uniform(-745.0, -708.0, 1 << 16)
    ys = both_blocks(probe.unary, "exp", xs)
    ref = np.exp(xs.astype(LD))
    spacing = np.maximum(np.spacing(ref.astype(np.float64)), 2.0 ** -1074).astype(LD)
    held("Mx<double>::exp, (-745, -708), spacings of the result", np.abs(ys.astype(LD) - ref) / spacing, 3e-16 * ref / spacing + 0.5)


def test_exp2_f64(probe):
    x = exp_sweep(-1022.0, 1000.0, 256.0, 5)
    assert_all_entries(x, 256.0)
    y = both_blocks(probe.unary, "exp2", x)
    ref = np.exp2(x.astype(LD))
    held("Mx<double>::exp2, [-1022, 1000], relative", rel(y, ref).max(), 3e-16)
    assert_exp_entries(x, y, ref, 256.0, "Mx<double>::exp2")
    assert both_blocks(probe.unary, "exp2", np.array([0.0, 1.0, -1.0, 10.0])).tolist() == [1.0, 2.0, 0.5, 1024.0]


def test_exp_poly_f64(probe):
    x = exp_sweep(-708.0, 700.0, C_EXP, 6)
    y = both_blocks(probe.unary, "exp_poly", x)
    held("Mx<double>::exp_poly, [-708, 700], relative", rel(y, np.exp(x.astype(LD))).max(), 3e-16)
    ye = both_blocks(probe.unary, "exp_poly", np.array([np.nan, 0.0, -745.2, -800.0, -1e9, -np.inf]))
    assert np.isnan(ye[0]) and ye[1] == 1.0 and np.array_equal(ye[2:], np.zeros(4))


def test_log_f64(probe):
    x = log_inputs()
    idx = (x.view(np.uint64) >> np.uint64(44)) & np.uint64(255)
    assert np.array_equal(np.unique(idx), np.arange(256, dtype=np.uint64)), "an entry of the log table is not reached"
    assert x.size <= 1 << 21 and (x >= np.finfo(np.float64).tiny).all()
    y = both_blocks(probe.unary, "log", x)
    ref = np.log(x.astype(LD))
    held("Mx<double>::log, positive normals, absolute against max(3e-16, 2e-15 |ln x|)", np.abs(y.astype(LD) - ref),
         np.maximum(LD(3e-16), 2e-15 * np.abs(ref)))
    near = (x >= 0.5) & (x <= 2.0)
    print(f"[devmath] Mx<double>::log: absolute on [0.5, 2] {float(np.abs(y.astype(LD) - ref)[near].max()):.3g}, "
          f"relative beyond {float(rel(y[~near], ref[~near]).max()):.3g}")
    assert y[x == 1.0].size and (y[x == 1.0] == 0.0).all()
    # One wrong unit in the last place of L[i] (3e-17 at most) is far inside the bound.  In [1, 2) the result is L[i] + log1p(z)
    # rounded once, so over the arguments that read entry i the signed error averages to L[i]'s own rounding error,
    # L[i] - (-ln R[i]) with R[i] = 1 / (1 + (i + 1/2) / 256) as a float64 (tools/gen_f64_tables.py); a wrong R[i] moves log1p(z)
    # by 1e-16 and shows the same way.  A wrong last digit is a whole unit in the last place of L[i]; the mean is good to a tenth
    # of one (the first entries' L[i] are no larger than log1p(z), whose roundings then weigh as much): held to a quarter.
    m = (x >= 1.0) & (x < 2.0)
    assert np.bincount(idx[m].astype(np.int64), minlength=256).min() >= 2000
    R = 1.0 / (1.0 + (np.arange(256) + 0.5) / 256.0)
    exact = -np.log(R.astype(LD))
    want = (exact.astype(np.float64).astype(LD) - exact).astype(np.float64)
    off = (per_entry_mean(idx[m].astype(np.int64), y[m].astype(LD) - ref[m]) - want) / np.spacing(exact.astype(np.float64))
    held("Mx<double>::log: mean signed error per table entry against the entry's own rounding, units in the last place of L[i]", np.abs(off).max(), 0.25)


def test_rcp_rsq_seeds_f64(probe):
    """the seeds of Mx<double>::rcp and sqrt, on whose accuracy the bounds of everything refined from them rest"""
    x = 10.0 ** np.random.default_rng(13).uniform(-300, 300, N64)
    held("v_rcp_f64 alone, relative", rel(probe.unary("rcp_seed", x, 1), 1 / x.astype(LD)).max(), SEED64["rcp"])
    held("v_rsq_f64 alone, relative", rel(probe.unary("rsq_seed", x, 1), 1 / np.sqrt(x.astype(LD))).max(), SEED64["rsq"])


def test_sqrt_f64(probe):
    """SQRT64 where the guard x + 1e-300 of the rsq argument is harmless; below 1e-292 the guard shifts the argument by
    d = 1e-300 / x, which adds 1 - (1 + d)^-1/2 <= d / 2 to the seed's own error (12 % low at x = 1e-300: csrc/spart_math.h says
    so).  Exact squares are inputs like any other: one Newton step does not round correctly, about half of them give the exact root."""
    rng = np.random.default_rng(7)
    n = np.concatenate([np.arange(1.0, 4097.0), rng.integers(1, 1 << 26, 1 << 14).astype(np.float64)])
    squares = np.concatenate([n * n, 4.0 ** np.arange(-400.0, 401.0)])       # (n < 2^26: n n is exact)
    x = np.concatenate([10.0 ** rng.uniform(-292, 300, N64), squares])
    y = probe.unary("sqrt", x, 1)
    held("Mx<double>::sqrt, 1e-292 ... 1e300, relative", rel(y, np.sqrt(x.astype(LD))).max(), SQRT64)
    roots = np.concatenate([n, 2.0 ** np.arange(-400.0, 401.0)])
    exact = y[N64:] == roots
    print(f"[devmath] Mx<double>::sqrt: {int(exact.sum())} of {exact.size} exact squares give the exact root")
    held("Mx<double>::sqrt, exact squares, relative", np.abs(y[N64:] - roots) / roots, SQRT64)
    lo = np.concatenate([10.0 ** rng.uniform(-300, -292, 1 << 16), [1e-300, 1e-299, 1e-296, 2e-293, 1e-292]])
    d = LD(1e-300) / lo.astype(LD)
    held("Mx<double>::sqrt, 1e-300 ... 1e-292, relative against the guard's shift", rel(probe.unary("sqrt", lo, 1), np.sqrt(lo.astype(LD))),
         sqrt64_bound(SEED64["rsq"] + d / 2))
    # below -1e-300 the rsq argument is negative: NaN.  AT -1e-300 it is 0: rsq = inf and the result is -inf, not NaN
    ye = probe.unary("sqrt", np.array([0.0, np.nextafter(-1e-300, -1.0), -1.0, -1e300, np.nan, -np.inf, -1e-300]), 1)
    assert ye[0] == 0.0 and np.isnan(ye[1:6]).all() and ye[6] == -np.inf


def rcp_inputs(seed):
    rng = np.random.default_rng(seed)
    x = 10.0 ** rng.uniform(-300, 300, N64)
    return x * rng.choice([-1.0, 1.0], N64)


def test_rcp_f64(probe):
    x = rcp_inputs(8)
    y = probe.unary("rcp", x, 1)
    held("Mx<double>::rcp, +-1e-300 ... +-1e300, relative", rel(y, 1 / x.astype(LD)).max(), RCP64)
    p = 2.0 ** np.arange(-1022.0, 1023.0)
    p = np.concatenate([p, -p])
    assert np.array_equal(probe.unary("rcp", p, 1), 1.0 / p), "the reciprocal of a power of two is not exact"


def test_divx_f64(probe):
    a, b = rcp_inputs(9), rcp_inputs(10)
    a = np.where(np.abs(np.log10(np.abs(a)) - np.log10(np.abs(b))) < 300, a, 1.0)       # (the quotient stays normal)
    y = probe.binary("divx", a, b, 1)
    held("divx<double>, relative", rel(y, a.astype(LD) / b.astype(LD)).max(), RCP64 + EPS)
    p = 2.0 ** np.random.default_rng(11).integers(-500, 500, 4096).astype(np.float64)
    a = rcp_inputs(12)[:4096]
    a = np.where(np.abs(np.log2(np.abs(a))) < 500, a, 3.0)
    assert np.array_equal(probe.binary("divx", a, p, 1), a / p), "division by a power of two is not exact"


# ------------------------------------------------------------------------------------------ float64 forms
def test_log1p_f64(probe):
    x = np.concatenate([[0.0], np.logspace(-12, 6, N64), [1e30], around(0.1, 1)])
    y = both_blocks(probe.unary, "log1p", x)
    assert y[0] == 0.0
    held("Mx<double>::log1p, relative", rel(y[1:], np.log1p(x[1:].astype(LD))).max(), 2.5e-15)


@pytest.mark.parametrize("name", ["omen", "omen_ez", "omen_poly"])
def test_one_minus_exp_neg_f64(probe, name):
    """one_minus_exp_neg(z), (z, ez = exp(-z)) and _poly.  A negative z beyond -0.02 must not take the series: there the series'
    own truncation error (|z|^8 / 9! relative, 1e-6 at z = -1) is far outside the bound."""
    z = np.logspace(-12, np.log10(700.0), N64 // 2)
    z = np.concatenate([[0.0, -0.0], z, -z, around(0.02, 1), -around(0.02, 1)])
    y = both_blocks(probe.unary, name, z)
    assert y[0] == 0.0 and y[1] == 0.0
    z, y = z[2:], y[2:]
    ref = -np.expm1(-z.astype(LD))
    az = np.abs(z)
    bound = np.where(az < 0.02, 3 * EPS, (3e-16 + EPS) / -np.expm1(-np.maximum(az, 0.02)))
    held(f"Mx<double>::{name}, +-1e-12 ... +-700, relative", rel(y, ref), bound)
    t = az < 0.02
    print(f"[devmath] Mx<double>::{name}: Taylor side {float(rel(y, ref)[t].max()):.3g}, direct side {float(rel(y, ref)[~t].max()):.3g}")


def plate_inputs(dtype):
    T = np.float64 if dtype else np.float32
    tiny = T(1e-300 if dtype else 1e-30)
    K = np.concatenate([[0.0, -1.0, np.nan, tiny, np.nextafter(tiny, T(0)), np.nextafter(tiny, T(1))],
                        np.logspace(-9, 2.5, 4000), around(1.0, dtype)]).astype(T)
    return K, 6


@pytest.mark.parametrize("dtype,tol", [(1, 2e-10), (0, 1e-6)])
def test_plate_tau(probe, dtype, tol):
    """the assertions of tests/test_hostmath.py::test_plate_transmittance for the device's tables and sequence, and both
    sides of the two switch points K = 1 and K = tiny()"""
    from scipy.special import exp1, expn
    K, ns = plate_inputs(dtype)
    tau, u = both_blocks(probe.plate, K) if dtype else probe.plate(K, 0)
    tau, u = tau.astype(np.float64), u.astype(np.float64)
    assert tau[0] == 1.0 and 0.0 <= u[0] < 1e-29 and tau[1] == 1.0  # K <= 0 -> tau = 1 (prospect_5d.py:195)
    assert np.isnan(tau[2]) and np.isnan(u[2])                        # NaN propagates
    assert (tau[3:ns] == 1.0).all() and (u[3:ns] >= 0.0).all() and (u[3:ns] < 1e-29).all()
    x = K[ns:].astype(np.float64)
    tau, u = tau[ns:], u[ns:]
    ref = 2 * expn(3, x)
    m = ref > 1e-6          # beyond K ~ 11 float32 exp(-K) itself carries K * 6e-8 relative error
    held(f"plate_tau<{'double' if dtype else 'float'}>: tau, relative where tau > 1e-6", np.max(np.abs(tau[m] - ref[m]) / ref[m]), tol)
    held(f"plate_tau<{'double' if dtype else 'float'}>: tau, absolute", np.max(np.abs(tau - ref)), tol * 0.25)
    ref_u = np.where(x < 0.5, -np.expm1(-x) * (1 - x) + x - x * x * exp1(x), 1 - ref)  # (1-x)(1-e^-x) + x - x^2 E1
    held(f"plate_tau<{'double' if dtype else 'float'}>: 1 - tau, relative", np.max(np.abs(u - ref_u) / ref_u),
         1e-7 if dtype == 1 else tol)   # (the fp64 reference form itself cancels ~1e-8)


# ------------------------------------------------------------------------------------------ float32 primitives
def binade(e, sign=1.0):
    """all 2^23 float32 values of [2^e, 2^(e+1))"""
    x = (np.arange(1 << 23, dtype=np.uint32) | np.uint32((e + 127) << 23)).view(np.float32)
    return x if sign > 0 else -x


def sampled_binades(lo, hi, per, seed):
    """`per` random mantissas in every binade 2^lo ... 2^hi"""
    rng = np.random.default_rng(seed)
    e = np.repeat(np.arange(lo, hi + 1, dtype=np.int64) + 127, per).astype(np.uint32)
    return ((e << np.uint32(23)) | rng.integers(0, 1 << 23, e.size, dtype=np.uint32)).view(np.float32)


def worst_steps(probe, name, chunks, ref, scale=None):
    """the worst error of a float32 unary function over the chunks, in multiples of U: relative to the float64 reference, or
    (scale given) absolute error divided by scale(x, ref)"""
    worst = 0.0
    for x in chunks:
        y = probe.unary(name, x, 0).astype(np.float64)
        xd = x.astype(np.float64)
        r = ref(xd)
        err = np.abs(y - r) / (np.abs(r) if scale is None else scale(xd, r))
        assert np.isfinite(err).all(), name
        worst = max(worst, float(err.max()) / U)
    return worst


def held_steps(key, what, steps):
    print(f"[devmath] {what}: {steps:.3f} U (asserted {F32_STEPS[key]} U, cap {F32_CAPS.get(key, CAP)} U)")
    assert F32_STEPS[key] <= F32_CAPS.get(key, CAP), key
    assert steps <= F32_STEPS[key], what


def clipped(x, lo):
    return x[x >= lo]


def test_exp_f32(probe):
    """__expf over the callers' domain [-87, 0]: every float32 of [-87, -0.25], sampled above; against (1 + |x|) U"""
    chunks = [clipped(binade(e, -1.0), -87.0) for e in range(-2, 7)]
    chunks.append(np.concatenate([[0.0, -0.0], -(10.0 ** np.random.default_rng(20).uniform(-30, np.log10(0.25), 1 << 20))]).astype(np.float32))
    held_steps("exp", "Mx<float>::exp, [-87, 0], error / (1 + |x|)", worst_steps(probe, "exp", chunks, np.exp, lambda x, r: r * (1 + np.abs(x))))
    assert probe.unary("exp", np.zeros(1), 0)[0] == 1.0


def test_exp2_f32(probe):
    """v_exp_f32 over the callers' domain [-100, 0]: every float32 of [-100, -0.25], sampled above"""
    chunks = [clipped(binade(e, -1.0), -100.0) for e in range(-2, 7)]
    chunks.append(np.concatenate([[0.0, -0.0], -(10.0 ** np.random.default_rng(21).uniform(-30, np.log10(0.25), 1 << 20))]).astype(np.float32))
    held_steps("exp2", "Mx<float>::exp2, [-100, 0], relative", worst_steps(probe, "exp2", chunks, np.exp2))
    assert probe.unary("exp2", np.zeros(1), 0)[0] == 1.0


@pytest.mark.parametrize("name,ref", [("log", np.log), ("log2", np.log2)])
def test_log_f32(probe, name, ref):
    """v_log_f32 (times ln 2): [0.5, 2) exhaustively against an ABSOLUTE bound, every other positive normal binade by sampling
    against a relative one"""
    held_steps(name + "_near_1", f"Mx<float>::{name}, [0.5, 2), absolute", worst_steps(probe, name, [binade(-1), binade(0)], ref, lambda x, r: 1.0))
    x = sampled_binades(-126, 127, 4096, 22)
    x = x[(x < 0.5) | (x >= 2.0)]
    held_steps(name, f"Mx<float>::{name}, positive normals outside [0.5, 2), relative", worst_steps(probe, name, [x], ref))
    assert probe.unary(name, np.ones(1), 0)[0] == 0.0


def test_sqrt_f32(probe):
    chunks = [binade(0), binade(1), sampled_binades(-126, 127, 4096, 23)]
    held_steps("sqrt", "Mx<float>::sqrt, [1, 4) exhaustively, normals sampled, relative", worst_steps(probe, "sqrt", chunks, np.sqrt))
    assert probe.unary("sqrt", np.zeros(1), 0)[0] == 0.0


def test_rcp_f32(probe):
    s = sampled_binades(-125, 125, 4096, 24)
    chunks = [binade(0), binade(1), binade(0, -1.0), s, -s]
    held_steps("rcp", "Mx<float>::rcp, +-[1, 2) and [2, 4) exhaustively, normals sampled, relative", worst_steps(probe, "rcp", chunks, lambda x: 1 / x))


def test_divx_f32(probe):
    rng = np.random.default_rng(25)
    worst = 0.0
    for b in (binade(0), binade(1), sampled_binades(-60, 60, 8192, 26)):
        a = (rng.uniform(1.0, 2.0, b.size) * rng.choice([-1.0, 1.0], b.size)).astype(np.float32)
        y = probe.binary("divx", a, b, 0).astype(np.float64)
        r = a.astype(np.float64) / b.astype(np.float64)
        worst = max(worst, float(np.max(np.abs(y - r) / np.abs(r))) / U)
    held_steps("divx", "divx<float>, divisors of [1, 4) exhaustively, sampled elsewhere, relative", worst)


# ------------------------------------------------------------------------------------------ float32 forms
def form_inputs(switch, seed):
    """0, 1e-12 ... 1e6, and every float32 of the binade that holds the switch point and of the one below it"""
    e = int(np.floor(np.log2(switch)))
    head = np.concatenate([[0.0], np.logspace(-12, 6, 1 << 20), around(switch, 0)]).astype(np.float32)
    return [head, binade(e - 1), binade(e)]


def log1p_bound(name, x):
    """log1p<float>: 4 U, the bound tests/test_hostmath.py::test_log1p_forms holds the host build to.
    log2_1p: first-order propagation through its own sequence, R = the bound asserted for Mx<float>::rcp above, in U.
    x < 0.5: s = x rcp(2 + x) carries Es = 1 (the sum) + R + 1 (the product); q = 1 + s2 P with s2 = s s <= 0.04 and
    P <= 0.34 carries 0.04 * 0.34 * (2 Es + 1 (s2) + 2 (P) + 1 (the product)) + 1 (the sum); the result (c s) q carries Es + 1 (c's own
    rounding) + 1 + 1 (the two products) + q's.  x >= 0.5: w = 1 + x is off by half a spacing, log2(e) spacing(w) / (2 w) absolute in
    the result; v_log_f32 adds what is asserted for it above: absolute on [0.5, 2), relative beyond."""
    if name == "log1p":
        return np.full(x.shape, 4 * U)
    Es = 2 + F32_STEPS["rcp"]
    series = (Es + 3 + 0.04 * 0.34 * (2 * Es + 4) + 1) * U
    w = (np.float32(1) + x.astype(np.float32)).astype(np.float64)
    lg = np.where(w > 1, np.log2(w), 1.0)       # (w == 1 only far inside the series side)
    direct = (np.spacing(w.astype(np.float32)).astype(np.float64) / (2 * w) / np.log(2.0)
              + np.where(w < 2, F32_STEPS["log2_near_1"] * U, F32_STEPS["log2"] * U * lg)) / lg
    return np.where(x < 0.5, series, direct)


@pytest.mark.parametrize("name,ref", [("log1p", np.log1p), ("log2_1p", lambda x: np.log1p(x) / np.log(2.0))])
def test_log1p_f32(probe, name, ref):
    worst = {}
    for x in form_inputs(0.5, 30):
        y = probe.unary(name, x, 0).astype(np.float64)
        nz = x > 0
        assert (y[~nz] == 0.0).all()
        xd = x[nz].astype(np.float64)
        r = ref(xd)
        err = np.abs(y[nz] - r) / r
        ratio = err / log1p_bound(name, xd)
        for side, m in (("series", xd < 0.5), ("direct", xd >= 0.5)):
            if m.any():
                i = np.flatnonzero(m)[np.argmax(ratio[m])]
                if ratio[i] > worst.get(side, (0,))[0]:
                    worst[side] = (float(ratio[i]), float(xd[i]), float(err[i]) / U)
    for side, (ratio, at, steps) in worst.items():
        print(f"[devmath] Mx<float>::{name}, {side} side: worst error / bound {ratio:.3f} at x = {at:.9g} ({steps:.3f} U)")
    assert max(v[0] for v in worst.values()) <= 1.0, name


@pytest.mark.parametrize("name,switch", [("omen", 0.25), ("omen_ez", 0.25), ("omen2_e", 0.360673760)])
def test_one_minus_exp_neg_f32(probe, name, switch):
    """1 - e^-z (two forms) and 1 - 2^-z.  Taylor side 4 U; direct side: E = e^-z resp. 2^-z carries the error asserted for
    Mx<float>::exp resp. exp2 above (absolute 2^-126 where it is flushed), 1 - E rounds once."""
    base2 = name == "omen2_e"
    sw = float(np.float32(switch))
    worst, at = 0.0, None
    for x in form_inputs(switch, 31):
        y = probe.unary(name, x, 0).astype(np.float64)
        nz = x > 0
        assert (y[~nz] == 0.0).all()
        z = x[nz].astype(np.float64)
        zl = z * np.log(2.0) if base2 else z
        r = -np.expm1(-zl)
        E = np.exp(-zl)
        errE = F32_STEPS["exp2"] * U * E if base2 else F32_STEPS["exp"] * U * (1 + z) * E
        bound = np.where(z < sw, 4 * U, (errE + 2.0 ** -126) / r + U)
        ratio = np.abs(y[nz] - r) / r / bound
        i = int(np.argmax(ratio))
        if ratio[i] > worst:
            worst, at = float(ratio[i]), (float(z[i]), float(np.abs(y[nz][i] - r[i]) / r[i]), float(bound[i]))
    print(f"[devmath] Mx<float>::{name}: worst error / bound {worst:.3f}, at z = {at[0]:.6g}: {at[1]:.3g} relative (bound {at[2]:.3g})")
    assert worst <= 1.0, name


# ------------------------------------------------------------------------------------------ wave votes
def arrangements(n_taylor=256):
    """three permutations of 64 n_taylor slots whose first n_taylor values are Taylor-side: sorted (waves wholly on one side),
    interleaved (Taylor-side values in every other lane of the first waves), one Taylor-side lane per wave (a different lane each)"""
    n = 64 * n_taylor
    sorted_ = np.arange(n)
    inter = np.empty(n, dtype=np.int64)
    inter[0:2 * n_taylor:2] = np.arange(n_taylor)
    inter[1:2 * n_taylor:2] = np.arange(n_taylor, 2 * n_taylor)
    inter[2 * n_taylor:] = np.arange(2 * n_taylor, n)
    one = np.empty(n, dtype=np.int64)
    slot = 64 * np.arange(n_taylor) + (np.arange(n_taylor) * 7) % 64
    rest = np.ones(n, dtype=bool)
    rest[slot] = False
    one[slot] = np.arange(n_taylor)
    one[rest] = np.arange(n_taylor, n)
    return {"sorted": sorted_, "interleaved": inter, "one per wave": one}


def assert_arrangement_free(run, values, what):
    """values: tuple of arrays, Taylor-side elements first.  run(*arrays) -> results; each input's result must not depend on
    where it sits"""
    first = None
    for label, perm in arrangements(values[0].size // 64).items():
        y = run(*[v[perm] for v in values])
        back = np.empty_like(y)
        back[perm] = y
        assert not np.isnan(back).any(), (what, label)
        if first is None:
            first = back
        else:
            differ = int((first.view(np.uint8) != back.view(np.uint8)).reshape(back.size, -1).any(axis=1).sum())
            assert differ == 0, f"{what}: {differ} results differ between the sorted and the {label} arrangement"


def two_sided(thresh, dtype, seed, n_taylor=256, lo=1e-6, hi=None, signed=False):
    """n_taylor values below thresh followed by 63 n_taylor values above it"""
    T = np.float64 if dtype else np.float32
    rng = np.random.default_rng(seed)
    t = 10.0 ** rng.uniform(np.log10(lo), np.log10(thresh * 0.999), n_taylor)
    d = 10.0 ** rng.uniform(np.log10(thresh * 1.001), np.log10(hi or thresh * 100), 63 * n_taylor)
    v = np.concatenate([t, d])
    if signed:
        v = v * rng.choice([-1.0, 1.0], v.size)
    v = v.astype(T)
    assert (np.abs(v[:n_taylor]) < T(thresh)).all() and (np.abs(v[n_taylor:]) >= T(thresh)).all()
    return v


@pytest.mark.parametrize("name,thresh", [("omen_ez", 0.25), ("omen2_e", 0.360673760), ("omen", 0.25), ("log1p", 0.5), ("log2_1p", 0.5)])
def test_f32_forms_do_not_depend_on_wave_mates(probe, name, thresh):
    z = two_sided(thresh, 0, 40)
    assert_arrangement_free(lambda v: probe.unary(name, v, 0), (z,), f"Mx<float>::{name}")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name", ["j1_d", "j1_a", "j2_d"])
def test_sail_j_does_not_depend_on_wave_mates(probe, name, dtype):
    thresh = 2e-3 if dtype else 0.06       # SailJ<T>::THRESH
    d = two_sided(thresh, dtype, 41, hi=5.0, signed=name != "j2_d")
    L = np.random.default_rng(42).uniform(0.1, 7.0, d.size).astype(d.dtype)
    assert_arrangement_free(lambda a, b: probe.binary(name, a, b, dtype), (d, L), f"sail_{name}<{'double' if dtype else 'float'}>")
