"""spart_vjp without a GPU: the definition tools/vjp_defined.py against the analytic gradient of a quadratic toy model (exact
rationals), the g++ build of csrc/spart_vjp.h's per-entry functions against the definition bit for bit (and as a stand-alone
sanitizer program), the consequences the header states on the toy model, every refusal in its order, the Python layer's checks
and the agreement of signatures, struct and header."""
import ctypes
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from helpers.vjp_calls import same, vd

SRC = os.path.join(ROOT, "tests", "hostmath", "vjp_host.cpp")
EPS = 2.0 ** -52
c_dp = ctypes.POINTER(ctypes.c_double)
GXX = ["-std=c++17", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1"]
S2 = "Sentinel2A-MSI"


def dp(a):
    return None if a is None else a.ctypes.data_as(c_dp)


# ---- the definition against analytic gradients.  The toy model is quadratic and separable in the free columns,
#   Y_c[j](p) = alpha_cj + sum_f beta_cjf p_f + gamma_cjf p_f^2,
# so a difference quotient over ANY two points a, b of column f is exactly beta + gamma (a + b): the slope at their midpoint,
# which is x itself for a central difference.  Coefficients and points are floats, the model is evaluated in exact rationals
# and each Y rounded once to float64.
class Toy:
    def __init__(self, free, nb, seed):
        rng = np.random.default_rng(seed)
        self.free, self.nb = list(free), nb
        self.alpha = rng.integers(-8, 9, (3, nb)) / 8.0
        self.beta = rng.integers(-16, 17, (3, nb, len(free))) / 16.0
        self.gamma = rng.integers(-16, 17, (3, nb, len(free))) / 64.0

    def exact(self, row, c, j):
        v = Fraction(self.alpha[c, j])
        for f, k in enumerate(self.free):
            p = Fraction(row[k])
            v += Fraction(self.beta[c, j, f]) * p + Fraction(self.gamma[c, j, f]) * p * p
        return v

    def forward(self, rows):
        ok = [bool(np.isfinite(r[self.free]).all()) for r in rows]                # (a NaN parameter: a NaN row)
        return [np.array([[float(self.exact(r, c, j)) if fine else np.nan for j in range(self.nb)] for r, fine in zip(rows, ok)])
                for c in range(3)]

    def slope(self, c, j, f, a, b):
        return Fraction(self.beta[c, j, f]) + Fraction(self.gamma[c, j, f]) * (Fraction(a) + Fraction(b))


def toy_case(seed=0, M=10, nb=5):
    """F = 3 on columns 15, 0, 2 with bounds of different scales; rows 0 .. 2 interior, 3 exactly on lo, 4 exactly on hi, 5 / 6
    outside on either side, 7 within h of hi, the rest interior"""
    rng = np.random.default_rng(seed)
    free = [15, 0, 2]
    lo, hi = np.array([0.1, 10.0, 0.005]), np.array([7.0, 80.0, 0.05])
    base = rng.uniform(0.0, 1.0, (M, 27))
    base[:, free] = lo + rng.uniform(0.05, 0.95, (M, 3)) * (hi - lo)
    base[3, free] = lo
    base[4, free] = hi
    base[5, free] = hi + 0.3 * (hi - lo)
    base[6, free] = lo - 2.0 * (hi - lo)
    base[7, free] = hi - 0.5e-3 * (hi - lo)
    return base, free, lo, hi, Toy(free, nb, seed + 1)


@pytest.mark.parametrize("subset", [(0,), (2,), (0, 1), (0, 1, 2)])
def test_the_definition_is_the_analytic_gradient_of_a_quadratic(subset):
    """|grad - G| <= ((n + 2) eps sum|g| max|Y|) / (a - b) + 2 eps |G| with eps = 2^-52, n = nb x columns terms and
    G = sum g (beta + gamma (a + b)) in exact rationals.  Where it comes from, with u = eps / 2 the unit roundoff: each Y is
    its exact value rounded once, |error| <= u max|Y|, so a difference d = Y+ - Y- is off by 2 u max|Y| from the two Y and by
    u |d| <= 2 u max|Y| from its own rounding: 2 eps max|Y| in all, sum|g| times that over a row.  A product g d and each of
    the n - 1 additions after it round once more, n u relative to the partial sums, which sum|g d| <= 2 sum|g| max|Y| bounds:
    n eps sum|g| max|Y|.  Together (n + 2) eps sum|g| max|Y| on s, divided by a - b.  The rounding of a - b and the division
    are two more relative errors of u on the result: 2 eps |G| covers them with the second-order terms."""
    base, free, lo, hi, toy = toy_case(seed=3 + len(subset))
    rng = np.random.default_rng(9)
    M, F, nb = base.shape[0], 3, toy.nb
    gy = [rng.normal(size=(M, nb)) if c in subset else None for c in range(3)]
    grad = vd.vjp_defined(base, free, lo, hi, gy, toy.forward, rel_step=1e-3)
    x = vd.clip_defined(base[:, free], lo, hi)
    a, b = vd.steps_defined(x, lo, hi, 1e-3)
    assert (a[3] - b[3] == a[3] - lo).all() and (b[4] == x[4] - 1e-3 * (hi - lo)).all() and (a[4] == hi).all()       # one-sided on a bound
    assert (x[5] == hi).all() and (x[6] == lo).all() and (a[7] == hi).all() and (b[0] < x[0]).all() and (x[0] < a[0]).all()
    Y = toy.forward(vd.rows_defined(base, free, x, a, b).reshape(-1, 27))
    ymax = max(np.abs(Y[c]).max() for c in subset)
    n = nb * len(subset)
    worst = 0.0
    for m in range(M):
        for f in range(F):
            G = sum(Fraction(gy[c][m, j]) * toy.slope(c, j, f, a[m, f], b[m, f]) for c in subset for j in range(nb))
            sg = sum(np.abs(gy[c][m]).sum() for c in subset)
            bound = ((n + 2) * EPS * sg * ymax) / (a[m, f] - b[m, f]) + 2 * EPS * abs(float(G))
            worst = max(worst, abs(float(Fraction(grad[m, f]) - G)) / bound)
            # in the interior the midpoint is x up to the rounding of x +- h: the analytic derivative AT x is met as well
            if m < 3:
                at_x = sum(Fraction(gy[c][m, j]) * toy.slope(c, j, f, x[m, f], x[m, f]) for c in subset for j in range(nb))
                assert abs(float(G - at_x)) <= 4 * EPS * max(abs(x[m, f]), 1.0) * float(sum(abs(Fraction(gy[c][m, j]) * Fraction(toy.gamma[c, j, f])) for c in subset for j in range(nb)))
    print(f"vjp definition against the analytic gradient, columns {subset}: worst |difference| / bound = {worst:.3e}")
    assert 0.0 < worst <= 1.0, worst


def test_consequences_on_the_toy_model():
    base, free, lo, hi, toy = toy_case(seed=11)
    rng = np.random.default_rng(2)
    M, nb = base.shape[0], toy.nb
    gy = [rng.normal(size=(M, nb)), None, rng.normal(size=(M, nb))]
    ref = vd.vjp_defined(base, free, lo, hi, gy, toy.forward)
    # a zero block is NULL; a row does not depend on its batch; a permutation of the batch permutes the rows
    assert same(vd.vjp_defined(base, free, lo, hi, [gy[0], np.zeros((M, nb)), gy[2]], toy.forward), ref)
    assert same(vd.vjp_defined(base[4:5], free, lo, hi, [gy[0][4:5], None, gy[2][4:5]], toy.forward), ref[4:5])
    p = rng.permutation(M)
    assert same(vd.vjp_defined(base[p], free, lo, hi, [gy[0][p], None, gy[2][p]], toy.forward), ref[p])
    # a zero g skips its band whatever Y holds there; a NaN g or parameter reaches its own row alone
    g0 = gy[0].copy()
    g0[:, 1] = 0.0

    def nan_band(rows):
        Y = toy.forward(rows)
        Y[0][:, 1] = np.nan
        return Y
    assert same(vd.vjp_defined(base, free, lo, hi, [g0, None, None], nan_band), vd.vjp_defined(base, free, lo, hi, [g0, None, None], toy.forward))
    g0[2, 0] = np.nan
    b2 = base.copy()
    b2[8, free[1]] = np.nan
    got = vd.vjp_defined(b2, free, lo, hi, [g0, None, None], toy.forward)
    assert np.isnan(got[2]).all() and np.isnan(got[8]).all() and np.isfinite(np.delete(got, [2, 8], axis=0)).all()
    # permuting the free columns permutes the gradient
    q = [2, 0, 1]
    assert same(vd.vjp_defined(base, [free[i] for i in q], lo[q], hi[q], gy, toy.forward), ref[:, q])


# ---- the g++ build of the per-entry functions
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vjp_host") / "libvjp_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *GXX, "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.vjh_chunk.restype = ctypes.c_int64
    L.vjh_max_rel_step.restype = L.vjh_rel_step.restype = ctypes.c_double
    L.vjh_step.argtypes = [ctypes.c_double] * 4 + [c_dp] * 2
    L.vjh_grad.argtypes = [ctypes.c_int] * 3 + [c_dp] * 6 + [ctypes.c_int, c_dp]
    return L


@pytest.mark.parametrize("nb", [1, 13, 17, 211])
@pytest.mark.parametrize("F", [1, 2, 6, 16])
def test_the_gxx_build_is_the_definition(lib, F, nb):
    W = lib.vjh_group(F)
    M = W + 3                                             # a whole group and a short one
    rng = np.random.default_rng(100 * F + nb)
    Yp, Ym = rng.normal(size=(3, F, M, nb)), rng.normal(size=(3, F, M, nb))
    den = 1e-3 * (1.0 + rng.random((M, F)))
    for subset in ((0, 1, 2), (1,), (0, 2)):
        gy = [rng.normal(size=(M, nb)) if c in subset else None for c in range(3)]
        zero = rng.random((M, nb)) < 0.3
        c0 = subset[0]
        gy[c0][zero] = 0.0
        gy[c0][0, 0] = 0.0
        yp = Yp.copy()
        yp[c0][:, gy[c0] == 0.0] = np.nan                  # NaN Y under a zero g
        yp[c0][0, 0, 0] = np.inf
        if len(subset) > 1:
            gy[subset[-1]][M - 1, nb - 1] = np.nan         # a NaN g: its row alone
        with np.errstate(all="ignore"):
            want = vd.sum_defined(gy, [yp[c] if c in subset else None for c in range(3)], [Ym[c] if c in subset else None for c in range(3)]) / den
        got = np.full((M, F), -1.0)
        lib.vjh_grad(M, F, nb, dp(gy[0]), dp(gy[1]), dp(gy[2]), dp(np.ascontiguousarray(yp)), dp(Ym), dp(den), W, dp(got))
        assert same(got, want), (F, nb, subset)
        finite = np.isfinite(want).all(axis=1)
        assert finite[:M - 1].all() and (len(subset) == 1 or not finite[M - 1])
        # the group width does not enter the result
        other = np.full((M, F), -1.0)
        lib.vjh_grad(M, F, nb, dp(gy[0]), dp(gy[1]), dp(gy[2]), dp(np.ascontiguousarray(yp)), dp(Ym), dp(den), 4, dp(other))
        assert same(other, want)


def test_the_steps_and_the_constants_are_the_definitions(lib):
    a, b = ctypes.c_double(), ctypes.c_double()
    for lo, hi in ((0.1, 7.0), (-0.5, 0.5), (950.0, 1030.0), (0.0, 1e-3)):
        for rel in (1e-3, 0.5, 1e-9):
            h = rel * (hi - lo)
            for x in (lo, hi, lo + h, hi - h, lo + 0.5 * h, hi - 0.5 * h, 0.5 * (lo + hi), lo - 1.0, hi + 1.0, np.nan, np.inf, -np.inf):
                lib.vjh_step(x, h, lo, hi, ctypes.byref(a), ctypes.byref(b))
                wa, wb = vd.steps_defined(vd.clip_defined(np.array([[x]]), lo, hi), np.array([lo]), np.array([hi]), rel)
                assert same(a.value, wa[0, 0]) and same(b.value, wb[0, 0]), (lo, hi, rel, x)
                if not np.isnan(x):
                    # a - b >= h but for the rounding of x + h and x - h, half an ulp of the larger bound each
                    assert a.value - b.value >= h - EPS * max(abs(lo), abs(hi)) > 0, (lo, hi, rel, x)
    assert lib.vjh_chunk(1) == vd.chunk_of(1) == 1 << 18 and lib.vjh_chunk(16) == vd.chunk_of(16) == 16384 and lib.vjh_chunk(6) == vd.chunk_of(6) == 43690
    assert lib.vjh_max_rel_step() == vd.MAX_REL_STEP == 0.5 and lib.vjh_rel_step() == vd.REL_STEP == 1e-3
    assert [lib.vjh_group(F) for F in (1, 2, 3, 4, 5, 8, 9, 16)] == [64, 32, 16, 16, 8, 8, 4, 4]


def test_the_lds_layout_has_no_bank_conflicts(lib):
    """the rules csrc/spart_vjp.h states: a staging store of 16 consecutive lanes (one (f, o), jj = 0 .. 15) hits 16 distinct
    banks of the 32 a 64-bit store has (dword address mod 32, two dwords per lane); the adding lanes of a half wave read 32
    distinct doubles mod 32 (64 banks of 4 bytes); tiles do not overlap"""
    for F in range(1, 17):
        W = lib.vjh_group(F)
        FS, WP = lib.vjh_fstride(W), W + 1
        assert W * F <= 64 and FS >= 16 * WP
        for o in range(W):
            assert len({(2 * (jj * WP + o)) % 32 for jj in range(16)}) == 16, (F, W, o)
        for half in (0, 32):
            lanes = [l for l in range(half, half + 32) if l // W < F]
            assert len({((l // W) * FS + l % W) % 32 for l in lanes}) == len(lanes), (F, W, half)


def test_the_functions_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """the .cpp's own main (F = 1, 2, 6, 16, nb = 1, 13, 17, 211, heap buffers of exact size, the staging tile of exactly the
    kernel's LDS size) as a stand-alone -fsanitize=address,undefined program in a child process; the sanitizer runtimes are
    linked into the program itself, so nothing is preloaded and nothing sanitised is loaded into python"""
    exe = str(tmp_path / "vjp_asan")
    subprocess.check_call(["g++", "-O1", "-g", *GXX, "-DVJP_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "WRONG" not in r.stdout and r.stdout.count(" ok") == 4 * 4 and "Sanitizer" not in r.stderr


# ---- refusals
@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    from spart_amd import _lib
    L = ctypes.CDLL(build.build(verbose=False))
    for name in ("spart_vjp", "spart_vjp_workspace_bytes"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
    L.spart_last_error.restype = ctypes.c_char_p
    return L


def test_null_context_is_refused_without_a_gpu(capi):
    assert capi.spart_vjp_workspace_bytes(None, 1, 3) == 0
    assert capi.spart_vjp(None, 0, None, 0, None, None, None, None, None, None, None, 0, None) == -1
    assert b"spart_vjp: null context" in capi.spart_last_error(None)


def test_every_refusal_in_its_order(capi):
    """A block of zeros stands for the context: no check before SPART_ERR_NOSENSOR reads anything of a context but its band
    count, which is 0 there, so the list ends with that refusal; nothing is launched and no pointer but the host arrays is
    followed.  (NOSENSOR on a real context and the workspace's size are tests/test_gpu_vjp.py's.)"""
    from spart_amd import _lib
    ctx = ctypes.create_string_buffer(1 << 20)
    host = np.zeros(64)                                              # what the never-followed device pointers point at
    fake = host.ctypes.data
    ok = dict(M=2, F=2, free=[15, 0], lo=[0.1, 10.0], hi=[7.0, 80.0], opt=(0, 0, 0, 0.0), gy=[fake, None, None], grad=fake,
              base=[fake] * 27)

    def call(null=(), **kw):
        a = dict(ok, **kw)
        fc, lo, hi = np.array(a["free"], dtype=np.int32), np.array(a["lo"], dtype=np.float64), np.array(a["hi"], dtype=np.float64)
        opt = _lib.SpartVjpOpt(*a["opt"])
        ptr = lambda name, v: None if name in null else v     # noqa: E731
        rc = capi.spart_vjp(ctypes.addressof(ctx), a["M"], ptr("base", (_lib.vp * 27)(*a["base"])), a["F"],
                            ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), ptr("lo", dp(lo)), ptr("hi", dp(hi)),
                            ptr("gy", (_lib.vp * 3)(*a["gy"])), ptr("opt", ctypes.byref(opt)), a["grad"], None, 0, None)
        return rc, capi.spart_last_error(None).decode()

    ladder = [("F = 0", dict(F=0)), ("F = 17", dict(F=17)), ("null argument", dict(null=("free",))), ("null argument", dict(null=("lo",))),
              ("null argument", dict(null=("hi",))), ("nlayers = -1", dict(opt=(0, 0, -1, 0.0))), ("free_cols[1] = 27", dict(free=[15, 27])),
              ("free twice", dict(free=[15, 15])), ("bounds of free_cols[0]", dict(lo=[np.nan, 1.0])),
              ("bounds of free_cols[1]", dict(lo=[0.1, 80.0])), ("opt is null", dict(null=("opt",))), ("band_model = 2", dict(opt=(2, 0, 0, 0.0))),
              ("rel_step = -1", dict(opt=(0, 0, 0, -1.0))), ("rel_step = nan", dict(opt=(0, 0, 0, np.nan))),
              ("rel_step = inf", dict(opt=(0, 0, 0, np.inf))), ("rel_step = 0.6", dict(opt=(0, 0, 0, 0.6))), ("gy is null", dict(null=("gy",))),
              ("every entry of gy is null", dict(gy=[None] * 3)), ("exactly one entry of gy, 2 given", dict(opt=(1, 0, 0, 0.0), gy=[fake, None, fake])),
              ("grad is null", dict(grad=None)), ("M = -1", dict(M=-1)), ("M = 2000000001", dict(M=2000000001)),
              ("base is null", dict(null=("base",))), ("base[3] is null", dict(base=[fake] * 3 + [None] + [fake] * 22 + [None]))]
    for text, kw in ladder:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg and msg.startswith("spart_vjp: "), (text, rc, msg)
    # the order: with everything wrong at once, mending the refusals one by one meets them in the header's order
    wrong = dict(F=0, opt=(2, 0, -1, -1.0), free=[27, 0], lo=[0.1, np.nan], gy=[fake, fake, fake], grad=None, M=-1, base=[None] * 27)
    mend = [("F", ok["F"]), ("opt", (2, 0, 0, -1.0)), ("free", ok["free"]), ("lo", ok["lo"]), ("opt", (1, 0, 0, -1.0)),
            ("opt", (1, 0, 0, 0.5)), ("gy", ok["gy"]), ("grad", fake), ("M", 2), ("base", ok["base"])]
    seen = []
    for key, value in mend:
        rc, msg = call(**wrong)
        assert rc == -1
        seen.append(msg)
        wrong[key] = value
    for msg, text in zip(seen, ("F = 0", "nlayers = -1", "free_cols[0] = 27", "bounds of free_cols[1]", "band_model = 2",
                                "rel_step = -1", "exactly one entry of gy, 3 given", "grad is null", "M = -1", "base[0] is null")):
        assert text in msg, (text, seen)
    # a NULL opt comes after the free columns and ahead of everything the options and the device pointers can get wrong
    assert "free twice" in call(null=("opt",), free=[15, 15])[1]
    assert "opt is null" in call(null=("opt", "gy"), grad=None, M=-1)[1]
    # the largest step is taken; NULL base with M = 0 is no refusal of its own; the list ends at the sensor
    for kw in (dict(), dict(opt=(0, 1, 60, 0.5)), dict(M=0, null=("base",))):
        rc, msg = call(**kw)
        assert rc == -4 and "no sensor" in msg, (kw, msg)
    assert capi.spart_vjp_workspace_bytes(ctypes.addressof(ctx), 2, 2) == 0


def test_vjp_arguments_are_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    P = workloads.lhs_params(3, "full", seed=1).T
    g = np.zeros((3, 13))
    ok = dict(grad_outputs={"R_TOC": g}, free=["LAI", "Cab"])
    for kw, text in ((dict(ok, free=["nope"]), "unknown"), (dict(ok, free=["LAI", "LAI"]), "twice"), (dict(ok, free=[]), "0 names"),
                     (dict(ok, bounds={"LAI": (3.0, 3.0)}), "lo < hi"), (dict(ok, bounds={"Cw": (0.0, 1.0)}), "not free"),
                     (dict(ok, rel_step=0.0), "rel_step"), (dict(ok, rel_step=0.6), "rel_step"), (dict(ok, rel_step=np.nan), "rel_step"),
                     (dict(ok, rel_step=-1e-3), "rel_step"), (dict(ok, band_model="wide"), "band_model"), (dict(ok, lidf="x"), "lidf"),
                     (dict(ok, grad_outputs={"rso": g}), "unknown column"), (dict(ok, grad_outputs={}), "0 names"),
                     (dict(ok, grad_outputs=g), "dict"), (dict(ok, grad_outputs={"R_TOC": None}), "every entry is None"),
                     (dict(ok, grad_outputs={"R_TOC": g, "R_TOA": g}, band_model="srf"), "one column per call"),
                     (dict(ok, grad_outputs={"R_TOC": g[0]}), "has shape"), (dict(ok, grad_outputs={"R_TOC": g, "L_TOA": g[:, :12]}), "like the others"),
                     (dict(ok, grad_outputs={"R_TOC": np.zeros((2, 13))}), "broadcast"), (dict(ok, nlayers=0), "nlayers")):
        with pytest.raises((ValueError, TypeError), match=text):
            spart_amd.vjp(P, sensor=S2, **kw)
    e = engine.Engine.__new__(engine.Engine)                   # an Engine object that never saw a device
    e.nb = 13
    with pytest.raises(ValueError, match="expected \\(M, nb\\) = \\(M, 13\\)"):
        e.vjp(P, {"R_TOC": np.zeros((3, 12))}, ["LAI"])
    with pytest.raises(ValueError, match="unknown"):
        e.vjp(P, {"R_TOC": g}, ["nope"])
    plan, params, M, gys = engine.vjp_args(P, {"L_TOA": g, "R_TOC": None}, ["LAI", "DOY"], {"DOY": (1, 365)}, 0.5, "newton", "srf", nb=13)
    assert (M, plan["names"], plan["cols"].tolist(), plan["rel_step"]) == (3, ["LAI", "DOY"], [15, 26], 0.5)
    assert gys[0] is None and gys[1] is None and gys[2] is g and len(params) == 27


def test_layer_arguments_are_checked_before_the_gpu_is_asked_for():
    import torch

    import spart_amd
    ok = dict(sensor=S2, free=["LAI", "Cab"])
    for kw, text in ((dict(ok, free=["nope"]), "unknown"), (dict(ok, free=["LAI", "LAI"]), "twice"), (dict(ok, rel_step=0.7), "rel_step"),
                     (dict(ok, rel_step=0), "rel_step"), (dict(ok, columns=("R_TOC", "R_TOA"), band_model="srf"), "one column per call"),
                     (dict(ok, columns=("R_TOC", "R_TOC")), "twice"), (dict(ok, columns=("rdd",)), "unknown column"), (dict(ok, columns=()), "0 names"),
                     (dict(ok, band_model="wide"), "band_model"), (dict(ok, lidf="x"), "lidf"), (dict(ok, nlayers=1.5), "nlayers"),
                     (dict(ok, bounds={"LAI": (1.0, np.inf)}), "lo < hi")):
        with pytest.raises((ValueError, TypeError), match=text):
            spart_amd.SpartLayer(**kw)
    layer = spart_amd.SpartLayer(S2, ["LAI", "Cab"], bounds={"LAI": (0.5, 6.0)}, columns=("R_TOC", "L_TOA"))
    assert isinstance(layer, torch.nn.Module) and layer.names == ["LAI", "Cab"] and layer.columns == ("R_TOC", "L_TOA")
    assert layer.lo.tolist() == [0.5, 10.0] and layer.hi.tolist() == [6.0, 80.0] and layer.lo.dtype == torch.float64
    u = torch.tensor([[0.0, 1.0], [0.5, 0.25]], dtype=torch.float32, requires_grad=True)
    x = layer.from_unit(u)
    assert x.dtype == torch.float32 and x.tolist() == [[0.5, 80.0], [3.25, 27.5]]
    x.sum().backward()
    assert u.grad.tolist() == [[5.5, 70.0]] * 2
    assert not list(layer.parameters()) and "lo" not in layer.state_dict()


def test_signatures_struct_and_header_agree():
    from spart_amd import _lib
    assert [f[0] for f in _lib.SpartVjpOpt._fields_] == ["band_model", "fast_prelude", "nlayers", "rel_step"]
    assert [f[1] for f in _lib.SpartVjpOpt._fields_] == [ctypes.c_int32] * 3 + [ctypes.c_double]
    assert ctypes.sizeof(_lib.SpartVjpOpt) == 24 and _lib.SpartVjpOpt.rel_step.offset == 16
    res, args = _lib.SIGNATURES["spart_vjp"]
    ref = list(_lib.SIGNATURES["spart_refine"][1])
    assert res is ctypes.c_int and len(args) == 13 and args[:7] == ref[:7] and args[10:] == ref[16:]
    assert args[7]._type_ is _lib.vp and args[8]._type_ is _lib.SpartVjpOpt and args[9] is _lib.vp
    res, args = _lib.SIGNATURES["spart_vjp_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [_lib.vp, ctypes.c_int64, ctypes.c_int]
    full = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    body = re.search(r"typedef struct spart_vjp_opt \{(.*?)\} spart_vjp_opt;", header, flags=re.S).group(1)
    assert re.findall(r"\b(int32_t|double)\s+([A-Za-z_0-9]+)\s*;", body) == [("int32_t", "band_model"), ("int32_t", "fast_prelude"),
                                                                              ("int32_t", "nlayers"), ("double", "rel_step")]
    assert re.search(r"int spart_vjp\(spart_ctx \*ctx, int64_t M, const double \*const base\[SPART_NPARAM\], int F,\s*const int32_t "
                     r"\*free_cols\s*, const double \*lo, const double \*hi\s*,\s*const double \*const gy\[3\]\s*,\s*"
                     r"const spart_vjp_opt \*opt, double \*grad\s*,\s*void \*workspace, size_t workspace_bytes, void \*stream\);", header)
    assert "size_t spart_vjp_workspace_bytes(const spart_ctx *ctx, int64_t M, int F);" in header
    assert "#define SPART_ABI_VERSION 14" in full and "spart_vjp and spart_vjp_workspace_bytes" in full and _lib.ABI_VERSION == 14
    assert _lib.VJP_MAX_REL_STEP == vd.MAX_REL_STEP
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_vjp.h")).read()
    assert "constexpr double VJP_REL_STEP = 1e-3, VJP_MAX_REL_STEP = 0.5;" in src and "constexpr int VJP_ROWS = REFINE_ROWS;" in src
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    assert any(d.endswith("spart_vjp.h") for d in build.DEPS)
    import spart_amd
    assert callable(spart_amd.vjp) and callable(spart_amd.Engine.vjp) and spart_amd.SpartLayer.__module__ == "spart_amd.autograd"
