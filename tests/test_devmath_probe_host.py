"""What tests/test_gpu_devmath.py rests on, checked without a GPU: the probe of the device math (tests/devmath/
devmath_probe.hip) compiles for gfx950 with the product's flags and reports the SPART_FAST_MATH build, and the
np.longdouble expressions that the GPU tests use as references agree with mpmath (200 bits) to 1e-18 relative over those
tests' own ranges."""
import ctypes
import os
import re

import numpy as np
import pytest

import build as B
from helpers import devmath_probe as D

LD = np.longdouble


def test_probe_builds_for_gfx950_with_the_product_flags():
    if not D.have_hipcc():
        pytest.skip("hipcc not available")
    for dtype, unit in ((1, "spart_capi.hip"), (0, "spart_bands_f32.hip")):
        assert D.flags(dtype) == B.tu_flags(os.path.join(B.CSRC, unit)) + ["-DSPART_FAST_MATH=1"]
        assert "--offload-arch=gfx950" in D.flags(dtype)
        so = D.build(dtype)
        assert os.path.exists(so) and open(so + ".hash").read().strip() == D.source_hash(dtype)
        assert D.build(dtype) == so                                          # (fresh now: no second compile)
        lib = ctypes.CDLL(so)
        assert lib.dm_fast_math() == 1
        data = open(so, "rb").read()
        assert b"gfx950" in data and all(s in data for s in (b"dm_unary", b"dm_binary", b"dm_plate_tau"))
        assert b"spart_ctx_create" not in data                               # no symbol of the product's C ABI
    assert (D.lib_path(0) == D.lib_path(1)) == (D.flags(0) == D.flags(1))    # one library exactly while the flag lists agree
    # the function ids are those of the probe's enums, in order
    src = open(D.SRC).read()
    for first, end, ids in (("F_EXP = 0", "F_UNARY_END", D.UNARY), ("B_DIVX = 0", "B_END", D.BINARY)):
        names = re.findall(r"\b[FB]_([A-Z0-9_]+)\b", src[src.index(first):src.index(end)])
        assert names == [n.upper() for n in ids] and list(ids.values()) == list(range(len(ids)))


def test_long_double_references_agree_with_mpmath():
    mp = pytest.importorskip("mpmath")
    assert np.finfo(LD).nmant >= 63
    mp.mp.prec = 200
    rng = np.random.default_rng(0)
    n = 3000
    pos = 10.0 ** rng.uniform(-300, 300, n)
    z = np.concatenate([10.0 ** rng.uniform(-12, np.log10(700.0), n // 2), -(10.0 ** rng.uniform(-12, np.log10(700.0), n // 2))])
    cases = [
        ("exp", np.exp, mp.exp, rng.uniform(-745.0, 700.0, n)),
        ("exp2", np.exp2, lambda v: mp.power(2, v), rng.uniform(-1022.0, 1000.0, n)),
        ("log", np.log, mp.log, np.concatenate([2.0 ** rng.uniform(-1022, 1023.9, n // 2), 1.0 + 10.0 ** rng.uniform(-16, -1, n // 4),
                                                1.0 - 10.0 ** rng.uniform(-16, -1, n // 4)])),
        ("sqrt", np.sqrt, mp.sqrt, pos),
        ("1/x", lambda v: 1 / v, lambda v: 1 / v, pos * rng.choice([-1.0, 1.0], n)),
        ("log1p", np.log1p, mp.log1p, np.concatenate([10.0 ** rng.uniform(-12, 6, n), [1e30]])),
        ("-expm1(-z)", lambda v: -np.expm1(-v), lambda v: -mp.expm1(-v), z),
    ]
    for name, f, g, x in cases:
        got = f(x.astype(LD))
        m, e = np.frexp(got)                                 # (the mantissa apart: a result may lie below float64's range)
        worst = 0.0
        for xi, mi, ei in zip(x, m, e):
            want = g(mp.mpf(float(xi)))
            if want == 0:                                    # (log at 1 + 1e-16 == 1)
                assert mi == 0, name
                continue
            hi = float(mi)                                   # a long double mantissa as the exact sum of two float64
            lo = float(mi - LD(hi))
            worst = max(worst, float(abs((mp.ldexp(mp.mpf(hi) + mp.mpf(lo), int(ei)) - want) / want)))
        print(f"[devmath] np.longdouble {name} against mpmath: {worst:.2e}")
        assert worst < 1e-18, name
