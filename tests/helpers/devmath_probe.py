"""Builds and loads tests/devmath/libdevmath_probe.so: the device branches of csrc/spart_math.h, function by function
(tests/devmath/devmath_probe.hip), compiled with the product's own flags and SPART_FAST_MATH.

The float64 functions take the flags of csrc/spart_capi.hip and the float32 ones those of csrc/spart_bands_f32.hip, the units
that run them in the product.  While the two lists are equal one library serves both; when they differ, two are built.

Staleness is a content hash of the probe, the three headers it reads and the flag lists, kept next to the library (not
modification times: see build.needs_build).  Several processes may build at once: each links under its own name and renames.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess

import build as B
import pytest

from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "devmath")
SRC = os.path.join(DIR, "devmath_probe.hip")
DEPS = [SRC] + [os.path.join(B.CSRC, f) for f in ("spart_math.h", "spart_e3_coeffs.h", "spart_f64_tables.h")]
UNIT = {1: "spart_capi.hip", 0: "spart_bands_f32.hip"}     # dtype (1 = float64, 0 = float32) -> the unit whose flags it takes

# function ids of devmath_probe.hip
UNARY = {n: i for i, n in enumerate(("exp", "exp2", "exp_poly", "log", "log2", "sqrt", "rcp", "log1p", "log2_1p", "omen", "omen_ez",
                                     "omen_poly", "omen2_e", "rcp_seed", "rsq_seed"))}
BINARY = {n: i for i, n in enumerate(("divx", "j1_d", "j1_a", "j2_d"))}


def flags(dtype):
    return B.tu_flags(os.path.join(B.CSRC, UNIT[dtype])) + ["-DSPART_FAST_MATH=1"]


def lib_path(dtype):
    """one library while both units compile with the same flags, one per type otherwise"""
    return os.path.join(DIR, "libdevmath_probe.so" if flags(0) == flags(1) else f"libdevmath_probe_f{64 if dtype else 32}.so")


def source_hash(dtype):
    h = hashlib.sha256()
    for d in DEPS:
        h.update(os.path.basename(d).encode() + b"\0" + open(d, "rb").read())
    h.update((" ".join(flags(dtype)) + "|" + " ".join(B.LDFLAGS)).encode())
    return h.hexdigest()


def have_hipcc():
    return any(c and os.path.exists(c) for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")))     # (helpers/compiled_meta's rule)


def build(dtype, force=False):
    """the path of an up-to-date library for dtype, compiled here if the one in the tree is missing or stale"""
    out, want = lib_path(dtype), source_hash(dtype)
    stamp = out + ".hash"
    try:
        fresh = os.path.exists(out) and open(stamp).read().strip() == want
    except OSError:
        fresh = False
    if fresh and not force:
        return out
    tmp = f"{out}.tmp.{os.getpid()}"
    try:
        # source -> shared library in one hipcc call: no object file is left anywhere
        subprocess.check_call([B.hipcc(), *flags(dtype), *B.LDFLAGS, "-o", tmp, SRC])
        os.replace(tmp, out)
        with open(f"{stamp}.tmp.{os.getpid()}", "w") as f:
            f.write(want + "\n")
        os.replace(f.name, stamp)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return out


def load(dtype):
    if not have_hipcc() and not os.path.exists(lib_path(dtype)):
        pytest.skip("hipcc not available")
    lib = ctypes.CDLL(build(dtype))
    vp, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    lib.dm_fast_math.restype = i
    for fn, args in ((lib.dm_unary, [i, i, vp, vp, ll, i]), (lib.dm_binary, [i, i, vp, vp, vp, ll, i]), (lib.dm_plate_tau, [i, vp, vp, vp, ll, i])):
        fn.restype, fn.argtypes = i, args
    return lib
