"""What the leaf-fit tests share (tests/test_refine_leaf_host.py, tests/test_refine_leaf_defined.py,
tests/test_gpu_refine_leaf.py): the g++ harness tests/hostmath/refine_leaf_host.cpp behind two functions, the free columns and
bounds of the cases, and the 24 / 64 leaves they fit."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import refine_leaf_defined as rld  # noqa: E402

from spart_amd import workloads  # noqa: E402

NWL = 2001
LEAF_NAMES = list(workloads.PARAM_NAMES[:9])
SRC = os.path.join(ROOT, "tests", "hostmath", "refine_leaf_host.cpp")
HDRS = [os.path.join(ROOT, "spart-python_amd", "csrc", h) for h in ("spart_refine_leaf.h", "spart_refine.h", "spart_math.h")]
FREE = {1: ["N"], 4: ["Cab", "Cw", "Cdm", "N"], 7: ["Cab", "Cdm", "Cw", "Cs", "Cca", "Cant", "N"], 9: LEAF_NAMES}


def free_cols(F):
    return [LEAF_NAMES.index(n) for n in FREE[F]]


def bounds(F):
    lo, hi = (np.array([workloads.RANGES[n][k] for n in FREE[F]], dtype=np.float64) for k in (0, 1))
    return lo, hi


def leaves(M, seed):
    """(M, 9) PROSPECT-5D leaves of BASELINE config 2's design"""
    return np.ascontiguousarray(workloads.lhs_params(M, "leaf", seed=seed)[:, :9])


def build_harness(exe, sanitize=False):
    """g++ -> exe; with ``sanitize`` under AddressSanitizer and UBSan (a stand-alone program: nothing is preloaded).
    -> None, or the compiler's complaint when it cannot link a sanitizer runtime"""
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1"]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    p = subprocess.run(cmd + ["-o", exe, SRC], capture_output=True, text=True)
    if p.returncode != 0:
        if sanitize and ("asan" in p.stderr or "ubsan" in p.stderr or "sanitize" in p.stderr):
            return p.stderr.strip().splitlines()[-1]
        raise RuntimeError(p.stderr)
    return None


def raw_tables(tables):
    return np.concatenate([np.asarray(tables[k], dtype=np.float64).reshape(NWL) for k in
                           ("nr", "Kab", "Kca", "Kdm", "Kw", "Ks", "Kant", "cbc", "prot")])


def _run(exe, mode, workdir, words, arrays, outs):
    src, dst = os.path.join(workdir, "in.bin"), os.path.join(workdir, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array(words, dtype="<i8").tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    p = subprocess.run([exe, mode, src, dst], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    flat = np.fromfile(dst, dtype="<f8")
    res, at = [], 0
    for shape in outs:
        n = int(np.prod(shape))
        res.append(flat[at:at + n].reshape(shape))
        at += n
    assert at == flat.size
    return res


def host_spectra(exe, workdir, raw, rows):
    """leaf_band<double> of the g++ build: rows (R, 9) -> (refl, tran), each (R, 2001)"""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    R = rows.shape[0]
    return tuple(_run(exe, "spectra", workdir, [R], [raw, rows], [(R, NWL), (R, NWL)]))


def host_fit(exe, workdir, raw, leaf, free, lo, hi, obs_refl, obs_tran, w_refl=None, w_tran=None, n_iter=20, rel_step=1e-3,
             lambda0=1e-2, prior_mean=None, prior_weight=None):
    """part 1 of csrc/spart_refine_leaf.h over 64 emulated lanes -> dict like refine_leaf_defined's (no spectra)"""
    M, F = leaf.shape[0], len(free)

    def mode(a, width):
        return 0 if a is None else 1 if np.shape(a) == (width,) else 2
    words = [M, F, n_iter, obs_refl is not None, obs_tran is not None, mode(w_refl, NWL), mode(w_tran, NWL), mode(prior_mean, F)]
    arrays = [raw, leaf, np.array(free, dtype=np.float64), lo, hi, np.array([rel_step, lambda0])]
    arrays += [a for a in (obs_refl, obs_tran, w_refl, w_tran, prior_mean, prior_weight) if a is not None]
    x, cost, cost0, std, na = _run(exe, "fit", workdir, [int(w) for w in words], arrays, [(M, F), (M,), (M,), (M, F), (M,)])
    return {"x": x, "cost": cost, "cost0": cost0, "std": std, "n_accept": na.astype(np.int32)}


def same_bits(a, b):
    """the same values bit for bit: equal numbers with equal signs (+0.0 is not -0.0); a NaN equals any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    num = ~np.isnan(a)
    return bool(np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[num]), np.signbit(b[num])))
