"""spart_sobol without a GPU: the definition tools/sobol_defined.py against scipy.stats.sobol_indices and the analytic Ishigami
indices, the g++ build of csrc/spart_sobol.h's per-entry functions against the definition bit for bit (and as a stand-alone
sanitizer program), the consequences the header states on a toy forward model, sobol_design, every refusal in its order, the
Python layer's checks, the agreement of signatures, structs and header, and the three kernels' resources."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from helpers.compiled_meta import kernel_meta_fixture  # noqa: F401  (the `kernel_meta` fixture)
from helpers.sobol_calls import OUTS, differing, same, sd

SRC = os.path.join(ROOT, "tests", "hostmath", "sobol_host.cpp")
EPS = 2.0 ** -52
c_dp = ctypes.POINTER(ctypes.c_double)
GXX = ["-std=c++17", "-ffp-contract=off", "-w", "-DSPART_FAST_MATH=1"]


def dp(a):
    return a.ctypes.data_as(c_dp)


# ---- the definition against scipy and the analytic indices
def ishigami(x):
    return np.sin(x[:, 0]) + 7.0 * np.sin(x[:, 1]) ** 2 + 0.1 * x[:, 2] ** 4 * np.sin(x[:, 0]) + 100.0


ISHIGAMI_S1 = (0.3139, 0.4424, 0.0)
ISHIGAMI_ST = (0.5576, 0.4424, 0.2437)


def ishigami_outputs(N):
    qmc = pytest.importorskip("scipy.stats.qmc")
    u = qmc.Sobol(6, scramble=True, seed=3).random(N)
    lo, hi = np.full(3, -np.pi), np.full(3, np.pi)
    xA, xB = sd.points_defined(u[:, :3], lo, hi), sd.points_defined(u[:, 3:], lo, hi)
    yA, yB = ishigami(xA)[:, None], ishigami(xB)[:, None]
    yC = np.empty((3, N, 1))
    for f in range(3):
        x = xA.copy()
        x[:, f] = xB[:, f]
        yC[f, :, 0] = ishigami(x)
    return yA, yB, yC


def against_scipy(yA, yB, yC, what):
    """|definition - scipy.stats.sobol_indices| on the same outputs, relative to 8 N eps kappa -> the worst ratio"""
    stats = pytest.importorskip("scipy.stats")
    N = yA.shape[0]
    res = sd.sobol_of_outputs(yA, yB, yC)
    ref = stats.sobol_indices(func={"f_A": yA.T.copy(), "f_B": yB.T.copy(), "f_AB": np.transpose(yC, (0, 2, 1)).copy()}, n=N)
    first, total = (np.reshape(v, res["S1"].shape) for v in (ref.first_order, ref.total_order))      # (s, d); scipy drops s = 1
    worst = 0.0
    for j in range(yA.shape[1]):
        y = np.concatenate([yA[:, j], yB[:, j]]) - yA[0, j]
        kappa = max(1.0, float(np.mean(y * y) / res["var"][j]))
        bound = 8 * N * EPS * kappa
        err = max(np.abs(res["S1"][j] - first[j]).max(), np.abs(res["ST"][j] - total[j]).max())
        worst = max(worst, err / bound)
    print(f"sobol definition against scipy, {what}: worst |difference| / (8 N eps kappa) = {worst:.3e}")
    return worst


@pytest.mark.parametrize("N", [128, 1024, 8192])
def test_the_definition_is_scipys_estimator_on_ishigami(N):
    worst = against_scipy(*ishigami_outputs(N), f"Ishigami + 100, N = {N}")
    assert 0.0 < worst <= 1.0, worst


def test_the_definition_is_scipys_estimator_on_the_oracle():
    import spart_oracle as O
    from spart_amd import workloads
    names = ["LAI", "Cab", "Cw"]
    free = [workloads.PARAM_NAMES.index(n) for n in names]
    lo, hi = (np.array([workloads.RANGES[n][k] for n in names], dtype=np.float64) for k in (0, 1))
    rng = np.random.default_rng(11)
    N = 128
    uA, uB = rng.random((N, 3)), rng.random((N, 3))
    T = sd.rows_defined(workloads.default_row()[0], free, sd.points_defined(uA, lo, hi), sd.points_defined(uB, lo, hi))
    with np.errstate(all="ignore"):
        y = O.spart_run(T, "Sentinel2A-MSI", pso="gl")["R_TOC"]
    worst = against_scipy(y[:N], y[N:2 * N], y[2 * N:].reshape(3, N, -1), "oracle R_TOC, F = 3, N = 128")
    assert 0.0 < worst <= 1.0, worst


def test_the_ishigami_indices_are_met_within_their_own_standard_errors():
    res = sd.sobol_of_outputs(*ishigami_outputs(8192))
    for key, want in (("S1", ISHIGAMI_S1), ("ST", ISHIGAMI_ST)):
        got, se = res[key][0], res[key + "_se"][0]
        print(f"Ishigami {key}: {got} +- {se} (analytic {want}; {np.abs(got - want) / se} se off)")
        assert (se > 0.0).all() and (se < 0.02).all(), (key, se)
        assert (np.abs(got - np.array(want)) <= 4.0 * se).all(), (key, got, se)


# ---- the g++ build of the per-entry functions
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sobol_host") / "libsobol_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *GXX, "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.sbh_point.restype = L.sbh_tree.restype = ctypes.c_double
    L.sbh_point.argtypes = [ctypes.c_double] * 3
    L.sbh_tree.argtypes = [c_dp, ctypes.c_int]
    L.sbh_site.argtypes = [ctypes.c_int] * 3 + [c_dp] * 3 + [ctypes.c_int] + [c_dp] * 6
    L.sbh_blocks.argtypes = [ctypes.c_int] * 3 + [c_dp] * 3 + [ctypes.c_int, c_dp, c_dp]
    L.sbh_entry.argtypes = [c_dp] + [ctypes.c_int] * 6 + [ctypes.c_double, ctypes.c_int, c_dp]
    return L


def random_outputs(N, F, nb, seed):
    """correlated outputs with an offset (so that the shift matters) and magnitudes spread over the bands"""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-3, 2, nb)
    yA = 50.0 + scale * rng.normal(size=(N, nb))
    yB = 50.0 + scale * rng.normal(size=(N, nb))
    mix = rng.random((F, 1, nb))
    yC = mix * yA + (1.0 - mix) * yB + 0.1 * scale * rng.normal(size=(F, N, nb))
    return yA, yB, yC


@pytest.mark.parametrize("stride", [1, 5])
@pytest.mark.parametrize("G", [2, 3, 64])
@pytest.mark.parametrize("F", [1, 3, 16])
def test_the_gxx_build_is_the_definition(lib, F, G, stride):
    N, nb = 64 * G, 4
    yA, yB, yC = random_outputs(N, F, nb, 100 * F + G)
    ref = sd.sobol_of_outputs(yA, yB, yC)
    got = {k: np.full(ref[k].shape, -7.0) for k in OUTS}
    lib.sbh_site(N, F, nb, dp(yA), dp(yB), dp(yC), stride, *[dp(got[k]) for k in OUTS])
    assert not differing(got, ref), differing(got, ref)
    assert np.isfinite(ref["S1_se"]).all() and (ref["S1_se"] > 0).all() and (ref["var"] > 0).all()
    # the block sums and the entry on their own: the (g, q, band) layout at this stride, and the call without the jackknife
    Q = 4 + 3 * F
    bs = np.full((G * Q * nb - 1) * stride + 1, np.nan)
    c = np.empty(nb)
    lib.sbh_blocks(N, F, nb, dp(yA), dp(yB), dp(yC), stride, dp(bs), dp(c))
    want = sd.blocks_defined(sd.terms_defined(yA, yB, yC)[1])                      # (Q, G, nb)
    assert same(bs[::stride].reshape(G, Q, nb), np.transpose(want, (1, 0, 2))) and same(c, yA[0])
    if stride > 1:
        rest = np.ones(bs.size, dtype=bool)
        rest[::stride] = False
        assert np.isnan(bs[rest]).all()
    out = np.full(6, -7.0)
    lib.sbh_entry(dp(bs), stride, G, F, nb, nb - 1, F - 1, c[nb - 1], 0, dp(out))
    assert same(out[:4], [ref[k][nb - 1] if k in ("mean", "var") else ref[k][nb - 1, F - 1] for k in OUTS[:4]]) and (out[4:] == -7.0).all()


def test_the_tree_and_the_point_are_the_definitions(lib):
    rng = np.random.default_rng(0)
    for k in range(20):
        t = rng.normal(size=64) * 10.0 ** rng.uniform(-8, 8, 64)
        want = sd.tree_defined(t[:, None])[0]
        assert lib.sbh_tree(dp(t), 1) == want == lib.sbh_tree(dp(t), 5)
    # the pairing, not any other: r + 32, then r + 16 ...
    t = np.zeros(64)
    t[0], t[32], t[16] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert lib.sbh_tree(dp(t), 1) == 1.0                       # (1 + 2^-53) rounds to 1 before the next half ulp arrives
    t = np.zeros(64)
    t[1], t[33], t[17] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert lib.sbh_tree(dp(t), 1) == sd.tree_defined(t[:, None])[0] == 1.0 and (t[33] + t[17]) + t[1] > 1.0
    for lo, hi, u in ((0.1, 7.0, 0.3), (-0.5, 0.5, 1.0 / 3.0), (950.0, 1030.0, 0.999999), (0.0, 1e-3, np.nan)):
        assert same(lib.sbh_point(lo, hi, u), sd.points_defined(u, lo, hi))
    assert lib.sbh_block() == 64 == sd.BLOCK and lib.sbh_nq(16) == 52 and lib.sbh_chunk_blocks(1) == 2730 and lib.sbh_chunk_blocks(16) == 455


def test_the_functions_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """the .cpp's own main (F = 1, 3, 16, G = 2, 3, 64, strides 1 and 5, heap buffers of exact size) as a stand-alone
    -fsanitize=address,undefined program in a child process; the sanitizer runtimes are linked into the program itself, so
    nothing is preloaded and nothing sanitised is loaded into python"""
    exe = str(tmp_path / "sobol_asan")
    subprocess.check_call(["g++", "-O1", "-g", *GXX, "-DSOBOL_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "WRONG" not in r.stdout and r.stdout.count(" ok") == 3 * 3 * 2 and "Sanitizer" not in r.stderr


# ---- the slots of the workspace: sobol_layout's rule, by brute force
def test_a_chunk_touches_at_most_nslot_sites_with_distinct_slots(lib):
    """csrc/spart_capi.hip, sobol_layout: "bc consecutive blocks touch at most bc / G + 2 sites", and a site's sums wait in slot
    m % nslot, nslot = min(M, bcap / G + 2).  Every launch of every call with F = 1 ... 16, G around the chunk's size and M up
    to three chunks' worth: the sites a launch touches (the one that entered from the launch before among them) are within
    the bound and have distinct slots; with one slot fewer, two of them share one in the cases listed, the shapes of
    tests/test_gpu_sobol_edges.py among them.  No GPU and no library but for sobol_chunk_blocks, which ROWS restates."""
    from helpers.sobol_calls import ROWS, chunk_blocks, chunks_of, layout_of
    assert ROWS == 1 << 19 and all(lib.sbh_chunk_blocks(F) == chunk_blocks(F) for F in range(1, 17))

    def shared_slot(F, N, M, nslot):
        return any(last - first + 1 > nslot for _, _, first, last in chunks_of(F, N, M))       # (consecutive m: distinct iff few enough)

    equal, checked = [], 0
    for F in range(1, 17):
        cb = chunk_blocks(F)
        for G in (2, 3, 5, 64, cb - 1, cb, cb + 1, 2 * cb + 1):
            if not sd.MIN_N <= 64 * G <= sd.MAX_N:
                continue
            for M in range(1, 3 * cb // G + 3):
                _, bcap, nslot = layout_of(F, 64 * G, M)
                launches = chunks_of(F, 64 * G, M)
                assert sum(bc for _, bc, _, _ in launches) == M * G and all(0 < bc <= bcap for _, bc, _, _ in launches)
                for b0, bc, first, last in launches:
                    touched = last - first + 1
                    assert touched <= min(M, bc // G + 2) <= nslot, (F, G, M, b0)
                    assert len({m % nslot for m in range(first, last + 1)}) == touched, (F, G, M, b0)
                    checked += 1
                if nslot < M and any(last - first + 1 == nslot for _, _, first, last in launches):
                    equal.append((F, G, M))
                    assert shared_slot(F, 64 * G, M, nslot - 1)
    per_F = {F: sum(1 for e in equal if e[0] == F) for F in range(1, 17)}
    print(f"{checked} launches checked; nslot < M met with equality in {len(equal)} calls (per F: {per_F}); the smallest M per (F, G):",
          sorted({(F, G): M for F, G, M in reversed(equal)}.items())[:12], "...")
    # the bound is met with equality where a launch begins with a site's last block(s) and ends with another's first:
    # G = 3 at F = 2 (2048 = 3 * 682 + 2) from M = 1366 on, so at test_gpu_sobol_edges' M = 1400; never at G = 2
    # (2048 is a multiple of 2: bc / G + 1 sites at most)
    assert (2, 3, 1400) in equal and (2, 3, 1366) in equal and (2, 3, 1365) not in equal and not any(e[:2] == (2, 2) for e in equal)
    # G > bcap (a site longer than a chunk): two slots, both in use in the launch that ends one site and begins the next
    assert layout_of(16, 29440, 3) == (460, 455, 2) and (16, 456, 3) in equal and (16, 911, 3) in equal
    # one slot fewer than the rule's, in the GPU tests' own shapes: two sites of one launch share a slot
    for F, N, M in ((2, 192, 1400), (16, 29440, 3)):
        nslot = layout_of(F, N, M)[2]
        assert nslot < M and not shared_slot(F, N, M, nslot) and shared_slot(F, N, M, nslot - 1), (F, N, M)
    # ... and not in any call of the suite before them: its calls have nslot = M or one site
    for F, N, M in ((2, 192, 684), (1, 1 << 18, 1), (3, 192, 3), (16, 128, 1)):
        assert layout_of(F, N, M)[2] == M


# ---- the consequences, on a toy forward model
NB = 5


def toy_forward(ignored=(), nan_band=None):
    """a smooth non-additive function of the 27 columns that does not read the ``ignored`` ones; with ``nan_band`` = (band, LAI
    threshold) a row above the threshold is NaN in that band"""
    rng = np.random.default_rng(42)
    W, V = rng.normal(size=(27, NB)), rng.normal(size=(27, NB))
    scale = 1.0 / np.array([80, .02, .05, .5, 20, 10, 3, .003, .01, .9, 30, 120, 55, 25, .015, 7, .5, .3, .2, 60, 30, 180, .5, .45, 4, 1030, 365.0])
    W[list(ignored)], V[list(ignored)] = 0.0, 0.0

    def forward(rows):
        z = rows * scale
        y = 3.0 + np.sin(z @ W) + (z @ V) ** 2
        if nan_band is not None:
            y[rows[:, 15] > nan_band[1], nan_band[0]] = np.nan
        return y
    return forward


FREE = [15, 0, 2, 26]                     # LAI, Cab, Cw, DOY
LO, HI = np.array([0.1, 10.0, 0.005, 1.0]), np.array([7.0, 80.0, 0.05, 365.0])


@pytest.fixture(scope="module")
def toy():
    from spart_amd import workloads
    base = workloads.lhs_params(3, "full", seed=2)
    rng = np.random.default_rng(9)
    uA, uB = rng.random((192, 4)), rng.random((192, 4))
    return base, uA, uB, sd.sobol_defined(base, FREE, LO, HI, uA, uB, toy_forward())


def test_a_site_does_not_depend_on_the_others(toy):
    base, uA, uB, ref = toy
    alone = sd.sobol_defined(base[1:2], FREE, LO, HI, uA, uB, toy_forward())
    assert all(same(alone[k][0], ref[k][1]) for k in OUTS)
    assert (ref["var"] > 0).all() and (ref["ST"] > 0).all() and np.isfinite(ref["S1_se"]).all()


def test_permuting_the_parameters_permutes_the_indices(toy):
    base, uA, uB, ref = toy
    p = [2, 0, 3, 1]
    got = sd.sobol_defined(base, [FREE[i] for i in p], LO[p], HI[p], uA[:, p], uB[:, p], toy_forward())
    assert same(got["mean"], ref["mean"]) and same(got["var"], ref["var"])
    assert all(same(got[k], ref[k][:, :, p]) for k in ("S1", "ST", "S1_se", "ST_se"))


def test_equal_designs_give_exact_zeros(toy):
    base, uA, _, _ = toy
    got = sd.sobol_defined(base, FREE, LO, HI, uA, uA, toy_forward())
    assert all((got[k] == 0).all() for k in ("S1", "ST", "S1_se", "ST_se")) and (got["var"] > 0).all()


def test_an_ignored_parameter_gives_exact_zeros_and_leaves_the_others_alone(toy):
    base, uA, uB, _ = toy
    with_doy = sd.sobol_defined(base, FREE, LO, HI, uA, uB, toy_forward(ignored=[26]))
    without = sd.sobol_defined(base, FREE[:3], LO[:3], HI[:3], uA[:, :3], uB[:, :3], toy_forward(ignored=[26]))
    assert (with_doy["S1"][:, :, 3] == 0).all() and (with_doy["ST"][:, :, 3] == 0).all()
    assert (with_doy["S1_se"][:, :, 3] == 0).all() and (with_doy["ST_se"][:, :, 3] == 0).all()
    assert same(with_doy["mean"], without["mean"]) and same(with_doy["var"], without["var"])
    assert all(same(with_doy[k][:, :, :3], without[k]) for k in ("S1", "ST", "S1_se", "ST_se"))


def test_a_nan_row_reaches_its_band_alone(toy):
    base, uA, uB, ref = toy
    got = sd.sobol_defined(base, FREE, LO, HI, uA, uB, toy_forward(nan_band=(2, 6.9)))
    assert all(np.isnan(got[k][:, 2]).all() for k in OUTS)
    keep = [0, 1, 3, 4]
    assert all(same(got[k][:, keep], ref[k][:, keep]) for k in OUTS)


def test_a_constant_output_gives_zero_variance_and_nan_indices():
    yA = np.full((128, 2), 0.25)
    yA[:, 1] = np.random.default_rng(1).random(128)
    res = sd.sobol_of_outputs(yA, yA[::-1].copy(), np.stack([yA, yA[::-1]]))
    assert res["var"][0] == 0.0 and res["mean"][0] == 0.25 and res["var"][1] > 0
    assert all(np.isnan(res[k][0]).all() for k in ("S1", "ST", "S1_se", "ST_se")) and np.isfinite(res["S1"][1]).all()


# ---- sobol_design
def test_sobol_design():
    import torch
    import spart_amd
    uA, uB = spart_amd.sobol_design(256, 3, seed=7)
    assert uA.shape == uB.shape == (256, 3) and uA.dtype == uB.dtype == np.float64
    assert uA.flags["C_CONTIGUOUS"] and uB.flags["C_CONTIGUOUS"]
    assert (uA >= 0).all() and (uA < 1).all() and (uB >= 0).all() and (uB < 1).all()
    again = spart_amd.sobol_design(256, 3, seed=7)
    other = spart_amd.sobol_design(256, 3, seed=8)
    assert same(again[0], uA) and same(again[1], uB) and not same(other[0], uA)
    draw = torch.quasirandom.SobolEngine(6, scramble=True, seed=7).draw(256, dtype=torch.float64).numpy()
    assert same(uA, draw[:, :3]) and same(uB, draw[:, 3:]) and not same(uA, uB)
    assert spart_amd.sobol_design(128, 1)[0].shape == (128, 1)           # (seed 0 is the default)
    for bad in ((0, 3), (128, 0), (128, 17), (12.5, 3)):
        with pytest.raises(ValueError):
            spart_amd.sobol_design(*bad)


# ---- refusals
@pytest.fixture(scope="module")
def capi():
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    from spart_amd import _lib
    L = ctypes.CDLL(build.build(verbose=False))
    for name in ("spart_sobol", "spart_sobol_workspace_bytes"):
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES[name]
    L.spart_last_error.restype = ctypes.c_char_p
    return L


def test_null_context_is_refused_without_a_gpu(capi):
    assert capi.spart_sobol_workspace_bytes(None, 1, 128, 3) == 0
    assert capi.spart_sobol(None, 0, None, 0, None, None, None, 0, None, None, None, None, None, 0, None) == -1 and b"spart_sobol: null context" in capi.spart_last_error(None)


def test_every_refusal_in_its_order(capi):
    """A block of zeros stands for the context: no check before SPART_ERR_NOSENSOR reads anything of a context but its band
    count, which is 0 there, so the list ends with that refusal; nothing is launched and no pointer but the host arrays is
    followed.  (NOSENSOR on a real context and the workspace's size are tests/test_gpu_sobol.py's.)"""
    from spart_amd import _lib
    ctx = ctypes.create_string_buffer(1 << 20)
    host = np.zeros(64)                                              # what the never-followed device pointers point at
    fake = host.ctypes.data
    ok = dict(M=2, F=2, free=[15, 0], lo=[0.1, 10.0], hi=[7.0, 80.0], N=128, opt=(0, 0, 0, 0), outs=OUTS, base=[fake] * 27,
              uA=fake, uB=fake)

    def call(null=(), **kw):
        a = dict(ok, **kw)
        fc, lo, hi = np.array(a["free"], dtype=np.int32), np.array(a["lo"], dtype=np.float64), np.array(a["hi"], dtype=np.float64)
        opt = _lib.SpartSobolOpt(*a["opt"])
        out = _lib.SpartSobolOut(**{k: fake for k in a["outs"]})
        base = (_lib.vp * 27)(*a["base"])
        ptr = lambda name, v: None if name in null else v     # noqa: E731
        rc = capi.spart_sobol(ctypes.addressof(ctx), a["M"], ptr("base", base), a["F"],
                              ptr("free", fc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), ptr("lo", dp(lo)), ptr("hi", dp(hi)), a["N"],
                              ptr("uA", a["uA"]), ptr("uB", a["uB"]), ptr("opt", ctypes.byref(opt)), ptr("out", ctypes.byref(out)),
                              None, 0, None)
        return rc, capi.spart_last_error(None).decode()

    bad_all = dict(F=0, free=[27, 0], lo=[0.1, np.nan], opt=(3, 2, 0, -1), N=100, M=-1, outs=(), uA=None)
    ladder = [("F = 0", dict(F=0)), ("F = 17", dict(F=17)), ("null argument", dict(null=("free",))), ("null argument", dict(null=("lo",))),
              ("null argument", dict(null=("hi",))), ("column = 3", dict(opt=(3, 2, 0, -1))), ("nlayers = -1", dict(opt=(0, 2, 0, -1))),
              ("free_cols[1] = 27", dict(free=[15, 27])), ("free twice", dict(free=[15, 15])), ("bounds of free_cols[0]", dict(lo=[np.nan, 1.0])),
              ("bounds of free_cols[1]", dict(lo=[0.1, 80.0])), ("band_model = 2", dict(opt=(0, 2, 0, 0))), ("N = 100", dict(N=100)),
              ("N = 64", dict(N=64)), ("N = 2097152", dict(N=1 << 21)), ("M = -1", dict(M=-1)), ("M = 2000000001", dict(M=2000000001)),
              ("opt is null", dict(null=("opt",))), ("out is null", dict(null=("out",))), ("base is null", dict(null=("base",))),
              ("base[3] is null", dict(base=[fake] * 3 + [None] + [fake] * 22 + [None])), ("uA is null", dict(uA=None)),
              ("uB is null", dict(uB=None)), ("every output is null", dict(outs=()))]
    for text, kw in ladder:
        rc, msg = call(**kw)
        assert rc == -1 and text in msg and msg.startswith("spart_sobol: "), (text, rc, msg)
    # the order: with everything wrong at once, mending the refusals one by one meets them in the header's order
    wrong = dict(bad_all)
    seen = []
    for key, _ in (("F", 0), ("opt", 0), ("opt", 1), ("free", 0), ("lo", 0), ("opt", 2), ("N", 0), ("M", 0), ("uA", 0), ("outs", 0)):
        rc, msg = call(**wrong)
        assert rc == -1
        seen.append(msg)
        if key == "opt":
            wrong["opt"] = {(3, 2, 0, -1): (0, 2, 0, -1), (0, 2, 0, -1): (0, 2, 0, 0), (0, 2, 0, 0): (0, 0, 0, 0)}[wrong["opt"]]
        else:
            wrong[key] = ok[key]
    for msg, text in zip(seen, ("F = 0", "column = 3", "nlayers = -1", "free_cols[0] = 27", "bounds of free_cols[1]", "band_model = 2",
                                "N = 100", "M = -1", "uA is null", "every output is null")):
        assert text in msg, (text, seen)
    # NULL data with M = 0 is no refusal of its own; the list ends at the sensor
    rc, msg = call()
    assert rc == -4 and "no sensor" in msg
    rc, msg = call(M=0, null=("opt", "out", "base"), uA=None, uB=None)
    assert rc == -4 and "no sensor" in msg
    assert capi.spart_sobol_workspace_bytes(ctypes.addressof(ctx), 2, 128, 2) == 0


def test_sobol_arguments_are_checked_before_the_gpu_is_asked_for():
    import spart_amd
    from spart_amd import engine, workloads
    P = workloads.lhs_params(3, "full", seed=1).T
    ok = dict(free=["LAI", "Cab"], N=128)
    u = np.zeros((128, 2))
    for kw, text in ((dict(ok, free=["nope"]), "unknown"), (dict(ok, free=["LAI", "LAI"]), "twice"), (dict(ok, free=[]), "0 names"),
                     (dict(ok, bounds={"LAI": (3.0, 3.0)}), "lo < hi"), (dict(ok, bounds={"Cw": (0.0, 1.0)}), "not free"),
                     (dict(ok, column="rso"), "column"), (dict(ok, band_model="wide"), "band_model"), (dict(ok, lidf="x"), "lidf"),
                     (dict(ok, N=100), "multiple of 64"), (dict(ok, N=64), "multiple of 64"), (dict(ok, N=1 << 21), "multiple of 64"),
                     (dict(ok, N=128.5), "multiple of 64"), (dict(ok, design=u), "design"), (dict(ok, design=(u, u[:, :1])), "uB has shape"),
                     (dict(ok, design=(u[:100], u[:100])), "multiple of 64"), (dict(ok, design=(u, np.zeros((192, 2)))), "differ"),
                     (dict(ok, nlayers=0), "nlayers")):
        with pytest.raises((ValueError, TypeError), match=text):
            spart_amd.sobol(P, "Sentinel2A-MSI", **kw)
    with pytest.raises(ValueError, match="27"):
        spart_amd.sobol(np.zeros((26, 2)), "Sentinel2A-MSI", ["LAI"])
    with pytest.raises(ValueError, match="broadcast"):
        spart_amd.sobol([np.zeros(2)] + [np.zeros(3)] * 26, "Sentinel2A-MSI", ["LAI"])
    e = engine.Engine.__new__(engine.Engine)                   # an Engine object that never saw a device
    e.nb = 13
    with pytest.raises(ValueError, match="unknown"):
        e.sobol(P, ["nope"])
    with pytest.raises(ValueError, match="multiple of 64"):
        e.sobol(P, ["LAI"], N=130)
    plan, params, M, N, uA, uB = engine.sobol_args(P, ["LAI", "DOY"], 192, {"DOY": (1, 365)}, None, 4, "R_TOA", "srf", "newton")
    assert (M, N, plan["column"], plan["names"], plan["cols"].tolist()) == (3, 192, 1, ["LAI", "DOY"], [15, 26])
    assert plan["lo"].tolist() == [0.1, 1.0] and plan["hi"].tolist() == [7.0, 365.0] and len(params) == 27
    want = spart_amd.sobol_design(192, 2, seed=4)
    assert same(uA, want[0]) and same(uB, want[1])
    assert engine.sobol_args([1.0] * 27, ["LAI"], 128, None, (u[:, :1], u[:, 1:]), 0, "R_TOC", "centre", "literal")[2:4] == (1, 128)
    with pytest.raises(ValueError, match="no range"):
        engine.sobol_args(P, ["DOY"], 128, None, None, 0, "R_TOC", "centre", "literal")


def test_signatures_structs_and_header_agree():
    from spart_amd import _lib
    assert [f[0] for f in _lib.SpartSobolOpt._fields_] == ["column", "band_model", "fast_prelude", "nlayers"]
    assert all(f[1] is ctypes.c_int32 for f in _lib.SpartSobolOpt._fields_) and ctypes.sizeof(_lib.SpartSobolOpt) == 16
    assert [f[0] for f in _lib.SpartSobolOut._fields_] == list(OUTS) == list(_lib.SOBOL_OUTS) and ctypes.sizeof(_lib.SpartSobolOut) == 48
    res, args = _lib.SIGNATURES["spart_sobol"]
    ref = list(_lib.SIGNATURES["spart_refine"][1])
    assert res is ctypes.c_int and len(args) == 15 and args[:7] == ref[:7] and args[7] is ctypes.c_int64 and args[12:] == ref[16:]
    assert args[10]._type_ is _lib.SpartSobolOpt and args[11]._type_ is _lib.SpartSobolOut
    res, args = _lib.SIGNATURES["spart_sobol_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [_lib.vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    full = open(os.path.join(ROOT, "include", "spart_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    body = re.search(r"typedef struct spart_sobol_opt \{(.*?)\} spart_sobol_opt;", header, flags=re.S).group(1)
    assert re.findall(r"\b([A-Za-z_0-9]+)\s*[;,]", body) == ["column", "band_model", "fast_prelude", "nlayers"]
    body = re.search(r"typedef struct spart_sobol_out \{(.*?)\} spart_sobol_out;", header, flags=re.S).group(1)
    assert re.findall(r"\*([A-Za-z_0-9]+)\s*[;,]", body) == list(OUTS)
    assert re.search(r"int spart_sobol\(spart_ctx \*ctx, int64_t M, const double \*const base\[SPART_NPARAM\], int F,\s*const int32_t "
                     r"\*free_cols\s*, const double \*lo, const double \*hi\s*,\s*int64_t N, const double \*uA, const double \*uB\s*,\s*"
                     r"const spart_sobol_opt \*opt, const spart_sobol_out \*out,\s*void \*workspace, size_t workspace_bytes, void \*stream\);",
                     header)
    assert "size_t spart_sobol_workspace_bytes(const spart_ctx *ctx, int64_t M, int64_t N, int F);" in header
    assert "#define SPART_ABI_VERSION 14" in full and "spart_sobol and spart_sobol_workspace_bytes" in full and _lib.ABI_VERSION == 14
    assert (_lib.SOBOL_BLOCK, _lib.SOBOL_MIN_N, _lib.SOBOL_MAX_N) == (sd.BLOCK, sd.MIN_N, sd.MAX_N) == (64, 128, 1 << 20)
    src = open(os.path.join(ROOT, "spart-python_amd", "csrc", "spart_sobol.h")).read()
    assert "constexpr int SOBOL_BLOCK = 64;" in src and "constexpr int64_t SOBOL_MIN_N = 128, SOBOL_MAX_N = 1 << 20;" in src
    sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
    import build
    assert any(d.endswith("spart_sobol.h") for d in build.DEPS)


def test_sobol_kernels_use_no_scratch_and_no_lds(kernel_meta):
    """DESIGN.md section 18 states: no spills, no scratch, 0 bytes of LDS (the tree crosses lanes without it)"""
    names = ("k_sobol_rows", "k_sobol_blocks", "k_sobol_finish")
    hits = {k: v for k, v in kernel_meta.items() if "k_sobol_" in k}
    assert len(hits) == 3 and all(any(n in k for k in hits) for n in names), sorted(hits)
    for name, k in hits.items():
        print(f"{name}: {k['vgpr_count']} VGPRs, {k['sgpr_count']} SGPRs, {k['group_segment_fixed_size']} bytes of LDS")
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (name, k)
        assert k["group_segment_fixed_size"] <= 0, (name, k)
    assert "0 bytes of LDS" in open(os.path.join(ROOT, "DESIGN.md")).read()
