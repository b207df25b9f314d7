"""spart_refine at its own edges, each case bit for bit against the definition tools/refine_defined.py (all six outputs of the
raw C call, np.array_equal with equal_nan; the definition's forward model is the engine's float64 pruned column path, configured
like the call; no tolerance anywhere):
  (a) later chunks of the host loop: chunk sizes other than 30 840, exactly one and exactly two chunks, a last chunk of one
      observation, per-observation weights and NULL optional outputs behind the first chunk, the workspace of one chunk;
  (b) band counts around the LDS tile of 16 bands, one band, and the widest sensor (2162 bands);
  (c) every F = 1 ... 16, both sides of the group-width switch at F = 14 -> 15;
  (d) the two options that reach the forward model (fast_prelude, nlayers), raw and through Python;
  (e) groups built so that the wave-uniform branches of the step kernel run: nobody moves, one moves among rejected mates;
  (f) the lambda clamps, n_iter = 100 and the prefix property."""
import numpy as np
import pytest

from helpers.lut_calls import hyper_si, torch_mod  # noqa: F401 (fixtures)
from helpers.refine_calls import COLUMNS, F16, FILL, FREE, OUTS, S2, bounds_of, cols_of, forward_of, make_case, rd, refine_call, same

pytestmark = pytest.mark.gpu

KINDS = ("none", "shared", "per_observation")
# Observations per wave (refine_group).  A column of LDS holds (F + 1) 16 + 2 * 16 + (F (F + 1) / 2 + F) + F (F + 1) / 2 + 3 F + 1
# doubles and a group of W observations has W + 1 columns of 8 bytes: F = 14 needs 539 * 9 * 8 = 38 808 B, within the budget of
# 40 960 B, so W = 8; F = 15 needs 589 * 9 * 8 = 42 408 B, so W = 4.  A table, not a call into the library.
GROUP = {1: 8, 2: 8, 3: 8, 4: 8, 5: 8, 6: 8, 7: 8, 8: 8, 9: 8, 10: 8, 11: 8, 12: 8, 13: 8, 14: 8, 15: 4, 16: 4}


@pytest.fixture(scope="module")
def engines(torch_mod, hyper_si):
    from spart_amd import get_engine
    return {"s2": get_engine(S2, 0), "hyper": get_engine(None, 0, sensor_info=hyper_si)}


def names_of(F):
    return FREE.get(F, F16[:F])


def mismatches(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return "shape" if a.shape != b.shape else int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def assert_same(got, ref, what, keys=OUTS):
    for k in keys:
        assert same(got[k], ref[k]), (what, k, mismatches(got[k], ref[k]))


def defined(torch, eng, case, column, n_iter, lidf="literal", nlayers=None, **kw):
    base, free, lo, hi, obs, w = case
    return rd.refine_defined(base, free, lo, hi, obs, forward_of(torch, eng, COLUMNS[column], lidf, nlayers), weights=w, n_iter=n_iter, **kw)


def call(torch, eng, case, column, n_iter, lidf="literal", nlayers=None, **kw):
    """the raw call configured like defined(...)"""
    base, free, lo, hi, obs, w = case
    rc, got = refine_call(torch, eng, base, free, lo, hi, obs, w, column=column, n_iter=n_iter, fast_prelude=1 if lidf == "newton" else 0,
                          nlayers=0 if nlayers is None else nlayers, **kw)
    assert rc == 0, eng.lib.spart_last_error(eng.ctx)
    return got


def check(torch, eng, case, column, n_iter, what, lidf="literal", nlayers=None, guard=False, **kw):
    """device == definition, all six outputs -> (definition's, device's)"""
    ref = defined(torch, eng, case, column, n_iter, lidf, nlayers, **kw)
    got = call(torch, eng, case, column, n_iter, lidf, nlayers, guard=guard, **kw)
    assert_same(got, ref, what)
    return ref, got


def rows_of(case, sl):
    base, free, lo, hi, obs, w = case
    return base[sl], free, lo, hi, obs[sl], (w[sl] if w is not None and np.ndim(w) == 2 else w)


# ---- (a) chunks

def plant_specials(case, chunk, at_cut):
    """Copies of make_case's special rows on both sides of the cut between the first two chunks: the dead rows 3 (a NaN
    observation) at chunk - 1 and ``at_cut`` at chunk itself, the others around them.  -> {position: special row}"""
    base, _, _, _, obs, w = case
    M = base.shape[0]
    where = {chunk - 4: 0, chunk - 3: 1, chunk - 2: 2, chunk - 1: 3, chunk: at_cut, chunk + 1: 4, chunk + 2: 6 if at_cut != 6 else 5}
    where = {p: s for p, s in where.items() if p < M}
    for p, s in where.items():
        base[p], obs[p] = base[s], obs[s]
        if w is not None and np.ndim(w) == 2:
            w[p] = w[s]
    return where


def check_specials(ref, where, kind, what):
    dead = (3, 4, 5) if kind == "per_observation" else (3, 4)
    for p, s in where.items():
        if s in dead:
            assert ref["n_accept"][p] == -1 and np.isnan(ref["std"][p]).all(), (what, p, s)
        elif s in (0, 1) or kind == "per_observation":
            assert ref["n_accept"][p] >= 0, (what, p, s)
        if s == 2 and kind == "per_observation":
            assert ref["cost0"][p] == 0 and ref["n_accept"][p] == 0, (what, p, s)


# One forward call takes 1 << 19 rows, so observations go in chunks of (1 << 19) // (F + 1).
# sensor, F, chunk, M, weights, n_iter, column, the special row put at position `chunk`
#   5 (a negative weight, dead): with M = chunk + 1 the last chunk is that observation alone, and it is dead by ITS weights only;
#   6 (a NaN observation under a zero weight, alive): the lone observation of the last chunk takes every step of the kernel
CHUNK_CASES = [("s2", 1, 262144, 262145, "per_observation", 1, 1, 5),
               ("s2", 7, 65536, 131072, "shared", 1, 0, 5),
               ("s2", 7, 65536, 65536, "none", 2, 2, 5),
               ("s2", 7, 65536, 65537, "per_observation", 1, 1, 6),
               ("s2", 15, 32768, 32769, "per_observation", 2, 2, 5),
               ("hyper", 6, 74898, 74899, "per_observation", 1, 0, 6)]


@pytest.mark.parametrize("sensor,F,chunk,M,kind,n_iter,column,at_cut", CHUNK_CASES, ids=[f"{c[0]}-F{c[1]}-M{c[3]}" for c in CHUNK_CASES])
def test_chunks(torch_mod, engines, sensor, F, chunk, M, kind, n_iter, column, at_cut):
    eng = engines[sensor]
    assert chunk == (1 << 19) // (F + 1) and n_iter <= 2
    what = (sensor, F, M, kind)
    case = make_case(torch_mod, eng, names_of(F), M, COLUMNS[column], kind, 1000 + F)
    where = plant_specials(case, chunk, at_cut)
    assert {chunk - 1, chunk if M > chunk else chunk - 1} <= set(where)
    ref, got = check(torch_mod, eng, case, column, n_iter, what, guard=(M == chunk + 1))
    check_specials(ref, where, kind, what)
    assert ref["n_accept"][chunk - 1] == -1                         # a dead observation ends the first chunk ...
    if M > chunk and kind == "per_observation":                     # ... and the next begins with a dead or a live one, as planted
        assert (ref["n_accept"][chunk] == -1) == (at_cut == 5), what
    alive = ref["n_accept"] >= 0
    assert alive.mean() > 0.5 and (ref["cost"][alive] <= ref["cost0"][alive]).all() and (ref["n_accept"][:chunk] >= 1).any()
    if M - chunk > 1:
        assert (ref["n_accept"][chunk:] >= 1).any() and (ref["n_accept"][chunk:] == -1).any(), what
    if M > chunk:
        part = call(torch_mod, eng, rows_of(case, slice(chunk, M)), column, n_iter)          # the later chunks on their own
        assert_same(part, {k: got[k][chunk:] for k in OUTS}, what + ("[chunk:] alone",))
    if F == 15:
        # NULL optional outputs behind the first chunk: the others as before, the NULL ones untouched
        null = ("cost0", "std", "n_accept", "y")
        few = call(torch_mod, eng, case, column, n_iter, null=null)
        for k in OUTS:
            assert (few[k] == FILL).all() if k in null else same(few[k], got[k]), (what, "NULL outputs", k)


@pytest.mark.parametrize("sensor,F,chunk", [("s2", 1, 262144), ("s2", 7, 65536), ("s2", 15, 32768), ("hyper", 6, 74898)])
def test_workspace_is_sized_by_one_chunk(torch_mod, engines, sensor, F, chunk):
    eng = engines[sensor]
    assert chunk == (1 << 19) // (F + 1)
    ws = lambda M: int(eng.lib.spart_refine_workspace_bytes(eng.ctx, M, F))      # noqa: E731
    assert ws(chunk) == ws(2 * chunk) == ws(2_000_000_000) > 0
    # M = chunk + 1 runs a call of `chunk` observations and one of a single observation in the same workspace: it needs what
    # the first needs, and the forward workspace of F + 1 rows, which ws(1) contains.  (test_chunks runs these sizes with a
    # guard region behind the workspace.)
    assert ws(chunk + 1) >= max(ws(chunk), ws(1)) and ws(chunk) > ws(1) > 0


# ---- (b) band counts

def cut_bands(si, nb):
    """the first nb bands of a reference-style sensorinfo dict"""
    out = dict(si)
    out["wl_smac"] = np.asarray(si["wl_smac"], dtype=np.float64).reshape(-1, 1)[:nb]
    out["band_id_smac"] = list(si["band_id_smac"])[:nb]
    out["SMAC_coef"] = {n: np.asarray(v, dtype=np.float64).reshape(1, -1)[:, :nb].copy() for n, v in si["SMAC_coef"].items()}
    out["wl_srf_smac"] = np.ascontiguousarray(np.asarray(si["wl_srf_smac"], dtype=np.float64)[:, :nb])
    out["p_srf_smac"] = np.ascontiguousarray(np.asarray(si["p_srf_smac"], dtype=np.float64)[:, :nb])
    return out


# nb, F, weights, column: the three weight forms and the three columns in rotation, nb = 1 with per-observation weights
BAND_CASES = [(nb, 2 if nb == 2162 else 6, KINDS[(i + 2) % 3], (i // 3 + i) % 3) for i, nb in enumerate((1, 15, 16, 17, 32, 33, 2162))]


@pytest.mark.parametrize("nb,F,kind,column", BAND_CASES, ids=[f"nb{c[0]}" for c in BAND_CASES])
def test_band_counts(torch_mod, hyper_si, nb, F, kind, column):
    """REFINE_JT = 16 bands per LDS tile: one band, a tile less one, exact tiles, one band past a tile, and 135 tiles plus 2"""
    from spart_amd import get_engine
    assert {c[2] for c in BAND_CASES} == set(KINDS) and {c[3] for c in BAND_CASES} == {0, 1, 2} and BAND_CASES[0][2] == "per_observation"
    if nb == 2162:
        from test_gpu_hyperspectral import model_grid, synthetic_sensor
        si = synthetic_sensor(model_grid())
    else:
        si = cut_bands(hyper_si, nb)
    eng = get_engine(None, 0, sensor_info=si)
    assert eng.nb == nb
    case = make_case(torch_mod, eng, names_of(F), 65, COLUMNS[column], kind, 2000 + nb)
    ref, _ = check(torch_mod, eng, case, column, 2, (nb, kind, column))
    base, free, lo, hi, obs, w = case
    assert ref["y"].shape == (65, nb)
    if nb == 1:
        # a zero weight on the only band: cost 0 at the start, so no trial is ever better
        zero = w[:, 0] == 0.0
        assert zero[2] and zero.sum() >= 2 and (ref["n_accept"][zero] == 0).all() and (ref["cost"][zero] == 0).all()
        assert (ref["cost0"][zero] == 0).all() and same(ref["x"][zero], rd.clip_defined(base[zero][:, free], lo, hi))
        assert (ref["n_accept"][~zero] >= 1).any() and ref["n_accept"][3] == -1 and ref["n_accept"][5] == -1
    else:
        dead = [3, 4] + ([5] if kind == "per_observation" else [])
        assert (ref["n_accept"][dead] == -1).all() and (ref["n_accept"] >= 1).mean() > 0.5


# ---- (c) every F

F_CASES = [(F, 2 * GROUP[F] + 1) for F in range(1, 17)] + [(14, 63), (14, 65), (15, 63), (15, 65)]


@pytest.mark.parametrize("F,M", F_CASES, ids=[f"F{F}-M{M}" for F, M in F_CASES])
def test_every_F(torch_mod, engines, F, M):
    """two full groups and a group of one; at M = 63 and 65, F = 14 (W = 8) and F = 15 (W = 4) lay the same rows out differently"""
    eng = engines["s2"]
    assert GROUP[F] == (8 if F <= 14 else 4) and (M in (63, 65) or M == 2 * GROUP[F] + 1)
    column = F % 3
    case = make_case(torch_mod, eng, F16[:F], M, COLUMNS[column], "per_observation", 3000 + 100 * F + M)
    ref, _ = check(torch_mod, eng, case, column, 2, (F, M))
    assert ref["x"].shape == (M, F) and (ref["n_accept"] >= 1).mean() > 0.5
    if M >= 63:
        assert (ref["n_accept"][[3, 4, 5]] == -1).all() and ref["n_accept"][2] == 0


# ---- (d) options

@pytest.fixture(scope="module")
def option_case(torch_mod, engines):
    eng = engines["s2"]
    case = make_case(torch_mod, eng, FREE[6], 65, "R_TOA", "per_observation", 4000)
    ref, plain = check(torch_mod, eng, case, 1, 2, "defaults")
    return case, plain


@pytest.mark.parametrize("lidf,nlayers", [("newton", None), ("literal", 1), ("literal", 30), ("newton", 30)])
def test_options_reach_the_forward_model(torch_mod, engines, option_case, lidf, nlayers):
    eng = engines["s2"]
    case, plain = option_case
    ref, got = check(torch_mod, eng, case, 1, 2, (lidf, nlayers), lidf=lidf, nlayers=nlayers)
    assert not same(got["x"], plain["x"]) and (ref["n_accept"] >= 1).mean() > 0.5, (lidf, nlayers)
    if lidf == "newton" and nlayers == 30:
        only_layers = call(torch_mod, eng, case, 1, 2, nlayers=30)
        only_prelude = call(torch_mod, eng, case, 1, 2, lidf="newton")
        assert not same(got["x"], only_layers["x"]) and not same(got["x"], only_prelude["x"])


def test_options_through_python(torch_mod, engines, option_case):
    import spart_amd
    eng = engines["s2"]
    case, plain = option_case
    base, free, lo, hi, obs, w = case
    raw = call(torch_mod, eng, case, 1, 2, lidf="newton", nlayers=30)
    assert not same(raw["x"], plain["x"])
    P = torch_mod.as_tensor(np.ascontiguousarray(base.T), device=eng.device)
    res = eng.refine(P, obs, FREE[6], weights=w, column="R_TOA", n_iter=2, lidf="newton", nlayers=30)
    assert res["names"] == FREE[6]
    assert_same({k: res[k].cpu().numpy() for k in OUTS}, raw, "Engine.refine")
    host = spart_amd.refine(base.T, obs, S2, FREE[6], weights=w, column="R_TOA", n_iter=2, lidf="newton", nlayers=30)
    assert host["names"] == FREE[6]
    assert_same({k: np.asarray(host[k]) for k in OUTS}, raw, "spart_amd.refine")


# ---- (e) constructed groups

def group_case(torch, eng, names, pattern, column, seed):
    """one observation per letter: 's' still (obs = the model at the clipped start: cost0 is exactly 0 and no trial can be
    better), 'm' moving (a noisy twin row), 'd' dead (a NaN observation)"""
    M = len(pattern)
    assert M < 63                                                   # (no special rows from make_case)
    case = make_case(torch, eng, names, M, COLUMNS[column], "none", seed)
    obs = case[4]
    start = defined(torch, eng, case, column, 0)["y"]               # the model at the clipped start, the call's own batch layout
    for i, ch in enumerate(pattern):
        if ch == "s":
            assert np.isfinite(start[i]).all()
            obs[i] = start[i]
        elif ch == "d":
            obs[i] = np.nan
    return case


def check_groups(ref, pattern, what):
    p = np.array(list(pattern))
    s, m, d = p == "s", p == "m", p == "d"
    assert (ref["n_accept"][s] == 0).all() and (ref["cost"][s] == 0).all() and (ref["cost0"][s] == 0).all(), what
    assert (ref["n_accept"][m] >= 1).all(), (what, ref["n_accept"])
    assert (ref["n_accept"][d] == -1).all(), what


GROUP_CASES = [(6, "ssssssss"), (6, "msssssss"), (6, "sssssssm"), (6, "ssssssss" + "mmmmmmmm"), (6, "dddmdddd"), (6, "ssssssss" + "m"),
               (15, "msss"), (15, "sssm")]


@pytest.mark.parametrize("F,pattern", GROUP_CASES, ids=[f"F{F}-{p}" for F, p in GROUP_CASES])
def test_constructed_groups(torch_mod, engines, F, pattern):
    """nobody in a group moves: the sums are not rebuilt but reloaded from the state; one moves: the sums are cleared for the
    whole group and the rejected mates get theirs back from the state"""
    eng = engines["s2"]
    W = GROUP[F]
    assert len(pattern) <= W or len(pattern) in (2 * W, W + 1)
    case = group_case(torch_mod, eng, names_of(F), pattern, 0, 5000 + 10 * F + len(pattern))
    ref, _ = check(torch_mod, eng, case, 0, 3, (F, pattern))
    check_groups(ref, pattern, (F, pattern))
    still = np.array(list(pattern)) == "s"
    if F <= 13:                                                     # (more free parameters than bands: a singular A, std is NaN)
        assert np.isfinite(ref["std"][still]).all()                 # what a still observation's restored sums must give


# ---- (f) long runs and the lambda clamps

def walled_case(torch, eng, M, seed):
    """F = 2 (uo3, LAI), column R_TOA, M rows: even rows still, odd rows `walled`.  A walled row starts at uo3 = 0.01 with the lower
    bound at -1: the model is NaN for uo3 < 0 in the bands with ozone absorption (SMAC raises uo3 m to a power), and the observation is the model at the start
    moved by -K h J_0 (J_0 = the forward difference in uo3), a target K h = 0.01 * 10^11.5 below the start.  The proposal in uo3
    is about -K h / (1 + lambda): at every lambda <= 1e11 it lands below 0 and is rejected, at 1e12 it is 0.00316 and is taken.
    So the default lambda0 = 1e-2 is rejected 14 times (1e-2 ... 1e11) and accepted at the clamp, and lambda0 = 1e11 once."""
    from spart_amd import workloads
    names = ["uo3", "LAI"]
    free = cols_of(names)
    lo, hi = bounds_of(names)
    lo[0] = -1.0
    base = workloads.lhs_params(M, "full", seed=seed)
    base[:, free[0]] = 0.01
    fwd = forward_of(torch, eng, "R_TOA")
    h = 1e-3 * (hi[0] - lo[0])
    moved = base.copy()
    moved[:, free[0]] += h
    Y = fwd(np.concatenate([base, moved]))
    y0, y1 = Y[:M], Y[M:]
    assert np.isfinite(Y).all()
    below = base[:1].copy()
    below[:, free[0]] = -1e-6
    assert np.isnan(fwd(below)).any()                               # the wall (in the bands that ozone absorbs in)
    obs = y0.copy()
    case = (base, free, lo, hi, obs, None)
    obs[:] = defined(torch, eng, case, 1, 0)["y"]                   # the model at the start, the call's own batch layout
    walled = np.arange(M) % 2 == 1
    obs[walled] = y0[walled] - (0.01 * 10 ** 11.5 / h) * (y1[walled] - y0[walled])
    return case, walled


@pytest.mark.parametrize("lambda0,n_iter", [(None, 16), (1e11, 3)])
def test_upper_lambda_clamp(torch_mod, engines, monkeypatch, lambda0, n_iter):
    """min(lambda * 10, 1e12).  Still observations reject every step, as many as it takes to reach the clamp, but their proposal
    is x itself at any lambda (g = 0), so the walled rows are what shows lambda: with a clamp at 1e11 they never move."""
    eng = engines["s2"]
    case, walled = walled_case(torch_mod, eng, 65, 6000)
    kw = {} if lambda0 is None else {"lambda0": lambda0}
    ref, got = check(torch_mod, eng, case, 1, n_iter, ("upper clamp", lambda0), **kw)
    assert (ref["n_accept"][~walled] == 0).all() and (ref["cost"][~walled] == 0).all()
    print("walled rows: n_accept", np.unique(ref["n_accept"][walled]), " uo3", ref["x"][walled, 0].min(), "...", ref["x"][walled, 0].max())
    assert (ref["n_accept"][walled] == 1).all() and (ref["x"][walled, 0] < 0.01).all() and (ref["x"][walled, 0] > 0.005).all()
    monkeypatch.setattr(rd, "LAMBDA_MAX", 1e11)                     # the definition with another clamp: the case can tell
    other = defined(torch_mod, eng, case, 1, n_iter, **kw)
    assert (other["n_accept"][walled] == 0).all() and (other["x"][walled, 0] == 0.01).all()


@pytest.fixture(scope="module")
def moving_case(torch_mod, engines):
    return make_case(torch_mod, engines["s2"], FREE[2], 65, "R_TOC", "none", 6100)


def test_lower_lambda_clamp(torch_mod, engines, moving_case, monkeypatch):
    """max(lambda / 10, 1e-12) from lambda0 = 1e-11: 1e-12 after the first accepted step and still 1e-12 after the second"""
    eng = engines["s2"]
    ref, _ = check(torch_mod, eng, moving_case, 0, 3, "lower clamp", lambda0=1e-11)
    print("lower clamp: n_accept", np.bincount(ref["n_accept"] + 1))
    assert (ref["n_accept"] == 3).sum() >= 8
    monkeypatch.setattr(rd, "LAMBDA_MIN", 1e-13)
    other = defined(torch_mod, eng, moving_case, 0, 3, lambda0=1e-11)
    assert not same(other["x"], ref["x"])


def test_hundred_iterations(torch_mod, engines, moving_case):
    eng = engines["s2"]
    ref, _ = check(torch_mod, eng, moving_case, 0, 100, "n_iter = 100")
    alive = ref["n_accept"] >= 0
    print("n_iter = 100: n_accept", ref["n_accept"][alive].min(), "...", ref["n_accept"][alive].max())
    assert (ref["n_accept"][alive] >= 3).mean() > 0.9 and (ref["n_accept"] <= 100).all()


def test_prefix_property(torch_mod, engines, moving_case):
    """the state after n_iter = k is the state after n_iter = 5 cut off after decision k.  `history` records x and cost; n_accept
    and y of each k come from a definition run of their own."""
    eng = engines["s2"]
    history = []
    full = defined(torch_mod, eng, moving_case, 0, 5, history=history)
    assert len(history) == 6 and same(history[5][0], full["x"]) and same(history[5][1], full["cost"])
    moved = 0
    for k in range(6):
        ref, got = check(torch_mod, eng, moving_case, 0, k, ("prefix", k))
        assert same(got["x"], history[k][0]) and same(got["cost"], history[k][1]), k
        moved += k > 0 and not same(history[k][0], history[k - 1][0])
    assert moved >= 3                                               # (the prefixes do differ from each other)
