"""Parameter summaries without a GPU: the definition of spart_lut_summarise (tools/lut_brute_force.summarise_defined) against
spart_amd.summarise_rows, the NULL-context refusal of the entry point, retrieve_stream's chunk arithmetic with an injected
search / summary pair, and the argument checks of retrieve(summary=..., params_cols=...)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))

import lut_brute_force as bf  # noqa: E402

U = 2.0 ** -53


def same(a, b):
    """equal element for element, NaN matching NaN"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def assert_within_bounds(params, idx, got_mean, got_std, ref_mean, ref_std, what=""):
    """mean within (k + 1) u max|x| and std within (2 k + 8) u max|x - mean| of another summation order, u = 2^-53: the
    forward error of a length-k sequential sum against any other order of the same terms.  Per observation and parameter,
    x = the values that observation selects; where they include inf or NaN (or there are none) both sides must be
    non-finite."""
    params, idx = np.asarray(params, dtype=np.float64), np.asarray(idx)
    B = params.shape[0]
    M, k = idx.shape
    assert got_mean.shape == got_std.shape == ref_mean.shape == ref_std.shape == (M, params.shape[1]), what
    for m0 in range(0, M, 4096):                                                 # (blocks: the gathered values are (m, k, P))
        sl = slice(m0, m0 + 4096)
        ok = (idx[sl] >= 0) & (idx[sl] < B)
        x = np.where(ok[:, :, None], params[np.where(ok, idx[sl], 0)], np.nan)   # NaN where skipped
        finite = (np.isfinite(x) | ~ok[:, :, None]).all(axis=1) & ok.any(axis=1)[:, None]
        for got, ref in ((got_mean[sl], ref_mean[sl]), (got_std[sl], ref_std[sl])):
            assert not np.isfinite(got[~finite]).any() and not np.isfinite(ref[~finite]).any(), what
        with np.errstate(all="ignore"):
            amax = np.nanmax(np.where(finite[:, None, :], np.abs(x), 0.0), axis=1, initial=0.0)
            dmax = np.nanmax(np.where(finite[:, None, :], np.abs(x - got_mean[sl][:, None, :]), 0.0), axis=1, initial=0.0)
            em = np.abs(got_mean[sl] - ref_mean[sl])[finite]
            es = np.abs(got_std[sl] - ref_std[sl])[finite]
        assert (em <= (k + 1) * U * amax[finite]).all(), (what, float(em.max()))
        assert (es <= (2 * k + 8) * U * dmax[finite]).all(), (what, float(es.max()))


def summary_case(B, P, k, seed):
    """a random table with +-inf in two rows and NaN in two; k + 1 observations with a padding suffix of every length
    0 ... k (the last all padding), duplicated rows, and three observations WITHOUT padding that select the NaN rows"""
    rng = np.random.default_rng(seed)
    params = rng.normal(0.0, 1.0, (B, P)) * rng.uniform(0.01, 100.0, P)
    params[B - 1, 0], params[B - 2, P - 1] = np.nan, np.nan
    params[3, 0], params[4, P // 2] = np.inf, -np.inf
    idx = rng.integers(5, B - 2, (k + 4, k))
    idx[:, k // 2] = idx[:, 0]                                    # a duplicated row in every observation
    for L in range(k + 1):
        idx[L, k - L:] = -1
    idx[1, 0] = 3 if k > 1 else idx[1, 0]                         # (inf under padding: numpy's nan* forms keep inf)
    idx[k + 1, 0], idx[k + 2, k - 1], idx[k + 3, :] = B - 1, B - 2, B - 1
    idx[k + 2, 0] = 4
    return params, idx.astype(np.int64)


@pytest.mark.parametrize("k", [1, 2, 3, 10, 64, 256])
@pytest.mark.parametrize("P", [27, 5])
def test_definition_against_summarise_rows(k, P):
    from spart_amd.lut import summarise_rows
    params, idx = summary_case(400, P, k, 100 * k + P)
    mean, median, std, count = bf.summarise_defined(params, idx)
    hm, hmed, hs = summarise_rows(params, idx)
    assert count.dtype == np.int32 and np.array_equal(count, (idx >= 0).sum(axis=1))
    assert count[k] == 0 and np.isnan(mean[k]).all() and np.isnan(median[k]).all() and np.isnan(std[k]).all()
    assert same(median, hmed)
    assert_within_bounds(params, idx, mean, std, hm, hs, (k, P))
    assert np.isnan(median[k + 3]).sum() == 1 and np.isnan(mean[k + 1, 0]) and np.isfinite(mean[k + 1, 1:]).all()


def test_definition_skips_what_is_out_of_range_and_keeps_place_order():
    params = np.array([[1.0, 1e17], [2.0, 1.0], [4.0, -1e17], [8.0, 3.0]])
    idx = np.array([[3, 7, 0, -2, 2, 4, 1, 1 << 40], [-1, 5, 4, -1, 9, -3, 4, 4], [2, 2, 2, -1, -1, -1, -1, -1]], dtype=np.int64)
    mean, median, std, count = bf.summarise_defined(params, idx)
    assert count.tolist() == [4, 0, 3]
    assert mean[0, 0] == 15.0 / 4 and median[0, 0] == 3.0
    assert mean[0, 1] == (((3.0 + 1e17) + -1e17) + 1.0) / 4 == 0.25            # place order: 3 + 1e17 rounds to 1e17
    assert median[0, 1] == 2.0
    assert np.isnan(mean[1]).all() and np.isnan(median[1]).all() and np.isnan(std[1]).all()
    assert mean[2].tolist() == [4.0, -1e17] and std[2].tolist() == [0.0, 0.0] and median[2].tolist() == [4.0, -1e17]


def test_null_context_is_refused_without_a_device():
    import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.spart_last_error.restype = ctypes.c_char_p
    f = lib.spart_lut_summarise
    f.restype = ctypes.c_int
    vp = ctypes.c_void_p
    f.argtypes = [vp, ctypes.c_int64, ctypes.c_int, vp, ctypes.c_int64, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    assert f(None, 10, 27, None, 4, 3, None, None, None, None, None, None) == -1
    msg = lib.spart_last_error(None)
    assert msg.startswith(b"spart_lut_summarise") and b"null context" in msg


# ---- retrieve_stream's chunk arithmetic with an injected search / summary pair
class PairStage:
    """the stage interface of spart_amd.lut._stream_chunks on the host: a search and a summary in numpy, two buffers"""

    def __init__(self, search, summary):
        self.search, self.summary = search, summary
        self.inp, self.res, self.sizes = [None, None], [None, None], []

    def upload(self, j, obs, w):
        assert obs.flags.c_contiguous and (w is None or (w.flags.c_contiguous and w.shape == obs.shape))
        self.inp[j] = (obs, w)

    def launch(self, j, n):
        obs, w = self.inp[j]
        assert obs.shape[0] == n
        self.sizes.append(n)
        idx, cost = self.search(obs, w)
        mean, median, std, count = self.summary(idx)
        self.res[j] = {"mean": mean, "median": median, "std": std, "count": count, "best_cost": cost[:, 0]}

    def download(self, j, n, dest):
        for name, a in dest.items():
            assert a.shape[0] == n
            a[...] = self.res[j][name]


@pytest.fixture()
def lut_dir(tmp_path):
    rng = np.random.default_rng(5)
    B, nb = 300, 6
    d = tmp_path / "lut"
    d.mkdir()
    from spart_amd import workloads
    np.save(d / "params.npy", rng.uniform(0, 10, (B, workloads.NPARAM)))
    np.save(d / "R_TOC.npy", rng.uniform(0, 0.6, (B, nb)).astype(np.float32))
    with open(d / "meta.json", "w") as f:
        json.dump({"dtype": "float32", "columns": ["R_TOC"], "rows": B, "param_names": workloads.PARAM_NAMES}, f)
    return str(d)


@pytest.mark.parametrize("weights", ["none", "shared", "per_observation"])
def test_retrieve_stream_chunks_give_the_arrays_of_one_call(lut_dir, weights):
    from spart_amd import retrieve_stream
    k, M = 4, 23
    lut = np.load(os.path.join(lut_dir, "R_TOC.npy"))
    params = np.load(os.path.join(lut_dir, "params.npy"))[:, [15, 0]]
    rng = np.random.default_rng(9)
    obs = (lut[rng.integers(0, lut.shape[0], M)] + rng.normal(0, 0.02, (M, lut.shape[1]))).astype(np.float32)
    obs[5, 2] = np.nan
    w = {"none": None, "shared": rng.uniform(0.5, 2, lut.shape[1]), "per_observation": rng.uniform(0.5, 2, obs.shape)}[weights]
    if weights == "per_observation":
        w[5, 2] = 0.0                                              # masked: observation 5 still matches
        w[6, 1] = -1.0                                             # a negative weight: observation 6 matches nothing
    shared = None if weights != "shared" else w.astype(np.float32)

    def search(o, wc):
        if weights == "per_observation":
            return bf.brute_force_topk_obs_weights_numpy(lut, o, k, wc)
        assert wc is None
        return bf.brute_force_topk_numpy(lut, o, k, shared)

    def summary(idx):
        return bf.summarise_defined(params, idx)
    widx, wcost = search(obs, None if weights != "per_observation" else w.astype(np.float32))
    want = dict(zip(("mean", "median", "std", "count"), summary(widx)), best_cost=wcost[:, 0])
    if weights == "per_observation":
        assert want["count"][6] == 0 and want["count"][5] == k
    else:
        assert want["count"][5] == 0 and np.isnan(want["mean"][5]).all() and np.isinf(want["best_cost"][5])
    for chunk, sizes in ((1, [1] * M), (7, [7, 7, 7, 2]), (M, [M]), (M + 1, [M])):
        stage = PairStage(search, summary)
        got = retrieve_stream(lut_dir, obs, k, weights=w, params_cols=["LAI", "Cab"], chunk=chunk, _stage=stage)
        assert stage.sizes == sizes and got["names"] == ["LAI", "Cab"]
        assert sorted(got) == sorted(list(want) + ["names"])
        for name, a in want.items():
            assert got[name].dtype == a.dtype and same(got[name], a), (chunk, name)
    # caller-owned arrays are filled in place
    out = {n: np.full_like(a, 7) for n, a in want.items()}
    got = retrieve_stream(lut_dir, obs, k, weights=w, params_cols=["LAI", "Cab"], chunk=7, out=out, _stage=PairStage(search, summary))
    assert all(got[n] is out[n] and same(out[n], want[n]) for n in want)
    with pytest.raises(ValueError, match="out"):
        retrieve_stream(lut_dir, obs, k, out={**out, "count": out["count"].astype(np.int64)}, params_cols=["LAI", "Cab"],
                        _stage=PairStage(search, summary))


def test_retrieve_stream_without_observations(lut_dir):
    from spart_amd import retrieve_stream, workloads
    stage = PairStage(None, None)
    got = retrieve_stream(lut_dir, np.empty((0, 6), dtype=np.float32), 3, _stage=stage)
    assert stage.sizes == [] and got["names"] == list(workloads.PARAM_NAMES)
    assert got["mean"].shape == got["median"].shape == got["std"].shape == (0, 27)
    assert got["count"].shape == got["best_cost"].shape == (0,) and got["count"].dtype == np.int32
    with pytest.raises(ValueError):
        retrieve_stream(lut_dir, np.empty((0, 5), dtype=np.float32), 3, _stage=stage)          # another band count
    with pytest.raises(ValueError):
        retrieve_stream(lut_dir, np.empty((0, 6), dtype=np.float32), 257, _stage=stage)


def test_retrieve_refuses_bad_summary_arguments(lut_dir, monkeypatch):
    from spart_amd import lut, retrieve, retrieve_stream
    obs = np.zeros((2, 6), dtype=np.float32)
    with pytest.raises(ValueError, match="summary"):
        retrieve(lut_dir, obs, 3, summary="gpu")
    for summary in ("host", "device"):
        with pytest.raises(ValueError, match="params_cols"):
            retrieve(lut_dir, obs, 3, summary=summary, params_cols=["LAI", "leaf_area"])
    with pytest.raises(ValueError, match="params_cols"):
        retrieve_stream(lut_dir, obs, 3, params_cols=["lai"])
    monkeypatch.setattr(lut, "_group_info", lambda shard, group: (2, 0) if shard else (1, 0))    # a world of two ranks
    with pytest.raises(ValueError, match="shard"):
        retrieve(lut_dir, obs, 3, summary="device", shard=True)
