"""The host side of the posterior quantiles without a GPU: the struct layouts of the binding, the level check, and what
retrieve / retrieve_stream do with bayes={"quantiles": ...} before (or without) any device work."""
import ctypes
import json
import math
import os

import numpy as np
import pytest


def test_struct_layouts_embed_the_plain_ones():
    from spart_amd import _lib
    assert ctypes.sizeof(_lib.SpartLutBayesQOpt) == 40 and _lib.SpartLutBayesQOpt.base.offset == 0
    assert _lib.SpartLutBayesQOpt.nq.offset == 24 and _lib.SpartLutBayesQOpt.levels.offset == 32
    assert ctypes.sizeof(_lib.SpartLutBayesQOut) == 64 and _lib.SpartLutBayesQOut.quant.offset == 56
    assert "spart_lut_bayes_quantiles" in _lib.SIGNATURES and _lib.LUT_BAYES_MAXQ == 8


def test_levels_are_checked():
    from spart_amd.engine import quantile_levels
    assert quantile_levels([0.05, 0.5, 0.95]) == [0.05, 0.5, 0.95] and quantile_levels(np.array([1.0, 0.0, 0.0])) == [1.0, 0.0, 0.0]
    assert quantile_levels((0.5,) * 8) == [0.5] * 8
    for bad in ([], [0.5] * 9, [1.5], [-0.01], [math.nan], [math.inf], 0.5, "median", [None], None):
        with pytest.raises(ValueError, match="quantiles"):
            quantile_levels(bad)


def write_lut(path, B=20, nb=4):
    os.makedirs(path)
    rng = np.random.default_rng(0)
    np.save(os.path.join(path, "R_TOC.npy"), rng.uniform(0, 1, (B, nb)).astype(np.float32))
    np.save(os.path.join(path, "params.npy"), rng.uniform(0, 1, (B, 27)))
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump({"sensor": "Sentinel2A-MSI", "dtype": "float32", "rows": B, "columns": ["R_TOC"], "band_model": "centre"}, f)


def test_retrieve_checks_the_levels_and_fills_unmatched_quantiles_without_a_device(tmp_path, monkeypatch):
    import spart_amd
    import spart_amd.lut as L

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(L, "get_engine", no_engine)
    path = str(tmp_path / "lut")
    write_lut(path)
    obs = np.zeros((3, 4), dtype=np.float32)
    for call in (spart_amd.retrieve, spart_amd.retrieve_stream):
        for bad in ([], [0.5] * 9, [1.5], [math.nan], 0.5, "median"):
            with pytest.raises(ValueError, match="quantiles"):
                call(path, obs, 3, bayes={"quantiles": bad})
    assert "quantiles" in L.BAYES_OPTS
    assert L._bayes_setup({"quantiles": (0.05, 0.5)}) == {"cut": 50.0, "temperature": 1.0, "quantiles": [0.05, 0.5]}
    assert L._bayes_setup({"quantiles": None}) == {"cut": 50.0, "temperature": 1.0}
    assert "bayes_quantiles" not in L._bayes_shapes(3, 2) and "bayes_quantiles" not in L._bayes_shapes(3, 2, {"cut": 1.0})
    assert L._bayes_shapes(3, 2, {"quantiles": [0.1, 0.5, 0.9, 1.0]})["bayes_quantiles"] == ((3, 2, 4), np.float64)
    # an empty table and M = 0: NaN beside the definition's empty outputs, no device
    empty = str(tmp_path / "empty")
    write_lut(empty, B=0)
    q = {"quantiles": [0.05, 0.5, 0.95]}
    r = spart_amd.retrieve_stream(empty, obs, 3, bayes=q, params_cols=["LAI", "Cab"])
    assert r["bayes_quantiles"].shape == (3, 2, 3) and np.isnan(r["bayes_quantiles"]).all() and r["bayes_count"].tolist() == [0, 0, 0]
    r = spart_amd.retrieve_stream(path, obs[:0], 3, bayes=q)
    assert r["bayes_quantiles"].shape == (0, 27, 3) and r["bayes_quantiles"].dtype == np.float64
    r = L._retrieve_bayes(empty, obs, "R_TOC", None, None, [0, 1], L._bayes_setup(q))
    assert r["bayes_quantiles"].shape == (3, 2, 3) and np.isnan(r["bayes_quantiles"]).all() and r["bayes_std"].shape == (3, 2)
    r = L._retrieve_bayes(path, obs[:0], "R_TOC", None, None, [0, 1], L._bayes_setup(q))
    assert r["bayes_quantiles"].shape == (0, 2, 3)
    assert "bayes_quantiles" not in spart_amd.retrieve_stream(empty, obs, 3, bayes={})
