"""The argument checks of the four LUT searches (spart_lut_nearest, _topk, _topk_wide, _topk_obs_weights) on the MI355X: one
table of refusals over all of them -- every case returns its documented code before anything is launched and leaves the
outputs alone -- and the valid call beside them."""
import pytest

from helpers.lut_calls import DT, ENTRIES, FILL, bf, eng, lut_call, tdtype, torch_mod  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_lut_refusals(torch_mod, eng, bf, entry, dtype):
    torch = torch_mod
    family, nb_max, _ = ENTRIES[entry]
    per_obs = entry == "spart_lut_topk_obs_weights"
    k = None if entry == "spart_lut_nearest" else 4
    B, nb, M = 100, 13, 3
    lut = torch.rand((B, nb), device="cuda:0", dtype=tdtype(torch, dtype))
    obs = lut[:M].clone()
    w = torch.ones((M, nb) if per_obs else (nb,), device="cuda:0", dtype=lut.dtype)
    ws_bytes = getattr(eng.lib, family + "_workspace_bytes")
    kk = () if k is None else (k,)
    dt = DT[dtype]
    need = int(ws_bytes(dt, B, nb, M, *kk))
    assert need > 0

    def refused(code, text, k=k, **kw):
        rc, idx, cost, _ = lut_call(torch, eng, entry, lut, obs, k, w, dtype, **kw)
        assert rc == code and text in eng.lib.spart_last_error(None).decode(), (kw, rc, eng.lib.spart_last_error(None))
        assert bool((idx == FILL).all()) and bool((cost == FILL).all()), kw          # nothing was written
        assert eng.lib.spart_last_error(None).decode().startswith(entry + ": ")

    for bad_nb in (0, nb_max + 1):
        refused(-1, "bad sizes", nb=bad_nb)
        assert ws_bytes(dt, B, bad_nb, M, *kk) == 0
    if k is not None:
        for bad_k in (0, 257):
            refused(-1, f"k = {bad_k}, expected 1 <= k <= 256", k=bad_k)
            assert ws_bytes(dt, B, nb, M, bad_k) == 0
    refused(-1, "bad dtype 2", dt=2)
    for name in ("lut", "obs", "idx", "cost"):
        refused(-1, "null argument", null=(name,))
    if per_obs:
        refused(-1, "null argument", null=("w",))
    refused(-3, f"workspace of {need} bytes needed, {need - 1} given", ws_bytes=need - 1)
    refused(-1, "empty LUT", B=0)
    # M == 0: nothing to do, no error, the outputs untouched
    rc, idx, cost, st = lut_call(torch, eng, entry, lut, obs, k, w, dtype, M=0)
    assert rc == 0 and st == {} and bool((idx == FILL).all()) and bool((cost == FILL).all())
    # the valid call, with and (where they are optional) without weights: the brute force's answer
    for ww in (w,) if per_obs else (w, None):
        rc, idx, cost, st = lut_call(torch, eng, entry, lut, obs, k, ww, dtype)
        assert rc == 0 and st["brute_force"] >= 0, eng.lib.spart_last_error(None)
        if per_obs:
            ti, tc = bf.brute_force_topk_obs_weights_torch(lut, obs, k, ww)
        else:
            ti, tc = bf.brute_force_topk_torch(lut, obs, 1 if k is None else k, ww)
        if k is None:
            ti, tc = ti[:, 0], tc[:, 0]
        assert torch.equal(idx, ti) and torch.equal(cost, tc)
