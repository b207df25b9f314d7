"""LUT top-k rate (spart_lut_topk, whole call) against spart_lut_nearest in the same process, alternating the two, on the
uniform and correlated LUTs of tools/lut_invert_rate.py; counts the observations that took the brute-force path and the
candidate tiles, and checks every result against the eager-torch brute force (tools/lut_brute_force.py).

    python tools/lut_topk_rate.py [lib.so]"""
import os, sys, time
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from lut_brute_force import brute_force_topk_torch
from spart_amd.engine import Engine
eng = Engine(None, 0, lib_path=sys.argv[1] if len(sys.argv) > 1 else None)
g = torch.Generator("cuda:0").manual_seed(7)


def correlated(B, M, nb, td):
    z = torch.rand((B, 4), device="cuda:0", dtype=torch.float64, generator=g)
    A = 1.5 * torch.randn((4, nb), device="cuda:0", dtype=torch.float64, generator=g)
    C = torch.randn((4, nb), device="cuda:0", dtype=torch.float64, generator=g)
    lut = (0.03 + 0.5 * torch.sigmoid(z @ A + (z * z) @ C - 1.0)).to(td)
    pick = torch.randint(0, B, (M,), device="cuda:0", generator=g)
    obs = (lut[pick].double() * (1 + 0.02 * torch.randn((M, nb), device="cuda:0", dtype=torch.float64, generator=g))).to(td)
    return lut, obs


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


B, M, nb = 1_000_000, 65536, 13
for dtype, td in (("float32", torch.float32), ("float64", torch.float64)):
    for kind in ("uniform", "correlated"):
        if kind == "uniform":
            lut = torch.rand((B, nb), device="cuda:0", dtype=td, generator=g)
            obs = torch.rand((M, nb), device="cuda:0", dtype=td, generator=g)
        else:
            lut, obs = correlated(B, M, nb, td)
        for k in ((10, 64) if dtype == "float32" else (10,)):
            idx, cost, st = eng.lut_topk(lut, obs, k, dtype=dtype, stats=True)
            ok = True
            for m0 in range(0, M, 8192):                   # every observation against the brute force
                ti, tc = brute_force_topk_torch(lut, obs[m0:m0 + 8192], k)
                ok = ok and torch.equal(idx[m0:m0 + 8192], ti) and torch.equal(cost[m0:m0 + 8192], tc)
            t1, tk = [], []
            for _ in range(5):                             # alternating, best of five each
                t1.append(timed(lambda: eng.lut_nearest(lut, obs, dtype=dtype)))
                tk.append(timed(lambda: eng.lut_topk(lut, obs, k, dtype=dtype)))
            a, b = min(t1), min(tk)
            print(f"{dtype} {kind} B={B} M={M} nb={nb} k={k}: top-k {b*1e3:.2f} ms, k=1 {a*1e3:.2f} ms, ratio {b/a:.2f}; "
                  f"brute-force path {st['brute_force']} of {M}, candidate tiles {st['candidate_tiles'] / M:.1f} per observation "
                  f"(max {st['max_candidate_tiles']}); exact {ok}", flush=True)
        del lut, obs
