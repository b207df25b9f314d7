"""Rate of spart_refine_leaf against the floor an unfused design would pay for its spectra.

    python tools/refine_leaf_rate.py [--leaves 10000] [--reps 20] [--n-iter 20] [--out profiles/refine_leaf_rate.txt]

Workload: BASELINE config 2's leaves (workloads.lhs_params(leaves, "leaf")), their own spectra with 1 % noise as observations,
starts at the middle of the ranges, F = 4 (Cab, Cw, Cdm, N) and F = 7 (the seven PROSPECT-5D parameters).  Per F, by device
events, medians of --reps after one warm-up:
  a  Engine.refine_leaf: ONE launch of k_refine_leaf<F>, n_iter + 1 evaluations of F + 1 leaves each, no spectra in memory;
  b  the floor of an unfused fit: n_iter + 1 calls of Engine.prospect on (F + 1) M rows (refl and tran written to memory).  A
     real unfused fit would also read them back, form J and the sums and solve; none of that is in b.
Each step runs in a child process of its own under a time limit (a step that hangs ends there and the report says so).  One
text report; every figure in it is measured in this run.  No test asserts a time.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
FREE = {4: ["Cab", "Cw", "Cdm", "N"], 7: ["Cab", "Cdm", "Cw", "Cs", "Cca", "Cant", "N"]}


def timed(torch, f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def step(F, M, n_iter, reps):
    """the child: one F, both timings -> one JSON line"""
    import torch
    from spart_amd import get_engine, workloads
    assert torch.cuda.is_available(), "refine_leaf_rate.py measures on the GPU; there is no CPU path"
    eng = get_engine(None, 0)
    rng = np.random.default_rng(5)
    truth = workloads.lhs_params(M, "leaf", seed=21)[:, :9]
    cols = [torch.as_tensor(np.ascontiguousarray(truth[:, k]), device="cuda:0") for k in range(9)]
    refl, tran, _ = eng.prospect(cols, outputs=("refl", "tran"))
    noise = lambda t: (t * (1 + 0.01 * torch.as_tensor(rng.standard_normal(tuple(t.shape)), device="cuda:0"))).contiguous()      # noqa: E731
    obs_r, obs_t = noise(refl), noise(tran)
    start = truth.copy()
    for n in FREE[F]:
        k = workloads.PARAM_NAMES.index(n)
        start[:, k] = 0.5 * sum(workloads.RANGES[n])
    leaf = torch.as_tensor(np.ascontiguousarray(start.T), device="cuda:0")
    rows = [c.repeat(F + 1) for c in cols]
    res = {}

    def fused():
        res["fit"] = eng.refine_leaf(leaf, obs_r, obs_t, free=FREE[F], n_iter=n_iter)

    def floor():
        for _ in range(n_iter + 1):
            eng.prospect(rows, outputs=("refl", "tran"))
    fused(), floor()                                            # warm-up: code objects, workspaces
    ts = {"fused": [], "floor": []}
    for _ in range(reps):
        ts["fused"].append(timed(torch, fused))
        ts["floor"].append(timed(torch, floor))
    fit = res["fit"]
    x = fit["x"].cpu().numpy()
    lo, hi = (np.array([workloads.RANGES[n][k] for n in FREE[F]]) for k in (0, 1))
    err = np.abs(x - truth[:, [workloads.PARAM_NAMES.index(n) for n in FREE[F]]]) / (hi - lo)
    print(json.dumps({"F": F, "fused": ts["fused"], "floor": ts["floor"], "median_err": float(np.median(err)),
                      "accepted": float(fit["n_accept"].double().mean().item()),
                      "cost_ratio": float((fit["cost"] / fit["cost0"]).median().item())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-iter", type=int, default=20)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step is not None:
        return step(a.step, a.leaves, a.n_iter, a.reps)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"spart_refine_leaf on MI355X (one GCD), tools/refine_leaf_rate.py: M = {a.leaves} config-2 leaves x 2001 bands, float64, "
        f"reflectance and transmittance, n_iter = {a.n_iter}; device events, medians of {a.reps} after one warm-up.")
    for F in (4, 7):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(F), "--leaves", str(a.leaves), "--reps", str(a.reps),
               "--n-iter", str(a.n_iter)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            say(f"  F = {F}: the step did not end within {a.limit} s; nothing after it was started")
            break
        if p.returncode != 0:
            say(f"  F = {F}: the step ended with status {p.returncode}; nothing after it was started\n{p.stderr[-1500:]}")
            break
        r = json.loads(p.stdout.strip().splitlines()[-1])
        fu, fl = float(np.median(r["fused"])), float(np.median(r["floor"]))
        evals = (a.n_iter + 1) * (F + 1) * a.leaves
        say(f"  F = {F}:  a  spart_refine_leaf, one launch            {fu:9.3f} ms (min {min(r['fused']):.3f}, max {max(r['fused']):.3f})"
            f"   = {evals * 2001.0 / fu / 1e6:.2f} G leaf-band evaluations/s")
        say(f"          b  {a.n_iter + 1} x Engine.prospect on {(F + 1) * a.leaves} rows   {fl:9.3f} ms (min {min(r['floor']):.3f}, max {max(r['floor']):.3f})")
        say(f"          a / b = {fu / fl:.3f};  median |x - truth| / range {r['median_err']:.2e}, accepted steps per leaf "
            f"{r['accepted']:.1f}, median cost / cost0 {r['cost_ratio']:.2e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
