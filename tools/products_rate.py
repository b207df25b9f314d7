"""Rate of spart_products against the float64 full-band evaluation it shares its per-band chain with.

    python tools/products_rate.py [--rows 1000000] [--reps 7] [--out profiles/products_rate.txt]

Workload: --rows LHS parameter rows ("full"), resident on the device.  In ONE run, alternating, by device events, medians of
--reps after one warm-up each:
  a  Engine.products: spart_products, all five outputs (the literal prelude with the leaf, soil and canopy groups, then
     k_products over the 2001 model bands);
  b  Engine.run(dtype="float64", prune=False): spart_run_batch with prune_unused_bands = 0 on a Sentinel-2A context (the
     prelude with all four groups, the float64 full-band kernel over 2162 band evaluations with the whole canopy solve and its
     band sums, and the column kernel on a side stream).
The comparison is fair because both evaluate the same float64 leaf, soil and canopy chain once per sample and band; b does
more per band (the view-direction half of the solve, cross-sample sums) and 8 % more bands.  A per-kernel split needs a
kernel trace in a run of its own:  rocprofv3 --kernel-trace --stats -d /tmp/products_trace -- python tools/products_rate.py --reps 2
One text report; every figure in it is measured in this run.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))


def stats(ts):
    return f"{np.median(ts):9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, n = {len(ts)})"


def timed(torch, f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from spart_amd import PRODUCT_NAMES, get_engine, workloads
    assert torch.cuda.is_available(), "products_rate.py measures on the GPU; there is no CPU path"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B = a.rows
    P = torch.as_tensor(np.ascontiguousarray(workloads.lhs_params(B, "full", seed=21).T), device="cuda:0")
    plain, s2 = get_engine(None, 0), get_engine("Sentinel2A-MSI", 0)
    out_p = {n: torch.empty((B,), dtype=torch.float64, device="cuda:0") for n in PRODUCT_NAMES}
    out_r = {n: torch.empty((B, s2.nb), dtype=torch.float64, device="cuda:0") for n in ("R_TOC", "R_TOA", "L_TOA")}
    calls = {"products": lambda: plain.products(P, out=out_p),
             "fcover": lambda: plain.products(P, names=["fCover"], out={"fCover": out_p["fCover"]}),
             "run_f64": lambda: s2.run(P, "float64", out=out_r, prune=False)}
    for f in calls.values():
        f()                                                    # warm-up: code objects, workspaces
    ts = {n: [] for n in calls}
    for _ in range(a.reps):                                    # alternating: both see the same machine state
        for n, f in calls.items():
            ts[n].append(timed(torch, f))
    med = {n: float(np.median(v)) for n, v in ts.items()}
    say(f"spart_products on MI355X (one GCD), tools/products_rate.py: B = {B} LHS rows resident on the device, float64; device "
        f"events, alternating, medians of {a.reps} after one warm-up.")
    say(f"  a  spart_products, five outputs (prelude + k_products, 2001 bands)           {stats(ts['products'])}"
        f"   = {B / med['products'] / 1e3:.2f} M rows/s")
    say(f"     spart_products, fCover alone (prelude + the LIDF iteration, no band loop)  {stats(ts['fcover'])}")
    say(f"  b  spart_run_batch float64, prune_unused_bands = 0 (Sentinel-2A, 2162 bands)  {stats(ts['run_f64'])}"
        f"   = {B / med['run_f64'] / 1e3:.2f} M rows/s")
    say(f"  a / b = {med['products'] / med['run_f64']:.3f}   (expected from the code alone: <= 1)")
    say(f"  per sample and band: a {med['products'] * 1e6 / (B * 2001.0):.3f} ns, b {med['run_f64'] * 1e6 / (B * 2162.0):.3f} ns")
    vals = {n: v.cpu().numpy() for n, v in out_p.items()}
    say("  products of the rows: " + ", ".join(f"{n} {v.min():.3f} ... {v.max():.3f}" for n, v in vals.items())
        + f"; all finite: {all(np.isfinite(v).all() for v in vals.values())}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
