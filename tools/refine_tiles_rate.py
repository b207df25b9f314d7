"""Rates of the refinement with parameters shared by a tile (spart_refine_tiles) against spart_refine with the same F, M and
n_iter: the forward calls are identical, so the difference is the tile kernels against k_refine_step.

    python tools/refine_tiles_rate.py [--pixels 262144] [--iters 10] [--reps 10] [--out profiles/refine_tiles_rate.txt]

Workload: Sentinel-2A (nb = 13), R_TOA, M LHS rows as the truth with one aot550 per tile, Fs = 1 shared parameter (aot550) and
Fl = 2 local ones (LAI, Cab), started 10 % of their range away, float64; tiles of 64 and of 4096 pixels.
  a  the whole call (Engine.refine_tiles / Engine.refine with F = 3), device events, medians after two warm-up calls;
then, from a separate run of the three calls in a child process under `rocprofv3 --kernel-trace --stats` with no counters, the
time of every kernel of the family per call and its share.  Every figure in the report is measured in this run.
"""
import argparse
import csv
import glob
import os
import signal
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from refine_rate import SENSOR, event_ms, stats  # noqa: E402

SHARED, LOCAL = ["aot550"], ["LAI", "Cab"]
TILES = (64, 4096)
PER_PIXEL = ("k_tiles_init", "k_tiles_cost", "k_tiles_normal", "k_tiles_eliminate", "k_tiles_local", "k_tiles_apply")
PER_TILE = ("k_tiles_decide", "k_tiles_schur")
KERNELS = PER_PIXEL + PER_TILE + ("k_refine_step", "k_columns", "k_prelude", "k_bands")


def workload(torch, eng, M, G):
    """(start (27, M), obs (M, nb)) device tensors with one aot550 per run of G pixels"""
    from spart_amd import workloads
    names = SHARED + LOCAL
    cols = [workloads.PARAM_NAMES.index(n) for n in names]
    lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
    truth = workloads.lhs_params(M, "full", seed=77)
    truth[:, cols[0]] = truth[(np.arange(M) // G) * G, cols[0]]
    rows = torch.as_tensor(np.ascontiguousarray(truth.T), device=eng.device)
    obs = eng.run(rows, "float64", prune=True)["R_TOA"].contiguous()
    start = truth.copy()
    start[:, cols] = truth[:, cols] + 0.1 * (hi - lo) * np.sign(0.5 * (lo + hi) - truth[:, cols])
    return torch.as_tensor(np.ascontiguousarray(start.T), device=eng.device), obs


def calls_of(torch, eng, a):
    """{label: a function that queues one call}"""
    out = {}
    for G in TILES:
        start, obs = workload(torch, eng, a.pixels, G)
        out[f"tiles of {G}"] = (lambda s=start, o=obs, g=G: eng.refine_tiles(s, o, SHARED, LOCAL, tile_size=g, column="R_TOA", n_iter=a.iters))
    out["spart_refine"] = lambda s=start, o=obs: eng.refine(s, o, LOCAL + SHARED, column="R_TOA", n_iter=a.iters)
    return out


def child(a):
    """the program rocprofv3 is pointed at: two calls of ONE of the three"""
    import torch
    from spart_amd import get_engine
    eng = get_engine(SENSOR, 0)
    f = calls_of(torch, eng, a)[a.child]
    for _ in range(2):
        f()
    torch.cuda.synchronize()


def kernel_rows(a, label):
    """--child under rocprofv3 --kernel-trace --stats in a fresh process group -> ({kernel: total ms of one call}, note)"""
    d = tempfile.mkdtemp(prefix="refine_tiles_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", label, "--pixels", str(a.pixels), "--iters", str(a.iters)]
    try:
        proc = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
    except OSError as e:
        return {}, f"(rocprofv3 could not be started: {e})"
    try:
        rc = proc.wait(timeout=a.trace_timeout)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        proc.wait()
        return {}, f"(rocprofv3 run killed after {a.trace_timeout} s)"
    if rc != 0:
        return {}, f"(rocprofv3 run failed: exit status {rc})"
    rows = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            hit = [k for k in KERNELS if k in row["Name"]]
            if hit:
                k = max(hit, key=len)
                rows[k] = rows.get(k, 0.0) + int(row["Calls"]) * float(row["AverageNs"]) / 1e6 / 2       # (two calls in the child)
    return rows, "" if rows else "(no kernel rows in the kernel stats)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=262144)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-timeout", type=int, default=240, help="seconds one rocprofv3 run may take")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    from spart_amd import get_engine
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = get_engine(SENSOR, 0)
    M, F = a.pixels, len(SHARED) + len(LOCAL)
    say(f"spart_refine_tiles on MI355X (one GCD), tools/refine_tiles_rate.py: {SENSOR}, nb = {eng.nb}, R_TOA, M = {M} pixels, shared "
        f"{SHARED}, local {LOCAL}, n_iter = {a.iters} ({a.iters + 1} forward calls of {(F + 1) * M} rows, in chunks of "
        f"{(1 << 19) // (F + 1)} pixels), float64; device events, medians of {a.reps} after 2 warm-up calls.")
    say()
    fs = calls_of(torch, eng, a)
    med = {}
    for label, f in fs.items():
        res = {}
        ts = event_ms(torch, lambda: res.update(f()), a.reps)
        med[label] = float(np.median(ts))
        cost, cost0, na = (res[k].cpu().numpy() for k in ("cost", "cost0", "n_accept"))
        alive = na >= 0
        say(f"  a  {label:16s}{stats(ts)}   {int(alive.sum())} of {na.size} alive, median cost / cost0 = "
            f"{np.median(cost[alive] / cost0[alive]):.3e}, median accepted steps = {np.median(na[alive]):.0f}")
    for G in TILES:
        say(f"  tiles of {G} / spart_refine = {med[f'tiles of {G}'] / med['spart_refine']:.3f}")
    say()
    ok = True
    if a.no_trace:
        say("rocprofv3 --kernel-trace --stats: (not collected: --no-trace)")
    for label in ([] if a.no_trace else fs):
        rows, note = kernel_rows(a, label)
        ok = ok and not note
        total = sum(rows.values())
        say(f"rocprofv3 --kernel-trace --stats, {label} (a separate run, 2 calls in a fresh process; ms of ONE call): {note}")
        for k, ms in sorted(rows.items(), key=lambda kv: -kv[1]):
            say(f"  {k:20s} {ms:9.3f} ms  {100 * ms / total:5.1f} %")
        if rows and label != "spart_refine":
            pp, pt = sum(rows.get(k, 0.0) for k in PER_PIXEL), sum(rows.get(k, 0.0) for k in PER_TILE)
            say(f"  per-pixel tile kernels {pp:.3f} ms, per-tile kernels {pt:.3f} ms" +
                ("  -- the per-tile kernels take MORE than the per-pixel ones" if pt > pp else ""))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
