"""Rates of the refinement of time series with a smoothness prior (spart_refine_series) against spart_refine_tiles with tiles
equal to the series on the same rows: the forward calls are identical, so the difference is the chain kernels against tiles'
k_tiles_decide / _eliminate / _schur / _local.

    python tools/refine_series_rate.py [--rows 262144] [--dates 32] [--iters 10] [--reps 10] [--out profiles/refine_series_rate.txt]

Workload: Sentinel-2A (nb = 13), R_TOA, M rows in series of 32 dates, Fs = 1 shared parameter (LIDFa) and Fl = 2 local ones
(LAI, Cab) tied with sigma = 5 % of their range, started 10 % of their range away, float64.
  a  the whole call (Engine.refine_series / Engine.refine_tiles), device events, medians after two warm-up calls;
then, from a separate run of each call in a child process under `rocprofv3 --kernel-trace --stats` with no counters, the time of
every kernel of the family per call and its share.  Every figure in the report is measured in this run.
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
from refine_tiles_rate import KERNELS as TILES_KERNELS  # noqa: E402

SHARED, LOCAL = ["LIDFa"], ["LAI", "Cab"]
CHAIN = ("k_series_decide", "k_series_augment", "k_series_sums", "k_series_factor", "k_series_shared", "k_series_back", "k_series_std")
KERNELS = TILES_KERNELS + CHAIN


def workload(torch, eng, M, T):
    from spart_amd import workloads
    names = SHARED + LOCAL
    cols = [workloads.PARAM_NAMES.index(n) for n in names]
    lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
    truth = workloads.lhs_params(M, "full", seed=77)
    first = (np.arange(M) // T) * T
    truth[:, cols[0]] = truth[first, cols[0]]
    phase = (np.arange(M) % T + 0.5) / T                                # the locals follow a season's bell around the series' draw
    for c, l, h in zip(cols[1:], lo[1:], hi[1:]):
        truth[:, c] = np.clip(truth[first, c] + 0.2 * (h - l) * (np.sin(np.pi * phase) ** 2 - 0.5), l, h)
    rows = torch.as_tensor(np.ascontiguousarray(truth.T), device=eng.device)
    obs = eng.run(rows, "float64", prune=True)["R_TOA"].contiguous()
    start = truth.copy()
    start[:, cols] = truth[:, cols] + 0.1 * (hi - lo) * np.sign(0.5 * (lo + hi) - truth[:, cols])
    smooth = {n: 0.05 * (h - l) for n, l, h in zip(LOCAL, lo[1:], hi[1:])}
    return torch.as_tensor(np.ascontiguousarray(start.T), device=eng.device), obs, smooth


def calls_of(torch, eng, a):
    start, obs, smooth = workload(torch, eng, a.pixels, a.dates)
    return {"series": lambda: eng.refine_series(start, obs, SHARED, LOCAL, n_dates=a.dates, smooth=smooth, column="R_TOA", n_iter=a.iters),
            "tiles": lambda: eng.refine_tiles(start, obs, SHARED, LOCAL, tile_size=a.dates, column="R_TOA", n_iter=a.iters)}


def child(a):
    """the program rocprofv3 is pointed at: two calls of ONE of the two"""
    import torch
    from spart_amd import get_engine
    eng = get_engine(SENSOR, 0)
    f = calls_of(torch, eng, a)[a.child]
    for _ in range(2):
        f()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", "--pixels", dest="pixels", type=int, default=262144)
    ap.add_argument("--dates", type=int, default=32)
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
    say(f"spart_refine_series on MI355X (one GCD), tools/refine_series_rate.py: {SENSOR}, nb = {eng.nb}, R_TOA, M = {M} rows in series of "
        f"{a.dates}, shared {SHARED}, local {LOCAL} (tied, sigma = 5 % of the range), n_iter = {a.iters} ({a.iters + 1} forward calls of "
        f"{(F + 1) * M} rows, in chunks of {(1 << 19) // (F + 1)} rows), float64; device events, medians of {a.reps} after 2 warm-up "
        "calls.  spart_refine_tiles: the same rows as tiles of the same size, no tie.")
    say()
    fs = calls_of(torch, eng, a)
    med = {}
    for label, f in fs.items():
        res = {}
        ts = event_ms(torch, lambda: res.update(f()), a.reps)
        med[label] = float(np.median(ts))
        cost, cost0, na = (res[k].cpu().numpy() for k in ("cost", "cost0", "n_accept"))
        alive = na >= 0
        say(f"  a  {label:8s}{stats(ts)}   {int(alive.sum())} of {na.size} alive, median cost / cost0 = "
            f"{np.median(cost[alive] / cost0[alive]):.3e}, median accepted steps = {np.median(na[alive]):.0f}")
    say(f"  series / tiles = {med['series'] / med['tiles']:.3f}")
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
        if rows and label == "series":
            chain = sum(rows.get(k, 0.0) for k in CHAIN)
            fwd = sum(rows.get(k, 0.0) for k in ("k_columns", "k_prelude", "k_bands"))
            say(f"  chain kernels {chain:.3f} ms, forward kernels {fwd:.3f} ms" +
                ("  -- the chain kernels take MORE than the forward call" if chain > fwd else ""))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


def kernel_rows(a, label):
    """--child under rocprofv3 --kernel-trace --stats in a fresh process group -> ({kernel: total ms of one call}, note)"""
    d = tempfile.mkdtemp(prefix="refine_series_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", label, "--rows", str(a.pixels), "--dates", str(a.dates), "--iters", str(a.iters)]
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


if __name__ == "__main__":
    sys.exit(main())
