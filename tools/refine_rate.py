"""Rates of the device-resident refinement (spart_refine) against the forward evaluations it is built around.

    python tools/refine_rate.py [--obs 262144] [--free 6] [--iters 10] [--reps 20] [--prior none|shared|per_obs]
                                [--band-model centre|srf] [--out profiles/refine_rate.txt]

Workload: Sentinel-2A (nb = 13), M LHS rows as the truth, the free parameters started 10 % of their range away, float64.
  a  the whole spart_refine call (Engine.refine: k_refine_views_init, n_iter + 1 forward calls, n_iter + 1 step kernels);
  b  the same n_iter + 1 forward calls alone, eng.run(..., "float64", prune=True) on (F + 1) M rows -- the yardstick: the
     parent commit's kernels on the same number of rows;
  c  the step kernel's own time per iteration, two ways: (a - b) / (n_iter + 1) by device events (it also holds the init
     kernel and the forward calls' chunking), and k_refine_step's row of `rocprofv3 --kernel-trace --stats` from a separate run
     in a child process.
``--prior``: the Gaussian prior of the call -- none (the default), shared ((F,) mean and weight) or per_obs ((M, F)); the means
are the truth, sigma a tenth of the range.
``--band-model srf`` (profiles/refine_srf_rate.txt): spart_refine_srf -- the observations are the SRF-convolved column, a is
Engine.refine(band_model="srf"), b is eng.run(..., "float64", prune=True, materialize=["R_TOC_srf"]) (which also launches the
centre column kernel, as spart_run_batch always does) -- followed by a and b of the centre model measured in the same session.
The goal is c <= a quarter of one forward call.  Device events, medians after two warm-up calls; every figure in the report is
measured in this run.
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
SENSOR = "Sentinel2A-MSI"
NAMES = ["LAI", "Cab", "Cw", "Cdm", "N", "B", "Cca", "Cs", "SMp", "q", "LIDFa", "LIDFb", "aot550", "uo3", "uh2o", "Cant"]


def stats(ts):
    return f"{np.median(ts):9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, n = {len(ts)})"


def event_ms(torch, f, reps, warm=2):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def prior_of(torch, eng, M, F, kind):
    """keywords of Engine.refine for --prior: device tensors, the truth of workload() as the mean, sigma = 10 % of the range"""
    if kind == "none":
        return {}
    from spart_amd import workloads
    names = NAMES[:F]
    cols = [workloads.PARAM_NAMES.index(n) for n in names]
    lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
    truth = workloads.lhs_params(M, "full", seed=77)[:, cols]
    sigma = 0.1 * (hi - lo)
    mean = np.ascontiguousarray(truth) if kind == "per_obs" else 0.5 * (lo + hi)
    weight = np.broadcast_to(1.0 / (sigma * sigma), mean.shape).copy()
    return {"prior_mean": torch.as_tensor(mean, device=eng.device), "prior_weight": torch.as_tensor(weight, device=eng.device)}


def workload(torch, eng, M, F, srf=False):
    """(start (27, M) device tensor, obs (M, nb) device tensor, names); srf: the observations are the SRF-convolved column"""
    from spart_amd import workloads
    names = NAMES[:F]
    cols = [workloads.PARAM_NAMES.index(n) for n in names]
    lo, hi = (np.array([workloads.RANGES[n][i] for n in names]) for i in (0, 1))
    truth = workloads.lhs_params(M, "full", seed=77)
    col = "R_TOC_srf" if srf else "R_TOC"
    obs = eng.run(torch.as_tensor(truth.T.copy(), device=eng.device), "float64", prune=True, materialize=[col] if srf else ())[col].clone()
    start = truth.copy()
    start[:, cols] = truth[:, cols] + 0.1 * (hi - lo) * np.sign(0.5 * (lo + hi) - truth[:, cols])
    return torch.as_tensor(start.T.copy(), device=eng.device), obs, names


def child(a):
    """the program rocprofv3 is pointed at: three refinement calls"""
    import torch
    from spart_amd import get_engine
    eng = get_engine(SENSOR, 0)
    start, obs, names = workload(torch, eng, a.obs, a.free, a.band_model == "srf")
    prior = prior_of(torch, eng, a.obs, a.free, a.prior)
    for _ in range(3):
        eng.refine(start, obs, names, n_iter=a.iters, band_model=a.band_model, **prior)
    torch.cuda.synchronize()


def kernel_lines(a):
    """--child under rocprofv3 --kernel-trace --stats in a fresh process group -> ({kernel: (calls, average ms, min, max)}, note)"""
    d = a.trace_dir or tempfile.mkdtemp(prefix="refine_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", "--obs", str(a.obs), "--free", str(a.free), "--iters", str(a.iters), "--prior", a.prior, "--band-model", a.band_model]
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
            for k in ("k_refine_step", "k_refine_views_init", "k_columns_srf", "k_columns", "k_prelude"):
                if k in row["Name"] and not (k == "k_columns" and "k_columns_srf" in row["Name"]):
                    rows[k] = (int(row["Calls"]), float(row["AverageNs"]) / 1e6, float(row["MinNs"]) / 1e6, float(row["MaxNs"]) / 1e6)
    return rows, "" if "k_refine_step" in rows else "(no k_refine_step row in the kernel stats)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=262144)
    ap.add_argument("--free", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prior", choices=("none", "shared", "per_obs"), default="none")
    ap.add_argument("--band-model", choices=("centre", "srf"), default="centre")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-timeout", type=int, default=240, help="seconds the rocprofv3 run may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if not 1 <= a.free <= len(NAMES):
        ap.error("--free: 1 ... 16")
    if a.child:
        return child(a)
    import torch
    from spart_amd import get_engine
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = get_engine(SENSOR, 0)
    M, F, nb, calls = a.obs, a.free, eng.nb, a.iters + 1
    rows = (F + 1) * M
    chunk = (1 << 19) // (F + 1)
    entry = "spart_refine_srf" if a.band_model == "srf" else "spart_refine"
    say(f"{entry} on MI355X (one GCD), tools/refine_rate.py: {SENSOR}, nb = {nb}, M = {M} observations, F = {F} free parameters "
        f"{NAMES[:F]}, prior = {a.prior}, n_iter = {a.iters} ({calls} forward calls of {rows} rows, in chunks of {chunk} observations), float64; device "
        f"events, medians of {a.reps} after 2 warm-up calls.")
    say()

    def measure(band_model):
        """a and b for one band model -> (median a, median b) in ms"""
        srf = band_model == "srf"
        start, obs, names = workload(torch, eng, M, F, srf)
        prior = prior_of(torch, eng, M, F, a.prior)
        res = {}

        def call_a():
            res.update(eng.refine(start, obs, names, n_iter=a.iters, band_model=band_model, **prior))
        Pf = torch.as_tensor(np.ascontiguousarray(np.tile(start.cpu().numpy(), (1, F + 1))), device=eng.device)
        fields = ["R_TOC_srf"] if srf else []
        out = {k: torch.empty((rows, nb), dtype=torch.float64, device=eng.device) for k in ["R_TOC", "R_TOA", "L_TOA"] + fields}

        def call_b():
            for _ in range(calls):
                eng.run(Pf, "float64", out=out, prune=True, materialize=fields)
        ta = event_ms(torch, call_a, a.reps)
        tb = event_ms(torch, call_b, a.reps)
        ma, mb = float(np.median(ta)), float(np.median(tb))
        name = "spart_refine_srf" if srf else "spart_refine"
        what = 'materialize=["R_TOC_srf"]; ' if srf else ""
        say(f"  a  the whole {name} call{' ' * (35 - len(name))}{stats(ta)}   = {ma * 1e6 / M:.1f} ns per observation")
        say(f"  b  {calls} forward calls alone ({what}(F + 1) M = {rows} rows each)   {stats(tb)}   = {mb / calls:.3f} ms per call, "
            f"{mb * 1e6 / (calls * rows):.2f} ns per row")
        say(f"     a / b = {ma / mb:.3f}")
        say(f"  c  (a - b) / {calls}: init, step kernel and chunking per iteration   {(ma - mb) / calls:9.3f} ms   = "
            f"{(ma - mb) / mb:.3f} of the forward time of its iteration")
        nchunks = (M + chunk - 1) // chunk
        say(f"     a / {calls} / {nchunks} chunks = {ma / calls / nchunks:.3f} ms per iteration of one chunk of {min(M, chunk)} observations")
        cost, cost0, na = (res[k].cpu().numpy() for k in ("cost", "cost0", "n_accept"))
        alive = na >= 0
        say(f"     the fit: {int(alive.sum())} of {M} observations alive, median cost / cost0 = {np.median(cost[alive] / cost0[alive]):.3e}, "
            f"median accepted steps = {np.median(na[alive]):.0f}")
        say()
        del out, Pf
        torch.cuda.empty_cache()
        return ma, mb
    ma, mb = measure(a.band_model)
    if a.band_model == "srf":
        say("the centre model (spart_refine) on the same shape, in the same session:")
        ca, cb = measure("centre")
        say(f"  srf / centre: the whole call {ma / ca:.2f}, the forward calls {mb / cb:.2f}")
        say()
    ok = True
    if a.no_trace:
        say("rocprofv3 --kernel-trace --stats: (not collected: --no-trace)")
    else:
        rows_, note = kernel_lines(a)
        ok = not note
        say(f"rocprofv3 --kernel-trace --stats (a separate run, 3 calls of a in a fresh process): {note}")
        for k, (n, avg, lo_, hi_) in sorted(rows_.items()):
            say(f"  {k:14s} {n:5d} calls, average {avg:.3f} ms (min {lo_:.3f}, max {hi_:.3f})")
        if a.band_model == "centre" and "k_refine_step" in rows_ and "k_columns" in rows_ and "k_prelude" in rows_:
            # per iteration of one chunk: one prelude + one column kernel against one step kernel
            fwd = rows_["k_columns"][1] + rows_["k_prelude"][1]
            ratio = rows_["k_refine_step"][1] / fwd
            say(f"  k_refine_step / (k_prelude + k_columns) = {ratio:.3f}   goal (at most 0.25): {'met' if ratio <= 0.25 else 'MISSED'}")
            bytes_ = (F + 1) * nb * 8 + F * (F + 1) * 8
            say(f"  the step kernel reads at least {(F + 1) * nb * 8} B of columns and writes {F * (F + 1) * 8} B of table per observation that "
                f"moves: {bytes_ * min(M, chunk) / (rows_['k_refine_step'][1] * 1e-3) / 1e12:.2f} TB/s if every observation did")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
