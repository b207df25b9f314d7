"""Rate of spart_refine_posterior (Engine.posterior) against the forward evaluation it is built around and against the step
kernel of spart_refine on the same shape.

    python tools/refine_posterior_rate.py [--obs 262144] [--free 6] [--reps 20] [--out profiles/refine_posterior_rate.txt]

Workload: tools/refine_rate.py's -- Sentinel-2A (nb = 13), M LHS rows, the free parameters moved 10 % of their range, float64,
weights 1 / (0.02 max(obs, 0.01))^2, a shared prior of sigma = 10 % of the range.
  a  the whole call with all ten outputs (k_refine_views_init, one forward call of (F + 1) M rows in chunks, k_refine_posterior);
  b  the same call without jac (the nb F doubles per observation are the bulk of what the kernel writes);
  c  one eng.run(..., "float64", prune=True) of the same (F + 1) M rows: the yardstick;
  d  k_refine_posterior's row of `rocprofv3 --kernel-trace --stats` beside k_refine_step's, from a separate run in a child
     process that makes three posterior calls and three spart_refine calls (n_iter = 2) on the same shape.
The kernel does strictly more than a step (the inverse, F^2 products, the Jacobian store), so d's ratio is above 1.  Device
events, medians after two warm-up calls; every figure in the report is measured in this run.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refine_rate import NAMES, SENSOR, event_ms, prior_of, stats, workload  # noqa: E402

KERNELS = ("k_refine_posterior", "k_refine_step", "k_refine_views_init", "k_columns", "k_prelude")


def setup(torch, eng, M, F):
    start, obs, names = workload(torch, eng, M, F)
    w = 1.0 / (0.02 * torch.clamp(obs, min=0.01)) ** 2
    return start, obs, names, w, prior_of(torch, eng, M, F, "shared")


def child(a):
    """the program rocprofv3 is pointed at"""
    import torch
    from spart_amd import get_engine
    eng = get_engine(SENSOR, 0)
    start, obs, names, w, prior = setup(torch, eng, a.obs, a.free)
    for _ in range(3):
        eng.posterior(start, obs, names, weights=w, **prior)
        eng.refine(start, obs, names, weights=w, n_iter=2, **prior)
    torch.cuda.synchronize()


def kernel_lines(a):
    """--child under rocprofv3 --kernel-trace --stats in a fresh process group -> ({kernel: (calls, average ms, min, max)}, note)"""
    d = a.trace_dir or tempfile.mkdtemp(prefix="refine_posterior_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
           "--child", "--obs", str(a.obs), "--free", str(a.free)]
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
            for k in KERNELS:
                if k in row["Name"] and not (k == "k_columns" and "k_columns_srf" in row["Name"]):
                    n, avg = int(row["Calls"]), float(row["AverageNs"]) / 1e6
                    old = rows.get(k)                               # (both instantiations of a template: the busier one)
                    if old is None or n > old[0]:
                        rows[k] = (n, avg, float(row["MinNs"]) / 1e6, float(row["MaxNs"]) / 1e6)
    return rows, "" if "k_refine_posterior" in rows else "(no k_refine_posterior row in the kernel stats)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obs", type=int, default=262144)
    ap.add_argument("--free", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
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
    from spart_amd import _lib, get_engine
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = get_engine(SENSOR, 0)
    M, F, nb = a.obs, a.free, eng.nb
    rows, chunk = (F + 1) * M, (1 << 19) // (F + 1)
    say(f"spart_refine_posterior on MI355X (one GCD), tools/refine_posterior_rate.py: {SENSOR}, nb = {nb}, M = {M} observations, F = {F} "
        f"free parameters {NAMES[:F]}, per-observation weights, a shared prior ({rows} forward rows, in chunks of {chunk} "
        f"observations), float64; device events, medians of {a.reps} after 2 warm-up calls.")
    say()
    start, obs, names, w, prior = setup(torch, eng, M, F)
    res = {}

    def call_a():
        res.update(eng.posterior(start, obs, names, weights=w, **prior))
    slim = tuple(k for k in _lib.POSTERIOR_OUTS if k != "jac")

    def call_b():
        eng.posterior(start, obs, names, weights=w, _outputs=slim, **prior)
    Pf = torch.as_tensor(np.ascontiguousarray(np.tile(start.cpu().numpy(), (1, F + 1))), device=eng.device)
    out = {k: torch.empty((rows, nb), dtype=torch.float64, device=eng.device) for k in ("R_TOC", "R_TOA", "L_TOA")}

    def call_c():
        eng.run(Pf, "float64", out=out, prune=True)
    ta, tb, tc = (event_ms(torch, f, a.reps) for f in (call_a, call_b, call_c))
    ma, mb, mc = (float(np.median(t)) for t in (ta, tb, tc))
    say(f"  a  the whole call, all ten outputs              {stats(ta)}   = {ma * 1e6 / M:.1f} ns per observation")
    say(f"  b  the same call without jac                    {stats(tb)}   = {mb * 1e6 / M:.1f} ns per observation")
    say(f"  c  one forward call of (F + 1) M = {rows} rows   {stats(tc)}   = {mc * 1e6 / rows:.2f} ns per row")
    say(f"     a / c = {ma / mc:.3f}   b / c = {mb / mc:.3f}   a - b = {ma - mb:.3f} ms for {M * nb * F * 8 / 1e6:.1f} MB of jac "
        f"({M * nb * F * 8 / max(ma - mb, 1e-9) / 1e9:.2f} TB/s)" if ma > mb else f"     a / c = {ma / mc:.3f}   b / c = {mb / mc:.3f}")
    say(f"     a - c = {ma - mc:.3f} ms: init, k_refine_posterior, the corr of Engine.posterior and the chunking = {(ma - mc) / mc:.3f} of "
        "the forward time")
    st, dfs = res["status"].cpu().numpy(), res["dfs"].cpu().numpy()
    say(f"     the result: {int((st == 0).sum())} of {M} at status 0, {int((st == 1).sum())} at 1, {int((st == -1).sum())} dead; median dfs = "
        f"{np.median(dfs[st == 0]):.3f} of {F}")
    say()
    ok = True
    if a.no_trace:
        say("rocprofv3 --kernel-trace --stats: (not collected: --no-trace)")
    else:
        rows_, note = kernel_lines(a)
        ok = not note
        say(f"rocprofv3 --kernel-trace --stats (a separate run in a fresh process: 3 posterior calls, 3 spart_refine calls of n_iter = 2): {note}")
        per = min(M, chunk)
        for k, (n, avg, lo_, hi_) in sorted(rows_.items()):
            say(f"  {k:18s} {n:5d} calls, average {avg:.3f} ms (min {lo_:.3f}, max {hi_:.3f})")
        if "k_refine_posterior" in rows_ and "k_refine_step" in rows_:
            p, s = rows_["k_refine_posterior"][1], rows_["k_refine_step"][1]
            say(f"  per observation of a full chunk of {per}: k_refine_posterior {p * 1e6 / per:.1f} ns, k_refine_step {s * 1e6 / per:.1f} ns "
                f"(averages over full and last chunks): ratio {p / s:.2f}")
            bytes_ = ((F + 1) * nb + nb * F + 2 * F * F + 2 * F + nb) * 8
            say(f"  k_refine_posterior moves at least {bytes_} B per observation ({(F + 1) * nb * 8} read, {nb * F * 8} of jac): "
                f"{bytes_ * per / (p * 1e-3) / 1e12:.2f} TB/s")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
