"""Rate of spart_lut_bayes (Engine.lut_bayes) on the README LUT shape, next to the k-NN chain it extends on the same inputs:
spart_lut_topk_obs_weights(k = 256) + spart_lut_summarise, which is the same filter machinery with the top-k threshold.

    python tools/lut_bayes_rate.py [--rows 1000000] [--obs 65536] [--reps 5] [--rel-sigma 0.02] [--cut 50]
                                   [--out profiles/lut_bayes_rate.txt]
    python tools/lut_bayes_rate.py --reps 3 --quantiles 0.05,0.5,0.95 --out profiles/lut_bayes_quantiles_rate.txt
                                   (spart_lut_bayes_quantiles too, in the same run, and the passes of its search)

Workload: a Sentinel-2A LUT (nb = 13, float32) of LHS parameters generated into a temporary directory, all 27 parameter
columns; observations = LUT rows x (1 + rel_sigma N(0, 1)); weights = noise_weights(obs, rel_sigma=rel_sigma), one row per
observation.  Device events around the calls, medians of --reps after one warm-up.  Per call: the time, and from the stats
the brute-forced observations and the candidate tiles per observation; for the posterior also the mean and the largest count
and the median effective sample size.  One text report; every figure in it is measured in this run.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lut_summarise_rate import event_ms, stats  # noqa: E402


def quantile_report(say, torch, eng, lut_t, par_t, obs_t, w_t, a, plain, bayes_ms):
    """--quantiles: spart_lut_bayes_quantiles on the same inputs in the same run, and the passes over S of its search.  The
    kernel keeps no counter (it writes nothing but the quantiles), so the passes are those of its search written out in numpy
    (lut_bayes_defined.quantile_search) on a sample of observations whose members are recomputed with torch; the observation
    with the largest set is part of the sample."""
    from lut_bayes_defined import quantile_search
    levels = [float(q) for q in a.quantiles.split(",")]
    M = obs_t.shape[0]
    say()
    ts, res = event_ms(torch, lambda: eng.lut_bayes(lut_t, par_t, obs_t, weights=w_t, cut=a.cut, quantiles=levels), a.reps)
    q_ms = float(np.median(ts))
    say(f"spart_lut_bayes_quantiles(levels = {levels})   {stats(ts)}")
    same = all(torch.equal(torch.nan_to_num(res[n].double(), nan=-1.0), torch.nan_to_num(plain[n].double(), nan=-1.0)) for n in plain)
    say(f"    the seven base outputs equal spart_lut_bayes' bit for bit: {same};  NaN quantiles: {int(torch.isnan(res['quantiles']).sum())}")
    say(f"    added to spart_lut_bayes ({bayes_ms:.3f} ms): {q_ms - bayes_ms:.3f} ms = {100.0 * (q_ms - bayes_ms) / bayes_ms:.1f} %")
    count = plain["count"].cpu().numpy()
    rng = np.random.default_rng(4)
    sample = np.unique(np.concatenate([rng.choice(M, min(a.pass_sample, M), replace=False), [int(count.argmax())]]))
    passes, matched, equal = [], 0, 0
    quant = res["quantiles"][torch.as_tensor(sample, device=lut_t.device)].cpu().numpy()
    for j, m in enumerate(sample):
        c = ((lut_t - obs_t[m]) ** 2 * w_t[m]).sum(dim=1).double()
        e = c - c.min()
        rows = torch.nonzero(e <= a.cut)[:, 0]
        matched += int(rows.numel() == count[m])
        got, n = quantile_search(par_t[rows].cpu().numpy(), np.exp(-(e[rows].cpu().numpy() / 2.0)), levels)
        passes.append(n)
        equal += int(np.array_equal(got, quant[j], equal_nan=True))
    passes = np.array(passes)
    say(f"    passes over S of the search (beside pass A and the pass for sum_w and the ranges), {sample.size} observations: mean "
        f"{passes.mean():.2f}, max {passes.max()} (set of {count[sample[passes.argmax()]]} rows; the largest set, {count.max()} rows, "
        f"takes {passes[list(sample).index(int(count.argmax()))]})")
    say(f"    members recomputed with torch: the device's count for {matched} of {sample.size}, the device's quantiles for {equal}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quantiles", default=None, help="levels, e.g. 0.05,0.5,0.95: time spart_lut_bayes_quantiles too")
    ap.add_argument("--pass-sample", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--obs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rel-sigma", type=float, default=0.02)
    ap.add_argument("--cut", type=float, default=50.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import spart_amd
    from spart_amd import get_engine, workloads
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    eng = get_engine(None, 0)
    d = os.path.join(tempfile.mkdtemp(prefix="spart_bayesrate_"), "lut")
    spart_amd.generate_lut(workloads.lhs_params(a.rows, "full", seed=21), "Sentinel2A-MSI", path=d, dtype="float32")
    _, params, cols = spart_amd.load_lut(d)
    table = cols["R_TOC"]
    B, nb = table.shape
    P = params.shape[1]
    rng = np.random.default_rng(3)
    M = a.obs
    obs = (np.asarray(table)[rng.integers(0, B, M)] * (1 + a.rel_sigma * rng.standard_normal((M, nb)))).astype(np.float32)
    lut_t = torch.as_tensor(np.array(table)).to(eng.device)
    par_t = torch.as_tensor(np.ascontiguousarray(np.asarray(params), dtype=np.float64)).to(eng.device)
    obs_t = torch.as_tensor(obs, device=eng.device)
    w_t = torch.as_tensor(spart_amd.noise_weights(obs, rel_sigma=a.rel_sigma).astype(np.float32), device=eng.device)
    say(f"spart_lut_bayes on MI355X (one GCD), tools/lut_bayes_rate.py: B = {B} rows, nb = {nb}, float32, P = {P} parameters, "
        f"M = {M} observations = LUT rows x (1 + {a.rel_sigma} N(0,1)), weights = noise_weights(rel_sigma={a.rel_sigma}); "
        f"device events, medians of {a.reps} after one warm-up.")
    say()
    _, st = eng.lut_bayes(lut_t, par_t, obs_t, weights=w_t, cut=a.cut, stats=True)
    ts, res = event_ms(torch, lambda: eng.lut_bayes(lut_t, par_t, obs_t, weights=w_t, cut=a.cut), a.reps)
    count = res["count"].cpu().numpy()
    ess = res["ess"].cpu().numpy()
    say(f"spart_lut_bayes(cut = {a.cut:g}, temperature = 1)            {stats(ts)}")
    say(f"    brute-forced observations {st['brute_force']}, candidate tiles per observation: mean {st['candidate_tiles'] / M:.2f}, "
        f"max {st['max_candidate_tiles']} (32 rows each, capacity 1088)")
    say(f"    count: mean {count.mean():.1f}, median {np.median(count):.0f}, max {count.max()};  ess: median "
        f"{np.nanmedian(ess):.2f}, share of observations with ess < 2: {np.mean(ess < 2):.3f}")
    bayes_ms = float(np.median(ts))
    _, _, sk = eng.lut_topk(lut_t, obs_t, 256, weights=w_t, stats=True)
    tk, (idx_t, _) = event_ms(torch, lambda: eng.lut_topk(lut_t, obs_t, 256, weights=w_t), a.reps)
    tsum, _ = event_ms(torch, lambda: eng.lut_summarise(par_t, idx_t), a.reps)
    say(f"spart_lut_topk_obs_weights(k = 256)                      {stats(tk)}")
    say(f"    brute-forced observations {sk['brute_force']}, candidate tiles per observation: mean {sk['candidate_tiles'] / M:.2f}, "
        f"max {sk['max_candidate_tiles']}")
    say(f"spart_lut_summarise of its (M, 256) indices              {stats(tsum)}")
    chain = float(np.median(tk) + np.median(tsum))
    say(f"k-NN chain (search + summary) {chain:.3f} ms;  spart_lut_bayes / chain = {bayes_ms / chain:.3f}")
    if a.quantiles:
        quantile_report(say, torch, eng, lut_t, par_t, obs_t, w_t, a, res, bayes_ms)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
