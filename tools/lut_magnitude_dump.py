"""A/B of two builds of the library on the magnitude cases of tests/helpers/lut_hostile.py (GPU).

    SPART_HIP_LIB=<one build> python tools/lut_magnitude_dump.py a.npz        (no SPART_HIP_LIB: the in-tree library)
    SPART_HIP_LIB=<another>   python tools/lut_magnitude_dump.py b.npz
    python tools/lut_magnitude_dump.py --compare a.npz b.npz [--skip huge_entry,norm_rule]

The first form runs every case through every search that takes it (k = 1 and 10), writes idx, cost and the statistics words
(brute-forced observations, candidate tiles, their maximum, Nmax / Nbound) of each call into the npz, and prints per call
whether idx and cost equal the numpy brute force.  --compare counts the arrays that are bit-identical in the two files;
--skip leaves out the cases whose name contains one of the given words (those a change is MEANT to move)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "spart-python_amd")]
import numpy as np  # noqa: E402


def compare(a, b, skip):
    a, b = np.load(a), np.load(b)
    assert sorted(a.files) == sorted(b.files), "the two files hold different calls"
    keys = [k for k in a.files if not any(s in k for s in skip)]
    diff = [k for k in keys if not np.array_equal(a[k], b[k], equal_nan=True)]
    print(f"{len(keys)} arrays compared, {len(keys) - len(diff)} bit-identical")
    for k in diff:
        print("differs:", k)
    return 1 if diff else 0


def dump(out):
    import torch
    import lut_brute_force as bf
    from helpers import lut_hostile as H
    import test_gpu_lut_magnitudes as T
    from spart_amd import _lib, get_engine
    eng = get_engine(None, 0)
    print("library", os.environ.get("SPART_HIP_LIB", "in-tree"), _lib.build_id(eng.lib), flush=True)
    res = {}
    for dtype in ("float32", "float64"):
        for nb, seed in T.WIDTHS:
            for case in H.hostile_cases(bf, dtype, nb, seed):
                wi, wc = H.oracle(bf, case, 10)
                for entry in T.searches_for(case, nb):
                    for k in (1, 10):
                        if entry == "spart_lut_nearest" and k != 1:
                            continue
                        idx, cost, st = T.run(torch, eng, entry, case, k, dtype)
                        key = f"{dtype}|{nb}|{case.name}|{entry}|{k}"
                        res[key + "|idx"], res[key + "|cost"] = idx, cost
                        res[key + "|st"] = np.array([st[n] for n in sorted(st)], dtype=np.float64)
                        bad = (idx != wi[:, :k]).any(axis=1) | (cost != wc[:, :k]).any(axis=1)
                        print("OK   " if not bad.any() else "WRONG", key, f"wrong {int(bad.sum())} / {len(bad)}, unmatched "
                              f"{int((idx[:, 0] == -1).sum())} (brute force: {int((wi[:, 0] == -1).sum())})", st, flush=True)
    np.savez_compressed(out, **res)


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        skip = sys.argv[sys.argv.index("--skip") + 1].split(",") if "--skip" in sys.argv else []
        sys.exit(compare(sys.argv[2], sys.argv[3], skip))
    dump(sys.argv[1])
