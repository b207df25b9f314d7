"""The workspace sizes of the refinement family, the tiles, the series, Sobol', the sampler and spart_vjp over a fixed grid of shapes:
one line per case, `entry  arguments  bytes`.  Two libraries lay their workspaces out alike in total when their outputs are
equal line for line.

    SPART_HIP_LIB=<a build> python tools/workspace_sizes.py [--out FILE]        (no SPART_HIP_LIB: the in-tree library)

Sensors: Sentinel-2A (13 bands) and the 211-band sensor of tests/golden/hyperspectral.npz.  0 bytes = the library refuses the
shape (more than 16 unknowns per pixel, for instance).  The size functions only need a context: nothing is launched.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "spart-python_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

MS = (1, 4097, 100000, 600000)
FS = (1, 5, 16)


def cases():
    """(entry, argument names, argument values) without the context"""
    for M in MS:
        for F in FS:
            yield "spart_refine_workspace_bytes", ("M", "F"), (M, F)
    for M in MS:
        for F in FS:
            for V, Fs in ((1, F), (3, 1)):
                yield "spart_views_workspace_bytes", ("M", "V", "F", "n_shared"), (M, V, F, Fs)
                yield "spart_mix_workspace_bytes", ("M", "V", "F", "n"), (M, V, F, Fs + V * (F - Fs))
    for entry in ("spart_tiles_workspace_bytes", "spart_series_workspace_bytes"):
        for M in MS:
            for F, Fs in ((5, 2), (16, 0), (4, 3)):
                yield entry, ("M", "F", "n_shared"), (M, F, Fs)
    for M, N, F in ((1, 128, 1), (64, 1024, 8), (1, 65536, 8), (3, 4096, 16)):
        yield "spart_sobol_workspace_bytes", ("M", "N", "F"), (M, N, F)
    for M, F, W in ((1, 1, 8), (16384, 4, 16), (70000, 16, 64)):
        yield "spart_sample_workspace_bytes", ("M", "F", "W"), (M, F, W)
    for M in MS:
        for F in FS:
            yield "spart_vjp_workspace_bytes", ("M", "F"), (M, F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from make_hyperspectral import sensorinfo_from_npz
    from spart_amd import Engine
    si211 = sensorinfo_from_npz(dict(np.load(os.path.join(ROOT, "tests", "golden", "hyperspectral.npz"))))
    lines = []
    for label, eng in (("Sentinel2A-MSI", Engine("Sentinel2A-MSI", 0)), ("hyperspectral-211", Engine(None, 0, sensor_info=si211))):
        lines.append(f"# {label}, nb = {eng.lib.spart_ctx_nb(eng.ctx)}")
        for entry, names, values in cases():
            args = ", ".join(f"{n} = {v}" for n, v in zip(names, values))
            lines.append(f"{entry:<30}  {args:<40}  {int(getattr(eng.lib, entry)(eng.ctx, *values))}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
