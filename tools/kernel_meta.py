"""Register / scratch / LDS budget of every kernel in libspart_hip (hipcc -S of the device code; no GPU needed).

    python tools/kernel_meta.py [extra hipcc flags]"""
import os
import re
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers.kernel_meta import kernel_meta  # noqa: E402  (the resource tests read the same dict)


if __name__ == "__main__":
    names = kernel_meta(tuple(sys.argv[1:]))
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    for d, (k, v) in zip(dem, names.items()):
        d = re.sub(r"\(.*", "", d).replace("void spart::", "")
        print(f"{d:60s} vgpr {v['vgpr_count']:4d} sgpr {v['sgpr_count']:4d} scratch {v['private_segment_fixed_size']:5d} "
              f"lds {v['group_segment_fixed_size']:6d} spill v{v['vgpr_spill_count']} s{v['sgpr_spill_count']}")
