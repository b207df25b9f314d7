"""Device assembly of two source trees, kernel by kernel (no GPU needed).

    python tools/asm_ab.py DIR_A DIR_B

DIR_A / DIR_B hold what build.device_asm(dir) writes for each tree (one .s per translation unit).  Kernels are compared with
comments and directives stripped; for each one that differs: its static instruction count and the six resource figures of
tests/helpers/kernel_meta.py, A -> B (profiles/columns_refactor_ab.txt)."""
import os
import re
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers.kernel_meta import FIELDS, read_kernels  # noqa: E402


def kernel_code(asm):
    """{mangled kernel name: its instructions and labels}"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s+s_endpgm", asm, flags=re.M | re.S):
        # (a label carries its function's number in the unit, which moves when a kernel before it comes or goes)
        lines = (re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in m.group(2).split("\n"))
        out[m.group(1)] = [l for l in lines if l and (not l.startswith(".") or re.match(r"\.LBB_\d+:", l))]
    return out


def main(dir_a, dir_b):
    for f in sorted(os.listdir(dir_a)):
        a, b = open(os.path.join(dir_a, f)).read(), open(os.path.join(dir_b, f)).read()
        ca, cb, ma, mb = kernel_code(a), kernel_code(b), read_kernels(a), read_kernels(b)
        assert set(ca) == set(ma) and set(cb) == set(mb), f
        both = [n for n in ca if n in cb]
        diff = [n for n in both if ca[n] != cb[n]]
        print(f"{f}: {len(both)} kernels in both, {len(both) - len(diff)} identical, {len(diff)} differ")
        for tag, only in (("A", set(ca) - set(cb)), ("B", set(cb) - set(ca))):
            for d in subprocess.run(["c++filt"], input="\n".join(sorted(only)), capture_output=True, text=True).stdout.split("\n"):
                if d:
                    print(f"  only in {tag}: {re.sub(r'[(].*', '', d).replace('void spart::', '')}")
        names = subprocess.run(["c++filt"], input="\n".join(diff), capture_output=True, text=True).stdout.split("\n")
        for n, d in zip(diff, names):
            na, nb = (sum(1 for l in c[n] if not l.endswith(":")) for c in (ca, cb))
            print(f"  {re.sub(r'[(].*', '', d).replace('void spart::', '')}: instructions {na} -> {nb} ({100.0 * (nb - na) / na:+.2f} %)")
            print("      " + ", ".join(f"{k} {ma[n][k]} -> {mb[n][k]}" for k in FIELDS.split("|")))


if __name__ == "__main__":
    main(*sys.argv[1:3])
