#!/usr/bin/env python3
"""Check that a refactor left the device code alone: compile every csrc/kernels/*.hip of the working
tree and of <git-ref> to gfx950 assembly with build.py's flags and compare the text.

Only lines containing `__hip_cuid_` (the per-compilation-unit id) are dropped before comparing; they
are the one thing that differs when nothing changed. Prints `identical` or the first differing
lines per file and exits non-zero on any difference.

Usage: python tools/kernel_isa_diff.py <git-ref> [-j N] [file.hip ...]
"""
import argparse
import concurrent.futures as cf
import difflib
import io
import os
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "csrc"))
import build as sxe_build  # noqa: E402


def _asm(csrc, name, out):
    cmd = ["hipcc"] + sxe_build.hip_flags(csrc) + ["--cuda-device-only", "-S",
                                                   os.path.join(csrc, "kernels", name), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("command failed:\n  " + " ".join(cmd) + "\n" + r.stdout)
    with open(out) as f:
        return [ln for ln in f if "__hip_cuid_" not in ln]


def _kernels(csrc):
    return {f for f in os.listdir(os.path.join(csrc, "kernels")) if f.endswith(".hip")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("ref", help="commit to compare the working tree against")
    ap.add_argument("files", nargs="*", help="kernel file names (default: all)")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--context", type=int, default=20, help="diff lines shown per file")
    a = ap.parse_args()

    with tempfile.TemporaryDirectory(prefix="sxe-isa-") as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.ref, "csrc"], stdout=subprocess.PIPE, check=True)
        with tarfile.open(fileobj=io.BytesIO(tar.stdout)) as t:
            t.extractall(os.path.join(tmp, "ref"))
        trees = {"ref": os.path.join(tmp, "ref", "csrc"), "new": os.path.join(ROOT, "csrc")}
        names = {k: _kernels(c) for k, c in trees.items()}
        wanted = sorted(set(a.files) or names["ref"] | names["new"])
        # longest compile first, so that it does not end up alone at the tail
        wanted.sort(key=lambda n: -max((os.path.getsize(os.path.join(c, "kernels", n))
                                        for k, c in trees.items() if n in names[k]), default=0))
        with cf.ThreadPoolExecutor(max(1, min(a.jobs, 8))) as ex:
            futs = {(n, k): ex.submit(_asm, c, n, os.path.join(tmp, f"{k}_{n}.s"))
                    for n in wanted for k, c in trees.items() if n in names[k]}
            bad = 0
            for n in sorted(wanted):
                if (n, "ref") not in futs or (n, "new") not in futs:
                    print(f"{n}: only in {'working tree' if (n, 'new') in futs else a.ref}")
                    bad += 1
                    continue
                old, new = futs[n, "ref"].result(), futs[n, "new"].result()
                if old == new:
                    print(f"{n}: identical ({len(new)} lines)", flush=True)
                    continue
                bad += 1
                print(f"{n}: DIFFERS", flush=True)
                d = difflib.unified_diff(old, new, a.ref + "/" + n, n, n=2)
                for i, ln in enumerate(d):
                    if i >= a.context:
                        print("  ...")
                        break
                    print("  " + ln.rstrip("\n"))
    print(f"{len(wanted) - bad} of {len(wanted)} identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
