#!/usr/bin/env python3
"""Check that a refactor left the device code alone: compile every csrc/kernels/*.hip of the working
tree and of <git-ref> to gfx950 assembly with build.py's flags and compare the text.

Only lines containing `__hip_cuid_` (the per-compilation-unit id) are dropped before comparing; they
are the one thing that differs when nothing changed. Prints `identical` or the first differing
lines per file and exits non-zero on any difference.

With --by-symbol a file whose text differs is compared function by function instead (same set of
symbols, identical text and metadata per symbol): a host-side change can make the compiler emit the
same kernels in another order.

Usage: python tools/kernel_isa_diff.py [-j N] [--by-symbol] <git-ref> [file.hip ...]
"""
import argparse
import concurrent.futures as cf
import difflib
import io
import os
import re
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


_BLOCK = re.compile(r"(?<![A-Za-z0-9_])((?:\.L)?BB)\d+_(\d+)")  # also named in comments: `Header=BB12_3`
_LABEL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")


def _by_symbol(lines):
    """{symbol: lines} of one assembly file, for comparing two files that hold the same functions in
    a different order: a function's text from its `Begin function` line to the end of its `Kernel
    info` comment, then its entry of the metadata. Everything else is kept under "". Local labels carry
    the function's index in the file (`.LBB12_3`, `.Lfunc_end12`): the index is dropped, and counters
    that run through the whole file (`.Ltmp7`) are renumbered from 0 per function."""
    out = {"": []}
    cur, ended, meta, entry = "", False, False, []

    def file_entry():  # a list item of the metadata goes to the kernel its `.name` gives
        names = [x.split(":", 1)[1].strip() for x in entry if x.startswith("    .name:")]
        out.setdefault(names[0] if names else "", []).extend(entry)
        entry.clear()
    for ln in lines:
        if ln.startswith("\t.amdgpu_metadata"):
            cur, meta = "", True
        if meta:
            if ln.startswith("  - ") or not ln.startswith("  "):
                file_entry()
            entry.append(ln)
            continue
        if "; -- Begin function " in ln:
            head = [out[cur].pop()] if out[cur] and out[cur][-1].startswith("\t.section\t.text") else []
            cur, ended = ln.rsplit(" ", 1)[1].strip(), False
            out[cur] = head
        elif "; -- End function" in ln:
            ended = True
        elif ended and not (ln.startswith("\t.set " + cur + ".") or ln.startswith(";") or ".AMDGPU.csdata" in ln):
            cur, ended = "", False
        out[cur].append(ln)
    file_entry()
    for sym, body in out.items():
        seen = {}

        def norm(m):
            if m.group(3) or m.group(1).startswith("func_"):  # per-function index: .LBB12_3 -> .LBB_3
                return ".L" + m.group(1) + (m.group(3) or "")
            return ".L" + m.group(1) + str(seen.setdefault(m.group(0), len(seen)))
        # (the comment column moves with the label's width)
        out[sym] = [re.sub(r"[ \t]+;", " ;", _LABEL.sub(norm, _BLOCK.sub(r"\1_\2", ln))) for ln in body]
    return out


def _kernels(csrc):
    return {f for f in os.listdir(os.path.join(csrc, "kernels")) if f.endswith(".hip")}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("ref", help="commit to compare the working tree against")
    ap.add_argument("files", nargs="*", help="kernel file names (default: all)")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--context", type=int, default=20, help="diff lines shown per file")
    ap.add_argument("--by-symbol", action="store_true",
                    help="a file whose text differs: compare per function symbol (same set, same text and "
                         "metadata each), for a host change that only reorders the emitted functions")
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
                if a.by_symbol:
                    so, sn = _by_symbol(old), _by_symbol(new)
                    diff = sorted(s for s in set(so) | set(sn) if so.get(s) != sn.get(s))
                    if not diff:
                        print(f"{n}: identical per symbol ({len(sn) - 1} symbols, in another order)", flush=True)
                        continue
                    bad += 1
                    print(f"{n}: {len(diff)} of {len(set(so) | set(sn)) - 1} symbols DIFFER", flush=True)
                    for s in diff:
                        where = "differs" if s in so and s in sn else ("only in " + (a.ref if s in so else "working tree"))
                        print(f"  {s or '(outside any function)'}: {where}")
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
