#!/usr/bin/env python3
"""Time grouped fake quantization on the GPU: the fused HIP op (csrc/kernels/fake_quant.hip, through
ops.fake_quant) against the PyTorch pass sequence it replaces (runtime.quantize.fake_quantize on
the same GPU tensor, what the compression layers ran before the kernel existed).

Method: HIP events around ``--inner`` back-to-back calls (100 by default, so a window is several
milliseconds of GPU work and the launches queue up behind it rather than being what is timed),
``--warmup`` untimed rounds, then ``--repeats`` timed rounds in which the two implementations
alternate (so drift on a shared box hits both); the median per call is reported with the min / max
spread. Consecutive calls rotate through enough distinct input tensors to exceed ``--cold-mib``
(default 1024, four times the 256 MiB Infinity Cache), so every call reads its input from HBM,
not from the cache a previous call left warm; ``--cold-mib 0`` reuses one tensor. Achieved GB/s is the
traffic model over the median: 6 B/element for a 16-bit tensor whose groups need the two-pass path
(read, read, write) and 4 B/element when a group fits one workgroup or the range is static (read,
write); twice that for fp32. The copy yardstick is csrc/kernels/accum.hip's kernel
(``acc2_bf16_``, 8 B/element: two bf16 reads and an fp32 write) at the same element count.

Standalone: not part of bench.py. Needs a GPU; fails without one.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SMALL_MAX = 16384  # csrc/kernels/fake_quant.hip kSmallMax
DEFAULT_CASES = ["4096x14336:1", "4096x14336:4096", "2048x4096:1:static"]


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner  # ms per call


def bench(fns, warmup, repeats, inner):
    for _ in range(warmup):
        for f in fns.values():
            timed(f, inner)
    samples = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            samples[k].append(timed(f, inner))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES, help="ROWSxCOLS:GROUPS[:static]")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"])
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--modes", nargs="*", default=["symmetric"],
                    help="symmetric asymmetric binary ternary (the PyTorch baseline is timed for the first two)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--cold-mib", type=int, default=1024, help="rotate inputs over at least this many MiB")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fake_quant_bench: needs a GPU")
    from shuffle_exchange_amd.ops import native
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    from shuffle_exchange_amd.runtime.quantize import fake_quantize
    native.require_hip()
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    esize = torch.empty(0, dtype=dtype).element_size()
    print(f"# device {torch.cuda.get_device_name(0)}; dtype {a.dtype}; bits {a.bits}; warmup {a.warmup}, "
          f"repeats {a.repeats} x inner {a.inner}; inputs rotate over >= {a.cold_mib} MiB; "
          f"median ms per call [min .. max]")
    results = []
    for case in a.cases:
        parts = case.split(":")
        rows, cols = (int(v) for v in parts[0].split("x"))
        groups = int(parts[1])
        static = len(parts) > 2 and parts[2] == "static"
        torch.manual_seed(0)
        n = rows * cols
        copies = max(1, -(-a.cold_mib * 2 ** 20 // (n * esize)))
        xs = [torch.randn(rows, cols, device="cuda").to(dtype) for _ in range(copies)]
        turn = [0]

        def nxt(pool):
            turn[0] += 1
            return pool[turn[0] % len(pool)]
        rng = torch.tensor([-3.0, 3.0], device="cuda") if static else None
        one_pass = static or n // groups <= SMALL_MAX
        model_bytes = n * esize * (2 if one_pass else 3)
        ncopy = max(1, -(-a.cold_mib * 2 ** 20 // (n * 8)))
        trios = [(torch.empty(n, device="cuda"), torch.randn(n, device="cuda").bfloat16(),
                  torch.randn(n, device="cuda").bfloat16()) for _ in range(ncopy)]
        copy = bench({"copy": lambda: torch.ops.sxe.acc2_bf16_(*nxt(trios), False)}, a.warmup, a.repeats, a.inner)
        copy_gbs = n * 8 / copy["copy"][0] / 1e6
        del trios
        print(f"\n## {rows}x{cols} {a.dtype}, groups {groups}{', static range' if static else ''}: "
              f"{n / 1e6:.1f} M elements x {copies} rotating inputs, traffic model {model_bytes / n:.0f} B/element; "
              f"accum.hip copy kernel {copy['copy'][0]:.4f} ms = {copy_gbs:.0f} GB/s")
        for mode in a.modes:
            if static and mode not in ("symmetric", "asymmetric"):
                continue  # a static range only exists for the two grid modes
            fns = {"hip": lambda: fake_quant(nxt(xs), a.bits, groups, mode, rng)}
            if mode in ("symmetric", "asymmetric"):
                # the parent's path ignored a static range: it always ran the dynamic pass sequence
                fns["pytorch"] = lambda: fake_quantize(nxt(xs), a.bits, groups, mode == "symmetric")
            r = bench(fns, a.warmup, a.repeats, a.inner)
            rec = {"case": case, "dtype": a.dtype, "mode": mode, "bits": a.bits, "elements": n,
                   "model_bytes_per_element": model_bytes / n, "copy_gbs": round(copy_gbs, 1)}
            for k, (med, lo, hi) in r.items():
                gbs = model_bytes / med / 1e6
                rec[k + "_ms"] = round(med, 5)
                rec[k + "_model_gbs"] = round(gbs, 1)
                print(f"{mode:>10} {k:>8}: {med:8.4f} ms [{lo:.4f} .. {hi:.4f}]  {gbs:7.0f} GB/s of the traffic model"
                      f" ({100 * gbs / copy_gbs:.0f} % of the copy kernel's rate)")
            if "pytorch" in r:
                rec["speedup"] = round(r["pytorch"][0] / r["hip"][0], 2)
                print(f"{mode:>10}  speedup: {rec['speedup']:.2f}x")
            results.append(rec)
    print("\n" + json.dumps({"fake_quant_bench": results}))


if __name__ == "__main__":
    main()
