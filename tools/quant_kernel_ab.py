#!/usr/bin/env python3
"""A/B of the quantize kernels between two builds of the HIP library (SXE_HIP_LIB selects the one a
process loads; one library per process). The [parity] and [quant-bench] sections of
profiles/quant_kernel_edges.log come from here.

  dump OUT.pt     outputs for seeded finite inputs: groups 128 / 256 / 512 / 2048 x fp32 / bf16 / fp16,
                  37 groups each scaled 1e-4 .. 1e3. Per (group, dtype): quantize_sym q and scales for
                  int8 and int4, dequantize_sym_ to the three dtypes, dequant_reduce_ (W = 3, alpha
                  0.125, accumulate), quantize_fp8 q and scales, dequantize_fp8_ to the three dtypes,
                  fpx_quantize q and scales for FP4 and FP6 (21 tensors; 252 in all), plus q and scales
                  of quantize_sym int8 / int4 and quantize_fp8 on 4 Mi bf16 values at group 128 (6)
  compare A B     bit-compare two dumps
  bench TAG [GROUPS [OPS]]
                  quantize_sym int8 / int4 and quantize_fp8 on 64 MiB of bf16 at groups 128 and 64 (or
                  the comma-separated GROUPS, and the OPS among int8,int4,fp8): median / min / max of 9
                  windows of 20 calls, device events. Builds from before the in-group pairing must not
                  run int4 / fp8 at group 64: they step outside the tensors there.
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DTS = (torch.float32, torch.bfloat16, torch.float16)


def dump(path):
    from shuffle_exchange_amd.ops import native
    ops = native.require_hip()
    out = {}
    g = torch.Generator().manual_seed(1234)
    for group in (128, 256, 512, 2048):
        for dt in DTS:
            ng = 37
            x = (torch.randn(ng, group, generator=g) * torch.logspace(-4, 3, ng)[:, None]).reshape(-1).to(dt).cuda()
            tag = f"g{group}-{dt}"
            for bits in (8, 4):
                q, s = ops.quantize_sym(x, group, bits)
                out[f"sym{bits}.q {tag}"], out[f"sym{bits}.s {tag}"] = q.cpu(), s.cpu()
                for od in DTS:
                    o = torch.empty(x.numel(), dtype=od, device="cuda")
                    ops.dequantize_sym_(q, s, group, bits, o)
                    out[f"sym{bits}.deq{od} {tag}"] = o.cpu()
                o = torch.ones(x.numel(), device="cuda")
                ops.dequant_reduce_(q.repeat(3), s.repeat(3), 3, group, bits, o, 0.125, True)
                out[f"sym{bits}.reduce {tag}"] = o.cpu()
            q, s = ops.quantize_fp8(x, group)
            out[f"fp8.q {tag}"], out[f"fp8.s {tag}"] = q.cpu(), s.cpu()
            for od in DTS:
                o = torch.empty(x.numel(), dtype=od, device="cuda")
                ops.dequantize_fp8_(q, s, group, o)
                out[f"fp8.deq{od} {tag}"] = o.cpu()
            for bits in (4, 6):
                q, s = ops.fpx_quantize(x, bits, group)
                out[f"fp{bits}.q {tag}"], out[f"fp{bits}.s {tag}"] = q.cpu(), s.cpu()
    x = torch.randn(1 << 22, generator=g).bfloat16().cuda()
    for bits in (8, 4):
        q, s = ops.quantize_sym(x, 128, bits)
        out[f"big sym{bits}.q"], out[f"big sym{bits}.s"] = q.cpu(), s.cpu()
    q, s = ops.quantize_fp8(x, 128)
    out["big fp8.q"], out["big fp8.s"] = q.cpu(), s.cpu()
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f"dumped {len(out)} tensors")


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    assert a.keys() == b.keys()
    bad = [k for k in a if not (a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)))]
    print(f"[parity] tensors compared: {len(a)}, bit-equal: {len(a) - len(bad)}, different: {len(bad)}")
    for k in bad[:20]:
        print("[parity] DIFFERENT", k)
    return 1 if bad else 0


def bench(tag, groups=(128, 64), kinds=("int8", "int4", "fp8")):
    from shuffle_exchange_amd.ops import native
    ops = native.require_hip()
    x = torch.randn(64 * 1024 * 1024 // 2, device="cuda").bfloat16()
    for group in groups:
        cases = {"int8": ("quantize_sym int8", lambda: ops.quantize_sym(x, group, 8)),
                 "int4": ("quantize_sym int4", lambda: ops.quantize_sym(x, group, 4)),
                 "fp8": ("quantize_fp8", lambda: ops.quantize_fp8(x, group))}
        for name, fn in (cases[k] for k in kinds):
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(9):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(20):
                    fn()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) / 20 * 1e3)
            print(f"[quant-bench] {tag} {name} 64MiB bf16 g={group}: median {statistics.median(ts):.1f} us "
                  f"min {min(ts):.1f} max {max(ts):.1f}", flush=True)


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "dump":
        dump(sys.argv[2])
    elif cmd == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        groups = tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (128, 64)
        kinds = tuple(sys.argv[4].split(",")) if len(sys.argv) > 4 else ("int8", "int4", "fp8")
        bench(sys.argv[2], groups, kinds)
