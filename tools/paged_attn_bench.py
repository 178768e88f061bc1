"""Micro-benchmark of the paged-attention decode kernel (HIP graph of N back-to-back calls, so
launch overhead is excluded): time per call vs batch, context, splits and KV-cache size.
  python tools/paged_attn_bench.py
  python tools/paged_attn_bench.py --kv fp8                      the same sweep over an FP8 cache
  python tools/paged_attn_bench.py --kv bf16 fp8 --shapes 1:1024 32:16384 --rounds 7
      both caches on the same shapes, timed in alternating rounds: median and min..max per cache and
      the fp8 / bf16 ratio of the medians"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _graph(B, ctx, nq, nkv, D, bs, total_blocks, splits, reps, kv):
    """(graph of `reps` calls, splits, cache bytes, K/V bytes one call streams, the call itself). The
    graph holds only addresses: the caller keeps the call, whose closure owns the operands, for as
    long as it replays the graph."""
    from shuffle_exchange_amd.ops.paged_attention import choose_splits, quantize_kv_fp8
    from shuffle_exchange_amd.ops import native
    native.require_hip()
    nb = (ctx + bs - 1) // bs
    total_blocks = total_blocks or B * nb
    cache = torch.randn(total_blocks, 2, nkv, bs, D, device="cuda", dtype=torch.bfloat16)
    perm = torch.randperm(total_blocks, device="cuda")[:B * nb].to(torch.int32)
    bt = perm.view(B, nb).contiguous()
    q = torch.randn(B, nq, D, device="cuda", dtype=torch.bfloat16)
    qs = torch.arange(B, device="cuda", dtype=torch.int32)
    ql = torch.ones(B, device="cuda", dtype=torch.int32)
    kl = torch.full((B,), ctx, device="cuda", dtype=torch.int32)
    sp = splits or choose_splits(B, nkv, ctx)
    if kv == "fp8":
        codes, scales = quantize_kv_fp8(cache)
        del cache
        f = lambda: torch.ops.sxe.paged_attention_fp8(q, codes, scales, bt, qs, ql, kl,  # noqa: E731
                                                      D ** -0.5, ctx, sp)
        cache_bytes, row_bytes = codes.numel() + scales.numel() * 4, D + 4
    else:
        f = lambda: torch.ops.sxe.paged_attention(q, cache, bt, qs, ql, kl, D ** -0.5, ctx, sp)  # noqa: E731
        cache_bytes, row_bytes = cache.numel() * 2, 2 * D
    f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            f()
    g.replay()
    torch.cuda.synchronize()
    return g, sp, cache_bytes, B * ctx * nkv * 2 * row_bytes, f


def _time_us(g, reps, replays=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (replays * reps) * 1e3


def bench(B, ctx, nq=32, nkv=8, D=128, bs=64, total_blocks=None, splits=None, reps=20, kv="bf16"):
    g, sp, cache_bytes, kv_bytes, _operands = _graph(B, ctx, nq, nkv, D, bs, total_blocks, splits, reps, kv)
    us = _time_us(g, reps)
    return {"kv": kv, "B": B, "ctx": ctx, "splits": sp, "cache_GB": round(cache_bytes / 1e9, 2), "us": round(us, 2),
            "TB_per_s": round(kv_bytes / us / 1e6, 2)}


def compare(B, ctx, kvs, rounds, nq=32, nkv=8, D=128, bs=64, reps=20):
    """The caches of `kvs` on one shape, timed in alternating rounds (same process, same block table
    seed): per cache the median and min..max time per call, then the ratio of the medians."""
    graphs = {}
    for kv in kvs:
        torch.manual_seed(0)
        graphs[kv] = _graph(B, ctx, nq, nkv, D, bs, None, None, reps, kv)
    # replays per timing window: at least 50 ms of work, so the window is not the clock's resolution
    replays = {kv: max(5, int(5e4 / (_time_us(graphs[kv][0], reps) * reps)) + 1) for kv in kvs}
    times = {kv: [] for kv in kvs}
    for _ in range(rounds):
        for kv in kvs:
            times[kv].append(_time_us(graphs[kv][0], reps, replays[kv]))
    out = {"B": B, "ctx": ctx, "splits": graphs[kvs[0]][1], "rounds": rounds}
    for kv in kvs:
        t = sorted(times[kv])
        med = t[len(t) // 2]
        out[kv] = {"us_median": round(med, 2), "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                   "cache_GB": round(graphs[kv][2] / 1e9, 3), "TB_per_s": round(graphs[kv][3] / med / 1e6, 2)}
    if "bf16" in out and "fp8" in out:
        out["fp8_over_bf16_time"] = round(out["fp8"]["us_median"] / out["bf16"]["us_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description="Micro-benchmark of the paged-attention decode kernel")
    ap.add_argument("--kv", nargs="+", choices=("bf16", "fp8"), default=["bf16"], help="KV-cache type(s)")
    ap.add_argument("--shapes", nargs="+", default=None, help="BATCH:CONTEXT ... (Llama-3-8B attention heads)")
    ap.add_argument("--rounds", type=int, default=7, help="alternating timing rounds per shape (with --shapes)")
    a = ap.parse_args()
    if a.shapes:
        for s in a.shapes:
            B, ctx = (int(v) for v in s.split(":"))
            print(json.dumps(compare(B, ctx, a.kv, a.rounds)), flush=True)
        return
    for kv in a.kv:
        for B, ctx in ((1, 1024), (1, 8192), (8, 1024), (32, 1024), (64, 2048), (128, 4096)):
            print(json.dumps(bench(B, ctx, kv=kv)), flush=True)
        for sp in (1, 2, 4, 8, 16):
            print(json.dumps(bench(1, 4096, splits=sp, kv=kv)), flush=True)
        print(json.dumps(bench(1, 1024, total_blocks=131072, kv=kv)), flush=True)  # 34 GB bf16 cache, scattered blocks


if __name__ == "__main__":
    main()
