"""One layer's ragged prefill attention, existing path vs variable-length flash (not a test):
  * loop   -- ``ragged_attention`` of inference/v2/model_implementations/hf_decoder.py (the same loop
              as RaggedLlama._attention): per fresh prompt a padded copy, one ``flash_attn_fwd`` launch
              and a copy back, then one paged launch over a gathered subset and more copies; with
              head dim != 128, prompts under 128 tokens or a narrow window, the paged kernel for all;
  * varlen -- ``dense_blocked_attention_varlen_prefill``: one ``flash_attn_fwd_varlen`` launch over the
              fresh prompts, one paged launch over the rest, no copies.
Both run on the same RaggedBatch, packed QKV and KV cache (K/V already appended; the append is the
same for both and is not timed). Each timing window is ``--iters`` back-to-back calls between two
device events, host work included (the loop path is bound by it); the two paths alternate for
``--rounds`` rounds after a warm-up and the table gives min..median..max per call and the ratio of
the medians. The two outputs are compared at every timed size.
  python tools/varlen_prefill_bench.py [--rounds 7] [--iters 20] [--short] > profiles/varlen_prefill_bench.log
``--short`` adds batches of 32 fresh prompts of 16..127 tokens with the routing threshold at 1: paged
kernel vs varlen below VARLEN_PREFILL_MIN (the crossover written next to that constant)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _setup(lens_seen, nq, nkv, D, window, varlen_min=None, bs=64, seed=0):
    from shuffle_exchange_amd.inference.v2.ragged.ragged import BlockedKVCache, DSStateManager, RaggedBatch
    from shuffle_exchange_amd.ops.paged_attention import kv_cache_append
    dev = torch.device("cuda")
    blocks = sum(-(-(n + s) // bs) for n, s in lens_seen) + 1
    kv = BlockedKVCache(1, blocks, bs, nkv, D, dtype=torch.bfloat16, device=dev)
    g = torch.Generator(device="cuda").manual_seed(seed)
    kv.cache.copy_(torch.randn(kv.cache.shape, device=dev, generator=g))
    sm = DSStateManager(kv)
    seqs, toks = [], []
    for uid, (n, seen) in enumerate(lens_seen):
        s = sm.get_or_create_sequence(uid)
        sm.allocate_blocks(s, seen + n)
        s.seen_tokens = seen
        s.pre_forward(n)
        seqs.append(s)
        toks.append(torch.zeros(n, dtype=torch.long))
    batch = RaggedBatch(seqs, toks, bs, dev, varlen_min=varlen_min)
    qkv = torch.randn(batch.num_tokens, nq + 2 * nkv, D, device=dev, generator=g).to(torch.bfloat16)
    kv_cache_append(qkv, kv.layer(0), batch.slots, nq, nkv)
    return batch, kv.layer(0), qkv


def _time_ms(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench(name, lens_seen, nq=32, nkv=8, D=128, window=None, varlen_min=None, rounds=7, iters=20):
    from shuffle_exchange_amd.inference.v2.model_implementations.hf_decoder import ragged_attention
    from shuffle_exchange_amd.inference.v2.modules.implementations import AttentionConfig, PagedAttentionVarlenPrefill
    batch, layer, qkv = _setup(lens_seen, nq, nkv, D, window, varlen_min)
    impl = PagedAttentionVarlenPrefill(AttentionConfig(D, nq, nkv, torch.bfloat16, window or 0, "cuda"))
    scale = D ** -0.5
    paths = {"loop": lambda: ragged_attention(qkv, layer, batch, nq, nkv, D, scale, window),
             "varlen": lambda: impl(qkv, layer, batch, nq, nkv, scale, window=window)}
    outs = {k: f() for k, f in paths.items()}
    torch.cuda.synchronize()
    a, b = outs["loop"].float(), outs["varlen"].float()
    rel = float((a - b).norm() / b.norm())
    for f in paths.values():  # warm-up
        _time_ms(f, max(2, iters // 4))
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, f in paths.items():
            times[k].append(_time_ms(f, iters))
    out = {"batch": name, "heads": f"{nq}/{nkv}", "D": D, "window": window, "tokens": batch.num_tokens,
           "routed_seqs": len(batch.varlen_ids), "table_rows": int(batch.varlen_table.shape[0]),
           "rel_diff_of_outputs": round(rel, 5), "finite": bool(torch.isfinite(a).all() and torch.isfinite(b).all())}
    for k in paths:
        t = sorted(times[k])
        out[k + "_ms"] = {"min": round(t[0], 4), "median": round(t[len(t) // 2], 4), "max": round(t[-1], 4)}
    out["varlen_over_loop"] = round(out["varlen_ms"]["median"] / out["loop_ms"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--short", action="store_true", help="add the sub-128-token crossover rows")
    a = ap.parse_args()
    from shuffle_exchange_amd.ops import native
    native.require_hip()
    ragged = [(129 + (i * 37) % 172, 0) for i in range(64)]  # 64 sequences of 129..300 tokens
    mixed = [(512, 0)] * 8 + [(1, 1024)] * 24
    rows = [("1 x 2048", [(2048, 0)], {}), ("8 x 512", [(512, 0)] * 8, {}), ("32 x 256", [(256, 0)] * 32, {}),
            ("64 x 129..300", ragged, {}), ("32 x 512, window 256", [(512, 0)] * 32, {"window": 256}),
            ("8 x 512 + 24 decode @1024", mixed, {}),
            ("8 x 512", [(512, 0)] * 8, {"nq": 32, "nkv": 8, "D": 64}),
            ("8 x 512", [(512, 0)] * 8, {"nq": 16, "nkv": 4, "D": 256})]
    if a.short:
        rows += [(f"32 x {n} (threshold 1)", [(n, 0)] * 32, {"varlen_min": 1}) for n in (16, 32, 64, 96, 127)]
    for name, lens_seen, kw in rows:
        print(json.dumps(bench(name, lens_seen, rounds=a.rounds, iters=a.iters, **kw)), flush=True)


if __name__ == "__main__":
    main()
