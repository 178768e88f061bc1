"""FP8 paged KV cache on the MI355X: the quantising append kernels against the PyTorch definition,
the FP8 paged-attention kernel against the fp32 reference over the dequantised cache (kernel error)
and over the unquantised bf16 cache (end to end), and the ragged engine served from an FP8 cache.

The history of every kv head is multiplied by its own factor spread over 1e-2 .. 1e2 and one cached
row is all zeros, so a dropped or mis-indexed scale is a gross error; the kernel error is taken per
query head, so that a small-magnitude head cannot hide behind a large one."""
import functools

import pytest
import torch

from .test_kv_cache_fp8 import ENGINE_COS_MIN, engine_min_cos, kv_fp8_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _native():
    from shuffle_exchange_amd.ops import native
    native.require_hip()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _rel_heads(a, b):
    """Largest per-head relative error of [T, heads, D] outputs."""
    d = (a.float() - b.float()).transpose(0, 1).flatten(1).norm(dim=1)
    return (d / b.float().transpose(0, 1).flatten(1).norm(dim=1)).max().item()


@functools.lru_cache(maxsize=None)
def _case(seqs, nq, nkv, D, bs, window=None, seed=0):
    """seqs: ((cached_tokens_before, new_tokens), ...). Random history scaled per kv head, one zero
    row; the new tokens are appended by the HIP kernels to a bf16 cache and to an FP8 layer. Returns
    the inputs and the two fp32 references (computed once per case, never modified)."""
    from shuffle_exchange_amd.ops.paged_attention import (FP8KVLayer, dequantize_kv_fp8, kv_cache_append,
                                                          paged_attention_reference, quantize_kv_fp8)
    g = torch.Generator(device="cuda").manual_seed(seed)
    head_scale = torch.logspace(-2, 2, nkv, device="cuda") if nkv > 1 else torch.full((1,), 30.0, device="cuda")
    total_blocks = sum((c + n + bs - 1) // bs for c, n in seqs) + 3
    cache = torch.randn(total_blocks, 2, nkv, bs, D, device="cuda", generator=g) * head_scale.view(1, 1, nkv, 1, 1)
    perm = torch.randperm(total_blocks, device="cpu", generator=torch.Generator().manual_seed(seed)).tolist()
    maxb = max((c + n + bs - 1) // bs for c, n in seqs)
    bt = torch.zeros(len(seqs), maxb, dtype=torch.int32)
    q_start, q_len, kv_len, slots = [], [], [], []
    t = 0
    for i, (c, n) in enumerate(seqs):
        nb = (c + n + bs - 1) // bs
        blocks = [perm.pop() for _ in range(nb)]
        bt[i, :nb] = torch.tensor(blocks, dtype=torch.int32)
        q_start.append(t)
        q_len.append(n)
        kv_len.append(c + n)
        slots += [blocks[p // bs] * bs + p % bs for p in range(c, c + n)]
        if c > 0:  # an all-zero cached row (k and v of kv head 0) in the middle of the history
            cache[blocks[(c // 2) // bs], :, 0, (c // 2) % bs] = 0
        t += n
    cache = cache.to(torch.bfloat16)
    qkv = torch.randn(t, nq + 2 * nkv, D, device="cuda", generator=g)
    qkv[:, nq:nq + nkv] *= head_scale.view(1, nkv, 1)
    qkv[:, nq + nkv:] *= head_scale.view(1, nkv, 1)
    qkv = qkv.to(torch.bfloat16)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
    bt, qs, ql, kl = bt.cuda(), i32(q_start), i32(q_len), i32(kv_len)
    slots = torch.tensor(slots, dtype=torch.int64, device="cuda")
    layer = FP8KVLayer(*quantize_kv_fp8(cache))
    kv_cache_append(qkv, cache, slots, nq, nkv)
    kv_cache_append(qkv, layer, slots, nq, nkv)
    q, scale = qkv[:, :nq], D ** -0.5
    ref_deq = paged_attention_reference(q.float(), dequantize_kv_fp8(layer), bt, qs, ql, kl, scale, window)
    ref32 = paged_attention_reference(q.float(), cache.float(), bt, qs, ql, kl, scale, window)
    return dict(q=q, layer=layer, meta=(bt, qs, ql, kl), scale=scale, maxkv=max(kv_len), ref_deq=ref_deq, ref32=ref32)


@pytest.mark.parametrize("bs", [16, 64])
@pytest.mark.parametrize("D", [64, 128, 256])
def test_fp8_append_matches_definition(D, bs):
    """kv_cache_append and rope_kv_cache_append into an FP8 layer: the scales are the PyTorch
    definition's (of the bf16 rows the bf16 op stores), the dequantised rows meet the e4m3 bound
    against those rows, slots never written stay zero, and the RoPE form rotates qkv bit-identically."""
    from shuffle_exchange_amd.ops.paged_attention import (FP8KVLayer, dequantize_kv_fp8, kv_cache_append,
                                                          quantize_kv_fp8, rope_kv_cache_append)
    from shuffle_exchange_amd.ops.rope import RopeCache
    torch.manual_seed(D + bs)
    T, nq, nkv, nblk = 37, 3, 2, 8  # nq + nkv odd: the v rows of the RoPE kernel start mid-group
    rope = RopeCache(D, 512, 10000.0, device="cuda")
    qkv = torch.randn(T, nq + 2 * nkv, D, device="cuda") * torch.logspace(-2, 2, T, device="cuda").view(T, 1, 1)
    qkv[5, nq + nkv] = 0  # an all-zero v row
    qkv = qkv.to(torch.bfloat16)
    pos = torch.randint(0, 512, (T,), device="cuda")
    slots = torch.randperm(nblk * bs, device="cuda")[:T].long()
    slots[11] = -1
    pos[11] = 7  # not position 0, where the rotation is the identity
    for fused in (False, True):
        ref = torch.zeros(nblk, 2, nkv, bs, D, device="cuda", dtype=torch.bfloat16)
        layer = FP8KVLayer(torch.zeros(nblk, 2, nkv, bs, D, device="cuda").to(torch.float8_e4m3fn),
                           torch.zeros(nblk, 2, nkv, bs, device="cuda"))
        a, b = qkv.clone(), qkv.clone()
        if fused:
            rope_kv_cache_append(a, rope, pos, ref, slots, nq, nkv)
            rope_kv_cache_append(b, rope, pos, layer, slots, nq, nkv)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16))
            assert not torch.equal(a[11], qkv[11])  # the skipped slot's token is still rotated
        else:
            kv_cache_append(a, ref, slots, nq, nkv)
            kv_cache_append(b, layer, slots, nq, nkv)
            assert torch.equal(b, qkv)
        torch.cuda.synchronize()
        written = torch.zeros(nblk * bs, dtype=torch.bool, device="cuda")
        written[slots[slots >= 0]] = True
        written = written.view(nblk, 1, 1, bs).expand(nblk, 2, nkv, bs)
        x = ref.float()
        _, s_def = quantize_kv_fp8(x)
        torch.testing.assert_close(layer.scales[written], s_def[written], rtol=1e-6, atol=0)
        err = (dequantize_kv_fp8(layer) - x).abs()
        assert bool((err <= kv_fp8_bound(x, layer.scales))[written].all()), (fused, float(err.max()))
        assert int(layer.scales[~written].count_nonzero()) == 0
        assert int(layer.codes.view(torch.uint8)[~written].count_nonzero()) == 0
        assert int(ref[~written].count_nonzero()) == 0


SEQS = [((0, 1),), ((37, 1), (500, 1), (0, 5)), ((130, 3), (1, 20), (300, 1)), ((0, 70),)]
LAYOUTS = [(8, 2, 128, 64), (4, 4, 64, 16), (8, 4, 256, 32)]


def _check(c, out):
    """Kernel error against the dequantised cache (global, as for the bf16 kernel, and per head), and
    the end-to-end bound against the unquantised cache with the quantiser's own error measured."""
    k_err, k_err_head = _rel(out, c["ref_deq"]), _rel_heads(out, c["ref_deq"])
    e2e, quant = _rel(out, c["ref32"]), _rel(c["ref_deq"], c["ref32"])
    print(f"kernel {k_err:.2e} (worst head {k_err_head:.2e}) end-to-end {e2e:.2e} quantiser {quant:.2e}")
    assert k_err < 1e-2, k_err
    assert k_err_head < 1e-2, k_err_head
    assert e2e <= quant + 1e-2, (e2e, quant)


@pytest.mark.parametrize("splits", [None, 1, 3])
@pytest.mark.parametrize("nq,nkv,D,bs", LAYOUTS)
@pytest.mark.parametrize("seqs", SEQS)
def test_paged_attention_fp8(seqs, nq, nkv, D, bs, splits):
    from shuffle_exchange_amd.ops.paged_attention import paged_attention
    c = _case(seqs, nq, nkv, D, bs)
    out = paged_attention(c["q"], c["layer"], *c["meta"], c["scale"], c["maxkv"], splits)
    _check(c, out)


@pytest.mark.parametrize("nq,nkv,D,bs,window", [(8, 2, 128, 64, 256), (4, 1, 64, 16, 100), (16, 2, 256, 64, 300)])
def test_paged_attention_fp8_window(nq, nkv, D, bs, window):
    from shuffle_exchange_amd.ops.paged_attention import paged_attention
    c = _case(((37, 1), (500, 1), (600, 5)), nq, nkv, D, bs, window=window, seed=3)
    for splits in (None, 2):
        out = paged_attention(c["q"], c["layer"], *c["meta"], c["scale"], c["maxkv"], splits, window=window)
        _check(c, out)


def test_paged_attention_parts_fp8():
    from shuffle_exchange_amd.ops.paged_attention import (merge_attention_parts, paged_attention,
                                                          paged_attention_parts)
    c = _case(((700, 1), (1500, 1), (37, 1)), 8, 2, 128, 64)
    out, parts = paged_attention_parts(c["q"], c["layer"], *c["meta"], c["scale"], c["maxkv"], 3)
    assert out is None and parts is not None and parts[0].shape[0] == 3
    merged = merge_attention_parts(parts[0], parts[1], c["q"].dtype)
    fused = paged_attention(c["q"], c["layer"], *c["meta"], c["scale"], c["maxkv"], 3)
    assert _rel(merged, fused) < 1e-2
    _check(c, merged)


@functools.lru_cache(maxsize=None)
def _exact_case(nq, nkv, D, bs, seqs=((37, 1), (130, 3), (0, 20))):
    """A cache that both formats hold exactly: random e4m3 codes (the two NaN codes replaced), code
    0x7e (= 448) once in every row so that every row scale is exactly 1, and one all-zero row in the
    history of the second sequence. Its bf16 image is what the bf16 kernel reads."""
    from shuffle_exchange_amd.ops.paged_attention import FP8KVLayer, dequantize_kv_fp8, quantize_kv_fp8
    g = torch.Generator(device="cuda").manual_seed(D + bs)
    nblk = [(c + n + bs - 1) // bs for c, n in seqs]
    bt = torch.zeros(len(seqs), max(nblk), dtype=torch.int32)
    perm = torch.randperm(sum(nblk) + 2, generator=torch.Generator().manual_seed(bs)).tolist()
    for i, nb in enumerate(nblk):
        bt[i, :nb] = torch.tensor([perm.pop() for _ in range(nb)], dtype=torch.int32)
    codes = torch.randint(0, 256, (sum(nblk) + 2, 2, nkv, bs, D), device="cuda", generator=g, dtype=torch.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0x38  # NaN -> 1.0
    top = torch.randint(0, D, codes.shape[:-1] + (1,), device="cuda", generator=g)
    codes.scatter_(-1, top, torch.full_like(top, 0x7e, dtype=torch.uint8))
    codes[int(bt[1, 65 // bs]), :, 0, 65 % bs] = 0
    layer = FP8KVLayer(codes.view(torch.float8_e4m3fn), torch.ones(codes.shape[:-1], device="cuda"))
    image = layer.codes.to(torch.bfloat16)
    qc, qscales = quantize_kv_fp8(image)
    assert torch.equal(qc.view(torch.uint8), codes) and bool((qscales == 1).all())
    assert torch.equal(image.float(), dequantize_kv_fp8(layer))
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
    q_len = [n for _, n in seqs]
    q_start = [sum(q_len[:i]) for i in range(len(seqs))]
    kv_len = [c + n for c, n in seqs]
    # |k| reaches 448: small queries keep the softmax spread over many keys
    q = (torch.randn(sum(q_len), nq, D, device="cuda", generator=g) / 64).to(torch.bfloat16)
    return dict(q=q, layer=layer, image=image, meta=(bt.cuda(), i32(q_start), i32(q_len), i32(kv_len)),
                scale=D ** -0.5, maxkv=max(kv_len))


@pytest.mark.parametrize("window", [None, 50])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("nq,nkv,D,bs", [(4, 2, 64, 16), (8, 2, 128, 64), (4, 2, 256, 32)])
def test_fp8_and_bf16_caches_share_one_kernel_body(nq, nkv, D, bs, splits, window):
    """With unit row scales the FP8 path does the bf16 path's arithmetic on the bf16 path's values
    (the widened codes are the bf16 image, and multiplying by 1.0f is exact), so the two outputs agree
    bit for bit: every head dim, a partial last chunk, several 16-row passes, window chunk skipping,
    and the partials with the merge launch. Before the two kernels were built from one body the
    outputs were also bit-equal (worst absolute difference 0 over these 12 cases)."""
    from shuffle_exchange_amd.ops.paged_attention import paged_attention
    c = _exact_case(nq, nkv, D, bs)
    out8 = paged_attention(c["q"], c["layer"], *c["meta"], c["scale"], c["maxkv"], splits, window=window)
    out16 = paged_attention(c["q"], c["image"], *c["meta"], c["scale"], c["maxkv"], splits, window=window)
    diff = (out8.float() - out16.float()).abs().max().item()
    print(f"worst |fp8 - bf16| {diff:.3e}; largest |out| {out16.float().abs().max().item():.3e}")
    assert bool(out16.float().abs().sum() > 0)
    assert torch.equal(out8, out16), diff


def test_fp8_ops_reject_wrong_operands():
    c = _case(((37, 1), (500, 1), (0, 5)), 8, 2, 128, 64)
    bt, qs, ql, kl = c["meta"]
    codes, scales = c["layer"]
    with pytest.raises(RuntimeError, match="scales"):
        torch.ops.sxe.paged_attention_fp8(c["q"], codes, scales[:, :, :, :-1].contiguous(), bt, qs, ql, kl, 0.1,
                                          c["maxkv"], 1, 0)
    with pytest.raises(RuntimeError, match="e4m3fn"):
        torch.ops.sxe.paged_attention_fp8(c["q"], codes.view(torch.uint8), scales, bt, qs, ql, kl, 0.1, c["maxkv"], 1,
                                          0)


# ------------------------------------------------------------------------------------------ engine
def _model(vocab=2048):
    from shuffle_exchange_amd.models import LlamaForCausalLM, llama_config
    torch.manual_seed(0)
    cfg = llama_config("llama-tiny", hidden_size=512, intermediate_size=1024, num_attention_heads=4,
                       num_key_value_heads=2, vocab_size=vocab, num_hidden_layers=2, max_position_embeddings=4096)
    return LlamaForCausalLM(cfg).to("cuda", torch.bfloat16).eval()


def test_ragged_engine_fp8_cache_matches_forward():
    """Flash prefill / paged prefill / chunked continuation / decode from an FP8 cache against the
    model's full forward, at the cosine threshold derived on the CPU reference path."""
    from shuffle_exchange_amd.inference.v2 import RaggedInferenceEngineConfig, build_engine
    m = _model()
    eng = build_engine(m, RaggedInferenceEngineConfig(kv_block_size=64, num_kv_blocks=256, kv_cache_dtype="fp8"))
    worst = engine_min_cos(m, eng, "cuda")
    print("minimum cosine", worst)
    assert worst > ENGINE_COS_MIN, worst


def test_decode_graphs_fp8_cache_match_eager():
    from shuffle_exchange_amd.inference.v2 import RaggedInferenceEngineConfig, build_engine
    m = _model(512)
    eg, ee = (build_engine(m, RaggedInferenceEngineConfig(kv_block_size=64, num_kv_blocks=64, decode_graphs=graphs,
                                                          kv_cache_dtype="fp8")) for graphs in (True, False))
    g = torch.Generator().manual_seed(1)
    prompts = {u: torch.randint(0, 512, (n,), generator=g).tolist() for u, n in {0: 300, 1: 17, 2: 70}.items()}
    torch.testing.assert_close(eg.put(list(prompts), list(prompts.values())),
                               ee.put(list(prompts), list(prompts.values())))
    for step in range(8):
        toks = [[int(torch.randint(0, 512, (1,), generator=g))] for _ in prompts]
        a, b = eg.put(list(prompts), toks), ee.put(list(prompts), toks)
        rel = _rel(a, b)
        assert rel < 2e-2, (step, rel)
    assert eg._decode_runner().replays == 8 and ee._decode_runner() is None


def test_fp8_cache_holds_more_blocks_for_the_same_budget():
    from shuffle_exchange_amd.inference.v2 import RaggedInferenceEngineConfig, build_engine
    from shuffle_exchange_amd.inference.v2.engine_v2 import MemoryConfig, StateManagerConfig
    m = _model(512)
    n = {}
    for name in ("bf16", "fp8"):
        sm = StateManagerConfig(memory_config=MemoryConfig(mode="allocate", size=32 * 2**20))
        n[name] = build_engine(m, RaggedInferenceEngineConfig(state_manager=sm, kv_cache_dtype=name)).n_kv_blocks
    assert n["fp8"] > n["bf16"], n
    assert n == {"bf16": 32 * 2**20 // (2 * 2 * 2 * 64 * 128 * 2), "fp8": 32 * 2**20 // (2 * 2 * 2 * 64 * 132)}, n
