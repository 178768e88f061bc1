"""gfx950 flash attention in band mode (packed documents and / or a sliding window) vs the fp32
reference: every head dim and kernel variant the host dispatches, exact no-leak checks across
document boundaries, clamped garbage bounds, the strided / fused / padded entry points, routing and
the Llama model's ``packed_samples`` switch. Tolerances are those of tests/test_flash_attn_gpu.py."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.fixture(scope="module", autouse=True)
def _native():
    from shuffle_exchange_amd.ops import native
    native.require_hip()


def _pos(S, starts_per_row, device="cuda"):
    pos = torch.zeros(len(starts_per_row), S, dtype=torch.long)
    for b, starts in enumerate(starts_per_row):
        st = sorted(starts) + [S]
        for a, e in zip(st[:-1], st[1:]):
            pos[b, a:e] = torch.arange(e - a)
    return pos.to(device)


def _bounds(S, starts_per_row, window=None):
    from shuffle_exchange_amd.ops.attention import band_bounds
    pos = _pos(S, starts_per_row) if any(len(s) > 1 for s in starts_per_row) else None
    return band_bounds(S, len(starts_per_row), "cuda", position_ids=pos, window=window)


def _qkv(B, S, H, Hk, D, seed=0):
    torch.manual_seed(seed)
    return (torch.randn(B, S, H, D, device="cuda", dtype=torch.bfloat16, requires_grad=True),
            torch.randn(B, S, Hk, D, device="cuda", dtype=torch.bfloat16, requires_grad=True),
            torch.randn(B, S, Hk, D, device="cuda", dtype=torch.bfloat16, requires_grad=True))


def _check(q, k, v, bounds):
    """attention(..., bounds) forward + backward against the fp32 oracle."""
    from shuffle_exchange_amd.ops.attention import attention, reference_attention
    o = attention(q, k, v, causal=True, bounds=bounds)
    q2, k2, v2 = (t.detach().float().requires_grad_() for t in (q, k, v))
    o2 = reference_attention(q2, k2, v2, causal=True, bounds=bounds)
    do = torch.randn_like(o2)
    (o.float() * do).sum().backward()
    (o2 * do).sum().backward()
    errs = [_rel(o, o2), _rel(q.grad, q2.grad), _rel(k.grad, k2.grad), _rel(v.grad, v2.grad)]
    if float(q2.grad.norm()) == 0.0 and float(k2.grad.norm()) == 0.0:
        # every query sees only itself (window 1): p = 1 and dS = dO.v - delta = 0 exactly, so the true
        # dq / dk are zero and a relative error has no denominator. Measure the error against the two
        # terms that cancel instead: dq_i = scale (dO_i.v_i - delta_i) k_i, dk_i = scale sum_h (...) q_ih
        rep = q.shape[2] // k.shape[2]
        dp = (do * v2.detach().repeat_interleave(rep, 2)).sum(-1, keepdim=True) * q.shape[-1] ** -0.5
        tq = dp * k2.detach().repeat_interleave(rep, 2)
        tk = (dp * q2.detach()).view(*k.shape[:3], rep, -1).sum(3)
        errs[1] = (q.grad.float().norm() / tq.norm()).item()
        errs[2] = (k.grad.float().norm() / tk.norm()).item()
    print("rel err o/dq/dk/dv:", errs)
    assert errs[0] < 1e-2
    assert errs[1] < 2e-2 and errs[2] < 2e-2 and errs[3] < 2e-2


STARTS_384 = [[0, 37, 200], [0, 129, 130, 300]]


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("H,Hk", [(4, 4), (8, 2)])
def test_band_documents(H, Hk, D):
    q, k, v = _qkv(2, 384, H, Hk, D)
    _check(q, k, v, _bounds(384, STARTS_384))


@pytest.mark.parametrize("waves", [4, 8])
def test_band_long_document_wave_variants(waves, monkeypatch):
    monkeypatch.setenv("SXE_FA_DQ_WAVES", str(waves))
    monkeypatch.setenv("SXE_FA_DKDV_WAVES", str(waves))
    q, k, v = _qkv(1, 512, 8, 2, 128)
    _check(q, k, v, _bounds(512, [[0, 300]]))


@pytest.mark.parametrize("D,fwd_waves,dma,bwd_waves", [(128, 4, "1", 4), (64, 4, "0", 8), (128, 8, "0", 8)])
def test_band_forward_knobs(D, fwd_waves, dma, bwd_waves, monkeypatch):
    """The forward knobs in band mode at a length that allows 8 waves: SXE_FA_FWD_WAVES=4 narrows the
    band forward too, SXE_FA_FWD_DMA=0 is ignored by it (the band forward is always the LDS-DMA one);
    head dim 64 with the 8-wave band dQ."""
    monkeypatch.setenv("SXE_FA_FWD_WAVES", str(fwd_waves))
    monkeypatch.setenv("SXE_FA_FWD_DMA", dma)
    monkeypatch.setenv("SXE_FA_DQ_WAVES", str(bwd_waves))
    monkeypatch.setenv("SXE_FA_DKDV_WAVES", str(bwd_waves))
    q, k, v = _qkv(1, 256, 2, 1, D)
    _check(q, k, v, _bounds(256, [[0, 100]]))


@pytest.mark.parametrize("hpw", [1, 2, 4])
def test_band_dkdv_heads_per_workgroup(hpw, monkeypatch):
    monkeypatch.setenv("SXE_FA_DKDV_HPW", str(hpw))
    q, k, v = _qkv(1, 512, 8, 2, 128)
    _check(q, k, v, _bounds(512, [[0, 300]]))


@pytest.mark.parametrize("one_sweep", [0, 1])
def test_band_d256_sweep_modes(one_sweep, monkeypatch):
    monkeypatch.setenv("SXE_FA_DKDV_ONE_SWEEP", str(one_sweep))
    q, k, v = _qkv(1, 512, 4, 2, 256)
    _check(q, k, v, _bounds(512, [[0, 300]]))


@pytest.mark.parametrize("W,starts", [(1, [0]), (20, [0]), (100, [0]), (128, [0]), (1000, [0]), (100, [0, 300])])
def test_band_window(W, starts):
    q, k, v = _qkv(1, 512, 4, 2, 128)
    _check(q, k, v, _bounds(512, [starts], window=W))


def test_band_no_leak_forward_and_backward():
    S, cut, D = 384, 200, 128
    q, k, v = (t.detach() for t in _qkv(2, S, 8, 2, D))
    klo, qhi = _bounds(S, [[0, cut], [0, cut]])
    sc = D ** -0.5
    ops = torch.ops.sxe
    o, lse = ops.flash_attn_fwd_band(q, k, v, klo, qhi, sc)
    k2, v2 = k.clone(), v.clone()
    k2[:, :cut], v2[:, :cut] = torch.randn_like(k[:, :cut]), torch.randn_like(v[:, :cut])
    o2, _ = ops.flash_attn_fwd_band(q, k2, v2, klo, qhi, sc)
    assert torch.equal(o[:, cut:], o2[:, cut:])
    assert not torch.equal(o[:, :cut], o2[:, :cut])

    def grads(do):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ops.flash_attn_bwd_band(do, q, k, v, o, lse, dq, dk, dv, klo, qhi, sc)
        return dq, dk, dv
    do = torch.randn_like(o)
    do2 = do.clone()
    do2[:, cut:] = torch.randn_like(do[:, cut:])
    (_, dk, dv), (_, dk2, dv2) = grads(do), grads(do2)
    assert torch.equal(dk[:, :cut], dk2[:, :cut]) and torch.equal(dv[:, :cut], dv2[:, :cut])
    assert not torch.equal(dk[:, cut:], dk2[:, cut:])


@pytest.mark.parametrize("D", [64, 128, 256])
def test_band_garbage_bounds_are_clamped(D):
    S = 256
    q, k, v = (t.detach() for t in _qkv(1, S, 4, 2, D))
    klo = torch.full((1, S), S + 5, dtype=torch.int32, device="cuda")
    qhi = torch.full((1, S), -3, dtype=torch.int32, device="cuda")
    o, lse = torch.ops.sxe.flash_attn_fwd_band(q, k, v, klo, qhi, D ** -0.5)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    torch.ops.sxe.flash_attn_bwd_band(torch.randn_like(o), q, k, v, o, lse, dq, dk, dv, klo, qhi, D ** -0.5)
    torch.cuda.synchronize()
    for t in (o, lse, dq, dk, dv):
        assert torch.isfinite(t.float()).all()
    # clamped to klo = i, qhi = j: every query sees only itself
    assert _rel(o, v.repeat_interleave(2, dim=2)) < 1e-2


def test_band_host_checks():
    q, k, v = (t.detach() for t in _qkv(1, 256, 4, 2, 128))
    klo, qhi = _bounds(256, [[0, 100]])
    with pytest.raises(RuntimeError):
        torch.ops.sxe.flash_attn_fwd_band(q, k, v, klo.long(), qhi.long(), 0.1)
    with pytest.raises(RuntimeError):
        torch.ops.sxe.flash_attn_fwd_band(q, k, v, klo[:, :128].contiguous(), qhi[:, :128].contiguous(), 0.1)
    with pytest.raises(RuntimeError):
        torch.ops.sxe.flash_attn_fwd_band(q[:, :128], k, v, klo, qhi, 0.1)


def _fused_ref(qkv, nq, nkv, bounds, do):
    from shuffle_exchange_amd.ops.attention import reference_attention
    r = qkv.detach().float().requires_grad_()
    o = reference_attention(r[:, :, :nq], r[:, :, nq:nq + nkv], r[:, :, nq + nkv:], causal=True, bounds=bounds)
    (o * do).sum().backward()
    return o, r.grad


def test_band_attention_qkv_rope_strided():
    from shuffle_exchange_amd.ops.attention import attention_qkv_rope
    torch.manual_seed(0)
    B, S, nq, nkv, D = 2, 384, 8, 2, 128
    base = torch.randn(B, S, nq + 2 * nkv, D, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    bounds = _bounds(S, STARTS_384)
    o = attention_qkv_rope(base * 1, nq, nkv, None, None, causal=True, bounds=bounds)
    do = torch.randn(B, S, nq, D, device="cuda")
    (o.float() * do).sum().backward()
    ro, rg = _fused_ref(base, nq, nkv, bounds, do)
    assert _rel(o, ro) < 1e-2
    assert _rel(base.grad, rg) < 2e-2


def test_band_qkv_proj_attention_fused():
    from shuffle_exchange_amd.ops import attention as att
    from shuffle_exchange_amd.ops.linear import Linear
    torch.manual_seed(0)
    B, S, nq, nkv, D, Hd = 2, 384, 4, 2, 64, 256
    proj = Linear(Hd, (nq + 2 * nkv) * D, bias=False, init_std=0.05).to("cuda", torch.bfloat16)
    x = torch.randn(B, S, Hd, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    bounds = _bounds(S, STARTS_384)
    ran = []
    orig = att._QKVProjAttn.apply
    att._QKVProjAttn.apply = lambda *a: (ran.append(a[-2:]), orig(*a))[1]  # (klo, qhi) trail the arguments
    try:
        o = att.qkv_proj_attention(x, proj, nq, nkv, None, None, causal=True, bounds=bounds)
    finally:
        att._QKVProjAttn.apply = orig
    assert len(ran) == 1, "the fused QKV-projection node did not run"
    assert ran[0][0] is bounds[0] and ran[0][1] is bounds[1], "the fused node did not get the band bounds"
    do = torch.randn(B, S, nq, D, device="cuda")
    (o.float() * do).sum().backward()
    qkv = torch.nn.functional.linear(x.detach(), proj.weight.detach()).view(B, S, nq + 2 * nkv, D)
    ro, rg = _fused_ref(qkv, nq, nkv, bounds, do)
    assert _rel(o, ro) < 1e-2
    dx = rg.reshape(B * S, -1) @ proj.weight.detach().float()
    dw = rg.reshape(B * S, -1).t() @ x.detach().float().reshape(B * S, -1)
    assert _rel(x.grad.reshape(B * S, -1), dx) < 2e-2
    assert _rel(proj.weight.grad, dw) < 2e-2


def test_band_padded_path():
    torch.manual_seed(0)
    q, k, v = _qkv(2, 200, 4, 2, 96)
    _check(q, k, v, _bounds(200, [[0, 77], [0, 150]]))


def test_band_routing(monkeypatch):
    from shuffle_exchange_amd.ops import attention as att

    def boom(*a, **kw):
        raise AssertionError("wrong attention path")
    q, k, v = (t.detach() for t in _qkv(1, 256, 4, 2, 128))
    bounds = _bounds(256, [[0, 100]])
    calls = []
    fwd_band = torch.ops.sxe.flash_attn_fwd_band
    with monkeypatch.context() as mp:
        mp.setattr(att, "_sdpa", boom)
        mp.setattr(torch.ops.sxe, "flash_attn_fwd_band", lambda *a: (calls.append(1), fwd_band(*a))[1])
        att.attention(q, k, v, causal=True, bounds=bounds)
    assert calls == [1]
    with monkeypatch.context() as mp:
        mp.setattr(att, "_sdpa", boom)
        mp.setattr(torch.ops.sxe, "flash_attn_fwd_band", boom)
        mp.setattr(torch.ops.sxe, "flash_attn_bwd_band", boom)
        o = att.attention(q, k, v, causal=True, bounds=None)
    o2 = att.reference_attention(q.float(), k.float(), v.float(), causal=True)
    assert _rel(o, o2) < 1e-2


def _tiny_cfg(**kw):
    from shuffle_exchange_amd.models import llama_config
    return llama_config("llama-tiny", hidden_size=256, intermediate_size=512, num_attention_heads=4,
                        num_key_value_heads=2, vocab_size=1024, num_hidden_layers=2, **kw)  # head dim 64


def test_llama_packed_samples_gpu():
    from shuffle_exchange_amd.models import LlamaForCausalLM
    from shuffle_exchange_amd.ops import attention as att
    torch.manual_seed(0)
    S, cut = 256, 100
    ref = LlamaForCausalLM(_tiny_cfg(packed_samples=True)).float()
    dev = copy.deepcopy(ref).to("cuda", torch.bfloat16)
    ids = torch.randint(0, 1024, (2, S))
    pos = _pos(S, [[0, cut], [0, cut]], "cpu")
    lr = ref(ids, labels=ids, position_ids=pos)
    ran = []
    orig = att._QKVProjAttn.apply
    att._QKVProjAttn.apply = lambda *a: (ran.append(a[-2:]), orig(*a))[1]  # (klo, qhi) trail the arguments
    try:
        ld = dev(ids.cuda(), labels=ids.cuda(), position_ids=pos.cuda())
        ld.backward()
    finally:
        att._QKVProjAttn.apply = orig
    assert len(ran) == 2, "both layers must run the fused node"
    assert all(torch.is_tensor(klo) and torch.is_tensor(qhi) for klo, qhi in ran), \
        "both layers must run the band kernels"
    print("loss gpu / cpu:", float(ld), float(lr))
    assert abs(float(ld) - float(lr)) / float(lr) < 2e-2
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in dev.parameters())
    # no leak: document 2's logits do not change with document 1's tokens
    ids2 = ids.clone()
    ids2[:, :cut] = torch.randint(0, 1024, (2, cut))
    with torch.no_grad():
        a = dev(ids.cuda(), position_ids=pos.cuda())
        b = dev(ids2.cuda(), position_ids=pos.cuda())
    assert torch.equal(a[:, cut:], b[:, cut:])
    assert not torch.equal(a[:, :cut], b[:, :cut])
