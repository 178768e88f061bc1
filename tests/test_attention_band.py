"""Band masks of the attention op (packed documents and / or a sliding window), CPU side:
``band_bounds`` against a brute-force loop, ``attention(..., bounds=...)`` against the fp32 oracle and
against every document run alone, and the Llama model's ``packed_samples`` switch."""
import pytest
import torch

from shuffle_exchange_amd.ops.attention import attention, band_bounds, reference_attention


def _pos_from_starts(S, starts_per_row):
    pos = torch.zeros(len(starts_per_row), S, dtype=torch.long)
    for b, starts in enumerate(starts_per_row):
        st = sorted(starts) + [S]
        for a, e in zip(st[:-1], st[1:]):
            pos[b, a:e] = torch.arange(e - a)
    return pos


def _brute(S, starts_per_row, window):
    """klo / qhi by definition: query i sees key j iff j <= i, same document, i - j < window."""
    B = len(starts_per_row)
    klo, qhi = torch.zeros(B, S, dtype=torch.int32), torch.zeros(B, S, dtype=torch.int32)
    for b, starts in enumerate(starts_per_row):
        doc = [sum(1 for s in starts if s <= i) for i in range(S)]

        def sees(i, j):
            return j <= i and doc[i] == doc[j] and (window is None or i - j < window)
        for i in range(S):
            klo[b, i] = min(j for j in range(S) if sees(i, j))
            qhi[b, i] = max(q for q in range(S) if sees(q, i))
    return klo, qhi


CASES = [
    ("docs", 24, [[0, 5, 17]], None),
    ("window", 24, [[0]], 4),
    ("both", 24, [[0, 5, 17]], 4),
    ("w1", 16, [[0, 7]], 1),
    ("w_ge_S", 16, [[0, 7]], 100),
    ("doc_len1", 16, [[0, 6, 7, 12]], None),
    ("two_rows", 24, [[0, 5, 17], [0, 1, 2, 20]], 6),
]


@pytest.mark.parametrize("name,S,starts,window", CASES, ids=[c[0] for c in CASES])
def test_band_bounds_matches_brute_force(name, S, starts, window):
    B = len(starts)
    docs = any(len(s) > 1 for s in starts)
    pos = _pos_from_starts(S, starts) if docs else None
    klo, qhi = band_bounds(S, B, "cpu", position_ids=pos, window=window)
    rk, rq = _brute(S, starts, window)
    assert klo.dtype == torch.int32 and qhi.dtype == torch.int32 and klo.shape == (B, S)
    assert torch.equal(klo, rk) and torch.equal(qhi, rq)
    idx = torch.arange(S)
    assert (klo[:, 1:] >= klo[:, :-1]).all() and (qhi[:, 1:] >= qhi[:, :-1]).all()
    assert (klo <= idx).all() and (qhi >= idx).all()
    if docs:  # doc_ids say the same as position_ids
        ids = torch.tensor([[sum(1 for s in st if s <= i) for i in range(S)] for st in starts])
        k2, q2 = band_bounds(S, B, "cpu", doc_ids=ids, window=window)
        assert torch.equal(k2, rk) and torch.equal(q2, rq)


def test_band_bounds_none_without_documents_or_window():
    assert band_bounds(16, 2, "cpu") is None


def test_attention_cpu_bounds_match_reference_and_per_document():
    torch.manual_seed(0)
    B, S, H, Hk, D = 2, 48, 4, 2, 16
    starts = [[0, 11, 30], [0, 1, 40]]
    q, k, v = torch.randn(B, S, H, D), torch.randn(B, S, Hk, D), torch.randn(B, S, Hk, D)
    bounds = band_bounds(S, B, "cpu", position_ids=_pos_from_starts(S, starts))
    o = attention(q, k, v, causal=True, bounds=bounds)
    ref = reference_attention(q, k, v, causal=True, bounds=bounds)
    assert (o - ref).abs().max().item() < 1e-5
    alone = torch.empty_like(ref)
    for b, st in enumerate(starts):
        for a, e in zip(st, st[1:] + [S]):
            alone[b:b + 1, a:e] = reference_attention(q[b:b + 1, a:e], k[b:b + 1, a:e], v[b:b + 1, a:e], causal=True)
    assert (o - alone).abs().max().item() < 1e-5
    # and a window on top differs from documents alone but still matches the oracle
    bw = band_bounds(S, B, "cpu", position_ids=_pos_from_starts(S, starts), window=5)
    ow = attention(q, k, v, causal=True, bounds=bw)
    assert (ow - reference_attention(q, k, v, causal=True, bounds=bw)).abs().max().item() < 1e-5
    assert (ow - o).abs().max().item() > 1e-3


def _tiny(**kw):
    from shuffle_exchange_amd.models import LlamaForCausalLM, llama_config
    torch.manual_seed(0)
    return LlamaForCausalLM(llama_config("llama-tiny", **kw)).float().eval()


def test_llama_packed_samples_isolates_documents():
    S, cut = 64, 23
    pos = _pos_from_starts(S, [[0, cut]])
    torch.manual_seed(1)
    ids = torch.randint(0, 512, (1, S))
    ids2 = ids.clone()
    ids2[:, :cut] = torch.randint(0, 512, (1, cut))
    assert not torch.equal(ids, ids2)
    with torch.no_grad():
        m = _tiny(packed_samples=True)
        a, b = m(ids, position_ids=pos), m(ids2, position_ids=pos)
        assert torch.equal(a[:, cut:], b[:, cut:])       # document 2 never saw document 1
        assert not torch.equal(a[:, :cut], b[:, :cut])
        m = _tiny(packed_samples=False)                   # the same check sees the leak without the mask
        a, b = m(ids, position_ids=pos), m(ids2, position_ids=pos)
        assert not torch.equal(a[:, cut:], b[:, cut:])


def test_llama_sliding_window_limits_the_context():
    S, W = 64, 8
    torch.manual_seed(1)
    ids = torch.randint(0, 512, (1, S))
    ids2 = ids.clone()
    ids2[:, :16] = torch.randint(0, 512, (1, 16))
    with torch.no_grad():
        m = _tiny(sliding_window=W)  # 2 layers: a token depends on the last 2 (W - 1) + 1 tokens
        a, b = m(ids), m(ids2)
        assert torch.equal(a[:, 16 + 2 * (W - 1):], b[:, 16 + 2 * (W - 1):])
        assert not torch.equal(a[:, 16:16 + W - 1], b[:, 16:16 + W - 1])


def test_ring_with_packed_samples_raises():
    m = _tiny(packed_samples=True, sequence_parallel=True, sp_mode="ring")
    ids = torch.randint(0, 512, (1, 64))
    with pytest.raises(NotImplementedError):
        m(ids, position_ids=_pos_from_starts(64, [[0, 20]]))
