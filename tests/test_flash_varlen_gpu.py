"""gfx950 variable-length flash forward (``flash_attn_fwd_varlen``: whole sequences packed in one
ragged token buffer, one launch) vs the fp32 ``reference_attention`` run per sequence: lengths around
every tile edge, GQA, the three head dims, sliding windows, rows past the buffer's end that hold NaN,
no leak between sequences, no write outside the table's sequences, and the host checks. Tolerance:
relative error of o < 1e-2 as in tests/test_flash_attn_gpu.py, asserted per sequence."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-2
EDGE_LENS = [1, 31, 32, 33, 127, 128, 129, 255, 257, 300]


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.fixture(scope="module", autouse=True)
def _native():
    from shuffle_exchange_amd.ops import native
    native.require_hip()


def _table(lens, routed=None):
    """Device work table over the sequences ``routed`` (default all) of a buffer holding ``lens``."""
    from shuffle_exchange_amd.inference.v2.ragged.ragged import build_varlen_table
    starts = [sum(lens[:i]) for i in range(len(lens))]
    seen = [0 if (routed is None or i in routed) else 1 for i in range(len(lens))]
    ids, _, rows = build_varlen_table(starts, lens, seen, min_len=1)
    assert ids == (list(range(len(lens))) if routed is None else sorted(routed))
    assert len(rows) == sum(-(-lens[i] // 128) for i in ids)
    return torch.tensor(rows, dtype=torch.int32, device="cuda").view(-1, 3)


def _packed(T, Hq, Hkv, D, seed=0, extra_rows=0, fill=0.0):
    """q, k, v as strided views of one packed [T, Hq + 2 Hkv, D] buffer (the first T rows of a larger
    allocation whose other rows hold ``fill``)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    big = torch.full((T + extra_rows, Hq + 2 * Hkv, D), fill, device="cuda", dtype=torch.bfloat16)
    big[:T] = torch.randn(T, Hq + 2 * Hkv, D, device="cuda", generator=g).to(torch.bfloat16)
    qkv = big[:T]
    return big, qkv, (qkv[:, :Hq], qkv[:, Hq:Hq + Hkv], qkv[:, Hq + Hkv:])


def _oracle(q, k, v, lens, window=None):
    from shuffle_exchange_amd.ops.attention import band_bounds, reference_attention
    outs, s = [], 0
    for n in lens:
        sl = slice(s, s + n)
        bounds = band_bounds(n, 1, "cuda", window=window) if window is not None else None
        outs.append(reference_attention(q[sl][None].float(), k[sl][None].float(), v[sl][None].float(), True,
                                        bounds=bounds)[0])
        s += n
    return outs


def _assert_close(o, refs, lens, ids=None):
    s = 0
    for i, n in enumerate(lens):
        if ids is None or i in ids:
            err = _rel(o[s:s + n], refs[i])
            print(f"seq {i} len {n}: rel err {err:.3e}")
            assert err < TOL, (i, n, err)
        s += n


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("Hq,Hkv", [(4, 4), (8, 2)])
def test_tile_edge_lengths(Hq, Hkv, D):
    T = sum(EDGE_LENS)
    _, _, (q, k, v) = _packed(T, Hq, Hkv, D)
    assert not q.is_contiguous() and q.stride(0) == (Hq + 2 * Hkv) * D
    o = torch.ops.sxe.flash_attn_fwd_varlen(q, k, v, _table(EDGE_LENS), D ** -0.5)
    assert o.shape == (T, Hq, D) and o.dtype == torch.bfloat16 and torch.isfinite(o.float()).all()
    _assert_close(o, _oracle(q, k, v, EDGE_LENS), EDGE_LENS)


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("W", [1, 20, 128, 1000])
def test_sliding_window(W, D):
    from shuffle_exchange_amd.ops.attention import varlen_attention
    lens = [300, 129, 512]
    _, _, (q, k, v) = _packed(sum(lens), 4, 2, D, seed=1)
    o = varlen_attention(q, k, v, _table(lens), window=W)
    _assert_close(o, _oracle(q, k, v, lens, window=W), lens)
    if W >= max(lens):  # a window wider than every sequence is no window
        assert torch.equal(o, varlen_attention(q, k, v, _table(lens)))


@pytest.mark.parametrize("D", [64, 128, 256])
def test_rows_past_the_buffer_are_never_read(D):
    """The buffer is the first T rows of an allocation whose later rows are NaN; the last sequence ends
    at T inside a 128-row block and a 64-key tile. Any Q / K / V fetch at or past row T shows as NaN
    (a masked key's NaN V row poisons P V) or as a difference from the run with those rows zeroed."""
    lens = [128, 77]
    T = sum(lens)
    big, _, (q, k, v) = _packed(T, 4, 2, D, seed=2, extra_rows=256, fill=float("nan"))
    assert torch.isnan(big[T:].float()).all()
    tab = _table(lens)
    o_nan = torch.ops.sxe.flash_attn_fwd_varlen(q, k, v, tab, D ** -0.5)
    o_nan_w = torch.ops.sxe.flash_attn_fwd_varlen(q, k, v, tab, D ** -0.5, 20)  # the windowed tile walk too
    assert torch.isfinite(o_nan.float()).all() and torch.isfinite(o_nan_w.float()).all()
    _assert_close(o_nan, _oracle(q, k, v, lens), lens)
    _assert_close(o_nan_w, _oracle(q, k, v, lens, window=20), lens)
    big[T:] = 0
    assert torch.equal(o_nan, torch.ops.sxe.flash_attn_fwd_varlen(q, k, v, tab, D ** -0.5))
    assert torch.equal(o_nan_w, torch.ops.sxe.flash_attn_fwd_varlen(q, k, v, tab, D ** -0.5, 20))


def test_no_leak_between_sequences_and_no_write_outside_the_table():
    lens, routed, D = [130, 257, 64, 300], [0, 1, 3], 128
    T = sum(lens)
    starts = [sum(lens[:i]) for i in range(len(lens))]
    _, qkv, (q, k, v) = _packed(T, 8, 2, D, seed=3)
    tab = _table(lens, routed)

    def run():
        out = torch.full((T, 8, D), 7.0, device="cuda", dtype=torch.bfloat16)  # sentinel
        r = torch.ops.sxe.flash_attn_fwd_varlen(q, k, v, tab, D ** -0.5, 0, out)
        assert r.data_ptr() == out.data_ptr()
        return out

    a = run()
    _assert_close(a, _oracle(q, k, v, lens), lens, routed)
    s, n = starts[1], lens[1]
    qkv[s:s + n] = torch.randn(n, *qkv.shape[1:], device="cuda").to(torch.bfloat16)  # new tokens for sequence 1
    b = run()
    _assert_close(b, _oracle(q, k, v, lens), lens, routed)
    assert not torch.equal(a[s:s + n], b[s:s + n])
    for i in (0, 3):  # the other routed sequences: bit-identical
        assert torch.equal(a[starts[i]:starts[i] + lens[i]], b[starts[i]:starts[i] + lens[i]]), i
    for o in (a, b):  # the sequence outside the table keeps the sentinel
        assert (o[starts[2]:starts[2] + lens[2]] == 7.0).all()


def test_empty_table_writes_nothing():
    _, _, (q, k, v) = _packed(64, 4, 2, 128)
    out = torch.full((64, 4, 128), 7.0, device="cuda", dtype=torch.bfloat16)
    tab = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    assert torch.ops.sxe.flash_attn_fwd_varlen(q, k, v, tab, 0.1, 0, out).data_ptr() == out.data_ptr()
    assert (out == 7.0).all()


def test_host_checks():
    op = torch.ops.sxe.flash_attn_fwd_varlen
    lens = [130]
    _, _, (q, k, v) = _packed(130, 4, 2, 128)
    tab = _table(lens)
    op(q, k, v, tab, 0.1)
    with pytest.raises(RuntimeError):  # dtype
        op(q.half(), k.half(), v.half(), tab, 0.1)
    with pytest.raises(RuntimeError):  # table dtype
        op(q, k, v, tab.long(), 0.1)
    with pytest.raises(RuntimeError):  # table shape
        op(q, k, v, torch.zeros(2, 4, dtype=torch.int32, device="cuda"), 0.1)
    with pytest.raises(RuntimeError):
        op(q, k, v, tab.reshape(-1), 0.1)
    with pytest.raises(RuntimeError):  # table device
        op(q, k, v, tab.cpu(), 0.1)
    with pytest.raises(RuntimeError):  # head dim
        _, _, (q96, k96, v96) = _packed(130, 4, 2, 96)
        op(q96, k96, v96, tab, 0.1)
    with pytest.raises(RuntimeError):  # misaligned rows
        op(q[:, :, 1:65], k[:, :, 1:65], v[:, :, 1:65], tab, 0.1)
    with pytest.raises(RuntimeError):  # out shape
        op(q, k, v, tab, 0.1, 0, torch.empty(130, 2, 128, device="cuda", dtype=torch.bfloat16))
