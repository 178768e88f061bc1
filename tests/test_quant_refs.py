"""CPU checks of the float64 references in tests/_quant_refs.py: against independent torch builtins
(torch.round, .to(float8_e4m3fn), the CPU paths of ops/quantizer.py, ops/fp_quantizer.py and ops/mx.py)
on random finite data, the non-finite / zero policies of those Python fallbacks, and the condition the
GPU tests (tests/test_quant_kernels_gpu.py) rely on: the tie window flags almost nothing."""
import pytest
import torch

from tests import _quant_refs as R

F32, F64 = torch.float32, torch.float64


def _inexact_ties(r, group):
    """Crafted cases sit ON the half-way points, in groups with s = 1 where t = x and the kernels'
    arithmetic is exact. What must not occur is a flagged element whose quotient is rounded."""
    return r.near_tie & (r.scales.repeat_interleave(group) != 1)


def _equal_nan(a, b):
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ------------------------------------------------------------------------------------------------
# references vs torch builtins, random finite data
# ------------------------------------------------------------------------------------------------
def test_format_tables_from_definition():
    assert R.E2M1.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert len(R.E3M2) == 32 and float(R.E3M2[-1]) == 28.0 and float(R.E3M2[1]) == 0.0625
    assert len(R.E4M3) == 127 and float(R.E4M3[-1]) == 448.0 and float(R.E4M3[1]) == 2.0 ** -9
    # every e4m3fn byte but the two NaN codes decodes to the table
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    assert torch.equal(R.fp8_value(codes), codes.view(torch.float8_e4m3fn).to(F64))


def test_rne_matches_torch_round():
    t = torch.cat([torch.randn(4096, generator=R._gen(1), dtype=F64) * 50, R.crafted_values("int8")])
    assert torch.equal(R._rne(t), torch.round(t))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("group", R.GROUPS)
@pytest.mark.parametrize("bits", [8, 4])
def test_sym_quant_vs_torch_round_and_cpu_path(bits, group, dtype):
    from shuffle_exchange_amd.ops import quantizer as Q
    x = R.rand_case(group, dtype)
    r = R.sym_quant(x, group, bits)
    qmax = R.KINDS[f"int{bits}"]
    assert r.finite.all() and r.codes.abs().max() <= qmax
    assert torch.equal(r.codes, torch.round(r.t).clamp(-qmax, qmax).to(torch.int64))
    pq, ps = Q.quantize(x, group, bits)          # CPU path: fp32 division x / s, torch.round
    assert torch.equal(ps, r.scales)
    pc = R.sym_codes_of(pq, bits)
    diff = pc != r.codes
    assert not (diff & ~r.near_tie).any() and torch.equal(pc[diff], r.alt[diff])
    for od in R.DTYPES:
        want = Q.dequantize(r.packed, r.scales, group, bits, numel=x.numel(), dtype=od)
        got = R.sym_dequant(r.packed, r.scales, group, bits, od)
        if od == F32:
            assert torch.equal(got, want)
        else:   # the CPU path rounds to fp32 first, the reference once
            assert ((got.double() - want.double()).abs() <= torch.finfo(od).eps * want.double().abs()).all()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("group", R.GROUPS)
def test_fp8_quant_vs_torch_float8(group, dtype):
    from shuffle_exchange_amd.ops import quantizer as Q
    x = R.rand_case(group, dtype)
    r = R.fp8_quant(x, group)
    assert r.finite.all() and ((r.codes & 0x7F) <= 126).all()
    # the same float64 quotient through torch's converter (exact in fp32 only near ties: compare off them)
    via = r.t.clamp(-448, 448).to(F32).to(torch.float8_e4m3fn).view(torch.uint8).to(torch.int64)
    diff = via != r.codes
    assert not (diff & ~r.near_tie).any() and torch.equal(via[diff], r.alt[diff])
    pq, ps = Q.quantize_fp8(x, group)            # CPU path
    assert torch.equal(ps, r.scales)
    diff = pq.to(torch.int64) != r.codes
    assert not (diff & ~r.near_tie).any() and torch.equal(pq.to(torch.int64)[diff], r.alt[diff])
    want = Q.dequantize_fp8(r.packed, r.scales, group, dtype=F32)
    assert torch.equal(R.fp8_dequant(r.packed, r.scales, group, F32), want)


def test_fp8_quant_exact_on_every_value_and_midpoint():
    for dtype in R.DTYPES:
        x = R.crafted_case("fp8", 128, dtype)
        r = R.fp8_quant(x, 128)
        assert not _inexact_ties(r, 128).any()
        via = x.to(F32).to(torch.float8_e4m3fn).view(torch.uint8).to(torch.int64)
        unit = r.scales.repeat_interleave(128) == 1
        assert unit.sum() >= x.numel() - 128 and torch.equal(via[unit], r.codes[unit])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("group", R.FPX_GROUPS)
@pytest.mark.parametrize("bits", [4, 6])
def test_fpx_quant_vs_cpu_path(bits, group, dtype):
    from shuffle_exchange_amd.ops.fp_quantizer import FP_Quantize
    x = R.fpx_case(bits, group, dtype)
    r = R.fpx_quant(x, bits, group)
    fq = FP_Quantize(group)
    pq, ps = fq.quantize(x, q_bits=bits, q_mantisa_bits=2 if bits == 6 else 1, return_meta_tensor=True)
    assert torch.equal(ps, r.scales)
    pc = R.fpx_codes_of(pq, bits)
    diff = pc != r.codes
    assert not (diff & ~r.near_tie).any() and torch.equal(pc[diff], r.alt[diff])
    fq.orig_dtype, fq.orig_shape = F32, None
    assert torch.equal(R.fpx_dequant(r.packed, r.scales, bits, group, x.numel(), F32), fq.dequantize(r.packed))
    # exact cases
    kind = "fp4" if bits == 4 else "fp6"
    if group >= 32 and group % 2 == 0:
        c = R.fpx_quant(R.crafted_case(kind, group, dtype), bits, group)
        assert not _inexact_ties(c, group).any()


def test_mx_fp8_block_vs_mx_quantize():
    from shuffle_exchange_amd.ops import mx
    x = (torch.randn(8, 128, generator=R._gen(5)) * torch.logspace(-6, 6, 8)[:, None]).bfloat16()
    x[3, 32:64] = 0
    x[4, 0:32] = torch.tensor([448.0, 224.0, -7.0, 0.4375] * 8).bfloat16()   # amax / 448 an exact power of two
    codes, ex = R.mx_fp8_block(x)
    wq, ws = mx.quantize(x.float(), "mxfp8")
    assert torch.equal(ex, ws) and torch.equal(codes, wq)
    for name, xr in R.mx_range_cases().items():
        assert torch.isfinite(xr.float()).all()
        codes, ex = R.mx_fp8_block(xr)
        back = R.fp8_value(codes) * torch.exp2(ex.to(F64) - 127).repeat_interleave(32, 1)
        # half an e4m3 step of the block's top binade: 16 * 2^e
        assert ((back - xr.to(F64)).abs() <= 16 * torch.exp2(ex.to(F64) - 127).repeat_interleave(32, 1)).all(), name
    assert R.mx_fp8_block(R.mx_range_cases()["min_bf16_subnormal"])[1].eq(0).all()


def test_dequant_reduce_ref_vs_cpu_path():
    from shuffle_exchange_amd.ops import quantizer as Q
    for bits in (8, 4):
        q, s, old = R.reduce_case(bits, 3, 64)
        m = old.numel()
        for acc in (False, True):
            out = old.clone()
            Q.dequant_reduce(q, s, 3, 64, bits, out, alpha=0.125, accumulate=acc)
            ref = R.dequant_reduce(q, s, 3, 64, bits, m, 0.125, old if acc else None)
            # the CPU path sums in fp32: W + 2 roundings of terms no larger than the largest |term|
            big = 3 * 127 * float(s.max()) * 0.125 + float(old.abs().max())
            assert ((out.double() - ref).abs() <= 5 * 2.0 ** -24 * big).all()


def test_onebit_refs():
    x, scale = R.onebit_case(64)
    packed, err = R.sign_pack_ef(x, scale)
    bits = ((packed.to(torch.int64)[:, None] >> torch.arange(8)) & 1).reshape(-1).bool()
    assert bits[1] and bits[2] and not bits[5] and bits[16:32].all() and not bits[40]   # -0.0 positive, NaN negative
    assert torch.isnan(err[5]) and err[1] == -scale and err[2] == -scale
    fin = ~torch.isnan(x)
    assert torch.equal(err[fin], (x - torch.sign(x + (x == 0)) * scale)[fin])
    avg = R.unpack_avg(torch.stack([packed, packed ^ 0xFF, packed]), torch.tensor([1.0, 2.0, 0.5]))
    sg = bits.double() * 2 - 1
    torch.testing.assert_close(avg, sg * (1.0 - 2.0 + 0.5) / 3, rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------
# policies of the Python fallbacks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", R.NONFINITE_POS)
@pytest.mark.parametrize("pattern", list(R.NONFINITE))
def test_cpu_paths_nonfinite_policy(pattern, pos):
    from shuffle_exchange_amd.ops import quantizer as Q
    from shuffle_exchange_amd.ops.fp_quantizer import FP_Quantize
    group = 64
    x, clean = R.nonfinite_case(pattern, pos, group, F32)
    mid = slice(group, 2 * group)

    def check(tag, s, s0, deq, deq0, codes_ok):
        assert not torch.isfinite(s[1]) and torch.isfinite(s[[0, 2]]).all(), tag
        assert not torch.isfinite(deq[mid]).any(), tag
        assert codes_ok, tag
        assert torch.equal(s[[0, 2]], s0[[0, 2]]) and torch.equal(deq[:group], deq0[:group]), tag
        assert torch.equal(deq[2 * group:], deq0[2 * group:]), tag

    for bits in (8, 4):
        (q, s), (q0, s0) = Q.quantize(x, group, bits), Q.quantize(clean, group, bits)
        r = R.sym_quant(x, group, bits)
        assert _equal_nan(s, r.scales) or (not torch.isfinite(s[1]) and not torch.isfinite(r.scales[1]))
        deq = Q.dequantize(q, s, group, bits, dtype=F32)
        deq0 = Q.dequantize(q0, s0, group, bits, dtype=F32)
        check(f"int{bits}", s, s0, deq, deq0, R.sym_codes_of(q, bits).abs().max() <= R.KINDS[f"int{bits}"])
        out = torch.ones(3 * group)
        Q.dequant_reduce(torch.cat([q0, q]), torch.cat([s0, s]), 2, group, bits, out, alpha=0.125, accumulate=True)
        assert not torch.isfinite(out[mid]).any() and torch.isfinite(out[:group]).all()
    (q, s), (q0, s0) = Q.quantize_fp8(x, group), Q.quantize_fp8(clean, group)
    check("fp8", s, s0, Q.dequantize_fp8(q, s, group, dtype=F32), Q.dequantize_fp8(q0, s0, group, dtype=F32),
          ((q & 0x7F) != 0x7F).all())
    for bits in (4, 6):
        fq, f0 = FP_Quantize(group), FP_Quantize(group)
        q = fq.quantize(x, q_bits=bits, q_mantisa_bits=2 if bits == 6 else 1)
        q0 = f0.quantize(clean, q_bits=bits, q_mantisa_bits=2 if bits == 6 else 1)
        check(f"fp{bits}", fq.get_scales(), f0.get_scales(), fq.dequantize(q).float(), f0.dequantize(q0).float(),
              (q < (1 << bits)).all() if bits == 6 else True)


@pytest.mark.parametrize("amax,dtype", R.TINY_CASES, ids=R.TINY_IDS)
def test_cpu_paths_zero_policy(amax, dtype):
    from shuffle_exchange_amd.ops import quantizer as Q
    from shuffle_exchange_amd.ops.fp_quantizer import FP_Quantize
    group = 64
    x, zeros = R.tiny_case(amax, group, dtype)
    assert zeros.sum() >= group // 4
    for bits in (8, 4):
        q, s = Q.quantize(x, group, bits)
        r = R.sym_quant(x, group, bits)
        assert torch.equal(s, r.scales) and (R.sym_codes_of(q, bits)[zeros] == 0).all()
        assert (r.codes[zeros] == 0).all()
        assert (Q.dequantize(q, s, group, bits, dtype=F32)[zeros] == 0).all()
    q, s = Q.quantize_fp8(x, group)
    r = R.fp8_quant(x, group)
    assert torch.equal(s, r.scales) and ((q[zeros] & 0x7F) == 0).all() and ((r.codes[zeros] & 0x7F) == 0).all()
    for bits in (4, 6):
        fq = FP_Quantize(group)
        q = fq.quantize(x, q_bits=bits, q_mantisa_bits=2 if bits == 6 else 1)
        r = R.fpx_quant(x, bits, group)
        assert torch.equal(fq.get_scales(), r.scales)
        assert (R.fpx_codes_of(q, bits)[zeros] == 0).all() and (r.codes[zeros] == 0).all()


# ------------------------------------------------------------------------------------------------
# the tie window flags almost nothing (reference alone)
# ------------------------------------------------------------------------------------------------
def _quant(kind, x, group):
    if kind == "fp8":
        return R.fp8_quant(x, group)
    return R.sym_quant(x, group, 8 if kind == "int8" else 4)


def _cap(dtype):
    return 1e-4 if dtype == F32 else 1e-2


def test_tie_window_caps_random_cases():
    worst = {}
    for kind, group, dtype in R.quant_table():
        r = _quant(kind, R.rand_case(group, dtype), group)
        frac = r.near_tie.double().mean().item()
        worst[dtype] = max(worst.get(dtype, 0.0), frac)
        assert frac <= _cap(dtype), (kind, group, dtype, frac)
    for dtype in R.DTYPES:
        for kind in R.KINDS:
            r = _quant(kind, R.stride_case(dtype), 64)
            frac = r.near_tie.double().mean().item()
            worst[dtype] = max(worst.get(dtype, 0.0), frac)
            assert frac <= _cap(dtype), ("stride", kind, dtype, frac)
    print({R.dtype_id(d): f"{v:.2e}" for d, v in worst.items()})


def _finite_frac(r, group):
    """Share of near_tie among the elements of finite groups (the ones the GPU tests compare)."""
    use = r.finite.repeat_interleave(group)
    return (r.near_tie & use).double().sum().item() / max(int(use.sum()), 1)


def test_tie_window_caps_guard_tiny_nonfinite_reduce_cases():
    """Every other table whose codes the GPU file compares: the guard-buffer inputs, the tiny groups
    (with their neighbours), the finite groups of the non-finite cases, and the data behind the
    dequant_reduce_ chunks."""
    for kind in R.KINDS:
        for dtype in R.DTYPES:
            for group in (64, 192, 320):
                frac = _finite_frac(_quant(kind, R.guard_case(group, dtype), group), group)
                assert frac <= _cap(dtype), ("guard", kind, group, dtype, frac)
            for group in (64, 128):
                for pattern in R.NONFINITE:
                    for pos in R.NONFINITE_POS:
                        x, clean = R.nonfinite_case(pattern, pos, group, dtype)
                        for t in (x, clean):
                            frac = _finite_frac(_quant(kind, t, group), group)
                            assert frac <= _cap(dtype), ("nonfinite", kind, group, dtype, pattern, pos, frac)
        for group in (64, 128):
            for amax, dtype in R.TINY_CASES:
                frac = _finite_frac(_quant(kind, R.tiny_case(amax, group, dtype)[0], group), group)
                assert frac <= _cap(dtype), ("tiny", kind, group, amax, dtype, frac)
    for bits in (4, 6):
        for amax, dtype in R.TINY_CASES:
            frac = _finite_frac(R.fpx_quant(R.tiny_case(amax, 32, dtype)[0], bits, 32), 32)
            assert frac <= _cap(dtype), ("fpx tiny", bits, amax, dtype, frac)
        for dtype in R.DTYPES:
            for pattern in R.NONFINITE:
                for pos in R.NONFINITE_POS:
                    for t in R.nonfinite_case(pattern, pos, 32, dtype):
                        frac = _finite_frac(R.fpx_quant(t, bits, 32), 32)
                        assert frac <= _cap(dtype), ("fpx nonfinite", bits, dtype, pattern, pos, frac)
    for bits in (8, 4):
        for W in R.REDUCE_W:
            for group in R.REDUCE_GROUPS:
                for x in R.reduce_inputs(bits, W, group):
                    frac = _finite_frac(R.sym_quant(x, group, bits), group)
                    assert frac <= _cap(F32), ("reduce", bits, W, group, frac)
        for x in R.reduce_inputs(bits, 2, 64, seed=5, m=R.STRIDE_GROUPS * 64):
            assert _finite_frac(R.sym_quant(x, 64, bits), 64) <= _cap(F32), ("reduce stride", bits)


def test_tie_window_caps_fpx_cases():
    for bits in (4, 6):
        for dtype in R.DTYPES:
            for group in R.FPX_GROUPS:
                x = R.fpx_case(bits, group, dtype)
                # a group's own amax sits on +-fmax exactly; everything else must be clear of the midpoints
                frac = R.fpx_quant(x, bits, group).near_tie.double().mean().item()
                assert frac <= _cap(dtype), (bits, group, dtype, frac)
            frac = R.fpx_quant(R.fpx_stride_case(dtype), bits, 32).near_tie.double().mean().item()
            assert frac <= _cap(dtype), ("stride", bits, dtype, frac)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
def test_crafted_cases_have_no_near_tie(dtype):
    for kind in R.KINDS:
        r = _quant(kind, R.crafted_case(kind, 128, dtype), 128)
        assert not _inexact_ties(r, 128).any(), kind
        # the body groups have s = 1: the codes are the values' own roundings
        assert (r.scales[:-2] == 1).all() and r.scales[-2] == 1
    for kind, bits in (("fp4", 4), ("fp6", 6)):
        r = R.fpx_quant(R.crafted_case(kind, 128, dtype), bits, 128)
        assert not _inexact_ties(r, 128).any() and (r.scales[:-2] == 1).all()
