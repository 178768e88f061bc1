"""Exact tests of the quantize kernels (quant.hip: int8 / int4 / FP8 group quantizers, their
dequantizers and dequant_reduce_; the FP6 / FP4 group pair of mxfp.hip; onebit.hip; the range ends of
mx_quant_fp8) against the float64 references of tests/_quant_refs.py.

  * scales: torch.equal (one IEEE fp32 division of identical operands on both sides);
  * codes: equal to the reference wherever ``near_tie`` is false; where it is true the reference's code
    or the one across that tie; crafted cases (s = 1, inputs ON the half-way points) equal everywhere;
    int4 / FP4 nibble by nibble; every byte of the returned tensor is accounted for;
  * dequantizers: torch.equal for fp32 output, <= 1 ulp of a 16-bit output (fp32 product, then the
    cast: two roundings against the reference's one);
  * round trip: |dequant(quant(x)) - x| <= s * (half the widest code step at the element) + |x| 2^-22
    for finite groups with a normal scale -- s/2 for the integer kinds;
  * zero and non-finite policies as documented in quant.hip;
  * dequant_reduce_: |kernel - ref| <= 2 max|fp32 baseline - ref| + 1 ulp, summation order being the only
    freedom;
  * onebit: bits and err exact, unpack_avg within W ulp.
One ``[quant-edge]`` line per case; profiles/quant_kernel_edges.log is a GPU run of this file.
"""
import pytest
import torch

from tests import _quant_refs as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
SENTINEL = 3.0e4       # finite in every dtype, far above any case's amax


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from shuffle_exchange_amd.ops import native
    native.require_hip()


def _ops():
    return torch.ops.sxe


def _log(msg):
    print(f"[quant-edge] {msg}")


def _ulp(ref, dtype):
    fi = torch.finfo(dtype)
    a = ref.abs().clamp_min(fi.tiny)
    return torch.exp2(torch.floor(torch.log2(a))) * fi.eps


def _same(a, b):
    """Equal, NaN matching NaN (and -0.0 == +0.0)."""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ------------------------------------------------------------------------------------------------
# the three group quantizers of quant.hip behind one face
# ------------------------------------------------------------------------------------------------
def _bits(kind):
    return {"int8": 8, "int4": 4}.get(kind)


def _gpu_quant(kind, x, group):
    if kind == "fp8":
        q, s = _ops().quantize_fp8(x, group)
    else:
        q, s = _ops().quantize_sym(x, group, _bits(kind))
    return q, s


def _ref_quant(kind, x, group):
    return R.fp8_quant(x, group) if kind == "fp8" else R.sym_quant(x, group, _bits(kind))


def _codes_of(kind, packed):
    return packed.to(torch.int64) if kind == "fp8" else R.sym_codes_of(packed, _bits(kind))


def _pack(kind, codes):
    if kind == "int4":
        return R._pack_nibbles(codes)
    return codes.to(torch.uint8) if kind == "fp8" else codes.to(torch.int8).view(torch.uint8)


def _gpu_dequant(kind, q, s, group, n, dtype):
    out = torch.full((n,), 7.0, dtype=dtype, device=DEV)
    if kind == "fp8":
        _ops().dequantize_fp8_(q, s, group, out)
    else:
        _ops().dequantize_sym_(q, s, group, _bits(kind), out)
    return out


def _ref_dequant(kind, packed, s, group, dtype):
    if kind == "fp8":
        return R.fp8_dequant(packed, s, group, dtype)
    return R.sym_dequant(packed, s, group, _bits(kind), dtype)


def _half_step(kind, codes):
    """Half the widest gap between a code's value and its neighbours, in units of the scale."""
    if kind != "fp8":
        return torch.full(codes.shape, 0.5, dtype=F64)
    i = (codes & 0x7F).clamp(max=126)
    up = R.E4M3[(i + 1).clamp(max=126)] - R.E4M3[i]
    dn = R.E4M3[i] - R.E4M3[(i - 1).clamp(min=0)]
    return torch.maximum(up, dn) / 2


def _check_quant(tag, kind, x, group, exact=False):
    """Quantize x (CPU tensor) on the GPU and hold scales, codes and every byte of the finite groups
    against the reference. -> (q, s, ref), on the CPU."""
    n = x.numel()
    q, s = _gpu_quant(kind, x.to(DEV), group)
    assert q.dtype == torch.uint8 and q.numel() == (n // 2 if kind == "int4" else n) and q.is_contiguous()
    assert s.dtype == F32 and s.numel() == n // group
    q, s = q.cpu(), s.cpu()
    ref = _ref_quant(kind, x, group)
    use_g = ref.finite
    use = use_g.repeat_interleave(group)
    assert torch.equal(s[use_g], ref.scales[use_g]), f"{tag}: scales differ from the fp32 division"
    got = _codes_of(kind, q)
    diff = (got != ref.codes) & use
    tie_taken = diff & ref.near_tie & (got == ref.alt)
    wrong = diff & ~tie_taken
    if exact:
        wrong = diff
    _log(f"{tag} kind={kind} group={group} in={R.dtype_id(x.dtype)} n={n} near_tie={int((ref.near_tie & use).sum())} "
         f"tie_alt_taken={int(tie_taken.sum())} wrong={int(wrong.sum())} scales_equal=True")
    assert not wrong.any(), (f"{tag}: {int(wrong.sum())} wrong codes, first at {int(wrong.nonzero()[0])}: "
                             f"got {int(got[wrong][0])} want {int(ref.codes[wrong][0])} (t = {float(ref.t[wrong][0])!r})")
    # no stray bytes: the whole returned tensor is the reference packing (with the ties as taken)
    want = torch.where(tie_taken, ref.alt, ref.codes)
    want = torch.where(use, want, got)
    assert torch.equal(q, _pack(kind, want)), f"{tag}: bytes differ from the reference packing"
    return q, s, ref


def _check_roundtrip(tag, kind, x, group, q, s, ref):
    """dequantize the kernel's own output (fp32) and bound the error per element."""
    n = x.numel()
    deq = _gpu_dequant(kind, q.to(DEV), s.to(DEV), group, n, F32).cpu()
    assert torch.equal(deq[ref.finite.repeat_interleave(group)],
                       _ref_dequant(kind, q, s, group, F32)[ref.finite.repeat_interleave(group)])
    normal = (ref.finite & (ref.scales >= torch.finfo(F32).tiny)).repeat_interleave(group)
    sc = ref.scales.to(F64).repeat_interleave(group)
    err = (deq.to(F64) - x.to(F64)).abs()
    bound = sc * _half_step(kind, _codes_of(kind, q)) + x.to(F64).abs() * 2.0 ** -22
    worst = (err / bound.clamp_min(1e-300))[normal].max().item() if normal.any() else 0.0
    _log(f"{tag} roundtrip kind={kind} worst_over_bound={worst:.4f}")
    assert (err <= bound)[normal].all(), f"{tag}: round trip over the bound ({worst:.4f})"
    zero = (x == 0) & ref.finite.repeat_interleave(group)
    assert ((_codes_of(kind, q) & (0x7F if kind == "fp8" else -1))[zero] == 0).all() and (deq[zero] == 0).all()


def _check_dequant(tag, kind, packed, s, group):
    """The dequantizer on reference codes and scales, for the three output dtypes."""
    n = s.numel() * group
    for od in R.DTYPES:
        out = _gpu_dequant(kind, packed.to(DEV), s.to(DEV), group, n, od).cpu()
        if od == F32:
            ok = _same(out, _ref_dequant(kind, packed, s, group, F32))
            _log(f"{tag} dequant kind={kind} out=float32 n={n} equal={ok}")
            assert ok, f"{tag}: fp32 dequant differs from code * s"
        else:
            r64 = _ref_dequant(kind, packed, s, group, F64)
            fin = torch.isfinite(r64) & (r64.abs() <= torch.finfo(od).max)
            e = ((out.to(F64) - r64).abs() / _ulp(r64, od))[fin].max().item() if fin.any() else 0.0
            _log(f"{tag} dequant kind={kind} out={R.dtype_id(od)} n={n} max_ulp={e:.3f}")
            assert e <= 1.0, f"{tag}: {R.dtype_id(od)} dequant {e:.3f} ulp off"
            assert not torch.isfinite(out[torch.isnan(r64)]).any()


# ================================================================================================
# quantize_sym / quantize_fp8 and their dequantizers
# ================================================================================================
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("group", R.GROUPS)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_quantize_groups(kind, group, dtype):
    """Every group size class: a lane's share odd (64, 192, 320: five groups) and even."""
    x = R.rand_case(group, dtype)
    tag = f"rand g={group}"
    q, s, ref = _check_quant(tag, kind, x, group)
    _check_roundtrip(tag, kind, x, group, q, s, ref)
    _check_dequant(tag, kind, ref.packed, ref.scales, group)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("group", [64, 192, 320])
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_quantize_odd_share_inside_guard_buffer(kind, group, dtype):
    """The input is a slice that ends inside a larger buffer filled with a sentinel (and starts at an
    odd element of it): nothing past the slice may be read into a code, nothing of the guard written.
    Only the input can be guarded: quantize_sym / quantize_fp8 allocate ``q`` themselves, so a write
    past the end of ``q`` cannot be observed through this API. That no such write exists rests on the
    kernels' indexing (every store is inside the lane's own group) and on every byte of ``q`` and
    every neighbouring group being checked here and in test_quantize_groups."""
    x = R.guard_case(group, dtype)
    n = x.numel()
    buf = torch.full((n + 2 * group + 1,), SENTINEL, dtype=dtype)
    buf[1:1 + n] = x
    dbuf = buf.to(DEV)
    xs = dbuf[1:1 + n]
    q, s = _gpu_quant(kind, xs, group)
    torch.cuda.synchronize()
    assert torch.equal(dbuf.cpu(), buf), "guard buffer or input modified"
    ref = _ref_quant(kind, x, group)
    assert torch.equal(s.cpu(), ref.scales)
    got = _codes_of(kind, q.cpu())
    diff = got != ref.codes
    ok = not (diff & ~(ref.near_tie & (got == ref.alt))).any()
    _log(f"guard g={group} kind={kind} in={R.dtype_id(dtype)} n={n} mismatches={int(diff.sum())} ok={ok}")
    assert ok, f"wrong codes at {diff.nonzero().flatten()[:8].tolist()} (last element is {n - 1})"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_quantize_crafted_exact(kind, dtype):
    """amax exactly qmax (s = 1): every half-way point, both signs, +-qmax, every representable value,
    an all-zero group with a -0.0, a group whose only non-zero value is negative. No tie window."""
    x = R.crafted_case(kind, 128, dtype)
    q, s, ref = _check_quant("crafted", kind, x, 128, exact=True)
    assert (s[:-2] == 1).all() and s[-2] == 1 and s[-1] == torch.tensor(3.0) / R.KINDS[kind]
    _check_roundtrip("crafted", kind, x, 128, q, s, ref)
    codes = _codes_of(kind, q)
    if kind == "fp8":
        assert codes[-256 + 3] == 0x80 and (codes[-256:-128] & 0x7F).eq(0).all()      # -0.0 keeps its sign bit
        assert codes[-128 + 64] == 0x80 | 126
    else:
        assert codes[-256:-128].eq(0).all() and codes[-128 + 64] == -R.KINDS[kind]
    _check_dequant("crafted", kind, ref.packed, ref.scales, 128)


@pytest.mark.parametrize("dtype", [torch.bfloat16, F32], ids=R.dtype_id)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_quantize_grid_stride(kind, dtype):
    """8208 groups of 64 > the 8192 waves of a launch: a wave's second group; 525,312 elements > the
    524,288 threads of the elementwise dequantizers."""
    x = R.stride_case(dtype)
    q, s, ref = _check_quant("stride", kind, x, 64)
    _check_roundtrip("stride", kind, x, 64, q, s, ref)
    _check_dequant("stride", kind, ref.packed, ref.scales, 64)


@pytest.mark.parametrize("amax,dtype", R.TINY_CASES, ids=R.TINY_IDS)
@pytest.mark.parametrize("group", [64, 128])
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_quantize_tiny_groups_keep_zeros(kind, group, amax, dtype):
    """A group whose scale is subnormal (1/s overflows below about qmax * 2^-128) or underflows to
    zero: exact zeros must still get code 0, the other codes must still be the reference's."""
    x, zeros = R.tiny_case(amax, group, dtype)
    q, s, ref = _check_quant(f"tiny amax={amax:.3e}", kind, x, group)
    codes = _codes_of(kind, q)
    assert ((codes & (0x7F if kind == "fp8" else -1))[zeros] == 0).all(), "an exact zero did not get code 0"
    deq = _gpu_dequant(kind, q.to(DEV), s.to(DEV), group, x.numel(), F32).cpu()
    assert (deq[zeros] == 0).all()
    assert _same(deq, _ref_dequant(kind, q, s, group, F32))


@pytest.mark.parametrize("pattern", list(R.NONFINITE))
@pytest.mark.parametrize("group", [64, 128])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_quantize_nonfinite_groups(kind, dtype, group, pattern):
    """NaN / +-Inf in the middle group of three, at the first, last and a middle element: that group
    gets a non-finite scale and dequantizes to non-finite values everywhere, its codes stay in range,
    and the neighbours are bit-equal to the same input with that group zeroed."""
    mid = slice(group, 2 * group)
    for pos in R.NONFINITE_POS:
        x, clean = R.nonfinite_case(pattern, pos, group, dtype)
        tag = f"nonfinite {pattern}@{pos} g={group}"
        q, s, ref = _check_quant(tag, kind, x, group)
        q0, s0 = (t.cpu() for t in _gpu_quant(kind, clean.to(DEV), group))
        assert not torch.isfinite(s[1]) and not ref.finite[1], f"{tag}: scale {float(s[1])} is finite"
        assert torch.equal(s[[0, 2]], s0[[0, 2]])
        codes, codes0 = _codes_of(kind, q), _codes_of(kind, q0)
        assert torch.equal(codes[:group], codes0[:group]) and torch.equal(codes[2 * group:], codes0[2 * group:])
        if kind == "fp8":
            assert ((codes[mid] & 0x7F) <= 126).all(), f"{tag}: NaN code emitted"
        else:
            assert (codes[mid].abs() <= R.KINDS[kind]).all(), f"{tag}: code out of range"
        for od in R.DTYPES:
            deq = _gpu_dequant(kind, q.to(DEV), s.to(DEV), group, x.numel(), od).cpu()
            assert not torch.isfinite(deq[mid]).any(), f"{tag}: finite value out of a non-finite group"
            assert torch.isfinite(deq[:group]).all() and torch.isfinite(deq[2 * group:]).all()
        if kind != "fp8":   # through the fused reduce: any W, alpha, accumulate
            m = x.numel()
            for W, alpha, acc in ((1, 1.0, False), (3, 0.125, True), (2, 1.0, True)):
                qq = torch.cat([q0] * (W - 1) + [q]).to(DEV)
                ss = torch.cat([s0] * (W - 1) + [s]).to(DEV)
                out = torch.ones(m, device=DEV)
                _ops().dequant_reduce_(qq, ss, W, group, _bits(kind), out, alpha, acc)
                out = out.cpu()
                assert not torch.isfinite(out[mid]).any(), f"{tag}: dequant_reduce_ W={W} hid the group"
                assert torch.isfinite(out[:group]).all() and torch.isfinite(out[2 * group:]).all()


# ================================================================================================
# dequant_reduce_
# ================================================================================================
def _check_reduce(tag, bits, W, group, q, s, old, alpha, acc):
    m = old.numel()
    out = old.clone().to(DEV)
    _ops().dequant_reduce_(q.to(DEV), s.to(DEV), W, group, bits, out, alpha, acc)
    out = out.cpu()
    ref = R.dequant_reduce(q, s, W, group, bits, m, alpha, old if acc else None)
    base = R.dequant_reduce(q, s, W, group, bits, m, alpha, old if acc else None, dt=F32)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(out), fin), f"{tag}: finiteness differs"
    eb = (base.to(F64) - ref)[fin].abs().max()
    ek = (out.to(F64) - ref).abs()
    bound = 2.0 * eb + _ulp(ref, F32)
    worst = (ek / bound)[fin].max().item()
    _log(f"{tag} bits={bits} W={W} group={group} alpha={alpha} accumulate={acc} m={m} base_max={eb.item():.3e} "
         f"kern_max={ek[fin].max().item():.3e} worst_over_bound={worst:.3f}")
    assert (ek <= bound)[fin].all(), f"{tag}: over the bound ({worst:.3f})"


@pytest.mark.parametrize("acc", [False, True], ids=["assign", "accumulate"])
@pytest.mark.parametrize("group", R.REDUCE_GROUPS)
@pytest.mark.parametrize("W", R.REDUCE_W)
@pytest.mark.parametrize("bits", [8, 4])
def test_dequant_reduce(bits, W, group, acc):
    for alpha in R.REDUCE_ALPHA:
        q, s, old = R.reduce_case(bits, W, group)
        _check_reduce("reduce", bits, W, group, q, s, old, alpha, acc)
        # one worker's second group carries a non-finite scale
        ng = old.numel() // group
        for bad in (R.NAN, R.INF):
            s2 = s.clone()
            s2[(W - 1) * ng + 1] = bad
            _check_reduce(f"reduce scale={bad}", bits, W, group, q, s2, old, alpha, acc)


@pytest.mark.parametrize("bits", [8, 4])
def test_dequant_reduce_grid_stride(bits):
    q, s, old = R.reduce_case(bits, 2, 64, seed=5, m=R.STRIDE_GROUPS * 64)
    _check_reduce("reduce stride", bits, 2, 64, q, s, old, 0.125, True)


# ================================================================================================
# FP6 / FP4 group quantizer (mxfp.hip)
# ================================================================================================
def _check_fpx(tag, bits, group, x, exact=False):
    n = x.numel()
    q, s = _ops().fpx_quantize(x.to(DEV), bits, group)
    assert q.dtype == torch.uint8 and q.numel() == (n // 2 if bits == 4 else n) and s.numel() == n // group
    q, s = q.cpu(), s.cpu()
    ref = R.fpx_quant(x, bits, group)
    use = ref.finite.repeat_interleave(group)
    assert torch.equal(s[ref.finite], ref.scales[ref.finite]), f"{tag}: scales"
    got = R.fpx_codes_of(q, bits)
    diff = (got != ref.codes) & use
    tie_taken = diff & ref.near_tie & (got == ref.alt)
    wrong = diff if exact else diff & ~tie_taken
    _log(f"{tag} fp{bits} group={group} in={R.dtype_id(x.dtype)} n={n} near_tie={int((ref.near_tie & use).sum())} "
         f"tie_alt_taken={int(tie_taken.sum())} wrong={int(wrong.sum())}")
    assert not wrong.any(), f"{tag}: wrong codes at {wrong.nonzero().flatten()[:8].tolist()}"
    want = torch.where(use, torch.where(tie_taken, ref.alt, ref.codes), got)
    assert torch.equal(q, R._pack_nibbles(want) if bits == 4 else want.to(torch.uint8))
    zero = (x == 0) & use
    assert (got[zero] == 0).all()
    return q, s, ref


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("group", R.FPX_GROUPS)
@pytest.mark.parametrize("bits", [4, 6])
def test_fpx_quantize_dequantize(bits, group, dtype):
    x = R.fpx_case(bits, group, dtype)
    n = x.numel()
    q, s, ref = _check_fpx("fpx", bits, group, x)
    for od in R.DTYPES:
        for nn in (n, n - 2):        # n smaller than scales.numel() * group
            out = _ops().fpx_dequantize(ref.packed.to(DEV), ref.scales.to(DEV), bits, group, nn, od).cpu()
            assert out.dtype == od and out.numel() == nn
            r64 = R.fpx_dequant(ref.packed, ref.scales, bits, group, nn, F64)
            if od == F32:
                assert torch.equal(out, r64.to(F32)), "fp32 dequant differs from value * s"
            else:
                e = ((out.to(F64) - r64).abs() / _ulp(r64, od)).max().item()
                assert e <= 1.0, f"{R.dtype_id(od)} dequant {e:.3f} ulp off"
    _log(f"fpx dequant fp{bits} group={group} n={n} and n-2: fp32 equal, 16-bit <= 1 ulp")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("bits", [4, 6])
def test_fpx_crafted_exact(bits, dtype):
    """s = 1 with an input on every midpoint (ties go to the smaller magnitude), every representable
    value, +-fmax, an all-zero group and a group whose only non-zero value is negative."""
    _check_fpx("fpx crafted", bits, 128, R.crafted_case("fp4" if bits == 4 else "fp6", 128, dtype), exact=True)


@pytest.mark.parametrize("amax,dtype", R.TINY_CASES, ids=R.TINY_IDS)
@pytest.mark.parametrize("bits", [4, 6])
def test_fpx_tiny_groups_keep_zeros(bits, amax, dtype):
    x, zeros = R.tiny_case(amax, 32, dtype)
    q, s, ref = _check_fpx(f"fpx tiny amax={amax:.3e}", bits, 32, x)
    assert (R.fpx_codes_of(q, bits)[zeros] == 0).all()
    deq = _ops().fpx_dequantize(q.to(DEV), s.to(DEV), bits, 32, x.numel(), F32).cpu()
    assert (deq[zeros] == 0).all()


@pytest.mark.parametrize("pattern", list(R.NONFINITE))
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("bits", [4, 6])
def test_fpx_nonfinite_groups(bits, dtype, pattern):
    group = 32
    mid = slice(group, 2 * group)
    for pos in R.NONFINITE_POS:
        x, clean = R.nonfinite_case(pattern, pos, group, dtype)
        q, s, ref = _check_fpx(f"fpx nonfinite {pattern}@{pos}", bits, group, x)
        q0, s0 = (t.cpu() for t in _ops().fpx_quantize(clean.to(DEV), bits, group))
        assert not torch.isfinite(s[1]) and torch.equal(s[[0, 2]], s0[[0, 2]])
        c, c0 = R.fpx_codes_of(q, bits), R.fpx_codes_of(q0, bits)
        assert torch.equal(c[:group], c0[:group]) and torch.equal(c[2 * group:], c0[2 * group:])
        assert (c[mid] < (1 << bits)).all()
        deq = _ops().fpx_dequantize(q.to(DEV), s.to(DEV), bits, group, x.numel(), F32).cpu()
        assert not torch.isfinite(deq[mid]).any() and torch.isfinite(deq[:group]).all()
        assert torch.isfinite(deq[2 * group:]).all()


@pytest.mark.parametrize("bits", [4, 6])
def test_fpx_grid_stride(bits):
    """16400 groups of 32 > 4096 blocks x 4 waves; 524,800 elements > the dequantizer's 524,288 threads."""
    x = R.fpx_stride_case(torch.bfloat16)
    q, s, ref = _check_fpx("fpx stride", bits, 32, x)
    out = _ops().fpx_dequantize(ref.packed.to(DEV), ref.scales.to(DEV), bits, 32, x.numel(), F32).cpu()
    assert torch.equal(out, R.fpx_dequant(ref.packed, ref.scales, bits, 32, x.numel(), F32))


# ================================================================================================
# onebit
# ================================================================================================
@pytest.mark.parametrize("n", R.ONEBIT_N)
def test_onebit_sign_pack_and_unpack(n):
    x, scale = R.onebit_case(n)
    r_packed, r_err = R.sign_pack_ef(x, scale)
    err = torch.full((n,), 9.0, device=DEV)
    packed = torch.full((n // 8,), 0x5A, dtype=torch.uint8, device=DEV)
    _ops().sign_pack_ef_(x.to(DEV), err, scale.to(DEV), packed)
    ok_b, ok_e = torch.equal(packed.cpu(), r_packed), _same(err.cpu(), r_err)
    _log(f"onebit n={n} bytes={n // 8} bits_equal={ok_b} err_equal={ok_e}")
    assert ok_b and ok_e
    g = R._gen(n % 97)
    for W in (1, 3):
        big = torch.randint(0, 256, (W + 2, n // 8), generator=g, dtype=torch.uint8)
        big[1] = r_packed
        scales = torch.tensor([0.7, 2.0, 0.3])[:W]
        rows = big.to(DEV)[1:1 + W]              # a row slice of a larger buffer
        assert rows.is_contiguous() and rows.storage_offset() > 0
        out = torch.full((n,), 9.0, device=DEV)
        _ops().unpack_avg(rows, scales.to(DEV), out)
        ref = R.unpack_avg(big[1:1 + W], scales)
        e = ((out.cpu().to(F64) - ref).abs() / _ulp(ref, F32)).max().item()
        _log(f"onebit unpack_avg n={n} W={W} max_ulp={e:.3f} bound={W}")
        assert e <= W


# ================================================================================================
# mx_quant_fp8 at the ends of the bf16 range
# ================================================================================================
@pytest.mark.parametrize("name", ["max_bf16", "min_bf16_subnormal"])
def test_mx_quant_fp8_range_ends(name):
    x = R.mx_range_cases()[name]
    q, s = _ops().mx_quant_fp8(x.to(DEV))
    codes, ex = R.mx_fp8_block(x)
    _log(f"mx_quant_fp8 {name} exponents kernel={s.cpu().flatten().tolist()} ref={ex.flatten().tolist()} "
         f"codes_equal={torch.equal(q.cpu(), codes)}")
    assert torch.equal(s.cpu(), ex) and torch.equal(q.cpu(), codes)


# ================================================================================================
# host checks
# ================================================================================================
def test_quantize_host_checks_raise():
    ops = _ops()
    x = torch.zeros(384, device=DEV, dtype=torch.bfloat16)
    for fn in (lambda t, g: ops.quantize_sym(t, g, 8), lambda t, g: ops.quantize_fp8(t, g)):
        with pytest.raises(RuntimeError, match="group size must be a positive multiple of 64"):
            fn(x, 0)
        with pytest.raises(RuntimeError, match="group size must be a positive multiple of 64"):
            fn(x, 96)
        with pytest.raises(RuntimeError, match="numel must be a multiple of the group size"):
            fn(x, 256)
        with pytest.raises(RuntimeError, match="contiguous input"):
            fn(torch.zeros(384, 2, device=DEV, dtype=torch.bfloat16)[:, 0], 128)
    with pytest.raises(RuntimeError, match="bits must be 4 or 8"):
        ops.quantize_sym(x, 128, 3)
    with pytest.raises(RuntimeError, match="even group_size"):
        ops.fpx_quantize(x, 4, 3)
    with pytest.raises(RuntimeError, match="bits 4"):
        ops.fpx_quantize(x, 5, 32)
    with pytest.raises(RuntimeError, match="contiguous input"):
        ops.fpx_quantize(torch.zeros(384, 2, device=DEV)[:, 0], 4, 32)


def test_dequantize_host_checks_raise():
    ops = _ops()
    n, group = 384, 128
    q8 = torch.zeros(n, dtype=torch.uint8, device=DEV)
    q4 = torch.zeros(n // 2, dtype=torch.uint8, device=DEV)
    s = torch.ones(n // group, device=DEV)
    out = torch.zeros(n, device=DEV)
    bad = [
        ("bits must be 4 or 8", lambda: ops.dequantize_sym_(q8, s, group, 3, out)),
        ("size mismatch", lambda: ops.dequantize_sym_(q8[:-1], s, group, 8, out)),
        ("size mismatch", lambda: ops.dequantize_sym_(q8, s, group, 4, out)),
        ("size mismatch", lambda: ops.dequantize_sym_(q4, s[:-1], group, 4, out)),
        ("q must be contiguous uint8", lambda: ops.dequantize_sym_(q8.to(torch.int32), s, group, 8, out)),
        ("q must be contiguous uint8", lambda: ops.dequantize_sym_(torch.zeros(n, 2, dtype=torch.uint8, device=DEV)[:, 0], s, group, 8, out)),
        ("scales must be contiguous fp32", lambda: ops.dequantize_sym_(q8, s.double(), group, 8, out)),
        ("scales must be contiguous fp32", lambda: ops.dequantize_sym_(q8, torch.ones(3, 2, device=DEV)[:, 0], group, 8, out)),
        ("out must be a contiguous", lambda: ops.dequantize_sym_(q8, s, group, 8, torch.zeros(n, 2, device=DEV)[:, 0])),
        ("size mismatch", lambda: ops.dequantize_fp8_(q8[:-1], s, group, out)),
        ("size mismatch", lambda: ops.dequantize_fp8_(q8, s[:-1], group, out)),
        ("q must be contiguous uint8", lambda: ops.dequantize_fp8_(q8.to(torch.int8), s, group, out)),
        ("scales must be contiguous fp32", lambda: ops.dequantize_fp8_(q8, s.half(), group, out)),
        ("group must be positive", lambda: ops.dequantize_fp8_(q8, s, 0, out)),
    ]
    for msg, call in bad:
        with pytest.raises(RuntimeError, match=msg):
            call()


def test_dequant_reduce_host_checks_raise():
    ops = _ops()
    W, m, group = 2, 384, 128
    q8 = torch.zeros(W * m, dtype=torch.uint8, device=DEV)
    q4 = torch.zeros(W * m // 2, dtype=torch.uint8, device=DEV)
    s = torch.ones(W * m // group, device=DEV)
    out = torch.zeros(m, device=DEV)
    bad = [
        ("bits must be 4 or 8", lambda: ops.dequant_reduce_(q8, s, W, group, 3, out, 1.0, False)),
        ("bits must be 4 or 8", lambda: ops.dequant_reduce_(q4, s, W, group, 2, out, 1.0, False)),
        ("q must hold W chunks", lambda: ops.dequant_reduce_(q8[:-1], s, W, group, 8, out, 1.0, False)),
        ("q must hold W chunks", lambda: ops.dequant_reduce_(q4, s, W, group, 8, out, 1.0, False)),   # short q: read out of bounds before
        ("q must hold W chunks", lambda: ops.dequant_reduce_(q8, s, W, group, 4, out, 1.0, False)),
        ("q must be contiguous uint8", lambda: ops.dequant_reduce_(q8.to(torch.int8), s, W, group, 8, out, 1.0, False)),
        ("scales size", lambda: ops.dequant_reduce_(q8, s[:-1], W, group, 8, out, 1.0, False)),
        ("scales size", lambda: ops.dequant_reduce_(q8, s, W, 256, 8, out, 1.0, False)),
        ("scales must be contiguous fp32", lambda: ops.dequant_reduce_(q8, s.double(), W, group, 8, out, 1.0, False)),
        ("out must be fp32", lambda: ops.dequant_reduce_(q8, s, W, group, 8, out.bfloat16(), 1.0, False)),
        ("out must be a contiguous", lambda: ops.dequant_reduce_(q8, s, W, group, 8, torch.zeros(m, 2, device=DEV)[:, 0], 1.0, False)),
        ("W and group must be positive", lambda: ops.dequant_reduce_(q8, s, W, 0, 8, out, 1.0, False)),
    ]
    for msg, call in bad:
        with pytest.raises(RuntimeError, match=msg):
            call()


def test_onebit_and_fpx_dequant_host_checks_raise():
    ops = _ops()
    x = torch.zeros(20, device=DEV)
    with pytest.raises(RuntimeError, match="sizes"):
        ops.sign_pack_ef_(x, torch.zeros_like(x), torch.ones(1, device=DEV), torch.zeros(2, dtype=torch.uint8, device=DEV))
    x = torch.zeros(16, device=DEV)
    with pytest.raises(RuntimeError, match="sizes"):
        ops.sign_pack_ef_(x, torch.zeros_like(x), torch.ones(1, device=DEV), torch.zeros(3, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="fp32 contiguous"):
        ops.sign_pack_ef_(x.half(), torch.zeros_like(x), torch.ones(1, device=DEV), torch.zeros(2, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="sizes"):
        ops.unpack_avg(torch.zeros(2, 2, dtype=torch.uint8, device=DEV), torch.ones(3, device=DEV), x)
    q = torch.zeros(32, dtype=torch.uint8, device=DEV)
    s = torch.ones(2, device=DEV)
    with pytest.raises(RuntimeError, match="fpx_dequantize: sizes"):
        ops.fpx_dequantize(q, s, 6, 32, 96, F32)
    with pytest.raises(RuntimeError, match="uint8 codes, fp32 scales"):
        ops.fpx_dequantize(q, s.double(), 6, 32, 32, F32)
    with pytest.raises(RuntimeError, match="bits 4 or 6"):
        ops.fpx_dequantize(q, s, 8, 32, 32, F32)
