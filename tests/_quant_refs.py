"""Plain float64 references for the quantize kernels (quant.hip, the group quantizer of mxfp.hip,
onebit.hip, mx_quant_fp8) and the case tables their tests share.

Plain torch on the CPU, no import of the ops under test. A reference takes the tensor the kernel sees
(already rounded to the test dtype). The only fp32 step of a group quantizer is its scale,
``s = fp32(amax) / qmax`` -- one IEEE division of identical operands on both sides, so scales are
compared with torch.equal. Everything after it (``t = x / s``, the rounding, the packing) is exact
float64 / integer arithmetic.

Policies the references define (and the kernels and the Python fallbacks follow):
  * NaN or +-Inf anywhere in a group -> a non-finite scale (NaN wins over Inf);
  * a group whose ``amax / qmax`` is zero (all zeros, or an fp32 underflow) -> scale 1, all codes 0;
  * an exactly-zero input of a finite group -> magnitude code 0.

``near_tie`` marks the elements whose exact quotient ``t`` is so close to a rounding boundary that the
kernel's fp32 quotient may land on its other side; there the kernel may return ``alt``, the code on
the other side of that boundary. The int / FP8 kernels form ``x * rn(1 / s)`` in fp32 (1/s, the
product: at most 3 half-ulps from t; the window is 4 * 2^-24 * max(|t|, 1)); the FP6 / FP4 kernel
divides, so its quotient is the correctly rounded t (window 2^-23 * |t|).
"""
import itertools
from types import SimpleNamespace

import torch

F64 = torch.float64
F32 = torch.float32
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
KINDS = {"int8": 127.0, "int4": 7.0, "fp8": 448.0}
NAN, INF = float("nan"), float("inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dtype_id(d):
    return str(d).replace("torch.", "")


# ------------------------------------------------------------------------------------------------
# formats
# ------------------------------------------------------------------------------------------------
def float_table(ebits, mbits, reserved_top=0):
    """Magnitudes of the codes 0 .. 2^(e+m) - 1 - reserved_top of a small float format, from its
    definition: subnormals m/2^mb * 2^(1-bias), normals (1 + m/2^mb) * 2^(e-bias). e4m3fn reserves
    its top code (S.1111.111) for NaN; e2m1 / e3m2 reserve nothing."""
    bias = 2 ** (ebits - 1) - 1
    vals = []
    for e in range(2 ** ebits):
        for m in range(2 ** mbits):
            vals.append((m / 2 ** mbits) * 2.0 ** (1 - bias) if e == 0 else (1 + m / 2 ** mbits) * 2.0 ** (e - bias))
    vals = vals[:len(vals) - reserved_top]
    assert vals == sorted(vals)
    return torch.tensor(vals, dtype=F64)


E4M3 = float_table(4, 3, reserved_top=1)   # 127 magnitudes, max 448
E2M1 = float_table(2, 1)                   # 0 .5 1 1.5 2 3 4 6
E3M2 = float_table(3, 2)                   # 32 magnitudes, max 28
FPX = {4: E2M1, 6: E3M2}


def _mids(tab):
    return (tab[1:] + tab[:-1]) / 2


def _rne(t):
    """Round half to even in float64 without torch.round."""
    f = torch.floor(t)
    d = t - f
    odd = torch.remainder(f, 2) == 1
    return f + ((d > 0.5) | ((d == 0.5) & odd)).to(t.dtype)


def group_scale(x, group, qmax):
    """-> (s fp32 [groups], finite [groups])."""
    a = x.reshape(-1, group).to(F32).abs()       # exact: every test dtype widens to fp32
    amax = a.amax(1)                             # torch's max propagates NaN
    s = amax / torch.tensor(qmax, dtype=F32)
    s = torch.where(s == 0, torch.ones_like(s), s)
    return s, torch.isfinite(s)


def _pack_nibbles(c):
    c = c.to(torch.int64) & 0xF
    return (c[0::2] | (c[1::2] << 4)).to(torch.uint8)


def unpack_nibbles(b, signed):
    b = b.to(torch.int64)
    v = torch.stack([b & 0xF, (b >> 4) & 0xF], 1).reshape(-1)
    return torch.where(v >= 8, v - 16, v) if signed else v


# ------------------------------------------------------------------------------------------------
# symmetric int8 / int4
# ------------------------------------------------------------------------------------------------
def sym_quant(x, group, bits):
    """-> namespace(codes int64 [n], alt, near_tie, packed uint8, scales fp32, finite [groups], t)."""
    qmax = 127.0 if bits == 8 else 7.0
    s, finite = group_scale(x, group, qmax)
    t = (x.reshape(-1, group).to(F64) / s.to(F64)[:, None]).reshape(-1)
    t = torch.where(torch.isnan(t), torch.full_like(t, qmax), t)   # only in non-finite groups; never compared
    lo = torch.floor(t)
    codes = _rne(t).clamp(-qmax, qmax)
    other = torch.where(codes == lo, lo + 1, lo).clamp(-qmax, qmax)
    near = ((t - lo) - 0.5).abs() <= 4 * 2.0 ** -24 * t.abs().clamp_min(1.0)
    codes, other = codes.to(torch.int64), other.to(torch.int64)
    packed = codes.to(torch.int8).view(torch.uint8) if bits == 8 else _pack_nibbles(codes)
    return SimpleNamespace(codes=codes, alt=other, near_tie=near, packed=packed, scales=s, finite=finite, t=t)


def sym_codes_of(packed, bits):
    """Per-element signed codes of a kernel's byte tensor."""
    return packed.view(torch.int8).to(torch.int64) if bits == 8 else unpack_nibbles(packed, True)


def sym_dequant(packed, scales, group, bits, dtype):
    """code * s, rounded once to ``dtype`` (float64 holds the product exactly)."""
    c = sym_codes_of(packed, bits).to(F64).reshape(-1, group)
    return (c * scales.to(F64)[:, None]).reshape(-1).to(dtype)


# ------------------------------------------------------------------------------------------------
# FP8 e4m3fn
# ------------------------------------------------------------------------------------------------
def _table_rne(a, tab):
    """Non-negative a (clamped to the table) -> (index by round-to-nearest, ties to the even index;
    index across the nearest midpoint; distance to that midpoint)."""
    mid = _mids(tab)
    a = a.clamp(max=float(tab[-1]))
    i = torch.bucketize(a, mid)                                   # mid[i-1] < a <= mid[i]: a tie gives the lower
    tie = (i < len(mid)) & (a == mid[i.clamp(max=len(mid) - 1)])
    i = i + (tie & (i % 2 == 1)).to(i.dtype)
    k = (a[:, None] - mid[None, :]).abs().argmin(1) if a.numel() else i   # nearest midpoint: between k and k+1
    dist = (a - mid[k]).abs()
    other = torch.where(i == k, k + 1, k)
    return i, other, dist


def _chunked(fn, a, tab, chunk=1 << 16):
    outs = [fn(a[o:o + chunk], tab) for o in range(0, max(a.numel(), 1), chunk)]
    return tuple(torch.cat(p) for p in zip(*outs))


def fp8_quant(x, group):
    """Codes are sign << 7 | magnitude index; the sign bit follows the sign of x (-0.0 included)."""
    s, finite = group_scale(x, group, 448.0)
    xg = x.reshape(-1, group).to(F64)
    t = (xg / s.to(F64)[:, None]).reshape(-1)
    t = torch.where(torch.isnan(t), torch.full_like(t, 448.0), t)
    a = t.abs()
    i, other, dist = _chunked(_table_rne, a, E4M3)
    sign = torch.signbit(x.reshape(-1).to(F64)).to(torch.int64) << 7
    near = dist <= 4 * 2.0 ** -24 * a.clamp_min(1.0)
    codes = sign | i
    return SimpleNamespace(codes=codes, alt=sign | other, near_tie=near, packed=codes.to(torch.uint8), scales=s,
                           finite=finite, t=t)


def fp8_value(codes):
    c = codes.to(torch.int64)
    mag = E4M3[(c & 0x7F).clamp(max=126)]
    return torch.where((c & 0x80) != 0, -mag, mag)


def fp8_dequant(packed, scales, group, dtype):
    v = fp8_value(packed).reshape(-1, group)
    return (v * scales.to(F64)[:, None]).reshape(-1).to(dtype)


# ------------------------------------------------------------------------------------------------
# FP6 e3m2 / FP4 e2m1 group quantizer (FP_Quantize)
# ------------------------------------------------------------------------------------------------
def _table_down(a, tab):
    """Nearest, ties to the smaller magnitude."""
    mid = _mids(tab)
    a = a.clamp(max=float(tab[-1]))
    i = torch.bucketize(a, mid)                                   # a == mid[i] stays on the lower index i
    k = (a[:, None] - mid[None, :]).abs().argmin(1) if a.numel() else i
    dist = (a - mid[k]).abs()
    other = torch.where(i == k, k + 1, k)
    return i, other, dist


def fpx_quant(x, bits, group):
    """Codes are sign << (bits - 1) | magnitude index, sign = (t < 0); FP4 packs two per byte, low
    nibble first, FP6 one per byte."""
    tab = FPX[bits]
    s, finite = group_scale(x, group, float(tab[-1]))
    t = (x.reshape(-1, group).to(F64) / s.to(F64)[:, None]).reshape(-1)
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
    a = t.abs()
    i, other, dist = _chunked(_table_down, a, tab)
    sign = (t < 0).to(torch.int64) << (bits - 1)
    near = dist <= 2.0 ** -23 * a
    codes = sign | i
    packed = _pack_nibbles(codes) if bits == 4 else codes.to(torch.uint8)
    return SimpleNamespace(codes=codes, alt=sign | other, near_tie=near, packed=packed, scales=s, finite=finite, t=t)


def fpx_codes_of(packed, bits):
    return unpack_nibbles(packed, False) if bits == 4 else packed.to(torch.int64)


def fpx_dequant(packed, scales, bits, group, n, dtype):
    c = fpx_codes_of(packed, bits)[:n]
    mag = FPX[bits][c & ((1 << (bits - 1)) - 1)]
    v = torch.where((c >> (bits - 1)) & 1 == 1, -mag, mag)
    sc = scales.to(F64).repeat_interleave(group)[:n]
    return (v * sc).to(dtype)


# ------------------------------------------------------------------------------------------------
# dequant_reduce
# ------------------------------------------------------------------------------------------------
def dequant_reduce(q, scales, W, group, bits, m, alpha, old=None, dt=F64):
    """out [m] = (old +) alpha * sum_w code_w * s_w. dt=float32 is the error baseline (the same
    arithmetic in fp32, summed in worker order)."""
    per = m if bits == 8 else m // 2
    ng = m // group
    acc = torch.zeros(m, dtype=dt)
    for w in range(W):
        c = sym_codes_of(q[w * per:(w + 1) * per], bits).to(dt).reshape(ng, group)
        acc = acc + (c * scales[w * ng:(w + 1) * ng].to(dt)[:, None]).reshape(-1)
    out = acc * torch.tensor(alpha, dtype=F32).to(dt)
    return out if old is None else old.to(dt) + out


# ------------------------------------------------------------------------------------------------
# 1-bit
# ------------------------------------------------------------------------------------------------
def sign_pack_ef(x, scale):
    """-> (packed uint8 [n/8], LSB first; err fp32 [n]). bit = x >= 0 (-0.0 positive, NaN negative);
    err = x - s or x + s, one fp32 operation."""
    pos = x >= 0
    s = scale.to(F32).reshape(())
    err = x - torch.where(pos, s, -s)
    w = (1 << torch.arange(8, dtype=torch.int64))
    packed = (pos.reshape(-1, 8).to(torch.int64) * w).sum(1).to(torch.uint8)
    return packed, err


def unpack_avg(packed, scales):
    """packed [W, n/8], scales [W] -> float64 [n]: mean over W of +-s_w."""
    W = packed.shape[0]
    bits = ((packed.to(torch.int64)[:, :, None] >> torch.arange(8)) & 1).reshape(W, -1)
    sg = bits.to(F64) * 2 - 1
    return (sg * scales.to(F64)[:, None]).sum(0) / W


# ------------------------------------------------------------------------------------------------
# MXFP8 activation block (mx_quant_fp8), finite inputs
# ------------------------------------------------------------------------------------------------
def mx_fp8_block(x):
    """x [R, K] (K % 32 == 0) -> (codes uint8 [R, K], E8M0 bytes uint8 [R, K/32]). Block exponent
    ceil(log2(amax / 448)) clamped to +-127 (-127 for a zero block); codes RNE onto e4m3, saturating."""
    R, K = x.shape
    g = x.to(F64).reshape(R, K // 32, 32)
    amax = g.abs().amax(-1)
    mant, ex = torch.frexp(amax / 448.0)            # amax / 448 = mant * 2^ex, mant in [.5, 1)
    e = torch.where(mant == 0.5, ex - 1, ex)
    e = torch.where(amax > 0, e, torch.full_like(e, -127)).clamp(-127, 127)
    t = (g * torch.exp2(-e.to(F64))[..., None]).reshape(-1)
    i, _, _ = _chunked(_table_rne, t.abs(), E4M3)
    codes = (torch.signbit(t).to(torch.int64) << 7) | i
    return codes.to(torch.uint8).reshape(R, K), (e + 127).to(torch.uint8)


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------
GROUPS = [64, 128, 192, 320, 512, 2048]


def n_groups(group):
    """5 groups where a lane's share (group / 64) is odd -- a neighbouring group's first byte and the
    allocation's tail are then both looked at -- else 3."""
    return 5 if (group // 64) % 2 else 3


def rand_case(group, dtype, seed=0, groups=None):
    """randn with a different magnitude per group (1e-3 .. 1e2). The base seed is one at which every
    table case stays under the tie-window caps that tests/test_quant_refs.py asserts (a bf16 group whose
    amax mantissa shares a factor with qmax puts many quotients on half-way points)."""
    ng = groups or n_groups(group)
    g = _gen(105 + group + seed)
    x = torch.randn(ng, group, generator=g, dtype=F64)
    mag = torch.tensor([3.0, 1e-3, 1e2, 0.25, 17.0], dtype=F64)[torch.arange(ng) % 5]
    return (x * mag[:, None]).reshape(-1).to(dtype)


STRIDE_GROUPS = 8208          # > 8192 one-wave groups per launch, and 8208 * 64 = 525,312 > 524,288 elements
FPX_STRIDE_GROUPS = 16400     # > 16384 (4096 blocks x 4 waves), groups of 32: 524,800 elements


def stride_case(dtype):
    return rand_case(64, dtype, seed=7, groups=STRIDE_GROUPS)


def fpx_stride_case(dtype):
    g = _gen(31)
    return (torch.randn(FPX_STRIDE_GROUPS * 32, generator=g, dtype=F64) * 2).to(dtype)


def _halves(qmax):
    h = torch.arange(0, int(qmax), dtype=F64) + 0.5
    i = torch.arange(0, int(qmax) + 1, dtype=F64)
    return torch.cat([h, -h, i, -i])


def crafted_values(kind):
    """Every half-way point of the format, both signs, its representable values and +-qmax."""
    if kind in ("int8", "int4"):
        return _halves(KINDS[kind])
    tab = {"fp8": E4M3, "fp4": E2M1, "fp6": E3M2}[kind]
    v = torch.cat([_mids(tab), tab])
    return torch.cat([v, -v])


def crafted_case(kind, group, dtype):
    """Groups of ``group`` holding the crafted values, each with one element at exactly qmax so that
    s = 1 and t = x; then an all-zero group (with one -0.0), and a group whose only non-zero value is
    negative. Every value is representable in bf16, fp16 and fp32."""
    qmax = {"fp4": 6.0, "fp6": 28.0}.get(kind) or KINDS[kind]
    vals = crafted_values(kind)
    per = group - 1
    ng = -(-len(vals) // per)
    body = torch.zeros(ng * per, dtype=F64)
    body[:len(vals)] = vals
    x = torch.cat([body.reshape(ng, per), torch.full((ng, 1), qmax, dtype=F64)], 1)
    x[1::2] = x[1::2].flip(1)                      # qmax first in odd groups, last in even ones
    zero = torch.zeros(1, group, dtype=F64)
    zero[0, 3] = -0.0
    neg = torch.zeros(1, group, dtype=F64)
    neg[0, group // 2] = -3.0
    out = torch.cat([x, zero, neg]).reshape(-1).to(dtype)
    assert torch.equal(out.to(F64), torch.cat([x, zero, neg]).reshape(-1)), "crafted values must be exact"
    return out


TINY_AMAX = [2.0 ** -120, 2.0 ** -127, 2.0 ** -133]   # the last is the smallest bf16 subnormal
TINY_DTYPES = [torch.float32, torch.bfloat16]         # fp16 stops at 2^-24
# 2^-149 (fp32 only): amax / qmax underflows to zero -- the zero group
TINY_CASES = [(a, d) for a in TINY_AMAX for d in TINY_DTYPES] + [(2.0 ** -149, torch.float32)]
TINY_IDS = [f"2^{int(torch.log2(torch.tensor(a, dtype=F64)))}-{dtype_id(d)}" for a, d in TINY_CASES]


# seeds of the neighbour / guard data: ones at which every case stays under the tie-window caps
TINY_SEED, NONFINITE_SEED, GUARD_SEED = 12, 13, 5


def guard_case(group, dtype):
    return rand_case(group, dtype, seed=GUARD_SEED)


def tiny_case(amax, group, dtype):
    """Three groups; the middle one has amax ``amax`` (multiples of it that the dtype holds) mixed with
    exact zeros. -> (x, zero mask of the middle group's elements [n])."""
    x = rand_case(group, dtype, seed=TINY_SEED, groups=3).to(F64).reshape(3, group)
    # multiples whose quotients (mult * qmax for 127, 7, 448, 6, 28) stay clear of every half-way point
    mult = torch.tensor([0.0, 1.0, -1.0, 0.0, 0.3125, -0.625, 0.0, 0.25], dtype=F64)
    mid = (mult[torch.arange(group) % 8] * amax).to(dtype).to(F64)
    mid[1] = amax
    mid[group - 1] = 0.0
    x[1] = mid
    x = x.reshape(-1).to(dtype)
    assert float(x.to(F64).reshape(3, group)[1].abs().max()) == amax
    zeros = torch.zeros(3, group, dtype=torch.bool)
    zeros[1] = x.reshape(3, group)[1] == 0
    return x, zeros.reshape(-1)


NONFINITE = {"nan": [NAN], "+inf": [INF], "-inf": [-INF], "nan+inf": [NAN, INF]}
NONFINITE_POS = ["first", "last", "mid"]


def nonfinite_case(pattern, pos, group, dtype):
    """Three groups, the middle one holding the pattern. -> (x, x with the middle group zeroed)."""
    x = rand_case(group, dtype, seed=NONFINITE_SEED, groups=3).reshape(3, group).clone()
    clean = x.clone()
    clean[1] = 0
    at = {"first": 0, "last": group - 1, "mid": group // 2 + 1}[pos]
    for k, v in enumerate(NONFINITE[pattern]):
        x[1, (at + 5 * k) % group] = v
    return x.reshape(-1), clean.reshape(-1)


REDUCE_W = [1, 3, 8]
REDUCE_GROUPS = [64, 128]
REDUCE_ALPHA = [1.0, 0.125]


def reduce_inputs(bits, W, group, seed=0, m=None):
    """The W workers' fp32 data behind ``reduce_case``."""
    m = m or group * n_groups(group)
    return [rand_case(group, F32, seed=seed + 17 * w + bits, groups=m // group) for w in range(W)]


def reduce_case(bits, W, group, seed=0, m=None):
    """W workers' reference-quantized chunks of m values -> (q [W * bytes], scales [W * m/group], old out)."""
    m = m or group * n_groups(group)
    qs, ss = [], []
    for x in reduce_inputs(bits, W, group, seed, m):
        r = sym_quant(x, group, bits)
        qs.append(r.packed)
        ss.append(r.scales)
    old = torch.randn(m, generator=_gen(900 + seed + W))
    return torch.cat(qs), torch.cat(ss), old


FPX_GROUPS = [2, 32, 66, 512]


def fpx_case(bits, group, dtype, seed=0):
    n = max(4 * group, 132)
    n = -(-n // group) * group
    g = _gen(200 + group + bits + seed)
    x = torch.randn(n, generator=g, dtype=F64) * 2
    x[::7] = 0.0
    return x.to(dtype)


ONEBIT_N = [8, 64, 8 * 65537 * 9]     # the last: 589,833 packed bytes > 524,288 threads


def onebit_case(n, seed=0):
    """-> (x fp32 [n] with -0.0, runs of +-0.0 and NaN spliced in, scale fp32 [1])."""
    g = _gen(400 + seed + n % 1000)
    x = torch.randn(n, generator=g)
    x[1] = -0.0
    x[2] = 0.0
    x[5] = NAN
    if n >= 64:
        x[16:24] = 0.0
        x[24:32] = -0.0
        x[40] = NAN
        x[n - 1] = -0.0
        x[n - 2] = NAN
    scale = x.nan_to_num(0.0).norm().div(n ** 0.5).reshape(1).clamp_min(0.25)
    return x, scale


def mx_range_cases():
    """name -> x [2, 64] bf16: blocks whose amax is the largest finite bf16 / the smallest bf16 subnormal."""
    big = torch.tensor(0x7F7F, dtype=torch.int16).view(torch.bfloat16).to(F64)
    tiny = 2.0 ** -133
    g = _gen(55)
    xb = (torch.rand(2, 64, generator=g, dtype=F64) * 2 - 1) * big
    xb[0, 3], xb[0, 40], xb[1, 0], xb[1, 63] = big, -big, -big, big
    xt = torch.randint(-1, 2, (2, 64), generator=g).to(F64) * tiny
    xt[0, 0], xt[0, 33], xt[1, 31], xt[1, 32] = tiny, -tiny, tiny, tiny
    return {"max_bf16": xb.to(torch.bfloat16), "min_bf16_subnormal": xt.to(torch.bfloat16)}


def quant_table():
    """(kind, group, dtype) of the random cases."""
    return list(itertools.product(KINDS, GROUPS, DTYPES))
