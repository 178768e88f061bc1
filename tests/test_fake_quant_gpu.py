"""gfx950 fused fake-quantize kernels (csrc/kernels/fake_quant.hip) against CPU oracles:
``runtime.quantize.fake_quantize`` for the symmetric / asymmetric grids and an fp64 evaluation of
the reference's binary / ternary formulas. Shapes are picked for the kernel's paths: one wave per
group, one block per group with 1 / 2 / 4 / 8 chunks per thread, 16-byte and scalar accesses,
tails, both sides of the register-path limit (16384 values per group) and the multi-block path."""
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SMALL_MAX = 16384  # csrc/kernels/fake_quant.hip kSmallMax
# (shape, groups): what each is there for
SHAPES = [
    ((96, 200), 96),          # one wave per group, aligned rows
    ((7, 203), 7),            # group starts unaligned for 16-bit types, tail
    ((5, 40), 5),             # a group smaller than a wave
    ((3 * 256 * 8 + 5,), 1),  # one group, not a multiple of 8: scalar accesses, 4 chunks per thread
    ((3, 1000), 3),           # one block per group, 1 chunk per thread, partly filled
    ((2, 3000), 2),           # 2 chunks per thread
    ((2, 6000), 2),           # 4 chunks per thread
    ((2, SMALL_MAX), 2),      # the largest group the register path takes (8 chunks per thread)
    ((2, SMALL_MAX + 8), 2),  # the smallest aligned group on the multi-block path
    ((2, 20000), 2),          # multi-block path, aligned groups
    ((2, 20001), 2),          # multi-block path, unaligned groups: scalar accesses
    ((SMALL_MAX + 8 * 300 + 5,), 1),  # multi-block path, one group: 16-byte accesses and a scalar tail
]
LARGE = [s for s in SHAPES if math.prod(s[0]) // s[1] > SMALL_MAX]
_IDS = [f"{'x'.join(map(str, s))}-g{g}" for s, g in SHAPES]


@functools.lru_cache(maxsize=None)
def make_input(shape, groups, dtype):
    """Seeded on the CPU: normal data with a different scale per group and a non-zero mean. About
    one element in 10^5 of such data lies within 1e-5 (relative) of its group's ternary threshold,
    where fp32 and fp64 may disagree about the mask, so the first seed of a fixed sequence whose
    data has no such element is used (the CPU-only test below checks that). Shared: do not modify."""
    for attempt in range(32):
        gen = torch.Generator().manual_seed(7919 * attempt + 1000 * len(shape) + sum(shape) + groups)
        x = torch.randn(groups, math.prod(shape) // groups, generator=gen)
        x = (x * (0.25 + 0.5 * torch.arange(groups).float()[:, None] / groups) + 0.1).reshape(shape).to(dtype)
        if not ternary_ref64(x, groups)[1].any():
            break
    return x


@pytest.fixture
def hip():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from shuffle_exchange_amd.ops import native
    return native.require_hip()


def grid_step(x, bits, groups, symmetric, value_range=None):
    """The oracle's per-group quantization step, [groups, 1]."""
    flat = x.float().reshape(groups, -1)
    if value_range is not None:
        lo, hi = value_range[0].reshape(1, 1), value_range[1].reshape(1, 1)
        amax = torch.maximum(lo.abs(), hi)
    else:
        lo, hi = flat.amin(1, keepdim=True), flat.amax(1, keepdim=True)
        amax = flat.abs().amax(1, keepdim=True)
    if symmetric:
        return amax.clamp_min(1e-12) / (2 ** (bits - 1) - 1)
    return (hi - lo).clamp_min(1e-12) / (2 ** bits - 1)


def check_grid(out, ref, step, what):
    """Within one step everywhere; at most 0.1 % of the elements differ at all (expected: none; the
    cap only absorbs a division-rounding difference exactly on a tie)."""
    assert out.dtype == ref.dtype and out.shape == ref.shape
    g = step.shape[0]
    diff = (out.float() - ref.float()).abs().reshape(g, -1)
    n_diff = int((diff > 0).sum())
    print(f"{what}: {n_diff} of {diff.numel()} differ, max |diff| / step = {float((diff / step).max()):.3g}")
    assert torch.isfinite(out.float()).all(), what
    assert (diff <= step).all(), what
    assert n_diff <= 0.001 * diff.numel(), (what, n_diff)


def binary_ref64(x, groups):
    flat = x.double().reshape(groups, -1)
    return (flat.sign() * flat.abs().mean(1, keepdim=True)).reshape(x.shape)


def ternary_ref64(x, groups):
    """fp64 reference TernaryQuantizer, and the elements too close to the threshold to compare
    (``||x| - thres| < 1e-5 * thres``: fp32 and fp64 may put them on different sides)."""
    flat = x.double().reshape(groups, -1)
    thres = 0.7 * flat.abs().mean(1, keepdim=True)
    mask = (flat.abs() > thres).double()
    alpha = (flat.abs() * mask).sum(1, keepdim=True) / mask.sum(1, keepdim=True).clamp_min(1)
    near = (flat.abs() - thres).abs() < 1e-5 * thres
    return (alpha * flat.sign() * mask).reshape(x.shape), near.reshape(x.shape)


def check_lowbit(out, ref, dtype, what, skip=None):
    """fp32: rtol 2e-5 (fp32 sums against fp64). bf16 / fp16: one ulp of the storage type."""
    assert out.dtype == dtype and out.shape == ref.shape
    assert torch.isfinite(out.float()).all(), what
    err = (out.double() - ref).abs()
    if dtype == torch.float32:
        tol = 2e-5 * ref.abs()
    else:
        mant = 7 if dtype == torch.bfloat16 else 10
        tol = torch.where(ref == 0, torch.zeros_like(ref),
                          torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - mant))
    bad = err > tol
    if skip is not None:
        bad &= ~skip
    print(f"{what}: max err / tol = {float((err / tol.clamp_min(1e-30)).max()):.3g}")
    assert not bad.any(), (what, int(bad.sum()))


def test_ternary_oracle_inputs_have_no_element_on_the_threshold():
    """CPU: with the seeds used, no input element is within 1e-5 (relative) of its group's ternary
    threshold, so the GPU comparison below leaves nothing out."""
    for (shape, groups) in SHAPES:
        for dtype in DTYPES:
            _, near = ternary_ref64(make_input(shape, groups, dtype), groups)
            assert int(near.sum()) == 0, (shape, groups, dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape,groups", SHAPES, ids=_IDS)
def test_symmetric_and_asymmetric_match_fake_quantize(hip, shape, groups, dtype):
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    from shuffle_exchange_amd.runtime.quantize import fake_quantize
    x = make_input(shape, groups, dtype)
    xg = x.cuda()
    for symmetric in (True, False):
        for bits in (3, 4, 8):
            mode = "symmetric" if symmetric else "asymmetric"
            out = fake_quant(xg, bits, groups, mode).cpu()
            check_grid(out, fake_quantize(x, bits, groups, symmetric), grid_step(x, bits, groups, symmetric),
                       f"{mode} {bits}b")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape,groups", SHAPES, ids=_IDS)
def test_binary_and_ternary_match_fp64_reference(hip, shape, groups, dtype):
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    x = make_input(shape, groups, dtype)
    xg = x.cuda()
    check_lowbit(fake_quant(xg, 1, groups, "binary").cpu(), binary_ref64(x, groups), dtype, "binary")
    ref, near = ternary_ref64(x, groups)
    assert int(near.sum()) <= 0.001 * near.numel()
    check_lowbit(fake_quant(xg, 2, groups, "ternary").cpu(), ref, dtype, "ternary", skip=near)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", [(3, 40), (3, 2048), (3, 20000)], ids=["wave", "block", "multiblock"])
def test_all_zero_group_gives_zeros(hip, shape, dtype):
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    x = make_input(shape, 3, dtype).clone()
    x[1] = 0
    xg = x.cuda()
    for mode, bits in (("symmetric", 4), ("asymmetric", 4), ("binary", 1), ("ternary", 2)):
        out = fake_quant(xg, bits, 3, mode).cpu()
        assert torch.isfinite(out.float()).all() and (out[1] == 0).all(), mode
        assert (out[0] != 0).any() and (out[2] != 0).any(), mode


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", [(37, 203), (64, 512), (5,)], ids=["7511", "32768", "5"])
def test_static_range_matches_cpu_formula(hip, shape, dtype):
    from shuffle_exchange_amd.ops.fake_quant import _torch_fake_quant, fake_quant
    x = make_input(shape, 1, dtype) * 3  # well outside the range on both sides
    r = torch.tensor([-0.7, 1.3])
    xg, rg = x.cuda(), r.cuda()
    for mode in ("symmetric", "asymmetric"):
        for bits in (3, 4, 8):
            out = fake_quant(xg, bits, 1, mode, rg).cpu()
            ref = _torch_fake_quant(x, bits, 1, mode, r)
            step = grid_step(x, bits, 1, mode == "symmetric", r)
            check_grid(out, ref, step, f"static {mode} {bits}b")
            if mode == "asymmetric":  # clamped to the stored range
                assert float(out.float().min()) >= -0.7 - float(step) and float(out.float().max()) <= 1.3 + float(step)


@gpu
@pytest.mark.parametrize("shape,groups", LARGE + [((96, 200), 96), ((2, SMALL_MAX), 2)])
def test_two_runs_are_bit_identical(hip, shape, groups):
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    xg = make_input(shape, groups, torch.bfloat16).cuda()
    for mode, bits in (("symmetric", 4), ("asymmetric", 4), ("binary", 1), ("ternary", 2)):
        a = fake_quant(xg, bits, groups, mode)
        b = fake_quant(xg, bits, groups, mode)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), mode


@gpu
def test_bad_arguments_raise_on_the_host(hip):
    x = torch.randn(4, 10, device="cuda")
    r = torch.tensor([-1.0, 1.0], device="cuda")
    op = torch.ops.sxe.fake_quant
    for args in [(x, 3, 0, 4, None),                        # 40 % 3 != 0
                 (x, 0, 0, 4, None),                        # no groups
                 (x, 1, 0, 2, None), (x, 1, 1, 17, None),   # bits outside 3..16
                 (x, 1, 7, 4, None),                        # unknown mode
                 (x.t(), 1, 0, 4, None),                    # not contiguous
                 (x.cpu(), 1, 0, 4, None),                  # not on the GPU
                 (x.long(), 1, 0, 4, None),                 # not a floating type
                 (x, 2, 0, 4, r), (x, 1, 2, 4, r),          # a range with groups, with the binary mode
                 (x, 1, 0, 4, r.cpu()), (x, 1, 0, 4, r.double()), (x, 1, 0, 4, torch.zeros(3, device="cuda"))]:
        with pytest.raises((RuntimeError, NotImplementedError)):
            op(*args)
    assert op(x[:0], 1, 0, 4, None).shape == (0, 10)
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    for bits in (2, 17):  # the CPU path takes these widths; a GPU tensor raises rather than changing path
        with pytest.raises(ValueError, match="3..16"):
            fake_quant(x, bits, 1, "symmetric")


@gpu
def test_fake_kernel_traces(hip):
    from torch._subclasses.fake_tensor import FakeTensorMode

    import shuffle_exchange_amd.ops.fake_kernels  # noqa: F401
    with FakeTensorMode():
        x = torch.empty(6, 40, device="cuda", dtype=torch.bfloat16)
        y = torch.ops.sxe.fake_quant(x, 6, 3, 2, None)
    assert y.shape == x.shape and y.dtype == x.dtype and y.device == x.device


def ulp_of(ref, dtype):
    """One unit in the last place of ``dtype`` at the magnitude of ``ref`` (0 at 0)."""
    mant = 7 if dtype == torch.bfloat16 else 10
    ref = ref.double()
    return torch.where(ref == 0, torch.zeros_like(ref),
                       torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - mant))


@gpu
def test_binary_linear_layer_runs_the_kernel_and_matches_cpu(hip, monkeypatch):
    """LinearLayer_Compress in bf16 with a 1-bit target: the GPU layer goes through
    torch.ops.sxe.fake_quant (counted; the PyTorch path is patched to raise), its binarized weight
    is within one bf16 ulp of the fp64 formula and of the CPU layer's, and the CPU layer's outputs
    are finite. The layer's GEMMs are then checked against fp64 products of the GPU's own operands
    (its binarized weight, x, the output gradient): each result is a K-term fp32-accumulated dot
    product rounded once to bf16, so it lies within one bf16 ulp of the exact value plus the fp32
    accumulation error, K * 2^-24 times the dot product of the absolute values."""
    import shuffle_exchange_amd.ops.fake_quant as fq
    from shuffle_exchange_amd.compression import LinearLayer_Compress
    torch.manual_seed(0)
    groups, bf16 = 4, torch.bfloat16
    cpu = LinearLayer_Compress(200, 48, bias=False, dtype=bf16)
    with torch.no_grad():  # the default bf16 uniform init draws exact zeros, which binarize to a third value, 0
        cpu.weight.copy_(torch.randn(48, 200) * 0.05)
    assert (cpu.weight != 0).all()
    dev = LinearLayer_Compress(200, 48, bias=False, dtype=bf16, device="cuda")
    dev.load_state_dict(cpu.state_dict())
    x = torch.randn(9, 200).to(bf16)
    c = torch.randn(9, 48).to(bf16)

    calls = []
    real = torch.ops.sxe.fake_quant

    def counted(*a, **k):
        calls.append(a[2])
        return real(*a, **k)

    def run(layer, x, c):
        layer.enable_weight_quantization(2, 1, 1, quantization_type="symmetric", num_groups=groups)
        x = x.clone().requires_grad_(True)
        y = layer(x)  # the ramp steps 2 -> 1 before the first quantization
        (y.float() * c.float()).sum().backward()
        layer.eval()
        return y.detach(), x.grad, layer.weight.grad, layer.effective_weight().detach()

    y0, gx0, gw0, w0 = run(cpu, x, c)
    assert not calls
    monkeypatch.setattr(torch.ops.sxe, "fake_quant", counted)

    def refuse(*a, **k):
        raise AssertionError("the GPU layer took the PyTorch fake-quantize path")
    monkeypatch.setattr(fq, "_torch_fake_quant", refuse)
    y1, gx1, gw1, w1 = [t.cpu() for t in run(dev, x.cuda(), c.cuda())]
    assert len(calls) > 0 and set(calls) == {fq.MODES["binary"]}

    for t in (y0, gx0, gw0, w0, y1, gx1, gw1, w1):
        assert torch.isfinite(t.float()).all()
    assert all(r.unique().numel() == 2 for r in w1.reshape(groups, -1))
    check_lowbit(w1, binary_ref64(cpu.weight.detach(), groups), bf16, "layer weight")
    assert ((w1.double() - w0.double()).abs() <= ulp_of(w0, bf16)).all()

    xd, cd, wd = x.double(), c.double(), w1.double()
    for name, got, ref, mag, k in (("y", y1, xd @ wd.t(), xd.abs() @ wd.abs().t(), 200),
                                   ("x.grad", gx1, cd @ wd, cd.abs() @ wd.abs(), 48),
                                   ("weight.grad", gw1, cd.t() @ xd, cd.abs().t() @ xd.abs(), 9)):
        err = (got.double() - ref).abs()
        tol = ulp_of(ref, bf16) + k * 2.0 ** -24 * mag
        print(f"layer {name}: max err / tol = {float((err / tol).max()):.3g}")
        assert (err <= tol).all(), name


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", [(3, 40), (3, 2048), (3, 20000)], ids=["wave", "block", "multiblock"])
def test_nan_elements_stay_nan(hip, shape, dtype):
    """A NaN input never becomes a finite grid point. In the symmetric / asymmetric modes the rest of
    its group is quantized on the grid of the group's other values (csrc/kernels/fake_quant.hip
    header), i.e. exactly as if the NaN were one of them; other groups are untouched in every mode."""
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    x = make_input(shape, 3, dtype).clone()
    clean = x.clone()
    clean[1, 7] = clean[1, 8]  # a value the group already has: same statistics as skipping the NaN
    x[1, 7] = float("nan")
    xg, cg = x.cuda(), clean.cuda()
    for mode, bits in (("symmetric", 4), ("asymmetric", 4), ("binary", 1), ("ternary", 2)):
        out, ref = fake_quant(xg, bits, 3, mode).cpu(), fake_quant(cg, bits, 3, mode).cpu()
        assert torch.isnan(out[1, 7]), mode
        assert torch.equal(out[0], ref[0]) and torch.equal(out[2], ref[2]), mode
        if bits == 4:
            keep = torch.ones(shape[1], dtype=torch.bool)
            keep[7] = False
            assert torch.equal(out[1][keep], ref[1][keep]), mode
