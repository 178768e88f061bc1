"""Edge-case tests of the row kernels (xent.hip, norm.hip, act.hip, rope.hip, softmax.hip) against the
float64 references of tests/_row_refs.py: the grid-stride branches training runs at 16k tokens, every
dtype, activation and mask form the launchers dispatch, vector/scalar and block/wave-per-row paths,
ragged widths, -inf logits, ignored rows and the host checks.

Every comparison is per element. The bound for one case is

    |kernel - ref| <= FACTOR * max|baseline - ref| + 1 ulp(output dtype, at |ref|)

where the baseline is the same reference arithmetic in plain fp32 torch on the GPU, rounded to the
output dtype. FACTOR is 2 for 16-bit outputs. For fp32 outputs (loss, lse, rstd, mean, dw, db and the
fp32 activations) the kernels use __expf / __logf / rsqrtf and FACTOR is FP32_FACTOR, chosen from the
errors measured on an MI355X that profiles/row_kernel_edges.log records per kernel family.
Exact claims (ignored rows, untouched RoPE regions, h_out, fully masked rows, gT) use torch.equal.
"""
import pytest
import torch

from tests import _row_refs as R

pytestmark = pytest.mark.gpu

F32 = torch.float32
# profiles/row_kernel_edges.log: the largest factor any fp32-output case needs is 2.71 (norm.dw, the
# sequential per-wave sums); the next power of two, well under the cap of 16
FP32_FACTOR = 4.0
DEV = "cuda"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from shuffle_exchange_amd.ops import native
    native.require_hip()


def _ops():
    return torch.ops.sxe


def _cu(*ts):
    return [t.to(DEV) if torch.is_tensor(t) else t for t in ts]


def _ulp(ref, dtype):
    """Spacing of ``dtype`` at |ref| (the subnormal spacing below the smallest normal)."""
    fi = torch.finfo(dtype)
    a = ref.abs().clamp_min(fi.tiny)
    return torch.exp2(torch.floor(torch.log2(a))) * fi.eps


def _check(tag, out, ref, base):
    """Per-element bound of the module docstring; prints the figures the log is built from."""
    dtype = out.dtype
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{tag}: non-finite kernel output"
    factor = FP32_FACTOR if dtype == F32 else 2.0
    eb = (base.to(dtype).double() - ref).abs().max()
    ek = (out.double() - ref).abs()
    ulp = _ulp(ref, dtype)
    bound = factor * eb + ulp
    need = ((ek - ulp).clamp_min(0) / eb.clamp_min(1e-300)).max() if eb > 0 else (ek - ulp).clamp_min(0).max()
    print(f"[row-edge] {tag} out={R.dtype_id(dtype)} n={out.numel()} base_max={eb.item():.3e} "
          f"kern_max={ek.max().item():.3e} worst_over_bound={(ek / bound).max().item():.3f} "
          f"factor_needed={need.item():.3f}")
    bad = ek > bound
    assert not bad.any(), (f"{tag}: {int(bad.sum())} elements over the bound, worst {ek.max().item():.3e} vs "
                           f"{bound.flatten()[ek.argmax()].item():.3e} (baseline max {eb.item():.3e})")


# ================================================================================================
# cross-entropy
# ================================================================================================
def _xent_modes(tag, logits, target, ign, check_position=True):
    ops = _ops()
    logits, target = _cu(logits, target)
    rows, V = logits.shape
    live = target != ign
    minf = logits == R.NEG_INF
    r_loss, r_lse, _ = R.xent_ref(logits, target, ign)
    b_loss, b_lse, _ = R.xent_ref(logits, target, ign, dt=F32)

    # forward only: the logits stay as they are
    work = logits.clone()
    loss, lse = ops.xent_fwd(work, target, ign, False, None, 1.0)
    assert torch.equal(work, logits)
    _check(f"xent.loss {tag}", loss, r_loss, b_loss)
    _check(f"xent.lse {tag}", lse, r_lse, b_lse)
    assert (loss[~live] == 0).all()

    # forward + in-place gradient, scale tensor combined with grad_scale
    scale_t = torch.tensor([0.25], device=DEV)
    work = logits.clone()
    loss2, lse2 = ops.xent_fwd(work, target, ign, True, scale_t, 3.0)
    assert torch.equal(loss2, loss) and torch.equal(lse2, lse)
    _, _, r_g = R.xent_ref(logits, target, ign, scale=0.75)
    _, _, b_g = R.xent_ref(logits, target, ign, scale=0.75, dt=F32)
    _check(f"xent.grad_inplace {tag}", work, r_g, b_g)
    assert torch.equal(work[~live], torch.zeros_like(work[~live]))
    assert (work[minf] == 0).all()
    if check_position:
        for r in torch.nonzero(live).flatten().tolist()[:4]:
            t = int(target[r])
            assert work[r, t] <= 0, (tag, r, t)
            assert (work[r, max(t - 2, 0):t] >= 0).all() and (work[r, t + 1:t + 3] >= 0).all(), (tag, r, t)

    # backward from a given lse with a distinct upstream gradient per row
    dloss = torch.linspace(0.5, 2.0, rows, device=DEV)
    lse32 = r_lse.float()
    _, _, r_g = R.xent_ref(logits, target, ign, scale=dloss, lse=lse32)
    _, _, b_g = R.xent_ref(logits, target, ign, scale=dloss, lse=lse32, dt=F32)
    work = logits.clone()
    g = ops.xent_bwd(work, target, lse32, dloss, ign, False)
    assert g.data_ptr() != work.data_ptr() and torch.equal(work, logits)
    _check(f"xent.bwd {tag}", g, r_g, b_g)
    assert torch.equal(g[~live], torch.zeros_like(g[~live])) and (g[minf] == 0).all()
    gi = ops.xent_bwd(work, target, lse32, dloss, ign, True)
    assert gi.data_ptr() == work.data_ptr() and gi.untyped_storage().data_ptr() == work.untyped_storage().data_ptr()
    assert torch.equal(gi, g)
    if check_position:
        for r in torch.nonzero(live).flatten().tolist()[:4]:
            t = int(target[r])
            assert g[r, t] <= 0 and (g[r, max(t - 2, 0):t] >= 0).all() and (g[r, t + 1:t + 3] >= 0).all()
    return loss, lse


@pytest.mark.parametrize("tset", list(R.XENT_TSETS))
@pytest.mark.parametrize("V", R.XENT_VOCABS)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
def test_xent_vocab_edges(dtype, V, tset):
    logits, target, ign = R.xent_case(V, dtype, tset)
    _xent_modes(f"V={V} {tset} {R.dtype_id(dtype)}", logits, target, ign)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
def test_xent_grid_stride(dtype):
    """8197 rows > the 8192-block cap: rows 8192.. are a block's second trip (LDS `red` reused)."""
    logits, target, ign = R.xent_stride_case(dtype)
    _xent_modes(f"stride 8197x64 {R.dtype_id(dtype)}", logits, target, ign)


@pytest.mark.parametrize("V", [2048, 1001])
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
def test_xent_extreme_rows(dtype, V):
    logits, target, ign = R.xent_extreme_case(V, dtype)
    _xent_modes(f"extreme V={V} {R.dtype_id(dtype)}", logits, target, ign)


@pytest.mark.parametrize("vec", [True, False], ids=["vector", "scalar"])
@pytest.mark.parametrize("pattern", R.XENT_INF)
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
def test_xent_neg_inf_logits(dtype, pattern, vec):
    """-inf logits (masked vocabulary padding, banned tokens): loss and lse finite and equal to the
    reference, gradient exactly 0 on the -inf columns. The vector path gave NaN rows here when all
    eight logits of a lane's chunk were -inf."""
    logits, target, ign = R.xent_inf_case(pattern, vec, dtype)
    assert (logits.shape[1] % 8 == 0) == vec
    _xent_modes(f"-inf {pattern} {'vec' if vec else 'scalar'} {R.dtype_id(dtype)}", logits, target, ign)


def test_xent_grad_dual_neg_inf_tail():
    ops = _ops()
    logits, target, ign = _cu(*R.xent_dual_inf_case())
    _, lse = ops.xent_fwd(logits.clone(), target, ign, False, None, 1.0)
    sa, sb = torch.tensor([1.0 / 63], device=DEV), torch.tensor([2.0], device=DEV)
    sc = float(sa.double() * sb.double())
    _, _, r_g = R.xent_ref(logits, target, ign, scale=sc, lse=lse)
    _, _, b_g = R.xent_ref(logits, target, ign, scale=sc, lse=lse, dt=F32)
    work = logits.clone()
    gT = ops.xent_grad_dual(work, target, lse, ign, sa, sb)
    _check("xent.grad_dual -inf tail 64x2304", work, r_g, b_g)
    assert (work[:, 2048:] == 0).all() and (work[target == ign] == 0).all()
    assert gT.shape == (2304, 64) and torch.equal(gT, work.t().contiguous())


@pytest.mark.parametrize("dtype", [torch.bfloat16, F32], ids=R.dtype_id)
@pytest.mark.parametrize("V", [1000, 1001])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_cross_entropy_autograd(reduction, V, dtype):
    from shuffle_exchange_amd.ops.cross_entropy import cross_entropy
    logits, target, ign = _cu(*R.xent_case(V, dtype, "seam_ign"))
    x = logits.clone().requires_grad_(True)
    out = cross_entropy(x, target, ignore_index=ign, reduction=reduction)
    n = int((target != ign).sum())
    sc = 1.0 / n if reduction == "mean" else 1.0
    r_loss, _, r_g = R.xent_ref(logits, target, ign, scale=sc)
    b_loss, _, b_g = R.xent_ref(logits, target, ign, scale=sc, dt=F32)
    if reduction == "none":
        _check(f"xent.wrapper none V={V}", out.detach(), r_loss, b_loss)
        out.sum().backward()
    else:
        _check(f"xent.wrapper {reduction} V={V}", out.detach(), r_loss.sum() * sc, b_loss.sum() * sc)
        out.backward()
    _check(f"xent.wrapper grad {reduction} V={V}", x.grad, r_g, b_g)
    assert torch.equal(x.grad[target == ign], torch.zeros_like(x.grad[target == ign]))


def test_cross_entropy_all_ignored_is_zero():
    from shuffle_exchange_amd.ops.cross_entropy import cross_entropy
    x = torch.randn(5, 1000, device=DEV).bfloat16().requires_grad_(True)
    target = torch.full((5,), -100, dtype=torch.long, device=DEV)
    out = cross_entropy(x, target, reduction="mean")
    out.backward()
    assert out.item() == 0.0
    assert torch.equal(x.grad, torch.zeros_like(x.grad))


# ================================================================================================
# RMSNorm / LayerNorm
# ================================================================================================
def _norm_fwd_bwd(tag, c, ln, with_res):
    ops = _ops()
    c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    x, w, b, eps = c["x"], c["w"], c["b"], c["eps"]
    res = c["res"] if with_res else None
    dres = c["dres"] if with_res else None
    y, rstd, mean, h = ops.norm_fwd(x, res, w, b, eps, ln)
    r_y, r_rstd, r_mean, r_h = R.norm_fwd_ref(x, res, w, b, eps, ln)
    b_y, b_rstd, b_mean, _ = R.norm_fwd_ref(x, res, w, b, eps, ln, dt=F32)
    _check(f"norm.y {tag}", y, r_y, b_y)
    _check(f"norm.rstd {tag}", rstd, r_rstd, b_rstd)
    if ln:
        _check(f"norm.mean {tag}", mean, r_mean, b_mean)
    else:
        assert mean.numel() == 0
    if with_res:
        assert torch.equal(h, r_h)
    else:
        assert h.numel() == 0
    # backward from the (fp32-rounded) reference statistics: the same inputs for kernel, baseline, reference
    rstd32 = r_rstd.float()
    mean32 = r_mean.float() if ln else None
    dx, dw, db = ops.norm_bwd(c["dy"], r_h, rstd32, mean32, w, dres, ln)
    r_dx, r_dw, r_db = R.norm_bwd_ref(c["dy"], r_h, rstd32, mean32, w, dres, ln)
    b_dx, b_dw, b_db = R.norm_bwd_ref(c["dy"], r_h, rstd32, mean32, w, dres, ln, dt=F32)
    _check(f"norm.dx {tag}", dx, r_dx, b_dx)
    assert dw.dtype == F32
    _check(f"norm.dw {tag}", dw, r_dw, b_dw)
    if ln:
        _check(f"norm.db {tag}", db, r_db, b_db)


_NORM_DT_H = [(d, H) for d in (torch.bfloat16, torch.float16) for H in R.NORM_HIDDEN] + [(F32, 64)]


@pytest.mark.parametrize("wf32", [True, False], ids=["w_fp32", "w_match"])
@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("rows", R.NORM_ROWS)
@pytest.mark.parametrize("dtype,H", _NORM_DT_H, ids=[f"{R.dtype_id(d)}-{H}" for d, H in _NORM_DT_H])
def test_norm_fwd_bwd(dtype, H, rows, ln, wf32):
    """rows=5 with H >= 1024: a block per row (1, 2 and 4 chunks per lane); otherwise a wave per row,
    exact-width at H=8192 and bounds-checked elsewhere. With a residual (+ bias, + dres) and without
    (LayerNorm then has bias=None)."""
    c = R.norm_case(rows, H, dtype, wf32, ln, bias=True)
    tag = f"{'ln' if ln else 'rms'} {rows}x{H} {R.dtype_id(dtype)} {'w32' if wf32 else 'wT'}"
    _norm_fwd_bwd(tag + " res", c, ln, True)
    c["b"] = None
    _norm_fwd_bwd(tag + " nores nobias", c, ln, False)


@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("rows,H", [(8197, 64), (2053, 64), (2053, 520)])
def test_norm_grid_stride(rows, H, ln):
    """8197 rows > 4 * 2048 forward blocks; 2053 rows > 4 * 512 backward blocks: a wave visits a second
    row and keeps adding into its dw/db registers before the LDS reduce."""
    c = R.norm_case(rows, H, torch.bfloat16, True, ln)
    _norm_fwd_bwd(f"stride {'ln' if ln else 'rms'} {rows}x{H}", c, ln, True)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("rows,H", [(300, 520), (5, 2056)])
def test_layernorm_large_offset(rows, H, dtype):
    """x = 1000 + randn: a one-pass E[x^2] - E[x]^2 variance would lose every digit."""
    c = R.norm_case(rows, H, dtype, True, True, offset=1000.0)
    _norm_fwd_bwd(f"ln offset1000 {rows}x{H} {R.dtype_id(dtype)}", c, True, False)


def test_norm_fwd_wide_few_rows():
    """8192 < H <= 16384 is served by the block-per-row forward when rows <= 256."""
    ops = _ops()
    for ln in (False, True):
        c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in R.norm_case(5, 12288, torch.bfloat16, True, ln).items()}
        y, rstd, mean, h = ops.norm_fwd(c["x"], c["res"], c["w"], c["b"], c["eps"], ln)
        r = R.norm_fwd_ref(c["x"], c["res"], c["w"], c["b"], c["eps"], ln)
        b = R.norm_fwd_ref(c["x"], c["res"], c["w"], c["b"], c["eps"], ln, dt=F32)
        _check(f"norm.y wide 5x12288 ln={ln}", y, r[0], b[0])
        _check(f"norm.rstd wide 5x12288 ln={ln}", rstd, r[1], b[1])
        assert torch.equal(h, r[3])


def test_norm_unsupported_sizes_raise():
    ops = _ops()

    def mk(rows, H):
        return torch.zeros(rows, H, device=DEV, dtype=torch.bfloat16), torch.ones(H, device=DEV)

    x, w = mk(4, 100)
    with pytest.raises(RuntimeError, match="norm_fwd: hidden size must be a multiple of 8"):
        ops.norm_fwd(x, None, w, None, 1e-5, False)
    x, w = mk(300, 12288)
    with pytest.raises(RuntimeError, match=r"norm_fwd: hidden size must be <= 8192 \(<= 16384 with at most 256 rows\)"):
        ops.norm_fwd(x, None, w, None, 1e-5, False)
    x, w = mk(2, 16392)
    with pytest.raises(RuntimeError, match="norm_fwd: hidden size must be <= 8192"):
        ops.norm_fwd(x, None, w, None, 1e-5, False)
    for rows, H in ((4, 100), (4, 12), (4, 12288)):
        x, w = mk(rows, H)
        rstd = torch.ones(rows, device=DEV)
        with pytest.raises(RuntimeError, match="norm_bwd: hidden size must be a multiple of 8 and <= 8192"):
            ops.norm_bwd(x, x, rstd, None, w, None, False)


@pytest.mark.parametrize("H", [100, 12288])
def test_rms_norm_unsupported_hidden_falls_back(H):
    """ops.norm.rms_norm / layer_norm at a hidden size the kernels do not take (not a multiple of 8;
    above 8192 with more than 256 rows) run the torch path, forward and backward."""
    from shuffle_exchange_amd.ops.norm import layer_norm, rms_norm
    c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in R.norm_case(300, H, torch.bfloat16, True, True).items()}
    for ln in (False, True):
        x = c["x"].clone().requires_grad_(True)
        w = c["w"].clone().requires_grad_(True)
        bb = c["b"].clone().requires_grad_(True) if ln else None
        y = layer_norm(x, w, bb, c["eps"]) if ln else rms_norm(x, w, c["eps"])
        y.backward(c["dy"])
        r = R.norm_fwd_ref(c["x"], None, c["w"], bb, c["eps"], ln)
        b = R.norm_fwd_ref(c["x"], None, c["w"], bb, c["eps"], ln, dt=F32)
        _check(f"norm.fallback y H={H} ln={ln}", y.detach(), r[0], b[0])
        rb = R.norm_bwd_ref(c["dy"], c["x"], r[1], r[2], c["w"], None, ln)
        bbk = R.norm_bwd_ref(c["dy"], c["x"], b[1], b[2], c["w"], None, ln, dt=F32)
        _check(f"norm.fallback dx H={H} ln={ln}", x.grad, rb[0], bbk[0])
        _check(f"norm.fallback dw H={H} ln={ln}", w.grad, rb[1], bbk[1])
        if ln:
            _check(f"norm.fallback db H={H} ln={ln}", bb.grad, rb[2], bbk[2])
    # with a residual the fallback also returns the new stream
    y, h = rms_norm(c["x"], c["w"], c["eps"], residual=c["res"])
    r = R.norm_fwd_ref(c["x"], c["res"], c["w"], None, c["eps"], False)
    b = R.norm_fwd_ref(c["x"], c["res"], c["w"], None, c["eps"], False, dt=F32)
    assert torch.equal(h, r[3])
    _check(f"norm.fallback y+res H={H}", y, r[0], b[0])


# ================================================================================================
# activations
# ================================================================================================
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("act", list(R.ACTS), ids=list(R.ACTS))
def test_gated_act(act, dtype):
    from shuffle_exchange_amd.ops.activation import gated_act
    ops, a = _ops(), R.ACTS[act]
    for rows, I in R.GATED_SHAPES:
        gu, dout = _cu(R.act_input((rows, 2 * I), dtype, seed=a), R.act_input((rows, I), dtype, seed=a + 50))
        tag = f"{act} {rows}x{I} {R.dtype_id(dtype)}"
        out = ops.gated_act_fwd(gu, a)
        _check(f"act.gated_fwd {tag}", out, R.gated_fwd_ref(gu, a), R.gated_fwd_ref(gu, a, dt=F32))
        dgu = ops.gated_act_bwd(dout, gu, a)
        _check(f"act.gated_bwd {tag}", dgu, R.gated_bwd_ref(dout, gu, a), R.gated_bwd_ref(dout, gu, a, dt=F32))
        # autograd through the wrapper runs the same two kernels
        x = gu.clone().requires_grad_(True)
        y = gated_act(x, act)
        y.backward(dout)
        assert torch.equal(y.detach(), out) and torch.equal(x.grad, dgu)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("act", list(R.ACTS), ids=list(R.ACTS))
def test_bias_act(act, dtype):
    from shuffle_exchange_amd.ops.activation import bias_act
    ops, a = _ops(), R.ACTS[act]
    for rows, C in R.BIAS_SHAPES:
        for with_bias in (True, False):
            x, dy = _cu(R.act_input((rows, C), dtype, seed=a + 7), R.act_input((rows, C), dtype, seed=a + 9))
            b = torch.randn(C, generator=torch.Generator().manual_seed(C)).to(dtype).to(DEV) if with_bias else None
            tag = f"{act} {rows}x{C} bias={with_bias} {R.dtype_id(dtype)}"
            y = ops.bias_act_fwd(x, b, a)
            _check(f"act.bias_fwd {tag}", y, R.bias_fwd_ref(x, b, a), R.bias_fwd_ref(x, b, a, dt=F32))
            dx = ops.bias_act_bwd(dy, x, b, a)
            _check(f"act.bias_bwd {tag}", dx, R.bias_bwd_ref(dy, x, b, a), R.bias_bwd_ref(dy, x, b, a, dt=F32))
            xa = x.clone().requires_grad_(True)
            ba = b.clone().requires_grad_(True) if with_bias else None
            ya = bias_act(xa, ba, act)
            ya.backward(dy)
            assert torch.equal(ya.detach(), y) and torch.equal(xa.grad, dx)
            if with_bias:  # the wrapper reduces the kernel's dx over the rows
                assert torch.equal(ba.grad, dx.float().sum(0).to(dtype))


def test_act_grid_stride():
    """2051 x 2064 / 8 = 529,158 work items > 2048 blocks x 256 threads: the last rows are a thread's
    second trip. The last row and its last 8-column chunk are checked on their own."""
    ops, a = _ops(), R.ACTS["silu"]
    rows, I = R.ACT_STRIDE_SHAPE
    g = torch.Generator().manual_seed(9)
    gu = (torch.randn(rows, 2 * I, generator=g) * 3).bfloat16().to(DEV)
    dout = torch.randn(rows, I, generator=g).bfloat16().to(DEV)
    out, dgu = ops.gated_act_fwd(gu, a), ops.gated_act_bwd(dout, gu, a)
    r_o, b_o = R.gated_fwd_ref(gu, a), R.gated_fwd_ref(gu, a, dt=F32)
    r_d, b_d = R.gated_bwd_ref(dout, gu, a), R.gated_bwd_ref(dout, gu, a, dt=F32)
    _check("act.gated_fwd stride 2051x2064", out, r_o, b_o)
    _check("act.gated_bwd stride 2051x2064", dgu, r_d, b_d)
    _check("act.gated_fwd stride last row", out[-1], r_o[-1], b_o[-1])
    _check("act.gated_fwd stride last chunk", out[-1, -8:], r_o[-1, -8:], b_o[-1, -8:])
    _check("act.gated_bwd stride last row", dgu[-1], r_d[-1], b_d[-1])
    _check("act.gated_bwd stride last chunk", dgu[-1, -8:], r_d[-1, -8:], b_d[-1, -8:])
    x = gu[:, :I].contiguous()
    b = torch.randn(I, generator=g).bfloat16().to(DEV)
    y, dx = ops.bias_act_fwd(x, b, a), ops.bias_act_bwd(dout, x, b, a)
    r_y, b_y = R.bias_fwd_ref(x, b, a), R.bias_fwd_ref(x, b, a, dt=F32)
    r_x, b_x = R.bias_bwd_ref(dout, x, b, a), R.bias_bwd_ref(dout, x, b, a, dt=F32)
    _check("act.bias_fwd stride 2051x2064", y, r_y, b_y)
    _check("act.bias_bwd stride 2051x2064", dx, r_x, b_x)
    _check("act.bias_fwd stride last chunk", y[-1, -8:], r_y[-1, -8:], b_y[-1, -8:])
    _check("act.bias_bwd stride last chunk", dx[-1, -8:], r_x[-1, -8:], b_x[-1, -8:])


def test_act_backward_shape_checks_raise():
    ops = _ops()
    gu = torch.zeros(3, 24, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="gated_act_bwd: inner size must be a multiple of 16"):
        ops.gated_act_bwd(torch.zeros(3, 12, device=DEV, dtype=torch.bfloat16), gu, 3)
    with pytest.raises(RuntimeError, match="gated_act_fwd: inner size must be a multiple of 16"):
        ops.gated_act_fwd(gu, 3)
    x = torch.zeros(3, 12, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="bias_act_bwd: numel % 8"):
        ops.bias_act_bwd(x, x, None, 3)
    x = torch.zeros(2, 12, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="bias_act_bwd: channels % 8"):
        ops.bias_act_bwd(x, x, None, 3)
    x = torch.zeros(2, 16, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="bias_act_bwd: bias"):
        ops.bias_act_bwd(x, x, torch.zeros(8, device=DEV, dtype=torch.bfloat16), 3)


# ================================================================================================
# RoPE
# ================================================================================================
def _rope_undo_bound(x, rd, dtype):
    """forward then inverse: each pass rounds once. With r = hypot(a, b) of a rotated pair, the forward
    leaves <= ulp(r)/2 on both components, the inverse mixes them (|cos| + |sin| <= sqrt 2) and rounds
    again: <= 1.21 ulp(r), plus the fp32 table's |cos^2 + sin^2 - 1| <= 4 * 2^-24 relative."""
    half = rd // 2
    xd = x.double()
    r = torch.hypot(xd[..., :half], xd[..., half:rd])
    r = torch.cat([r, r], dim=-1)
    return 1.25 * _ulp(r, dtype) + 4 * 2.0 ** -24 * r


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("D", R.ROPE_DIMS)
def test_rope_direct_positions(D, dtype):
    """rope_ on the first 3 of 5 heads with shuffled, repeated positions; then the inverse."""
    ops = _ops()
    T, heads, n_rot = 11, 5, 3
    x0, pos = _cu(R.rope_case(T, heads, D, dtype), R.rope_positions(T))
    cos, sin = _cu(*R.rope_tables(D, R.ROPE_MAX_POS))
    x = x0.clone()
    ops.rope_(x.unsqueeze(0)[:, :, :n_rot], cos, sin, pos, T, 0, False)
    _check(f"rope.fwd D={D} {R.dtype_id(dtype)}", x, R.rope_ref(x0, cos, sin, pos, n_rot), R.rope_ref(x0, cos, sin, pos, n_rot, dt=F32))
    assert torch.equal(x[:, n_rot:], x0[:, n_rot:])
    y = x.clone()
    ops.rope_(y.unsqueeze(0)[:, :, :n_rot], cos, sin, pos, T, 0, True)
    _check(f"rope.inv D={D} {R.dtype_id(dtype)}", y, R.rope_ref(x, cos, sin, pos, n_rot, inverse=True),
           R.rope_ref(x, cos, sin, pos, n_rot, inverse=True, dt=F32))
    assert torch.equal(y[:, n_rot:], x0[:, n_rot:])
    err = (y.double() - x0.double()).abs()[:, :n_rot]
    assert (err <= _rope_undo_bound(x0[:, :n_rot], D, dtype)).all()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
def test_rope_seq_len_pos_offset(dtype):
    ops = _ops()
    B, S, heads, D, off = 2, 7, 4, 64, 5
    x0 = R.rope_case(B * S, heads, D, dtype, seed=3).to(DEV)
    cos, sin = _cu(*R.rope_tables(D, R.ROPE_MAX_POS))
    pos = (torch.arange(S, device=DEV) + off).repeat(B)
    x = x0.clone()
    ops.rope_(x.view(B, S, heads, D), cos, sin, None, S, off, False)
    _check(f"rope.fwd offset {R.dtype_id(dtype)}", x, R.rope_ref(x0, cos, sin, pos), R.rope_ref(x0, cos, sin, pos, dt=F32))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("D,rd", R.ROPE_PARTIAL)
def test_rope_partial_rotary_tokens(D, rd, dtype):
    """apply_rope_tokens_: only the first rd dims of the first n_rot heads change (head_stride > rd)."""
    from shuffle_exchange_amd.ops.rope import RopeCache, apply_rope_tokens_
    T, heads, n_rot = 13, 6, 4
    x0, pos = _cu(R.rope_case(T, heads, D, dtype, seed=5), R.rope_positions(T))
    cache = RopeCache(rd, R.ROPE_MAX_POS, device=DEV)
    cos, sin = _cu(*R.rope_tables(rd, R.ROPE_MAX_POS))
    assert torch.equal(cache.cos, cos) and torch.equal(cache.sin, sin)
    x = x0.clone()
    out = apply_rope_tokens_(x, cache, n_rot, pos, rot_dim=rd)
    assert out.data_ptr() == x.data_ptr()
    _check(f"rope.partial D={D} rd={rd} {R.dtype_id(dtype)}", x, R.rope_ref(x0, cos, sin, pos, n_rot, rd),
           R.rope_ref(x0, cos, sin, pos, n_rot, rd, dt=F32))
    assert torch.equal(x[:, n_rot:], x0[:, n_rot:]) and torch.equal(x[:, :, rd:], x0[:, :, rd:])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
def test_rope_qkv_autograd(dtype):
    """apply_rope_qkv_ rotates q and k heads in place and leaves v; its gradient is the inverse rotation
    of the upstream gradient. apply_rope is the out-of-place form."""
    from shuffle_exchange_amd.ops.rope import RopeCache, apply_rope, apply_rope_qkv_
    B, S, nq, nkv, D = 2, 6, 4, 2, 64
    Ht, n_rot = nq + 2 * nkv, nq + nkv
    cache = RopeCache(D, R.ROPE_MAX_POS, device=DEV)
    pos = R.rope_positions(B * S).to(DEV)
    x0 = R.rope_case(B * S, Ht, D, dtype, seed=8).to(DEV)
    g0 = R.rope_case(B * S, Ht, D, dtype, seed=9).to(DEV)
    leaf = x0.view(B, S, Ht, D).clone().requires_grad_(True)
    out = apply_rope_qkv_(leaf * 1, cache, n_rot, position_ids=pos.view(B, S))
    out.backward(g0.view(B, S, Ht, D))
    _check(f"rope.qkv fwd {R.dtype_id(dtype)}", out.detach().view(B * S, Ht, D), R.rope_ref(x0, cache.cos, cache.sin, pos, n_rot),
           R.rope_ref(x0, cache.cos, cache.sin, pos, n_rot, dt=F32))
    assert torch.equal(out.detach()[:, :, n_rot:], x0.view(B, S, Ht, D)[:, :, n_rot:])
    _check(f"rope.qkv grad {R.dtype_id(dtype)}", leaf.grad.view(B * S, Ht, D),
           R.rope_ref(g0, cache.cos, cache.sin, pos, n_rot, inverse=True),
           R.rope_ref(g0, cache.cos, cache.sin, pos, n_rot, inverse=True, dt=F32))
    assert torch.equal(leaf.grad[:, :, n_rot:], g0.view(B, S, Ht, D)[:, :, n_rot:])
    # out of place, seq_len / pos_offset form
    x = x0.view(B, S, Ht, D).clone()
    y = apply_rope(x, cache, pos_offset=5)
    assert torch.equal(x, x0.view(B, S, Ht, D))
    p2 = (torch.arange(S, device=DEV) + 5).repeat(B)
    _check(f"rope.apply_rope {R.dtype_id(dtype)}", y.view(B * S, Ht, D), R.rope_ref(x0, cache.cos, cache.sin, p2),
           R.rope_ref(x0, cache.cos, cache.sin, p2, dt=F32))


def test_rope_grid_stride():
    """4100 tokens x 8 heads x 256/16 = 524,800 work items > 2048 blocks x 256 threads."""
    ops = _ops()
    T, heads, D = 4100, 8, 256
    g = torch.Generator().manual_seed(12)
    x0 = torch.randn(T, heads, D, generator=g).bfloat16().to(DEV)
    pos = torch.randint(0, R.ROPE_MAX_POS, (T,), generator=g).to(DEV)
    cos, sin = _cu(*R.rope_tables(D, R.ROPE_MAX_POS))
    x = x0.clone()
    ops.rope_(x.unsqueeze(0), cos, sin, pos, T, 0, False)
    r, b = R.rope_ref(x0, cos, sin, pos), R.rope_ref(x0, cos, sin, pos, dt=F32)
    _check("rope.fwd stride 4100x8x256", x, r, b)
    _check("rope.fwd stride last token", x[-1], r[-1], b[-1])


def test_rope_host_checks_raise():
    ops = _ops()
    T = 6
    cos, sin = _cu(*R.rope_tables(32, 16))
    pos = torch.arange(T, device=DEV)

    def x(D, heads=2):
        return torch.zeros(1, T, heads, D, device=DEV, dtype=torch.bfloat16)

    with pytest.raises(RuntimeError, match="head dim must be a multiple of 16"):
        ops.rope_(x(24), cos, sin, pos, T, 0, False)
    with pytest.raises(RuntimeError, match=r"cos/sin tables must be fp32 \[max_pos, D/2\]"):
        ops.rope_(x(64), cos, sin, pos, T, 0, False)
    with pytest.raises(RuntimeError, match="table too short for seq_len"):
        ops.rope_(x(32), cos, sin, None, T, 11, False)
    with pytest.raises(RuntimeError, match=r"pos must be int64 \[tokens\]"):
        ops.rope_(x(32), cos, sin, pos[:-1], T, 0, False)
    buf = torch.zeros(T * 68 + 64, device=DEV, dtype=torch.bfloat16)
    odd = buf.as_strided((1, T, 2, 32), (T * 68, 68, 32, 1))
    with pytest.raises(RuntimeError, match="token stride must be a multiple of 8 elements"):
        ops.rope_(odd, cos, sin, pos, T, 0, False)


# ================================================================================================
# masked softmax
# ================================================================================================
def _softmax_case(tag, s, kw):
    ops = _ops()
    kw = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}
    mask = kw.get("mask")
    if mask is not None and mask.dtype != torch.bool:
        mask = mask.float()
    out = ops.masked_softmax(s, float(kw.get("scale", 1.0)), mask, kw.get("alibi"), bool(kw.get("causal", False)),
                             int(kw.get("window", 0)))
    ref, base = R.softmax_ref(s, **kw), R.softmax_ref(s, dt=F32, **kw)
    assert out.dtype == s.dtype
    _check(f"softmax {tag}", out, ref, base)
    dead = ref.sum(-1) == 0
    assert torch.equal(out[dead], torch.zeros_like(out[dead]))
    if (~dead).any():
        # each element is rounded once (<= eps/2 relative), so a live row sums to 1 within eps of a
        # 16-bit output dtype. fp32: __expf (2 ulp) + its argument rounding (sum p_j |v_j - m| ulp, ~3)
        # + the multiply by 1/l + the rounding of 1/l: ~7 * 2^-24 relative, bound 8 * 2^-23
        eps = torch.finfo(s.dtype).eps * (8.0 if s.dtype == F32 else 1.0)
        sums = (out[~dead].double().sum(-1) - 1).abs()
        print(f"[row-sum] {tag} {R.dtype_id(s.dtype)} max|sum-1|={sums.max().item():.3e} bound={eps:.3e}")
        assert (sums <= eps).all()
    return out, ref, kw


_SMX_QK = [(q, k) for k in R.SOFTMAX_K for q in R.SOFTMAX_Q] + [(5, 5), (5, 3)]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("Q,K", _SMX_QK, ids=[f"q{q}k{k}" for q, k in _SMX_QK])
def test_masked_softmax_edges(Q, K, dtype):
    from shuffle_exchange_amd.ops import inference_ops
    B, H = 2, 3
    s = R.softmax_scores(B, H, Q, K, dtype).to(DEV)
    for name, kw in R.softmax_variants(B, H, Q, K, dtype).items():
        out, ref, kwd = _softmax_case(f"{name} q{Q}k{K} {R.dtype_id(dtype)}", s, kw)
        if name == "causal" and Q > K:
            assert (out[:, :, :Q - K] == 0).all()  # queries before the first key see nothing
        if name == "window1":
            assert int((out != 0).sum()) == B * H * min(Q, K) and ((out == 0) | (out == 1)).all()
        if name in ("add_inf", "bool_causal_alibi", "window1"):
            via = inference_ops.softmax(s, attn_mask=kwd.get("mask"), alibi=kwd.get("alibi"),
                                        triangular=kwd.get("causal", False), local_attention=kwd.get("window", 0) > 0,
                                        window_size=kwd.get("window", 1), layer_scale=kwd.get("scale", 1.0))
            assert torch.equal(via, out)


@pytest.mark.parametrize("causal", [False, True])
def test_masked_softmax_grid_stride(causal):
    """B*H*Q = 16,400 rows > 4 rows x 4096 blocks."""
    B, H, Q, K = 8, 41, 50, 8
    g = torch.Generator().manual_seed(21)
    s = (torch.randn(B, H, Q, K, generator=g) * 3).bfloat16().to(DEV)
    pad = torch.rand(B, 1, 1, K, generator=g) > 0.3
    pad[:, :, :, K - 1] = True
    out, ref, _ = _softmax_case(f"stride 16400x8 causal={causal}", s, dict(mask=pad, causal=causal))
    assert (ref[-1, -1, -1].sum() - 1).abs() < 1e-12 and (out[-1, -1, -1].double().sum() - 1).abs() <= 2 ** -7
