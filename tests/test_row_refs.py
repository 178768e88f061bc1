"""CPU checks of the float64 references in tests/_row_refs.py against torch's own builtins, on the case
tables the GPU tests (tests/test_row_kernels_gpu.py) use. Every reference output must also be finite,
the -inf cross-entropy and softmax cases included: the oracle is checked without a GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import _row_refs as R

F64 = torch.float64
TOL = dict(rtol=1e-12, atol=1e-13)
# derivatives: the GELU forms subtract O(1) terms in the tails, so float64 leaves ~1e-16 * |dy * u| absolute
DTOL = dict(rtol=1e-10, atol=1e-13)


def _finite(*ts):
    for t in ts:
        if t is not None:
            assert torch.isfinite(t).all()


def _xent_cases():
    for V in R.XENT_VOCABS:
        for ts in R.XENT_TSETS:
            yield f"rand-{V}-{ts}", lambda V=V, ts=ts: R.xent_case(V, torch.bfloat16, ts)
    for V in (2048, 1001):
        yield f"extreme-{V}", lambda V=V: R.xent_extreme_case(V, torch.float16)
    for pat in R.XENT_INF:
        for vec in (True, False):
            yield f"inf-{pat}-{'vec' if vec else 'scalar'}", lambda pat=pat, vec=vec: R.xent_inf_case(pat, vec, torch.bfloat16)
    yield "stride", lambda: R.xent_stride_case(torch.bfloat16)
    yield "dual-inf", R.xent_dual_inf_case


@pytest.mark.parametrize("name,make", list(_xent_cases()), ids=[n for n, _ in _xent_cases()])
def test_xent_ref_vs_torch(name, make):
    logits, target, ign = make()
    loss, lse, grad = R.xent_ref(logits, target, ign)
    _finite(loss, lse, grad)
    x = logits.double().requires_grad_(True)
    want = F.cross_entropy(x, target, ignore_index=ign, reduction="none")
    torch.testing.assert_close(loss, want.detach(), **TOL)
    torch.testing.assert_close(lse, torch.logsumexp(logits.double(), -1), **TOL)
    dloss = torch.linspace(0.5, 2.0, logits.shape[0], dtype=F64)
    (gx,) = torch.autograd.grad(want, x, dloss)
    _, _, g2 = R.xent_ref(logits, target, ign, scale=dloss)
    torch.testing.assert_close(g2, gx, **TOL)
    live = target != ign
    assert (loss[~live] == 0).all() and (grad[~live] == 0).all()
    assert (grad[logits.double() == R.NEG_INF] == 0).all()
    # gradient position: p - 1 on the target column, p elsewhere
    p = torch.softmax(logits.double(), -1)
    for r in torch.nonzero(live).flatten().tolist()[:4]:
        t = int(target[r])
        torch.testing.assert_close(grad[r, t], p[r, t] - 1.0, **TOL)
        assert grad[r, t] <= 0 and (grad[r, :t] >= 0).all() and (grad[r, t + 1:] >= 0).all()


def test_xent_ref_all_ignored():
    logits = torch.randn(3, 16).bfloat16()
    target = torch.full((3,), -100, dtype=torch.long)
    loss, lse, grad = R.xent_ref(logits, target, -100)
    _finite(loss, lse, grad)
    assert (loss == 0).all() and (grad == 0).all()


@pytest.mark.parametrize("ln", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("H", R.NORM_HIDDEN)
@pytest.mark.parametrize("rows", [5, 37])
def test_norm_ref_vs_torch(rows, H, ln):
    c = R.norm_case(rows, H, torch.bfloat16, True, ln, bias=(H != 64), offset=1000.0 if H == 520 else 0.0)
    y, rstd, mean, h = R.norm_fwd_ref(c["x"], c["res"], c["w"], c["b"], c["eps"], ln)
    _finite(y, rstd, mean)
    assert torch.equal(h, (c["x"].double() + c["res"].double()).bfloat16())
    hr = h.double().requires_grad_(True)
    wr = c["w"].double().requires_grad_(True)
    br = c["b"].double().requires_grad_(True) if c["b"] is not None else None
    if ln:
        want = F.layer_norm(hr, (H,), wr, br, c["eps"])
    else:
        want = hr * torch.rsqrt(hr.pow(2).mean(-1, keepdim=True) + c["eps"]) * wr
    torch.testing.assert_close(y, want.detach(), rtol=1e-10, atol=1e-10)
    dx, dw, db = R.norm_bwd_ref(c["dy"], h, rstd, mean, c["w"], c["dres"], ln)
    _finite(dx, dw, db)
    ins = (hr, wr) + ((br,) if br is not None else ())
    gs = torch.autograd.grad(want, ins, c["dy"].double())
    torch.testing.assert_close(dx, gs[0] + c["dres"].double(), rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(dw, gs[1], rtol=1e-9, atol=1e-9)
    if br is not None:
        torch.testing.assert_close(db, gs[2], rtol=1e-9, atol=1e-9)
    # without a residual the input itself is normalised
    y2, _, _, h2 = R.norm_fwd_ref(c["x"], None, c["w"], c["b"], c["eps"], ln)
    assert h2 is c["x"]
    _finite(y2)


def _torch_act(x, act):
    return {0: lambda v: v, 1: torch.relu, 2: lambda v: F.gelu(v, approximate="tanh"), 3: F.silu, 4: F.gelu,
            5: lambda v: v * torch.sigmoid(1.702 * v)}[act](x)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.dtype_id)
@pytest.mark.parametrize("act", list(R.ACTS.values()), ids=list(R.ACTS))
def test_act_ref_vs_autograd(act, dtype):
    for rows, I in R.GATED_SHAPES:
        gu = R.act_input((rows, 2 * I), dtype, seed=act)
        dout = R.act_input((rows, I), dtype, seed=act + 50)
        x = gu.double().requires_grad_(True)
        g, u = x.chunk(2, dim=-1)
        want = _torch_act(g, act) * u
        out = R.gated_fwd_ref(gu, act)
        dgu = R.gated_bwd_ref(dout, gu, act)
        _finite(out, dgu)
        torch.testing.assert_close(out, want.detach(), rtol=1e-12, atol=1e-15)  # 1 + tanh / 1 + erf cancel in the negative tail
        (gx,) = torch.autograd.grad(want, x, dout.double())
        torch.testing.assert_close(dgu, gx, **DTOL)
    for rows, C in R.BIAS_SHAPES:
        for with_bias in (True, False):
            xb = R.act_input((rows, C), dtype, seed=act + 7)
            b = torch.randn(C, generator=torch.Generator().manual_seed(C)).to(dtype) if with_bias else None
            dy = R.act_input((rows, C), dtype, seed=act + 9)
            x = xb.double().requires_grad_(True)
            want = _torch_act(x + (b.double() if b is not None else 0.0), act)
            y = R.bias_fwd_ref(xb, b, act)
            dx = R.bias_bwd_ref(dy, xb, b, act)
            _finite(y, dx)
            torch.testing.assert_close(y, want.detach(), rtol=1e-12, atol=1e-15)  # 1 + tanh / 1 + erf cancel in the negative tail
            (gx,) = torch.autograd.grad(want, x, dy.double())
            torch.testing.assert_close(dx, gx, **DTOL)


@pytest.mark.parametrize("D,rd", [(d, d) for d in R.ROPE_DIMS] + R.ROPE_PARTIAL)
def test_rope_ref(D, rd):
    T, heads, n_rot = 11, 5, 3
    x = R.rope_case(T, heads, D, torch.bfloat16)
    cos, sin = R.rope_tables(rd, R.ROPE_MAX_POS)
    pos = R.rope_positions(T)
    assert int(pos.min()) == 0 and int(pos.max()) == R.ROPE_MAX_POS - 1 and pos.unique().numel() < T
    y = R.rope_ref(x, cos, sin, pos, n_rot, rd)
    _finite(y)
    xd = x.double()
    assert torch.equal(y[:, n_rot:], xd[:, n_rot:]) and torch.equal(y[:, :, rd:], xd[:, :, rd:])
    # the rotation as a complex multiply: (a + ib) * (cos + i sin)
    half = rd // 2
    z = torch.complex(xd[:, :n_rot, :half], xd[:, :n_rot, half:rd])
    w = torch.polar(torch.ones(T, half, dtype=F64), torch.atan2(sin.double(), cos.double())[pos])[:, None, :]
    zr = z * w
    torch.testing.assert_close(y[:, :n_rot, :half], zr.real, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(y[:, :n_rot, half:rd], zr.imag, rtol=1e-6, atol=1e-6)
    # the inverse undoes it (to the fp32 table's cos^2 + sin^2 - 1), and norms are preserved
    back = R.rope_ref(y, cos, sin, pos, n_rot, rd, inverse=True)
    torch.testing.assert_close(back, xd, rtol=1e-6, atol=1e-6)
    # position 0 is the identity
    t0 = int(torch.nonzero(pos == 0)[0])
    assert torch.equal(y[t0], xd[t0])


@pytest.mark.parametrize("Q,K", [(q, k) for k in R.SOFTMAX_K for q in R.SOFTMAX_Q] + [(5, 5), (5, 3)])
def test_softmax_ref_vs_torch(Q, K):
    B, H = 2, 3
    s = R.softmax_scores(B, H, Q, K, torch.bfloat16)
    for name, kw in R.softmax_variants(B, H, Q, K, torch.bfloat16).items():
        out = R.softmax_ref(s, **kw)
        _finite(out)
        t = s.double() * kw.get("scale", 1.0)
        if kw.get("alibi") is not None:
            t = t + kw["alibi"].double()
        keep = torch.ones(B, H, Q, K, dtype=torch.bool)
        m = kw.get("mask")
        if m is not None and m.dtype == torch.bool:
            keep &= m
        elif m is not None:
            t = t + m.double()
        q = torch.arange(K - Q, K)[:, None]
        k = torch.arange(K)[None, :]
        if kw.get("causal"):
            keep &= k <= q
        if kw.get("window", 0) > 0:
            keep &= k > q - kw["window"]
        want = torch.nan_to_num(torch.softmax(t.masked_fill(~keep, R.NEG_INF), -1), nan=0.0)
        torch.testing.assert_close(out, want, rtol=1e-12, atol=1e-15, msg=lambda m_, n=name: f"{n}: {m_}")
        dead = ~(keep & (t > R.NEG_INF)).any(-1)
        assert (out[dead] == 0).all()
        torch.testing.assert_close(out[~dead].sum(-1), torch.ones_like(out[~dead].sum(-1)), rtol=1e-12, atol=0)
        if name == "window1":
            idx = torch.arange(Q) + K - Q
            ok = idx >= 0
            diag = out[:, :, torch.arange(Q)[ok], idx[ok]]
            assert (diag == 1).all() and out.sum() == B * H * int(ok.sum())
        if name == "all_masked":
            assert (out == 0).all()
    if Q > K:
        out = R.softmax_ref(s, causal=True)
        assert (out[:, :, :Q - K] == 0).all() and (out[:, :, Q - K:].sum(-1) - 1).abs().max() < 1e-12
