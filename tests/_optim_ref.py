"""float64 references of the optimizer updates (Adam/AdamW, Lion, Adagrad) and the element-wise
comparison shared by test_cpu_optim.py and test_optim_kernels_gpu.py.

Every reference is computed from the values actually stored in its inputs: a bf16 / fp16 gradient
is upcast exactly, then multiplied by ``gs`` (grad_scale * scale_t, both powers of two in the tests,
so their fp32 product is exact). Formulas: header comments of csrc/kernels/optim.hip."""
import math

import torch

RTOL, ATOL = 1e-5, 1e-6  # the project's tolerance for this class of kernel (tests/test_cpu_adam.py)
LION_GUARD = 1e-6        # p is compared where the fp64 c = b1*m + (1-b1)*g has |c| >= guard, or c == 0
LION_MAX_EXCLUDED = 1e-3  # cap on the share of elements the guard may exclude

WORST = {}  # kernel name -> [max abs error, max error / (ATOL + RTOL*|ref|), excluded by the Lion guard]


def adam_ref(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, adamw, bias_correction, gs=1.0):
    p, g, m, v = p.double(), g.double() * gs, m.double(), v.double()
    if not adamw:
        g = g + weight_decay * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step if bias_correction else 1.0
    bc2 = 1 - beta2 ** step if bias_correction else 1.0
    denom = v.sqrt() / math.sqrt(bc2) + eps
    if adamw:
        p = p - lr * weight_decay * p
    return p - (lr / bc1) * m / denom, m, v


def lion_ref(p, g, m, *, lr, beta1, beta2, weight_decay, gs=1.0):
    """Returns (p, m, c): c is the fp64 argument of sign()."""
    p, g, m = p.double(), g.double() * gs, m.double()
    c = beta1 * m + (1 - beta1) * g
    return p - lr * (c.sign() + weight_decay * p), beta2 * m + (1 - beta2) * g, c


def adagrad_ref(p, g, s, *, lr, eps, weight_decay, gs=1.0):
    p, s = p.double(), s.double()
    g = g.double() * gs + weight_decay * p
    s = s + g * g
    return p - lr * g / (s.sqrt() + eps), s


def _record(kernel, got, ref, excluded=0):
    err = (got.double() - ref).abs()
    w = WORST.setdefault(kernel, [0.0, 0.0, 0])
    if err.numel():
        w[0] = max(w[0], err.max().item())
        w[1] = max(w[1], (err / (ATOL + RTOL * ref.abs())).max().item())
    w[2] += int(excluded)


def check(kernel, what, got, ref):
    """Element-wise got (fp32) vs ref (fp64) at the shared tolerance; records the worst error."""
    assert got.dtype == torch.float32 and ref.dtype == torch.float64
    _record(kernel, got, ref)
    torch.testing.assert_close(got, ref, rtol=RTOL, atol=ATOL, check_dtype=False, msg=lambda m: f"{kernel} {what}: {m}")


def check_lion_p(kernel, got, ref, c):
    """Lion's p: sign(c) is discontinuous at 0, so elements with 0 < |c| < LION_GUARD are left out
    (at most LION_MAX_EXCLUDED of them); an exact c == 0 (u = 0) is compared like any other."""
    keep = (c.abs() >= LION_GUARD) | (c == 0)
    excluded = int((~keep).sum())
    assert excluded <= LION_MAX_EXCLUDED * c.numel(), f"{kernel}: sign guard excludes {excluded} of {c.numel()}"
    _record(kernel, got[keep], ref[keep], excluded)
    torch.testing.assert_close(got[keep], ref[keep], rtol=RTOL, atol=ATOL, check_dtype=False,
                               msg=lambda m: f"{kernel} p: {m}")
    return excluded


# ------------------------------------------------------------------------------------- front ends
SHAPES = [(3,), (17, 5), (257, 64)]


def _params(dtype, device="cpu"):
    gen = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, generator=gen).to(dtype).to(device)) for s in SHAPES]


def _grads(step, dtype, device="cpu"):
    gen = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=gen).to(dtype).to(device) for s in SHAPES]


def run_fused_lion(dtype, device, kernel):
    """3 steps of FusedLion; every step is judged against the fp64 update of the state it started
    from (fp32 parameters: the parameter itself; bit16: the fp32 master, and p == master cast)."""
    from shuffle_exchange_amd.ops import optim as fused
    LR, B1, B2 = 1e-3, 0.9, 0.99
    ps = _params(dtype, device)
    opt = fused.FusedLion(ps, lr=LR, betas=(B1, B2), weight_decay=0.1)
    for step in range(3):
        gs = _grads(step, dtype, device)
        before = []
        for p, g in zip(ps, gs):
            p.grad = g
            st = opt.state[p]
            master = st["master_param"] if st and st["master_param"] is not None else p.detach().float()
            m = st["exp_avg"] if st else torch.zeros(p.shape, device=device)
            before.append(lion_ref(master.reshape(-1), g.reshape(-1), m.reshape(-1), lr=LR, beta1=B1, beta2=B2,
                                   weight_decay=0.1))
        opt.step()
        for p, (rp, rm, c) in zip(ps, before):
            st = opt.state[p]
            master = st["master_param"] if st["master_param"] is not None else p.detach()
            check_lion_p(kernel, master.reshape(-1), rp, c)
            check(kernel, "m", st["exp_avg"].reshape(-1), rm)
            if dtype != torch.float32:
                assert torch.equal(p.detach(), master.to(dtype))


def run_fused_adagrad(dtype, device, kernel):
    """3 steps of FusedAdagrad against torch.optim.Adagrad (same formula) on fp32 copies; for bit16
    parameters the fp32 master is what is compared, and p == master cast."""
    ps = _params(dtype, device)
    from shuffle_exchange_amd.ops import optim as fused
    EPS = 1e-10
    ref = [torch.nn.Parameter(p.detach().float().cpu().clone()) for p in ps]
    opt = fused.FusedAdagrad(ps, lr=1e-2, eps=EPS, weight_decay=0.1)
    ropt = torch.optim.Adagrad(ref, lr=1e-2, eps=EPS, weight_decay=0.1)
    for step in range(3):
        for p, r, g in zip(ps, ref, _grads(step, dtype, device)):
            p.grad = g
            r.grad = g.float().cpu()
        opt.step()
        ropt.step()
    for p, r in zip(ps, ref):
        st = opt.state[p]
        master = st["master_param"] if st["master_param"] is not None else p.detach()
        torch.testing.assert_close(master.cpu(), r.detach(), rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(st["exp_avg_sq"].cpu(), ropt.state[r]["sum"], rtol=RTOL, atol=ATOL)
        if dtype != torch.float32:
            assert torch.equal(p.detach(), master.to(dtype))


def report():
    for k in sorted(WORST):
        a, r, x = WORST[k]
        print(f"[optim-ref] {k}: worst abs err {a:.3e}, worst err/tolerance {r:.3f}, sign-guard excluded {x}")
