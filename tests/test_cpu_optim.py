"""Host Lion / Adagrad / sumsq kernels (csrc/cpu/cpu_adam.cpp, AVX-512 / AVX2 / baseline clones), the
torch fallback branches of lion_flat_ / adagrad_flat_ and the FusedLion / FusedAdagrad front ends on
CPU tensors, element-wise against the float64 update (tests/_optim_ref.py), plus the input checks of
the host kernels: misuse must raise and leave every tensor untouched."""
import pytest
import torch

from shuffle_exchange_amd.ops import native
from shuffle_exchange_amd.ops import optim as fused

from . import _optim_ref as R

SIZES = [1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 123]  # SIMD-width and 4096-tile edges
LR, B1, B2, EPS = 1e-3, 0.9, 0.99, 1e-10
PLANT = (0, 5, 17, 4096)  # planted ties / zeros (those below n)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    R.report()


def _need_cpu():
    if not native.cpu_available():
        pytest.skip("native CPU extension not built")


def _inputs(n, seed=0):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.1
    return p, g, m


def _plant(n):
    return torch.tensor([i for i in PLANT if i < n], dtype=torch.long)


# ------------------------------------------------------------------------------------ host kernels
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("n", SIZES)
def test_cpu_lion_matches_fp64(n, wd):
    _need_cpu()
    p, g, m = _inputs(n)
    idx = _plant(n)
    g[idx] = 0.0
    m[idx] = 0.0  # exact ties: c == 0, u == 0, p -> p * (1 - lr * wd)
    for step in range(2):  # step 2 reads the state step 1 wrote
        if step == 1:
            g = torch.randn(n, generator=torch.Generator().manual_seed(7))
        rp, rm, c = R.lion_ref(p, g, m, lr=LR, beta1=B1, beta2=B2, weight_decay=wd)
        if step == 0:
            assert (c[idx] == 0).all()
            torch.testing.assert_close(rp[idx], p[idx].double() * (1 - LR * wd), rtol=1e-14, atol=0)
        torch.ops.sxe_cpu.lion_step_(p, g, m, LR, B1, B2, wd)
        # worst observed over all sizes, both steps: 2.3e-7 abs, 0.04 of the tolerance; guard excluded 0
        R.check_lion_p("cpu lion_step_", p, rp, c)
        R.check("cpu lion_step_", "m", m, rm)


@pytest.mark.parametrize("n", [1, 17, 4097])
def test_cpu_lion_exact_cancellation_gives_zero_update(n):
    """beta1 = 0.5 and g = -m: c = 0.5*m - 0.5*m is exactly 0 in fp32 with or without FMA, so u = 0.
    A kernel that sends c == 0 to +1 or -1 moves every element by lr."""
    _need_cpu()
    p, _, m = _inputs(n)
    g = -m
    rp, rm, c = R.lion_ref(p, g, m, lr=LR, beta1=0.5, beta2=B2, weight_decay=0.1)
    assert (c == 0).all()
    torch.ops.sxe_cpu.lion_step_(p, g, m, LR, 0.5, B2, 0.1)
    assert R.check_lion_p("cpu lion_step_", p, rp, c) == 0
    R.check("cpu lion_step_", "m", m, rm)


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("n", SIZES)
def test_cpu_adagrad_matches_fp64(n, wd):
    _need_cpu()
    p, g, _ = _inputs(n)
    s = torch.rand(n, generator=torch.Generator().manual_seed(3)) * 0.01
    idx = _plant(n)
    p[idx] = 0.0
    g[idx] = 0.0
    s[idx] = 0.0  # 0 / (sqrt(0) + eps): p stays 0, no NaN
    for step in range(2):
        if step == 1:
            g = torch.randn(n, generator=torch.Generator().manual_seed(7))
        rp, rs = R.adagrad_ref(p, g, s, lr=LR, eps=EPS, weight_decay=wd)
        torch.ops.sxe_cpu.adagrad_step_(p, g, s, LR, EPS, wd)
        assert torch.isfinite(p).all() and torch.isfinite(s).all()
        if step == 0:
            assert (p[idx] == 0).all() and (s[idx] == 0).all()
        # worst observed over all sizes, both steps: 1.0e-6 abs (on s), 0.016 of the tolerance
        R.check("cpu adagrad_step_", "p", p, rp)
        R.check("cpu adagrad_step_", "s", s, rs)


@pytest.mark.parametrize("n", [1, 4097, 100003])
def test_cpu_sumsq_exact(n):
    """Integers in [-2, 2]: every partial sum is an integer <= 4n < 2^53, exact in any order."""
    _need_cpu()
    x = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(0)).float()
    x[-1] = 2.0  # a dropped last element changes the sum
    assert torch.ops.sxe_cpu.sumsq(x) == x.double().pow(2).sum().item()


def test_cpu_sumsq_propagates_inf():
    _need_cpu()
    x = torch.ones(4097)
    x[4096] = float("inf")
    assert torch.ops.sxe_cpu.sumsq(x) == float("inf")


# ------------------------------------------------------------------------- torch fallback branches
def _lp(n, dt):
    return None if dt is None else torch.full((n,), 7.0, dtype=dt)


@pytest.mark.parametrize("lpdt", [None, torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_lion_flat_torch_branch(gdt, lpdt):
    n = 1027
    p, g, m = _inputs(n)
    g = g.to(gdt)
    idx = _plant(n)
    g[idx] = 0.0
    m[idx] = 0.0
    lp = _lp(n, lpdt)
    scale = torch.tensor([0.5])
    rp, rm, c = R.lion_ref(p, g, m, lr=LR, beta1=B1, beta2=B2, weight_decay=0.1, gs=2.0 * 0.5)
    fused.lion_flat_(p, g, m, lp, lr=LR, beta1=B1, beta2=B2, weight_decay=0.1, grad_scale=2.0, scale_t=scale,
                     skip_t=torch.zeros(1))
    R.check_lion_p("torch lion_flat_", p, rp, c)
    R.check("torch lion_flat_", "m", m, rm)
    if lp is not None:
        assert torch.equal(lp, p.to(lpdt))


@pytest.mark.parametrize("lpdt", [None, torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_adagrad_flat_torch_branch(gdt, lpdt):
    n = 1027
    p, g, _ = _inputs(n)
    g = g.to(gdt)
    s = torch.rand(n, generator=torch.Generator().manual_seed(3)) * 0.01
    lp = _lp(n, lpdt)
    scale = torch.tensor([0.5])
    rp, rs = R.adagrad_ref(p, g, s, lr=LR, eps=EPS, weight_decay=0.1, gs=2.0 * 0.5)
    fused.adagrad_flat_(p, g, s, lp, lr=LR, eps=EPS, weight_decay=0.1, grad_scale=2.0, scale_t=scale,
                        skip_t=torch.zeros(1))
    R.check("torch adagrad_flat_", "p", p, rp)
    R.check("torch adagrad_flat_", "s", s, rs)
    if lp is not None:
        assert torch.equal(lp, p.to(lpdt))


def test_grad_scale_reaches_the_torch_branches():
    """grad_scale * scale_t = 4: Adagrad's state grows 16-fold; Lion's momentum takes 4 g."""
    n = 257
    p, g, m = _inputs(n)
    s = torch.zeros(n)
    rp, rs = R.adagrad_ref(p, g, s, lr=LR, eps=EPS, weight_decay=0.0, gs=4.0)
    pa = p.clone()
    fused.adagrad_flat_(pa, g, s, lr=LR, eps=EPS, grad_scale=2.0, scale_t=torch.tensor([2.0]))
    R.check("torch adagrad_flat_", "s", s, rs)
    R.check("torch adagrad_flat_", "p", pa, rp)
    rp, rm, c = R.lion_ref(p, g, m, lr=LR, beta1=B1, beta2=B2, weight_decay=0.0, gs=4.0)
    fused.lion_flat_(p, g, m, lr=LR, beta1=B1, beta2=B2, grad_scale=2.0, scale_t=torch.tensor([2.0]))
    R.check("torch lion_flat_", "m", m, rm)
    R.check_lion_p("torch lion_flat_", p, rp, c)


@pytest.mark.parametrize("which", ["lion", "adagrad"])
def test_skip_flag_leaves_the_torch_branches_untouched(which):
    n = 257
    p, g, m = _inputs(n)
    lp = torch.full((n,), 7.0, dtype=torch.bfloat16)
    before = [t.clone() for t in (p, g, m, lp)]
    if which == "lion":
        fused.lion_flat_(p, g, m, lp, lr=LR, weight_decay=0.1, skip_t=torch.ones(1))
    else:
        fused.adagrad_flat_(p, g, m, lp, lr=LR, weight_decay=0.1, skip_t=torch.ones(1))
    assert all(torch.equal(a, b) for a, b in zip((p, g, m, lp), before))


# ------------------------------------------------------------------------------------- front ends
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_lion_cpu(dtype):
    R.run_fused_lion(dtype, "cpu", "FusedLion cpu")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_adagrad_cpu(dtype):
    R.run_fused_adagrad(dtype, "cpu", "FusedAdagrad cpu")


# ----------------------------------------------------------------------------------------- misuse
def _misuse_cases(n=8):
    """name -> (p, g, state): each breaks one precondition of the host kernels."""
    f = lambda k=n: torch.arange(k, dtype=torch.float32) + 1.0  # noqa: E731
    return {
        "noncontiguous_p": (f(2 * n)[::2], f(), f()),
        "noncontiguous_state": (f(), f(), f(2 * n)[::2]),
        "noncontiguous_grad": (f(), f(2 * n)[::2], f()),
        "grad_numel": (f(), f(n + 4), f()),
        "state_numel": (f(), f(), f(n + 4)),
        "p_numel": (f(n + 4), f(), f()),
        "bf16_master": (f().bfloat16(), f(), f()),
        "f64_state": (f(), f(), f().double()),
        "bf16_grad": (f(), f().bfloat16(), f()),
    }


@pytest.mark.parametrize("case", sorted(_misuse_cases()))
@pytest.mark.parametrize("op", ["lion", "adagrad"])
def test_cpu_kernels_reject_misuse(op, case):
    _need_cpu()
    p, g, s = _misuse_cases()[case]
    bases = [t._base if t._base is not None else t for t in (p, g, s)]
    before = [b.clone() for b in bases]
    with pytest.raises(RuntimeError):
        if op == "lion":
            torch.ops.sxe_cpu.lion_step_(p, g, s, LR, B1, B2, 0.1)
        else:
            torch.ops.sxe_cpu.adagrad_step_(p, g, s, LR, EPS, 0.1)
    assert all(torch.equal(a, b) for a, b in zip(bases, before))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["p", "g", "state"])
@pytest.mark.parametrize("op", ["lion", "adagrad"])
def test_cpu_kernels_reject_gpu_tensors(op, where):
    _need_cpu()
    ts = {k: torch.ones(8) for k in ("p", "g", "state")}
    ts[where] = ts[where].cuda()
    before = {k: t.clone() for k, t in ts.items()}
    with pytest.raises(RuntimeError):
        if op == "lion":
            torch.ops.sxe_cpu.lion_step_(ts["p"], ts["g"], ts["state"], LR, B1, B2, 0.1)
        else:
            torch.ops.sxe_cpu.adagrad_step_(ts["p"], ts["g"], ts["state"], LR, EPS, 0.1)
    assert all(torch.equal(ts[k], before[k]) for k in ts)
