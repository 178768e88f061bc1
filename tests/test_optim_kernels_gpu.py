"""The optimizer HIP kernels of csrc/kernels/optim.hip (lion_flat_, adagrad_flat_, adam_flat_,
multi_tensor_adam_, sumsq), the FusedLion / FusedAdagrad front ends and the ZeRO Lion / Adagrad
branches on one MI355X: element-wise against the float64 update (tests/_optim_ref.py) at the sizes
where each code path can go wrong, plus the entry points' input checks (MI355X only)."""
import functools

import pytest
import torch

from . import _dist_cases as C
from . import _optim_ref as R
from .dist_utils import run_dist

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
GDT = [F32, BF16, F16]
LPDT = [None, BF16, F16, F32]
# stream_grid caps the grid at kNumCUs * 8 blocks of 256 threads; kNumCUs = 256 (csrc/include/sxe_common.h)
GRID_CAP = 256 * 8
LR, B1, B2 = 1e-3, 0.9, 0.99
GS, SCALE_T = 2.0, 0.5  # grad_scale (host) and scale_t (device): powers of two, the fp32 product is exact


@pytest.fixture(scope="module", autouse=True)
def _native():
    from shuffle_exchange_amd.ops import native
    native.require_hip()
    yield
    R.report()


@functools.lru_cache(maxsize=None)
def _host_inputs(n):
    """(p, g, m, v) ~ (N(0,1), N(0,1), 0.1 N(0,1), 0.01 U(0,1)), seed 0, built once per size."""
    gen = torch.Generator().manual_seed(0)
    return (torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1,
            torch.rand(n, generator=gen) * 0.01)


def _inputs(n, gdt):
    p, g, m, v = (t.cuda() for t in _host_inputs(n))
    return p, g.to(gdt), m, v


def _lp(n, dt):
    return None if dt is None else torch.full((n,), 7.0, dtype=dt, device="cuda")  # 7: sentinel


def _plant(n):
    return torch.tensor([i for i in (0, 2, 255, 256, 1026) if i < n], dtype=torch.long, device="cuda")


def _flags(skip=0.0):
    return torch.tensor([SCALE_T], device="cuda"), torch.tensor([skip], device="cuda")


# ---------------------------------------------------------------------------- lion_flat_ / adagrad_flat_
# one element per thread: block edges, and one size past the grid cap so the grid-stride loop runs twice
FLAT_SIZES = [1, 3, 255, 256, 257, 1027, GRID_CAP * 256 + 257]


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("lpdt", LPDT, ids=str)
@pytest.mark.parametrize("gdt", GDT, ids=str)
def test_lion_flat(gdt, lpdt, wd):
    from shuffle_exchange_amd.ops.optim import lion_flat_
    for n in FLAT_SIZES:
        p, g, m, _ = _inputs(n, gdt)
        idx = _plant(n)
        g[idx] = 0.0
        m[idx] = 0.0  # exact ties: c == 0 -> u == 0 -> p * (1 - lr * wd)
        lp = _lp(n, lpdt)
        scale_t, skip_t = _flags()
        for step in range(2):  # step 2 reads the momentum step 1 wrote
            if step == 1:
                g = _inputs(n, gdt)[0].to(gdt)  # another gradient: the p draw, rounded to gdt
            rp, rm, c = R.lion_ref(p, g, m, lr=LR, beta1=B1, beta2=B2, weight_decay=wd, gs=GS * SCALE_T)
            if step == 0:
                assert (c[idx] == 0).all()
            lion_flat_(p, g, m, lp, lr=LR, beta1=B1, beta2=B2, weight_decay=wd, grad_scale=GS, scale_t=scale_t,
                       skip_t=skip_t)
            # worst observed on MI355X: 2.4e-7 abs, 0.04 of the tolerance; the guard excluded 120 elements
            # in all 48 runs of the large size (4.8e-6 of them), none at n <= 1027
            R.check_lion_p("lion_flat_", p, rp, c)
            R.check("lion_flat_", f"m (n={n}, step {step})", m, rm)
            if lp is not None:
                assert torch.equal(lp, p.to(lpdt)), n


@pytest.mark.parametrize("n", [1, 257, 1027])
def test_lion_flat_exact_cancellation_gives_zero_update(n):
    """beta1 = 0.5 and g = -m: c = 0.5*m - 0.5*m is exactly 0 in fp32 with or without FMA, so u = 0.
    A kernel that sends c == 0 to +1 or -1 moves every element by lr."""
    from shuffle_exchange_amd.ops.optim import lion_flat_
    p, _, m, _ = _inputs(n, F32)
    g = -m
    rp, rm, c = R.lion_ref(p, g, m, lr=LR, beta1=0.5, beta2=B2, weight_decay=0.1)
    assert (c == 0).all()
    lion_flat_(p, g, m, lr=LR, beta1=0.5, beta2=B2, weight_decay=0.1)
    assert R.check_lion_p("lion_flat_", p, rp, c) == 0
    R.check("lion_flat_", "m", m, rm)


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("lpdt", LPDT, ids=str)
@pytest.mark.parametrize("gdt", GDT, ids=str)
def test_adagrad_flat(gdt, lpdt, wd):
    from shuffle_exchange_amd.ops.optim import adagrad_flat_
    for n in FLAT_SIZES:
        p, g, _, s = _inputs(n, gdt)
        idx = _plant(n)
        p[idx] = 0.0
        g[idx] = 0.0
        s[idx] = 0.0  # 0 / (sqrt(0) + eps): p stays 0, no NaN
        lp = _lp(n, lpdt)
        scale_t, skip_t = _flags()
        for step in range(2):  # step 2 reads the sum step 1 wrote
            if step == 1:
                g = _inputs(n, gdt)[2].mul(10).to(gdt)
            rp, rs = R.adagrad_ref(p, g, s, lr=LR, eps=1e-10, weight_decay=wd, gs=GS * SCALE_T)
            adagrad_flat_(p, g, s, lp, lr=LR, eps=1e-10, weight_decay=wd, grad_scale=GS, scale_t=scale_t,
                          skip_t=skip_t)
            assert torch.isfinite(p).all() and torch.isfinite(s).all()
            if step == 0:
                assert (p[idx] == 0).all() and (s[idx] == 0).all()
            # worst observed on MI355X: 2.8e-6 abs (on s), 0.017 of the tolerance
            R.check("adagrad_flat_", f"p (n={n}, step {step})", p, rp)
            R.check("adagrad_flat_", f"s (n={n}, step {step})", s, rs)
            if lp is not None:
                assert torch.equal(lp, p.to(lpdt)), n


# -------------------------------------------------------------------------------------------- adam_flat_
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)


def _adam_case(n, gdt, lpdt, adamw, bias_correction):
    """Two calls (step 1, then step 3 on the state the first one wrote), each against the fp64
    update of the values it started from."""
    from shuffle_exchange_amd.ops.optim import adam_flat_
    p, g, m, v = _inputs(n, gdt)
    idx = _plant(n)
    g[idx] = 0.0
    v[idx] = 0.0
    m[idx] = 0.05  # v = 0, g = 0, m != 0: under AdamW the denominator is eps alone
    lp = _lp(n, lpdt)
    scale_t, skip_t = _flags()
    for step in (1, 3):
        rp, rm, rv = R.adam_ref(p, g, m, v, step=step, adamw=adamw, bias_correction=bias_correction,
                                gs=GS * SCALE_T, **ADAM)
        adam_flat_(p, g, m, v, lp, step=step, adamw=adamw, bias_correction=bias_correction, grad_scale=GS,
                   scale_t=scale_t, skip_t=skip_t, **ADAM)
        # worst observed on MI355X: 0.46 of the tolerance (5.0e-3 abs, on a planted p of 4.5e4). The largest
        # share is v: the kernel forms 1 - beta2 in fp32, and 1.f - 0.999f is 1.3e-5 (relative) off 0.001.
        for what, got, ref in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
            R.check("adam_flat_", f"{what} (n={n}, step {step})", got, ref)
        if lp is not None:
            assert torch.equal(lp, p.to(lpdt)), n


@pytest.mark.parametrize("bias_correction", [True, False])
@pytest.mark.parametrize("adamw", [True, False])
@pytest.mark.parametrize("lpdt", LPDT, ids=str)
@pytest.mark.parametrize("gdt", GDT, ids=str)
def test_adam_flat_every_dtype_and_mode(gdt, lpdt, adamw, bias_correction):
    _adam_case(1027, gdt, lpdt, adamw, bias_correction)  # 256 vec4 threads + a tail of 3


# four elements per thread and a scalar tail of n % 4; the last size is past the grid cap with a tail of 3
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 4 * (GRID_CAP * 256 + 300) + 3])
@pytest.mark.parametrize("gdt,lpdt,adamw,bias_correction", [(F32, None, True, True), (BF16, BF16, True, True),
                                                            (F16, F32, False, False), (F32, F16, False, True)])
def test_adam_flat_sizes(n, gdt, lpdt, adamw, bias_correction):
    _adam_case(n, gdt, lpdt, adamw, bias_correction)


# ------------------------------------------------------------------------------------ multi_tensor_adam_
MT_SIZES = (0, 1, 3, 17, 65535, 65536, 65537, 131073)  # chunk edges at multiples of 65536, an empty tensor


def _mt_lists(gdt, lpdt, views):
    """Per-tensor (p, g, m, v[, lp]); ``views``: every tensor is flat[1 : 1 + n] of a buffer of its
    own dtype, so no pointer is 16-byte aligned and the kernel takes its scalar path (vec_ok false)."""
    def place(t):
        if not views:
            return t.cuda()
        buf = torch.zeros(t.numel() + 2, dtype=t.dtype, device="cuda")
        out = buf[1:1 + t.numel()]
        out.copy_(t)
        assert t.numel() == 0 or out.data_ptr() % 16 != 0
        return out
    ps, gs, ms, vs, lps = [], [], [], [], []
    for n in MT_SIZES:
        p, g, m, v = _host_inputs(n)
        ps.append(place(p.clone()))
        gs.append(place(g.to(gdt)))
        ms.append(place(m.clone()))
        vs.append(place(v.clone()))
        if lpdt is not None:
            lps.append(place(torch.full((n,), 7.0, dtype=lpdt)))
    return ps, gs, ms, vs, lps


@pytest.mark.parametrize("adamw", [True, False])
@pytest.mark.parametrize("gdt,lpdt", [(F32, None), (BF16, BF16), (F16, F32)], ids=str)
@pytest.mark.parametrize("views", [False, True], ids=["aligned", "views"])
def test_multi_tensor_adam(views, gdt, lpdt, adamw):
    """Direct call, judged per tensor against the fp64 update (not against adam_flat_). (bf16, bf16)
    is FusedAdam's mixed-precision path: fp32 masters, bit16 gradients and parameters."""
    ps, gs, ms, vs, lps = _mt_lists(gdt, lpdt, views)
    scale_t, skip_t = _flags()
    for step in (1, 2):
        refs = [R.adam_ref(p, g, m, v, step=step, adamw=adamw, bias_correction=True, gs=GS * SCALE_T, **ADAM)
                for p, g, m, v in zip(ps, gs, ms, vs)]
        torch.ops.sxe.multi_tensor_adam_(ps, gs, ms, vs, lps, scale_t, skip_t, ADAM["lr"], ADAM["beta1"],
                                         ADAM["beta2"], ADAM["eps"], ADAM["weight_decay"], step, adamw, True, GS)
        for i, (rp, rm, rv) in enumerate(refs):
            # worst observed on MI355X: 4.7e-7 abs, 0.22 of the tolerance (v, 1 - beta2 in fp32 as in adam_flat_)
            for what, got, ref in (("p", ps[i], rp), ("m", ms[i], rm), ("v", vs[i], rv)):
                R.check("multi_tensor_adam_", f"{what} (tensor {i}, n={MT_SIZES[i]}, step {step})", got, ref)
            if lps:
                assert torch.equal(lps[i], ps[i].to(lpdt)), i


# ------------------------------------------------------------------------------------------------- skip
@pytest.mark.parametrize("op", ["lion", "adagrad", "adam", "multi_tensor_adam"])
def test_skip_flag_leaves_every_output_bit_identical(op):
    from shuffle_exchange_amd.ops import optim as O
    n = 1027
    p, g, m, v = _inputs(n, BF16)
    lp = _lp(n, BF16)
    before = [t.clone() for t in (p, g, m, v, lp)]
    scale_t, skip_t = _flags(skip=1.0)
    if op == "lion":
        O.lion_flat_(p, g, m, lp, lr=LR, weight_decay=0.1, grad_scale=GS, scale_t=scale_t, skip_t=skip_t)
    elif op == "adagrad":
        O.adagrad_flat_(p, g, v, lp, lr=LR, weight_decay=0.1, grad_scale=GS, scale_t=scale_t, skip_t=skip_t)
    elif op == "adam":
        O.adam_flat_(p, g, m, v, lp, step=1, grad_scale=GS, scale_t=scale_t, skip_t=skip_t, **ADAM)
    else:
        torch.ops.sxe.multi_tensor_adam_([p], [g], [m], [v], [lp], scale_t, skip_t, ADAM["lr"], ADAM["beta1"],
                                         ADAM["beta2"], ADAM["eps"], ADAM["weight_decay"], 1, True, True, GS)
    assert all(torch.equal(a, b) for a, b in zip((p, g, m, v, lp), before))
    assert (lp == 7).all()


# ------------------------------------------------------------------------------------------------ sumsq
# eight elements per thread and a scalar tail of n % 8; the last size is past the 1024-block cap, tail 5
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2055, 8 * (1024 * 256 + 300) + 5])
@pytest.mark.parametrize("dt", GDT, ids=str)
def test_sumsq_exact(n, dt):
    """Integers in [-2, 2] (exact in bf16 / fp16): every partial sum is an integer <= 4n < 2^24, so
    the fp32 sum is exact in any order and must EQUAL the fp64 sum."""
    assert 4 * n < 2 ** 24
    x = torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(0)).to(dt)
    x[n - (n & 7):] = 2.0  # the whole tail counts
    x[0] = -2.0
    x = x.cuda()
    assert torch.ops.sxe.sumsq(x).item() == x.double().pow(2).sum().item()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("where", [100, 2054])  # in the vector part, in the tail
def test_sumsq_propagates_nonfinite(bad, where):
    x = torch.ones(2055, device="cuda")
    x[where] = bad
    out = torch.ops.sxe.sumsq(x).item()
    assert out != out if bad != bad else out == float("inf")


# ------------------------------------------------------------------------------------------- front ends
@pytest.mark.parametrize("dtype", [F32, BF16], ids=str)
def test_fused_lion_gpu(dtype):
    R.run_fused_lion(dtype, "cuda", "FusedLion gpu")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=str)
def test_fused_adagrad_gpu(dtype):
    R.run_fused_adagrad(dtype, "cuda", "FusedAdagrad gpu")


# ----------------------------------------------------------------------------------------------- engine
def _engine_case(rank, world, ds_opt, steps):
    import shuffle_exchange_amd as sxe
    torch.cuda.set_device(0)
    model, cfg = C.tiny_llama(0)
    ds = {"train_micro_batch_size_per_gpu": 2, "zero_optimization": {"stage": 1}, "optimizer": ds_opt}
    eng, _, _, _ = sxe.initialize(model=model, config=ds)
    for b in C.global_batches(cfg, 1, 2, 16, steps):
        b = b.cuda()
        loss = eng(b, labels=b)
        eng.backward(loss)
        eng.step()
    torch.cuda.synchronize()
    return {"params": {k: v.cpu() for k, v in C.full_params(eng).items()}, "kind": eng.optimizer.kind}


@pytest.mark.parametrize("ds_opt", [{"type": "Lion", "params": {"lr": 1e-3, "weight_decay": 0.01}},
                                    {"type": "Adagrad", "params": {"lr": 1e-2, "weight_decay": 0.01}}],
                         ids=["lion", "adagrad"])
def test_zero1_engine_lion_adagrad(ds_opt):
    """World of one, ZeRO-1, fp32 tiny llama, two steps through the ZeRO Lion / Adagrad branches
    (runtime/zero/base.py) against the single-process CPU reference.

    Tolerance, from the update rules: both optimizers move an element by about lr per step whatever
    the gradient's size (Lion: lr * sign(c); Adagrad's first step: lr * g / |g|), and the GPU forward
    differs from the CPU reference by the attention kernel's bf16 rounding (2^-8 relative), which
    flips the sign of near-zero entries. So (a) no element may be further from the reference than
    2 * lr * steps (every step flipped) plus the decay term's share; (b) the update as a whole must
    point the same way: cosine(update, reference update) >= 0.9, i.e. at most about 5 % of the
    update's mass flipped -- a wrong state offset, swapped betas or a missing bit16 write-back
    decorrelates whole tensors and fails it."""
    steps, lr = 2, ds_opt["params"]["lr"]
    got = run_dist(_engine_case, 1, ds_opt, steps)[0]
    assert got["kind"] == ds_opt["type"].lower()
    ref = C.reference_train(ds_opt, steps, 1, 2, 16)
    init = {n: q.detach().float().clone() for n, q in C.tiny_llama(0)[0].named_parameters()}
    for k, v in ref.items():
        a = got["params"][k]
        bound = 2 * lr * steps * (1 + 0.01 * v.abs().max().item()) + 1e-6
        assert (a - v).abs().max().item() <= bound, k
        du, dr = (a - init[k]).double().flatten(), (v - init[k]).double().flatten()
        cos = (du @ dr / (du.norm() * dr.norm() + 1e-300)).item()
        # observed on MI355X: cosine >= 0.991 for every tensor, largest difference 2 * lr * steps
        print(f"[optim-ref] engine {ds_opt['type']} {k}: cosine {cos:.4f}, max diff {(a - v).abs().max().item():.2e}")
        assert cos >= 0.9, (k, cos)


# ----------------------------------------------------------------------------------------------- misuse
# Every case stays in bounds even without the check: the operand that breaks the rule is LARGER than
# the n elements a launch would touch (n + 4 elements, or a [::2] view of a 2n buffer).
def _flat_misuse(n=64):
    f = lambda k=n, dt=F32: torch.ones(k, dtype=dt, device="cuda")  # noqa: E731
    ok = lambda: dict(p=f(), g=f(), s=f(), lp=f(dt=BF16))  # noqa: E731
    return {
        "noncontiguous_p": dict(ok(), p=f(2 * n)[::2]),
        "noncontiguous_g": dict(ok(), g=f(2 * n)[::2]),
        "noncontiguous_state": dict(ok(), s=f(2 * n)[::2]),
        "noncontiguous_lp": dict(ok(), lp=f(2 * n, BF16)[::2]),
        "g_numel": dict(ok(), g=f(n + 4)),
        "state_numel": dict(ok(), s=f(n + 4)),
        "lp_numel": dict(ok(), lp=f(n + 4, BF16)),
        "bf16_master": dict(ok(), p=f(2 * n, BF16)[:n]),  # n elements of a buffer with the bytes of n floats
        "bf16_state": dict(ok(), s=f(2 * n, BF16)[:n]),
    }


FLAT_MISUSE = ["noncontiguous_p", "noncontiguous_g", "noncontiguous_state", "noncontiguous_lp", "g_numel",
               "state_numel", "lp_numel", "bf16_master", "bf16_state"]


@pytest.mark.parametrize("case", FLAT_MISUSE)
@pytest.mark.parametrize("op", ["lion", "adagrad"])
def test_flat_kernels_reject_misuse(op, case):
    cases = _flat_misuse()
    assert sorted(cases) == sorted(FLAT_MISUSE)
    t = cases[case]
    bases = [x._base if x._base is not None else x for x in t.values()]
    before = [b.clone() for b in bases]
    with pytest.raises(RuntimeError):
        if op == "lion":
            torch.ops.sxe.lion_flat_(t["p"], t["g"], t["s"], t["lp"], None, None, LR, B1, B2, 0.1, 1.0)
        else:
            torch.ops.sxe.adagrad_flat_(t["p"], t["g"], t["s"], t["lp"], None, None, LR, 1e-10, 0.1, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bases, before))


@pytest.mark.parametrize("case", ["g_numel", "m_numel", "v_numel", "lp_numel", "lp_mixed_dtype", "lp_noncontiguous"])
def test_multi_tensor_adam_rejects_misuse(case):
    n = 64
    f = lambda k=n, dt=F32: torch.ones(k, dtype=dt, device="cuda")  # noqa: E731
    ps, gs, ms, vs = ([f(), f()] for _ in range(4))
    lps = [f(dt=BF16), f(dt=BF16)]
    if case == "g_numel":
        gs[1] = f(n + 4)
    elif case == "m_numel":
        ms[1] = f(n + 4)
    elif case == "v_numel":
        vs[1] = f(n + 4)
    elif case == "lp_numel":
        lps[1] = f(n + 4, BF16)
    elif case == "lp_mixed_dtype":
        lps[1] = f(dt=F16)  # the dtype is read from lp[0]; same element size, so still in bounds
    else:
        lps[1] = f(2 * n, BF16)[::2]
    every = ps + gs + ms + vs + lps
    bases = [x._base if x._base is not None else x for x in every]
    before = [b.clone() for b in bases]
    with pytest.raises(RuntimeError):
        torch.ops.sxe.multi_tensor_adam_(ps, gs, ms, vs, lps, None, None, ADAM["lr"], ADAM["beta1"], ADAM["beta2"],
                                         ADAM["eps"], ADAM["weight_decay"], 1, True, True, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bases, before))
