"""Plain float64 references for the row kernels (xent.hip, norm.hip, act.hip, rope.hip, softmax.hip)
and the case tables their tests share.

Every reference takes the tensors the kernel sees (already rounded to the test dtype), upcasts them to
``dt`` (float64) and computes the operation with ordinary torch arithmetic -- no fused builtin, so
tests/test_row_refs.py can check each one against torch's own builtin on the CPU. The GPU tests call
the same functions with ``dt=torch.float32`` on the device for their error baseline.

The case builders draw from a seeded CPU generator, so the CPU checks and the GPU tests see the same
numbers.
"""
import math

import torch

F64 = torch.float64
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
NEG_INF = float("-inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dtype_id(d):
    return str(d).replace("torch.", "")


# ------------------------------------------------------------------------------------------------
# cross-entropy
# ------------------------------------------------------------------------------------------------
def xent_ref(logits, target, ignore_index=-100, scale=1.0, lse=None, dt=F64):
    """-> (loss [rows], lse [rows], grad [rows, V]) with grad = scale * (softmax - onehot); ``scale``
    is a number or a per-row tensor. Ignored rows: loss 0 and a zero gradient row. ``lse`` (optional)
    replaces the computed one in the gradient (xent_bwd receives it as an input). -inf logits carry
    no mass; a row needs one finite logit."""
    x = logits.to(dt)
    rows, V = x.shape
    m = x.max(-1, keepdim=True).values
    own_lse = m.squeeze(-1) + (x - m).exp().sum(-1).log()
    ign = target == ignore_index
    t = torch.where(ign, torch.zeros_like(target), target)
    xt = x.gather(1, t[:, None]).squeeze(1)
    zero = torch.zeros((), dtype=dt, device=x.device)
    loss = torch.where(ign, zero, own_lse - xt)
    use = own_lse if lse is None else lse.to(dt)
    p = (x - use[:, None]).exp()
    onehot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    sc = scale.to(dt) if torch.is_tensor(scale) else torch.full((rows,), float(scale), dtype=dt, device=x.device)
    sc = torch.where(ign, zero, sc.expand(rows))
    grad = sc[:, None] * (p - onehot)
    grad = torch.where(ign[:, None], zero, grad)
    return loss, own_lse, grad


XENT_VOCABS = [8, 1000, 2048, 2056, 1001, 2047]
# target sets for 3 rows; "ign" is replaced by the case's ignore_index, columns are clamped to V-1
XENT_TSETS = {
    "edges": (-100, [0, "last", 7]),
    "seam_ign": (-100, [8, "ign", "mid"]),
    "ign_m1": (-1, ["ign", 7, 8]),
}
XENT_INF = ["tail256", "group8", "scatter"]


def _targets(spec, V, ignore_index):
    out = []
    for s in spec:
        if s == "last":
            out.append(V - 1)
        elif s == "mid":
            out.append(V // 2)
        elif s == "ign":
            out.append(ignore_index)
        else:
            out.append(min(int(s), V - 1))
    return torch.tensor(out, dtype=torch.long)


def xent_case(V, dtype, tset, seed=0):
    """3 rows of randn*3 logits -> (logits, target, ignore_index)."""
    ignore_index, spec = XENT_TSETS[tset]
    logits = (torch.randn(3, V, generator=_gen(1000 + V + seed)) * 3).to(dtype)
    return logits, _targets(spec, V, ignore_index), ignore_index


def xent_stride_case(dtype, rows=8197, V=64):
    """More rows than the launcher's 8192-block cap; the last row (a second-trip row) is live with its
    target in the last column, a few rows are ignored."""
    g = _gen(77)
    logits = (torch.randn(rows, V, generator=g) * 3).to(dtype)
    target = torch.randint(0, V, (rows,), generator=g)
    target[5] = -100
    target[8192] = -100
    target[8193] = 0
    target[rows - 1] = V - 1
    return logits, target, -100


def xent_extreme_case(V, dtype):
    """One logit at +80, the rest at -80: the hot column is the target (loss ~ 0), is not the target
    (loss ~ 160), and sits in the last column."""
    logits = torch.full((3, V), -80.0)
    hot = [5, V // 2, V - 1]
    for r, c in enumerate(hot):
        logits[r, c] = 80.0
    target = torch.tensor([5, 0, V - 1], dtype=torch.long)
    return logits.to(dtype), target, -100


def xent_inf_case(pattern, vec, dtype):
    """-inf logits; the targets are finite columns. vec=True: V % 8 == 0 (vector path), else V - 1."""
    V = {"tail256": 2304, "group8": 4096, "scatter": 2304}[pattern] - (0 if vec else 1)
    g = _gen(300 + len(pattern))
    logits = torch.randn(3, V, generator=g) * 3
    if pattern == "tail256":
        logits[:, 2048:] = NEG_INF
        cols = [0, 2047, 7]
    elif pattern == "group8":
        logits[:, 2048:2056] = NEG_INF
        cols = [2047, 2056, V - 1]
    else:
        hit = torch.rand(3, V, generator=g) < 0.1
        cols = [0, 8, V - 1]
        for r, c in enumerate(cols):
            hit[r, c] = False
        logits[hit] = NEG_INF
    return logits.to(dtype), torch.tensor(cols, dtype=torch.long), -100


def xent_dual_inf_case():
    """64 x 2304 bf16 with the last 256 columns -inf (xent_grad_dual's tile: rows % 64, V % 256)."""
    g = _gen(411)
    logits = torch.randn(64, 2304, generator=g) * 3
    logits[:, 2048:] = NEG_INF
    target = torch.randint(0, 2048, (64,), generator=g)
    target[3] = -100
    target[63] = 2047
    return logits.bfloat16(), target, -100


# ------------------------------------------------------------------------------------------------
# RMSNorm / LayerNorm
# ------------------------------------------------------------------------------------------------
def norm_fwd_ref(x, res, w, b, eps, ln, dt=F64):
    """-> (y, rstd [rows], mean [rows] or None, h). h = x + res rounded to the activation dtype (the
    residual stream is stored in it) and is what gets normalised; h is x itself without a residual."""
    if res is not None:
        h_store = (x.to(dt) + res.to(dt)).to(x.dtype)
    else:
        h_store = x
    h = h_store.to(dt)
    if ln:
        mean = h.mean(-1, keepdim=True)
        var = ((h - mean) ** 2).mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        y = (h - mean) * rstd * w.to(dt)
        if b is not None:
            y = y + b.to(dt)
        return y, rstd.squeeze(-1), mean.squeeze(-1), h_store
    rstd = 1.0 / torch.sqrt((h * h).mean(-1, keepdim=True) + eps)
    return h * rstd * w.to(dt), rstd.squeeze(-1), None, h_store


def norm_bwd_ref(dy, h, rstd, mean, w, dres, ln, dt=F64):
    """Analytic backward from the saved statistics -> (dx, dw [H], db [H] or None); ``dres`` (optional)
    is added into dx."""
    d, hh, r = dy.to(dt), h.to(dt), rstd.to(dt)[:, None]
    mu = mean.to(dt)[:, None] if ln else 0.0
    xhat = (hh - mu) * r
    g = d * w.to(dt)
    s1 = (g * xhat).mean(-1, keepdim=True)
    t = g - xhat * s1
    if ln:
        t = t - g.mean(-1, keepdim=True)
    dx = t * r
    if dres is not None:
        dx = dx + dres.to(dt)
    return dx, (d * xhat).sum(0), (d.sum(0) if ln else None)


NORM_HIDDEN = [8, 64, 504, 520, 1032, 2056, 8192]
NORM_ROWS = [5, 300]


def norm_case(rows, H, dtype, wf32, ln, bias=True, offset=0.0, seed=0):
    """-> dict(x, res, w, b, dy, dres, eps). w is fp32 (module default) or the activation dtype."""
    g = _gen(2000 + H + rows + seed)
    wd = torch.float32 if wf32 else dtype
    x = (torch.randn(rows, H, generator=g) + offset).to(dtype)
    return dict(x=x, res=torch.randn(rows, H, generator=g).to(dtype),
                w=(torch.rand(H, generator=g) + 0.5).to(wd),
                b=torch.randn(H, generator=g).to(wd) if (ln and bias) else None,
                dy=torch.randn(rows, H, generator=g).to(dtype), dres=torch.randn(rows, H, generator=g).to(dtype),
                eps=1e-5)


# ------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------
ACTS = {"identity": 0, "relu": 1, "gelu": 2, "silu": 3, "gelu_exact": 4, "quick_gelu": 5}
_K0, _K1 = 0.7978845608028654, 0.044715


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def act_ref(x, act):
    if act == 1:
        return torch.where(x > 0, x, torch.zeros_like(x))
    if act == 2:
        return 0.5 * x * (1.0 + torch.tanh(_K0 * (x + _K1 * x * x * x)))
    if act == 3:
        return x * _sigmoid(x)
    if act == 4:
        return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))
    if act == 5:
        return x * _sigmoid(1.702 * x)
    return x


def dact_ref(x, act):
    if act == 1:
        return (x > 0).to(x.dtype)
    if act == 2:
        t = torch.tanh(_K0 * (x + _K1 * x * x * x))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _K0 * (1.0 + 3.0 * _K1 * x * x)
    if act == 3:
        s = _sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    if act == 4:
        return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == 5:
        s = _sigmoid(1.702 * x)
        return s + 1.702 * x * s * (1.0 - s)
    return torch.ones_like(x)


def gated_fwd_ref(gu, act, dt=F64):
    g, u = gu.to(dt).chunk(2, dim=-1)
    return act_ref(g, act) * u


def gated_bwd_ref(dout, gu, act, dt=F64):
    g, u = gu.to(dt).chunk(2, dim=-1)
    d = dout.to(dt)
    return torch.cat([d * u * dact_ref(g, act), d * act_ref(g, act)], dim=-1)


def bias_fwd_ref(x, bias, act, dt=F64):
    v = x.to(dt) + (bias.to(dt) if bias is not None else 0.0)
    return act_ref(v, act)


def bias_bwd_ref(dy, x, bias, act, dt=F64):
    v = x.to(dt) + (bias.to(dt) if bias is not None else 0.0)
    return dy.to(dt) * dact_ref(v, act)


def act_input(shape, dtype, seed=0):
    """randn*3 with 0, -0.0, +-30 and the dtype's smallest normal spliced into the first entries."""
    x = torch.randn(*shape, generator=_gen(3000 + seed + sum(shape))) * 3
    flat = x.view(-1)
    special = [0.0, -0.0, 30.0, -30.0, torch.finfo(dtype).tiny]
    flat[:len(special)] = torch.tensor(special, dtype=torch.float64).float()
    return x.to(dtype)


GATED_SHAPES = [(3, 8), (3, 24)]     # (rows, I)
BIAS_SHAPES = [(3, 8), (5, 24)]      # (rows, C)
ACT_STRIDE_SHAPE = (2051, 2064)      # 2051 * 2064 / 8 = 529,158 work items > 2048 blocks * 256 threads


# ------------------------------------------------------------------------------------------------
# RoPE
# ------------------------------------------------------------------------------------------------
def rope_tables(rot_dim, max_pos, theta=10000.0):
    """fp32 cos/sin [max_pos, rot_dim/2], computed in float64 like ops.rope.RopeCache."""
    inv = 1.0 / (theta ** (torch.arange(0, rot_dim, 2, dtype=F64) / rot_dim))
    f = torch.outer(torch.arange(max_pos, dtype=F64), inv)
    return f.cos().float(), f.sin().float()


def rope_ref(x, cos, sin, pos, n_rot=None, rot_dim=None, inverse=False, dt=F64):
    """x [T, heads, D]: rotate-half on the first ``rot_dim`` dims of the first ``n_rot`` heads at
    positions ``pos`` [T]; everything else is returned unchanged. inverse: sin negated."""
    T, Hh, D = x.shape
    n_rot = Hh if n_rot is None else n_rot
    rd = D if rot_dim is None else rot_dim
    half = rd // 2
    out = x.to(dt).clone()
    c = cos.to(dt)[pos][:, None, :]
    s = sin.to(dt)[pos][:, None, :] * (-1.0 if inverse else 1.0)
    a, b = out[:, :n_rot, :half].clone(), out[:, :n_rot, half:rd].clone()
    out[:, :n_rot, :half] = a * c - b * s
    out[:, :n_rot, half:rd] = b * c + a * s
    return out


ROPE_DIMS = [16, 48, 64, 128, 256]
ROPE_PARTIAL = [(64, 32), (48, 16)]  # (D, rot_dim)
ROPE_MAX_POS = 64


def rope_positions(T, max_pos=ROPE_MAX_POS):
    """Shuffled positions with repeats; 0 and max_pos-1 are always present."""
    g = _gen(500 + T)
    pos = torch.randint(0, max_pos, (T,), generator=g)
    pos[T // 2] = 0
    pos[0] = max_pos - 1
    pos[T - 1] = pos[1]
    return pos


def rope_case(T, heads, D, dtype, seed=0):
    return torch.randn(T, heads, D, generator=_gen(4000 + D + seed)).to(dtype)


# ------------------------------------------------------------------------------------------------
# masked softmax
# ------------------------------------------------------------------------------------------------
def softmax_ref(scores, scale=1.0, mask=None, alibi=None, causal=False, window=0, dt=F64):
    """scores [B, H, Q, K]; additive (float) or boolean (keep = True) mask and ALiBi broadcast to it;
    causal relative to the last query (query i sits at key position K - Q + i); window > 0 keeps keys
    qpos - window < j. A fully masked row gives zeros."""
    B, H, Q, K = scores.shape
    s = scores.to(dt) * scale
    if alibi is not None:
        s = s + alibi.to(dt)
    if mask is not None and mask.dtype != torch.bool:
        s = s + mask.to(dt)
    dead = torch.zeros(B, H, Q, K, dtype=torch.bool, device=scores.device)
    if mask is not None and mask.dtype == torch.bool:
        dead = dead | ~mask.expand(B, H, Q, K)
    qpos = torch.arange(K - Q, K, device=scores.device)[:, None]
    kpos = torch.arange(K, device=scores.device)[None, :]
    if causal:
        dead = dead | (kpos > qpos)
    if window > 0:
        dead = dead | (kpos <= qpos - window)
    s = s.masked_fill(dead, NEG_INF)
    m = s.max(-1, keepdim=True).values
    m = torch.where(m == NEG_INF, torch.zeros_like(m), m)
    e = torch.exp(s - m)
    tot = e.sum(-1, keepdim=True)
    return torch.where(tot > 0, e / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(e))


SOFTMAX_K = [1, 63, 64, 65, 200]
SOFTMAX_Q = [1, 5]


def softmax_variants(B, H, Q, K, dtype):
    """name -> kwargs of softmax_ref for one score shape (every mask form, causal, window, ALiBi)."""
    g = _gen(600 + 7 * K + Q)
    fmin = torch.finfo(torch.float32).min
    pad = torch.rand(B, 1, 1, K, generator=g) > 0.3
    pad[:, :, :, 0] = True
    add = torch.randn(B, 1, Q, K, generator=g)
    add[torch.rand(B, 1, Q, K, generator=g) < 0.2] = NEG_INF
    add[torch.rand(B, 1, Q, K, generator=g) < 0.1] = fmin
    if K > 1:
        add[0, 0, 0, :] = NEG_INF          # one fully masked row per head of batch 0
    alibi = torch.randn(1, H, 1, K, generator=g)
    qmask = torch.rand(B, 1, Q, K, generator=g) > 0.4
    return {
        "plain": dict(),
        "scale": dict(scale=0.5),
        "causal": dict(causal=True),
        "window1": dict(causal=True, window=1),
        "window_wide": dict(causal=True, window=K + 3),
        "window_only": dict(window=2),
        "add_inf": dict(mask=add),
        "bool_pad": dict(mask=pad),
        "bool_causal_alibi": dict(mask=qmask, alibi=alibi, causal=True, scale=0.7),
        "alibi_head": dict(alibi=alibi),
        "all_masked": dict(mask=torch.zeros(B, 1, 1, K, dtype=torch.bool)),
    }


def softmax_scores(B, H, Q, K, dtype):
    return (torch.randn(B, H, Q, K, generator=_gen(700 + 11 * K + Q)) * 3).to(dtype)
