"""Low-bit compression on the CPU path: binary (1-bit) and ternary (2-bit) weight quantizers,
learned-score (topk) sparse pruning, static activation ranges, and ``ops.fake_quant`` against
``runtime.quantize.fake_quantize``."""
import math

import pytest
import torch
import torch.nn as nn


def binary_ref64(x, groups):
    """Reference BinaryQuantizer in fp64: sign(x) * mean|x| per group."""
    flat = x.double().reshape(groups, -1)
    return (flat.sign() * flat.abs().mean(1, keepdim=True)).reshape(x.shape)


def ternary_ref64(x, groups):
    """Reference TernaryQuantizer in fp64; also returns the per-group threshold."""
    flat = x.double().reshape(groups, -1)
    thres = 0.7 * flat.abs().mean(1, keepdim=True)
    mask = (flat.abs() > thres).double()
    alpha = (flat.abs() * mask).sum(1, keepdim=True) / mask.sum(1, keepdim=True)
    return (alpha * flat.sign() * mask).reshape(x.shape), thres


@pytest.mark.parametrize("groups", [1, 6])
def test_binary_and_ternary_match_fp64_reference(groups):
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    torch.manual_seed(0)
    x = torch.randn(6, 200)
    out = fake_quant(x, 1, groups, "binary")
    assert out.dtype == x.dtype and out.shape == x.shape
    torch.testing.assert_close(out.double(), binary_ref64(x, groups), rtol=1e-5, atol=0)
    ref, thres = ternary_ref64(x, groups)
    # no element sits on the threshold, so the fp32 and fp64 masks agree
    assert ((x.double().reshape(groups, -1).abs() - thres).abs() > 1e-5 * thres).all()
    torch.testing.assert_close(fake_quant(x, 2, groups, "ternary").double(), ref, rtol=1e-5, atol=0)


def test_all_zero_group_gives_zeros():
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    x = torch.randn(3, 40)
    x[1] = 0
    for mode, bits in (("symmetric", 4), ("asymmetric", 4), ("binary", 1), ("ternary", 2)):
        out = fake_quant(x, bits, 3, mode)
        assert torch.isfinite(out).all() and (out[1] == 0).all(), mode


@pytest.mark.parametrize("target,levels", [(1, 2), (2, 3)])
def test_linear_ramp_to_low_bits(target, levels):
    from shuffle_exchange_amd.compression import LinearLayer_Compress
    torch.manual_seed(0)
    groups = 4
    lin = LinearLayer_Compress(16, 8)
    lin.enable_weight_quantization(8, target, 1, quantization_type="symmetric", num_groups=groups)
    x = torch.randn(5, 16)
    for _ in range(10):
        y = lin(x)
        assert torch.isfinite(y).all()
        lin.zero_grad()
        y.pow(2).mean().backward()
        assert lin.weight.grad is not None and torch.isfinite(lin.weight.grad).all()
    assert lin.wq["bits"] == target
    lin.eval()
    w = lin.effective_weight().detach().reshape(groups, -1)
    assert torch.isfinite(w).all()
    for row in w:
        n = row.unique().numel()
        assert n == 2 if target == 1 else n <= levels
    if target == 1:
        torch.testing.assert_close(w.double(), binary_ref64(lin.weight.detach(), groups).reshape(groups, -1),
                                   rtol=1e-5, atol=0)


@pytest.mark.parametrize("target", [1, 2])
def test_low_bit_targets_need_symmetric(target):
    from shuffle_exchange_amd.compression import Conv2dLayer_Compress, Embedding_Compress, LinearLayer_Compress
    for layer in (LinearLayer_Compress(8, 8), Embedding_Compress(10, 8), Conv2dLayer_Compress(2, 2, 3)):
        with pytest.raises(ValueError):
            layer.enable_weight_quantization(8, target, 1, quantization_type="asymmetric")
        layer.enable_weight_quantization(8, target, 1, quantization_type="symmetric")


def test_low_start_bits_need_symmetric():
    """A ramp that starts at 1 or 2 bits runs the binary / ternary quantizer whatever the target."""
    from shuffle_exchange_amd.compression import LinearLayer_Compress
    lin = LinearLayer_Compress(8, 8)
    for start in (1, 2):
        with pytest.raises(ValueError):
            lin.enable_weight_quantization(start, 4, 1, quantization_type="asymmetric")
    with pytest.raises(ValueError):
        lin.enable_weight_quantization(0, 0, 1)
    assert not lin.weight_quantization_enabled


def test_embedding_and_conv_binary():
    from shuffle_exchange_amd.compression import Conv2dLayer_Compress, Embedding_Compress
    torch.manual_seed(0)
    emb = Embedding_Compress(10, 8)
    emb.enable_weight_quantization(1, 1, 1, num_groups=10)
    out = emb(torch.arange(10))
    assert torch.isfinite(out).all() and all(r.unique().numel() == 2 for r in out)
    conv = Conv2dLayer_Compress(2, 4, 3)
    conv.enable_weight_quantization(2, 2, 1)
    assert torch.isfinite(conv(torch.randn(1, 2, 5, 5))).all()
    assert conv.effective_weight().unique().numel() <= 3


@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_topk_sparse_pruning(kind):
    from shuffle_exchange_amd.compression import Conv2dLayer_Compress, LinearLayer_Compress
    torch.manual_seed(0)
    ratio = 0.3
    if kind == "linear":
        layer, x = LinearLayer_Compress(16, 9), torch.randn(4, 16)
    else:
        layer, x = Conv2dLayer_Compress(3, 5, 3, padding=1), torch.randn(2, 3, 6, 6)
    layer.enable_sparse_pruning(ratio, method="topk")
    scores = layer.sparse_mask_scores
    assert isinstance(scores, nn.Parameter) and scores.shape == layer.weight.shape
    assert "sparse_mask_scores" in dict(layer.named_parameters())
    y = layer(x)
    y.pow(2).mean().backward()
    assert scores.grad is not None and scores.grad.abs().sum() > 0
    keep = math.ceil(ratio * layer.weight.numel())
    assert int(layer.sparse_mask.sum()) == keep and set(layer.sparse_mask.unique().tolist()) == {0.0, 1.0}
    # the mask follows the scores, not the weight magnitudes
    top = scores.detach().flatten().topk(keep).indices
    assert (layer.sparse_mask.flatten()[top] == 1).all()
    layer.fix_all()
    assert not hasattr(layer, "sparse_mask_scores") and "sparse_mask_scores" not in dict(layer.named_parameters())
    assert int((layer.weight != 0).sum()) <= keep
    torch.testing.assert_close(layer(x), y.detach(), rtol=0, atol=0)


def test_topk_redundancy_clean():
    from shuffle_exchange_amd.compression import LinearLayer_Compress, redundancy_clean
    torch.manual_seed(0)
    m = nn.Sequential(LinearLayer_Compress(8, 8))
    m[0].enable_sparse_pruning(0.5, method="topk")
    x = torch.randn(3, 8)
    y = m(x).detach()
    redundancy_clean(m, {})
    assert [n for n, _ in m.named_parameters()] == ["0.weight", "0.bias"]
    torch.testing.assert_close(m(x), y, rtol=0, atol=0)


def test_unknown_pruning_methods_raise():
    from shuffle_exchange_amd.compression import Conv2dLayer_Compress, LinearLayer_Compress
    lin, conv = LinearLayer_Compress(8, 8), Conv2dLayer_Compress(2, 2, 3)
    for bad in ("snip", "topk"):
        with pytest.raises(ValueError):
            lin.enable_row_pruning(0.5, method=bad)
        with pytest.raises(ValueError):
            lin.enable_head_pruning(0.5, 2, method=bad)
        with pytest.raises(ValueError):
            conv.enable_channel_pruning(0.5, method=bad)
    with pytest.raises(ValueError, match="sparse pruning only"):
        lin.enable_row_pruning(0.5, method="topk")
    for layer in (lin, conv):
        with pytest.raises(ValueError):
            layer.enable_sparse_pruning(0.5, method="snip")
    assert not lin.row_pruning_enabled and not lin.sparse_pruning_enabled and not conv.channel_pruning_enabled


@pytest.mark.parametrize("qtype", ["symmetric", "asymmetric"])
def test_static_activation_range(qtype):
    from shuffle_exchange_amd.compression import LinearLayer_Compress
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    torch.manual_seed(0)
    lin = LinearLayer_Compress(4, 4)
    lin.enable_activation_quantization(8, qtype, range_calibration="static")
    assert "x_min_max" in dict(lin.named_buffers()) and lin.x_min_max.shape == (2,)
    batches = [torch.tensor([[-1.0, 0.5, 0.25, 2.0]]), torch.tensor([[-3.0, 0.0, 1.0, 1.5]]),
               torch.tensor([[-0.5, 0.1, 0.2, 4.0]])]
    mom = 0.95
    lo, hi = -1.0, 2.0  # the first batch initialises the range
    for i, b in enumerate(batches):
        lin(b)
        if i > 0:
            lo = lo * mom + float(b.min()) * (1 - mom)
            hi = hi * mom + float(b.max()) * (1 - mom)
        torch.testing.assert_close(lin.x_min_max, torch.tensor([lo, hi]), rtol=1e-6, atol=0)
    lin.eval()
    stored = lin.x_min_max.clone()
    with torch.no_grad():  # identity layer: the output is the quantized activation, exactly
        lin.weight.copy_(torch.eye(4))
        lin.bias.zero_()
    x = torch.tensor([[-50.0, 0.3, 1.0, 70.0]])
    xq = lin(x).detach()
    torch.testing.assert_close(lin.x_min_max, stored, rtol=0, atol=0)  # eval does not move the range
    torch.testing.assert_close(xq, fake_quant(x, 8, 1, qtype, stored), rtol=0, atol=0)
    bound = max(abs(float(stored[0])), float(stored[1])) if qtype == "symmetric" else None
    step = (2 * bound / 254) if bound else (float(stored[1] - stored[0]) / 255)
    if qtype == "symmetric":
        assert float(xq.max()) <= bound + 1e-6 and float(xq.min()) >= -bound - step - 1e-6
    else:
        assert float(xq.min()) >= float(stored[0]) - 1e-6 and float(xq.max()) <= float(stored[1]) + 1e-6
    assert abs(float(xq[0, 1]) - 0.3) <= step  # in-range values only move by the grid


def test_unknown_range_calibration_raises():
    from shuffle_exchange_amd.compression import Conv2dLayer_Compress, LinearLayer_Compress
    for layer in (LinearLayer_Compress(4, 4), Conv2dLayer_Compress(2, 2, 3)):
        with pytest.raises(ValueError):
            layer.enable_activation_quantization(8, "symmetric", range_calibration="percentile")
        assert not layer.activation_quantization_enabled
        layer.enable_activation_quantization(8, "symmetric", range_calibration="dynamic")
        assert not hasattr(layer, "x_min_max")


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = nn.Linear(16, 32)
        self.fc2 = nn.Linear(32, 16)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x)))


_CFG = {"compression_training": {
    "weight_quantization": {"shared_parameters": {"enabled": True, "schedule_offset": 0, "quantize_groups": 2,
                                                  "quantization_type": "symmetric"},
                            "different_groups": {"wq": {"params": {"start_bits": 4, "target_bits": 1,
                                                                   "quantization_period": 1}, "modules": ["fc2"]}}},
    "activation_quantization": {"shared_parameters": {"enabled": True, "schedule_offset": 0,
                                                      "quantization_type": "asymmetric",
                                                      "range_calibration": "static"},
                                "different_groups": {"aq": {"params": {"bits": 8}, "modules": ["fc2"]}}},
    "sparse_pruning": {"shared_parameters": {"enabled": True, "schedule_offset": 0, "method": "topk"},
                       "different_groups": {"sp": {"params": {"dense_ratio": 0.25}, "modules": ["fc1"]}}}}}


def test_config_wires_low_bit_topk_and_static_range():
    from shuffle_exchange_amd.compression import (LinearLayer_Compress, compression_scheduler, init_compression,
                                                  redundancy_clean)
    torch.manual_seed(0)
    m = init_compression(_Net(), _CFG)
    assert isinstance(m.fc1, LinearLayer_Compress) and isinstance(m.fc2, LinearLayer_Compress)
    sch = compression_scheduler(m, _CFG)
    sch.step()
    assert m.fc2.wq["target"] == 1 and m.fc2.wq["groups"] == 2
    assert m.fc2.aq["static"] and not m.fc2.aq["symmetric"] and hasattr(m.fc2, "x_min_max")
    assert m.fc1.sparse_method == "topk" and isinstance(m.fc1.sparse_mask_scores, nn.Parameter)
    opt = torch.optim.SGD(m.parameters(), lr=0.01)  # after the scheduler step: the scores are parameters now
    x = torch.randn(8, 16)
    for _ in range(4):
        loss = m(x).pow(2).mean()
        assert torch.isfinite(loss)
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert m.fc2.wq["bits"] == 1 and m.fc1.sparse_mask_scores.grad.abs().sum() > 0
    assert float(m.fc2.x_min_max[0]) == 0.0 and float(m.fc2.x_min_max[1]) > 0  # fc2 sees relu outputs
    assert int(m.fc1.sparse_mask.sum()) == math.ceil(0.25 * m.fc1.weight.numel())
    m.eval()
    before = m(x)
    redundancy_clean(m, _CFG)
    assert not hasattr(m.fc1, "sparse_mask_scores")
    assert all(r.unique().numel() == 2 for r in m.fc2.weight.detach().reshape(2, -1))


@pytest.mark.parametrize("offset", [0, 3])
def test_init_compression_creates_scores_and_range_before_the_optimizer(offset):
    """The usual order: init_compression, build the optimizer, then step the scheduler inside the
    loop. The topk scores and the static-range buffer exist from init_compression on (techniques
    off until their schedule_offset), so the optimizer holds the scores and updates them once the
    pruning is on, and a state dict saved late loads strictly into a freshly initialised model."""
    import copy

    from shuffle_exchange_amd.compression import compression_scheduler, init_compression
    cfg = copy.deepcopy(_CFG)
    for tech in ("sparse_pruning", "activation_quantization"):
        cfg["compression_training"][tech]["shared_parameters"]["schedule_offset"] = offset
    torch.manual_seed(0)
    m = init_compression(_Net(), cfg)
    assert isinstance(m.fc1.sparse_mask_scores, nn.Parameter) and not m.fc1.sparse_pruning_enabled
    assert "x_min_max" in dict(m.fc2.named_buffers()) and not m.fc2.activation_quantization_enabled
    assert not hasattr(m.fc2, "sparse_mask_scores") and not hasattr(m.fc1, "x_min_max")
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    assert any(p is m.fc1.sparse_mask_scores for g in opt.param_groups for p in g["params"])
    sch = compression_scheduler(m, cfg)
    scores = m.fc1.sparse_mask_scores
    before = scores.detach().clone()
    x = torch.randn(8, 16)
    for step in range(1, offset + 3):
        sch.step()
        loss = m(x).pow(2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert m.fc1.sparse_pruning_enabled == (step >= offset)
        if step < offset:  # not on yet: no gradient, no movement, no range
            assert torch.equal(scores.detach(), before) and float(m.fc2.x_min_max.abs().sum()) == 0
    assert m.fc1.sparse_mask_scores is scores  # enabling did not replace the parameter the optimizer holds
    assert not torch.equal(scores.detach(), before)
    assert float(m.fc2.x_min_max[1]) > 0
    fresh = init_compression(_Net(), cfg)
    fresh.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(fresh.fc1.sparse_mask_scores, scores) and torch.equal(fresh.fc2.x_min_max, m.fc2.x_min_max)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("bits", [3, 4, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ops_fake_quant_is_fake_quantize_on_cpu(bits, symmetric, dtype):
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    from shuffle_exchange_amd.runtime.quantize import fake_quantize
    torch.manual_seed(bits)
    x = torch.randn(6, 200).to(dtype)
    for groups in (1, 6):
        got = fake_quant(x, bits, groups, "symmetric" if symmetric else "asymmetric")
        want = fake_quantize(x, bits, groups, symmetric)
        assert got.dtype == want.dtype and torch.equal(got, want)


@pytest.mark.parametrize("bits,symmetric", [(2, True), (2, False), (1, False), (17, True), (20, False)])
def test_cpu_path_keeps_the_widths_fake_quantize_accepts(bits, symmetric):
    """Only the HIP kernel is limited to 3..16 bits: on the CPU every width that worked through
    ``fake_quantize`` still does, with the same result (an activation quantized to 2 bits, a ramp
    that starts above 16)."""
    from shuffle_exchange_amd.compression import LinearLayer_Compress
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    from shuffle_exchange_amd.runtime.quantize import fake_quantize
    torch.manual_seed(bits)
    x = torch.randn(6, 50)
    assert torch.equal(fake_quant(x, bits, 2, "symmetric" if symmetric else "asymmetric"),
                       fake_quantize(x, bits, 2, symmetric))
    lin = LinearLayer_Compress(50, 4)
    lin.enable_activation_quantization(bits, "symmetric" if symmetric else "asymmetric")
    want = torch.nn.functional.linear(fake_quantize(x, bits, 1, symmetric), lin.weight, lin.bias)
    assert torch.equal(lin(x), want)


def test_fake_quant_argument_checks():
    from shuffle_exchange_amd.ops.fake_quant import fake_quant
    x = torch.randn(4, 10)
    with pytest.raises(ValueError):
        fake_quant(x, 4, 1, "stochastic")
    with pytest.raises(ValueError):
        fake_quant(x, 4, 3, "symmetric")  # 40 % 3 != 0
    with pytest.raises(ValueError):
        fake_quant(x, 1, 1, "symmetric")  # 2^0 - 1 = 0 levels: the binary mode is the 1-bit quantizer
    r = torch.tensor([-1.0, 1.0])
    with pytest.raises(ValueError):
        fake_quant(x, 4, 2, "symmetric", r)  # a static range is per tensor
    with pytest.raises(ValueError):
        fake_quant(x, 1, 1, "binary", r)
    with pytest.raises(ValueError):
        fake_quant(x, 4, 1, "symmetric", torch.tensor([-1.0, 0.0, 1.0]))
