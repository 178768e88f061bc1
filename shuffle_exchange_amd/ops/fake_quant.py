"""Grouped fake quantization (quantize + dequantize in one step) for quantization-aware training,
on the fused gfx950 kernels of csrc/kernels/fake_quant.hip, with a PyTorch path for CPU tensors.

``fake_quant(x, bits, groups=1, mode="symmetric", value_range=None)`` views ``x`` as
``[groups, numel / groups]`` and returns a tensor of x's shape and dtype (no autograd; the
compression layers wrap it in a straight-through estimator):

* ``"symmetric"`` / ``"asymmetric"``: the absmax / min-max grids of
  ``runtime.quantize.fake_quantize``, which *is* the CPU path, at any width it accepts; the HIP
  kernel takes 3..16 bits and a GPU tensor outside that range raises rather than changing path;
* ``"binary"``: ``sign(x) * mean|x|`` per group (reference compression/utils.py ``BinaryQuantizer``);
* ``"ternary"``: ``alpha * sign(x) * (|x| > 0.7 * mean|x|)`` with ``alpha`` the mean of the kept
  magnitudes (reference ``TernaryQuantizer``); an all-zero group gives zeros, where the reference
  divides 0 / 0;
* ``value_range``: an fp32 tensor ``[2]`` (min, max) that replaces the batch statistics by a static
  range (``groups == 1``, symmetric / asymmetric). The kernel reads it on the device, so a running
  activation range costs no host sync.

``bits`` is ignored by the binary and ternary modes.
"""
import torch

from . import native

MODES = {"symmetric": 0, "asymmetric": 1, "binary": 2, "ternary": 3}
_HIP_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _check(x, bits, groups, mode, value_range):
    if mode not in MODES:
        raise ValueError(f"fake_quant: unknown mode {mode!r} (expected one of {sorted(MODES)})")
    if groups < 1 or x.numel() % groups != 0:
        raise ValueError(f"fake_quant: numel {x.numel()} is not a multiple of groups {groups}")
    if MODES[mode] <= 1 and bits < (2 if mode == "symmetric" else 1):
        raise ValueError(f"fake_quant: the {mode} grid has no levels at {bits} bits "
                         "(1 bit is the binary mode, 2 bits the ternary mode)")
    if value_range is not None:
        if MODES[mode] > 1 or groups != 1:
            raise ValueError("fake_quant: value_range needs groups == 1 and the symmetric or asymmetric mode")
        if value_range.shape != (2,) or value_range.dtype != torch.float32 or value_range.device != x.device:
            raise ValueError("fake_quant: value_range must be an fp32 tensor of shape [2] (min, max) on x's device")


def _torch_fake_quant(x, bits, groups, mode, value_range):
    """The four formulas in fp32 PyTorch: the CPU path, and the oracle of the kernel tests."""
    from ..runtime.quantize import fake_quantize
    if mode in ("symmetric", "asymmetric") and value_range is None:
        return fake_quantize(x, bits, groups, mode == "symmetric")
    flat = x.detach().float().reshape(groups, -1)
    if mode == "symmetric":
        q = 2 ** (bits - 1) - 1
        s = torch.maximum(value_range[0].abs(), value_range[1]).clamp_min(1e-12) / q
        out = torch.round(flat / s).clamp(-q - 1, q) * s
    elif mode == "asymmetric":
        lo, hi = value_range[0], value_range[1]
        s = (hi - lo).clamp_min(1e-12) / (2 ** bits - 1)
        out = torch.round((flat - lo) / s).clamp(0, 2 ** bits - 1) * s + lo
    else:
        mag = flat.abs()
        m = mag.sum(1, keepdim=True) / flat.shape[1]
        if mode == "binary":
            out = flat.sign() * m
        else:
            mask = mag > 0.7 * m
            alpha = (mag * mask).sum(1, keepdim=True) / mask.sum(1, keepdim=True).clamp_min(1)
            out = alpha * flat.sign() * mask
    return out.reshape(x.shape).to(x.dtype)


def fake_quant(x, bits, groups=1, mode="symmetric", value_range=None):
    bits, groups = int(bits), int(groups)
    _check(x, bits, groups, mode, value_range)
    if x.dtype in _HIP_DTYPES and native.use_hip(x):
        if MODES[mode] <= 1 and not 3 <= bits <= 16:
            raise ValueError(f"fake_quant: the HIP kernel takes bits in 3..16 for the {mode} mode, got {bits}")
        return torch.ops.sxe.fake_quant(x.detach().contiguous(), groups, MODES[mode], bits, value_range)
    return _torch_fake_quant(x, bits, groups, mode, value_range)
