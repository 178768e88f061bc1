// Grouped fake quantization (quantize + dequantize in one step) for quantization-aware training.
//
//   sxe::fake_quant(Tensor x, int groups, int mode, int bits, Tensor? range) -> Tensor
//
// x (fp32 / bf16 / fp16, contiguous) is viewed as [groups, numel / groups]; the result has x's
// dtype and shape. All arithmetic is fp32 whatever the storage type. Modes (n = group length):
//   0 symmetric   q = 2^(bits-1) - 1, s = max(amax|x|, 1e-12) / q, out = clamp(rint(x / s), -q-1, q) * s
//   1 asymmetric  s = max(hi - lo, 1e-12) / (2^bits - 1), out = clamp(rint((x - lo) / s), 0, 2^bits-1) * s + lo
//   2 binary      m = sum|x| / n, out = sign(x) * m
//   3 ternary     thres = 0.7 * sum|x| / n, mask = |x| > thres, alpha = sum(|x| * mask) / count(mask),
//                 out = alpha * sign(x) * mask
// Modes 0 / 1 are runtime/quantize.py::fake_quantize: a true IEEE division and rintf (round half to
// even, as torch.round), no reciprocal multiply, and no contraction of `* s + lo` into an fma (see
// apply1), so the grid points are the ones the PyTorch formula produces. Modes 2 / 3 are the
// reference's BinaryQuantizer / TernaryQuantizer. For an all-zero group the reference's ternary
// quantizer divides 0 / 0; here count(mask) == 0 gives alpha = 0, so such a group outputs zeros
// (as it does in the other three modes).
// NaN: a NaN element comes out as NaN in every mode. Around it the modes differ from the PyTorch
// formulas, which make the whole group NaN: the max / min statistics of modes 0 / 1 skip NaNs
// (fmaxf), so the group's other elements are quantized on the grid of its non-NaN values; the
// sum|x| of modes 2 / 3 becomes NaN, so binary makes the group's non-zero elements NaN and ternary
// (no |x| exceeds a NaN threshold) zeroes the group's other elements.
// `range` (fp32 [2] = min, max, on x's device; groups == 1, modes 0 / 1) replaces the statistics by a
// static range: amax = max(|min|, max) resp. lo, hi = min, max. It is read by the kernel, so a
// running activation range never costs a host sync.
//
// Geometry, chosen on the host by group length n:
//  * n <= 16384 (small): a group lives in the registers of the threads that own it. One wave per
//    group for n <= 512 (4 groups per 256-thread block, butterfly reduction only), else one
//    256-thread block per group with 1 / 2 / 4 / 8 chunks of 8 values per thread (butterfly + one LDS
//    exchange). One read, one write: 4 B/element for 16-bit types. Ternary's second reduction runs
//    on the register copy.
//  * n > 16384, or a static range (large): a 1-D grid of groups x blocks_per_group blocks. A
//    statistics kernel writes one (a, b) partial per block to a workspace (amax | max, max(-x) |
//    sum|x|); ternary runs it a second time for (masked sum, count); the apply kernel has every
//    block re-reduce its group's partials in a fixed order and quantizes. Two reads and one write:
//    6 B/element for 16-bit types. No floating-point atomics anywhere: results are bit-identical
//    from run to run.
//  * 16-byte loads / stores need n % 8 == 0 (every group start aligned) or groups == 1 (tail of
//    n % 8 scalar elements, as accum.hip does), and a 16-byte aligned base; other shapes take the
//    scalar-load instantiation of the same kernels (coalesced 2- or 4-byte accesses).
#include "sxe_common.h"
#include <torch/library.h>

namespace sxe {
namespace fq {

enum Mode : int { kSym = 0, kAsym = 1, kBinary = 2, kTernary = 3 };
constexpr int kSmallMax = 16384;  // largest group the register path holds: 256 threads x 8 chunks x 8 values
constexpr int kMaxBlocksPerGroup = 1024;

template <bool MAX>
__device__ __forceinline__ float comb(float a, float b) {
  return MAX ? fmaxf(a, b) : a + b;
}

// Butterfly over the 64 lanes: every lane ends with the same bits (each step adds / maxes the same
// two operands in both partners).
template <bool MAX>
__device__ __forceinline__ float wave_red(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = comb<MAX>(v, __shfl_xor(v, o, 64));
  return v;
}

// Reduce (a, b) over the NT threads that share a group; NT == 256 is the whole block and uses
// 8 floats of LDS, NT == 64 is one wave and touches neither LDS nor a barrier.
template <bool MAX, int NT>
__device__ __forceinline__ void group_red2(float& a, float& b, float* red) {
  a = wave_red<MAX>(a);
  b = wave_red<MAX>(b);
  if constexpr (NT == 256) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[w] = a; red[4 + w] = b; }
    __syncthreads();
    a = comb<MAX>(comb<MAX>(red[0], red[1]), comb<MAX>(red[2], red[3]));
    b = comb<MAX>(comb<MAX>(red[4], red[5]), comb<MAX>(red[6], red[7]));
    __syncthreads();
  }
}

template <int NT>
__device__ __forceinline__ void group_red2(bool is_max, float& a, float& b, float* red) {
  if (is_max) group_red2<true, NT>(a, b, red);
  else group_red2<false, NT>(a, b, red);
}

// First-pass statistics of one value. sym: a = max|x|; asym: a = max x, b = max -x; binary /
// ternary: a = sum|x|.
__device__ __forceinline__ void stat1(int mode, float x, float& a, float& b) {
  if (mode == kSym) a = fmaxf(a, fabsf(x));
  else if (mode == kAsym) { a = fmaxf(a, x); b = fmaxf(b, -x); }
  else a += fabsf(x);
}
// Ternary second pass: a = sum of |x| above the threshold, b = how many.
__device__ __forceinline__ void stat2(float thres, float x, float& a, float& b) {
  const float ax = fabsf(x);
  if (ax > thres) { a += ax; b += 1.f; }
}

struct Params {
  float s, lo, hi, off;
};

// (a, b) of the first pass -> quantizer constants. Ternary only gets its threshold here (in lo).
__device__ __forceinline__ Params make_params(int mode, int bits, float n, float a, float b) {
  Params p{0.f, 0.f, 0.f, 0.f};
  if (mode == kSym) {
    const float q = (float)((1 << (bits - 1)) - 1);
    p.s = fmaxf(a, 1e-12f) / q;
    p.lo = -q - 1.f;
    p.hi = q;
  } else if (mode == kAsym) {
    const float lo = -b, hi = a;
    const float qmax = (float)((1 << bits) - 1);
    p.s = fmaxf(hi - lo, 1e-12f) / qmax;
    p.hi = qmax;
    p.off = lo;
  } else if (mode == kBinary) {
    p.s = a / n;
  } else {
    p.lo = 0.7f * (a / n);
  }
  return p;
}

__device__ __forceinline__ float apply1(int mode, const Params& p, float x) {
  if (x != x) return x;  // the clamps below would turn a NaN into a grid point
  if (mode == kSym) return fminf(fmaxf(rintf(x / p.s), p.lo), p.hi) * p.s;
  if (mode == kAsym) {
    float t = fminf(fmaxf(rintf((x - p.off) / p.s), 0.f), p.hi) * p.s;
    // The product is rounded before the add, as in PyTorch. The build's -ffp-contract=fast fuses
    // across statements and disregards `#pragma clang fp contract(off)`; an empty asm on the
    // register is what keeps the multiply and the add apart.
    asm("" : "+v"(t));
    return t + p.off;
  }
  if (mode == kBinary) return x > 0.f ? p.s : (x < 0.f ? -p.s : 0.f);
  return fabsf(x) > p.lo ? copysignf(p.s, x) : 0.f;
}

// ------------------------------------------------------------------------------ small groups
// NT threads own one group of n <= NT * CH * 8 values. VEC: thread tl holds the 8-value chunks
// c * NT + tl (16-byte accesses, n % 8 == 0); otherwise value j of chunk c is element
// (c * 8 + j) * NT + tl (coalesced scalar accesses, any n).
template <DT T, int NT, int CH, bool VEC>
__global__ void __launch_bounds__(256) fq_small_kernel(const typename dt_traits<T>::storage* __restrict__ x,
                                                       typename dt_traits<T>::storage* __restrict__ out, int64_t groups,
                                                       int n, int mode, int bits) {
  __shared__ float red[8];
  const int tl = threadIdx.x % NT;
  const int64_t g = (int64_t)blockIdx.x * (256 / NT) + threadIdx.x / NT;
  if (g >= groups) return;  // only reachable for NT == 64 (wave-uniform, no barrier in that instance)
  const typename dt_traits<T>::storage* src = x + g * n;
  typename dt_traits<T>::storage* dst = out + g * n;

  float v[CH][8];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if constexpr (VEC) {
      const int base = (c * NT + tl) * 8;
      if (base < n) {
        load8<T>(src + base, v[c]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[c][j] = 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int idx = (c * 8 + j) * NT + tl;
        v[c][j] = idx < n ? to_f32<T>(src[idx]) : 0.f;
      }
    }
  }
  auto valid = [&](int c, int j) { return VEC ? (c * NT + tl) * 8 < n : (c * 8 + j) * NT + tl < n; };

  const bool is_max = mode <= kAsym;
  float a = is_max ? -INFINITY : 0.f, b = a;
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (valid(c, j)) stat1(mode, v[c][j], a, b);
  group_red2<NT>(is_max, a, b, red);
  Params p = make_params(mode, bits, (float)n, a, b);
  if (mode == kTernary) {
    float ms = 0.f, cnt = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (valid(c, j)) stat2(p.lo, v[c][j], ms, cnt);
    group_red2<false, NT>(ms, cnt, red);
    p.s = cnt > 0.f ? ms / cnt : 0.f;
  }

#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if constexpr (VEC) {
      const int base = (c * NT + tl) * 8;
      if (base < n) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = apply1(mode, p, v[c][j]);
        store8<T>(dst + base, o);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int idx = (c * 8 + j) * NT + tl;
        if (idx < n) dst[idx] = from_f32<T>(apply1(mode, p, v[c][j]));
      }
    }
  }
}

// ------------------------------------------------------------------------------ large groups
// Block blockIdx.x = g * bpg + k handles, of group g, the chunks k * 256 + t, + bpg * 256, ...

// Fixed-order reduction of a group's bpg per-block partials (every block of the group gets the
// same bits).
__device__ __forceinline__ void reduce_partials(bool is_max, const float* __restrict__ ws, int bpg, float& a, float& b,
                                                float* red) {
  a = is_max ? -INFINITY : 0.f;
  b = a;
  for (int i = threadIdx.x; i < bpg; i += 256) {
    if (is_max) { a = fmaxf(a, ws[2 * i]); b = fmaxf(b, ws[2 * i + 1]); }
    else { a += ws[2 * i]; b += ws[2 * i + 1]; }
  }
  group_red2<256>(is_max, a, b, red);
}

// pass 0: first statistics -> ws0. pass 1 (ternary): threshold from ws0, (masked sum, count) -> ws1.
template <DT T, bool VEC>
__global__ void __launch_bounds__(256) fq_stats_kernel(const typename dt_traits<T>::storage* __restrict__ x, int64_t n,
                                                       int bpg, int mode, int pass, const float* __restrict__ ws0,
                                                       float* __restrict__ ws_out) {
  __shared__ float red[8];
  const int64_t g = blockIdx.x / bpg;
  const int k = blockIdx.x % bpg;
  const typename dt_traits<T>::storage* src = x + g * n;
  const bool is_max = pass == 0 && mode <= kAsym;
  float thres = 0.f;
  if (pass == 1) {
    float s0, s1;
    reduce_partials(false, ws0 + g * bpg * 2, bpg, s0, s1, red);
    thres = 0.7f * (s0 / (float)n);
  }
  float a = is_max ? -INFINITY : 0.f, b = a;
  const int64_t stride = (int64_t)bpg * 256;
  const int64_t first = (int64_t)k * 256 + threadIdx.x;
  const int64_t nv = VEC ? n / 8 : 0;
  for (int64_t i = first; i < nv; i += stride) {
    float v[8];
    load8<T>(src + i * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (pass == 0) stat1(mode, v[j], a, b);
      else stat2(thres, v[j], a, b);
    }
  }
  for (int64_t i = nv * 8 + first; i < n; i += stride) {
    const float xv = to_f32<T>(src[i]);
    if (pass == 0) stat1(mode, xv, a, b);
    else stat2(thres, xv, a, b);
  }
  group_red2<256>(is_max, a, b, red);
  if (threadIdx.x == 0) {
    ws_out[(int64_t)blockIdx.x * 2] = a;
    ws_out[(int64_t)blockIdx.x * 2 + 1] = b;
  }
}

template <DT T, bool VEC>
__global__ void __launch_bounds__(256) fq_apply_kernel(const typename dt_traits<T>::storage* __restrict__ x,
                                                       typename dt_traits<T>::storage* __restrict__ out, int64_t n,
                                                       int bpg, int mode, int bits, const float* __restrict__ ws0,
                                                       const float* __restrict__ ws1, const float* __restrict__ range) {
  __shared__ float red[8];
  const int64_t g = blockIdx.x / bpg;
  const int k = blockIdx.x % bpg;
  const typename dt_traits<T>::storage* src = x + g * n;
  typename dt_traits<T>::storage* dst = out + g * n;
  float a, b;
  if (range != nullptr) {  // static range (groups == 1, sym / asym): min, max read on the device
    const float lo = range[0], hi = range[1];
    a = mode == kSym ? fmaxf(fabsf(lo), hi) : hi;
    b = -lo;
  } else {
    reduce_partials(mode <= kAsym, ws0 + g * bpg * 2, bpg, a, b, red);
  }
  Params p = make_params(mode, bits, (float)n, a, b);
  if (mode == kTernary) {
    float ms, cnt;
    reduce_partials(false, ws1 + g * bpg * 2, bpg, ms, cnt, red);
    p.s = cnt > 0.f ? ms / cnt : 0.f;
  }
  const int64_t stride = (int64_t)bpg * 256;
  const int64_t first = (int64_t)k * 256 + threadIdx.x;
  const int64_t nv = VEC ? n / 8 : 0;
  for (int64_t i = first; i < nv; i += stride) {
    float v[8];
    load8<T>(src + i * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = apply1(mode, p, v[j]);
    store8<T>(dst + i * 8, v);
  }
  for (int64_t i = nv * 8 + first; i < n; i += stride) dst[i] = from_f32<T>(apply1(mode, p, to_f32<T>(src[i])));
}

template <DT T, int NT, int CH>
void launch_small(const at::Tensor& x, at::Tensor& out, int64_t groups, int n, int mode, int bits, bool vec) {
  using S = typename dt_traits<T>::storage;
  const int64_t blocks = (groups + (256 / NT) - 1) / (256 / NT);
  const S* xp = reinterpret_cast<const S*>(x.data_ptr());
  S* op = reinterpret_cast<S*>(out.data_ptr());
  SXE_DISPATCH_BOOL(vec, VEC, hipLaunchKernelGGL((fq_small_kernel<T, NT, CH, VEC>), dim3((unsigned)blocks), dim3(256),
                                                 0, cur_stream(), xp, op, groups, n, mode, bits));
}

at::Tensor fake_quant(const at::Tensor& x, int64_t groups, int64_t mode, int64_t bits,
                      const c10::optional<at::Tensor>& range) {
  SXE_CHECK_CUDA(x);
  SXE_CHECK_CONTIG(x);
  SXE_CHECK(mode >= kSym && mode <= kTernary, "fake_quant: mode must be 0 (symmetric), 1 (asymmetric), 2 (binary) or ",
            "3 (ternary), got ", mode);
  SXE_CHECK(groups >= 1, "fake_quant: groups must be positive, got ", groups);
  SXE_CHECK(x.numel() % groups == 0, "fake_quant: numel ", x.numel(), " is not a multiple of groups ", groups);
  if (mode <= kAsym) SXE_CHECK(bits >= 3 && bits <= 16, "fake_quant: bits must be in 3..16 for mode ", mode, ", got ", bits);
  const float* rp = nullptr;
  if (range.has_value()) {
    const at::Tensor& r = *range;
    SXE_CHECK(mode <= kAsym && groups == 1, "fake_quant: a static range needs groups == 1 and the symmetric or ",
              "asymmetric mode");
    SXE_CHECK(r.is_cuda() && r.device() == x.device(), "fake_quant: range must be on x's device");
    SXE_CHECK(r.scalar_type() == at::kFloat && r.dim() == 1 && r.numel() == 2 && r.is_contiguous(),
              "fake_quant: range must be a contiguous fp32 tensor of shape [2] (min, max)");
    rp = r.data_ptr<float>();
  }
  const DT dt = dtype_of(x);
  at::Tensor out = at::empty_like(x);
  const int64_t total = x.numel();
  if (total == 0) return out;
  const int64_t n = total / groups;
  SXE_CHECK(groups < (int64_t)1 << 30, "fake_quant: too many groups");
  c10::DeviceGuard guard(x.device());
  const bool aligned = reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0 &&
                       reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0;

  if (rp == nullptr && n <= kSmallMax) {
    const bool vec = aligned && n % 8 == 0;
    const int ni = (int)n, m = (int)mode, bi = (int)bits;
    SXE_DISPATCH_DT(dt, T, {
      if (n <= 512) launch_small<T, 64, 1>(x, out, groups, ni, m, bi, vec);
      else if (n <= 2048) launch_small<T, 256, 1>(x, out, groups, ni, m, bi, vec);
      else if (n <= 4096) launch_small<T, 256, 2>(x, out, groups, ni, m, bi, vec);
      else if (n <= 8192) launch_small<T, 256, 4>(x, out, groups, ni, m, bi, vec);
      else launch_small<T, 256, 8>(x, out, groups, ni, m, bi, vec);
    });
    SXE_LAUNCH_CHECK();
    return out;
  }

  const bool vec = aligned && (n % 8 == 0 || groups == 1);
  const int64_t per_block = (n + 2047) / 2048;  // blocks a group can feed with one 8-value chunk per thread
  const int64_t share = std::max<int64_t>(1, (int64_t)kNumCUs * 8 / groups);
  const int bpg = (int)std::min<int64_t>(std::min(per_block, share), kMaxBlocksPerGroup);
  const int64_t blocks = groups * bpg;
  SXE_CHECK(blocks < (int64_t)1 << 31, "fake_quant: grid too large");
  const int passes = rp != nullptr ? 0 : (mode == kTernary ? 2 : 1);
  at::Tensor ws;
  float *ws0 = nullptr, *ws1 = nullptr;
  if (passes > 0) {
    ws = at::empty({passes * blocks * 2}, x.options().dtype(at::kFloat));
    ws0 = ws.data_ptr<float>();
    ws1 = passes == 2 ? ws0 + blocks * 2 : nullptr;
  }
  SXE_DISPATCH_DT(dt, T, {
    using S = typename dt_traits<T>::storage;
    const S* xp = reinterpret_cast<const S*>(x.data_ptr());
    S* op = reinterpret_cast<S*>(out.data_ptr());
    SXE_DISPATCH_BOOL(vec, VEC, {
      for (int pass = 0; pass < passes; ++pass) {
        hipLaunchKernelGGL((fq_stats_kernel<T, VEC>), dim3((unsigned)blocks), dim3(256), 0, cur_stream(), xp, n, bpg,
                           (int)mode, pass, pass == 0 ? (const float*)nullptr : (const float*)ws0, pass == 0 ? ws0 : ws1);
        SXE_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL((fq_apply_kernel<T, VEC>), dim3((unsigned)blocks), dim3(256), 0, cur_stream(), xp, op, n, bpg,
                         (int)mode, (int)bits, (const float*)ws0, (const float*)ws1, rp);
    });
  });
  SXE_LAUNCH_CHECK();
  return out;
}

}  // namespace fq
}  // namespace sxe

TORCH_LIBRARY_FRAGMENT(sxe, m) { m.def("fake_quant(Tensor x, int groups, int mode, int bits, Tensor? range) -> Tensor"); }
TORCH_LIBRARY_IMPL(sxe, CUDA, m) { m.impl("fake_quant", &sxe::fq::fake_quant); }
