// Group-wise quantization kernels (ZeRO++ quantized weights / gradients, MoQ, FP8 quantizer).
//
// Parity: reference csrc/quantization (``quantize`` / ``dequantize`` / ``swizzle_quant`` /
// ``quantized_reduction``, symmetric int8 / int4) and ops/fp_quantizer (FP8 e4m3 with per-group
// scales). MI355X design:
//  * one wave per quantization group (group sizes are multiples of 64, odd multiples included): a
//    lane handles the element pairs (2j, 2j+1), j = lane, lane+64, ... of its group and nothing
//    outside it; the absmax is a wave butterfly, no LDS. A group has group/2 pairs, so at group 64
//    only lanes 0..31 of the wave load and store (int8 included); the butterfly still spans 64
//    lanes. Measured on 64 MiB of bf16 (profiles/quant_kernel_edges.log): against the previous
//    lane-contiguous layout group 128 is 12% faster for all three kinds, int8 at group 64 -- the
//    only kind that layout got right there -- is 14% slower (75 -> 86 us) for the idle half wave;
//  * int4 packs two values per byte (low nibble first), int8 as-is, scales fp32 per group;
//  * scale policy: s = amax / qmax in fp32. NaN or +-Inf in a group gives a non-finite scale (NaN
//    wins), so every element of that group dequantizes to a non-finite value; the codes stay in
//    range. s == 0 (an all-zero group, or amax / qmax underflowing fp32) becomes 1 with all codes 0;
//  * codes are round(x * (1/s)). Where s is subnormal 1/s could overflow and turn an exact zero
//    into 0 * inf = NaN = +qmax; there the quotient is formed as (x * 2^64) * (1 / (s * 2^64)) --
//    both scalings are exact, so zeros give code 0 and the result equals x * (1/s) bit for bit
//    wherever that was finite;
//  * FP8 e4m3 conversion uses CDNA4's hardware converters (v_cvt_pk_fp8_f32 via the
//    __builtin_amdgcn_cvt_pk_fp8_f32 builtin, OCP e4m3 on gfx950) and v_cvt_f32_fp8 back;
//  * dequant_reduce fuses the qgZ receive side: W quantized chunks -> fp32 sum in one pass.
#include "sxe_common.h"
#include <torch/library.h>

namespace sxe {
namespace quant {

// |v| as an integer: for non-negative floats the bit patterns order like the values, every NaN
// pattern sorts above +Inf, so an integer max is an absmax that keeps NaN (fmaxf would drop it).
__device__ __forceinline__ int abs_bits(float v) { return (int)(__float_as_uint(v) & 0x7fffffffu); }

// Scale of one group, by the whole wave: s = amax / qmax. A lane reads the element pairs
// (2j, 2j + 1), j = lane, lane + 64, ... < group / 2 -- the pairing of the code loops below, inside the
// group for every multiple of 64. `up` is the pre-scale of the quotient (see the header).
template <DT T>
__device__ __forceinline__ float group_scale(const typename dt_traits<T>::storage* __restrict xg, int group, int lane,
                                             float qmax, float& inv, float& up) {
  int mb = 0;
  for (int j = lane; j < group / 2; j += 64) {
    mb = max(mb, abs_bits(to_f32<T>(xg[2 * j])));
    mb = max(mb, abs_bits(to_f32<T>(xg[2 * j + 1])));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mb = max(mb, __shfl_xor(mb, o, 64));
  float s = __uint_as_float((unsigned)mb) / qmax;
  if (s == 0.f) s = 1.f;  // all zeros, or amax / qmax underflows: the zero group (NaN != 0 stays NaN)
  up = s < 0x1p-126f ? 0x1p64f : 1.f;
  inv = 1.f / (s * up);
  return s;
}

template <DT T, int BITS>
__global__ void quant_kernel(const typename dt_traits<T>::storage* __restrict x, int64_t n_groups, int group,
                             uint8_t* __restrict q, float* __restrict scales) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  constexpr float qmax = BITS == 8 ? 127.f : 7.f;
  for (int64_t gi = wid; gi < n_groups; gi += nw) {
    const typename dt_traits<T>::storage* src = x + gi * group;
    float inv, up;
    const float s = group_scale<T>(src, group, lane, qmax, inv, up);
    if (lane == 0) scales[gi] = s;
    for (int j = lane; j < group / 2; j += 64) {
      const int a = (int)fmaxf(-qmax, fminf(qmax, rintf(to_f32<T>(src[2 * j]) * up * inv)));
      const int b = (int)fmaxf(-qmax, fminf(qmax, rintf(to_f32<T>(src[2 * j + 1]) * up * inv)));
      if constexpr (BITS == 8) {
        int8_t* dst = reinterpret_cast<int8_t*>(q) + gi * group + 2 * j;
        dst[0] = (int8_t)a;
        dst[1] = (int8_t)b;
      } else {
        q[gi * (group / 2) + j] = (uint8_t)((a & 0xF) | ((b & 0xF) << 4));
      }
    }
  }
}

template <DT T, int BITS>
__global__ void dequant_kernel(const uint8_t* __restrict q, const float* __restrict scales, int64_t n, int group,
                               typename dt_traits<T>::storage* __restrict out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float s = scales[i / group];
    float v;
    if constexpr (BITS == 8) {
      v = (float)reinterpret_cast<const int8_t*>(q)[i];
    } else {
      const uint8_t b = q[i >> 1];
      int nib = (i & 1) ? (b >> 4) : (b & 0xF);
      if (nib & 0x8) nib -= 16;
      v = (float)nib;
    }
    out[i] = from_f32<T>(v * s);
  }
}

// q: [W, m] quantized chunks (m values each), scales: [W, m / group]; out fp32 [m] = sum_w deq_w
template <int BITS>
__global__ void dequant_reduce_kernel(const uint8_t* __restrict q, const float* __restrict scales, int W, int64_t m,
                                      int group, float* __restrict out, float alpha, bool accumulate) {
  const int64_t bytes_per = BITS == 8 ? m : m / 2;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int w = 0; w < W; ++w) {
      const float s = scales[(int64_t)w * (m / group) + i / group];
      float v;
      if constexpr (BITS == 8) {
        v = (float)reinterpret_cast<const int8_t*>(q)[(int64_t)w * bytes_per + i];
      } else {
        const uint8_t b = q[(int64_t)w * bytes_per + (i >> 1)];
        int nib = (i & 1) ? (b >> 4) : (b & 0xF);
        if (nib & 0x8) nib -= 16;
        v = (float)nib;
      }
      acc += v * s;
    }
    out[i] = accumulate ? out[i] + alpha * acc : alpha * acc;
  }
}

// ---- FP8 e4m3 (OCP on gfx950) ---------------------------------------------------------------
template <DT T>
__global__ void fp8_quant_kernel(const typename dt_traits<T>::storage* __restrict x, int64_t n_groups, int group,
                                 uint8_t* __restrict q, float* __restrict scales) {
  const int lane = threadIdx.x & 63;
  const int64_t wid = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  constexpr float fmax8 = 448.f;
  for (int64_t gi = wid; gi < n_groups; gi += nw) {
    const typename dt_traits<T>::storage* src = x + gi * group;
    float inv, up;
    const float s = group_scale<T>(src, group, lane, fmax8, inv, up);
    if (lane == 0) scales[gi] = s;
    uint8_t* dst = q + gi * group;
    for (int j = lane; j < group / 2; j += 64) {
      const float a = fmaxf(-fmax8, fminf(fmax8, to_f32<T>(src[2 * j]) * up * inv));
      const float b = fmaxf(-fmax8, fminf(fmax8, to_f32<T>(src[2 * j + 1]) * up * inv));
      const int packed = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
      dst[2 * j] = (uint8_t)(packed & 0xFF);
      dst[2 * j + 1] = (uint8_t)((packed >> 8) & 0xFF);
    }
  }
}

template <DT T>
__global__ void fp8_dequant_kernel(const uint8_t* __restrict q, const float* __restrict scales, int64_t n, int group,
                                   typename dt_traits<T>::storage* __restrict out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = __builtin_amdgcn_cvt_f32_fp8((int)q[i], 0);
    out[i] = from_f32<T>(v * scales[i / group]);
  }
}

}  // namespace quant

static void check_group(const at::Tensor& x, int64_t group) {
  SXE_CHECK_CUDA(x);
  SXE_CHECK(x.is_contiguous(), "contiguous input");
  SXE_CHECK(group % 64 == 0 && group > 0, "group size must be a positive multiple of 64");
  SXE_CHECK(x.numel() % group == 0, "numel must be a multiple of the group size");
}

// what every dequantizer reads and writes: uint8 codes, fp32 scales, a contiguous output, one device
static void check_codes_scales(const at::Tensor& q, const at::Tensor& scales, const at::Tensor& out, const char* op) {
  SXE_CHECK(q.scalar_type() == at::kByte && q.is_contiguous(), op, ": q must be contiguous uint8");
  SXE_CHECK(scales.is_cuda() && scales.scalar_type() == at::kFloat && scales.is_contiguous(), op,
            ": scales must be contiguous fp32 on the GPU");
  SXE_CHECK(out.is_cuda() && out.is_contiguous(), op, ": out must be a contiguous GPU tensor");
}

// bits in {4, 8}: returns [q (uint8/int8 storage), scales fp32 [numel / group]]
std::vector<at::Tensor> quantize_sym(const at::Tensor& x, int64_t group, int64_t bits) {
  check_group(x, group);
  SXE_CHECK(bits == 8 || bits == 4, "bits must be 4 or 8");
  c10::DeviceGuard g(x.device());
  const int64_t n = x.numel(), ng = n / group;
  auto q = at::empty({bits == 8 ? n : n / 2}, x.options().dtype(at::kByte));
  auto s = at::empty({ng}, x.options().dtype(at::kFloat));
  if (n == 0) return {q, s};
  const int blocks = stream_grid(ng * 64, 256);
  SXE_DISPATCH_DT(dtype_of(x), T, {
    using st = typename dt_traits<T>::storage;
    if (bits == 8)
      hipLaunchKernelGGL((quant::quant_kernel<T, 8>), dim3(blocks), dim3(256), 0, cur_stream(),
                         reinterpret_cast<const st*>(x.data_ptr()), ng, (int)group, q.data_ptr<uint8_t>(), s.data_ptr<float>());
    else
      hipLaunchKernelGGL((quant::quant_kernel<T, 4>), dim3(blocks), dim3(256), 0, cur_stream(),
                         reinterpret_cast<const st*>(x.data_ptr()), ng, (int)group, q.data_ptr<uint8_t>(), s.data_ptr<float>());
  });
  SXE_LAUNCH_CHECK();
  return {q, s};
}

void dequantize_sym_(const at::Tensor& q, const at::Tensor& scales, int64_t group, int64_t bits, at::Tensor out) {
  SXE_CHECK_CUDA(q);
  SXE_CHECK(bits == 8 || bits == 4, "dequantize_sym_: bits must be 4 or 8");
  SXE_CHECK(group > 0 && (bits == 8 || group % 2 == 0), "dequantize_sym_: group must be positive, and even for int4");
  check_codes_scales(q, scales, out, "dequantize_sym_");
  c10::DeviceGuard g(q.device());
  const int64_t n = out.numel();
  SXE_CHECK(scales.numel() * group == n && q.numel() == (bits == 8 ? n : n / 2), "dequantize_sym_: size mismatch");
  if (n == 0) return;
  SXE_DISPATCH_DT(dtype_of(out), T, {
    using st = typename dt_traits<T>::storage;
    if (bits == 8)
      hipLaunchKernelGGL((quant::dequant_kernel<T, 8>), dim3(stream_grid(n, 256)), dim3(256), 0, cur_stream(),
                         q.data_ptr<uint8_t>(), scales.data_ptr<float>(), n, (int)group, reinterpret_cast<st*>(out.data_ptr()));
    else
      hipLaunchKernelGGL((quant::dequant_kernel<T, 4>), dim3(stream_grid(n, 256)), dim3(256), 0, cur_stream(),
                         q.data_ptr<uint8_t>(), scales.data_ptr<float>(), n, (int)group, reinterpret_cast<st*>(out.data_ptr()));
  });
  SXE_LAUNCH_CHECK();
}

// q: [W * bytes(m)] chunks of m values, scales [W * m / group]; out fp32 [m] (+)= alpha * sum_w
void dequant_reduce_(const at::Tensor& q, const at::Tensor& scales, int64_t W, int64_t group, int64_t bits,
                     at::Tensor out, double alpha, bool accumulate) {
  SXE_CHECK_CUDA(q);
  SXE_CHECK(bits == 8 || bits == 4, "dequant_reduce_: bits must be 4 or 8");
  SXE_CHECK(W > 0 && group > 0 && (bits == 8 || group % 2 == 0),
            "dequant_reduce_: W and group must be positive, group even for int4");
  SXE_CHECK(out.scalar_type() == at::kFloat, "dequant_reduce_: out must be fp32");
  check_codes_scales(q, scales, out, "dequant_reduce_");
  c10::DeviceGuard g(q.device());
  const int64_t m = out.numel();
  SXE_CHECK(m % group == 0 && scales.numel() == W * (m / group), "dequant_reduce_: scales size");
  SXE_CHECK(q.numel() == W * (bits == 8 ? m : m / 2), "dequant_reduce_: q must hold W chunks of m values");
  if (m == 0) return;
  if (bits == 8)
    hipLaunchKernelGGL(quant::dequant_reduce_kernel<8>, dim3(stream_grid(m, 256)), dim3(256), 0, cur_stream(),
                       q.data_ptr<uint8_t>(), scales.data_ptr<float>(), (int)W, m, (int)group, out.data_ptr<float>(),
                       (float)alpha, accumulate);
  else
    hipLaunchKernelGGL(quant::dequant_reduce_kernel<4>, dim3(stream_grid(m, 256)), dim3(256), 0, cur_stream(),
                       q.data_ptr<uint8_t>(), scales.data_ptr<float>(), (int)W, m, (int)group, out.data_ptr<float>(),
                       (float)alpha, accumulate);
  SXE_LAUNCH_CHECK();
}

std::vector<at::Tensor> quantize_fp8(const at::Tensor& x, int64_t group) {
  check_group(x, group);
  c10::DeviceGuard g(x.device());
  const int64_t n = x.numel(), ng = n / group;
  auto q = at::empty({n}, x.options().dtype(at::kByte));
  auto s = at::empty({ng}, x.options().dtype(at::kFloat));
  if (n == 0) return {q, s};
  SXE_DISPATCH_DT(dtype_of(x), T, {
    using st = typename dt_traits<T>::storage;
    hipLaunchKernelGGL((quant::fp8_quant_kernel<T>), dim3(stream_grid(ng * 64, 256)), dim3(256), 0, cur_stream(),
                       reinterpret_cast<const st*>(x.data_ptr()), ng, (int)group, q.data_ptr<uint8_t>(), s.data_ptr<float>());
  });
  SXE_LAUNCH_CHECK();
  return {q, s};
}

void dequantize_fp8_(const at::Tensor& q, const at::Tensor& scales, int64_t group, at::Tensor out) {
  SXE_CHECK_CUDA(q);
  SXE_CHECK(group > 0, "dequantize_fp8_: group must be positive");
  check_codes_scales(q, scales, out, "dequantize_fp8_");
  c10::DeviceGuard g(q.device());
  const int64_t n = out.numel();
  SXE_CHECK(q.numel() == n && scales.numel() * group == n, "dequantize_fp8_: size mismatch");
  if (n == 0) return;
  SXE_DISPATCH_DT(dtype_of(out), T, {
    using st = typename dt_traits<T>::storage;
    hipLaunchKernelGGL((quant::fp8_dequant_kernel<T>), dim3(stream_grid(n, 256)), dim3(256), 0, cur_stream(),
                       q.data_ptr<uint8_t>(), scales.data_ptr<float>(), n, (int)group, reinterpret_cast<st*>(out.data_ptr()));
  });
  SXE_LAUNCH_CHECK();
}

}  // namespace sxe

TORCH_LIBRARY_FRAGMENT(sxe, m) {
  m.def("quantize_sym(Tensor x, int group, int bits) -> Tensor[]");
  m.def("dequantize_sym_(Tensor q, Tensor scales, int group, int bits, Tensor(a!) out) -> ()");
  m.def("dequant_reduce_(Tensor q, Tensor scales, int W, int group, int bits, Tensor(a!) out, float alpha, "
        "bool accumulate) -> ()");
  m.def("quantize_fp8(Tensor x, int group) -> Tensor[]");
  m.def("dequantize_fp8_(Tensor q, Tensor scales, int group, Tensor(a!) out) -> ()");
}
TORCH_LIBRARY_IMPL(sxe, CUDA, m) {
  m.impl("quantize_sym", &sxe::quantize_sym);
  m.impl("dequantize_sym_", &sxe::dequantize_sym_);
  m.impl("dequant_reduce_", &sxe::dequant_reduce_);
  m.impl("quantize_fp8", &sxe::quantize_fp8);
  m.impl("dequantize_fp8_", &sxe::dequantize_fp8_);
}
