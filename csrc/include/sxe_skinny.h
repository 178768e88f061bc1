// What the decode ("skinny", M <= 16) GEMM kernels share: skinny_gemm.hip, mxfp.hip (skinny_gemm_fpxw)
// and skinny_dq.hip. All of them give one workgroup 16 output columns, split K over NW waves, sum the
// waves' partial 16x16 tiles through `red[NW][64]` in LDS and let wave 0 scale, add the bias and store
// bf16. Here: the host-side operand checks and wave plan, the dynamic-LDS opt-in, and the reduce.
#pragma once
#include "sxe_common.h"

namespace sxe {
namespace skinny {

// ---- host: operand checks. `op` is the entry point's name, the prefix of every message. ----------
// Activation: bf16 [M, K], unit column stride, 16-byte aligned rows, 1 <= M <= max_m.
inline const unsigned short* check_x(const at::Tensor& x, const char* op, int max_m) {
  SXE_CHECK(x.is_cuda(), op, ": x must be a GPU tensor");
  SXE_CHECK(x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.stride(1) == 1 && x.stride(0) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
            op, ": x bf16 [M, K], unit stride along K, 16-byte aligned rows");
  SXE_CHECK(x.size(0) >= 1 && x.size(0) <= max_m, op, ": 1 <= M <= ", max_m);
  return reinterpret_cast<const unsigned short*>(x.data_ptr());
}

// Optional bias: bf16 [N] contiguous, or nullptr.
inline const unsigned short* bias_ptr(const c10::optional<at::Tensor>& bias, int64_t N, const char* op) {
  if (!bias.has_value() || !bias->defined()) return nullptr;
  SXE_CHECK(bias->is_cuda() && bias->scalar_type() == at::kBFloat16 && bias->is_contiguous() && bias->numel() == N,
            op, ": bias bf16 [N]");
  return reinterpret_cast<const unsigned short*>(bias->data_ptr());
}

// Weight (or code plane): 2-D, row-major, every row 16-byte aligned.
inline void check_w_rows(const at::Tensor& w, const char* op) {
  SXE_CHECK(w.is_cuda() && w.dim() == 2 && w.stride(1) == 1 && w.stride(0) * w.element_size() % 16 == 0 &&
                reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0,
            op, ": w [N, K] row-major, 16-byte aligned rows");
}

// Per-output-row weight scale: fp32 [N] contiguous.
inline const float* row_scale_ptr(const at::Tensor& s, int64_t N, const char* op) {
  SXE_CHECK(s.is_cuda() && s.scalar_type() == at::kFloat && s.is_contiguous() && s.numel() == N, op, ": wscale fp32 [N]");
  return s.data_ptr<float>();
}

// ---- host: wave plan ------------------------------------------------------------------------------
// Waves per workgroup: NW = 8 (more waves streaming per CU) while the tiles still fit on the chip
// in ONE round -- at ~150 VGPRs (bf16) one 8-wave workgroup fits per CU, at ~115 (fp8) two -- and
// every wave keeps >= `min_ss` super-steps; otherwise NW = 4 (three / four workgroups per CU), so
// e.g. the 384-tile QKV projection does not run a second, half-empty round of 8-wave workgroups.
inline int pick_nw(int tiles, int ss_total, int min_ss, int wg8_per_cu) {
  int nw = 4;
  while (nw < 8 && (int64_t)tiles * nw < 4096 && ss_total >= min_ss * nw) nw *= 2;
  if (nw == 8 && tiles > kNumCUs * wg8_per_cu) nw = 4;
  return nw;
}
// `wg8_per_cu` for a kernel without the one-round cap: NW = 8 needs tiles * 4 < 4096, and a cap of
// 1024 tiles never binds below that.
constexpr int kNoRoundCap = 1024 / kNumCUs;
static_assert(kNumCUs * kNoRoundCap * 4 >= 4096, "kNoRoundCap must not bind");

// ---- host: dynamic LDS (sxe_common.h) -------------------------------------------------------------
using sxe::allow_max_dynamic_lds;
using sxe::kMaxDynamicLds;

// ---- device: the cross-wave reduce ----------------------------------------------------------------
// After `red[wave][lane] = acc; __syncthreads();`: the sum of the NW waves' partial tiles, for wave 0.
// (skinny_dq.hip keeps its own: it adds whole vectors, which compiles to different instructions.)
template <int NW>
__device__ __forceinline__ f32x4 reduce_waves(const f32x4 (&red)[NW][64], int lane) {
  f32x4 t = red[0][lane];
#pragma unroll
  for (int v = 1; v < NW; ++v) {
    const f32x4 u = red[v][lane];
    t[0] += u[0];
    t[1] += u[1];
    t[2] += u[2];
    t[3] += u[3];
  }
  return t;
}
// The scale + bias + bf16 store that follows stays in each kernel: moved into a helper here, the
// compiler commutes the operands of its adds / FMAs, so the kernels' assembly would no longer be
// the text it has been (same values, but tools/kernel_isa_diff.py compares text).

}  // namespace skinny
}  // namespace sxe
