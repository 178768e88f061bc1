// Matrix-core building blocks shared by every kernel that drives the MFMAs directly (64-wide waves,
// gfx950). Each primitive is defined and derived here, once; the kernel files refer to this header.
//
//   types       bf16x8 i16x4 i16x8 i32x8 f32x16 u32x4 u32x2
//   LDS image   ROWB, soff<D>, lds_row16<D>, lds_tr, lds_trA<D>: XOR-swizzled [rows][D bf16] tiles
//               readable by rows (ds_read_b128) and transposed (ds_read_b64_tr_b16)
//   MFMA        mfma (32x32x16 bf16), zero16, acc_row, acc_to_b, store_acc_t
//   softmax     xor32, fast_exp2, LOG2E, LN2
//   LDS-DMA     glds16 / glds4 (builtin), glds16_m0 / glds4_m0 (inline asm), vm_wait<N>,
//               vm_wait_all, raw_barrier
//   staging     RowStager: global -> registers -> swizzled LDS
#pragma once
#include <hip/hip_runtime.h>
#include "sxe_common.h"

namespace sxe {
namespace mf {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef short i16x8 __attribute__((ext_vector_type(8)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int ROWB = 256;  // bytes per LDS row of a 128-wide bf16 tile (the D = 128 instances below)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// Byte offset of 16-byte chunk `ch` (0..D/8-1) of row `row` in a swizzled [rows][D bf16] tile: the
// chunk index is XORed with a 4-bit function of the row (3 bits when a row has only 8 chunks) so
// both the row reads (ds_read_b128) and the transposed 4-row reads (ds_read_b64_tr_b16) spread over
// the banks. The XOR is an involution, which the direct-to-LDS loaders use: they write rows
// linearly and swizzle the per-lane SOURCE chunk instead. A tile narrower than its image (a 32- or
// 64-wide head in a D = 128 image) uses the first chunks of each row.
template <int D>
__device__ __forceinline__ int soff(int row, int ch) {
  constexpr int CH = D / 8;
  return row * (2 * D) + 16 * (ch ^ ((((row & 3) << 2) | ((row >> 2) & 3)) & (CH >= 16 ? 15 : CH - 1)));
}

template <int D>
__device__ __forceinline__ bf16x8 lds_row16(const char* base, int row, int ch) {
  return *reinterpret_cast<const bf16x8*>(base + soff<D>(row, ch));
}

// Transposed read: 4 consecutive rows x one column per lane (ds_read_b64_tr_b16). Within a group of
// 16 lanes, lane i addresses row i >> 2, 8-byte column group i & 3, and receives column i of the
// 16 the group covers, from all 4 rows.
__device__ __forceinline__ i16x4 lds_tr(const char* base, int byte_off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) i16x4*)(const_cast<char*>(base) + byte_off));
}

// Two transposed reads as one MFMA operand. Whole-vector bitcast: element-wise bf16 inserts from
// the tr-read result miscompile (hipcc 7.2).
__device__ __forceinline__ bf16x8 tr_pair(i16x4 lo, i16x4 hi) {
  const i16x8 c = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, c);
}

// A operand of a 32x32x16 MFMA taken from a row-major [rows][D] LDS tile, transposed:
// A[m = d][k] with d = 32*dt + (lane&31), k permuted to match an accumulator used as B operand
// (acc_to_b): element j of lane half h <- tile row (row0 + 8*(j>>2) + 4h + (j&3)), column d.
template <int D>
__device__ __forceinline__ bf16x8 lds_trA(const char* base, int row0, int dt, int lane) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3, h = g >> 1;
  const int ch = 4 * dt + 2 * (g & 1) + (p >> 1);
  const int row = row0 + 4 * h + q;
  return tr_pair(lds_tr(base, soff<D>(row, ch) + 8 * (p & 1)), lds_tr(base, soff<D>(row + 8, ch) + 8 * (p & 1)));
}

// accumulator register i <-> row within a 32x32 tile for lane half h (the column is lane & 31)
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// Accumulator-as-operand: registers 8s..8s+7 of a 32x32 accumulator, rounded to bf16, are the B
// operand of k-step s of a product over the accumulator's ROW index -- lane half h then holds rows
// acc_row(8s + j, h) = 16s + 8*(j>>2) + 4h + (j&3) as its k elements j = 0..7, not the MFMA's
// natural 8h + j. The A operand must use the same k order (lds_trA does); the permutation then
// cancels in the sum and the accumulator never goes through LDS.
__device__ __forceinline__ bf16x8 acc_to_b(const f32x16& a, int s) {
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = (__bf16)a[8 * s + e];
  return r;
}

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// Epilogue of a TRANSPOSED accumulator (the weight was the MFMA's A operand, so the 32x32 tile is
// Y^T): lane (l32, h) owns one output row and registers 4g .. 4g+3 are its columns 8g + 4h + 0..3.
// `y` points at that row's column 4h of the tile; one 8-byte store per run, no per-element branch
// or load (a per-element `if` + scale load makes hipcc wait vmcnt(0) -- i.e. for the previous
// store -- before every element).
__device__ __forceinline__ void store_acc_t(const f32x16& c, unsigned short* y, float s) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const unsigned lo = (unsigned)f32_to_bf16(c[4 * g] * s) | ((unsigned)f32_to_bf16(c[4 * g + 1] * s) << 16);
    const unsigned hi = (unsigned)f32_to_bf16(c[4 * g + 2] * s) | ((unsigned)f32_to_bf16(c[4 * g + 3] * s) << 16);
    *reinterpret_cast<unsigned long long*>(y + 8 * g) = (unsigned long long)lo | ((unsigned long long)hi << 32);
  }
}

// raw v_exp_f32: exp2f() wraps it in denormal range reduction, pure VALU overhead for softmax
// probabilities (a denormal p is 0 for every purpose here)
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// value of the lane 32 apart (lane ^ 32) via v_permlane32_swap: a VALU op instead of a
// ds_bpermute round trip through the LDS
__device__ __forceinline__ float xor32(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}

// ---------------------------------------------------------------------------------------------
// Direct-to-LDS loads (global_load_lds_dwordx4 / _dword): no staging registers; lane i's 16 (4)
// bytes land at the wave-uniform LDS base + 16 i (4 i). Two forms, because of the compiler's
// wait-count pass:
//  * glds16 / glds4, the builtin. The pass tracks it, but cannot tell the DMA's LDS writes from the
//    kernel's LDS reads, so it puts `s_waitcnt vmcnt(0)` before the first ds_read after every issue.
//    Use it where the loop waits for the stage it is about to read anyway and the reads of a stage
//    come before the next issue (grouped_gemm dp, mx_gemm dp).
//  * glds16_m0 / glds4_m0, inline asm the pass cannot see. Use it wherever loads must stay in flight
//    across ds_reads of other ring slots (flash_attn: with the builtin every dK/dV tile waited for
//    the NEXT tile's load before its first MFMA; gemm_wgrad: the whole prefetch drained each
//    K-step). Completion is then tracked by hand: a counted vm_wait<N>() or vm_wait_all(), then a
//    barrier, before any wave reads the slot. `lds_addr` is the wave-uniform LDS byte address, in
//    an SGPR; it goes to M0.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void glds16(const void* gsrc, char* lds) {
  __builtin_amdgcn_global_load_lds(gsrc, (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const void* gsrc, char* lds) {
  __builtin_amdgcn_global_load_lds(gsrc, (__attribute__((address_space(3))) void*)lds, 4, 0, 0);
}
__device__ __forceinline__ void glds16_m0(const void* gsrc, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_addr), "v"(gsrc) : "memory", "m0");
}
__device__ __forceinline__ void glds4_m0(const void* gsrc, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dword %1, off" ::"s"(lds_addr), "v"(gsrc) : "memory", "m0");
}

// Counted wait from inline asm: at most N of this wave's vector-memory operations still in flight.
// Invisible to the wait-count pass, like the _m0 loads it pairs with.
template <int N>
__device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// s_waitcnt vmcnt(0) through the builtin (expcnt / lgkmcnt fields left at their maxima), not inline
// asm: the compiler's wait-count pass then knows every load it tracks has landed, so it does not
// keep counting the operand loads issued before a tile loop as pending inside the loop (where its
// counted waits would also wait for the hand-tracked LDS-DMA)
__device__ __forceinline__ void vm_wait_all() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// s_barrier without __syncthreads()'s vmcnt(0): loads stay in flight across it
__device__ __forceinline__ void raw_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// Stage ROWS rows x DH bf16 (DH/8 16-byte chunks per row) from global into a swizzled [ROWS][128]
// LDS tile through registers, NTHREADS threads sharing the chunks: issue early with load(), write
// late with store(). Rows at or beyond `valid` read as zeros. (flash_attn.hip has a [ROWS][D] copy
// that cannot join without a change to its assembly; it says why.)
template <int ROWS, int DH, int NTHREADS>
struct RowStager {
  static constexpr int CPR = DH / 8;  // 16-byte chunks per row
  static constexpr int N = (ROWS * CPR + NTHREADS - 1) / NTHREADS;
  u32x4 r[N];
  __device__ __forceinline__ void load(const unsigned short* base, int64_t row_stride, int row0, int valid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = threadIdx.x + i * NTHREADS;
      const int row = c / CPR, ch = c % CPR;
      r[i] = (c < ROWS * CPR && row0 + row < valid)
                 ? *reinterpret_cast<const u32x4*>(base + (int64_t)(row0 + row) * row_stride + ch * 8)
                 : u32x4{0u, 0u, 0u, 0u};
    }
  }
  __device__ __forceinline__ void store(char* lds) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = threadIdx.x + i * NTHREADS;
      if (c < ROWS * CPR) *reinterpret_cast<u32x4*>(lds + soff<128>(c / CPR, c % CPR)) = r[i];
    }
  }
};

}  // namespace mf
}  // namespace sxe
