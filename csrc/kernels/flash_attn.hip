// Flash attention forward + backward for gfx950 (MI355X), bf16 in / fp32 accumulate, head dims 64,
// 128 and 256 (templated: no zero-padding of the head dim), causal or full, GQA, query length !=
// key length (cross / prefix / chunked-prefill attention: the causal mask is bottom-right aligned by
// `qoff`, query i sees keys <= i + qoff), arbitrary [B, S, H, D] strides (so the fused QKV projection
// output is read in place and dq/dk/dv are written straight into one dqkv buffer).
//
// Reference users: FPDT's chunked attention with LSE merging (deepspeed/sequence/fpdt_layer.py:134-460),
// Ulysses local attention (sequence/layer.py:434), the Triton flash kernels of the inference path
// (ops/transformer/inference/triton/attention.py:263, triton_ops.py:16) and the external
// flash-attn the FastGen blocked_flash op calls (inference/v2/kernels/ragged_ops/blocked_flash/).
//
// CDNA4 design (see /opt/skills/guides/cdna_hip_programming.md §3, §5.5 T2/T10/T12-T14, App. B):
//  * v_mfma_f32_32x32x16_bf16 everywhere; 64-wide waves; one wave owns 32 query rows (fwd, dQ)
//    or 32 key rows (dK/dV);
//  * "swapped" products: the forward computes S^T = K Q^T so one lane holds one query's scores
//    (softmax max/sum are lane-local + one lane^32 exchange, the rescale is a per-lane scalar),
//    and S^T is consumed directly as the B operand of O^T += V^T P^T (the accumulator-as-operand
//    identity of guide §3, with its permuted k order), so P never touches LDS;
//  * V^T / K^T / Q^T / dO^T operands come from row-major LDS tiles through ds_read_b64_tr_b16
//    (hardware transpose), with the XOR-swizzled 256-byte-row image that is conflict-free for
//    both the row reads (ds_read_b128) and the transposed reads (guide T10, image (b));
//  * K/V (or Q/dO) tiles are register-staged one tile ahead (T14 issue-early/write-late) into a
//    double-buffered LDS ring: one barrier per tile;
//  * backward = pre-pass (-delta = -rowsum(dO * O), lse * log2(e)) + dQ kernel (forward-shaped) +
//    dK/dV kernel (keys on lanes, dK^T/dV^T accumulated in registers across the GQA query heads): no
//    atomics, deterministic.
//  * heavy-first block order for the causal triangle.
#include "sxe_common.h"
#include "sxe_mfma.h"
#include <torch/library.h>
#include <type_traits>

namespace sxe {
namespace fa {
using namespace mf;  // swizzled LDS image, transposed reads, MFMA helpers, LDS-DMA: see sxe_mfma.h

constexpr int NW = 4;           // waves per workgroup
constexpr int QW = 32;          // rows per wave
constexpr int QB = NW * QW;     // 128 rows per workgroup
constexpr int KT = 64;          // keys per K/V tile (forward / dQ)

// Per-lane byte offsets of mf::lds_row16 and mf::lds_trA, computed once per kernel: the swizzle only
// looks at the low 4 row bits, so for a tile row base row0 that is a multiple of 16
//   lds_row16(base, row0 + r, 2 t2 + h)  = base + 2D row0 + row[t2]
//   lds_trA(base, row0, dt, lane)        = tr_read(base + 2D row0, tr[dt][0], tr[dt][1])
// and every read in a tile loop is a hoisted VGPR plus an instruction immediate (recomputed per read,
// the XOR'd offsets cost ~40 VALU adds per forward tile).
template <int D>
struct LaneOffs {
  int row[D / 16];
  int tr[D / 32][2];
  __device__ __forceinline__ void init(int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int t2 = 0; t2 < D / 16; ++t2) row[t2] = soff<D>(r, 2 * t2 + h);
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3, hh = g >> 1;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) {
      const int ch = 4 * dt + 2 * (g & 1) + (p >> 1);
      tr[dt][0] = soff<D>(4 * hh + q, ch) + 8 * (p & 1);
      tr[dt][1] = soff<D>(4 * hh + q + 8, ch) + 8 * (p & 1);
    }
  }
};
__device__ __forceinline__ bf16x8 lds_row_at(const char* base, int off) {
  return *reinterpret_cast<const bf16x8*>(base + off);
}
__device__ __forceinline__ bf16x8 lds_tr_at(const char* base, const int (&o)[2]) {
  return tr_pair(lds_tr(base, o[0]), lds_tr(base, o[1]));
}

struct Strides {
  int64_t b, s, h;  // element strides; d is unit stride
};

// mf::RowStager for a [ROWS][D] tile, kept as a local copy for two reasons: it has no bounds test
// on the chunk index (ROWS * CH is a multiple of the thread count), and its store() evaluates the
// XOR term of mf::soff BEFORE the row offset, where mf::soff evaluates it after -- hipcc schedules
// the non-DMA forward kernels differently for the two orders. Merge the two when those kernels are
// next re-measured.
template <int ROWS, int NWAVES, int D>
struct Stager {
  static constexpr int CH = D / 8;
  static constexpr int N = ROWS * CH / (NWAVES * 64);
  u32x4 r[N];
  __device__ __forceinline__ void load(const unsigned short* base, int64_t row_stride, int row0, int nrows_valid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = threadIdx.x + i * NWAVES * 64;
      const int row = c / CH, ch = c % CH;
      if (row0 + row < nrows_valid)
        r[i] = *reinterpret_cast<const u32x4*>(base + (int64_t)(row0 + row) * row_stride + ch * 8);
      else
        r[i] = u32x4{0, 0, 0, 0};
    }
  }
  __device__ __forceinline__ void store(char* lds) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = threadIdx.x + i * NWAVES * 64;
      const int row = c / CH, ch = c % CH;
      const int f = (((row & 3) << 2) | ((row >> 2) & 3)) & (CH >= 16 ? 15 : CH - 1);
      *reinterpret_cast<u32x4*>(lds + (row * (2 * D) + 16 * (ch ^ f))) = r[i];
    }
  }
};

// Block-sparse attention (reference ops/sparse_attention: Triton SDD/DSD matmuls + block softmax):
// a uint8 layout [H, nb, nb] over blk x blk blocks (blk in {16, 32, 64, 128, ...}, a multiple of 16)
// says which (query block, key block) pairs exist. The kernels below walk only the K (or Q) tiles
// that intersect a non-zero block -- a compacted tile list built in LDS at kernel start -- and mask
// scores element-wise inside them, so compute and HBM traffic scale with the layout's density.
struct Sparse {
  const uint8_t* layout;  // nullptr = dense
  int blk, nb;
};

// Build the list of tiles [t_lo, t_hi) of `tile` rows along one axis whose block range intersects
// a non-zero block of rows [r_lo, r_hi) along the other axis; `q_axis_rows` says whether the fixed
// range is the query axis. Returns the count (also in list[-1]); all threads participate.
__device__ __forceinline__ int build_tile_list(const Sparse sp, int head, int t_lo, int t_hi, int tile, int r_lo,
                                               int r_hi, bool fixed_is_query, int* list) {
  int* flags = list + 1024;  // scratch after the list (t_hi - t_lo <= 1024)
  for (int t = t_lo + (int)threadIdx.x; t < t_hi; t += blockDim.x) {
    const int a0 = r_lo / sp.blk, a1 = (r_hi - 1) / sp.blk;
    const int b0 = (t * tile) / sp.blk, b1 = (t * tile + tile - 1) / sp.blk;
    int act = 0;
    for (int a = a0; a <= a1 && !act; ++a)
      for (int bb = b0; bb <= b1; ++bb) {
        const int qb_ = fixed_is_query ? a : bb, kb_ = fixed_is_query ? bb : a;
        if (sp.layout[((int64_t)head * sp.nb + qb_) * sp.nb + kb_]) { act = 1; break; }
      }
    flags[t - t_lo] = act;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int t = t_lo; t < t_hi; ++t)
      if (flags[t - t_lo]) list[n++] = t;
    list[-1] = n;
  }
  __syncthreads();
  return list[-1];
}

// Band mask (packed documents and / or a sliding window, on top of the causal mask): query i sees keys
// klo[i] <= j <= i, equivalently key j is seen by queries j <= i <= qhi[j]. Both int32 [B, S], non-decreasing
// along S (a precondition of the raw ops, not checked on the device: a workgroup takes its first K/V tile
// from the klo of its first row and the end of its query sweep from the qhi of its last key). Every
// value is clamped on read -- klo to [0, i], qhi to [j, S - 1] -- and every tile index derives from the
// clamped values, so wrong bounds give wrong numbers but never an out-of-range tile or address.
// Band mode needs causal, Sq == Sk, causal offset 0 and a dense layout (checked on the host).
struct Band {
  const int* klo;  // nullptr = no band
  const int* qhi;
};
__device__ __forceinline__ int band_klo(const Band& bd, int b, int S, int i) {
  return min(max(bd.klo[(int64_t)b * S + i], 0), i);
}
__device__ __forceinline__ int band_qhi(const Band& bd, int b, int S, int j) {
  return max(min(bd.qhi[(int64_t)b * S + j], S - 1), j);
}

// Ragged (variable-length) forward: q / k / v / o are [T, H, D] token buffers holding sequences back to
// back, and an int32 work table [N, 3] lists one (first row, length, query block) entry per workgroup
// and head -- the query blocks are aligned to their sequence's first row, not to multiples of 128 of
// the buffer. Entries are clamped on read (first row to [0, T - 1], length to [1, T - first row], block
// to the sequence's last) and every address derives from the clamped values. `window` >= 1: query i of
// a sequence sees its keys max(0, i - window + 1) .. i (the host passes 2^30 for "no window"); the bound
// is computed from the sequence-local index, there are no per-token bounds arrays.
struct Varlen {
  const int* table;
  int T, window;
};

// Heavy-first mapping of the flat block index onto (b, head, row-block) for the causal triangle.
__device__ __forceinline__ void map_block(int nblk, int BH, bool heavy_last_index, int& bh, int& blk) {
  const int idx = blockIdx.x;
  const int rank = idx / BH;
  bh = idx - rank * BH;
  blk = heavy_last_index ? (nblk - 1 - rank) : rank;
}

// =============================================================================================
// Direct-to-LDS tile loads (global_load_lds_dwordx4): no staging registers. A wave-instruction
// writes 1 KiB = 1024 / (2 D) rows linearly, so the XOR swizzle goes on the per-lane SOURCE chunk
// (the swizzle is an involution: position c' of row `row` holds logical chunk c' ^ f(row)).
// =============================================================================================
//
// Issued with mf::glds16_m0 / glds4_m0, the inline-asm form (sxe_mfma.h says why): the loads stay in
// flight across the ring's ds_reads, and every consumer runs vm_wait_all() + a barrier before it
// reads a slot.
extern __shared__ __attribute__((aligned(16))) char smem[];  // every kernel's dynamic LDS
// M0 value of a wave-uniform pointer into smem: the symbol's LDS address plus the byte offset (a
// generic-to-LDS cast of the pointer itself costs a 64-bit null check per DMA instruction)
__device__ __forceinline__ unsigned lds_addr(const char* p) {
  return __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem +
                                        (unsigned)(p - smem));
}
// CLAMP (varlen forward): rows past `rmax` re-read row `rmax`, so no row beyond a sequence's last is
// ever fetched (the tail mask drops their scores; their V rows are finite copies, never junk)
template <int ROWS, int D, int NWV = NW, bool CLAMP = false>
__device__ __forceinline__ void tile_glds(const unsigned short* base, int64_t row_stride, int row0, char* lds,
                                          int rmax = 0) {
  constexpr int CH = D / 8, RPK = 64 / CH;  // rows per 1 KiB wave-instruction
  static_assert(ROWS % (RPK * NWV) == 0, "tile rows must split evenly over the waves");
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int i = 0; i < ROWS / RPK / NWV; ++i) {
    const int n = i * NWV + w;
    const int row = RPK * n + lane / CH;
    const int cpos = lane % CH;
    const int ch = cpos ^ ((((row & 3) << 2) | ((row >> 2) & 3)) & (CH >= 16 ? 15 : CH - 1));
    const int grow = CLAMP ? min(row0 + row, rmax) : row0 + row;
    glds16_m0(base + (int64_t)grow * row_stride + ch * 8, lds_addr(lds + n * 1024));
  }
}


// =============================================================================================
// Forward. Grid: (Sq / rows per workgroup) * B * H blocks. q: [B, Sq, *, D], k/v/o: [B, Sk, *, D]
// strided; lse [B, H, Sq]. Causal: query i sees keys <= i + qoff (qoff = Sk - Sq unless padded).
// =============================================================================================
// One K/V tile of a wave's online softmax. MASK = false is the interior-tile body (no causal
// diagonal, no padded tail, dense): none of the per-score compares / selects are emitted -- on
// the Llama-3 shape ~90 % of the tiles take it; the masked body handles the diagonal, the kv_len
// tail and block-sparse layouts. BAND (band kernels only): `band` says the tile holds keys below the
// klo of some row of the wave; `kl` is this lane's (clamped) klo.
template <bool MASK, int D, bool BAND = false>
__device__ __forceinline__ void fwd_tile(const LaneOffs<D>& lo, const char* kt, const char* vt, const bf16x8 (&qf)[D / 16],
                                         f32x16 (&oacc)[D / 32], float& m, float& l, float c, int kbase, int qpos,
                                         int r, int h, int lane, bool diag, bool tail, int kvlen, const uint8_t* lrow,
                                         int blk, bool band = false, int kl = 0) {
  // causal diagonal tile whose second 32-key half lies entirely above this wave's last query
  // (the wave's queries start at the tile's first key): that half's QK^T and PV MFMAs are skipped
  const bool skip1 = MASK && diag && !tail && lrow == nullptr && !(BAND && band) && kbase + 32 > qpos + QW - 1;
  f32x16 s[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    s[j] = zero16();
    if (j == 1 && skip1) break;
#pragma unroll
    for (int t2 = 0; t2 < D / 16; ++t2) s[j] = mfma(lds_row_at(kt + 32 * j * 2 * D, lo.row[t2]), qf[t2], s[j]);
  }
  // raw scores: the max is taken before scaling (c > 0) and the scale folds into the exp's FMA
  float mx = -INFINITY;
  // key - query offsets of this lane's first score row; opaque, so the compares below keep
  // compile-time row constants instead of 32 hoisted per-row thresholds per mask (VGPRs)
  int dd = kbase + 4 * h - qpos - r, dl = kbase + 4 * h - kvlen;
  if (MASK) asm volatile("" : "+v"(dd), "+v"(dl));
  int db = kbase + 4 * h - kl;  // key - klo of this lane's first score row
  if (BAND) asm volatile("" : "+v"(db));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    bool b0 = true, b1 = true;  // layout bits of keys kbase+32j+[0,16) and +[16,32)
    if (MASK && lrow) {
      b0 = lrow[(kbase + 32 * j) / blk] != 0;
      b1 = lrow[(kbase + 32 * j + 16) / blk] != 0;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float x = s[j][i];
      if (MASK) {
        if (diag && dd + 32 * j + acc_row(i, 0) > 0) x = -INFINITY;
        if (tail && dl + 32 * j + acc_row(i, 0) >= 0) x = -INFINITY;
        if (!(i < 8 ? b0 : b1)) x = -INFINITY;
        if (BAND && band && db + 32 * j + acc_row(i, 0) < 0) x = -INFINITY;
        s[j][i] = x;
      }
      mx = fmaxf(mx, x);
    }
  }
  mx = fmaxf(mx, xor32(mx)) * c;
  // lazy rescale: the reference max only moves when the tile max exceeds it by > 2^8, so
  // p <= 256 (harmless in fp32 / bf16) and the O rescale is skipped whenever no lane of the wave
  // moved (most tiles after the first few)
  const bool grow = mx > m + 8.f;
  const float mnew = grow ? mx : m;
  const float mref = (mnew == -INFINITY) ? 0.f : mnew;
  const float alpha = fast_exp2(m - mref);
  float ps = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float p = fast_exp2(__builtin_fmaf(s[j][i], c, -mref));
      s[j][i] = p;
      ps += p;
    }
  l = l * alpha + ps;
  m = mnew;
  if (__any(grow)) {
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j == 1 && skip1) break;  // its p are all exp2(-inf) = 0
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const bf16x8 pb = acc_to_b(s[j], s2);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
        oacc[dt] = mfma(lds_tr_at(vt + (32 * j + 16 * s2) * 2 * D, lo.tr[dt]), pb, oacc[dt]);
    }
  }
}

// Waves per workgroup (each 32 queries): NWF = 8 (256 queries; one workgroup of 2 waves per SIMD
// per CU) shares every staged K/V tile among twice the queries of NWF = 4, which serves sequences
// that are not a multiple of 256 and head dim 256 (whose accumulators need a whole SIMD's
// register file: 1 wave per SIMD).
template <int D, int NWF>
constexpr int fwd_min_waves() { return D >= 256 ? 1 : 8 / NWF; }

// DMA: K/V tiles go straight to LDS (global_load_lds from inline asm, see tile_glds) instead of through
// the register Stager; head dim 256 always (staging registers would not fit next to its 128
// accumulator + 64 Q-fragment registers), smaller head dims by default (SXE_FA_FWD_DMA=0 selects the
// register Stager: 4-7 % slower at D 128, B4 S2048 to B1 S32k, equal at D 64 --
// profiles/r05/attn_fwd_dma_ab.log)
// The body is shared by fwd_kernel (dense / sparse) and fwd_band_kernel (BAND: the tile walk starts at
// the first tile the workgroup's first row sees, a wave skips the tiles wholly below its first row's
// klo, and tiles that the klo of its last row cuts take the masked body with one more compare).
// VARLEN (fwd_varlen_kernel, always with BAND and DMA): the workgroup takes its sequence and query block
// from the work table; the sequence is then one batch row of length Sq = Sk = kvlen = its length. Q, K
// and V rows past the sequence's last re-read that last row (no row at or beyond T is touched: an
// unwritten V row with NaN bits would poison P V even under a zero weight), keys past it fall to the
// tail mask, query rows past it are computed and not stored, and no LSE is written.
template <bool SPARSE, int NWF, int D, bool DMA, bool BAND, bool VARLEN = false>
__device__ __forceinline__ void fwd_body(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, unsigned short* __restrict__ o, Strides os,
    float* __restrict__ lse, int B, int H, int Hk, int Sq, int Sk, float scale, int causal, Sparse sp, int kvlen,
    int qoff, Band bd, Varlen vl = Varlen{nullptr, 0, 0}) {
  constexpr int ROWB = 2 * D;
  constexpr int BUF = 2 * KT * ROWB;  // one ring slot = K tile + V tile
  int* tlist = reinterpret_cast<int*>(smem + 4 * KT * ROWB) + 1;
  constexpr int QBF = NWF * QW;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  const int nqb = Sq / QBF;
  int bh, qb;
  if constexpr (VARLEN) {
    const int e = blockIdx.x / H;
    const int* te = vl.table + 3 * (int64_t)e;
    const int start = min(max(te[0], 0), vl.T - 1);
    Sq = Sk = kvlen = min(max(te[1], 1), vl.T - start);
    qb = min(max(te[2], 0), (Sq - 1) / QBF);
    bh = blockIdx.x - e * H;  // the sequence is batch row 0 of the shifted pointers
    q += start * qs.s;
    k += start * ks.s;
    v += start * vs.s;
    o += start * os.s;
  } else {
    map_block(nqb, B * H, causal != 0, bh, qb);
  }
  const int b = bh / H, head = bh - b * H;
  const int kh = head / (H / Hk);
  const int q0 = qb * QBF + w * QW;  // this wave's first query
  const int qpos = q0 + qoff;        // its position on the key axis (causal diagonal)
  const unsigned short* qp = q + b * qs.b + head * qs.h;
  const unsigned short* kp = k + b * ks.b + kh * ks.h;
  const unsigned short* vp = v + b * vs.b + kh * vs.h;
  const float c = scale * LOG2E;

  bf16x8 qf[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t)
    qf[t] = *reinterpret_cast<const bf16x8*>(qp + (int64_t)(VARLEN ? min(q0 + r, Sq - 1) : q0 + r) * qs.s + 16 * t +
                                             8 * h);

  f32x16 oacc[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t) oacc[t] = zero16();
  float m = -INFINITY, l = 0.f;

  // keys needed by the workgroup (causal: up to its last query's diagonal)
  const int kend = causal ? min(Sk, (qb + 1) * QBF + qoff) : Sk;
  const int nkt = (max(kend, 0) + KT - 1) / KT;
  // band: first tile of the workgroup, this lane's klo and the klo of the wave's first / last row
  auto klo_at = [&](int i) {
    if constexpr (VARLEN) return max(i - vl.window + 1, 0);
    else return band_klo(bd, b, Sq, i);
  };
  const int tfirst = BAND ? klo_at(qb * QBF) / KT : 0;
  const int kl = BAND ? klo_at(q0 + r) : 0;
  const int kl_lo = BAND ? __builtin_amdgcn_readfirstlane(kl) : 0;
  const int kl_hi = BAND ? __builtin_amdgcn_readlane(kl, QW - 1) : 0;
  const int ntiles = SPARSE ? build_tile_list(sp, head, 0, nkt, KT, qb * QBF, qb * QBF + QBF, true, tlist)
                            : (BAND ? nkt - tfirst : nkt);
  auto tile_at = [&](int i) { return SPARSE ? tlist[i] : (BAND ? tfirst + i : i); };
  const uint8_t* lrow = SPARSE ? sp.layout + ((int64_t)head * sp.nb + (q0 + r) / sp.blk) * sp.nb : nullptr;
  Stager<KT, NWF, D> sk, sv;
  const int t0 = ntiles > 0 ? tile_at(0) : 0;
  if constexpr (DMA) {
    if (ntiles > 0) {
      tile_glds<KT, D, NWF, VARLEN>(kp, ks.s, t0 * KT, smem, Sk - 1);
      tile_glds<KT, D, NWF, VARLEN>(vp, vs.s, t0 * KT, smem + KT * ROWB, Sk - 1);
    }
    vm_wait_all();
  } else {
    sk.load(kp, ks.s, t0 * KT, Sk);
    sv.load(vp, vs.s, t0 * KT, Sk);
    sk.store(smem);
    sv.store(smem + KT * ROWB);
  }
  __syncthreads();
  LaneOffs<D> lo;
  lo.init(lane);
  // the tile loop runs unrolled by two so the ring slot is a compile-time constant in each copy: every
  // LDS address is then a hoisted per-lane offset plus an instruction immediate (with a runtime slot
  // each K / V read paid a VALU add per tile -- ~50 of the interior tile's ~200 VALU instructions)
  auto step = [&](const int t, auto slot) {
    constexpr int CUR = decltype(slot)::value;
    const bool more = (t + 1) < ntiles;
    if (more) {
      if constexpr (DMA) {
        tile_glds<KT, D, NWF, VARLEN>(kp, ks.s, tile_at(t + 1) * KT, smem + (CUR ^ 1) * BUF, Sk - 1);
        tile_glds<KT, D, NWF, VARLEN>(vp, vs.s, tile_at(t + 1) * KT, smem + (CUR ^ 1) * BUF + KT * ROWB, Sk - 1);
      } else {
        sk.load(kp, ks.s, tile_at(t + 1) * KT, Sk);
        sv.load(vp, vs.s, tile_at(t + 1) * KT, Sk);
      }
    }
    const int kbase = tile_at(t) * KT;
    // a wave whose queries all precede this tile has nothing to add (causal)
    const bool active = (!causal || kbase <= qpos + QW - 1) && !(BAND && kbase + KT - 1 < kl_lo) &&
                        !(VARLEN && q0 >= Sq);  // (varlen: a wave wholly past the sequence's end)
    if (active) {
      const char* kt = smem + CUR * BUF;
      const char* vt = kt + KT * ROWB;
      const bool diag = causal && (kbase + KT - 1 > qpos);
      const bool tail = kbase + KT > kvlen;  // keys past the valid length (padded key axis)
      const bool band = BAND && kbase < kl_hi;
      if (SPARSE || diag || tail || band)
        fwd_tile<true, D, BAND>(lo, kt, vt, qf, oacc, m, l, c, kbase, qpos, r, h, lane, diag, tail, kvlen, lrow,
                                SPARSE ? sp.blk : 1, band, kl);
      else
        fwd_tile<false, D>(lo, kt, vt, qf, oacc, m, l, c, kbase, qpos, r, h, lane, false, false, kvlen, nullptr, 1);
    }
    if constexpr (DMA) {
      vm_wait_all();
    } else if (more) {
      sk.store(smem + (CUR ^ 1) * BUF);
      sv.store(smem + (CUR ^ 1) * BUF + KT * ROWB);
    }
    __syncthreads();
  };
  for (int t = 0; t < ntiles; t += 2) {
    step(t, std::integral_constant<int, 0>{});
    if (t + 1 < ntiles) step(t + 1, std::integral_constant<int, 1>{});
  }
  const float lt = l + __shfl_xor(l, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;  // a fully masked row outputs zeros
  unsigned short* op = o + b * os.b + head * os.h + (int64_t)(q0 + r) * os.s;
  if (VARLEN && q0 + r >= Sq) return;  // the last block's overhang: those rows are the next sequence's
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      u16x4 pk;
#pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = f32_to_bf16(oacc[dt][4 * rg + e] * inv);
      *reinterpret_cast<u16x4*>(op + 32 * dt + 8 * rg + 4 * h) = pk;
    }
  if (VARLEN) return;
  if (h == 0) lse[((int64_t)b * H + head) * Sq + q0 + r] = lt > 0.f ? (m + log2f(lt)) * LN2 : INFINITY;
}

template <bool SPARSE, int NWF, int D, bool DMA = (D >= 256)>
__global__ void __launch_bounds__(NWF * 64, (fwd_min_waves<D, NWF>())) fwd_kernel(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, unsigned short* __restrict__ o, Strides os,
    float* __restrict__ lse, int B, int H, int Hk, int Sq, int Sk, float scale, int causal, Sparse sp, int kvlen,
    int qoff) {
  fwd_body<SPARSE, NWF, D, DMA, false>(q, qs, k, ks, v, vs, o, os, lse, B, H, Hk, Sq, Sk, scale, causal, sp, kvlen,
                                       qoff, Band{nullptr, nullptr});
}

// Band mode always stages K/V by LDS-DMA (SXE_FA_FWD_DMA=0 is ignored here: one forward variant per
// head dim and wave count keeps the compile time down, and the DMA form is the faster one).
template <int NWF, int D>
__global__ void __launch_bounds__(NWF * 64, (fwd_min_waves<D, NWF>())) fwd_band_kernel(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, unsigned short* __restrict__ o, Strides os,
    float* __restrict__ lse, int B, int H, int Hk, int S, float scale, Band bd) {
  fwd_body<false, NWF, D, true, true>(q, qs, k, ks, v, vs, o, os, lse, B, H, Hk, S, S, scale, 1,
                                      Sparse{nullptr, 0, 0}, S, 0, bd);
}

// Ragged forward (see Varlen): grid = table entries * H, head fastest, so the query heads of one GQA
// group read the same K/V tiles at about the same time. One variant per head dim -- 4 waves, LDS-DMA,
// band walk (no window = a window of 2^30) -- for the compile-time reason given at fwd_band_kernel.
template <int D>
__global__ void __launch_bounds__(NW * 64, (fwd_min_waves<D, NW>())) fwd_varlen_kernel(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, unsigned short* __restrict__ o, Strides os, int H, int Hk,
    float scale, Varlen vl) {
  fwd_body<false, NW, D, true, true, true>(q, qs, k, ks, v, vs, o, os, nullptr, 1, H, Hk, 0, 0, scale, 1,
                                           Sparse{nullptr, 0, 0}, 0, 0, Band{nullptr, nullptr}, vl);
}

// =============================================================================================
// Backward pre-pass, per (batch, head, query) row: -delta = -sum_d dO * O and lse * log2(e) (fp32),
// D/8 threads per row. (Computing delta inside the dQ kernel instead -- it holds the dO rows --
// measured neutral: the dQ prologue's extra O load cost what the launch saved.)
// =============================================================================================
template <int D>
__global__ void __launch_bounds__(256) delta_kernel(const unsigned short* __restrict__ dout, Strides ds,
                                                    const unsigned short* __restrict__ o, Strides os,
                                                    const float* __restrict__ lse, float* __restrict__ ndelta,
                                                    float* __restrict__ lse2, int B, int H, int S) {
  constexpr int TPR = D / 8, RPB = 256 / TPR;
  const int64_t row = (int64_t)blockIdx.x * RPB + (threadIdx.x / TPR);
  const int part = threadIdx.x % TPR;
  if (row >= (int64_t)B * H * S) return;
  const int s = (int)(row % S);
  const int64_t bh = row / S;
  const int hh = (int)(bh % H), b = (int)(bh / H);
  float x[8], y[8];
  load8<DT::BF16>(dout + b * ds.b + hh * ds.h + (int64_t)s * ds.s + part * 8, x);
  load8<DT::BF16>(o + b * os.b + hh * os.h + (int64_t)s * os.s + part * 8, y);
  float acc = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc += x[e] * y[e];
#pragma unroll
  for (int off = TPR / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, TPR);
  if (part == 0) {
    ndelta[row] = -acc;
    lse2[row] = lse[row] * LOG2E;
  }
}

template <int D>
constexpr int bwd_min_waves() { return D >= 256 ? 1 : 2; }

// =============================================================================================
// dQ: forward-shaped. Per wave 32 queries; per K/V tile recompute S^T, P^T, dP^T = V dO^T,
// dS^T = P^T (dP^T - delta), dQ^T += K^T dS^T.
// =============================================================================================
template <bool MASK, int D, bool BAND = false>
__device__ __forceinline__ void dq_tile(const LaneOffs<D>& lo, const char* kt, const char* vt, const bf16x8 (&qf)[D / 16],
                                        const bf16x8 (&df)[D / 16], f32x16 (&dqacc)[D / 32], float c, float lse2,
                                        float ndlt, int kbase, int qpos, int r, int h, int lane, bool diag, bool tail,
                                        int kvlen, const uint8_t* lay_row, int blk, bool band = false,
                                        int kl = 0) {
  int dd = kbase + 4 * h - qpos - r, dl = kbase + 4 * h - kvlen;  // see fwd_tile
  if (MASK) asm volatile("" : "+v"(dd), "+v"(dl));
  int db = kbase + 4 * h - kl;  // band: key - klo, see fwd_tile
  if (BAND) asm volatile("" : "+v"(db));
  const bool skip1 = MASK && diag && !tail && lay_row == nullptr && !(BAND && band) &&
                     kbase + 32 > qpos + QW - 1;  // see fwd_tile
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j == 1 && skip1) break;
    f32x16 s = zero16(), dp = zero16();
#pragma unroll
    for (int t2 = 0; t2 < D / 16; ++t2) {
      s = mfma(lds_row_at(kt + 32 * j * 2 * D, lo.row[t2]), qf[t2], s);
      dp = mfma(lds_row_at(vt + 32 * j * 2 * D, lo.row[t2]), df[t2], dp);
    }
    bool b0 = true, b1 = true;
    if (MASK && lay_row) {
      b0 = lay_row[(kbase + 32 * j) / blk] != 0;
      b1 = lay_row[(kbase + 32 * j + 16) / blk] != 0;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float p = fast_exp2(__builtin_fmaf(s[i], c, -lse2));
      if (MASK) {
        if (diag && dd + 32 * j + acc_row(i, 0) > 0) p = 0.f;
        if (tail && dl + 32 * j + acc_row(i, 0) >= 0) p = 0.f;
        if (!(i < 8 ? b0 : b1)) p = 0.f;
        if (BAND && band && db + 32 * j + acc_row(i, 0) < 0) p = 0.f;
      }
      s[i] = p * (dp[i] + ndlt);  // dS^T (ndlt = -delta)
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const bf16x8 db = acc_to_b(s, s2);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
        dqacc[dt] = mfma(lds_tr_at(kt + (32 * j + 16 * s2) * 2 * D, lo.tr[dt]), db, dqacc[dt]);
    }
  }
}

// NWF waves per workgroup, 32 queries each: 8 (256 queries) shares every staged K/V tile among twice
// the queries of 4 -- half the L2-to-LDS tile traffic per query, at one workgroup per CU
// (SXE_FA_DQ_WAVES, read per call; Sq a multiple of 256, head dims 64 / 128)
// (body shared with dq_band_kernel: BAND walks and masks the tiles as the forward does)
template <bool SPARSE, int D, int NWF, bool BAND>
__device__ __forceinline__ void dq_body(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, const unsigned short* __restrict__ dout, Strides dos,
    const float* __restrict__ lse, const float* __restrict__ ndelta, unsigned short* __restrict__ dq, Strides dqs,
    int B, int H, int Hk, int Sq, int Sk, float scale, int causal, Sparse sp, int kvlen, int qoff, Band bd) {
  constexpr int ROWB = 2 * D;
  constexpr int BUF = 2 * KT * ROWB;
  int* tlist = reinterpret_cast<int*>(smem + 4 * KT * ROWB) + 1;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
  constexpr int QBF = NWF * QW;
  const int nqb = Sq / QBF;
  int bh, qb;
  map_block(nqb, B * H, causal != 0, bh, qb);
  const int b = bh / H, head = bh - b * H;
  const int kh = head / (H / Hk);
  const int q0 = qb * QBF + w * QW;
  const int qpos = q0 + qoff;
  const unsigned short* qp = q + b * qs.b + head * qs.h;
  const unsigned short* dop = dout + b * dos.b + head * dos.h;
  const unsigned short* kp = k + b * ks.b + kh * ks.h;
  const unsigned short* vp = v + b * vs.b + kh * vs.h;
  const float c = scale * LOG2E;
  const int64_t lrow = ((int64_t)b * H + head) * Sq + q0 + r;
  const int kend = causal ? min(Sk, (qb + 1) * QBF + qoff) : Sk;
  const int nkt = (max(kend, 0) + KT - 1) / KT;
  const int tfirst = BAND ? band_klo(bd, b, Sq, qb * QBF) / KT : 0;  // band: see fwd_body
  const int kl = BAND ? band_klo(bd, b, Sq, q0 + r) : 0;
  const int kl_lo = BAND ? __builtin_amdgcn_readfirstlane(kl) : 0;
  const int kl_hi = BAND ? __builtin_amdgcn_readlane(kl, QW - 1) : 0;
  const int ntiles = SPARSE ? build_tile_list(sp, head, 0, nkt, KT, qb * QBF, qb * QBF + QBF, true, tlist)
                            : (BAND ? nkt - tfirst : nkt);
  auto tile_at = [&](int i) { return SPARSE ? tlist[i] : (BAND ? tfirst + i : i); };
  const uint8_t* lay_row = SPARSE ? sp.layout + ((int64_t)head * sp.nb + (q0 + r) / sp.blk) * sp.nb : nullptr;
  if (ntiles > 0) {
    tile_glds<KT, D, NWF>(kp, ks.s, tile_at(0) * KT, smem);
    tile_glds<KT, D, NWF>(vp, vs.s, tile_at(0) * KT, smem + KT * ROWB);
  }

  const float lse2 = lse[lrow] * LOG2E;
  bf16x8 qf[D / 16], df[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t) {
    qf[t] = *reinterpret_cast<const bf16x8*>(qp + (int64_t)(q0 + r) * qs.s + 16 * t + 8 * h);
    df[t] = *reinterpret_cast<const bf16x8*>(dop + (int64_t)(q0 + r) * dos.s + 16 * t + 8 * h);
  }
  const float ndlt = ndelta[lrow];
  f32x16 dqacc[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t) dqacc[t] = zero16();
  vm_wait_all();
  // pin the Q / dO fragments and row constants as loaded before the loop (see dkdv_kernel)
#pragma unroll
  for (int t = 0; t < D / 16; ++t) asm volatile("" ::"v"(qf[t]), "v"(df[t]));
  asm volatile("" ::"v"(lse2), "v"(ndlt));
  __syncthreads();
  LaneOffs<D> lo;
  lo.init(lane);
  // unrolled by two: compile-time ring slot, hoisted LDS offsets (see fwd_kernel)
  auto step = [&](const int t, auto slot) {
    constexpr int CUR = decltype(slot)::value;
    if (t + 1 < ntiles) {
      tile_glds<KT, D, NWF>(kp, ks.s, tile_at(t + 1) * KT, smem + (CUR ^ 1) * BUF);
      tile_glds<KT, D, NWF>(vp, vs.s, tile_at(t + 1) * KT, smem + (CUR ^ 1) * BUF + KT * ROWB);
    }
    const int kbase = tile_at(t) * KT;
    const bool active = (!causal || kbase <= qpos + QW - 1) && !(BAND && kbase + KT - 1 < kl_lo);
    if (active) {
      const char* kt = smem + CUR * BUF;
      const char* vt = smem + CUR * BUF + KT * ROWB;
      const bool diag = causal && (kbase + KT - 1 > qpos);
      const bool tail = kbase + KT > kvlen;
      const bool band = BAND && kbase < kl_hi;
      if (SPARSE || diag || tail || band)
        dq_tile<true, D, BAND>(lo, kt, vt, qf, df, dqacc, c, lse2, ndlt, kbase, qpos, r, h, lane, diag, tail, kvlen,
                               lay_row, SPARSE ? sp.blk : 1, band, kl);
      else
        dq_tile<false, D>(lo, kt, vt, qf, df, dqacc, c, lse2, ndlt, kbase, qpos, r, h, lane, false, false, kvlen,
                          nullptr, 1);
    }
    vm_wait_all();
    __syncthreads();
  };
  for (int t = 0; t < ntiles; t += 2) {
    step(t, std::integral_constant<int, 0>{});
    if (t + 1 < ntiles) step(t + 1, std::integral_constant<int, 1>{});
  }
  unsigned short* op = dq + b * dqs.b + head * dqs.h + (int64_t)(q0 + r) * dqs.s;
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      u16x4 pk;
#pragma unroll
      for (int e = 0; e < 4; ++e) pk[e] = f32_to_bf16(dqacc[dt][4 * rg + e] * scale);
      *reinterpret_cast<u16x4*>(op + 32 * dt + 8 * rg + 4 * h) = pk;
    }
}

template <bool SPARSE, int D, int NWF = 4>
__global__ void __launch_bounds__(NWF * 64, (NWF == 8 ? 1 : bwd_min_waves<D>())) dq_kernel(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, const unsigned short* __restrict__ dout, Strides dos,
    const float* __restrict__ lse, const float* __restrict__ ndelta, unsigned short* __restrict__ dq, Strides dqs,
    int B, int H, int Hk, int Sq, int Sk, float scale, int causal, Sparse sp, int kvlen, int qoff) {
  dq_body<SPARSE, D, NWF, false>(q, qs, k, ks, v, vs, dout, dos, lse, ndelta, dq, dqs, B, H, Hk, Sq, Sk, scale,
                                 causal, sp, kvlen, qoff, Band{nullptr, nullptr});
}

template <int D, int NWF = 4>
__global__ void __launch_bounds__(NWF * 64, (NWF == 8 ? 1 : bwd_min_waves<D>())) dq_band_kernel(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, const unsigned short* __restrict__ dout, Strides dos,
    const float* __restrict__ lse, const float* __restrict__ ndelta, unsigned short* __restrict__ dq, Strides dqs,
    int B, int H, int Hk, int S, float scale, Band bd) {
  dq_body<false, D, NWF, true>(q, qs, k, ks, v, vs, dout, dos, lse, ndelta, dq, dqs, B, H, Hk, S, S, scale, 1,
                               Sparse{nullptr, 0, 0}, S, 0, bd);
}

// =============================================================================================
// dK, dV: per wave 32 keys held on the lanes; sweep every query head of the GQA group and every
// 32-query tile at or after the keys (causal). Q/dO tiles + LSE/delta arrive by LDS-DMA into a
// 2-slot ring; the workgroup's V block (128 keys) sits in LDS for the whole kernel (V fragments in
// registers too would exceed the VGPR budget and spill); K fragments, dK^T and dV^T live in
// registers.
// =============================================================================================
constexpr int QT = 32;  // queries per tile in the dK/dV sweep
template <int D, int KB = QB> struct KVL {
  static constexpr int TILE = QT * 2 * D;              // one Q (or dO) tile
  static constexpr int SLOT = 2 * TILE + 2 * QT * 4;   // Q, dO, lse[32], delta[32]
  static constexpr int VBLK = KB * 2 * D;              // the V block of KB keys
};

// PART: 3 = dK and dV in one sweep; 1 = dV only; 2 = dK only (head dim 256: the two 128-register
// accumulators of one sweep would spill, so two sweeps each recompute S = Q K^T)
// BAND (band kernels only): `band` says the tile holds queries above the qhi of some key of the
// wave; `qh` is this lane's (clamped) qhi.
template <bool MASK, int D, int PART, bool BAND = false>
__device__ __forceinline__ void dkdv_tile(const LaneOffs<D>& lo, const char* slot, const char* vblk,
                                          const bf16x8 (&kf)[D / 16],
                                          f32x16 (&dka)[D / 32], f32x16 (&dva)[D / 32], float c, int qt0, int k0,
                                          int w, int r, int h, int lane, bool diag, const Sparse& sp, int hq0,
                                          int kbl, int qoff, bool band = false, int qh = 0) {
  const char* qt = slot;
  const char* dt_ = slot + KVL<D>::TILE;
  const float* l2 = reinterpret_cast<const float*>(slot + 2 * KVL<D>::TILE);
  const float* dl = l2 + QT;
  f32x16 s = zero16(), dp = zero16();
#pragma unroll
  for (int t2 = 0; t2 < D / 16; ++t2) {
    s = mfma(lds_row_at(qt, lo.row[t2]), kf[t2], s);  // S  [query][key]
    if constexpr ((PART & 2) != 0)
      dp = mfma(lds_row_at(dt_, lo.row[t2]), lds_row_at(vblk + w * QW * 2 * D, lo.row[t2]), dp);  // dP
  }
  bool b0 = true, b1 = true;  // layout bits of query rows qt0+[0,16) and qt0+[16,32) vs this key
  if (MASK && sp.layout) {
    b0 = sp.layout[((int64_t)hq0 * sp.nb + qt0 / sp.blk) * sp.nb + kbl] != 0;
    b1 = sp.layout[((int64_t)hq0 * sp.nb + (qt0 + 16) / sp.blk) * sp.nb + kbl] != 0;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) s[i] = fast_exp2(__builtin_fmaf(s[i], c, -l2[acc_row(i, h)]));  // P; l2 = lse log2(e)
  // masks under wave-uniform (scalar) branches: interior tiles -- most of them -- run no per-score
  // compares / selects (`diag` and the layout pointer are SGPR values; see the readfirstlane of w)
  if (MASK && diag) {
    int dd = k0 + r - 4 * h - qt0 - qoff;  // masked iff key > query + qoff, i.e. dd > row(i, 0)
    asm volatile("" : "+v"(dd));            // keep the per-row compares against constants (see fwd_tile)
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (dd > acc_row(i, 0)) s[i] = 0.f;
  }
  if (MASK && sp.layout) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (!(acc_row(i, h) < 16 ? b0 : b1)) s[i] = 0.f;
  }
  if (BAND && band) {
    int db = qh - qt0 - 4 * h;  // masked iff query > qhi of this lane's key, i.e. row(i, 0) > db
    asm volatile("" : "+v"(db));
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (acc_row(i, 0) > db) s[i] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) dp[i] = s[i] * (dp[i] + dl[acc_row(i, h)]);  // dS = P (dP - delta); dl = -delta
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    const bf16x8 pb = acc_to_b(s, s2);
    const bf16x8 db = acc_to_b(dp, s2);
#pragma unroll
    for (int t = 0; t < D / 32; ++t) {
      if constexpr ((PART & 1) != 0) dva[t] = mfma(lds_tr_at(dt_ + 16 * s2 * 2 * D, lo.tr[t]), pb, dva[t]);  // dV^T
      if constexpr ((PART & 2) != 0) dka[t] = mfma(lds_tr_at(qt + 16 * s2 * 2 * D, lo.tr[t]), db, dka[t]);   // dK^T
    }
  }
}

// SPLIT (GQA): one workgroup per (batch, group of `hpw` QUERY heads, key block) instead of per KV
// head: under a causal mask the KV-head form gives key block 0 G x (Sq/128) query tiles while the
// mean block has half of that, and with B*Hk*Sk/128 ~ 2 workgroups per CU the whole launch waits for
// block 0 (measured 650 us at B4 S2048 H32/8). Splitting the G query heads into G/hpw groups cuts the
// longest job by G/hpw; the per-group fp32 dK/dV partials [B, Sk, H/hpw, D] are summed by
// dkdv_reduce_kernel (hpw = 2 halves that partial traffic against hpw = 1).
// NWK waves per workgroup, 32 keys each: 8 (256 keys, head dim 128; SXE_FA_DKDV_WAVES, read per
// call) shares every staged Q / dO tile among twice the keys of 4 -- half the L2-to-LDS traffic per
// key, at one workgroup per CU
// The body is shared with dkdv_band_kernel (BAND: the query sweep of each head ends at the qhi of the
// workgroup's last key, rounded up to the query tile; a wave skips the tiles wholly above its last
// key's qhi, and tiles that the qhi of its first key cuts get one more mask).
template <bool SPLIT, int D, int PART, int NWK, bool BAND>
__device__ __forceinline__ void dkdv_body(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, const unsigned short* __restrict__ dout, Strides dos,
    const float* __restrict__ lse, const float* __restrict__ delta, unsigned short* __restrict__ dk, Strides dks,
    unsigned short* __restrict__ dv, Strides dvs, float* __restrict__ pk, float* __restrict__ pv, int B, int H,
    int Hk, int Sq, int Sk, float scale, int causal, Sparse sp, int qoff, int hpw, Band bd) {
  constexpr int KB = NWK * QW;  // keys per workgroup
  using G_ = KVL<D, KB>;
  char* vblk = smem;
  char* ring = smem + G_::VBLK;
  int* tlist = reinterpret_cast<int*>(ring + 2 * G_::SLOT) + 1;
  // w via readfirstlane: the compiler then knows it (and k0, the causal `diag` test) is wave-uniform,
  // so the diagonal mask is a scalar branch rather than per-lane selects on every tile
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 31,
            h = lane >> 5;
  const int nkb = Sk / KB;
  int bh, kb;
  const int G = SPLIT ? hpw : H / Hk;  // query heads swept by this workgroup (sparse: 1)
  const int HB = H / G;                 // workgroups along the head axis
  map_block(nkb, B * HB, false, bh, kb);  // key block 0 is the heaviest under causality
  const int b = bh / HB, hsel = bh - b * HB;
  const int hq0 = hsel * G;             // first query head swept by this workgroup
  const int kh = hq0 / (H / Hk);
  const int k0 = kb * KB + w * QW;  // this wave's first key
  const unsigned short* kp = k + b * ks.b + kh * ks.h;
  const unsigned short* vp = v + b * vs.b + kh * vs.h;
  const float c = scale * LOG2E;
  // causal: the first query that sees key block kb (query i sees keys <= i + qoff)
  const int qstart = causal ? min(Sq, max(0, kb * KB - qoff) / QT * QT) : 0;
  // end of the query sweep (band: past the last query that sees the workgroup's last key; <= Sq, a
  // multiple of QT), this lane's qhi and the qhi of the wave's first / last key
  const int qend = BAND ? (band_qhi(bd, b, Sq, kb * KB + KB - 1) / QT + 1) * QT : Sq;
  const int qh = BAND ? band_qhi(bd, b, Sq, k0 + r) : 0;
  const int qh_lo = BAND ? __builtin_amdgcn_readfirstlane(qh) : 0;
  const int qh_hi = BAND ? __builtin_amdgcn_readlane(qh, QW - 1) : 0;
  const int ntq = (qend - qstart) / QT;
  // sparse: SPLIT mode (G == 1), list of the active 32-query tiles of this key block
  const int total = sp.layout ? build_tile_list(sp, hq0, qstart / QT, Sq / QT, QT, kb * KB, kb * KB + KB, false, tlist)
                              : ntq * G;
  const int kbl = sp.layout ? (k0 + r) / sp.blk : 0;
  // dense tile order: the query tiles qstart .. Sq of head hq0, then of hq0 + 1, ... -- walked by
  // incremented iterators (a runtime `it % ntq` / `it / ntq` per tile was a scalar division
  // sequence, a third of the kernel's instructions as SALU)
  int is_h = hq0, is_q = qstart;  // next tile to issue
  int c_q = qstart;               // tile being computed
  auto issue = [&](int it, char* slot) {
    const int hq = sp.layout ? hq0 : is_h;
    const int qt0 = sp.layout ? tlist[it] * QT : is_q;
    if (!sp.layout) {
      is_q += QT;
      if (is_q >= qend) {
        is_q = qstart;
        ++is_h;
      }
    }
    tile_glds<QT, D, NWK>(q + b * qs.b + hq * qs.h, qs.s, qt0, slot);
    tile_glds<QT, D, NWK>(dout + b * dos.b + hq * dos.h, dos.s, qt0, slot + G_::TILE);
    if (w == 0) {  // 64 lanes x 4 B: lse[32] then delta[32]
      const int64_t lr = ((int64_t)b * H + hq) * Sq + qt0 + (lane & 31);
      glds4_m0(lane < 32 ? (const void*)(lse + lr) : (const void*)(delta + lr), lds_addr(slot + 2 * G_::TILE));
    }
  };
  if constexpr ((PART & 2) != 0) tile_glds<KB, D, NWK>(vp, vs.s, kb * KB, vblk);
  if (total > 0) issue(0, ring);
  bf16x8 kf[D / 16];
#pragma unroll
  for (int t = 0; t < D / 16; ++t)
    kf[t] = *reinterpret_cast<const bf16x8*>(kp + (int64_t)(k0 + r) * ks.s + 16 * t + 8 * h);
  f32x16 dka[D / 32], dva[D / 32];
#pragma unroll
  for (int t = 0; t < D / 32; ++t) {
    dka[t] = zero16();
    dva[t] = zero16();
  }
  vm_wait_all();
  // pin the K fragments as loaded before the loop: left to itself the compiler sinks their loads
  // below the barrier, and its counted waits for them inside the loop then also wait on the
  // hand-tracked LDS-DMA of the next tile
#pragma unroll
  for (int t = 0; t < D / 16; ++t) asm volatile("" ::"v"(kf[t]));
  __syncthreads();
  LaneOffs<D> lo;
  lo.init(lane);
  // unrolled by two: compile-time ring slot, hoisted LDS offsets (see fwd_kernel)
  auto step = [&](const int it, auto slotc) {
    constexpr int CUR = decltype(slotc)::value;
    const int qt0 = sp.layout ? tlist[it] * QT : c_q;
    c_q = c_q + QT >= qend ? qstart : c_q + QT;
    const bool active = (!causal || (qt0 + QT - 1 + qoff >= k0)) && !(BAND && qt0 > qh_hi);
    const bool diag = causal && (qt0 + qoff < k0 + QW);
    const bool band = BAND && qt0 + QT - 1 > qh_lo;
    if (it + 1 < total) issue(it + 1, ring + (CUR ^ 1) * G_::SLOT);
    if (active)
      dkdv_tile<true, D, PART, BAND>(lo, ring + CUR * G_::SLOT, vblk, kf, dka, dva, c, qt0, k0, w, r, h, lane, diag,
                                     sp, hq0, kbl, qoff, band, qh);
    vm_wait_all();
    __syncthreads();
  };
  for (int it = 0; it < total; it += 2) {
    step(it, std::integral_constant<int, 0>{});
    if (it + 1 < total) step(it + 1, std::integral_constant<int, 1>{});
  }
  if (SPLIT && pk != nullptr) {  // fp32 partials, layout [B, Sk, H / hpw, D] contiguous
    float* kp32 = pk + (((int64_t)b * Sk + k0 + r) * HB + hsel) * D;
    float* vp32 = pv + (((int64_t)b * Sk + k0 + r) * HB + hsel) * D;
#pragma unroll
    for (int t = 0; t < D / 32; ++t)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        f32x4 a, cc;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = dka[t][4 * rg + e] * scale;
          cc[e] = dva[t][4 * rg + e];
        }
        if constexpr ((PART & 2) != 0) *reinterpret_cast<f32x4*>(kp32 + 32 * t + 8 * rg + 4 * h) = a;
        if constexpr ((PART & 1) != 0) *reinterpret_cast<f32x4*>(vp32 + 32 * t + 8 * rg + 4 * h) = cc;
      }
    return;
  }
  unsigned short* kop = dk + b * dks.b + kh * dks.h + (int64_t)(k0 + r) * dks.s;
  unsigned short* vop = dv + b * dvs.b + kh * dvs.h + (int64_t)(k0 + r) * dvs.s;
#pragma unroll
  for (int t = 0; t < D / 32; ++t)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      u16x4 pk4, pv4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pk4[e] = f32_to_bf16(dka[t][4 * rg + e] * scale);
        pv4[e] = f32_to_bf16(dva[t][4 * rg + e]);
      }
      if constexpr ((PART & 2) != 0) *reinterpret_cast<u16x4*>(kop + 32 * t + 8 * rg + 4 * h) = pk4;
      if constexpr ((PART & 1) != 0) *reinterpret_cast<u16x4*>(vop + 32 * t + 8 * rg + 4 * h) = pv4;
    }
}

template <bool SPLIT, int D, int PART = 3, int NWK = 4>
__global__ void __launch_bounds__(NWK * 64, (NWK == 8 ? 1 : bwd_min_waves<D>())) dkdv_kernel(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, const unsigned short* __restrict__ dout, Strides dos,
    const float* __restrict__ lse, const float* __restrict__ delta, unsigned short* __restrict__ dk, Strides dks,
    unsigned short* __restrict__ dv, Strides dvs, float* __restrict__ pk, float* __restrict__ pv, int B, int H,
    int Hk, int Sq, int Sk, float scale, int causal, Sparse sp, int qoff, int hpw) {
  dkdv_body<SPLIT, D, PART, NWK, false>(q, qs, k, ks, v, vs, dout, dos, lse, delta, dk, dks, dv, dvs, pk, pv, B, H,
                                        Hk, Sq, Sk, scale, causal, sp, qoff, hpw, Band{nullptr, nullptr});
}

template <bool SPLIT, int D, int PART = 3, int NWK = 4>
__global__ void __launch_bounds__(NWK * 64, (NWK == 8 ? 1 : bwd_min_waves<D>())) dkdv_band_kernel(
    const unsigned short* __restrict__ q, Strides qs, const unsigned short* __restrict__ k, Strides ks,
    const unsigned short* __restrict__ v, Strides vs, const unsigned short* __restrict__ dout, Strides dos,
    const float* __restrict__ lse, const float* __restrict__ delta, unsigned short* __restrict__ dk, Strides dks,
    unsigned short* __restrict__ dv, Strides dvs, float* __restrict__ pk, float* __restrict__ pv, int B, int H,
    int Hk, int S, float scale, int hpw, Band bd) {
  dkdv_body<SPLIT, D, PART, NWK, true>(q, qs, k, ks, v, vs, dout, dos, lse, delta, dk, dks, dv, dvs, pk, pv, B, H,
                                       Hk, S, S, scale, 1, Sparse{nullptr, 0, 0}, 0, hpw, bd);
}


// dk[b, s, kh, :] = sum_g pk[b, s, kh*G + g, :] (dv likewise) over the G = H / Hk partial groups of
// each KV head (H here = the partial count, query heads / hpw); one thread per 8 output elements.
template <int D>
__global__ void __launch_bounds__(256) dkdv_reduce_kernel(const float* __restrict__ pk, const float* __restrict__ pv,
                                                          unsigned short* __restrict__ dk, Strides dks,
                                                          unsigned short* __restrict__ dv, Strides dvs, int B, int S,
                                                          int H, int Hk) {
  const int G = H / Hk;
  const int64_t n8 = (int64_t)B * S * Hk * (D / 8);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % (D / 8)) * 8;
    const int64_t rest = i / (D / 8);
    const int kh = (int)(rest % Hk);
    const int64_t bs = rest / Hk;  // b * S + s
    const int b = (int)(bs / S), s_ = (int)(bs - (int64_t)b * S);
    float ak[8] = {0, 0, 0, 0, 0, 0, 0, 0}, av[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int g = 0; g < G; ++g) {
      const int64_t off = (bs * H + kh * G + g) * D + c;
      float x[8], y[8];
      load8<DT::F32>(pk + off, x);
      load8<DT::F32>(pv + off, y);
#pragma unroll
      for (int e = 0; e < 8; ++e) { ak[e] += x[e]; av[e] += y[e]; }
    }
    store8<DT::BF16>(dk + b * dks.b + (int64_t)s_ * dks.s + kh * dks.h + c, ak);
    store8<DT::BF16>(dv + b * dvs.b + (int64_t)s_ * dvs.s + kh * dvs.h + c, av);
  }
}

}  // namespace fa

// ---------------------------------------------------------------------------------------------
static fa::Strides strides_of(const at::Tensor& t) {
  return fa::Strides{t.stride(0), t.stride(1), t.stride(2)};
}
static unsigned short* u16(const at::Tensor& t) { return reinterpret_cast<unsigned short*>(t.data_ptr()); }

// What the kernels' 16-byte loads and stores need of each of `ts` ([.., D], at least 2-D): bf16,
// unit stride on D, every other stride and the base address a multiple of 16 bytes
static void check_bf16_rows(std::initializer_list<const at::Tensor*> ts, const char* op) {
  for (const at::Tensor* t : ts) {
    bool ok = t->scalar_type() == at::kBFloat16 && t->stride(-1) == 1 &&
              (reinterpret_cast<uintptr_t>(t->data_ptr()) & 15) == 0;
    for (int64_t i = 0; i + 1 < t->dim(); ++i) ok = ok && t->stride(i) % 8 == 0;
    SXE_CHECK(ok, op, ": bf16 with unit stride on D and 16-byte aligned rows required");
  }
}

// q: [B, Sq, Hq, D]; k, v: [B, Sk, Hk, D]; D in {64, 128, 256}; Sq, Sk multiples of 128
static void check_qkv(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v) {
  SXE_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "flash_attn: tensors must be [B, S, H, D]");
  check_bf16_rows({&q, &k, &v}, "flash_attn");
  const int64_t D = q.size(3);
  SXE_CHECK(D == 64 || D == 128 || D == 256, "flash_attn: head dim must be 64, 128 or 256");
  SXE_CHECK(k.size(3) == D && v.size(3) == D, "flash_attn: q/k/v head dims differ");
  SXE_CHECK(k.sizes() == v.sizes() && q.size(0) == k.size(0), "flash_attn: q/k/v shapes");
  SXE_CHECK(q.size(2) % k.size(2) == 0, "flash_attn: Hq must be a multiple of Hkv");
  SXE_CHECK(q.size(1) % fa::QB == 0 && k.size(1) % fa::QB == 0, "flash_attn: seq lengths must be multiples of 128");
}

static fa::Sparse sparse_of(const c10::optional<at::Tensor>& layout, int64_t block, const at::Tensor& q) {
  if (!layout.has_value() || !layout->defined()) return fa::Sparse{nullptr, 0, 0};
  const at::Tensor& L = *layout;
  const int S = q.size(1), H = q.size(2);
  SXE_CHECK(L.is_cuda() && L.scalar_type() == at::kByte && L.is_contiguous() && L.dim() == 3, "layout: uint8 [H, nb, nb]");
  SXE_CHECK(block >= 16 && block % 16 == 0 && S % block == 0, "layout block must be a multiple of 16 dividing seq_len");
  SXE_CHECK(L.size(0) == H && L.size(1) == S / block && L.size(2) == S / block, "layout shape must be [H, S/block, S/block]");
  SXE_CHECK(S / fa::KT <= 1024, "sparse attention: seq_len <= 65536");
  return fa::Sparse{L.data_ptr<uint8_t>(), (int)block, (int)(S / block)};
}

// klo / qhi of band mode: int32 [B, S] contiguous on q's device (values are clamped by the kernels)
static fa::Band band_of(const at::Tensor& klo, const at::Tensor& qhi, const at::Tensor& q, const at::Tensor& k) {
  SXE_CHECK(q.dim() == 4 && k.dim() == 4 && q.size(1) == k.size(1), "flash_attn band: needs Sq == Sk");
  for (const at::Tensor* t : {&klo, &qhi})
    SXE_CHECK(t->is_cuda() && t->device() == q.device() && t->scalar_type() == at::kInt && t->is_contiguous() &&
                  t->dim() == 2 && t->size(0) == q.size(0) && t->size(1) == q.size(1),
              "flash_attn band: klo / qhi must be contiguous int32 [B, S] on the device of q");
  return fa::Band{klo.data_ptr<int>(), qhi.data_ptr<int>()};
}

constexpr size_t kListBytes = (1 + 2048) * sizeof(int) + 16;  // tile list + scratch flags (sparse mode)

// Kernel-variant knob, read on every call (not cached at static init) so a test or an A/B run can
// switch variants inside one process: SXE_FA_FWD_WAVES=4 forces the 4-wave forward.
static int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return (e != nullptr && *e != 0) ? std::atoi(e) : dflt;
}

// Dynamic LDS of the forward, dQ and varlen kernels: the K/V tile ring (sparse mode adds kListBytes)
template <int D> constexpr size_t kRingBytes = 4 * fa::KT * 2 * D;

// Compile-time tags that carry a kernel or a variant parameter through the generic launch lambdas
template <auto Kernel> using kern_t = std::integral_constant<decltype(Kernel), Kernel>;
template <int N> using int_t = std::integral_constant<int, N>;

// Every flash kernel starts here: opt `Kernel` into more than 64 KiB of dynamic LDS (the first call
// per instantiation), launch it on the current stream, check.
template <auto Kernel, typename... Args>
static void launch(int grid, int waves, size_t lds, Args... args) {
  allow_max_dynamic_lds<Kernel>();
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(waves * 64), lds, cur_stream(), args...);
  SXE_LAUNCH_CHECK();
}

// The mask of one call. kvlen: valid keys (the rest of the padded key axis is masked); qoff: causal
// offset (query i sees keys <= i + qoff), default Sk - Sq (bottom-right aligned); sp.layout / bd.klo
// are null unless the call is block-sparse / banded.
struct Mask {
  bool causal;
  int kvlen, qoff;
  fa::Sparse sp;
  fa::Band bd;
};
constexpr fa::Sparse kNoSparse{nullptr, 0, 0};
constexpr fa::Band kNoBand{nullptr, nullptr};

static Mask mask_of(const at::Tensor& q, const at::Tensor& k, bool causal, fa::Sparse sp, int64_t kv_len,
                    int64_t causal_offset, fa::Band bd) {
  const int Sq = q.size(1), Sk = k.size(1);
  const int kvlen = kv_len < 0 ? Sk : (int)kv_len;
  SXE_CHECK(kvlen >= 1 && kvlen <= Sk, "flash_attn: kv_len must be in [1, Sk]");
  const int qoff = causal_offset == INT64_MIN ? Sk - Sq : (int)causal_offset;
  SXE_CHECK(!sp.layout || (Sq == Sk && qoff == 0), "block-sparse attention needs Sq == Sk");
  SXE_CHECK(!bd.klo || (causal && Sq == Sk && qoff == 0 && kvlen == Sk && !sp.layout),
            "flash_attn band: needs causal, Sq == Sk, causal offset 0, no kv_len and no sparse layout");
  return Mask{causal, kvlen, qoff, sp, bd};
}

template <int D>
static std::vector<at::Tensor> fwd_impl_d(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, double scale,
                                          const Mask& m) {
  static_assert(kRingBytes<D> + kListBytes <= kMaxDynamicLds, "forward LDS exceeds the opt-in limit");
  const int B = q.size(0), Sq = q.size(1), H = q.size(2), Sk = k.size(1), Hk = k.size(2);
  auto o = at::empty({B, Sq, H, D}, q.options());
  auto lse = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  const size_t lds = kRingBytes<D> + (m.sp.layout ? kListBytes : 0);
  const int grid = (Sq / fa::QB) * B * H;
  // one variant: NWF waves per workgroup, K/V staged by LDS-DMA or through registers
  auto run = [&](auto nwf, auto dma) {
    constexpr int NWF = decltype(nwf)::value;
    constexpr bool DMA = decltype(dma)::value;
    auto go = [&](auto kern, auto... tail) {
      launch<decltype(kern)::value>(NWF == 8 ? grid / 2 : grid, NWF, lds, u16(q), strides_of(q), u16(k), strides_of(k),
                                    u16(v), strides_of(v), u16(o), strides_of(o), lse.data_ptr<float>(), B, H, Hk, Sq,
                                    tail...);
    };
    auto dense = [&](auto kern) { go(kern, Sk, (float)scale, m.causal ? 1 : 0, m.sp, m.kvlen, m.qoff); };
    if (m.bd.klo != nullptr) go(kern_t<fa::fwd_band_kernel<NWF, D>>{}, (float)scale, m.bd);  // always LDS-DMA
    else if (m.sp.layout != nullptr) dense(kern_t<fa::fwd_kernel<true, NWF, D, DMA>>{});
    else dense(kern_t<fa::fwd_kernel<false, NWF, D, DMA>>{});
  };
  if constexpr (D < 256) {
    // 8 waves share each staged K/V tile when the query axis allows. 4-wave workgroups only when
    // forced (SXE_FA_FWD_WAVES=4): 8 waves are equal or faster on every measured shape -- causal
    // equal at head dims 64 / 128, non-causal 3-7 % faster (profiles/r05/attn_fwd_waves_ab.log,
    // attn_fwd_waves_d64_ab.log; one earlier box showed 4 waves 6 % ahead at D64 causal, which a
    // second box did not reproduce)
    const bool wide = Sq % 256 == 0 && env_int("SXE_FA_FWD_WAVES", 8) != 4;
    const bool dma = m.bd.klo != nullptr || env_int("SXE_FA_FWD_DMA", 1) != 0;
    if (wide) dma ? run(int_t<8>{}, std::true_type{}) : run(int_t<8>{}, std::false_type{});
    else dma ? run(int_t<4>{}, std::true_type{}) : run(int_t<4>{}, std::false_type{});
  } else {
    run(int_t<4>{}, std::true_type{});  // head dim 256: 4 waves (register budget), LDS-DMA only
  }
  return {o, lse};
}

static std::vector<at::Tensor> fwd_impl(at::Tensor q, at::Tensor k, at::Tensor v, bool causal, double scale,
                                        fa::Sparse sp, int64_t kv_len = -1, int64_t causal_offset = INT64_MIN,
                                        fa::Band bd = kNoBand) {
  check_qkv(q, k, v);
  const Mask m = mask_of(q, k, causal, sp, kv_len, causal_offset, bd);
  c10::DeviceGuard guard(q.device());
  std::vector<at::Tensor> out;
  dispatch_head_dim(q.size(3), "flash_attn", [&](auto d) { out = fwd_impl_d<decltype(d)::value>(q, k, v, scale, m); });
  return out;
}

template <int D>
static void bwd_impl_d(const at::Tensor& dout, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                       const at::Tensor& o, const at::Tensor& lse, const at::Tensor& dq, const at::Tensor& dk,
                       const at::Tensor& dv, double scale, const Mask& m) {
  using G_ = fa::KVL<D>;
  constexpr int KB8 = D == 128 ? 256 : fa::QB;  // keys per dK/dV workgroup in its widest (8-wave) form
  static_assert(kRingBytes<D> + kListBytes <= kMaxDynamicLds, "dQ LDS exceeds the opt-in limit");
  static_assert(fa::KVL<D, KB8>::VBLK + 2 * G_::SLOT + kListBytes <= kMaxDynamicLds,
                "dK/dV LDS exceeds the opt-in limit");
  const bool causal = m.causal;
  const fa::Sparse sp = m.sp;
  const int B = q.size(0), Sq = q.size(1), H = q.size(2), Sk = k.size(1), Hk = k.size(2);
  auto ndelta = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  auto lse2 = at::empty({B, H, Sq}, q.options().dtype(at::kFloat));
  const int64_t rows = (int64_t)B * H * Sq;
  constexpr int RPB = 256 / (D / 8);
  hipLaunchKernelGGL(fa::delta_kernel<D>, dim3((rows + RPB - 1) / RPB), dim3(256), 0, cur_stream(), u16(dout),
                     strides_of(dout), u16(o), strides_of(o), lse.data_ptr<float>(), ndelta.data_ptr<float>(),
                     lse2.data_ptr<float>(), B, H, Sq);
  SXE_LAUNCH_CHECK();
  const size_t lds_dq = kRingBytes<D> + (sp.layout ? kListBytes : 0);
  auto run_dq = [&](auto nwf) {
    constexpr int NWF = decltype(nwf)::value;
    auto go = [&](auto kern, auto... tail) {
      launch<decltype(kern)::value>((Sq / (NWF * fa::QW)) * B * H, NWF, lds_dq, u16(q), strides_of(q), u16(k),
                                    strides_of(k), u16(v), strides_of(v), u16(dout), strides_of(dout),
                                    lse.data_ptr<float>(), ndelta.data_ptr<float>(), u16(dq), strides_of(dq), B, H, Hk,
                                    Sq, tail...);
    };
    auto dense = [&](auto kern) { go(kern, Sk, (float)scale, causal ? 1 : 0, sp, m.kvlen, m.qoff); };
    if (m.bd.klo != nullptr) go(kern_t<fa::dq_band_kernel<D, NWF>>{}, (float)scale, m.bd);
    else if (sp.layout != nullptr) dense(kern_t<fa::dq_kernel<true, D, NWF>>{});
    else dense(kern_t<fa::dq_kernel<false, D, NWF>>{});
  };
  // 8-wave dQ workgroups from 8k queries on (auto; SXE_FA_DQ_WAVES=4 / 8 forces): 1.5-2 % faster
  // fwd+bwd at S8k / S32k, neutral at 2k (profiles/r05/attn_bwd_waves_ab.log)
  const int dqw = env_int("SXE_FA_DQ_WAVES", 0);
  const bool dq8 = D < 256 && Sq % 256 == 0 && (dqw == 8 || (dqw == 0 && Sq >= 8192));
  if constexpr (D < 256) {
    dq8 ? run_dq(int_t<8>{}) : run_dq(int_t<4>{});
  } else {
    run_dq(int_t<4>{});
  }
  // sparse: always one workgroup per query head (per-head tile lists); with GQA the per-head fp32
  // partials are reduced; causal GQA: split to remove the key-block-0 tail (see dkdv_kernel)
  // query heads per dK/dV workgroup in the split form (a divisor of the GQA group; sparse: 1). Auto
  // (SXE_FA_DKDV_HPW unset / 0): the largest divisor whose heaviest workgroup -- key block 0 sweeps
  // hpw x Sq/32 query tiles under the causal mask -- still fits the mean load of the 2 x CUs
  // workgroup slots (hpw <= B H nkb / (4 CUs)), and at most 2 from 8k keys on, where the partials'
  // traffic no longer matters and the balance does. Measured fwd+bwd (H32/8 D128 causal; 1 / 2 / 4
  // heads per workgroup): B8 S2048 1.88 / 1.76 / 1.69 ms, B4 S2048 0.84 / 0.76 / 0.88, B1 S32k
  // 36.4 / 36.2 / 37.3; B1 S32k H4/1 4.75 / 6.14 / 9.15 (profiles/r05/attn_dkdv_hpw_sweep.log)
  int hpw = sp.layout != nullptr ? 1 : env_int("SXE_FA_DKDV_HPW", 0);
  if (hpw == 0) {
    int64_t cap = (int64_t)B * H * (Sk / fa::QB) / (4 * kNumCUs);
    if (Sk >= 8192 && cap > 2) cap = 2;
    for (int d = H / Hk; d >= 1; --d)
      if ((H / Hk) % d == 0 && d <= cap) {
        hpw = d;
        break;
      }
  }
  if (hpw < 1 || (H / Hk) % hpw != 0) hpw = 1;
  const bool split = sp.layout != nullptr || (causal && H / Hk > hpw);
  const bool partials = split && H / hpw > Hk;
  const int np = H / hpw;  // partial head groups
  // head dim 256: dV and dK in one sweep (S once, 256 accumulators, a few spilled registers; default)
  // or two (SXE_FA_DKDV_ONE_SWEEP=0: PART 1 / 2, each recomputes S): one sweep is 1-9 % faster
  // fwd+bwd (profiles/r05/attn_d256_one_sweep_ab.log)
  const bool one_sweep = D >= 256 && env_int("SXE_FA_DKDV_ONE_SWEEP", 1) != 0;
  // head dim 128: 8-wave dK/dV workgroups of 256 keys (SXE_FA_DKDV_WAVES=8, read per call)
  // (auto from 8k keys on, as the dQ kernel; SXE_FA_DKDV_WAVES=4 / 8 forces)
  const int kvw = env_int("SXE_FA_DKDV_WAVES", 0);
  const bool kv8 = D == 128 && Sk % 256 == 0 && (kvw == 8 || (kvw == 0 && Sk >= 8192));
  const size_t lds_kv = (kv8 ? fa::KVL<D, 256>::VBLK : G_::VBLK) + 2 * G_::SLOT + (sp.layout ? kListBytes : 0);
  at::Tensor pk, pv;
  if (partials) {
    pk = at::empty({B, Sk, np, D}, q.options().dtype(at::kFloat));
    pv = at::empty({B, Sk, np, D}, q.options().dtype(at::kFloat));
  }
  // one dK/dV kernel: SPLIT = one workgroup per query-head group (partials / direct), PART (see
  // dkdv_tile), NWK waves per workgroup; `heads` = workgroups per key block and batch
  auto run = [&](auto splitc, auto part, auto nwk, int heads) {
    constexpr bool SP = decltype(splitc)::value;
    constexpr int PART = decltype(part)::value, NWK = decltype(nwk)::value;
    auto go = [&](auto kern, auto... tail) {
      launch<decltype(kern)::value>((Sk / (NWK * fa::QW)) * B * heads, NWK, lds_kv, u16(q), strides_of(q), u16(k),
                                    strides_of(k), u16(v), strides_of(v), u16(dout), strides_of(dout),
                                    lse2.data_ptr<float>(), ndelta.data_ptr<float>(), u16(dk), strides_of(dk), u16(dv),
                                    strides_of(dv), partials ? pk.data_ptr<float>() : nullptr,
                                    partials ? pv.data_ptr<float>() : nullptr, B, H, Hk, Sq, tail...);
    };
    if (m.bd.klo != nullptr) go(kern_t<fa::dkdv_band_kernel<SP, D, PART, NWK>>{}, (float)scale, hpw, m.bd);
    else go(kern_t<fa::dkdv_kernel<SP, D, PART, NWK>>{}, Sk, (float)scale, causal ? 1 : 0, sp, m.qoff, hpw);
  };
  auto run_dkdv = [&](auto splitc, int heads) {
    if constexpr (D >= 256) {
      if (!one_sweep) {
        run(splitc, int_t<1>{}, int_t<4>{}, heads);
        run(splitc, int_t<2>{}, int_t<4>{}, heads);
        return;
      }
    }
    if constexpr (D == 128) {
      if (kv8) {
        run(splitc, int_t<3>{}, int_t<8>{}, heads);
        return;
      }
    }
    run(splitc, int_t<3>{}, int_t<4>{}, heads);
  };
  if (split) {
    run_dkdv(std::true_type{}, np);
    if (partials) {
      const int64_t n8 = (int64_t)B * Sk * Hk * (D / 8);
      hipLaunchKernelGGL(fa::dkdv_reduce_kernel<D>, dim3(stream_grid(n8, 256)), dim3(256), 0, cur_stream(),
                         pk.data_ptr<float>(), pv.data_ptr<float>(), u16(dk), strides_of(dk), u16(dv), strides_of(dv),
                         B, Sk, np, Hk);
      SXE_LAUNCH_CHECK();
    }
  } else {
    run_dkdv(std::false_type{}, Hk);
  }
}

// dq/dk/dv are caller-provided (possibly strided views of one dqkv buffer).
static void bwd_impl(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse,
                     at::Tensor dq, at::Tensor dk, at::Tensor dv, bool causal, double scale, fa::Sparse sp,
                     int64_t kv_len = -1, int64_t causal_offset = INT64_MIN,
                     fa::Band bd = kNoBand) {
  check_qkv(q, k, v);
  check_qkv(dq, dk, dv);
  const Mask m = mask_of(q, k, causal, sp, kv_len, causal_offset, bd);
  SXE_CHECK(dout.sizes() == q.sizes() && o.sizes() == q.sizes() && dout.stride(3) == 1 && o.stride(3) == 1,
            "flash_attn_bwd: dout/o shapes");
  SXE_CHECK(dq.sizes() == q.sizes() && dk.sizes() == k.sizes() && dv.sizes() == v.sizes(), "flash_attn_bwd: grad shapes");
  SXE_CHECK(lse.is_contiguous() && lse.size(2) == q.size(1), "flash_attn_bwd: lse [B, H, Sq]");
  c10::DeviceGuard guard(q.device());
  dispatch_head_dim(q.size(3), "flash_attn_bwd", [&](auto d) {
    bwd_impl_d<decltype(d)::value>(dout, q, k, v, o, lse, dq, dk, dv, scale, m);
  });
}

static int64_t offset_arg(int64_t causal_offset) { return causal_offset == -(int64_t(1) << 40) ? INT64_MIN : causal_offset; }

std::vector<at::Tensor> flash_attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v, bool causal, double scale,
                                       int64_t kv_len, int64_t causal_offset) {
  return fwd_impl(q, k, v, causal, scale, kNoSparse, kv_len, offset_arg(causal_offset));
}

void flash_attn_bwd(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse,
                    at::Tensor dq, at::Tensor dk, at::Tensor dv, bool causal, double scale, int64_t kv_len,
                    int64_t causal_offset) {
  bwd_impl(dout, q, k, v, o, lse, dq, dk, dv, causal, scale, kNoSparse, kv_len, offset_arg(causal_offset));
}

std::vector<at::Tensor> flash_attn_fwd_sparse(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor layout,
                                              int64_t block, bool causal, double scale) {
  return fwd_impl(q, k, v, causal, scale, sparse_of(layout, block, q));
}

void flash_attn_bwd_sparse(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse,
                           at::Tensor dq, at::Tensor dk, at::Tensor dv, at::Tensor layout, int64_t block, bool causal,
                           double scale) {
  bwd_impl(dout, q, k, v, o, lse, dq, dk, dv, causal, scale, sparse_of(layout, block, q));
}

// Band mask on top of the causal one (packed documents, sliding window; see fa::Band): query i sees
// keys klo[b, i] <= j <= i, and qhi[b, j] is the last query that sees key j.
std::vector<at::Tensor> flash_attn_fwd_band(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor klo, at::Tensor qhi,
                                            double scale) {
  return fwd_impl(q, k, v, true, scale, kNoSparse, -1, INT64_MIN, band_of(klo, qhi, q, k));
}

void flash_attn_bwd_band(at::Tensor dout, at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse,
                         at::Tensor dq, at::Tensor dk, at::Tensor dv, at::Tensor klo, at::Tensor qhi, double scale) {
  bwd_impl(dout, q, k, v, o, lse, dq, dk, dv, true, scale, kNoSparse, -1, INT64_MIN, band_of(klo, qhi, q, k));
}

// Causal GQA forward over a ragged token buffer (see fa::Varlen): q [T, Hq, D], k / v [T, Hkv, D], strided
// views of the packed QKV allowed; table int32 [N, 3] on the device, one (first row, length, query block
// of 128) row per workgroup and head; window 0 = none. Writes the rows of the table's sequences into
// `out` (or a fresh [T, Hq, D] tensor whose other rows stay unwritten) and returns it. One launch of
// N * Hq workgroups, nothing read back on the host.
template <int D>
static void fwd_varlen_d(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const at::Tensor& o,
                         const at::Tensor& table, double scale, int window) {
  static_assert(kRingBytes<D> <= kMaxDynamicLds, "varlen LDS exceeds the opt-in limit");
  auto st = [](const at::Tensor& t) { return fa::Strides{0, t.stride(0), t.stride(1)}; };
  const int H = q.size(1), N = table.size(0);
  launch<fa::fwd_varlen_kernel<D>>(N * H, fa::NW, kRingBytes<D>, u16(q), st(q), u16(k), st(k), u16(v), st(v), u16(o),
                                   st(o), H, (int)k.size(1), (float)scale,
                                   fa::Varlen{table.data_ptr<int>(), (int)q.size(0), window});
}

at::Tensor flash_attn_fwd_varlen(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor table, double scale,
                                 int64_t window, c10::optional<at::Tensor> out) {
  SXE_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3, "flash_attn varlen: tensors must be [T, H, D]");
  SXE_CHECK(q.is_cuda() && k.device() == q.device() && v.device() == q.device(), "flash_attn varlen: q/k/v on one GPU");
  const int64_t T = q.size(0), H = q.size(1), D = q.size(2);
  SXE_CHECK(D == 64 || D == 128 || D == 256, "flash_attn varlen: head dim must be 64, 128 or 256");
  SXE_CHECK(k.size(2) == D && v.size(2) == D, "flash_attn varlen: q/k/v head dims differ");
  SXE_CHECK(k.sizes() == v.sizes() && k.size(0) == T, "flash_attn varlen: q/k/v shapes");
  SXE_CHECK(k.size(1) >= 1 && H % k.size(1) == 0, "flash_attn varlen: Hq must be a multiple of Hkv");
  SXE_CHECK(T < (int64_t(1) << 31) / 3, "flash_attn varlen: too many tokens");
  SXE_CHECK(window >= 0, "flash_attn varlen: window must be >= 0 (0 = none)");
  SXE_CHECK(table.is_cuda() && table.device() == q.device() && table.scalar_type() == at::kInt && table.dim() == 2 &&
                table.size(1) == 3 && table.is_contiguous(),
            "flash_attn varlen: table must be contiguous int32 [N, 3] on the device of q");
  SXE_CHECK(table.size(0) * H < (int64_t(1) << 31), "flash_attn varlen: table too long");
  at::Tensor o = out.has_value() && out->defined() ? *out : at::empty({T, H, D}, q.options());
  SXE_CHECK(o.dim() == 3 && o.sizes() == q.sizes() && o.scalar_type() == at::kBFloat16 && o.device() == q.device(),
            "flash_attn varlen: out must be bf16 [T, Hq, D] on the device of q");
  check_bf16_rows({&q, &k, &v, &o}, "flash_attn varlen");
  if (T == 0 || table.size(0) == 0) return o;
  c10::DeviceGuard guard(q.device());
  const int w = window == 0 ? (1 << 30) : (int)std::min<int64_t>(window, 1 << 30);
  dispatch_head_dim(D, "flash_attn varlen", [&](auto d) { fwd_varlen_d<decltype(d)::value>(q, k, v, o, table, scale, w); });
  return o;
}

}  // namespace sxe

TORCH_LIBRARY_FRAGMENT(sxe, m) {
  // causal_offset: query i sees keys <= i + causal_offset; the default sentinel means Sk - Sq
  m.def("flash_attn_fwd(Tensor q, Tensor k, Tensor v, bool causal, float scale, int kv_len=-1, "
        "int causal_offset=-1099511627776) -> Tensor[]");
  m.def("flash_attn_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor(a!) dq, Tensor(b!) dk, "
        "Tensor(c!) dv, bool causal, float scale, int kv_len=-1, int causal_offset=-1099511627776) -> ()");
  m.def("flash_attn_fwd_sparse(Tensor q, Tensor k, Tensor v, Tensor layout, int block, bool causal, float scale) -> Tensor[]");
  m.def("flash_attn_bwd_sparse(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor(a!) dq, "
        "Tensor(b!) dk, Tensor(c!) dv, Tensor layout, int block, bool causal, float scale) -> ()");
  m.def("flash_attn_fwd_band(Tensor q, Tensor k, Tensor v, Tensor klo, Tensor qhi, float scale) -> Tensor[]");
  m.def("flash_attn_bwd_band(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor o, Tensor lse, Tensor(a!) dq, "
        "Tensor(b!) dk, Tensor(c!) dv, Tensor klo, Tensor qhi, float scale) -> ()");
  // returns `out` itself when it is given (eager inference only: the result then aliases an argument)
  m.def("flash_attn_fwd_varlen(Tensor q, Tensor k, Tensor v, Tensor table, float scale, int window=0, "
        "Tensor(a!)? out=None) -> Tensor");
}
TORCH_LIBRARY_IMPL(sxe, CUDA, m) {
  m.impl("flash_attn_fwd", &sxe::flash_attn_fwd);
  m.impl("flash_attn_bwd", &sxe::flash_attn_bwd);
  m.impl("flash_attn_fwd_sparse", &sxe::flash_attn_fwd_sparse);
  m.impl("flash_attn_bwd_sparse", &sxe::flash_attn_bwd_sparse);
  m.impl("flash_attn_fwd_band", &sxe::flash_attn_fwd_band);
  m.impl("flash_attn_bwd_band", &sxe::flash_attn_bwd_band);
  m.impl("flash_attn_fwd_varlen", &sxe::flash_attn_fwd_varlen);
}
