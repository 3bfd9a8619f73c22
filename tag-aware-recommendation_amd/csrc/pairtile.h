// The "owned tile x walked tile" scheme of the fused pairwise losses (csrc/inbatch.hip, csrc/directau.hip, csrc/catsoftmax.hip):
// every piece of it lives here once, and the three files add only what the loss itself needs.
//
// The score matrix is never stored.  One block of four wavefronts OWNS a tile of 64 rows of one operand and WALKS the other
// operand in tiles of 64 rows; both tiles sit in LDS (row stride Dp + 4 floats: the 16 rows a wavefront reads land on 16
// distinct groups of four banks).  A wavefront holds 16 owned rows.  Its 16 x 64 score tile comes from the exact-fp32 MFMA
// 16x16x4 (the one csrc/eval.hip uses): A = walked rows, B = owned rows, so lane (r = lane % 16, q = lane / 16) ends with the
// scores of owned row r against the walked rows 16 t + 4 q + v (t, v = 0 .. 3)  -- score_tile.
//   forward   a softmax keeps a running (maximum, sum) of the lane's own columns, rescaled when the maximum moves (lse_push);
//             the four lanes of a row are merged once, after the walk (lse_merge_q).  The maximum starts at the finite
//             sentinel kLowest, so neither "-inf - (-inf)" nor log(0) can be formed.  A logit z is rounded ONCE, by the same
//             expression in every pass, so that the backward meets the forward's bits.
//   backward  the score tile is recomputed, the coefficient tile C is formed in registers (in place of the scores) and fed
//             STRAIGHT to the second MFMA as its A operand (grad_tile): the k index of an MFMA step may be any permutation of
//             the walked rows as long as the B operand (the walked tile read from LDS by row 16 t + 4 q + v, column 16 f + r)
//             uses the same one, so no hand-over of C through LDS is needed.  The accumulators (NF = Dp / 16 tiles of 16 x 16)
//             stay in registers over the walk and every owned row is stored once: no atomics, and the order of every sum is
//             a function of the shapes only.
// The L2 term rides along: 0.5 |row|^2 one row per wavefront at a time (l2_rows), and in the backward either added to the
// owned rows' store (the L2 gradient shares the buffer of the loss gradient; then the L2 rows ARE the scored rows, which the
// caller checks) or written to buffers of its own after it (l2_grad_tail).
#pragma once
#include <type_traits>

#include "common.h"

namespace tagrec {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kTile = 64;                 // rows of the owned tile = rows of a walked tile = 16 per wavefront
constexpr float kLowest = -3.0e38f;       // start of a running maximum: finite, below every score

struct PairLane {
  int wave, lane, r, q;                   // the lane ends with the scores of the owned row 16 wave + r of the block
};
__device__ __forceinline__ PairLane pair_lane() {
  const int tid = threadIdx.x, lane = tid & 63;
  return {tid >> 6, lane, lane & 15, lane >> 4};
}

constexpr int tile_stride(int Dp) { return Dp + 4; }
constexpr int round16(int D) { return (D + 15) & ~15; }
// the owned and the walked tile
inline size_t tiles_bytes(int Dp) { return 2 * static_cast<size_t>(kTile) * tile_stride(Dp) * sizeof(float); }

// ---- tile staging ----------------------------------------------------------------------------------------------------------

// rows of an operand as a tile walk sees them: row i is X[idx ? idx[i] : i]
struct Rows {
  const float* X;
  int64_t ld;
  const int64_t* idx;
  int vec;                                // 16-byte aligned with ld % 4 == 0: float4 loads
};

__device__ __forceinline__ f32x4 load4(const float* p, bool vec) {
  f32x4 v;
  if (vec) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
  }
  return v;
}

// rows row0 .. row0 + 63 of X (SCALED: each times its inv) -> sh [64, Dp + 4]; rows past B and columns past D are zero
template <bool SCALED>
__device__ __forceinline__ void stage_tile(float* sh, const float* __restrict__ X, const float* __restrict__ inv, int64_t ld, int D,
                                           int Dp, int64_t row0, int64_t B, bool vec) {
  const int S = tile_stride(Dp), c4n = Dp >> 2;
  for (int idx = threadIdx.x; idx < kTile * c4n; idx += kThreads) {
    const int row = idx / c4n, c = (idx - row * c4n) << 2;
    const int64_t gr = row0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (gr < B && c < D) {
      v = load4(X + gr * ld + c, vec);
      if (SCALED) v *= inv[gr];
    }
    *reinterpret_cast<f32x4*>(sh + row * S + c) = v;
  }
}

// the same tile through registers, so that the loads can be in flight under another tile's MFMAs: rows row0 .. row0 + 63 ->
// NF float4 per thread (element idx = tid + 256 i of the [64, Dp / 4] tile); rows >= hi and columns >= D read as zero
template <int NF>
__device__ __forceinline__ void load_tile(f32x4 (&pre)[NF], const Rows& s, int D, int64_t row0, int64_t hi) {
  constexpr int c4n = 4 * NF;
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int idx = threadIdx.x + kThreads * i;
    const int row = idx / c4n, c = (idx - row * c4n) << 2;
    const int64_t gr = row0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (gr < hi && c < D) v = load4(s.X + (s.idx ? s.idx[gr] : gr) * s.ld + c, s.vec != 0);
    pre[i] = v;
  }
}

template <int NF>
__device__ __forceinline__ void store_tile(float* sh, const f32x4 (&pre)[NF]) {
  constexpr int c4n = 4 * NF, S = tile_stride(16 * NF);
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int idx = threadIdx.x + kThreads * i;
    const int row = idx / c4n, c = (idx - row * c4n) << 2;
    *reinterpret_cast<f32x4*>(sh + row * S + c) = pre[i];
  }
}

// ---- the two MFMA loops ----------------------------------------------------------------------------------------------------

// sc[t][v] = owned row 16 wave + r . walked row 16 t + 4 q + v, over the first Dk columns (a multiple of 16)
__device__ __forceinline__ void score_tile(const float* sh_own, const float* sh_walk, int S, int Dk, const PairLane& ln, f32x4 (&sc)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* po = sh_own + (16 * ln.wave + ln.r) * S + 4 * ln.q;
  const float* pw = sh_walk + ln.r * S + 4 * ln.q;
  for (int kk = 0; kk < Dk; kk += 16) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(po + kk);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(pw + t * 16 * S + kk);
#pragma unroll
      for (int c = 0; c < 4; ++c) sc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bv[c], sc[t], 0, 0, 0);
    }
  }
}

// The gradient accumulators of a lane: f[k][v] = owned row 16 wave + 4 q + v, column 16 k + r.  A struct and not a bare array
// on purpose: the compiler's early alloca-to-vector pass leaves a struct alone, so the tiles end as NF independent
// four-register values; as an array they became one 16 NF-wide vector, which cost cat_dt_kernel<4> a wave of occupancy.
template <int NF>
struct AccTiles {
  f32x4 f[NF];
};

template <int NF>
__device__ __forceinline__ void zero_acc(AccTiles<NF>& acc) {
#pragma unroll
  for (int f = 0; f < NF; ++f) acc.f[f] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc.f[f] += C [16 owned, 64 walked] . walked tile [64, 16 f .. 16 f + 15], C in the layout score_tile leaves; MFMA step
// (t, v) takes k = 16 t + 4 q + v
template <int NF>
__device__ __forceinline__ void grad_tile(const float* sh_walk, int S, const PairLane& ln, const f32x4 (&sc)[4], AccTiles<NF>& acc) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float* pb = sh_walk + (16 * t + 4 * ln.q + v) * S + ln.r;
#pragma unroll
      for (int f = 0; f < NF; ++f) acc.f[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[t][v], pb[16 * f], acc.f[f], 0, 0, 0);
    }
  }
}

// ---- log-sum-exp as a running (maximum, sum) ---------------------------------------------------------------------------------

__device__ __forceinline__ void lse_push(float& m, float& s, float z) {
  if (z > m) {
    s = s * expf(m - z) + 1.0f;
    m = z;
  } else {
    s += expf(z - m);
  }
}

// an empty side holds (kLowest, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = s * expf(m - mn) + s2 * expf(m2 - mn);
  m = mn;
}

// merge the four lanes of a row (q = 0 .. 3) in a fixed order; every one of them ends with the row's pair
__device__ __forceinline__ void lse_merge_q(float& m, float& s) {
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) lse_merge(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
}

// ---- fixed-order sums ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

// this lane's share of s + |p[0 .. n)|^2
__device__ __forceinline__ float lane_sumsq(const float* __restrict__ p, int n, int lane, float s = 0.f) {
  for (int c = lane; c < n; c += 64) s = fmaf(p[c], p[c], s);
  return s;
}

// sum of |row|^2 over the rows row0 + rows * wave + i (i < rows, row < B) of two operands, row_ptr(side, row) -> the row:
// one row per wavefront at a time, fixed order; every lane of a wavefront returns the wavefront's sum
template <class RowPtr>
__device__ __forceinline__ float l2_rows(RowPtr row_ptr, int64_t row0, int rows, int64_t B, int n, const PairLane& ln) {
  float reg = 0.f;
  for (int side = 0; side < 2; ++side) {
    for (int i = 0; i < rows; ++i) {
      const int64_t row = row0 + rows * ln.wave + i;
      if (row >= B) break;
      reg += wave_sum(lane_sumsq(row_ptr(side, row), n, ln.lane));
    }
  }
  return reg;
}

// out[k] = p[k] + p[k + stride] + .. (n terms): strided per-thread sums, then a fixed tree; every thread gets the totals
template <int K>
__device__ __forceinline__ void block_sum(const float* __restrict__ p, int64_t n, int stride, float (*sh)[kThreads], float (&out)[K]) {
  float s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += p[i * stride + k];
  }
  __syncthreads();                                       // the previous use of sh is over
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int off = kThreads / 2; off >= 1; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) {
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = sh[k][0];
}

// the body of a one-block reduce kernel: loss_out[k] = inv_b * sum over blocks of partials[2 i + k] = [loss, l2reg]
__device__ __forceinline__ void reduce_loss_pair(const float* __restrict__ partials, int64_t n, float inv_b, float* __restrict__ loss_out) {
  __shared__ float sh[2][kThreads];
  float tot[2];
  block_sum<2>(partials, n, 2, sh, tot);
  if (threadIdx.x == 0) {
    loss_out[0] = tot[0] * inv_b;
    loss_out[1] = tot[1] * inv_b;
  }
}

// the L2 gradient of the block's 64 owned rows into a buffer of its own: dR[row] = rscale R[row]
__device__ __forceinline__ void l2_grad_tail(float* dR, const float* R, int64_t ldreg, int Dreg, float rscale, int64_t own0, int64_t B) {
  for (int idx = threadIdx.x; idx < kTile * Dreg; idx += kThreads) {
    const int row = idx / Dreg, c = idx - row * Dreg;
    const int64_t gr = own0 + row;
    if (gr < B) dR[gr * ldreg + c] = rscale * R[gr * ldreg + c];
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------

// the accumulator tiles the NF-templated kernels are built for: the smallest NF with 16 NF >= D
inline int pick_nf(int D) {
  const int nfs[] = {1, 2, 4, 8, 12, 16};
  for (int nf : nfs)
    if (16 * nf >= D) return nf;
  return 0;
}

// f(std::integral_constant<int, NF>) for the NF that pick_nf gave
template <class F>
int dispatch_nf(int nf, F&& f) {
  switch (nf) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}

// Dynamic LDS past the default 64 KB (D > 112) needs the function attribute: it is set once per kernel instantiation and
// device (the largest size asked for so far), so a later launch -- one inside a stream capture included -- makes no host call.
template <class Args, void (*KERN)(Args)>
int launch_lds(dim3 grid, size_t lds, const Args& a, hipStream_t s) {
  constexpr int kMaxDevices = 64;
  static int granted[kMaxDevices] = {};
  if (lds > 64 * 1024) {
    int dev = 0;
    TAGREC_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices || granted[dev] < static_cast<int>(lds)) {
      TAGREC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
      if (dev >= 0 && dev < kMaxDevices) granted[dev] = static_cast<int>(lds);
    }
  }
  KERN<<<grid, kThreads, lds, s>>>(a);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

// D and B as the tiles can take them; b_note goes after the range of B in the message
inline int check_rows(const std::string& what, int64_t B, int64_t b_min, const char* b_note, int D) {
  if (D < 8 || D > 256 || (D & 3) != 0)
    return fail(TAGREC_E_UNSUPPORTED, what + ": D must be a multiple of 4 in 8 .. 256, got " + std::to_string(D));
  if (B < b_min || B > 65536)
    return fail(TAGREC_E_UNSUPPORTED, what + ": B must be in " + std::to_string(b_min) + " .. 65536" + b_note + ", got " + std::to_string(B));
  return TAGREC_OK;
}

inline int check_stride(const std::string& what, int64_t ld, int D) {
  if (ld < D) return fail(TAGREC_E_INVALID, what + ": row stride below D");
  return TAGREC_OK;
}

inline int check_temperature(const std::string& what, float temperature) {
  if (!(temperature > 0.f && temperature <= 3.4028234e38f)) return fail(TAGREC_E_INVALID, what + ": the temperature must be finite and > 0");
  return TAGREC_OK;
}

}  // namespace tagrec
