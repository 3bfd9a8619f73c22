// DirectAU on compact rows: alignment of the positive pairs plus the uniformity of the batch's users and of its items on the
// unit sphere (Wang et al., KDD 2022) as a fused B x B loss (tagrec_directau_fwd_f32 / tagrec_directau_bwd_f32).
//
// The tile scheme is the one of csrc/inbatch.hip: one block of four wavefronts OWNS 64 rows and WALKS tiles of 64 rows, both
// tiles in LDS (row stride Dp + 4 floats), scores from the exact-fp32 MFMA 16x16x4, lane (r = lane % 16, q = lane / 16) ending
// with the scores of owned row r against the walked rows 16 t + 4 q + v.  What differs:
//   * one operand against ITSELF (blockIdx.y picks the users or the items), staged already normalised (row x inv), so a score
//     is a cosine and |x_i - x_j|^2 = 2 - 2 s_ij: a term is expf(2 t (s_ij - 1)), its exponent <= 0 up to rounding and >= -4 t
//     >= -80 (t <= 20), a normal fp32 number -- no running maximum, no rescaling;
//   * the forward uses the symmetry: the block that owns tile k walks tiles k .. last and a lane adds an entry iff o < w < B;
//   * one global sum per side: lane -> wavefront tree -> block partial -> the reduce kernel, every step in a fixed order;
//   * the backward walks all tiles, forms C_ij = coef expf(2 t (s_ij - 1) - ls) (never a product with 1 / S: S reaches 1e-35),
//     feeds it STRAIGHT to the second MFMA as its A operand (G = C X^ in the accumulators) and its epilogue adds the alignment
//     term, pushes G through the row normalisation dE_i = inv_i (G_i - x^_i (x^_i . G_i)) and stores every owned row once.
// No float atomics anywhere: the order of every sum is a function of (B, D) only.
#include <cmath>

#include "common.h"

namespace tagrec {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kTile = 64;                 // rows of the owned tile = rows of a walked tile = 16 per wavefront
constexpr int kPrepRows = 4;              // au_prep: batch positions per block, one per wavefront
constexpr float kNormEps = 1e-12f;        // F.normalize's clamp

struct AuArgs {
  const float* X[2];                      // 0: Ub, 1: Ib (row b of Ib is the positive of row b of Ub)
  int64_t ld;
  int D, Dk, Dp;                          // Dk = D rounded up to 16 (score loop), Dp = 16 NF >= Dk (LDS row width)
  int vec;                                // both operands 16-byte aligned with ld % 4 == 0: float4 loads
  const float* Xreg[2];
  int64_t ldreg;
  int Dreg;
  int64_t B;
  float t2, inv_b, gamma;                 // t2 = 2 t
  const float* inv;                       // [2 B]: 1 / max(|row|, 1e-12) of the rows of Ub, then of Ib
  float* partials;                        // forward: block sums of the uniformity terms, [2][ceil(B / 64)]
  const float* ls;                        // backward: log S of the two sides
  const float* g;
  float* dX[2];
  float* dXreg[2];
};

// rows row0 .. row0 + 63 of X, each times its inv -> sh [64, Dp + 4]; rows past B and columns past D are zero
__device__ __forceinline__ void stage_tile(float* sh, const float* __restrict__ X, const float* __restrict__ inv, int64_t ld, int D,
                                           int Dp, int64_t row0, int64_t B, bool vec) {
  const int S = Dp + 4, c4n = Dp >> 2;
  for (int idx = threadIdx.x; idx < kTile * c4n; idx += kThreads) {
    const int row = idx / c4n, c = (idx - row * c4n) << 2;
    const int64_t gr = row0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (gr < B && c < D) {
      const float* p = X + gr * ld + c;
      if (vec) {
        v = *reinterpret_cast<const f32x4*>(p);
      } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
      }
      v *= inv[gr];
    }
    *reinterpret_cast<f32x4*>(sh + row * S + c) = v;
  }
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

// One wavefront per batch position b: inv of U_b and I_b, the alignment term sum_c (u^_c - i^_c)^2 in the difference form
// and 0.5 |row|^2 of the two L2 rows; partials[2 block] / [2 block + 1] = the block's sums over its four positions.
__global__ __launch_bounds__(kThreads) void au_prep_kernel(AuArgs a, float* __restrict__ inv_out, float* __restrict__ partials) {
  __shared__ float sh_red[2 * kPrepRows];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kPrepRows + wave;
  float align = 0.f, reg = 0.f;
  if (b < a.B) {
    const float* pu = a.X[0] + b * a.ld;
    const float* pi = a.X[1] + b * a.ld;
    float su = 0.f, si = 0.f;
    for (int c = lane; c < a.D; c += 64) {
      su = fmaf(pu[c], pu[c], su);
      si = fmaf(pi[c], pi[c], si);
    }
    const float iu = 1.0f / fmaxf(sqrtf(wave_sum(su)), kNormEps), ii = 1.0f / fmaxf(sqrtf(wave_sum(si)), kNormEps);
    if (lane == 0) {
      inv_out[b] = iu;
      inv_out[a.B + b] = ii;
    }
    for (int c = lane; c < a.D; c += 64) {
      const float d = pu[c] * iu - pi[c] * ii;
      align = fmaf(d, d, align);
    }
    align = wave_sum(align);
    if (a.Xreg[0]) {
      const float* ru = a.Xreg[0] + b * a.ldreg;
      const float* ri = a.Xreg[1] + b * a.ldreg;
      float s = 0.f;
      for (int c = lane; c < a.Dreg; c += 64) s = fmaf(ru[c], ru[c], s);
      for (int c = lane; c < a.Dreg; c += 64) s = fmaf(ri[c], ri[c], s);
      reg = wave_sum(s);
    }
  }
  if (lane == 0) {
    sh_red[wave] = align;
    sh_red[kPrepRows + wave] = reg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = (sh_red[0] + sh_red[1]) + (sh_red[2] + sh_red[3]);
    partials[2 * blockIdx.x + 1] = 0.5f * ((sh_red[4] + sh_red[5]) + (sh_red[6] + sh_red[7]));
  }
}

// MODE 0: the triangular forward sum.  MODE 1: the backward with its epilogue.  blockIdx.y = the side.
template <int MODE, int NF>
__device__ __forceinline__ void au_body(const AuArgs& a, unsigned char* smem) {
  float* sh_red = reinterpret_cast<float*>(smem);        // 16 floats
  float* sh_own = sh_red + 16;
  const int S = a.Dp + 4;
  float* sh_walk = sh_own + kTile * S;

  const int side = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int64_t B = a.B, own0 = static_cast<int64_t>(blockIdx.x) * kTile;
  const bool vec = a.vec != 0;
  const float* X = a.X[side];
  const float* inv = a.inv + side * B;

  stage_tile(sh_own, X, inv, a.ld, a.D, a.Dp, own0, B, vec);

  const int64_t o = own0 + 16 * wave + r;                // the owned row whose scores this lane ends up with
  const float g0 = (MODE == 1 && a.g) ? a.g[0] : 1.0f;
  const float coef = MODE == 1 ? (g0 * (0.5f * a.gamma)) * a.t2 : 0.f;
  const float ls = MODE == 1 ? a.ls[side] : 0.f;

  float sum = 0.f;                                       // forward: this lane's entries only
  f32x4 acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t w0 = MODE == 0 ? own0 : 0; w0 < B; w0 += kTile) {
    __syncthreads();                                     // the previous walked tile has been consumed
    stage_tile(sh_walk, X, inv, a.ld, a.D, a.Dp, w0, B, vec);
    __syncthreads();

    f32x4 sc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* po = sh_own + (16 * wave + r) * S + 4 * q;
    const float* pw = sh_walk + r * S + 4 * q;
    for (int kk = 0; kk < a.Dk; kk += 16) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(po + kk);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(pw + t * 16 * S + kk);
#pragma unroll
        for (int c = 0; c < 4; ++c) sc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bv[c], sc[t], 0, 0, 0);
      }
    }
    // sc[t][v] = owned row o . walked row w0 + 16 t + 4 q + v (both unit rows: a cosine)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t w = w0 + 16 * t + 4 * q + v;
        const float z = a.t2 * (sc[t][v] - 1.0f);
        if (MODE == 0) {
          if (o < w && w < B) sum += expf(z);
        } else {
          sc[t][v] = (o < B && w < B && w != o) ? coef * expf(z - ls) : 0.0f;
        }
      }
    }
    if (MODE != 0) {
      // acc[f] += C [16 owned, 64 walked] . walked tile [64, 16 f .. 16 f + 15]; MFMA step (t, v) takes k = 16 t + 4 q + v
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float* pb = sh_walk + (16 * t + 4 * q + v) * S + r;
#pragma unroll
          for (int f = 0; f < NF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[t][v], pb[16 * f], acc[f], 0, 0, 0);
        }
      }
    }
  }

  if (MODE == 0) {
    sum = wave_sum(sum);
    if (lane == 0) sh_red[wave] = sum;
    __syncthreads();
    if (tid == 0) a.partials[static_cast<int64_t>(side) * gridDim.x + blockIdx.x] = (sh_red[0] + sh_red[1]) + (sh_red[2] + sh_red[3]);
  } else {
    float* dX = a.dX[side];
    float* dR = a.dXreg[side];
    const float* R = a.Xreg[side];
    const float* P = a.X[1 - side];                      // the partner rows of the alignment term
    const float* pinv = a.inv + (1 - side) * B;
    const float ascale = g0 * (2.0f * a.inv_b);
    const float rscale = (a.g ? a.g[1] : 1.0f) * a.inv_b;
    const bool shared = dR != nullptr && dR == dX;       // one buffer takes both parts (then Xreg = X, checked by the caller)
    // acc[f][v] = G of owned row 16 wave + 4 q + v, column 16 f + r; the row's x^ is sh_own[that row][that column]
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int lrow = 16 * wave + 4 * q + v;
      const int64_t row = own0 + lrow;
      const bool ok = row < B;
      const float pi = ok ? pinv[row] : 0.f, oi = ok ? inv[row] : 0.f;
      const float* xo = sh_own + lrow * S + r;
      float dot = 0.f;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int c = 16 * f + r;
        const float xh = xo[16 * f];
        if (ok && c < a.D) acc[f][v] = fmaf(ascale, xh - P[row * a.ld + c] * pi, acc[f][v]);
        dot = fmaf(acc[f][v], xh, dot);
      }
#pragma unroll
      for (int off = 1; off <= 8; off <<= 1) dot += __shfl_xor(dot, off);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int c = 16 * f + r;
        if (ok && c < a.D) {
          float val = oi * fmaf(-xo[16 * f], dot, acc[f][v]);
          if (shared) val += rscale * R[row * a.ldreg + c];
          dX[row * a.ld + c] = val;
        }
      }
    }
    if (dR != nullptr && !shared) {
      for (int idx = tid; idx < kTile * a.Dreg; idx += kThreads) {
        const int row = idx / a.Dreg, c = idx - row * a.Dreg;
        const int64_t gr = own0 + row;
        if (gr < B) dR[gr * a.ldreg + c] = rscale * R[gr * a.ldreg + c];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void au_uniform_fwd_kernel(AuArgs a) {
  extern __shared__ __align__(16) unsigned char au_smem[];
  au_body<0, 1>(a, au_smem);
}

template <int NF>
__global__ __launch_bounds__(kThreads) void au_bwd_kernel(AuArgs a) {
  extern __shared__ __align__(16) unsigned char au_smem[];
  au_body<1, NF>(a, au_smem);
}

// sum of p[0], p[stride], .. (n terms): strided per-thread sums, then a fixed tree; every thread returns the total
__device__ __forceinline__ float block_sum(const float* __restrict__ p, int64_t n, int stride, float* sh) {
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) s += p[i * stride];
  __syncthreads();                                       // the previous use of sh is over
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = kThreads / 2; off >= 1; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  return sh[0];
}

// prep [2 n_prep] and uni [2][n_uni] -> ls[side] = logf(S_side), parts = [align, unif_u, unif_i], loss_out = [mul_loss, l2reg]
__global__ __launch_bounds__(kThreads) void au_reduce_kernel(const float* __restrict__ prep, int64_t n_prep, const float* __restrict__ uni,
                                                             int64_t n_uni, float inv_b, float gamma, float log_pairs,
                                                             float* __restrict__ ls, float* __restrict__ parts,
                                                             float* __restrict__ loss_out) {
  __shared__ float sh[kThreads];
  const float align = block_sum(prep, n_prep, 2, sh) * inv_b;
  const float reg = block_sum(prep + 1, n_prep, 2, sh) * inv_b;
  const float lu = logf(block_sum(uni, n_uni, 1, sh));
  const float li = logf(block_sum(uni + n_uni, n_uni, 1, sh));
  if (threadIdx.x == 0) {
    const float uu = lu + log_pairs, ui = li + log_pairs;
    ls[0] = lu;
    ls[1] = li;
    parts[0] = align;
    parts[1] = uu;
    parts[2] = ui;
    loss_out[0] = fmaf(0.5f * gamma, uu + ui, align);
    loss_out[1] = reg;
  }
}

size_t lds_bytes(int Dp) { return 16 * sizeof(float) + 2 * static_cast<size_t>(kTile) * (Dp + 4) * sizeof(float); }

// the accumulator tiles the backward is built for: the smallest NF with 16 NF >= D
int pick_nf(int D) {
  const int nfs[] = {1, 2, 4, 8, 12, 16};
  for (int nf : nfs)
    if (16 * nf >= D) return nf;
  return 0;
}

int check_args(const char* what, int64_t B, int D, int64_t ld, float t, float gamma) {
  const std::string w(what);
  if (D < 8 || D > 256 || (D & 3) != 0)
    return fail(TAGREC_E_UNSUPPORTED, w + ": D must be a multiple of 4 in 8 .. 256, got " + std::to_string(D));
  if (B < 2 || B > 65536)
    return fail(TAGREC_E_UNSUPPORTED, w + ": B must be in 2 .. 65536 (one pair has no other to be uniform against), got " + std::to_string(B));
  if (ld < D) return fail(TAGREC_E_INVALID, w + ": row stride below D");
  if (!(t > 0.f && t <= 20.f)) return fail(TAGREC_E_INVALID, w + ": t must be in (0, 20]");
  if (!(gamma >= 0.f && gamma <= 3.4028234e38f)) return fail(TAGREC_E_INVALID, w + ": gamma must be finite and >= 0");
  return TAGREC_OK;
}

// Dynamic LDS past the default 64 KB (D > 112) needs the function attribute: it is set once per kernel instantiation and
// device (the largest size asked for so far), so a later launch -- one inside a stream capture included -- makes no host call.
template <void (*KERN)(AuArgs)>
int launch(dim3 grid, size_t lds, const AuArgs& a, hipStream_t s) {
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

AuArgs make_args(const float* Ub, const float* Ib, int64_t ld, int D, int Dp, const float* Ureg, const float* Ireg, int64_t ldreg,
                 int Dreg, int64_t B, float t, float gamma, const float* inv) {
  AuArgs a = {};
  a.X[0] = Ub; a.X[1] = Ib; a.ld = ld; a.D = D; a.Dk = (D + 15) & ~15; a.Dp = Dp;
  a.vec = aligned16(Ub) && aligned16(Ib) && (ld & 3) == 0;
  a.Xreg[0] = Ureg; a.Xreg[1] = Ireg; a.ldreg = ldreg; a.Dreg = Dreg;
  a.B = B; a.t2 = 2.0f * t; a.inv_b = 1.0f / static_cast<float>(B); a.gamma = gamma; a.inv = inv;
  return a;
}

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_directau_fwd_f32(const float* Ub, const float* Ib, int64_t ld, int D, const float* Ureg, const float* Ireg,
                                       int64_t ldreg, int Dreg, int64_t B, float t, float gamma, float* inv, float* ls,
                                       float* partials, float* parts, float* loss_out, void* stream) {
  TAGREC_REQUIRE(Ub && Ib && inv && ls && partials && parts && loss_out, "directau_fwd: null pointer");
  TAGREC_REQUIRE((Ureg == nullptr) == (Ireg == nullptr), "directau_fwd: Ureg/Ireg must both be given or both null");
  TAGREC_REQUIRE(!Ureg || (Dreg >= 1 && ldreg >= Dreg), "directau_fwd: bad reg shape");
  if (int rc = check_args("directau_fwd", B, D, ld, t, gamma)) return rc;
  AuArgs a = make_args(Ub, Ib, ld, D, (D + 15) & ~15, Ureg, Ireg, ldreg, Dreg, B, t, gamma, inv);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n_prep = (B + kPrepRows - 1) / kPrepRows, n_uni = (B + kTile - 1) / kTile;
  float* uni = partials + 2 * n_prep;
  a.partials = uni;
  au_prep_kernel<<<static_cast<unsigned>(n_prep), kThreads, 0, s>>>(a, inv, partials);
  TAGREC_LAUNCH_CHECK();
  if (int rc = launch<au_uniform_fwd_kernel>(dim3(static_cast<unsigned>(n_uni), 2), lds_bytes(a.Dp), a, s)) return rc;
  // the number of pairs in double on the host: log(2 / (B (B - 1)))
  const float log_pairs = static_cast<float>(std::log(2.0 / (static_cast<double>(B) * static_cast<double>(B - 1))));
  au_reduce_kernel<<<1, kThreads, 0, s>>>(partials, n_prep, uni, n_uni, a.inv_b, gamma, log_pairs, ls, parts, loss_out);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_directau_bwd_f32(const float* Ub, const float* Ib, int64_t ld, int D, const float* Ureg, const float* Ireg,
                                       int64_t ldreg, int Dreg, int64_t B, float t, float gamma, const float* inv, const float* ls,
                                       const float* g, float* dUb, float* dIb, float* dUreg, float* dIreg, void* stream) {
  TAGREC_REQUIRE(Ub && Ib && inv && ls && dUb && dIb, "directau_bwd: null pointer");
  TAGREC_REQUIRE((Ureg == nullptr) == (Ireg == nullptr) && (dUreg == nullptr) == (dIreg == nullptr),
                 "directau_bwd: Ureg/Ireg and dUreg/dIreg must both be given or both null");
  TAGREC_REQUIRE(!dUreg || (Ureg && Dreg >= 1 && ldreg >= Dreg), "directau_bwd: bad reg arguments");
  TAGREC_REQUIRE(!dUreg || ((dUreg == dUb) == (dIreg == dIb)), "directau_bwd: dUreg/dIreg must both alias dUb/dIb or neither");
  TAGREC_REQUIRE(!dUreg || dUreg != dUb || (Ureg == Ub && Ireg == Ib && ldreg == ld && Dreg == D),
                 "directau_bwd: a gradient buffer shared by both parts needs Ureg = Ub and Ireg = Ib");
  if (int rc = check_args("directau_bwd", B, D, ld, t, gamma)) return rc;
  const int nf = pick_nf(D);
  AuArgs a = make_args(Ub, Ib, ld, D, 16 * nf, Ureg, Ireg, ldreg, Dreg, B, t, gamma, inv);
  a.ls = ls; a.g = g; a.dX[0] = dUb; a.dX[1] = dIb; a.dXreg[0] = dUreg; a.dXreg[1] = dIreg;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((B + kTile - 1) / kTile), 2);
  const size_t lds = lds_bytes(a.Dp);
  switch (nf) {
    case 1: return launch<au_bwd_kernel<1>>(grid, lds, a, s);
    case 2: return launch<au_bwd_kernel<2>>(grid, lds, a, s);
    case 4: return launch<au_bwd_kernel<4>>(grid, lds, a, s);
    case 8: return launch<au_bwd_kernel<8>>(grid, lds, a, s);
    case 12: return launch<au_bwd_kernel<12>>(grid, lds, a, s);
    default: return launch<au_bwd_kernel<16>>(grid, lds, a, s);
  }
}
