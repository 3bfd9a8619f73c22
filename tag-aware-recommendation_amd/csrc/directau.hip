// DirectAU on compact rows: alignment of the positive pairs plus the uniformity of the batch's users and of its items on the
// unit sphere (Wang et al., KDD 2022) as a fused B x B loss (tagrec_directau_fwd_f32 / tagrec_directau_bwd_f32).
//
// The tile scheme is the one of csrc/pairtile.h (owned tile x walked tile in LDS, score MFMA, the coefficients fed straight
// to the second MFMA).  What is this loss's own:
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

#include "pairtile.h"

namespace tagrec {
namespace {

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
      reg = wave_sum(lane_sumsq(ri, a.Dreg, lane, lane_sumsq(ru, a.Dreg, lane)));
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
  const int S = tile_stride(a.Dp);
  float* sh_walk = sh_own + kTile * S;

  const int side = blockIdx.y;
  const PairLane ln = pair_lane();
  const int tid = threadIdx.x, wave = ln.wave, lane = ln.lane, r = ln.r, q = ln.q;
  const int64_t B = a.B, own0 = static_cast<int64_t>(blockIdx.x) * kTile;
  const bool vec = a.vec != 0;
  const float* X = a.X[side];
  const float* inv = a.inv + side * B;

  stage_tile<true>(sh_own, X, inv, a.ld, a.D, a.Dp, own0, B, vec);

  const int64_t o = own0 + 16 * wave + r;                // the owned row whose scores this lane ends up with
  const float g0 = (MODE == 1 && a.g) ? a.g[0] : 1.0f;
  const float coef = MODE == 1 ? (g0 * (0.5f * a.gamma)) * a.t2 : 0.f;
  const float ls = MODE == 1 ? a.ls[side] : 0.f;

  float sum = 0.f;                                       // forward: this lane's entries only
  AccTiles<NF> acc;
  zero_acc(acc);

  for (int64_t w0 = MODE == 0 ? own0 : 0; w0 < B; w0 += kTile) {
    __syncthreads();                                     // the previous walked tile has been consumed
    stage_tile<true>(sh_walk, X, inv, a.ld, a.D, a.Dp, w0, B, vec);
    __syncthreads();

    f32x4 sc[4];
    score_tile(sh_own, sh_walk, S, a.Dk, ln, sc);
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
    if (MODE != 0) grad_tile<NF>(sh_walk, S, ln, sc, acc);
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
    // acc.f[f][v] = G of owned row 16 wave + 4 q + v, column 16 f + r; the row's x^ is sh_own[that row][that column]
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
        if (ok && c < a.D) acc.f[f][v] = fmaf(ascale, xh - P[row * a.ld + c] * pi, acc.f[f][v]);
        dot = fmaf(acc.f[f][v], xh, dot);
      }
#pragma unroll
      for (int off = 1; off <= 8; off <<= 1) dot += __shfl_xor(dot, off);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int c = 16 * f + r;
        if (ok && c < a.D) {
          float val = oi * fmaf(-xo[16 * f], dot, acc.f[f][v]);
          if (shared) val += rscale * R[row * a.ldreg + c];
          dX[row * a.ld + c] = val;
        }
      }
    }
    if (dR != nullptr && !shared) l2_grad_tail(dR, R, a.ldreg, a.Dreg, rscale, own0, B);
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

// prep [2 n_prep] and uni [2][n_uni] -> ls[side] = logf(S_side), parts = [align, unif_u, unif_i], loss_out = [mul_loss, l2reg]
__global__ __launch_bounds__(kThreads) void au_reduce_kernel(const float* __restrict__ prep, int64_t n_prep, const float* __restrict__ uni,
                                                             int64_t n_uni, float inv_b, float gamma, float log_pairs,
                                                             float* __restrict__ ls, float* __restrict__ parts,
                                                             float* __restrict__ loss_out) {
  __shared__ float sh[2][kThreads];
  float pre[2], su[1], si[1];                            // [align, l2reg] of the pairs, S of the two sides
  block_sum<2>(prep, n_prep, 2, sh, pre);
  block_sum<1>(uni, n_uni, 1, sh, su);
  block_sum<1>(uni + n_uni, n_uni, 1, sh, si);
  if (threadIdx.x == 0) {
    const float align = pre[0] * inv_b, reg = pre[1] * inv_b, lu = logf(su[0]), li = logf(si[0]);
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

size_t lds_bytes(int Dp) { return 16 * sizeof(float) + tiles_bytes(Dp); }

int check_args(const char* what, int64_t B, int D, int64_t ld, float t, float gamma) {
  const std::string w(what);
  if (int rc = check_rows(w, B, 2, " (one pair has no other to be uniform against)", D)) return rc;
  if (int rc = check_stride(w, ld, D)) return rc;
  if (!(t > 0.f && t <= 20.f)) return fail(TAGREC_E_INVALID, w + ": t must be in (0, 20]");
  if (!(gamma >= 0.f && gamma <= 3.4028234e38f)) return fail(TAGREC_E_INVALID, w + ": gamma must be finite and >= 0");
  return TAGREC_OK;
}

AuArgs make_args(const float* Ub, const float* Ib, int64_t ld, int D, int Dp, const float* Ureg, const float* Ireg, int64_t ldreg,
                 int Dreg, int64_t B, float t, float gamma, const float* inv) {
  AuArgs a = {};
  a.X[0] = Ub; a.X[1] = Ib; a.ld = ld; a.D = D; a.Dk = round16(D); a.Dp = Dp;
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
  AuArgs a = make_args(Ub, Ib, ld, D, round16(D), Ureg, Ireg, ldreg, Dreg, B, t, gamma, inv);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n_prep = (B + kPrepRows - 1) / kPrepRows, n_uni = (B + kTile - 1) / kTile;
  float* uni = partials + 2 * n_prep;
  a.partials = uni;
  au_prep_kernel<<<static_cast<unsigned>(n_prep), kThreads, 0, s>>>(a, inv, partials);
  TAGREC_LAUNCH_CHECK();
  if (int rc = launch_lds<AuArgs, au_uniform_fwd_kernel>(dim3(static_cast<unsigned>(n_uni), 2), lds_bytes(a.Dp), a, s)) return rc;
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
  return dispatch_nf(nf, [&](auto n) { return launch_lds<AuArgs, au_bwd_kernel<decltype(n)::value>>(grid, lds, a, s); });
}
