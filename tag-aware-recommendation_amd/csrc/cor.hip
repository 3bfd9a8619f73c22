// Distance-correlation loss between the K factor slices of X [n, D] (the reference's cor_loss,
// /root/reference/model/help/loss.py:53-80) and its gradient, without an n x n buffer.
//
//   d^f_ij = sqrt(|x^f_i - x^f_j|^2 + 1e-8)               per slice f (width dk = D / K), direct differences
//   A^f    = d^f - rowmean - colmean + mean
//   dcov(f, g) = sqrt(max(sum_ij A^f A^g / n^2, 0) + 1e-8)
//   loss   = sum_{f < K-1} dcov(f, f+1) / (sqrt(max(dcov(f, f) dcov(f+1, f+1), 0)) + 1e-10) / ((K + 1) K / 2)
//
// Every pass recomputes the distances from a tile of j-rows held in LDS.  A row i is owned by W = G * spl lanes of one
// wavefront: G lanes side by side hold the K slices of x_i in registers (S slices each, S = 1 unless K > 64) and spl
// such groups share the j-rows of a tile (lane group s takes j = s, s + spl, ...).  A pair's centred value of the
// neighbouring slice comes from the neighbouring lane; sums over j are folded across the spl groups by a butterfly of
// lane exchanges, so every sum has one fixed order and a row's result is written once, by its owner -- no atomics.
//
//   forward :  rowsum [n, K]  ->  column sums (grand sums [K])  ->  per-row sum_j A^f A^f, A^f A^{f+1} [n, 2K]
//              ->  column sums (the 2K - 1 covariance sums)  ->  loss and the backward coefficients coef [K, 3]
//   backward:  dL/dd^f_ij = coef[f][0] A^{f-1}_ij + coef[f][1] A^f_ij + coef[f][2] A^{f+1}_ij  (centring is a projection),
//              dX^f_i = 2 sum_j dL/dd^f_ij (x^f_i - x^f_j) / d^f_ij
//
// The sums over j and over rows are kept in double (a handful of operations per pair next to the 2 dk of the distance);
// distances, centring and the gradient rows are fp32.
#include "common.h"

namespace tagrec {
namespace {

constexpr int kCorThreads = 256;
constexpr int kCorLdsFloats = 12288;      // 48 KiB of tile per workgroup

template <int DK, int S>
struct CorShape {
  static constexpr int E = DK * S;               // floats of x_i per lane
  static constexpr int PAD = DK >= 8 ? 4 : 0;    // floats between two slices of an LDS row: spreads the G lanes over the banks
  static constexpr int FS = DK + PAD;            // LDS floats per slice
  static_assert(S == 1 || PAD == 0, "several slices per lane are read as one contiguous run");
};

struct CorPlan {
  int DK, S, G, spl, tj;
  unsigned blocks;
  size_t lds_bytes;
};

// lanes of a row and its place in the block
struct CorLane {
  int rl, s, g;
  __device__ CorLane(int G, int spl) {
    const int W = G * spl, t = threadIdx.x;
    rl = t / W;
    s = (t % W) / G;
    g = t % G;
  }
};

// rows [j0, j0 + tj) of x -> LDS, slice f of a row at f * FS; rows past n are zero-filled
template <int DK, int S>
__device__ __forceinline__ void cor_load_tile(float* sm, const float* __restrict__ x, int64_t ld, int64_t n, int64_t j0, int tj,
                                              int D, int rs) {
  using Sh = CorShape<DK, S>;
  const int shift = __builtin_ctz(static_cast<unsigned>(D >> 2));
  const int total = tj << shift;
  for (int idx = threadIdx.x; idx < total; idx += kCorThreads) {
    const int jj = idx >> shift, e = (idx - (jj << shift)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j0 + jj < n) v = *reinterpret_cast<const float4*>(x + (j0 + jj) * ld + e);
    const int off = jj * rs + (DK >= 4 ? (e / DK) * Sh::FS + (e % DK) : e);
    *reinterpret_cast<float4*>(sm + off) = v;
  }
}

// row means of the tile's rows (0 past n)
__device__ __forceinline__ void cor_load_means(float* sm_rm, const double* __restrict__ rowsum, int64_t n, int64_t j0, int tj, int K,
                                               double inv_n) {
  const int shift = __builtin_ctz(static_cast<unsigned>(K));
  for (int idx = threadIdx.x; idx < tj * K; idx += kCorThreads) {
    const int64_t j = j0 + (idx >> shift);
    sm_rm[idx] = j < n ? static_cast<float>(rowsum[j * K + (idx & (K - 1))] * inv_n) : 0.f;
  }
}

// sqrt(|xi - xj|^2 + 1e-8) over one slice: xi in registers, xj in LDS
template <int DK>
__device__ __forceinline__ float cor_dist(const float* xi, const float* xj) {
  float d2 = 0.f;
  if constexpr (DK >= 4) {
#pragma unroll
    for (int c = 0; c < DK; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(xj + c);
      const float t0 = xi[c] - v.x, t1 = xi[c + 1] - v.y, t2 = xi[c + 2] - v.z, t3 = xi[c + 3] - v.w;
      d2 = fmaf(t0, t0, d2);
      d2 = fmaf(t1, t1, d2);
      d2 = fmaf(t2, t2, d2);
      d2 = fmaf(t3, t3, d2);
    }
  } else {
    const float2 v = *reinterpret_cast<const float2*>(xj);
    const float t0 = xi[0] - v.x, t1 = xi[1] - v.y;
    d2 = fmaf(t0, t0, d2);
    d2 = fmaf(t1, t1, d2);
  }
  return sqrtf(d2 + 1e-8f);
}

template <int DK, int S>
__device__ __forceinline__ void cor_load_xi(float* xi, const float* __restrict__ x, int64_t ld, int64_t i, int g) {
  constexpr int E = CorShape<DK, S>::E;
  const float* p = x + i * ld + g * E;
#pragma unroll
  for (int e = 0; e < E; ++e) xi[e] = p[e];
}

// ---- forward pass 1: rowsum[i, f] = sum_j d^f_ij -------------------------------------------------------------------
template <int DK, int S>
__global__ __launch_bounds__(kCorThreads) void cor_rowsum_kernel(const float* __restrict__ x, int64_t ld, int64_t n, int D, int K,
                                                                 int G, int spl, int tj, double* __restrict__ rowsum) {
  using Sh = CorShape<DK, S>;
  extern __shared__ float4 cor_lds[];
  float* sm = reinterpret_cast<float*>(cor_lds);
  const CorLane ln(G, spl);
  const int W = G * spl, rs = K * Sh::FS;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * (kCorThreads / W) + ln.rl;
  float xi[Sh::E];
  cor_load_xi<DK, S>(xi, x, ld, i < n ? i : n - 1, ln.g);
  double acc[S];
#pragma unroll
  for (int sl = 0; sl < S; ++sl) acc[sl] = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += tj) {
    __syncthreads();
    cor_load_tile<DK, S>(sm, x, ld, n, j0, tj, D, rs);
    __syncthreads();
    const int tjn = static_cast<int>(n - j0 < tj ? n - j0 : tj);
    for (int jj0 = 0; jj0 < tjn; jj0 += spl) {
      const int jj = jj0 + ln.s;
      const bool valid = jj < tjn;
      const float* xj = sm + (jj < tj ? jj : tj - 1) * rs + ln.g * S * Sh::FS;
#pragma unroll
      for (int sl = 0; sl < S; ++sl) {
        const float d = cor_dist<DK>(xi + sl * DK, xj + sl * Sh::FS);
        acc[sl] += valid ? static_cast<double>(d) : 0.0;
      }
    }
  }
  for (int o = G; o < W; o <<= 1) {
#pragma unroll
    for (int sl = 0; sl < S; ++sl) acc[sl] += __shfl_xor(acc[sl], o);
  }
  if (ln.s == 0 && i < n) {
#pragma unroll
    for (int sl = 0; sl < S; ++sl) rowsum[i * K + ln.g * S + sl] = acc[sl];
  }
}

// ---- out[c] = sum_i in[i, c], one block per column, fixed order ----------------------------------------------------
__global__ __launch_bounds__(kCorThreads) void cor_colsum_kernel(const double* __restrict__ in, int64_t n, int C, double* __restrict__ out) {
  __shared__ double red[kCorThreads];
  const int c = blockIdx.x, t = threadIdx.x;
  double a = 0.0;
  for (int64_t i = t; i < n; i += kCorThreads) a += in[i * C + c];
  red[t] = a;
  __syncthreads();
  for (int o = kCorThreads / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) out[c] = red[0];
}

// ---- forward pass 2: part[i, f] = sum_j A^f_ij A^f_ij, part[i, K + f] = sum_j A^f_ij A^{f+1}_ij ----------------------
template <int DK, int S>
__global__ __launch_bounds__(kCorThreads) void cor_cov_kernel(const float* __restrict__ x, int64_t ld, int64_t n, int D, int K, int G,
                                                              int spl, int tj, const double* __restrict__ rowsum,
                                                              const double* __restrict__ gsum, double* __restrict__ part) {
  using Sh = CorShape<DK, S>;
  extern __shared__ float4 cor_lds[];
  float* sm = reinterpret_cast<float*>(cor_lds);
  const CorLane ln(G, spl);
  const int W = G * spl, rs = K * Sh::FS;
  float* sm_rm = sm + tj * rs;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * (kCorThreads / W) + ln.rl;
  const int64_t ic = i < n ? i : n - 1;
  const double inv_n = 1.0 / static_cast<double>(n);
  float xi[Sh::E];
  cor_load_xi<DK, S>(xi, x, ld, ic, ln.g);
  const int f0 = ln.g * S;
  float rmi[S], gm[S];
  double pff[S], pfg[S];
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    rmi[sl] = static_cast<float>(rowsum[ic * K + f0 + sl] * inv_n);
    gm[sl] = static_cast<float>(gsum[f0 + sl] * inv_n * inv_n);
    pff[sl] = pfg[sl] = 0.0;
  }
  for (int64_t j0 = 0; j0 < n; j0 += tj) {
    __syncthreads();
    cor_load_tile<DK, S>(sm, x, ld, n, j0, tj, D, rs);
    cor_load_means(sm_rm, rowsum, n, j0, tj, K, inv_n);
    __syncthreads();
    const int tjn = static_cast<int>(n - j0 < tj ? n - j0 : tj);
    for (int jj0 = 0; jj0 < tjn; jj0 += spl) {
      const int jj = jj0 + ln.s, jc = jj < tj ? jj : tj - 1;
      const bool valid = jj < tjn;
      const float* xj = sm + jc * rs + f0 * Sh::FS;
      float a[S];
#pragma unroll
      for (int sl = 0; sl < S; ++sl) {
        const float d = cor_dist<DK>(xi + sl * DK, xj + sl * Sh::FS);
        a[sl] = valid ? (d - rmi[sl]) - sm_rm[jc * K + f0 + sl] + gm[sl] : 0.f;
      }
      const float up = __shfl_down(a[0], 1);          // this pair's value in the next lane's first slice
#pragma unroll
      for (int sl = 0; sl < S; ++sl) {
        const float nx = sl + 1 < S ? a[sl + 1 < S ? sl + 1 : sl] : (ln.g + 1 < G ? up : 0.f);
        const double ad = static_cast<double>(a[sl]);
        pff[sl] = fma(ad, ad, pff[sl]);
        pfg[sl] = fma(ad, static_cast<double>(nx), pfg[sl]);
      }
    }
  }
  for (int o = G; o < W; o <<= 1) {
#pragma unroll
    for (int sl = 0; sl < S; ++sl) {
      pff[sl] += __shfl_xor(pff[sl], o);
      pfg[sl] += __shfl_xor(pfg[sl], o);
    }
  }
  if (ln.s == 0 && i < n) {
#pragma unroll
    for (int sl = 0; sl < S; ++sl) {
      part[i * 2 * K + f0 + sl] = pff[sl];
      part[i * 2 * K + K + f0 + sl] = pfg[sl];        // 0 for the last slice
    }
  }
}

// ---- the scalar end of the forward pass: loss and the coefficients of the backward pass ----------------------------
struct CorPair {
  double dcor, g_sxx, g_syy, g_sxy;      // dcor(p, p+1) / Z's numerator and d loss / d (the three sums it reads)
};
// gradient of max(s, 0) as torch.maximum splits a tie
__device__ __forceinline__ double cor_relu_grad(double s) { return s > 0.0 ? 1.0 : (s == 0.0 ? 0.5 : 0.0); }

__device__ CorPair cor_pair(const double* sums, int K, int p, double n2, double Z) {
  const double sxx = sums[p] / n2, syy = sums[p + 1] / n2, sxy = sums[K + p] / n2;
  const double vxx = sqrt(fmax(sxx, 0.0) + 1e-8), vyy = sqrt(fmax(syy, 0.0) + 1e-8), vxy = sqrt(fmax(sxy, 0.0) + 1e-8);
  const double prod = vxx * vyy, root = sqrt(fmax(prod, 0.0)), den = root + 1e-10;
  CorPair r;
  r.dcor = vxy / den;
  const double d_vxy = 1.0 / (den * Z), d_den = -vxy / (den * den * Z);
  const double d_vxx = d_den * vyy / (2.0 * root), d_vyy = d_den * vxx / (2.0 * root);      // prod >= 1e-8 > 0
  r.g_sxy = d_vxy * cor_relu_grad(sxy) / (2.0 * vxy * n2);
  r.g_sxx = d_vxx * cor_relu_grad(sxx) / (2.0 * vxx * n2);
  r.g_syy = d_vyy * cor_relu_grad(syy) / (2.0 * vyy * n2);
  return r;
}

__global__ void cor_finish_kernel(const double* __restrict__ sums, int64_t n, int K, float* __restrict__ loss, float* __restrict__ coef) {
  const int f = threadIdx.x;
  if (f >= K) return;
  const double n2 = static_cast<double>(n) * static_cast<double>(n), Z = (K + 1.0) * K / 2.0;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  if (f > 0) {
    const CorPair lo = cor_pair(sums, K, f - 1, n2, Z);
    c0 = lo.g_sxy;
    c1 += 2.0 * lo.g_syy;
  }
  if (f + 1 < K) {
    const CorPair hi = cor_pair(sums, K, f, n2, Z);
    c2 = hi.g_sxy;
    c1 += 2.0 * hi.g_sxx;
  }
  coef[3 * f] = static_cast<float>(c0);
  coef[3 * f + 1] = static_cast<float>(c1);
  coef[3 * f + 2] = static_cast<float>(c2);
  if (f == 0) {
    double total = 0.0;
    for (int p = 0; p + 1 < K; ++p) total += cor_pair(sums, K, p, n2, Z).dcor;
    loss[0] = static_cast<float>(total / Z);
  }
}

// ---- backward: dX_i = 2 g sum_j (c0 A^{f-1} + c1 A^f + c2 A^{f+1})_ij (x_i - x_j) / d^f_ij ---------------------------
template <int DK, int S>
__global__ __launch_bounds__(kCorThreads) void cor_bwd_kernel(const float* __restrict__ x, int64_t ld, int64_t n, int D, int K, int G,
                                                              int spl, int tj, const double* __restrict__ rowsum,
                                                              const double* __restrict__ gsum, const float* __restrict__ coef,
                                                              const float* __restrict__ gup, float* __restrict__ dx, int64_t lddx) {
  using Sh = CorShape<DK, S>;
  extern __shared__ float4 cor_lds[];
  float* sm = reinterpret_cast<float*>(cor_lds);
  const CorLane ln(G, spl);
  const int W = G * spl, rs = K * Sh::FS;
  float* sm_rm = sm + tj * rs;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * (kCorThreads / W) + ln.rl;
  const int64_t ic = i < n ? i : n - 1;
  const double inv_n = 1.0 / static_cast<double>(n);
  float xi[Sh::E], acc[Sh::E];
  cor_load_xi<DK, S>(xi, x, ld, ic, ln.g);
#pragma unroll
  for (int e = 0; e < Sh::E; ++e) acc[e] = 0.f;
  const int f0 = ln.g * S;
  const float gu = gup[0];
  float rmi[S], gm[S], c0[S], c1[S], c2[S];
#pragma unroll
  for (int sl = 0; sl < S; ++sl) {
    rmi[sl] = static_cast<float>(rowsum[ic * K + f0 + sl] * inv_n);
    gm[sl] = static_cast<float>(gsum[f0 + sl] * inv_n * inv_n);
    c0[sl] = gu * coef[3 * (f0 + sl)];
    c1[sl] = gu * coef[3 * (f0 + sl) + 1];
    c2[sl] = gu * coef[3 * (f0 + sl) + 2];
  }
  for (int64_t j0 = 0; j0 < n; j0 += tj) {
    __syncthreads();
    cor_load_tile<DK, S>(sm, x, ld, n, j0, tj, D, rs);
    cor_load_means(sm_rm, rowsum, n, j0, tj, K, inv_n);
    __syncthreads();
    const int tjn = static_cast<int>(n - j0 < tj ? n - j0 : tj);
    for (int jj0 = 0; jj0 < tjn; jj0 += spl) {
      const int jj = jj0 + ln.s, jc = jj < tj ? jj : tj - 1;
      const bool valid = jj < tjn;
      const float* xj = sm + jc * rs + f0 * Sh::FS;
      float a[S], d[S];
#pragma unroll
      for (int sl = 0; sl < S; ++sl) {
        d[sl] = cor_dist<DK>(xi + sl * DK, xj + sl * Sh::FS);
        a[sl] = valid ? (d[sl] - rmi[sl]) - sm_rm[jc * K + f0 + sl] + gm[sl] : 0.f;
      }
      const float up = __shfl_down(a[0], 1), dn = __shfl_up(a[S - 1], 1);
#pragma unroll
      for (int sl = 0; sl < S; ++sl) {
        const float nx = sl + 1 < S ? a[sl + 1 < S ? sl + 1 : sl] : (ln.g + 1 < G ? up : 0.f);
        const float pv = sl > 0 ? a[sl > 0 ? sl - 1 : 0] : (ln.g > 0 ? dn : 0.f);
        const float q = (c0[sl] * pv + c1[sl] * a[sl] + c2[sl] * nx) / d[sl];      // a = 0 where the pair is not valid
        const float* xs = xj + sl * Sh::FS;
#pragma unroll
        for (int c = 0; c < DK; ++c) acc[sl * DK + c] = fmaf(q, xi[sl * DK + c] - xs[c], acc[sl * DK + c]);
      }
    }
  }
  for (int o = G; o < W; o <<= 1) {
#pragma unroll
    for (int e = 0; e < Sh::E; ++e) acc[e] += __shfl_xor(acc[e], o);
  }
  if (ln.s == 0 && i < n) {
    float* o = dx + i * lddx + ln.g * Sh::E;
#pragma unroll
    for (int e = 0; e < Sh::E; ++e) o[e] = 2.f * acc[e];
  }
}

int cor_plan(int64_t n, int D, int K, CorPlan& p) {
  TAGREC_REQUIRE(n >= 2 && n < (int64_t(1) << 31), "cor: n must be in [2, 2^31)");
  TAGREC_REQUIRE(D == 8 || D == 16 || D == 32 || D == 64 || D == 128 || D == 256, "cor: D must be one of 8 16 32 64 128 256");
  TAGREC_REQUIRE(K >= 2 && D % K == 0 && D / K >= 2, "cor: need 2 <= K, K | D and D / K >= 2");
  p.DK = D / K;
  p.S = K > 64 ? K / 64 : 1;
  p.G = K / p.S;
  const int max_spl = 64 / p.G;
  p.spl = 1;
  // rows of a block = 256 / (G spl): split the j-rows over more lanes until the grid fills the chip
  while (p.spl < max_spl && n * p.G * p.spl / kCorThreads < 1024) p.spl *= 2;
  const int fs = p.DK + (p.DK >= 8 ? 4 : 0);
  const int row = K * fs + K;                       // a tile row and its K row means
  int tj = kCorLdsFloats / row;
  if (tj > 128) tj = 128;
  tj -= tj % p.spl;
  TAGREC_REQUIRE(tj >= p.spl && tj >= 1, "cor: tile does not fit");
  if (tj > n) tj = static_cast<int>((n + p.spl - 1) / p.spl) * p.spl;
  p.tj = tj;
  const int rows = kCorThreads / (p.G * p.spl);
  p.blocks = static_cast<unsigned>((n + rows - 1) / rows);
  p.lds_bytes = static_cast<size_t>(tj) * row * sizeof(float);
  return TAGREC_OK;
}

template <int DK, int S>
int cor_fwd_t(const CorPlan& p, const float* x, int64_t ld, int64_t n, int D, int K, double* rowsum, double* gsum, double* part,
              double* sums, float* loss, float* coef, hipStream_t s) {
  cor_rowsum_kernel<DK, S><<<p.blocks, kCorThreads, p.lds_bytes, s>>>(x, ld, n, D, K, p.G, p.spl, p.tj, rowsum);
  TAGREC_LAUNCH_CHECK();
  cor_colsum_kernel<<<K, kCorThreads, 0, s>>>(rowsum, n, K, gsum);
  TAGREC_LAUNCH_CHECK();
  cor_cov_kernel<DK, S><<<p.blocks, kCorThreads, p.lds_bytes, s>>>(x, ld, n, D, K, p.G, p.spl, p.tj, rowsum, gsum, part);
  TAGREC_LAUNCH_CHECK();
  cor_colsum_kernel<<<2 * K, kCorThreads, 0, s>>>(part, n, 2 * K, sums);
  TAGREC_LAUNCH_CHECK();
  cor_finish_kernel<<<1, 128, 0, s>>>(sums, n, K, loss, coef);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

template <int DK, int S>
int cor_bwd_t(const CorPlan& p, const float* x, int64_t ld, int64_t n, int D, int K, const double* rowsum, const double* gsum,
              const float* coef, const float* g, float* dx, int64_t lddx, hipStream_t s) {
  cor_bwd_kernel<DK, S><<<p.blocks, kCorThreads, p.lds_bytes, s>>>(x, ld, n, D, K, p.G, p.spl, p.tj, rowsum, gsum, coef, g, dx, lddx);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

// one instantiation per slice width; two slices per lane only where K = 128 (dk = 2)
#define TAGREC_COR_DISPATCH(FN, ...)                           \
  switch (p.DK) {                                              \
    case 2: return p.S == 2 ? FN<2, 2>(__VA_ARGS__) : FN<2, 1>(__VA_ARGS__); \
    case 4: return FN<4, 1>(__VA_ARGS__);                      \
    case 8: return FN<8, 1>(__VA_ARGS__);                      \
    case 16: return FN<16, 1>(__VA_ARGS__);                    \
    case 32: return FN<32, 1>(__VA_ARGS__);                    \
    case 64: return FN<64, 1>(__VA_ARGS__);                    \
    case 128: return FN<128, 1>(__VA_ARGS__);                  \
    default: return fail(TAGREC_E_INVALID, "cor: unsupported slice width"); \
  }

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_cor_fwd_f32(const float* X, int64_t ld, int64_t n, int D, int K, double* rowsum, double* gsum, double* part,
                                  double* sums, float* loss, float* coef, void* stream) {
  TAGREC_REQUIRE(X && rowsum && gsum && part && sums && loss && coef, "cor_fwd: null pointer");
  CorPlan p;
  if (int rc = cor_plan(n, D, K, p)) return rc;
  TAGREC_REQUIRE(ld >= D && ld % 4 == 0 && aligned16(X), "cor_fwd: rows must be 16-byte aligned (ld a multiple of 4)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  TAGREC_COR_DISPATCH(cor_fwd_t, p, X, ld, n, D, K, rowsum, gsum, part, sums, loss, coef, s)
}

extern "C" int tagrec_cor_bwd_f32(const float* X, int64_t ld, int64_t n, int D, int K, const double* rowsum, const double* gsum,
                                  const float* coef, const float* g, float* dX, int64_t lddx, void* stream) {
  TAGREC_REQUIRE(X && rowsum && gsum && coef && g && dX, "cor_bwd: null pointer");
  CorPlan p;
  if (int rc = cor_plan(n, D, K, p)) return rc;
  TAGREC_REQUIRE(ld >= D && ld % 4 == 0 && aligned16(X), "cor_bwd: rows must be 16-byte aligned (ld a multiple of 4)");
  TAGREC_REQUIRE(lddx >= D, "cor_bwd: bad output stride");
  hipStream_t s = static_cast<hipStream_t>(stream);
  TAGREC_COR_DISPATCH(cor_bwd_t, p, X, ld, n, D, K, rowsum, gsum, coef, g, dX, lddx, s)
}
