// DisenHAN: relation attention over a heterogeneous (user, item, tag) graph (/root/reference/model/disenhan.py:28-97).
//
// Per relation e (row type a, column type b) and routing iteration, the reference gathers [K, E, 2 dk] rows for every
// stored entry to form relu(<[new_a[i]_k, ego_b[j]_k], at[e,k]>).  The attention vector splits into a row half and a
// column half, so the host forms per-node factor scores once (sL[i,k] = <new_a[i]_k, at[e,k,:dk]>, sR[j,k] =
// <ego_b[j]_k, at[e,k,dk:]>, [n, K] each) and an entry here reads K floats of sR[col] instead of 2 D floats:
//     logit(i, j) = m_ij * sum_k r[i,k] relu(sL[i,k] + sR[j,k])      (m_ij: multiplicity of the merged entry -- the
//                                                                      reference's duplicates, summed by coalescing)
//     alpha = softmax over the stored entries of row i                 (torch.sparse.softmax(adj, dim=1), :48-49)
// then (the product A(alpha) ego_b is route_spmm with one weight per entry, routing.hip)
//     Yl = leaky_0.2(Y);  Z_k = Yl_k W;  r[i,:] = softmax_k <tanh(Z_k), q>          (:51-59)
//     new = slice_normalize(ego + r_e1 (.) Z_e1 + r_e2 (.) Z_e2)                     (:62-66)
//
// Layout as in routing.hip: embeddings [n, D] with factor k in columns [k dk, (k+1) dk); per-node per-factor [n, K];
// per-entry [nnz] in CSR entry order.  No float atomics anywhere: every sum has a fixed order, so results (and the
// gradients of the backward passes) are bit-reproducible.
//   edge passes : one wavefront per CSR row (or column of the transposed structure), a lane per entry, K in {1,2,4,8}
//   row passes  : one thread per element of [n, D], 256 / D rows per block; a factor slice's sums are taken by its
//                 first thread from LDS in index order.  W ([dk, dk]) is staged in LDS when dk <= 32.
#include <math.h>

#include <type_traits>

#include "common.h"

namespace tagrec {
namespace {

constexpr int kDhWaves = 4;            // wavefronts per block of the edge passes
constexpr int kDhBlock = 256;          // threads per block of the row passes
constexpr int kDhLdsW = 32 * 32;       // W staged in LDS up to dk = 32

__device__ __forceinline__ float dh_wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ float dh_wave_max(float v) {
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

template <int K>
__device__ __forceinline__ float dh_logit(const float (&l)[K], const float (&rr)[K], const float* __restrict__ s, float m) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) acc = fmaf(rr[k], fmaxf(l[k] + s[k], 0.f), acc);
  return m * acc;
}

// alpha[j] for the entries of row i.  The logits pass through `alpha` (same lane, same entry) and are not kept.
template <int K>
__global__ __launch_bounds__(kDhWaves * kWave) void dh_edge_softmax_fwd_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ mult, int64_t n_rows,
    const float* __restrict__ sL, const float* __restrict__ sR, const float* __restrict__ r, float* __restrict__ alpha) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kDhWaves + (threadIdx.x >> 6);
  if (i >= n_rows) return;
  const int64_t start = rowptr[i], end = rowptr[i + 1];
  if (start == end) return;
  float l[K], rr[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { l[k] = sL[i * K + k]; rr[k] = r[i * K + k]; }
  float mx = -INFINITY;
  for (int64_t j = start + lane; j < end; j += kWave) {
    const float v = dh_logit<K>(l, rr, sR + static_cast<int64_t>(col[j]) * K, mult[j]);
    alpha[j] = v;
    mx = fmaxf(mx, v);
  }
  mx = dh_wave_max(mx);
  float sum = 0.f;
  for (int64_t j = start + lane; j < end; j += kWave) sum += expf(alpha[j] - mx);
  sum = dh_wave_sum(sum);
  for (int64_t j = start + lane; j < end; j += kWave) alpha[j] = expf(alpha[j] - mx) / sum;
}

// Row pass of the backward: dlogit = alpha (dalpha - sum_row alpha dalpha); g[j] = m_j dlogit_j (kept for the column
// pass); dr[i,k] = sum_j g_j relu(sL + sR), dsL[i,k] = sum_j g_j r[i,k] [sL + sR > 0].  Empty rows get zeros.
template <int K>
__global__ __launch_bounds__(kDhWaves * kWave) void dh_edge_softmax_bwd_rows_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ mult, int64_t n_rows,
    const float* __restrict__ sL, const float* __restrict__ sR, const float* __restrict__ r, const float* __restrict__ alpha,
    const float* __restrict__ dalpha, float* __restrict__ g, float* __restrict__ dr, float* __restrict__ dsL) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kDhWaves + (threadIdx.x >> 6);
  if (i >= n_rows) return;
  const int64_t start = rowptr[i], end = rowptr[i + 1];
  float l[K], rr[K], acc_r[K], acc_l[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { l[k] = sL[i * K + k]; rr[k] = r[i * K + k]; acc_r[k] = 0.f; acc_l[k] = 0.f; }
  float dot = 0.f;
  for (int64_t j = start + lane; j < end; j += kWave) dot = fmaf(alpha[j], dalpha[j], dot);
  dot = dh_wave_sum(dot);
  for (int64_t j = start + lane; j < end; j += kWave) {
    const float gj = alpha[j] * (dalpha[j] - dot) * mult[j];
    g[j] = gj;
    const float* __restrict__ s = sR + static_cast<int64_t>(col[j]) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float pre = l[k] + s[k];
      if (pre > 0.f) {
        acc_r[k] = fmaf(gj, pre, acc_r[k]);
        acc_l[k] = fmaf(gj, rr[k], acc_l[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    acc_r[k] = dh_wave_sum(acc_r[k]);
    acc_l[k] = dh_wave_sum(acc_l[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) { dr[i * K + k] = acc_r[k]; dsL[i * K + k] = acc_l[k]; }
  }
}

// Column pass: dsR[c,k] = sum over the entries (i, c) of g_j r[i,k] [sL[i,k] + sR[c,k] > 0], walking the transposed
// structure (rowptr_t / col_t = row ids, perm = the entry's index in the row-major order).
template <int K>
__global__ __launch_bounds__(kDhWaves * kWave) void dh_edge_softmax_bwd_cols_kernel(
    const int64_t* __restrict__ rowptr_t, const int32_t* __restrict__ col_t, const int32_t* __restrict__ perm, int64_t n_cols,
    const float* __restrict__ sL, const float* __restrict__ sR, const float* __restrict__ r, const float* __restrict__ g,
    float* __restrict__ dsR) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t c = static_cast<int64_t>(blockIdx.x) * kDhWaves + (threadIdx.x >> 6);
  if (c >= n_cols) return;
  const int64_t start = rowptr_t[c], end = rowptr_t[c + 1];
  float s[K], acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { s[k] = sR[c * K + k]; acc[k] = 0.f; }
  for (int64_t t = start + lane; t < end; t += kWave) {
    const float gj = g[perm[t]];
    const int64_t i = col_t[t];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (sL[i * K + k] + s[k] > 0.f) acc[k] = fmaf(gj, r[i * K + k], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = dh_wave_sum(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) dsR[c * K + k] = acc[k];
  }
}

// ---- row passes: thread t of a block owns element (row rb, column cc of factor k) of a group of 256 / D rows --------
struct RowSlot {
  int rb, c, k, cc;
};
__device__ __forceinline__ RowSlot dh_slot(int D, int dk) {
  const int t = threadIdx.x;
  return RowSlot{t / D, t % D, (t % D) / dk, (t % D) % dk};
}

// Sum of v over the thread's factor slice, in index order; every thread of the slice gets it.  sv / ss: LDS scratch.
// Starts and ends with a block barrier (all threads of the block must call it).
__device__ __forceinline__ float dh_slice_sum(float v, float* sv, float* ss, const RowSlot& s, int K, int dk) {
  __syncthreads();
  sv[threadIdx.x] = v;
  __syncthreads();
  if (s.cc == 0) {
    float acc = 0.f;
    for (int d = 0; d < dk; ++d) acc += sv[threadIdx.x + d];
    ss[s.rb * K + s.k] = acc;
  }
  __syncthreads();
  return ss[s.rb * K + s.k];
}

// Yl = leaky_0.2(Y);  Z = Yl_k W;  r = softmax_k <tanh(Z_k), q>
__global__ __launch_bounds__(kDhBlock) void dh_rel_epi_fwd_kernel(const float* __restrict__ Y, const float* __restrict__ W,
                                                                  const float* __restrict__ q, int64_t n, int D, int K,
                                                                  float* __restrict__ Yl, float* __restrict__ Z,
                                                                  float* __restrict__ r) {
  __shared__ float sW[kDhLdsW];
  __shared__ float sv[kDhBlock];
  __shared__ float ss[kDhBlock];
  const int dk = D / K;
  const RowSlot s = dh_slot(D, dk);
  const bool lds_w = dk * dk <= kDhLdsW;
  if (lds_w)
    for (int x = threadIdx.x; x < dk * dk; x += kDhBlock) sW[x] = W[x];
  const float* Wp = lds_w ? sW : W;
  const float qc = q[s.cc];
  const int RB = kDhBlock / D;
  const int64_t n_groups = (n + RB - 1) / RB;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int64_t i = grp * RB + s.rb;
    const bool ok = i < n;
    const float y = ok ? Y[i * D + s.c] : 0.f;
    const float yl = y > 0.f ? y : 0.2f * y;
    __syncthreads();                                       // sW staged; the previous group's reads of sv are done
    sv[threadIdx.x] = yl;
    __syncthreads();
    const float* yrow = sv + s.rb * D + s.k * dk;
    float z = 0.f;
    for (int d = 0; d < dk; ++d) z = fmaf(yrow[d], Wp[d * dk + s.cc], z);
    const float th = tanhf(z);
    dh_slice_sum(th * qc, sv, ss, s, K, dk);
    float mx = -INFINITY;
    for (int kk = 0; kk < K; ++kk) mx = fmaxf(mx, ss[s.rb * K + kk]);
    float den = 0.f;
    for (int kk = 0; kk < K; ++kk) den += expf(ss[s.rb * K + kk] - mx);
    const float rk = expf(ss[s.rb * K + s.k] - mx) / den;
    if (ok) {
      Yl[i * D + s.c] = yl;
      Z[i * D + s.c] = z;
      if (s.cc == 0) r[i * K + s.k] = rk;
    }
  }
}

// Backward of the epilogue given dZ (nullable = 0) and dr (nullable = 0):
//   ds_k = r_k (dr_k - sum r dr);  dZt = dZ + ds_k q (1 - tanh(Z)^2);  dY = (dZt_k W^T) * leaky'(Y)
//   dsT = ds_k tanh(Z)  (dq = column sums of dsT viewed [n K, dk]; dW = Yl^T dZt over the same view: host GEMMs)
__global__ __launch_bounds__(kDhBlock) void dh_rel_epi_bwd_kernel(const float* __restrict__ Yl, const float* __restrict__ Z,
                                                                  const float* __restrict__ r, const float* __restrict__ dZ,
                                                                  const float* __restrict__ dr, const float* __restrict__ W,
                                                                  const float* __restrict__ q, int64_t n, int D, int K,
                                                                  float* __restrict__ dY, float* __restrict__ dZt,
                                                                  float* __restrict__ dsT) {
  __shared__ float sW[kDhLdsW];
  __shared__ float sv[kDhBlock];
  const int dk = D / K;
  const RowSlot s = dh_slot(D, dk);
  const bool lds_w = dk * dk <= kDhLdsW;
  if (lds_w)
    for (int x = threadIdx.x; x < dk * dk; x += kDhBlock) sW[x] = W[x];
  const float* Wp = lds_w ? sW : W;
  const float qc = q[s.cc];
  const int RB = kDhBlock / D;
  const int64_t n_groups = (n + RB - 1) / RB;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int64_t i = grp * RB + s.rb;
    const bool ok = i < n;
    float dzt = 0.f, yl = 0.f;
    if (ok) {
      const int64_t e = i * D + s.c;
      const float th = tanhf(Z[e]);
      float dsk = 0.f;
      if (dr) {
        float rd = 0.f;
        for (int kk = 0; kk < K; ++kk) rd = fmaf(r[i * K + kk], dr[i * K + kk], rd);
        dsk = r[i * K + s.k] * (dr[i * K + s.k] - rd);
      }
      dzt = (dZ ? dZ[e] : 0.f) + dsk * qc * (1.f - th * th);
      dZt[e] = dzt;
      dsT[e] = dsk * th;
      yl = Yl[e];
    }
    __syncthreads();                                       // sW staged; the previous group's reads of sv are done
    sv[threadIdx.x] = dzt;
    __syncthreads();
    const float* drow = sv + s.rb * D + s.k * dk;
    float dyl = 0.f;
    for (int c2 = 0; c2 < dk; ++c2) dyl = fmaf(drow[c2], Wp[s.cc * dk + c2], dyl);
    if (ok) dY[i * D + s.c] = yl > 0.f ? dyl : 0.2f * dyl;
  }
}

// x = ego + r1 (.) Z1 + r2 (.) Z2;  y = x / max(||x slice||, 1e-12);  inv[i,k] = 1 / max(||x slice||, 1e-12)
__global__ __launch_bounds__(kDhBlock) void dh_combine_fwd_kernel(const float* __restrict__ ego, const float* __restrict__ Z1,
                                                                  const float* __restrict__ r1, const float* __restrict__ Z2,
                                                                  const float* __restrict__ r2, int64_t n, int D, int K,
                                                                  float* __restrict__ x_out, float* __restrict__ y,
                                                                  float* __restrict__ inv) {
  __shared__ float sv[kDhBlock];
  __shared__ float ss[kDhBlock];
  const int dk = D / K;
  const RowSlot s = dh_slot(D, dk);
  const int RB = kDhBlock / D;
  const int64_t n_groups = (n + RB - 1) / RB;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int64_t i = grp * RB + s.rb;
    const bool ok = i < n;
    float x = 0.f;
    if (ok) {
      const int64_t e = i * D + s.c;
      x = ego[e] + Z1[e] * r1[i * K + s.k];
      x = x + Z2[e] * r2[i * K + s.k];
    }
    const float den = fmaxf(sqrtf(dh_slice_sum(x * x, sv, ss, s, K, dk)), 1e-12f);
    if (ok) {
      x_out[i * D + s.c] = x;
      y[i * D + s.c] = x / den;
      if (s.cc == 0) inv[i * K + s.k] = 1.0f / den;
    }
  }
}

// dx = inv (dy - z (z . dy)), z = x inv (the clamp is constant where ||x|| <= eps);  d ego = dx;
// dZ_e = r_e (.) dx;  dr_e[i,k] = < Z_e[i]_k, dx[i]_k >
__global__ __launch_bounds__(kDhBlock) void dh_combine_bwd_kernel(const float* __restrict__ x, const float* __restrict__ inv,
                                                                  const float* __restrict__ dy, const float* __restrict__ Z1,
                                                                  const float* __restrict__ r1, const float* __restrict__ Z2,
                                                                  const float* __restrict__ r2, int64_t n, int D, int K,
                                                                  float* __restrict__ dx, float* __restrict__ dZ1,
                                                                  float* __restrict__ dZ2, float* __restrict__ dr1,
                                                                  float* __restrict__ dr2) {
  __shared__ float sv[kDhBlock];
  __shared__ float ss[kDhBlock];
  const int dk = D / K;
  const RowSlot s = dh_slot(D, dk);
  const int RB = kDhBlock / D;
  const int64_t n_groups = (n + RB - 1) / RB;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int64_t i = grp * RB + s.rb;
    const bool ok = i < n;
    const int64_t e = i * D + s.c;
    const float iv = ok ? inv[i * K + s.k] : 0.f;
    const float z = ok ? x[e] * iv : 0.f;
    const float g = ok ? dy[e] : 0.f;
    float dot = dh_slice_sum(z * g, sv, ss, s, K, dk);
    if (iv >= 1e12f) dot = 0.f;
    const float d = iv * (g - z * dot);
    const float z1 = ok ? Z1[e] : 0.f, z2 = ok ? Z2[e] : 0.f;
    if (ok) {
      dx[e] = d;
      dZ1[e] = r1[i * K + s.k] * d;
      dZ2[e] = r2[i * K + s.k] * d;
    }
    const float a1 = dh_slice_sum(z1 * d, sv, ss, s, K, dk);
    if (ok && s.cc == 0) dr1[i * K + s.k] = a1;
    const float a2 = dh_slice_sum(z2 * d, sv, ss, s, K, dk);
    if (ok && s.cc == 0) dr2[i * K + s.k] = a2;
  }
}

bool dh_row_shape_ok(int D, int K) {
  return (D == 16 || D == 32 || D == 64 || D == 128 || D == 256) && (K == 1 || K == 2 || K == 4 || K == 8) && D % K == 0;
}

unsigned dh_row_blocks(int64_t n, int D) {
  const int64_t groups = (n + kDhBlock / D - 1) / (kDhBlock / D);
  return static_cast<unsigned>(groups < 4096 ? groups : 4096);
}

template <typename F>
int dh_k_dispatch(int K, const char* who, F&& f) {
  switch (K) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return fail(TAGREC_E_UNSUPPORTED, std::string(who) + ": K must be 1, 2, 4 or 8 (got " + std::to_string(K) + ")");
  }
}

#define DH_ROW_CHECK(who)                                                                                        \
  TAGREC_REQUIRE(n >= 0, who ": negative row count");                                                             \
  if (!dh_row_shape_ok(D, K))                                                                                     \
    return fail(TAGREC_E_UNSUPPORTED, std::string(who ": needs D in {16,32,64,128,256}, K in {1,2,4,8} (got D=") + \
                                          std::to_string(D) + ", K=" + std::to_string(K) + ")");

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_dh_edge_softmax_fwd_f32(const int64_t* rowptr, const int32_t* col, const float* mult, int64_t n_rows,
                                              const float* sL, const float* sR, const float* r, int K, float* alpha,
                                              void* stream) {
  TAGREC_REQUIRE(n_rows >= 0, "dh_edge_softmax_fwd: negative row count");
  if (n_rows == 0) return TAGREC_OK;
  TAGREC_REQUIRE(rowptr && col && mult && sL && sR && r && alpha, "dh_edge_softmax_fwd: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dh_k_dispatch(K, "dh_edge_softmax_fwd", [&](auto kc) {
    constexpr int KK = decltype(kc)::value;
    const unsigned blocks = static_cast<unsigned>((n_rows + kDhWaves - 1) / kDhWaves);
    dh_edge_softmax_fwd_kernel<KK><<<blocks, kDhWaves * kWave, 0, s>>>(rowptr, col, mult, n_rows, sL, sR, r, alpha);
    TAGREC_LAUNCH_CHECK();
    return TAGREC_OK;
  });
}

extern "C" int tagrec_dh_edge_softmax_bwd_f32(const int64_t* rowptr, const int32_t* col, const float* mult, int64_t n_rows,
                                              const int64_t* rowptr_t, const int32_t* col_t, const int32_t* perm,
                                              int64_t n_cols, const float* sL, const float* sR, const float* r, int K,
                                              const float* alpha, const float* dalpha, float* g, float* dr, float* dsL,
                                              float* dsR, void* stream) {
  TAGREC_REQUIRE(n_rows >= 0 && n_cols >= 0, "dh_edge_softmax_bwd: negative size");
  TAGREC_REQUIRE(n_rows == 0 || (rowptr && col && mult && sL && r && alpha && dalpha && g && dr && dsL),
                 "dh_edge_softmax_bwd: null pointer");
  TAGREC_REQUIRE(n_cols == 0 || (rowptr_t && col_t && perm && sR && dsR), "dh_edge_softmax_bwd: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  return dh_k_dispatch(K, "dh_edge_softmax_bwd", [&](auto kc) {
    constexpr int KK = decltype(kc)::value;
    if (n_rows > 0) {
      const unsigned blocks = static_cast<unsigned>((n_rows + kDhWaves - 1) / kDhWaves);
      dh_edge_softmax_bwd_rows_kernel<KK><<<blocks, kDhWaves * kWave, 0, s>>>(rowptr, col, mult, n_rows, sL, sR, r, alpha,
                                                                               dalpha, g, dr, dsL);
      TAGREC_LAUNCH_CHECK();
    }
    if (n_cols > 0) {
      const unsigned blocks = static_cast<unsigned>((n_cols + kDhWaves - 1) / kDhWaves);
      dh_edge_softmax_bwd_cols_kernel<KK><<<blocks, kDhWaves * kWave, 0, s>>>(rowptr_t, col_t, perm, n_cols, sL, sR, r, g, dsR);
      TAGREC_LAUNCH_CHECK();
    }
    return TAGREC_OK;
  });
}

extern "C" int tagrec_dh_rel_epi_fwd_f32(const float* Y, const float* W, const float* q, int64_t n, int D, int K, float* Yl,
                                         float* Z, float* r, void* stream) {
  DH_ROW_CHECK("dh_rel_epi_fwd");
  if (n == 0) return TAGREC_OK;
  TAGREC_REQUIRE(Y && W && q && Yl && Z && r, "dh_rel_epi_fwd: null pointer");
  dh_rel_epi_fwd_kernel<<<dh_row_blocks(n, D), kDhBlock, 0, static_cast<hipStream_t>(stream)>>>(Y, W, q, n, D, K, Yl, Z, r);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_dh_rel_epi_bwd_f32(const float* Yl, const float* Z, const float* r, const float* dZ, const float* dr,
                                         const float* W, const float* q, int64_t n, int D, int K, float* dY, float* dZt,
                                         float* dsT, void* stream) {
  DH_ROW_CHECK("dh_rel_epi_bwd");
  if (n == 0) return TAGREC_OK;
  TAGREC_REQUIRE(Yl && Z && r && W && q && dY && dZt && dsT, "dh_rel_epi_bwd: null pointer");
  dh_rel_epi_bwd_kernel<<<dh_row_blocks(n, D), kDhBlock, 0, static_cast<hipStream_t>(stream)>>>(Yl, Z, r, dZ, dr, W, q, n, D, K,
                                                                                                dY, dZt, dsT);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_dh_combine_fwd_f32(const float* ego, const float* Z1, const float* r1, const float* Z2, const float* r2,
                                         int64_t n, int D, int K, float* x, float* y, float* inv, void* stream) {
  DH_ROW_CHECK("dh_combine_fwd");
  if (n == 0) return TAGREC_OK;
  TAGREC_REQUIRE(ego && Z1 && r1 && Z2 && r2 && x && y && inv, "dh_combine_fwd: null pointer");
  dh_combine_fwd_kernel<<<dh_row_blocks(n, D), kDhBlock, 0, static_cast<hipStream_t>(stream)>>>(ego, Z1, r1, Z2, r2, n, D, K, x,
                                                                                                y, inv);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_dh_combine_bwd_f32(const float* x, const float* inv, const float* dy, const float* Z1, const float* r1,
                                         const float* Z2, const float* r2, int64_t n, int D, int K, float* dx, float* dZ1,
                                         float* dZ2, float* dr1, float* dr2, void* stream) {
  DH_ROW_CHECK("dh_combine_bwd");
  if (n == 0) return TAGREC_OK;
  TAGREC_REQUIRE(x && inv && dy && Z1 && r1 && Z2 && r2 && dx && dZ1 && dZ2 && dr1 && dr2, "dh_combine_bwd: null pointer");
  dh_combine_bwd_kernel<<<dh_row_blocks(n, D), kDhBlock, 0, static_cast<hipStream_t>(stream)>>>(x, inv, dy, Z1, r1, Z2, r2, n, D,
                                                                                                K, dx, dZ1, dZ2, dr1, dr2);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}
