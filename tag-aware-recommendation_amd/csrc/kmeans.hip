// K22: nearest-centroid assignment, the E-step of Lloyd's algorithm (tagrec_kmeans_assign_f32) -- a fused n x K search whose
// distance matrix is never stored.  The fourth client of csrc/pairtile.h: a block OWNS 64 rows of X and WALKS the centroid
// table C in tiles of 64 rows, the score tile comes from the exact-fp32 MFMA (score_tile), and where the softmax of
// csrc/catsoftmax.hip pushes an expf onto a running (maximum, sum) this kernel does a compare-select on a running (best, id).
//
//   s_ij = x_i . c_j - h_j,  h_j = 0.5 |c_j|^2        argmax_j s_ij = the Euclidean nearest centroid (|x_i|^2 is constant per row)
//
//   * h_j is ONE expression for every column (km_half_norm_kernel: an fmaf chain over ascending d from 0, then * 0.5f) and
//     the dot is the MFMA's chain over ascending feature blocks, so two identical centroid rows score bit-identically.
//   * ties go to the LOWER centroid id: a lane meets its columns in ascending order and replaces on a strict > only; the four
//     lanes of a row and nothing else are merged after the walk, by (greater score, or equal score and lower id).
//   * a walked tile's padded rows (j >= K) would score 0 - 0 = 0 and beat every real column of a row whose true scores are
//     all negative: a column past K is never admitted (the `w < a.K` of the select).  Padded feature columns are zero in both
//     tiles and add exact zeros.
//   * the walk is pipelined through registers as the catalogue softmax's: the loads of the NEXT tile (and of its 64 half
//     norms) are issued before the MFMAs of the current one.
//   * no column split: one block walks all of C (L2-resident at the sizes a k-means of node tables uses).  No atomics; every
//     output is a pure function of the operands.
// NaN / Inf operands: the assignment is unspecified but lies in [0, K), and no read leaves the operands.
#include "pairtile.h"

namespace tagrec {
namespace {

constexpr int kNoId = INT32_MAX;          // "no column admitted yet": above every id (K <= 2^31 - 1, ids < K)

struct KmArgs {
  Rows x, c;
  int64_t n, K;
  int D, Dk;                              // Dk = D rounded up to 16 (score loop); the LDS row width Dp = 16 NF >= Dk
  const float* h;                         // [K] half norms
  int64_t* assign;
  float* best;                            // may be null
};

// h[j] = 0.5 |c_j|^2: one thread per centroid, one chain
__global__ __launch_bounds__(kThreads) void km_half_norm_kernel(const float* __restrict__ C, int64_t ldc, int64_t K, int D,
                                                                float* __restrict__ h) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (j >= K) return;
  const float* row = C + j * ldc;
  float s = 0.f;
  for (int d = 0; d < D; ++d) s = fmaf(row[d], row[d], s);
  h[j] = 0.5f * s;
}

// (b, id) <- the better of (b, id) and (b2, id2): the greater score, on equal scores the lower id
__device__ __forceinline__ void km_merge(float& b, int& id, float b2, int id2) {
  if (b2 > b || (b2 == b && id2 < id)) {
    b = b2;
    id = id2;
  }
}

template <int NF>
__global__ __launch_bounds__(kThreads) void km_assign_kernel(KmArgs a) {
  extern __shared__ __align__(16) unsigned char km_smem[];
  constexpr int S = tile_stride(16 * NF);
  float* sh_h = reinterpret_cast<float*>(km_smem);     // half norms of the walked tile's 64 rows
  float* sh_own = sh_h + kTile;
  float* sh_walk = sh_own + kTile * S;

  const PairLane ln = pair_lane();
  const int tid = threadIdx.x, q = ln.q;
  const int64_t own0 = static_cast<int64_t>(blockIdx.x) * kTile;

  f32x4 pre[NF];
  load_tile<NF>(pre, a.x, a.D, own0, a.n);
  store_tile<NF>(sh_own, pre);

  const int64_t o = own0 + 16 * ln.wave + ln.r;        // the owned row whose scores this lane ends up with
  float run_b = kLowest;                               // this lane's columns only
  int run_id = kNoId;

  float hpre = 0.f;
  load_tile<NF>(pre, a.c, a.D, 0, a.K);
  if (tid < kTile) hpre = tid < a.K ? a.h[tid] : 0.f;
  for (int64_t w0 = 0; w0 < a.K; w0 += kTile) {
    __syncthreads();                                   // the previous walked tile has been consumed
    store_tile<NF>(sh_walk, pre);
    if (tid < kTile) sh_h[tid] = hpre;
    __syncthreads();
    if (w0 + kTile < a.K) {                            // in flight under this tile's MFMAs
      load_tile<NF>(pre, a.c, a.D, w0 + kTile, a.K);
      if (tid < kTile) hpre = w0 + kTile + tid < a.K ? a.h[w0 + kTile + tid] : 0.f;
    }

    f32x4 sc[4];
    score_tile(sh_own, sh_walk, S, a.Dk, ln, sc);
    // sc[t][v] = owned row o . walked row w0 + 16 t + 4 q + v: ascending in (t, v), so a strict > keeps the lower id
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 hv = *reinterpret_cast<const f32x4*>(sh_h + 16 * t + 4 * q);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t w = w0 + 16 * t + 4 * q + v;
        const float s = sc[t][v] - hv[v];
        if (w < a.K && s > run_b) {
          run_b = s;
          run_id = static_cast<int>(w);
        }
      }
    }
  }

  // the four lanes of a row (q = 0 .. 3); the rule is symmetric, so every one of them ends with the row's pair
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) km_merge(run_b, run_id, __shfl_xor(run_b, off), __shfl_xor(run_id, off));
  if (o < a.n && q == 0) {
    a.assign[o] = run_id == kNoId ? 0 : run_id;        // no score above the sentinel (NaN / -Inf operands): still inside [0, K)
    if (a.best) a.best[o] = run_b;
  }
}

size_t km_lds_bytes(int Dp) { return kTile * sizeof(float) + tiles_bytes(Dp); }

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_kmeans_assign_f32(const float* X, int64_t ldx, int64_t n, const float* C, int64_t ldc, int64_t K, int D,
                                        float* half_norm, int64_t* assign, float* best, void* stream) {
  const std::string what = "kmeans_assign";
  if (D < 8 || D > 256 || (D & 3) != 0)
    return fail(TAGREC_E_UNSUPPORTED, what + ": D must be a multiple of 4 in 8 .. 256, got " + std::to_string(D));
  if (n < 1 || (n + kTile - 1) / kTile > INT32_MAX)
    return fail(TAGREC_E_UNSUPPORTED, what + ": n must be in 1 .. 64 (2^31 - 1), got " + std::to_string(n));
  if (K < 1 || K > INT32_MAX) return fail(TAGREC_E_UNSUPPORTED, what + ": K must be in 1 .. 2^31 - 1, got " + std::to_string(K));
  if (int rc = check_stride(what, ldx < ldc ? ldx : ldc, D)) return rc;
  TAGREC_REQUIRE(X && C && half_norm && assign, what + ": null pointer");
  KmArgs a = {};
  a.x.X = X; a.x.ld = ldx; a.x.idx = nullptr; a.x.vec = aligned16(X) && (ldx & 3) == 0;
  a.c.X = C; a.c.ld = ldc; a.c.idx = nullptr; a.c.vec = aligned16(C) && (ldc & 3) == 0;
  a.n = n; a.K = K; a.D = D; a.Dk = round16(D);
  a.h = half_norm; a.assign = assign; a.best = best;
  hipStream_t s = static_cast<hipStream_t>(stream);
  km_half_norm_kernel<<<static_cast<unsigned>((K + kThreads - 1) / kThreads), kThreads, 0, s>>>(C, ldc, K, D, half_norm);
  TAGREC_LAUNCH_CHECK();
  const int nf = pick_nf(D);
  const dim3 grid(static_cast<unsigned>((n + kTile - 1) / kTile));
  const size_t lds = km_lds_bytes(16 * nf);
  return dispatch_nf(nf, [&](auto k) {
    constexpr int NF = decltype(k)::value;
    return launch_lds<KmArgs, km_assign_kernel<NF>>(grid, lds, a, s);
  });
}
