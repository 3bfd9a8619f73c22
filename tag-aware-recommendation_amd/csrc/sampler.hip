// Negative sampler with a choice of proposal and of candidates per entry (tagrec_sample_negative_ex_i64).
//
// The reference draws one uniform non-positive item per train edge (train_data/utils.py:19-28) and nothing else; the
// uniform kernel of rowops.hip restates that.  Here the same counter-based stream is extended in two directions:
//   proposal   uniform, or an alias table (Vose) over the right ids -- one more hash and two table reads per try;
//   candidates n_cand draws per entry (with replacement), of which the one the tables score highest is kept:
//              score_c = U[left[e]] . I[cand_c] in fp32, first arg-max in c order ("dynamic" hard negatives).
// Candidate c of entry e is a pure function of (seed, e, c) and candidate 0 under the uniform proposal is the draw of
// sample_negative_kernel, so n_cand = 1 reproduces the old stream.  Nothing is sorted or stored, no LDS, no atomics.
#include "common.h"

namespace tagrec {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxCand = 16;
constexpr uint32_t kMaxTries = 4096u;

__device__ __forceinline__ uint64_t cand_base(uint64_t base0, int c) {
  return c == 0 ? base0 : mix64(base0 + (static_cast<uint64_t>(c) << 32));
}

// The rejection loop of sample_negative_kernel on the stream that starts at `base`: at most 4096 tries, the last one is
// kept.  ALIAS: try t reads two words -- a column j of the alias table and a 24-bit uniform u; the draw is j if
// u < prob[j], else alias[j].
template <bool ALIAS>
__device__ __forceinline__ int64_t draw_negative(uint64_t base, int64_t lo0, int64_t hi0, const int32_t* __restrict__ cols,
                                                 uint64_t n_right, const float* __restrict__ prob,
                                                 const int32_t* __restrict__ alias) {
  int64_t draw = 0;
  for (uint32_t t = 0; t < kMaxTries; ++t) {
    if (ALIAS) {
      const uint64_t j = __umul64hi(mix64(base + 2ull * t), n_right);
      const float u = static_cast<float>(static_cast<uint32_t>(mix64(base + 2ull * t + 1ull) >> 40)) * 0x1p-24f;
      draw = u < prob[j] ? static_cast<int64_t>(j) : static_cast<int64_t>(alias[j]);
    } else {
      draw = static_cast<int64_t>(__umul64hi(mix64(base + t), n_right));
    }
    int64_t lo = lo0, hi = hi0;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cols[mid] < draw) lo = mid + 1; else hi = mid;
    }
    if (lo == hi0 || cols[lo] != draw) break;
  }
  return draw;
}

// n_cand == 1: one thread per entry, as sample_negative_kernel; no table is read.
template <bool ALIAS>
__global__ __launch_bounds__(kThreads) void sample_one_kernel(const int64_t* __restrict__ left, int64_t n_rows,
                                                              const int64_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ cols, uint64_t n_right, uint64_t seed,
                                                              const float* __restrict__ prob, const int32_t* __restrict__ alias,
                                                              int64_t* __restrict__ neg, int64_t* __restrict__ cand_out) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (e >= n_rows) return;
  const int64_t l = left[e];
  const uint64_t base = mix64(seed ^ mix64(static_cast<uint64_t>(e)));
  const int64_t draw = draw_negative<ALIAS>(base, rowptr[l], rowptr[l + 1], cols, n_right, prob, alias);
  neg[e] = draw;
  if (cand_out) cand_out[e] = draw;
}

__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
  return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, fmaf(a.w, b.w, acc))));
}

// n_cand > 1: a group of LPR lanes owns one entry (64 / LPR entries per wavefront).  Lane c of the group draws candidate c
// (with LPR < n_cand, also c + LPR, ...), so the rejection loops of an entry's candidates run side by side; the ids are
// then handed round the group.  Each lane reads one float4 per row per pass (PASSES = ceil(D / 4 / LPR) > 1 only for rows
// wider than 256 floats), the user row once.  The candidate rows of a chunk are all requested before the first is
// reduced: a group otherwise walks a chain of dependent latencies.  The xor butterfly leaves the same bits in every lane
// of the group, so the lanes agree on the winner without a broadcast.
template <int LPR, int PASSES>
__global__ __launch_bounds__(kThreads) void sample_hard_kernel(const int64_t* __restrict__ left, int64_t n_rows,
                                                               const int64_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ cols, uint64_t n_right, uint64_t seed,
                                                               int n_cand, const float* __restrict__ prob,
                                                               const int32_t* __restrict__ alias, const float4* __restrict__ U,
                                                               int64_t ldu4, const float4* __restrict__ I, int64_t ldi4, int D4,
                                                               int64_t* __restrict__ neg, int64_t* __restrict__ cand_out,
                                                               float* __restrict__ score_out) {
  constexpr int NPI = kWave / LPR;                          // entries per wavefront
  constexpr int SLOTS = (kMaxCand + LPR - 1) / LPR;         // candidates a lane may have to draw
  constexpr int CH = PASSES == 1 ? 8 : 4;                   // candidate rows in flight per group
  const int lane = threadIdx.x & (kWave - 1);
  const int grp = lane / LPR, c4 = lane % LPR;
  const int64_t e = (static_cast<int64_t>(blockIdx.x) * (kThreads / kWave) + (threadIdx.x >> 6)) * NPI + grp;
  const bool ok = e < n_rows;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  int64_t l = 0;
  int64_t mine[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) mine[s] = 0;
  if (ok) {
    l = left[e];
    const int64_t lo0 = rowptr[l], hi0 = rowptr[l + 1];
    const uint64_t base0 = mix64(seed ^ mix64(static_cast<uint64_t>(e)));
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c = c4 + s * LPR;
      if (c < n_cand) {
        const uint64_t base = cand_base(base0, c);
        mine[s] = prob ? draw_negative<true>(base, lo0, hi0, cols, n_right, prob, alias)
                       : draw_negative<false>(base, lo0, hi0, cols, n_right, prob, alias);
        if (cand_out) cand_out[e * n_cand + c] = mine[s];
      }
    }
  }

  float4 ur[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int k = c4 + p * LPR;
    ur[p] = (ok && k < D4) ? U[l * ldu4 + k] : zero4;
  }

  float best = 0.f;
  int64_t pick = 0;
  for (int c0 = 0; c0 < n_cand; c0 += CH) {
    int64_t cand[CH];
    float4 x[CH][PASSES];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int c = c0 + u;                                 // (wave-uniform; c < kMaxCand + CH)
      int64_t v = mine[0];
#pragma unroll
      for (int s = 1; s < SLOTS; ++s) v = (c / LPR == s) ? mine[s] : v;
      cand[u] = __shfl(v, grp * LPR + (c & (LPR - 1)));
      const bool in = ok && c < n_cand;
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        const int k = c4 + p * LPR;
        x[u][p] = (in && k < D4) ? I[cand[u] * ldi4 + k] : zero4;
      }
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int c = c0 + u;
      if (c < n_cand) {                                     // (wave-uniform)
        float s = 0.f;
#pragma unroll
        for (int p = 0; p < PASSES; ++p) s = dot4(ur[p], x[u][p], s);
#pragma unroll
        for (int m = 1; m < LPR; m <<= 1) s += __shfl_xor(s, m);
        // first arg-max: a later candidate wins only with a strictly greater score, so ties keep the lowest c and a NaN
        // never replaces an earlier candidate (nor is a NaN of candidate 0 ever replaced)
        if (c == 0 || s > best) { best = s; pick = cand[u]; }
        if (score_out && ok && c4 == 0) score_out[e * n_cand + c] = s;
      }
    }
  }
  if (ok && c4 == 0) neg[e] = pick;
}

template <int LPR, int PASSES>
void launch_hard(const int64_t* left, int64_t n_rows, const int64_t* rowptr, const int32_t* cols, int64_t n_right, uint64_t seed,
                 int n_cand, const float* prob, const int32_t* alias, const float* U, int64_t ld_u, const float* I, int64_t ld_i,
                 int D, int64_t* neg, int64_t* cand_out, float* score_out, hipStream_t st) {
  const int64_t per_block = (kThreads / kWave) * (kWave / LPR);
  sample_hard_kernel<LPR, PASSES><<<static_cast<unsigned>((n_rows + per_block - 1) / per_block), kThreads, 0, st>>>(
      left, n_rows, rowptr, cols, static_cast<uint64_t>(n_right), seed, n_cand, prob, alias, reinterpret_cast<const float4*>(U),
      ld_u / 4, reinterpret_cast<const float4*>(I), ld_i / 4, D / 4, neg, cand_out, score_out);
}

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_sample_negative_ex_i64(const int64_t* left, int64_t n_rows, const int64_t* rowptr, const int32_t* cols,
                                             int64_t n_left, int64_t n_right, uint64_t seed, int n_cand, const float* alias_prob,
                                             const int32_t* alias_idx, const float* U, int64_t ld_u, const float* I, int64_t ld_i,
                                             int D, int64_t* neg, int64_t* cand_out, float* score_out, void* stream) {
  TAGREC_REQUIRE(left && rowptr && neg && (cols || n_rows == 0), "sample_negative_ex: null pointer");
  TAGREC_REQUIRE(n_rows >= 0 && n_left >= 1 && n_right >= 1, "sample_negative_ex: bad shape");
  TAGREC_REQUIRE(n_cand >= 1 && n_cand <= kMaxCand, "sample_negative_ex: n_cand must be in 1 .. 16");
  TAGREC_REQUIRE((alias_prob == nullptr) == (alias_idx == nullptr), "sample_negative_ex: alias_prob / alias_idx must both be given or both null");
  TAGREC_REQUIRE(!alias_prob || n_right <= 0x7fffffff, "sample_negative_ex: an alias table holds int32 ids");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_cand == 1) {
    TAGREC_REQUIRE(!score_out, "sample_negative_ex: n_cand = 1 scores nothing (score_out must be null)");
    if (n_rows == 0) return TAGREC_OK;
    const unsigned blocks = static_cast<unsigned>((n_rows + kThreads - 1) / kThreads);
    if (alias_prob)
      sample_one_kernel<true><<<blocks, kThreads, 0, st>>>(left, n_rows, rowptr, cols, static_cast<uint64_t>(n_right), seed,
                                                           alias_prob, alias_idx, neg, cand_out);
    else
      sample_one_kernel<false><<<blocks, kThreads, 0, st>>>(left, n_rows, rowptr, cols, static_cast<uint64_t>(n_right), seed,
                                                            nullptr, nullptr, neg, cand_out);
    TAGREC_LAUNCH_CHECK();
    return TAGREC_OK;
  }
  TAGREC_REQUIRE(U && I, "sample_negative_ex: n_cand > 1 needs the two scoring tables");
  TAGREC_REQUIRE(D % 4 == 0 && D >= 8 && D <= 1024, "sample_negative_ex: D must be a multiple of 4 in 8 .. 1024");
  TAGREC_REQUIRE(ld_u % 4 == 0 && ld_i % 4 == 0 && ld_u >= D && ld_i >= D, "sample_negative_ex: row strides must be multiples of 4, >= D");
  TAGREC_REQUIRE(aligned16(U) && aligned16(I), "sample_negative_ex: 16-byte aligned tables expected");
  if (n_rows == 0) return TAGREC_OK;
#define TAGREC_HARD(LPR, PASSES) \
  launch_hard<LPR, PASSES>(left, n_rows, rowptr, cols, n_right, seed, n_cand, alias_prob, alias_idx, U, ld_u, I, ld_i, D, neg, \
                           cand_out, score_out, st)
  const int d4 = D / 4;                 // group = smallest power of two >= D / 4, capped at the wavefront
  if (d4 <= 2) TAGREC_HARD(2, 1);
  else if (d4 <= 4) TAGREC_HARD(4, 1);
  else if (d4 <= 8) TAGREC_HARD(8, 1);
  else if (d4 <= 16) TAGREC_HARD(16, 1);
  else if (d4 <= 32) TAGREC_HARD(32, 1);
  else if (d4 <= 64) TAGREC_HARD(64, 1);
  else if (d4 <= 128) TAGREC_HARD(64, 2);
  else if (d4 <= 192) TAGREC_HARD(64, 3);
  else TAGREC_HARD(64, 4);
#undef TAGREC_HARD
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}
