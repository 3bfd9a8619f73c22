// N1: evaluation scoring -> train-item mask -> top-K, fused (one pass over the item table per block of users).
//
// Replaces, per 512-user batch of `epoch_test` (/root/reference/training/basic_test.py:36-50):
//     rating = sigmoid(U_b I^T)        model/lightgcn.py:84-89 (predict_rating)
//     rating[train positives] = -1024  basic_test.py:42-47
//     _, top = torch.topk(rating, k)   basic_test.py:48
// The reference materialises the [512, n_item] rating matrix; here scores live in MFMA accumulators: a wave
// keeps 16 users' embeddings in registers (B-operand), streams 16-item tiles of the item table as A-operand
// (exact-fp32 MFMA 16x16x4, D/4 per tile), and keeps each user's running top-K in LDS.  A score is looked at
// again only if it beats the user's current K-th best (about K ln(n_item / K) times per user), and only then is
// the train-item mask consulted (binary search in the user's sorted train list), so the mask costs nothing per
// score.  Ranking uses the sigmoid value, as the reference does (fp32 sigmoid saturates for scores >~ 17, which
// creates ties there too); ties resolve to the lower item id.
#include <math.h>

#include "common.h"

namespace tagrec {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kEvalThreads = 256;                 // 4 waves x 16 users
constexpr int kEvalUsers = 64;
constexpr int kMaxTopK = 64;

template <int D>
__global__ __launch_bounds__(kEvalThreads) void eval_topk_kernel(const float* __restrict__ U, const float* __restrict__ I,
                                                                 int64_t n_item, const int64_t* __restrict__ users,
                                                                 int64_t n_users, const int64_t* __restrict__ train_ptr,
                                                                 const int32_t* __restrict__ train_items, int K,
                                                                 int64_t* __restrict__ top_idx, float* __restrict__ top_val) {
  constexpr int DS = D / 4;                        // the lane's quarter of an embedding row
  extern __shared__ float lds[];                   // [64][K] scores, then [64][K] item ids
  float* sh_sc = lds;
  int* sh_id = reinterpret_cast<int*>(lds + kEvalUsers * K);
  for (int i = threadIdx.x; i < kEvalUsers * K; i += kEvalThreads) { sh_sc[i] = -INFINITY; sh_id[i] = -1; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int uslot = wave * 16 + r;
  const int64_t upos = static_cast<int64_t>(blockIdx.x) * kEvalUsers + uslot;
  const bool uok = upos < n_users;
  const int64_t user = uok ? users[upos] : 0;
  float ub[DS];
#pragma unroll
  for (int s = 0; s < DS; s += 4) {
    const float4 t = uok ? *reinterpret_cast<const float4*>(U + user * D + q * DS + s) : make_float4(0.f, 0.f, 0.f, 0.f);
    ub[s] = t.x; ub[s + 1] = t.y; ub[s + 2] = t.z; ub[s + 3] = t.w;
  }
  const int64_t tlo = uok ? train_ptr[user] : 0, thi = uok ? train_ptr[user + 1] : 0;
  // The four lanes q = 0..3 of a user slot share its list and take turns (wave_barrier below).  That intrinsic orders
  // execution, not memory, so the list is accessed through volatile pointers: every threshold read and every insertion
  // goes to LDS and sees what the previous lane wrote.
  volatile float* my_sc = sh_sc + uslot * K;
  volatile int* my_id = sh_id + uslot * K;
  for (int64_t item0 = 0; item0 < n_item; item0 += 16) {
    // A-operand: row m = r is item item0 + r; k-slot q covers features q*DS .. q*DS+DS-1 (same split as ub)
    const int64_t it = item0 + r;
    float a[DS];
#pragma unroll
    for (int s = 0; s < DS; s += 4) {
      const float4 t = it < n_item ? *reinterpret_cast<const float4*>(I + it * D + q * DS + s) : make_float4(0.f, 0.f, 0.f, 0.f);
      a[s] = t.x; a[s + 1] = t.y; a[s + 2] = t.z; a[s + 3] = t.w;
    }
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < DS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], ub[s], acc, 0, 0, 0);
    // acc[v] = score of (user slot r, item item0 + 4 q + v)
    float sg[4];
    bool cand = false;
    const float thr = my_sc[K - 1];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      sg[v] = 1.0f / (1.0f + expf(-acc[v]));
      cand |= uok && (item0 + 4 * q + v < n_item) && sg[v] > thr;
    }
    if (__any(cand)) {
      // serialise the (rare) insertions: one k-slot and one register at a time, so a user's list has one writer
      for (int qq = 0; qq < 4; ++qq) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int64_t item = item0 + 4 * q + v;
          if (q == qq && uok && item < n_item && sg[v] > my_sc[K - 1]) {
            // train positives are masked out (basic_test.py:47): binary search in the user's sorted train list
            int64_t lo = tlo, hi = thi;
            while (lo < hi) {
              const int64_t mid = (lo + hi) >> 1;
              if (train_items[mid] < item) lo = mid + 1; else hi = mid;
            }
            if (!(lo < thi && train_items[lo] == item)) {
              int p = K - 1;
              while (p > 0 && my_sc[p - 1] < sg[v]) {
                const float ps = my_sc[p - 1];
                const int pi = my_id[p - 1];
                my_sc[p] = ps;
                my_id[p] = pi;
                --p;
              }
              my_sc[p] = sg[v];
              my_id[p] = static_cast<int>(item);
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
  }
  __syncthreads();
  if (uok && q == 0) {
    for (int p = 0; p < K; ++p) {
      top_idx[upos * K + p] = my_id[p];
      if (top_val) top_val[upos * K + p] = my_sc[p];
    }
  }
}


// N1 + AUC: the same pass, plus each user's AUC over its un-masked items (basic_test.py:53,73 -> utils.auc, sklearn's
// roc_auc_score on the masked rating row) as the Mann-Whitney pair count
//     auc_num2 = sum over valid positives p and valid negatives x of 2 [s_p > s_x] + [s_p == s_x],
// so AUC = auc_num2 / (2 n_pos n_neg) stays an integer until the host divides.  valid = not a train id; positives =
// unique test ids that are valid; negatives = the other valid items.
//   1. Lane q = 0 of a user slot walks the user's sorted test list against its sorted train list (a merge, skipping
//      duplicates) and writes up to kAucPosCap valid positive ids into LDS.
//   2. The wave scores them in 16-row tiles with the SAME MFMA sequence and k-slot split as the item stream (row m of a
//      tile is one positive, column n = r its user), so s_p is bit-identical to the score the stream computes for that
//      item; the owning user's column is kept and the list sorted ascending in place.
//   3. The item stream: every lane sees its items in increasing id order, so one cursor into the train list and one
//      into the test list mark which of its four items in a tile are "masked" / "positive" (one compare per tile).
//      For a valid negative two binary searches over the sorted positive scores give 2 #(s_p > s_x) + #(s_p == s_x)
//      (the second search only on a tie).
// A user with more than kAucPosCap valid positives makes its block repeat steps 1-3 over the next chunk of positives
// (the counts add up; top-K and n_neg come from the first pass).
constexpr int kAucPosSlot = 128;                  // 64 users x 128 scores = 32 KB beside the top-K lists
constexpr int kAucPosCap = kAucPosSlot - 1;       // positives per pass; the slot's tail is +inf padding
constexpr int kAucPosStride = kAucPosSlot + 1;    // slots 129 floats apart: entry i of the wave's 16 users in 16 banks

template <int D>
__global__ __launch_bounds__(kEvalThreads) void eval_topk_auc_kernel(
    const float* __restrict__ U, const float* __restrict__ I, int64_t n_item, const int64_t* __restrict__ users,
    int64_t n_users, const int64_t* __restrict__ train_ptr, const int32_t* __restrict__ train_items,
    const int64_t* __restrict__ test_ptr, const int32_t* __restrict__ test_items, int K, int64_t* __restrict__ top_idx,
    float* __restrict__ top_val, int64_t* __restrict__ auc_num2, int64_t* __restrict__ n_pos,
    int64_t* __restrict__ n_neg) {
  constexpr int DS = D / 4;
  extern __shared__ float lds[];                   // [64][K] scores, [64][K] ids, [64][129] positives, [64] counts, passes
  float* sh_sc = lds;
  int* sh_id = reinterpret_cast<int*>(lds + kEvalUsers * K);
  float* sh_pos = lds + 2 * kEvalUsers * K;        // a positive's item id (as float bits) until it is replaced by its score
  int* sh_cnt = reinterpret_cast<int*>(sh_pos + kEvalUsers * kAucPosStride);
  int* sh_pass = sh_cnt + kEvalUsers;
  for (int i = threadIdx.x; i < kEvalUsers * K; i += kEvalThreads) { sh_sc[i] = -INFINITY; sh_id[i] = -1; }
  if (threadIdx.x == 0) *sh_pass = 1;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int uslot = wave * 16 + r;
  const int64_t upos = static_cast<int64_t>(blockIdx.x) * kEvalUsers + uslot;
  const bool uok = upos < n_users;
  const int64_t user = uok ? users[upos] : 0;
  float ub[DS];
#pragma unroll
  for (int s = 0; s < DS; s += 4) {
    const float4 t = uok ? *reinterpret_cast<const float4*>(U + user * D + q * DS + s) : make_float4(0.f, 0.f, 0.f, 0.f);
    ub[s] = t.x; ub[s + 1] = t.y; ub[s + 2] = t.z; ub[s + 3] = t.w;
  }
  const int64_t tlo = uok ? train_ptr[user] : 0, thi = uok ? train_ptr[user + 1] : 0;
  const int64_t slo = uok ? test_ptr[user] : 0, shi = uok ? test_ptr[user + 1] : 0;
  volatile float* my_sc = sh_sc + uslot * K;
  volatile int* my_id = sh_id + uslot * K;
  float* my_pos = sh_pos + uslot * kAucPosStride;
  int64_t npos = 0, num2 = 0;                      // npos: lane q = 0; nneg / num2: this lane's share
  int nneg = 0;
  int passes = 1;
  for (int pass = 0; pass < passes; ++pass) {
    // 1. valid positives [pass * cap, pass * cap + cap) of this user, in increasing id order
    if (q == 0) {
      int64_t np = 0, tc = tlo;
      const int64_t first = static_cast<int64_t>(pass) * kAucPosCap;
      int32_t prev = -1;
      for (int64_t e = slo; e < shi; ++e) {
        const int32_t x = test_items[e];
        if (x <= prev || x >= n_item) continue;    // duplicates (and ids outside the table)
        prev = x;
        while (tc < thi && train_items[tc] < x) ++tc;
        if (tc < thi && train_items[tc] == x) continue;
        if (np >= first && np < first + kAucPosCap) my_pos[np - first] = __int_as_float(x);
        ++np;
      }
      if (pass == 0) {
        npos = np;
        if (np > kAucPosCap) atomicMax(sh_pass, static_cast<int>((np + kAucPosCap - 1) / kAucPosCap));
      }
      const int64_t left = np - first;
      sh_cnt[uslot] = static_cast<int>(left < 0 ? 0 : (left > kAucPosCap ? kAucPosCap : left));
    }
    __syncthreads();
    passes = *sh_pass;
    // 2. score them with the stream's arithmetic: tile row m = positive t0 + m of user slot j, B-operand as in the stream
    for (int j = 0; j < 16; ++j) {
      const int cnt = sh_cnt[wave * 16 + j];
      float* pj = sh_pos + (wave * 16 + j) * kAucPosStride;
      for (int t0 = 0; t0 < cnt; t0 += 16) {
        const int64_t it = t0 + r < cnt ? static_cast<int64_t>(__float_as_int(pj[t0 + r])) : -1;
        float a[DS];
#pragma unroll
        for (int s = 0; s < DS; s += 4) {
          const float4 t = it >= 0 ? *reinterpret_cast<const float4*>(I + it * D + q * DS + s) : make_float4(0.f, 0.f, 0.f, 0.f);
          a[s] = t.x; a[s + 1] = t.y; a[s + 2] = t.z; a[s + 3] = t.w;
        }
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < DS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], ub[s], acc, 0, 0, 0);
        // acc[v] = score of (user slot r, positive t0 + 4 q + v); the ids of this tile were read before the MFMA
        if (r == j) {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (t0 + 4 * q + v < cnt) pj[t0 + 4 * q + v] = 1.0f / (1.0f + expf(-acc[v]));
        }
      }
    }
    __syncthreads();
    const int cnt = sh_cnt[uslot];
    if (q == 0) {                                  // insertion sort, ascending
      for (int i = 1; i < cnt; ++i) {
        const float x = my_pos[i];
        int p = i;
        while (p > 0 && my_pos[p - 1] > x) { my_pos[p] = my_pos[p - 1]; --p; }
        my_pos[p] = x;
      }
      for (int i = cnt; i < kAucPosSlot; ++i) my_pos[i] = INFINITY;   // the searches below need no bounds check
    }
    __syncthreads();
    // 3. the item stream; binary searches start at the largest power of two <= the wave's longest positive list
    int wmax = 0;
    for (int j = 0; j < 16; ++j) wmax = max(wmax, sh_cnt[wave * 16 + j]);
    const int top = wmax > 0 ? 1 << (31 - __clz(wmax)) : 0;
    const bool first = pass == 0;
    int64_t tc = tlo, sc = slo;
    int64_t tv = tc < thi ? train_items[tc] : INT64_MAX;
    int64_t sv = sc < shi ? test_items[sc] : INT64_MAX;
    for (int64_t item0 = 0; item0 < n_item; item0 += 16) {
      const int64_t it = item0 + r;
      float a[DS];
#pragma unroll
      for (int s = 0; s < DS; s += 4) {
        const float4 t = it < n_item ? *reinterpret_cast<const float4*>(I + it * D + q * DS + s) : make_float4(0.f, 0.f, 0.f, 0.f);
        a[s] = t.x; a[s + 1] = t.y; a[s + 2] = t.z; a[s + 3] = t.w;
      }
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < DS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], ub[s], acc, 0, 0, 0);
      // acc[v] = score of (user slot r, item item0 + 4 q + v)
      // the lane's four items base .. base + 3: which of them are train ids / test ids, one cursor step per list entry
      const int64_t base = item0 + 4 * q;
      unsigned tmask = 0, smask = 0;
      if (uok && base < n_item) {
        while (tv < base + 4) {
          if (tv >= base) tmask |= 1u << (tv - base);
          ++tc;
          tv = tc < thi ? train_items[tc] : INT64_MAX;
        }
        while (sv < base + 4) {
          if (sv >= base) smask |= 1u << (sv - base);
          ++sc;
          sv = sc < shi ? test_items[sc] : INT64_MAX;
        }
      }
      float sg[4];
      bool ok[4], neg[4];
      bool cand = false;
      const float thr = my_sc[K - 1];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        sg[v] = 1.0f / (1.0f + expf(-acc[v]));
        ok[v] = uok && base + v < n_item && !((tmask >> v) & 1u);   // train positives are masked out (basic_test.py:47)
        neg[v] = ok[v] && !((smask >> v) & 1u);                     // a valid negative
        cand |= ok[v] && sg[v] > thr;
        nneg += first && neg[v];
      }
      if (cnt > 0) {
        // #(s_p <= s_x) for the four scores at once (independent LDS reads; the +inf padding keeps every probe in the
        // slot and never counts), then #(s_p < s_x) only on a tie
        int le[4] = {0, 0, 0, 0};
        for (int step = top; step > 0; step >>= 1) {
#pragma unroll
          for (int v = 0; v < 4; ++v)
            if (my_pos[le[v] + step - 1] <= sg[v]) le[v] += step;
        }
        int tile2 = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if (!neg[v]) continue;
          int lt = le[v];
          if (le[v] > 0 && my_pos[le[v] - 1] == sg[v]) {
            lt = 0;
            for (int step = top; step > 0; step >>= 1)
              if (my_pos[lt + step - 1] < sg[v]) lt += step;
          }
          tile2 += 2 * (cnt - le[v]) + (le[v] - lt);
        }
        num2 += tile2;
      }
      if (first && __any(cand)) {
        // the top-K insertions exactly as eval_topk_kernel makes them (one writer per list at a time)
        for (int qq = 0; qq < 4; ++qq) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int64_t item = item0 + 4 * q + v;
            if (q == qq && ok[v] && sg[v] > my_sc[K - 1]) {
              int p = K - 1;
              while (p > 0 && my_sc[p - 1] < sg[v]) {
                const float ps = my_sc[p - 1];
                const int pi = my_id[p - 1];
                my_sc[p] = ps;
                my_id[p] = pi;
                --p;
              }
              my_sc[p] = sg[v];
              my_id[p] = static_cast<int>(item);
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
      }
    }
    __syncthreads();                               // the next pass overwrites the positive lists
  }
  // the four lanes q = 0..3 of a user slot are lanes r, r + 16, r + 32, r + 48
  num2 += __shfl_xor(num2, 16);
  num2 += __shfl_xor(num2, 32);
  nneg += __shfl_xor(nneg, 16);
  nneg += __shfl_xor(nneg, 32);
  if (uok && q == 0) {
    for (int p = 0; p < K; ++p) {
      top_idx[upos * K + p] = my_id[p];
      if (top_val) top_val[upos * K + p] = my_sc[p];
    }
    auc_num2[upos] = num2;
    n_pos[upos] = npos;
    n_neg[upos] = nneg;
  }
}

}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_eval_topk_f32(const float* U, const float* I, int64_t n_item, int D, const int64_t* users,
                                    int64_t n_users, const int64_t* train_ptr, const int32_t* train_items, int K,
                                    int64_t* top_idx, float* top_val, void* stream) {
  TAGREC_REQUIRE(U && I && users && train_ptr && top_idx, "eval_topk: null pointer");
  TAGREC_REQUIRE(n_item >= 1 && n_users >= 0 && K >= 1 && K <= kMaxTopK, "eval_topk: bad shape (1 <= K <= 64)");
  TAGREC_REQUIRE(n_item < (1ll << 31), "eval_topk: item ids must fit int32");
  TAGREC_REQUIRE(aligned16(U) && aligned16(I), "eval_topk: rows must be 16-byte aligned");
  if (n_users == 0) return TAGREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned blocks = static_cast<unsigned>((n_users + kEvalUsers - 1) / kEvalUsers);
  const size_t lds = static_cast<size_t>(kEvalUsers) * K * 8;
#define LAUNCH(DD) \
  eval_topk_kernel<DD><<<blocks, kEvalThreads, lds, s>>>(U, I, n_item, users, n_users, train_ptr, train_items, K, top_idx, top_val)
  switch (D) {
    case 16: LAUNCH(16); break;
    case 32: LAUNCH(32); break;
    case 64: LAUNCH(64); break;
    case 128: LAUNCH(128); break;
    case 192: LAUNCH(192); break;
    case 256: LAUNCH(256); break;
    case 384: LAUNCH(384); break;
    case 512: LAUNCH(512); break;
    default:
      return fail(TAGREC_E_UNSUPPORTED,
                  "eval_topk: embedding width must be 16, 32, 64, 128, 192, 256, 384 or 512 (got " + std::to_string(D) + ")");
  }
#undef LAUNCH
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_eval_topk_auc_f32(const float* U, const float* I, int64_t n_item, int D, const int64_t* users,
                                        int64_t n_users, const int64_t* train_ptr, const int32_t* train_items,
                                        const int64_t* test_ptr, const int32_t* test_items, int K, int64_t* top_idx,
                                        float* top_val, int64_t* auc_num2, int64_t* n_pos, int64_t* n_neg, void* stream) {
  TAGREC_REQUIRE(U && I && users && train_ptr && test_ptr && top_idx && auc_num2 && n_pos && n_neg,
                 "eval_topk_auc: null pointer");
  TAGREC_REQUIRE(n_item >= 1 && n_users >= 0 && K >= 1 && K <= kMaxTopK, "eval_topk_auc: bad shape (1 <= K <= 64)");
  TAGREC_REQUIRE(n_item < (1ll << 31), "eval_topk_auc: item ids must fit int32");
  TAGREC_REQUIRE(aligned16(U) && aligned16(I), "eval_topk_auc: rows must be 16-byte aligned");
  if (n_users == 0) return TAGREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned blocks = static_cast<unsigned>((n_users + kEvalUsers - 1) / kEvalUsers);
  const size_t lds = static_cast<size_t>(kEvalUsers) * K * 8 + static_cast<size_t>(kEvalUsers) * kAucPosStride * 4 +
                     (kEvalUsers + 1) * sizeof(int);
#define LAUNCH(DD)                                                                                                    \
  do {                                                                                                                \
    if (lds > 64 * 1024)                                                                                              \
      TAGREC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(eval_topk_auc_kernel<DD>),                         \
                                     hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));             \
    eval_topk_auc_kernel<DD><<<blocks, kEvalThreads, lds, s>>>(U, I, n_item, users, n_users, train_ptr, train_items,  \
                                                               test_ptr, test_items, K, top_idx, top_val, auc_num2,   \
                                                               n_pos, n_neg);                                         \
  } while (0)
  switch (D) {
    case 16: LAUNCH(16); break;
    case 32: LAUNCH(32); break;
    case 64: LAUNCH(64); break;
    case 128: LAUNCH(128); break;
    case 192: LAUNCH(192); break;
    case 256: LAUNCH(256); break;
    case 384: LAUNCH(384); break;
    case 512: LAUNCH(512); break;
    default:
      return fail(TAGREC_E_UNSUPPORTED,
                  "eval_topk_auc: embedding width must be 16, 32, 64, 128, 192, 256, 384 or 512 (got " + std::to_string(D) + ")");
  }
#undef LAUNCH
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}
