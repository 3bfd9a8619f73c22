// K14: fixed-order scatter of compact batch rows into a node table -- dst[row] (=|+=) sum of src[j] over rows[j] == row --
// without float atomics: the deterministic form of `index_add_` / the BPR backward's atomicAdd for a row list that names
// a node more than once (a BPR batch repeats its popular positive items as a matter of course).
//
//   plan (per row list, device only, no host read):
//     keys    : key[j] = rows[j], or the sentinel n for an id outside [0, n) (counted, sorted to the end, never read again)
//     sort    : stable rocPRIM radix sort of (key, slot j): `order` = the slots by ascending row id, ascending slot inside a row
//     heads   : head[i] = sorted position i opens a new row; inclusive scan -> the segment every position belongs to
//     segments: seg_row[s] / seg_ptr[s] per distinct row in ascending row id, seg_ptr[S] = the valid count; S and the valid
//               count stay on the device (the scatter's grid is sized by the list length and surplus groups leave on them)
//   scatter : one lane group per 1024-slot chunk of a segment (chunks start at the segment's first slot).  A chunk is ONE
//             left-to-right fp32 chain that starts from its first term, in ascending slot id.  A segment of <= 1024 slots is
//             its only chunk and lands on dst directly; a longer one parks its chunk sums in a slab and a second launch adds
//             them left to right (the scheme of the long CSR rows).  dst is touched once per segment: stored (assign), or one
//             fp32 add of the finished sum (accumulate).
//
// The slab slot of a chunk is found without a work list: two chunks can begin inside one 1024-aligned window of sorted
// positions only as (a later chunk of a long segment, the FIRST chunk of the next one) -- a long segment is longer than the
// window -- so slot 2 * (position / 1024) + (first chunk of its segment) is unique.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "rowlist.h"

namespace tagrec {
namespace {

constexpr int kThreads = 256;

// with_tmp = false: the parts a scatter reads (everything up to the slab); `total` then ends there and no rocPRIM size query is made
int rowlist_layout(int64_t n_listed, int width, RowListLayout* L, bool with_tmp = true) {
  size_t o = rowlist_layout_head(n_listed, width, L);
  if (!with_tmp) return TAGREC_OK;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  const size_t T = static_cast<size_t>(n_listed);
  L->keys_in = take(T * sizeof(uint32_t));
  L->keys_out = take(T * sizeof(uint32_t));
  L->slots_in = take(T * sizeof(int32_t));
  L->head = take(T * sizeof(int32_t));
  size_t sort_bytes = 0, scan_bytes = 0;
  TAGREC_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, static_cast<const uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                       static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr), T, 0u, 32u));
  TAGREC_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr), T,
                                     rocprim::plus<int32_t>()));
  L->tmp_sort = sort_bytes;
  L->tmp_scan = scan_bytes;
  L->tmp = take(sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
  L->total = o;
  return TAGREC_OK;
}

// ---- plan ----
__global__ __launch_bounds__(kThreads) void rowlist_keys_kernel(const int64_t* __restrict__ rows, int n_listed, int64_t n,
                                                                uint32_t* __restrict__ keys, int32_t* __restrict__ slots,
                                                                int32_t* __restrict__ counts) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_listed) return;
  const int64_t r = rows[i];
  const bool ok = r >= 0 && r < n;
  if (!ok) atomicAdd(counts + kCountBad, 1);           // (an integer counter: its value does not depend on the order)
  keys[i] = ok ? static_cast<uint32_t>(r) : static_cast<uint32_t>(n);
  slots[i] = i;
}

__global__ __launch_bounds__(kThreads) void rowlist_heads_kernel(const uint32_t* __restrict__ keys, int n_listed, uint32_t n,
                                                                 int32_t* __restrict__ head) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_listed) return;
  const uint32_t k = keys[i];
  head[i] = k < n && (i == 0 || keys[i - 1] != k);
}

// seg_of holds the INCLUSIVE scan of head: position i belongs to segment seg_of[i] - 1
__global__ __launch_bounds__(kThreads) void rowlist_segments_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ head,
                                                                    const int32_t* __restrict__ seg_of, int n_listed, uint32_t n,
                                                                    int32_t* __restrict__ seg_row, int32_t* __restrict__ seg_ptr,
                                                                    int32_t* __restrict__ counts) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_listed) return;
  const uint32_t k = keys[i];
  if (k >= n) {                                        // the sentinel tail; position 0 there: nothing valid at all
    if (i == 0) { counts[kCountSegments] = 0; counts[kCountValid] = 0; seg_ptr[0] = 0; }
    return;
  }
  const int32_t s = seg_of[i] - 1;                     // 0 <= s <= i < n_listed
  if (head[i]) { seg_row[s] = static_cast<int32_t>(k); seg_ptr[s] = i; }
  if (i == n_listed - 1 || keys[i + 1] >= n) {         // the last valid position closes the last segment
    seg_ptr[s + 1] = i + 1;
    counts[kCountSegments] = s + 1;
    counts[kCountValid] = i + 1;
  }
}

// ---- scatter (the segment sum itself: scatter_column of rowlist.h) ----
// where a finished segment sum lands: one store, or one fp32 add, per segment and column
template <typename V>
struct LandOnRow {
  V* dst; int64_t ldd; int accumulate;
  __device__ __forceinline__ void operator()(int64_t row, const V& acc) const {
    V* d = dst + row * ldd;
    *d = accumulate ? vadd(*d, acc) : acc;
  }
};

// Lane group q of a wave owns sorted position (wave * NPI + q), lane c of the group its float4 column c.
template <int LPR, bool FOLD>
__global__ __launch_bounds__(kScatterWaves * kWave) void row_scatter_vec_kernel(ScatterPlan pl, const float* __restrict__ src, int64_t lds,
                                                                                float* __restrict__ dst, int64_t ldd,
                                                                                float* __restrict__ slab, int64_t n_dst, int accumulate) {
  constexpr int NPI = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = lane / LPR, c = lane % LPR;
  const int64_t wv = static_cast<int64_t>(blockIdx.x) * kScatterWaves + (threadIdx.x >> 6);
  const int64_t i = wv * NPI + q;
  if (i >= pl.n_listed || i >= pl.counts[kCountValid]) return;
  scatter_column<float4, FOLD>(pl, static_cast<int32_t>(i), reinterpret_cast<const float4*>(src) + c, lds / 4,
                               reinterpret_cast<float4*>(slab) + c, LPR, n_dst,
                               LandOnRow<float4>{reinterpret_cast<float4*>(dst) + c, ldd / 4, accumulate});
}

// Any width: one wavefront per sorted position, lane c takes columns c, c + 64, ...
template <bool FOLD>
__global__ __launch_bounds__(kScatterWaves * kWave) void row_scatter_scalar_kernel(ScatterPlan pl, const float* __restrict__ src, int64_t lds,
                                                                                   float* __restrict__ dst, int64_t ldd,
                                                                                   float* __restrict__ slab, int64_t n_dst, int D,
                                                                                   int accumulate) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kScatterWaves + (threadIdx.x >> 6);
  if (i >= pl.n_listed || i >= pl.counts[kCountValid]) return;
  for (int c = lane; c < D; c += kWave)
    scatter_column<float, FOLD>(pl, static_cast<int32_t>(i), src + c, lds, slab + c, D, n_dst, LandOnRow<float>{dst + c, ldd, accumulate});
}

template <int LPR>
int launch_vec(const ScatterPlan& pl, const float* src, int64_t lds, float* dst, int64_t ldd, float* slab, int64_t n_dst, int accumulate,
               hipStream_t s) {
  constexpr int per_block = kScatterWaves * (kWave / LPR);
  const unsigned blocks = static_cast<unsigned>((pl.n_listed + per_block - 1) / per_block);
  row_scatter_vec_kernel<LPR, false><<<blocks, kScatterWaves * kWave, 0, s>>>(pl, src, lds, dst, ldd, slab, n_dst, accumulate);
  TAGREC_LAUNCH_CHECK();
  if (pl.n_listed > kScatterChunk) {                   // only then can a segment be long
    row_scatter_vec_kernel<LPR, true><<<blocks, kScatterWaves * kWave, 0, s>>>(pl, src, lds, dst, ldd, slab, n_dst, accumulate);
    TAGREC_LAUNCH_CHECK();
  }
  return TAGREC_OK;
}

int launch_scalar(const ScatterPlan& pl, const float* src, int64_t lds, float* dst, int64_t ldd, float* slab, int64_t n_dst, int D,
                  int accumulate, hipStream_t s) {
  const unsigned blocks = static_cast<unsigned>((pl.n_listed + kScatterWaves - 1) / kScatterWaves);
  row_scatter_scalar_kernel<false><<<blocks, kScatterWaves * kWave, 0, s>>>(pl, src, lds, dst, ldd, slab, n_dst, D, accumulate);
  TAGREC_LAUNCH_CHECK();
  if (pl.n_listed > kScatterChunk) {
    row_scatter_scalar_kernel<true><<<blocks, kScatterWaves * kWave, 0, s>>>(pl, src, lds, dst, ldd, slab, n_dst, D, accumulate);
    TAGREC_LAUNCH_CHECK();
  }
  return TAGREC_OK;
}

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int64_t tagrec_rowlist_workspace(int64_t n_listed, int width) {
  if (check_list("rowlist_workspace", n_listed, width) != TAGREC_OK) return 0;
  RowListLayout L;
  if (rowlist_layout(n_listed, width, &L) != TAGREC_OK) return 0;
  return static_cast<int64_t>(L.total);
}

extern "C" int64_t tagrec_rowlist_plan_result(int64_t n_listed, int width, int part) {
  if (check_list("rowlist_plan_result", n_listed, width) != TAGREC_OK) return -1;
  RowListLayout L;
  if (rowlist_layout(n_listed, width, &L, false) != TAGREC_OK) return -1;
  switch (part) {
    case 0: return static_cast<int64_t>(L.order);
    case 1: return static_cast<int64_t>(L.seg_row);
    case 2: return static_cast<int64_t>(L.seg_ptr);
    case 3: return static_cast<int64_t>(L.counts);
    default: set_error("rowlist_plan_result: part must be 0 (order), 1 (seg_row), 2 (seg_ptr) or 3 (counts)"); return -1;
  }
}

extern "C" int tagrec_rowlist_plan_i64(const int64_t* rows, int64_t n_listed, int64_t n, int width, void* ws, int64_t ws_bytes,
                                       void* stream) {
  TAGREC_REQUIRE(rows != nullptr && ws != nullptr, "rowlist_plan: null pointer");
  int rc = check_list("rowlist_plan", n_listed, width);
  if (rc != TAGREC_OK) return rc;
  TAGREC_REQUIRE(n >= 1 && n < (1ll << 31) - 1, "rowlist_plan: the table holds 1 .. 2^31 - 2 rows");
  TAGREC_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255u) == 0, "rowlist_plan: the workspace must be 256-byte aligned");
  RowListLayout L;
  rc = rowlist_layout(n_listed, width, &L);
  if (rc != TAGREC_OK) return rc;
  TAGREC_REQUIRE(ws_bytes >= static_cast<int64_t>(L.total), "rowlist_plan: workspace smaller than tagrec_rowlist_workspace(...)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  int32_t* order = reinterpret_cast<int32_t*>(base + L.order);
  int32_t* seg_row = reinterpret_cast<int32_t*>(base + L.seg_row);
  int32_t* seg_ptr = reinterpret_cast<int32_t*>(base + L.seg_ptr);
  int32_t* counts = reinterpret_cast<int32_t*>(base + L.counts);
  int32_t* seg_of = reinterpret_cast<int32_t*>(base + L.seg_of);
  uint32_t* keys_in = reinterpret_cast<uint32_t*>(base + L.keys_in);
  uint32_t* keys_out = reinterpret_cast<uint32_t*>(base + L.keys_out);
  int32_t* slots_in = reinterpret_cast<int32_t*>(base + L.slots_in);
  int32_t* head = reinterpret_cast<int32_t*>(base + L.head);
  const int T = static_cast<int>(n_listed);
  const unsigned blocks = static_cast<unsigned>((n_listed + kThreads - 1) / kThreads);
  TAGREC_HIP(hipMemsetAsync(counts, 0, 4 * sizeof(int32_t), s));
  rowlist_keys_kernel<<<blocks, kThreads, 0, s>>>(rows, T, n, keys_in, slots_in, counts);
  TAGREC_LAUNCH_CHECK();
  size_t tmp = L.tmp_sort;
  TAGREC_HIP(rocprim::radix_sort_pairs(base + L.tmp, tmp, static_cast<const uint32_t*>(keys_in), keys_out,
                                       static_cast<const int32_t*>(slots_in), order, static_cast<size_t>(n_listed), 0u, 32u, s));
  rowlist_heads_kernel<<<blocks, kThreads, 0, s>>>(keys_out, T, static_cast<uint32_t>(n), head);
  TAGREC_LAUNCH_CHECK();
  tmp = L.tmp_scan;
  TAGREC_HIP(rocprim::inclusive_scan(base + L.tmp, tmp, static_cast<const int32_t*>(head), seg_of, static_cast<size_t>(n_listed),
                                     rocprim::plus<int32_t>(), s));
  rowlist_segments_kernel<<<blocks, kThreads, 0, s>>>(keys_out, head, seg_of, T, static_cast<uint32_t>(n), seg_row, seg_ptr, counts);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_row_scatter_ordered_f32(const void* ws, int64_t ws_bytes, int64_t n_listed, int width, const float* src,
                                              int64_t lds, float* dst, int64_t ldd, int64_t n_dst, int D, int accumulate,
                                              void* stream) {
  TAGREC_REQUIRE(ws != nullptr && src != nullptr && dst != nullptr, "row_scatter_ordered: null pointer");
  int rc = check_list("row_scatter_ordered", n_listed, width);
  if (rc != TAGREC_OK) return rc;
  TAGREC_REQUIRE(D >= 1 && D <= width, "row_scatter_ordered: D must be 1 .. the width the plan's workspace was sized for");
  TAGREC_REQUIRE(lds >= D && ldd >= D, "row_scatter_ordered: a row stride is smaller than D");
  TAGREC_REQUIRE(n_dst >= 1 && n_dst < (1ll << 31) - 1, "row_scatter_ordered: bad destination row count");
  TAGREC_REQUIRE(src + (n_listed - 1) * lds + D <= dst || dst + (n_dst - 1) * ldd + D <= src,
                 "row_scatter_ordered: src and dst overlap");
  RowListLayout L;
  rc = rowlist_layout(n_listed, width, &L, false);
  if (rc != TAGREC_OK) return rc;
  TAGREC_REQUIRE(ws_bytes >= static_cast<int64_t>(L.total), "row_scatter_ordered: workspace smaller than tagrec_rowlist_workspace(...)");
  const char* base = static_cast<const char*>(ws);
  const ScatterPlan pl = scatter_plan(ws, L, n_listed);
  float* slab = reinterpret_cast<float*>(const_cast<char*>(base) + L.slab);     // scratch of the launch in flight: one stream per plan
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = aligned16(src) && aligned16(dst) && lds % 4 == 0 && ldd % 4 == 0;
  if (vec) {
    switch (D) {
      case 8: return launch_vec<2>(pl, src, lds, dst, ldd, slab, n_dst, accumulate, s);
      case 16: return launch_vec<4>(pl, src, lds, dst, ldd, slab, n_dst, accumulate, s);
      case 32: return launch_vec<8>(pl, src, lds, dst, ldd, slab, n_dst, accumulate, s);
      case 64: return launch_vec<16>(pl, src, lds, dst, ldd, slab, n_dst, accumulate, s);
      case 128: return launch_vec<32>(pl, src, lds, dst, ldd, slab, n_dst, accumulate, s);
      case 256: return launch_vec<64>(pl, src, lds, dst, ldd, slab, n_dst, accumulate, s);
      default: break;
    }
  }
  return launch_scalar(pl, src, lds, dst, ldd, slab, n_dst, D, accumulate, s);
}
