// What a kernel needs of a built row-list plan (rowscatter.hip builds it): the part of the workspace a consumer reads, its
// device view, and the ONE statement of the fixed-order segment sum.  rowscatter.hip lands the sum on a destination row;
// rowadam.hip hands it to Adam's update as the row's gradient.
#pragma once
#include "common.h"

namespace tagrec {

constexpr int kScatterChunk = 1024;      // slots per chain (= kLongRow of the CSR kernels)
constexpr int kScatterWaves = 4;         // wavefronts per block

// ---- workspace layout (bytes, every part 256-byte aligned) ----
struct RowListLayout {
  size_t order, seg_row, seg_ptr, counts, seg_of, slab, keys_in, keys_out, slots_in, head, tmp, tmp_sort, tmp_scan, total;
};
enum { kCountSegments = 0, kCountValid = 1, kCountBad = 2 };   // counts[4] (int32)

inline size_t up256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

inline int64_t slab_rows(int64_t n_listed) { return n_listed > kScatterChunk ? 2 * ((n_listed + kScatterChunk - 1) / kScatterChunk) : 0; }

// the parts a consumer of the plan reads (everything up to the slab); `total` ends there.  -> the running offset, from
// which rowscatter.hip lays out the parts only the plan's construction needs
inline size_t rowlist_layout_head(int64_t n_listed, int width, RowListLayout* L) {
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  const size_t T = static_cast<size_t>(n_listed);
  L->order = take(T * sizeof(int32_t));
  L->seg_row = take(T * sizeof(int32_t));
  L->seg_ptr = take((T + 1) * sizeof(int32_t));
  L->counts = take(4 * sizeof(int32_t));
  L->seg_of = take(T * sizeof(int32_t));
  L->slab = take(static_cast<size_t>(slab_rows(n_listed)) * width * sizeof(float));
  L->total = o;
  return o;
}

inline int check_list(const char* who, int64_t n_listed, int width) {
  TAGREC_REQUIRE(n_listed >= 1 && n_listed < (1ll << 30), std::string(who) + ": the list holds 1 .. 2^30 - 1 rows");
  TAGREC_REQUIRE(width >= 1 && width <= (1 << 16), std::string(who) + ": the width must be 1 .. 65536");
  return TAGREC_OK;
}

struct ScatterPlan {        // device view of a built plan
  const int32_t* order;     // [n_listed] slot ids by (row, slot)
  const int32_t* seg_row;   // [S]
  const int32_t* seg_ptr;   // [S + 1]
  const int32_t* seg_of;    // [n_listed] inclusive head scan
  const int32_t* counts;
  int32_t n_listed;
};

inline ScatterPlan scatter_plan(const void* ws, const RowListLayout& L, int64_t n_listed) {
  const char* base = static_cast<const char*>(ws);
  return ScatterPlan{reinterpret_cast<const int32_t*>(base + L.order), reinterpret_cast<const int32_t*>(base + L.seg_row),
                     reinterpret_cast<const int32_t*>(base + L.seg_ptr), reinterpret_cast<const int32_t*>(base + L.seg_of),
                     reinterpret_cast<const int32_t*>(base + L.counts), static_cast<int32_t>(n_listed)};
}

__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ float4 vadd(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

__device__ __forceinline__ int64_t slab_slot(int32_t pos, bool first_chunk) { return 2 * static_cast<int64_t>(pos >> 10) + (first_chunk ? 1 : 0); }

// One column (V = float) or one 16-byte column group (V = float4) of the work of sorted position i.  src / slab point at
// that column; lds / lslab are row strides in units of V.
//   FOLD = false: position i opens a chunk -> chain over the chunk; the sum is a short segment's whole sum, or parked in the slab.
//   FOLD = true : position i opens a LONG segment -> its chunk sums, left to right.
// A finished segment sum is handed to land(row, sum), once per segment and column.
template <typename V, bool FOLD, typename Land>
__device__ __forceinline__ void scatter_column(const ScatterPlan& pl, int32_t i, const V* __restrict__ src, int64_t lds, V* __restrict__ slab,
                                               int64_t lslab, int64_t n_dst, Land&& land) {
  const int32_t s = pl.seg_of[i] - 1;
  const int32_t start = pl.seg_ptr[s];
  const int32_t len = pl.seg_ptr[s + 1] - start;
  const int32_t rel = i - start;
  V acc;
  if constexpr (!FOLD) {
    if (rel & (kScatterChunk - 1)) return;
    const int32_t m = min(kScatterChunk, len - rel);
    const int32_t* __restrict__ ord = pl.order + i;
    acc = src[static_cast<int64_t>(ord[0]) * lds];
    int32_t t = 1;
    for (; t + 4 <= m; t += 4) {                       // four rows in flight, added in slot order
      const V x0 = src[static_cast<int64_t>(ord[t]) * lds], x1 = src[static_cast<int64_t>(ord[t + 1]) * lds];
      const V x2 = src[static_cast<int64_t>(ord[t + 2]) * lds], x3 = src[static_cast<int64_t>(ord[t + 3]) * lds];
      acc = vadd(acc, x0); acc = vadd(acc, x1); acc = vadd(acc, x2); acc = vadd(acc, x3);
    }
    for (; t < m; ++t) acc = vadd(acc, src[static_cast<int64_t>(ord[t]) * lds]);
    if (len > kScatterChunk) {
      slab[slab_slot(i, rel == 0) * lslab] = acc;
      return;
    }
  } else {
    if (rel != 0 || len <= kScatterChunk) return;
    acc = slab[slab_slot(start, true) * lslab];
    for (int32_t p = start + kScatterChunk; p < start + len; p += kScatterChunk) acc = vadd(acc, slab[slab_slot(p, false) * lslab]);
  }
  const int64_t row = pl.seg_row[s];
  if (row < 0 || row >= n_dst) return;                 // (the plan admits ids of [0, n) only; n_dst >= n is checked on the host)
  land(row, acc);
}

}  // namespace tagrec
