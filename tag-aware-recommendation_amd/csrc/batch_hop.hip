// K13: the masked backward hop below the top layer of a restricted LightGCN step, driven by an inverted list.
//
// The hop computes, for every row j of the mask (the batch rows and their neighbours: ~40 % of the graph at C2),
//   G[j] = sum_b At[j, b] g[b]   over the <= 3 B batch rows b,   + the normalize-backward term on the batch rows.
// The masked row kernel (spmm.hip, spmm_rows_grouped_kernel) walks every stored entry of every masked row -- 95 M column
// ids and flag bytes at C2 -- to find the ~1 M entries that point at a batch row.  Those entries are exactly the stored
// entries of the batch rows of the TRANSPOSED matrix, which `graph_mark_rows` already walks to build the mask.  So:
//
//   plan (per step, device only, no host read):
//     leader : the first occurrence of every distinct batch node (a batch lists a node more than once);
//     count  : cnt[j] += 1 for every stored entry (b, j) of a leading batch row b          (integer atomics)
//     scan   : off = exclusive prefix of cnt over the n + 1 node slots                      (rocPRIM)
//     fill   : record (j, b, w) at off[j] + slot, slot handed out by an integer atomic (any order inside a segment)
//     order  : every record finds its rank by source id inside its segment and moves there: segment j then lists its
//              sources in ASCENDING b -- the order in which row j of At stores them
//   hop  : one lane group per destination row (the layout of spmm_rows_grouped_kernel) takes its segment in order with
//          sequential fmaf from zero and runs the same epilogue.  For rows of <= kLongRow entries that is the arithmetic
//          of the masked kernel in the same order: the same bits.  Longer rows (popular items next to a batch user), which
//          the masked kernel sums through chunk partials and a butterfly, are summed here in ascending source order too, in
//          an fp64 accumulator rounded once: a fixed order, and no further from the exact sum than the tree-shaped fp32 sum
//          it replaces (a plain fp32 chain over ~50 terms measured 3x the masked kernel's error against fp64).
//
// No float atomics; the segment order does not depend on which thread won an integer atomic.  The record buffers have a
// capacity fixed by the caller (the sum of the T largest row degrees bounds the record count); the device total is
// checked against it, nothing is written past it, and an overflow raises a flag the host reads at its next check.
#include <algorithm>
#include <cstring>

#include <rocprim/device/device_scan.hpp>

#include "common.h"
#include "graph.h"

namespace tagrec {
namespace {

constexpr int kSplits = 32;              // ranges per listed row (batch rows are popular items: 1e5 entries), as graph_mark_rows
constexpr int64_t kMaxListed = 1 << 14;  // the leader pass compares every pair of list elements

// ---- workspace layout (bytes, every part 256-byte aligned) ----
struct HopLayout {
  size_t cnt, off, leader, dst, src, w, src_s, w_s, scan_tmp, scan_bytes, total;
};

size_t up256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

int hop_layout(int64_t n_rows, int64_t n_listed, int64_t capacity, HopLayout* L) {
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  L->cnt = take((n_rows + 1) * sizeof(int32_t));
  L->off = take((n_rows + 1) * sizeof(int32_t));
  L->leader = take(static_cast<size_t>(n_listed));
  L->dst = take(capacity * sizeof(int32_t));
  L->src = take(capacity * sizeof(int32_t));
  L->w = take(capacity * sizeof(float));
  L->src_s = take(capacity * sizeof(int32_t));
  L->w_s = take(capacity * sizeof(float));
  size_t tmp = 0;
  TAGREC_HIP(rocprim::exclusive_scan(nullptr, tmp, static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr), 0,
                                     static_cast<size_t>(n_rows + 1), rocprim::plus<int32_t>()));
  L->scan_bytes = tmp;
  L->scan_tmp = take(tmp);
  L->total = o;
  return TAGREC_OK;
}

struct HopPlan {           // device view of a built plan
  const int32_t* off;      // [n_rows + 1]: segment of destination j = [off[j], off[j + 1])
  const int32_t* src;      // [capacity] source row of each record, ascending inside a segment
  const float* w;          // [capacity] its weight
  int32_t capacity;
};

// leader[i] = 1 iff no earlier element of the list names the same node
__global__ __launch_bounds__(256) void hop_leader_kernel(const int64_t* __restrict__ rows, int n_listed, uint8_t* __restrict__ leader) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_listed) return;
  const int64_t r = rows[i];
  int dup = 0;
#pragma unroll 8
  for (int k = 0; k < i; ++k) dup |= rows[k] == r;
  leader[i] = !dup;
}

// One block per (listed row, range).  FILL = false: count the records per destination; true: write them.
template <bool FILL>
__global__ __launch_bounds__(256) void hop_walk_kernel(GraphView g, const int64_t* __restrict__ rows, const uint8_t* __restrict__ leader,
                                                       int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                                                       int32_t* __restrict__ dst, int32_t* __restrict__ src, float* __restrict__ w,
                                                       int32_t capacity, int32_t* __restrict__ err) {
  const int64_t i = blockIdx.x / kSplits;
  const int part = blockIdx.x % kSplits;
  if (!leader[i]) return;
  const int64_t b = rows[i];
  if (b < 0 || b >= g.n_rows) {                     // not a row of the matrix: nothing is walked, the host is told
    if (part == 0 && threadIdx.x == 0) atomicOr(err, 2);
    return;
  }
  const int64_t start = g.rowptr[b], end = g.rowptr[b + 1];
  const int64_t per = (end - start + kSplits - 1) / kSplits;
  const int64_t b0 = start + part * per;
  const int64_t b1 = (b0 + per < end) ? b0 + per : end;
  for (int64_t e = b0 + threadIdx.x; e < b1; e += blockDim.x) {
    const int32_t j = g.col[e];
    if constexpr (!FILL) {
      atomicAdd(cnt + j, 1);
    } else {
      // slots are handed out from the top; the counter is back at zero when the segment is full
      const int64_t pos = static_cast<int64_t>(off[j]) + (atomicSub(cnt + j, 1) - 1);
      if (pos >= 0 && pos < capacity) {
        dst[pos] = j;
        src[pos] = static_cast<int32_t>(b);
        w[pos] = g.val[e];
      } else {
        atomicOr(err, 1);                           // more records than the caller's bound: never written
      }
    }
  }
}

// Every record moves to (segment start + its rank by source id): ascending sources inside a segment, whatever order the
// fill left them in.  (Sources of a segment are distinct: leaders are distinct nodes and a CSR row stores a column once;
// equal sources, should a matrix store duplicates, are kept apart by their position.)
__global__ __launch_bounds__(256) void hop_order_kernel(const int32_t* __restrict__ off, int64_t n_rows, const int32_t* __restrict__ dst,
                                                        const int32_t* __restrict__ src, const float* __restrict__ w,
                                                        int32_t* __restrict__ src_s, float* __restrict__ w_s, int32_t capacity) {
  const int32_t total = min(off[n_rows], capacity);
  const int64_t step = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; p < total; p += step) {
    const int32_t j = dst[p];
    if (j < 0 || j >= n_rows) continue;             // (a slot the fill refused to write: overflow, flagged there)
    const int32_t s = off[j], e = min(off[j + 1], capacity);
    const int32_t b = src[p];
    int32_t rank = 0;
    for (int32_t q = s; q < e; ++q) {
      const int32_t o = src[q];
      rank += (o < b) || (o == b && q < p);
    }
    if (s + rank < e) {
      src_s[s + rank] = b;
      w_s[s + rank] = w[p];
    }
  }
}

// ---- the hop ------------------------------------------------------------------------------------------------------
struct HopEpi {            // the EPI_NORMBWD epilogue of spmm.hip
  float* Y;
  const float* inv_norm;
  const float* Xraw;
  const float* B;
  float s;
  DropMask drop;
  uint8_t* out_flags;
  const uint8_t* row_mask;
  const uint8_t* b_flags;
};

typedef float nt_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_stream(const float4* p) {
  const nt_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f32x4*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream(float4* p, const float4& a) {
  __builtin_nontemporal_store(nt_f32x4{a.x, a.y, a.z, a.w}, reinterpret_cast<nt_f32x4*>(p));
}
__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void f4_fma(float4& a, float s, const float4& x) {
  a.x = fmaf(s, x.x, a.x); a.y = fmaf(s, x.y, a.y); a.z = fmaf(s, x.z, a.z); a.w = fmaf(s, x.w, a.w);
}
__device__ __forceinline__ float f4_dot(const float4& a, const float4& b) {
  return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w)));
}
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
// gradient of z = x / max(||x||, eps), as spmm.hip's normalize_bwd (the same expressions: the same roundings)
template <int LPR>
__device__ __forceinline__ float4 normalize_bwd(const float4& xr, float inv, const float4& dz) {
  const float4 z = make_float4(xr.x * inv, xr.y * inv, xr.z * inv, xr.w * inv);
  float dot = group_sum<LPR>(f4_dot(z, dz));
  if (inv >= 1e12f) dot = 0.f;
  return make_float4(inv * (dz.x - z.x * dot), inv * (dz.y - z.y * dot), inv * (dz.z - z.z * dot),
                     inv * (dz.w - z.w * dot));
}

// Lane group q of a wave owns destination row (wave * NPI + q).  A row is visited when its mask byte is set and it has
// records or an epilogue term; every other row is left unwritten with its out_flags byte as the caller zeroed it.
template <int LPR>
__global__ __launch_bounds__(kWavesPerBlock * kWave) void batch_hop_kernel(int64_t n_rows, const int64_t* __restrict__ rowptr, HopPlan pl,
                                                                            const float* __restrict__ X, HopEpi e) {
  constexpr int NPI = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = lane / LPR, c = lane % LPR;
  const int64_t wv = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t r = wv * NPI + q;
  bool valid = r < n_rows && e.row_mask[r];
  int32_t start = 0, len = 0;
  if (valid) {
    start = min(pl.off[r], pl.capacity);
    len = min(pl.off[r + 1], pl.capacity) - start;
    if (len <= 0 && e.b_flags && !e.b_flags[r]) valid = false;
  }
  if (!valid) len = 0;
  // a row the masked kernel cuts into chunks (its result there is not a plain chain): fp64 chain below
  const bool is_long = len > 0 && rowptr[r + 1] - rowptr[r] > kLongRow;
  const int32_t len_long = is_long ? len : 0;
  if (is_long) len = 0;
  int maxlen = len;
#pragma unroll
  for (int m = LPR; m < kWave; m <<= 1) maxlen = max(maxlen, __shfl_xor(maxlen, m));
  const float4* __restrict__ Xv = reinterpret_cast<const float4*>(X) + c;
  float4 acc = f4_zero();
  for (int t = 0; t < maxlen; t += 4) {
    float4 x[4];
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ok = t + u < len;
      const int32_t col = ok ? pl.src[start + t + u] : 0;
      v[u] = ok ? pl.w[start + t + u] : 0.f;
      x[u] = ok ? Xv[static_cast<int64_t>(col) * LPR] : f4_zero();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) f4_fma(acc, v[u], x[u]);
  }
  if (is_long) {                                 // (no cross-lane traffic in here: lane groups may diverge)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
    for (int t = 0; t < len_long; ++t) {
      const double w = static_cast<double>(pl.w[start + t]);
      const float4 x = Xv[static_cast<int64_t>(pl.src[start + t]) * LPR];
      a0 = fma(w, static_cast<double>(x.x), a0); a1 = fma(w, static_cast<double>(x.y), a1);
      a2 = fma(w, static_cast<double>(x.z), a2); a3 = fma(w, static_cast<double>(x.w), a3);
    }
    acc = make_float4(static_cast<float>(a0), static_cast<float>(a1), static_cast<float>(a2), static_cast<float>(a3));
  }
  if (!valid) return;                            // (whole lane groups leave: the group reductions below stay inside a group)
  const int64_t off = r * LPR + c;
  float4 o = acc;
  if (!e.b_flags || e.b_flags[r]) {
    const float4 xr = ld_stream(reinterpret_cast<const float4*>(e.Xraw) + off);
    float4 dz = ld_stream(reinterpret_cast<const float4*>(e.B) + off);
    dz.x *= e.s; dz.y *= e.s; dz.z *= e.s; dz.w *= e.s;
    const float4 gz = normalize_bwd<LPR>(xr, e.inv_norm[r], dz);
    o = make_float4(acc.x + gz.x, acc.y + gz.y, acc.z + gz.z, acc.w + gz.w);
  }
  drop4(e.drop, off, o.x, o.y, o.z, o.w);
  st_stream(reinterpret_cast<float4*>(e.Y) + off, o);
  if (e.out_flags) {
    const float nz = group_sum<LPR>((o.x != 0.f || o.y != 0.f || o.z != 0.f || o.w != 0.f) ? 1.f : 0.f);
    if (c == 0) e.out_flags[r] = nz != 0.f;
  }
}

template <int LPR>
int launch_hop(int64_t n_rows, const int64_t* rowptr, const HopPlan& pl, const float* X, const HopEpi& e, hipStream_t s) {
  constexpr int rows_per_block = kWavesPerBlock * (kWave / LPR);
  const unsigned blocks = static_cast<unsigned>((n_rows + rows_per_block - 1) / rows_per_block);
  batch_hop_kernel<LPR><<<blocks, kWavesPerBlock * kWave, 0, s>>>(n_rows, rowptr, pl, X, e);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

int check_shape(const char* who, int64_t n_rows, int64_t n_listed, int64_t capacity) {
  TAGREC_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31) - 1, std::string(who) + ": bad row count");
  TAGREC_REQUIRE(n_listed >= 1 && n_listed <= kMaxListed, std::string(who) + ": the list holds 1 .. 16384 rows");
  TAGREC_REQUIRE(capacity >= 1 && capacity < (1ll << 31), std::string(who) + ": the record capacity must be 1 .. 2^31 - 1");
  return TAGREC_OK;
}

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int64_t tagrec_batch_hop_workspace(int64_t n_rows, int64_t n_listed, int64_t capacity) {
  if (check_shape("batch_hop_workspace", n_rows, n_listed, capacity) != TAGREC_OK) return 0;
  HopLayout L;
  if (hop_layout(n_rows, n_listed, capacity, &L) != TAGREC_OK) return 0;
  return static_cast<int64_t>(L.total);
}

extern "C" int tagrec_batch_hop_plan(const tagrec_graph* gt, const int64_t* rows, int64_t n_listed, int64_t capacity, void* ws,
                                     int64_t ws_bytes, int32_t* err, void* stream) {
  TAGREC_REQUIRE(gt != nullptr && rows != nullptr && ws != nullptr && err != nullptr, "batch_hop_plan: null pointer");
  // gt = the TRANSPOSE of the matrix the hop multiplies by: its row b lists the destinations of source b
  const int64_t n_dst = gt->n_cols;
  int rc = check_shape("batch_hop_plan", n_dst, n_listed, capacity);
  if (rc != TAGREC_OK) return rc;
  TAGREC_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255u) == 0, "batch_hop_plan: the workspace must be 256-byte aligned");
  HopLayout L;
  rc = hop_layout(n_dst, n_listed, capacity, &L);
  if (rc != TAGREC_OK) return rc;
  TAGREC_REQUIRE(ws_bytes >= static_cast<int64_t>(L.total), "batch_hop_plan: workspace smaller than tagrec_batch_hop_workspace(...)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  int32_t* cnt = reinterpret_cast<int32_t*>(base + L.cnt);
  int32_t* off = reinterpret_cast<int32_t*>(base + L.off);
  uint8_t* leader = reinterpret_cast<uint8_t*>(base + L.leader);
  int32_t* dst = reinterpret_cast<int32_t*>(base + L.dst);
  int32_t* src = reinterpret_cast<int32_t*>(base + L.src);
  float* w = reinterpret_cast<float*>(base + L.w);
  const GraphView gv{gt->n_rows, gt->rowptr, gt->col, gt->val, gt->n_cols};
  const int32_t cap = static_cast<int32_t>(capacity);
  TAGREC_HIP(hipMemsetAsync(cnt, 0, (n_dst + 1) * sizeof(int32_t), s));
  hop_leader_kernel<<<static_cast<unsigned>((n_listed + 255) / 256), 256, 0, s>>>(rows, static_cast<int>(n_listed), leader);
  TAGREC_LAUNCH_CHECK();
  const unsigned wblocks = static_cast<unsigned>(n_listed * kSplits);
  hop_walk_kernel<false><<<wblocks, 256, 0, s>>>(gv, rows, leader, cnt, off, dst, src, w, cap, err);
  TAGREC_LAUNCH_CHECK();
  size_t tmp = L.scan_bytes;
  TAGREC_HIP(rocprim::exclusive_scan(base + L.scan_tmp, tmp, static_cast<const int32_t*>(cnt), off, 0, static_cast<size_t>(n_dst + 1),
                                     rocprim::plus<int32_t>(), s));
  hop_walk_kernel<true><<<wblocks, 256, 0, s>>>(gv, rows, leader, cnt, off, dst, src, w, cap, err);
  TAGREC_LAUNCH_CHECK();
  const unsigned oblocks = static_cast<unsigned>(std::min<int64_t>((capacity + 255) / 256, 4096));
  hop_order_kernel<<<oblocks, 256, 0, s>>>(off, n_dst, dst, src, w, reinterpret_cast<int32_t*>(base + L.src_s),
                                           reinterpret_cast<float*>(base + L.w_s), cap);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_batch_hop_normbwd_f32(const tagrec_graph* g, const void* ws, int64_t ws_bytes, int64_t n_listed, int64_t capacity,
                                            const float* G_in, const float* X_raw, const float* inv_norm, const float* dZ,
                                            float d_scale, float* G_out, uint8_t* out_flags, const uint8_t* row_mask,
                                            const uint8_t* dz_flags, int D, void* stream) {
  TAGREC_REQUIRE(g != nullptr && ws != nullptr && G_in != nullptr && G_out != nullptr && row_mask != nullptr,
                 "batch_hop_normbwd: null pointer");
  TAGREC_REQUIRE(X_raw != nullptr && inv_norm != nullptr && dZ != nullptr, "batch_hop_normbwd: null X_raw, inv_norm or dZ");
  TAGREC_REQUIRE(static_cast<const void*>(G_in) != static_cast<const void*>(G_out), "batch_hop_normbwd: output aliases the gathered input");
  TAGREC_REQUIRE(aligned16(G_in) && aligned16(G_out) && aligned16(X_raw) && aligned16(dZ), "batch_hop_normbwd: rows must be 16-byte aligned");
  int rc = check_shape("batch_hop_normbwd", g->n_rows, n_listed, capacity);
  if (rc != TAGREC_OK) return rc;
  HopLayout L;
  rc = hop_layout(g->n_rows, n_listed, capacity, &L);
  if (rc != TAGREC_OK) return rc;
  TAGREC_REQUIRE(ws_bytes >= static_cast<int64_t>(L.total), "batch_hop_normbwd: workspace smaller than tagrec_batch_hop_workspace(...)");
  const char* base = static_cast<const char*>(ws);
  const HopPlan pl{reinterpret_cast<const int32_t*>(base + L.off), reinterpret_cast<const int32_t*>(base + L.src_s),
                   reinterpret_cast<const float*>(base + L.w_s), static_cast<int32_t>(capacity)};
  const HopEpi e{G_out, inv_norm, X_raw, dZ, d_scale, DropMask{0.f, 0}, out_flags, row_mask, dz_flags};
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (D) {
    case 8: return launch_hop<2>(g->n_rows, g->rowptr, pl, G_in, e, s);
    case 16: return launch_hop<4>(g->n_rows, g->rowptr, pl, G_in, e, s);
    case 32: return launch_hop<8>(g->n_rows, g->rowptr, pl, G_in, e, s);
    case 64: return launch_hop<16>(g->n_rows, g->rowptr, pl, G_in, e, s);
    case 128: return launch_hop<32>(g->n_rows, g->rowptr, pl, G_in, e, s);
    case 256: return launch_hop<64>(g->n_rows, g->rowptr, pl, G_in, e, s);
    default: return fail(TAGREC_E_UNSUPPORTED, "batch_hop_normbwd: D must be 8 .. 256, a power of two");
  }
}
