// K13: the masked backward hop below the top layer of a restricted LightGCN step, driven by an inverted list.
//
// The hop computes, for every row j of the mask (the batch rows and their neighbours: ~40 % of the graph at C2),
//   G[j] = sum_b At[j, b] g[b]   over the <= 3 B batch rows b,   + the normalize-backward term on the batch rows.
// The masked row kernel (spmm.hip, spmm_rows_grouped_kernel) walks every stored entry of every masked row -- 95 M column
// ids and flag bytes at C2 -- to find the ~1 M entries that point at a batch row.  Those entries are exactly the stored
// entries of the batch rows of the TRANSPOSED matrix, which `graph_mark_rows` already walks to build the mask.  So:
//
//   plan (per step, device only, no host read, no global atomic on the records):
//     leader : one block sorts the list (bitonic, LDS), drops repeats and ids outside the matrix, and takes the exclusive
//              prefix of the leaders' row lengths: the leading rows laid end to end are `total` entries;
//     count  : kWalkBlocks blocks take equal shares of those entries, wherever the row boundaries fall (binary search in the
//              prefix), and count them per BUCKET of kBucketRows destinations in LDS;
//     offsets: per bucket, the prefix of the blocks' counts; the buckets' totals;
//     scatter: the same walk writes record (j, b, w) into its bucket's range -- the place handed out by an LDS counter that
//              starts at (bucket start + counts of the blocks before);
//     bucket : one block per bucket counts its records per destination in LDS, takes the prefix, appends to `dest` one entry
//              (row, segment start, segment length) per destination with a record and per leader without one (it still has
//              an epilogue term), groups the records by destination and moves every record to its rank by source id
//              inside its segment: segment j lists its sources in ASCENDING b -- the order in which row j of At stores them
//     Global integer atomics cost one memory-side transaction each (a pass of 1 M of them measured 66 us without, 140 us
//     with a returned value); the only ones left are one add per bucket to reserve its places in `dest`.
//   hop  : a fixed grid strides over `dest` (length n_dest, read from device memory); one lane group per entry (the layout of
//          spmm_rows_grouped_kernel) takes its segment in order with
//          sequential fmaf from zero and runs the same epilogue.  For rows of <= kLongRow entries that is the arithmetic
//          of the masked kernel in the same order: the same bits.  Longer rows (popular items next to a batch user), which
//          the masked kernel sums through chunk partials and a butterfly, are summed here in ascending source order too, in
//          an fp64 accumulator rounded once: a fixed order, and no further from the exact sum than the tree-shaped fp32 sum
//          it replaces (a plain fp32 chain over ~50 terms measured 3x the masked kernel's error against fp64).
//
// No float atomics; the segment order does not depend on which thread won an integer atomic, and the order of `dest` does
// not matter (rows are independent).  The record buffers have a capacity fixed by the caller (the sum of the T largest row
// degrees bounds the record count); the device total is checked against it, nothing is written past it, and an overflow
// raises a flag the host reads at its next check.
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstring>

#include "common.h"
#include "graph.h"

namespace tagrec {
namespace {

constexpr int64_t kMaxListed = 1 << 14;  // one block sorts the list in LDS
constexpr int64_t kMaxNodes = 1 << 24;   // kMaxBuckets buckets of kBucketRows destinations
constexpr int kBucketShift = 11;
constexpr int kBucketRows = 1 << kBucketShift;
constexpr int kMaxBuckets = static_cast<int>(kMaxNodes >> kBucketShift);   // 8192: one LDS counter each in the walks
static_assert(kMaxBuckets * sizeof(int32_t) <= 32768, "the walks keep one LDS counter per bucket");
constexpr int kLeadThreads = 1024;
constexpr int kWalkBlocks = 256;
constexpr int kWalkThreads = 1024;
constexpr int kBucketThreads = 1024;
constexpr int kHopBlocks = 2048;         // the hop's grid: 8 blocks per CU of a 256-CU device; it strides over the list

// ---- workspace layout (bytes, every part 256-byte aligned) ----
struct HopLayout {
  size_t hdr, lead, lpre, hist, tot, bst, dst, src, w, src_g, w_g, dest, total;
  int64_t n_buckets, dest_cap;
};

struct HopHeader {         // device-side counts of a plan
  int64_t total;           // stored entries of the leading rows = records the plan wants (may exceed the capacity)
  int32_t n_lead;          // distinct listed rows
  int32_t n_dest;          // entries appended to `dest` (may exceed its capacity: nothing is written past it)
};

size_t up256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

void hop_layout(int64_t n_rows, int64_t n_listed, int64_t capacity, HopLayout* L) {
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += up256(bytes); return at; };
  L->n_buckets = (n_rows + kBucketRows - 1) >> kBucketShift;
  L->hdr = take(sizeof(HopHeader));
  L->lead = take(n_listed * sizeof(int32_t));
  L->lpre = take((n_listed + 1) * sizeof(int64_t));
  L->hist = take(static_cast<size_t>(kWalkBlocks) * L->n_buckets * sizeof(int32_t));
  L->tot = take(L->n_buckets * sizeof(int32_t));
  L->bst = take((L->n_buckets + 1) * sizeof(int32_t));
  L->dst = take(capacity * sizeof(int32_t));
  L->src = take(capacity * sizeof(int32_t));
  L->w = take(capacity * sizeof(float));
  L->src_g = take(capacity * sizeof(int32_t));
  L->w_g = take(capacity * sizeof(float));
  // every destination with a record (at most one per record, at most one per row) + every leading row without one
  L->dest_cap = std::min<int64_t>(std::min(capacity, n_rows) + n_listed, INT_MAX);
  L->dest = take(L->dest_cap * sizeof(int4));
  L->total = o;
}

struct HopPlan {           // device view of a built plan
  const int32_t* src;      // [capacity] source row of each record, ascending inside a segment
  const float* w;          // [capacity] its weight
  const int4* dest;        // [dest_cap] (row, segment start, segment length, -): the rows to visit, each once, in no order
  const HopHeader* hdr;
  int32_t dest_cap;
};

__device__ __forceinline__ int32_t ld_l2(const int32_t* p) {      // served by L2: data this block's other threads just wrote
  return __hip_atomic_load(const_cast<int32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// inclusive scan of one value per thread over the block (NT threads), in place in LDS
template <typename V, int NT>
__device__ __forceinline__ void block_scan(V* part, int tid) {
  for (int d = 1; d < NT; d <<= 1) {
    const V add = tid >= d ? part[tid - d] : V(0);
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
}

// One block.  lead[0 .. n_lead) = the distinct listed ids that are rows of the matrix, ascending; lpre = exclusive prefix of
// their row lengths, lpre[n_lead] = hdr->total; hdr->n_dest = 0.
__global__ __launch_bounds__(kLeadThreads) void hop_leader_kernel(GraphView g, const int64_t* __restrict__ rows, int n_listed,
                                                                  int32_t* __restrict__ lead, int64_t* __restrict__ lpre,
                                                                  HopHeader* __restrict__ hdr, int32_t* __restrict__ err) {
  __shared__ __align__(8) int32_t key[kMaxListed];
  constexpr int kPer = static_cast<int>(kMaxListed) / kLeadThreads;
  const int tid = threadIdx.x;
  int P = kLeadThreads;                              // padded length: a power of two, a multiple of the block
  while (P < n_listed) P <<= 1;
  for (int i = tid; i < P; i += kLeadThreads) {
    int32_t v = INT_MAX;                             // (pads and rejected ids sort to the end)
    if (i < n_listed) {
      const int64_t r = rows[i];
      if (r >= 0 && r < g.n_rows) v = static_cast<int32_t>(r);
      else atomicOr(err, 2);                         // not a row of the matrix: nothing is walked, the host is told
    }
    key[i] = v;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kLeadThreads) {
        const int l = i ^ j;
        if (l > i) {
          const int32_t a = key[i], b = key[l];
          if ((a > b) == ((i & k) == 0)) { key[i] = b; key[l] = a; }
        }
      }
      __syncthreads();
    }
  }
  const int per = P / kLeadThreads, i0 = tid * per;  // consecutive sorted positions per thread
  int32_t id[kPer];
  int64_t len[kPer];
  int32_t n_mine = 0;
  int64_t sum = 0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    id[u] = -1;
    len[u] = 0;
    if (u < per) {
      const int32_t v = key[i0 + u];
      if (v != INT_MAX && (i0 + u == 0 || key[i0 + u - 1] != v)) {
        id[u] = v;
        len[u] = g.rowptr[v + 1] - g.rowptr[v];
        ++n_mine;
        sum += len[u];
      }
    }
  }
  __syncthreads();                                   // the keys are in registers: their LDS now holds the two scans
  int32_t* cnt = key;
  int64_t* deg = reinterpret_cast<int64_t*>(key + kLeadThreads);
  cnt[tid] = n_mine;
  deg[tid] = sum;
  __syncthreads();
  block_scan<int32_t, kLeadThreads>(cnt, tid);
  block_scan<int64_t, kLeadThreads>(deg, tid);
  int32_t at = cnt[tid] - n_mine;
  int64_t run = deg[tid] - sum;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    if (id[u] >= 0) {
      lead[at] = id[u];
      lpre[at] = run;
      ++at;
      run += len[u];
    }
  }
  if (tid == kLeadThreads - 1) {
    int64_t total = deg[tid];
    if (total >= INT_MAX) {                          // positions are 32-bit: far beyond any capacity, nothing is planned
      atomicOr(err, 1);
      total = 0;
    }
    lpre[cnt[tid]] = total;
    hdr->total = total;
    hdr->n_lead = cnt[tid];
    hdr->n_dest = 0;
  }
}

// last position i of [lo, hi] with lpre[i] <= e (lpre[lo] <= e is given)
__device__ __forceinline__ int row_of_entry(const int64_t* __restrict__ lpre, int lo, int hi, int64_t e) {
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lpre[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The rows of the leaders laid end to end are hdr->total entries; block g takes the g-th of kWalkBlocks equal shares,
// wherever the row boundaries fall.  SCATTER = false: hist[g][bucket] = its entries per bucket of destinations.
// true: hist[g][bucket] holds the count of the blocks before (hop_offsets_kernel) and tot the buckets' totals; the block
// takes the buckets' starts (prefix of tot), and every entry's record goes to the next free place of its bucket's range.
// LDS: one counter per bucket.
template <bool SCATTER>
__global__ __launch_bounds__(kWalkThreads) void hop_walk_kernel(GraphView g, const int32_t* __restrict__ lead, const int64_t* __restrict__ lpre,
                                                                const HopHeader* __restrict__ hdr, int n_buckets,
                                                                int32_t* __restrict__ hist, const int32_t* __restrict__ tot,
                                                                int32_t* __restrict__ bst, int32_t* __restrict__ dst,
                                                                int32_t* __restrict__ src, float* __restrict__ w, int32_t capacity,
                                                                int32_t* __restrict__ err) {
  extern __shared__ int32_t lds[];
  __shared__ int32_t part[kWalkThreads];
  __shared__ int s_lo, s_hi;
  int32_t* bin = lds;
  const int tid = threadIdx.x;
  const int64_t total = hdr->total;
  const int n_lead = hdr->n_lead;
  int32_t* mine = hist + static_cast<int64_t>(blockIdx.x) * n_buckets;
  if constexpr (SCATTER) {
    const int per = (n_buckets + kWalkThreads - 1) / kWalkThreads;
    const int k0 = min(tid * per, n_buckets), k1 = min(k0 + per, n_buckets);
    int32_t sum = 0;
    for (int k = k0; k < k1; ++k) sum += tot[k];
    part[tid] = sum;
    __syncthreads();
    block_scan<int32_t, kWalkThreads>(part, tid);
    int32_t run = part[tid] - sum;
    for (int k = k0; k < k1; ++k) {
      bin[k] = run + mine[k];
      if (blockIdx.x == 0) bst[k] = run;
      run += tot[k];
    }
    if (blockIdx.x == 0 && tid == kWalkThreads - 1) bst[n_buckets] = part[tid];
  } else {
    for (int k = tid; k < n_buckets; k += kWalkThreads) bin[k] = 0;
  }
  const int64_t e0 = total * blockIdx.x / gridDim.x, e1 = total * (blockIdx.x + 1) / gridDim.x;
  if (e1 > e0) {                                    // (uniform over the block)
    if (tid == 0) s_lo = row_of_entry(lpre, 0, n_lead - 1, e0);
    if (tid == 1) s_hi = row_of_entry(lpre, 0, n_lead - 1, e1 - 1);
  }
  __syncthreads();
  if (e1 > e0) {
    const int lo = s_lo, hi = s_hi;
#pragma unroll 4
    for (int64_t e = e0 + tid; e < e1; e += kWalkThreads) {
      const int i = row_of_entry(lpre, lo, hi, e);
      const int32_t b = lead[i];
      const int64_t ge = g.rowptr[b] + (e - lpre[i]);
      const int32_t j = g.col[ge];
      const int k = j >> kBucketShift;
      if constexpr (!SCATTER) {
        atomicAdd(bin + k, 1);
      } else {
        const int32_t pos = atomicAdd(bin + k, 1);
        if (pos < capacity) {
          dst[pos] = j;
          src[pos] = b;
          w[pos] = g.val[ge];
        } else {
          atomicOr(err, 1);                         // more records than the caller's bound: never written
        }
      }
    }
  }
  if constexpr (!SCATTER) {
    __syncthreads();
    for (int k = tid; k < n_buckets; k += kWalkThreads) mine[k] = bin[k];
  }
}

// One block per bucket, one thread per walk block: hist[g][k] becomes the count of the blocks before g, tot[k] the bucket's total.
__global__ __launch_bounds__(kWalkBlocks) void hop_offsets_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ tot, int n_buckets) {
  __shared__ int32_t part[kWalkBlocks];
  const int g = threadIdx.x;
  int32_t* p = hist + static_cast<int64_t>(g) * n_buckets + blockIdx.x;
  const int32_t v = *p;
  part[g] = v;
  __syncthreads();
  block_scan<int32_t, kWalkBlocks>(part, g);
  *p = part[g] - v;
  if (g == kWalkBlocks - 1) tot[blockIdx.x] = part[g];
}

// first position of lead[0 .. n) that is >= v
__device__ __forceinline__ int lower_bound(const int32_t* __restrict__ lead, int n, int64_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lead[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One block per bucket of kBucketRows destinations; its records sit in [bst[k], bst[k + 1]) of (dst, src, w) in any order.
// Counts per destination and their prefix in LDS; one `dest` entry per destination with a record and per leader without
// one; the records grouped by destination into (src_g, w_g); then every record moves to (segment start + its rank by source
// id) of (src, w): ascending sources inside a segment.  (Sources of a segment are distinct: leaders are distinct nodes and a
// CSR row stores a column once; equal sources, should a matrix store duplicates, are kept apart by their position.)  The
// block reads back what its own threads wrote to (src_g, w_g) through L2 (ld_l2), after a barrier.
__global__ __launch_bounds__(kBucketThreads) void hop_bucket_kernel(int64_t n_dst, const int32_t* __restrict__ lead, HopHeader* __restrict__ hdr,
                                                                    const int32_t* __restrict__ bst, const int32_t* __restrict__ dst,
                                                                    int32_t* src, float* w, int32_t* src_g, float* w_g,
                                                                    int32_t capacity, int4* __restrict__ dest, int32_t dest_cap,
                                                                    int32_t* __restrict__ err) {
  __shared__ int32_t cntL[kBucketRows], offL[kBucketRows], fillL[kBucketRows], listL[kBucketRows];
  __shared__ int32_t part[kBucketThreads];
  __shared__ int s_n, s_base;
  constexpr int kPer = kBucketRows / kBucketThreads;
  const int tid = threadIdx.x;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) << kBucketShift;
  const int W = static_cast<int>(min(static_cast<int64_t>(kBucketRows), n_dst - j0));
  const int32_t bs = min(bst[blockIdx.x], capacity), be = min(bst[blockIdx.x + 1], capacity);
  for (int t = tid; t < kBucketRows; t += kBucketThreads) cntL[t] = fillL[t] = 0;
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int32_t p = bs + tid; p < be; p += kBucketThreads) atomicAdd(cntL + (dst[p] - j0), 1);
  __syncthreads();
  int32_t sum = 0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) sum += cntL[tid * kPer + u];
  part[tid] = sum;
  __syncthreads();
  block_scan<int32_t, kBucketThreads>(part, tid);
  int32_t run = part[tid] - sum;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    offL[tid * kPer + u] = run;
    run += cntL[tid * kPer + u];
  }
  __syncthreads();
  for (int t = tid; t < W; t += kBucketThreads)
    if (cntL[t] > 0) listL[atomicAdd(&s_n, 1)] = t;
  const int n_lead = hdr->n_lead;
  const int l0 = lower_bound(lead, n_lead, j0), l1 = lower_bound(lead, n_lead, j0 + W);
  for (int i = l0 + tid; i < l1; i += kBucketThreads) {
    const int t = static_cast<int>(lead[i] - j0);
    if (cntL[t] == 0) listL[atomicAdd(&s_n, 1)] = t;
  }
  __syncthreads();
  const int n_app = s_n;
  if (tid == 0) s_base = n_app > 0 ? atomicAdd(&hdr->n_dest, n_app) : 0;
  __syncthreads();
  for (int a = tid; a < n_app; a += kBucketThreads) {
    const int t = listL[a];
    const int64_t p = static_cast<int64_t>(s_base) + a;
    if (p < dest_cap) dest[p] = make_int4(static_cast<int32_t>(j0 + t), bs + offL[t], cntL[t], 0);
    else atomicOr(err, 1);
  }
  for (int32_t p = bs + tid; p < be; p += kBucketThreads) {
    const int t = static_cast<int>(dst[p] - j0);
    const int32_t q = bs + offL[t] + atomicAdd(fillL + t, 1);
    src_g[q] = src[p];
    w_g[q] = w[p];
  }
  __syncthreads();                                  // (every store above has been acknowledged by L2 when the barrier opens)
  for (int32_t q = bs + tid; q < be; q += kBucketThreads) {
    int lo = 0, hi = W - 1;                         // the segment of q: the last t with offL[t] <= q - bs
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (offL[mid] <= q - bs) lo = mid; else hi = mid - 1;
    }
    const int32_t s = bs + offL[lo], e = s + cntL[lo];
    const int32_t b = ld_l2(src_g + q);
    int32_t rank = 0;
    for (int32_t o = s; o < e; ++o) {
      const int32_t v = ld_l2(src_g + o);
      rank += (v < b) || (v == b && o < q);
    }
    src[s + rank] = b;
    w[s + rank] = __int_as_float(ld_l2(reinterpret_cast<const int32_t*>(w_g) + q));
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

// Lane group q of a wave owns one entry of the destination list per pass of its block over the block's share.  A listed row is visited when its mask
// byte is set and it has records or an epilogue term; every other row -- listed or not -- is left unwritten with its
// out_flags byte as the caller zeroed it.  The entry of the next pass is fetched before the work of this one.
template <int LPR>
__global__ __launch_bounds__(kWavesPerBlock * kWave) void batch_hop_kernel(int64_t n_rows, const int64_t* __restrict__ rowptr, HopPlan pl,
                                                                            const float* __restrict__ X, HopEpi e) {
  constexpr int NPI = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = lane / LPR, c = lane % LPR;
  const int64_t n_dest = min(pl.hdr->n_dest, pl.dest_cap);
  // a block takes a contiguous share of the list (the plan appends bucket by bucket: neighbouring entries are rows of the
  // same 2048-row window, so the block's reads of mask, flags and row lengths and its stores stay inside a few pages)
  constexpr int stride = kWavesPerBlock * NPI;
  const int64_t share = (n_dest + gridDim.x - 1) / gridDim.x;
  const int64_t k1 = min(n_dest, (blockIdx.x + 1) * share);
  const float4* __restrict__ Xv = reinterpret_cast<const float4*>(X) + c;
  const int4 none = make_int4(-1, 0, 0, 0);
  int64_t k0 = blockIdx.x * share + (threadIdx.x >> 6) * NPI;
  int4 next = k0 + q < k1 ? pl.dest[k0 + q] : none;
  for (; k0 < k1; k0 += stride) {
    const int4 d = next;
    next = k0 + stride + q < k1 ? pl.dest[k0 + stride + q] : none;
    const int64_t r = d.x;
    bool valid = r >= 0 && r < n_rows && e.row_mask[r];
    const int32_t start = d.y;
    int32_t len = d.z;
    if (valid && len <= 0 && e.b_flags && !e.b_flags[r]) valid = false;
    if (!valid) len = 0;
    // a row the masked kernel cuts into chunks (its result there is not a plain chain): fp64 chain below
    const bool is_long = len > 0 && rowptr[r + 1] - rowptr[r] > kLongRow;
    const int32_t len_long = is_long ? len : 0;
    if (is_long) len = 0;
    int maxlen = len;
#pragma unroll
    for (int m = LPR; m < kWave; m <<= 1) maxlen = max(maxlen, __shfl_xor(maxlen, m));
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
    if (is_long) {                               // (no cross-lane traffic in here: lane groups may diverge)
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
    if (!valid) continue;                        // (whole lane groups skip: the group reductions below stay inside a group)
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
}

template <int LPR>
constexpr int hop_grid_rows() { return kHopBlocks * kWavesPerBlock * (kWave / LPR); }

template <int LPR>
int launch_hop(int64_t n_rows, const int64_t* rowptr, const HopPlan& pl, const float* X, const HopEpi& e, hipStream_t s) {
  batch_hop_kernel<LPR><<<kHopBlocks, kWavesPerBlock * kWave, 0, s>>>(n_rows, rowptr, pl, X, e);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

int check_shape(const char* who, int64_t n_rows, int64_t n_listed, int64_t capacity) {
  TAGREC_REQUIRE(n_rows >= 1 && n_rows <= kMaxNodes, std::string(who) + ": the matrix holds 1 .. 2^24 rows");
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
  hop_layout(n_rows, n_listed, capacity, &L);
  return static_cast<int64_t>(L.total);
}

extern "C" int tagrec_batch_hop_plan(const tagrec_graph* gt, const int64_t* rows, int64_t n_listed, int64_t capacity, void* ws,
                                     int64_t ws_bytes, int32_t* err, void* stream) {
  TAGREC_REQUIRE(gt != nullptr && rows != nullptr && ws != nullptr && err != nullptr, "batch_hop_plan: null pointer");
  // gt = the TRANSPOSE of the matrix the hop multiplies by: its row b lists the destinations of source b
  const int64_t n_dst = gt->n_cols;
  TAGREC_TRY(check_shape("batch_hop_plan", n_dst, n_listed, capacity));
  TAGREC_REQUIRE(gt->n_rows == n_dst, "batch_hop_plan: square matrix expected");   // (a leader may be a destination itself)
  TAGREC_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255u) == 0, "batch_hop_plan: the workspace must be 256-byte aligned");
  HopLayout L;
  hop_layout(n_dst, n_listed, capacity, &L);
  TAGREC_REQUIRE(ws_bytes >= static_cast<int64_t>(L.total), "batch_hop_plan: workspace smaller than tagrec_batch_hop_workspace(...)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  HopHeader* hdr = reinterpret_cast<HopHeader*>(base + L.hdr);
  int32_t* lead = reinterpret_cast<int32_t*>(base + L.lead);
  int64_t* lpre = reinterpret_cast<int64_t*>(base + L.lpre);
  int32_t* hist = reinterpret_cast<int32_t*>(base + L.hist);
  int32_t* tot = reinterpret_cast<int32_t*>(base + L.tot);
  int32_t* bst = reinterpret_cast<int32_t*>(base + L.bst);
  int32_t* dst = reinterpret_cast<int32_t*>(base + L.dst);
  int32_t* src = reinterpret_cast<int32_t*>(base + L.src);
  float* w = reinterpret_cast<float*>(base + L.w);
  const GraphView gv = view_of(gt);
  const int32_t cap = static_cast<int32_t>(capacity);
  const int nb = static_cast<int>(L.n_buckets);
  const size_t walk_lds = static_cast<size_t>(nb) * sizeof(int32_t);
  hop_leader_kernel<<<1, kLeadThreads, 0, s>>>(gv, rows, static_cast<int>(n_listed), lead, lpre, hdr, err);
  TAGREC_LAUNCH_CHECK();
  hop_walk_kernel<false><<<kWalkBlocks, kWalkThreads, walk_lds, s>>>(gv, lead, lpre, hdr, nb, hist, tot, bst, dst, src, w, cap, err);
  TAGREC_LAUNCH_CHECK();
  hop_offsets_kernel<<<nb, kWalkBlocks, 0, s>>>(hist, tot, nb);
  TAGREC_LAUNCH_CHECK();
  hop_walk_kernel<true><<<kWalkBlocks, kWalkThreads, walk_lds, s>>>(gv, lead, lpre, hdr, nb, hist, tot, bst, dst, src, w, cap, err);
  TAGREC_LAUNCH_CHECK();
  hop_bucket_kernel<<<nb, kBucketThreads, 0, s>>>(n_dst, lead, hdr, bst, dst, src, w, reinterpret_cast<int32_t*>(base + L.src_g),
                                                  reinterpret_cast<float*>(base + L.w_g), cap, reinterpret_cast<int4*>(base + L.dest),
                                                  static_cast<int32_t>(L.dest_cap), err);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int64_t tagrec_batch_hop_list_result(int64_t n_rows, int64_t n_listed, int64_t capacity, int what) {
  if (check_shape("batch_hop_list_result", n_rows, n_listed, capacity) != TAGREC_OK) return -1;
  HopLayout L;
  hop_layout(n_rows, n_listed, capacity, &L);
  switch (what) {
    case 0: return static_cast<int64_t>(L.hdr + offsetof(HopHeader, n_dest));
    case 1: return static_cast<int64_t>(L.dest);
    case 2: return L.dest_cap;
    default: return -1;
  }
}

extern "C" int tagrec_batch_hop_grid_rows(int D) {
  if (!is_vec_width(D)) return 0;
  return vec_width_dispatch(D, "batch_hop_grid_rows", [](auto lc) { return hop_grid_rows<decltype(lc)::value>(); });
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
  TAGREC_TRY(check_shape("batch_hop_normbwd", g->n_rows, n_listed, capacity));
  HopLayout L;
  hop_layout(g->n_rows, n_listed, capacity, &L);
  TAGREC_REQUIRE(ws_bytes >= static_cast<int64_t>(L.total), "batch_hop_normbwd: workspace smaller than tagrec_batch_hop_workspace(...)");
  const char* base = static_cast<const char*>(ws);
  const HopPlan pl{reinterpret_cast<const int32_t*>(base + L.src), reinterpret_cast<const float*>(base + L.w),
                   reinterpret_cast<const int4*>(base + L.dest), reinterpret_cast<const HopHeader*>(base + L.hdr),
                   static_cast<int32_t>(L.dest_cap)};
  const HopEpi e{G_out, inv_norm, X_raw, dZ, d_scale, DropMask{0.f, 0}, out_flags, row_mask, dz_flags};
  hipStream_t s = static_cast<hipStream_t>(stream);
  return vec_width_dispatch(D, "batch_hop_normbwd", [&](auto lc) { return launch_hop<decltype(lc)::value>(g->n_rows, g->rowptr, pl, G_in, e, s); });
}
