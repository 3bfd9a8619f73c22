// Item co-occurrence top-k: row i of the sparse A^T A (A = the user x item train matrix, 0 / 1), reduced on the fly to the k
// heaviest columns.  The dense n_item x n_item product is never formed.
//
//   c_ij  = |N(i) n N(j)| (common users), c_ii = deg(i) -- or 0 with zero_diagonal
//   D_i   = sum_j c_ij = sum_{u in N(i)} deg(u) [- deg(i)]            (cooc_degree_kernel, int64)
//   order = descending key c_ij^2 / (D_j + 1) in fp64 (c^2 and D + 1 are exact, the division is IEEE), ties to the lower id
//   w_ij  = c_ij sqrt(D_i + 1) / D_i / sqrt(D_j + 1), formed in fp64 and rounded once to fp32
//
// Row i is the walk "every user u of i, every item j of u": D_i visits.  Counts are integers and are accumulated with integer
// atomics only, so a row does not depend on the order its visits arrive in.  Two tiers, chosen per item by D_i:
//   light (D_i <= lds_limit <= 4096)  one block per item; an open-addressing (id, count) table in LDS with 2^m >= 2 D_i slots
//                                     (load <= 1/2): compare-and-swap on the id, add on the count; then a scan of the table
//   heavy                             one dense int32 counter row of n_item entries per resident block (caller's workspace,
//                                     all zero): the walk adds with global atomics, a barrier, then the SAME walk exchanges
//                                     every counter it meets with zero -- the one visit that gets a non-zero back owns that
//                                     candidate.  The row is zero again for the block's next item, no plain load reads a
//                                     counter, and the cost follows D_i, not n_item.
//   hub                               a heavy item whose walk alone would outlast the rest of the tier is cut into parts, one
//                                     block each, over three launches (add, take, merge): see HubParts below.
// All tiers feed the same threshold-gated candidate list in LDS (the pattern of eval.hip's top-k): a candidate that does not
// beat the current k-th best is dropped at once, the list is cut back to its k best (rank by counting: (key, id) is a total
// order, so a rank is a position) whenever another 256 pushes might not fit.
#include <algorithm>

#include "common.h"

namespace tagrec {
namespace {

constexpr int kT = 256;                  // threads per block
constexpr int kLdsLimit = 4096;          // largest D_i of the light tier
constexpr int kTable = 2 * kLdsLimit;    // slots of the LDS table at that limit
constexpr int kCap = 512;                // candidate list: at most kCap - kT entries before a round of kT pushes
constexpr int kMaxK = 64;
constexpr int kMaxRows = 2048;           // resident blocks of the heavy tier

struct Sel {
  double key[kCap];
  int id[kCap];
  int c[kCap];
  int n;
  int has_thr;
  int thr_id;
  double thr_key;
};

struct Group {                           // the users of one walk group: where their item lists start and the running length
  int64_t p0[kT];
  int64_t end[kT];
  int64_t wave_tot[kT / kWave];
};

struct Csr {
  const int64_t* iu_ptr; const int32_t* iu_idx;      // item -> users
  const int64_t* ui_ptr; const int32_t* ui_idx;      // user -> items
};

__device__ __forceinline__ bool better(double ka, int ia, double kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

__device__ __forceinline__ double cooc_key(int c, int64_t dj) {
  return (static_cast<double>(c) * static_cast<double>(c)) / static_cast<double>(dj + 1);
}

__device__ __forceinline__ void sel_push(Sel& s, double key, int id, int c) {
  if (s.has_thr && !better(key, id, s.thr_key, s.thr_id)) return;
  const int pos = atomicAdd(&s.n, 1);
  if (pos < kCap) { s.key[pos] = key; s.id[pos] = id; s.c[pos] = c; }     // (always: see sel_round)
}

// Cut the list back to its k best, in order.  Every thread of the block calls it, after a barrier.
__device__ void sel_prune(Sel& s, int k) {
  const int n = min(s.n, kCap);
  double mk[kCap / kT]; int mi[kCap / kT], mc[kCap / kT], rk[kCap / kT];
#pragma unroll
  for (int e = 0; e < kCap / kT; ++e) {
    const int at = threadIdx.x + e * kT;
    rk[e] = kCap;
    if (at < n) {
      mk[e] = s.key[at]; mi[e] = s.id[at]; mc[e] = s.c[at];
      int r = 0;
      for (int t = 0; t < n; ++t) r += better(s.key[t], s.id[t], mk[e], mi[e]) ? 1 : 0;
      rk[e] = r;
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < kCap / kT; ++e)
    if (rk[e] < k) { s.key[rk[e]] = mk[e]; s.id[rk[e]] = mi[e]; s.c[rk[e]] = mc[e]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    s.n = min(n, k);
    if (n >= k) { s.has_thr = 1; s.thr_key = s.key[k - 1]; s.thr_id = s.id[k - 1]; }
  }
  __syncthreads();
}

// The end of a round in which every thread pushed at most once: keep room for the next round.
__device__ __forceinline__ void sel_round(Sel& s, int k) {
  // (the thread that pushed last reads the full count, so the OR is the same for every thread; a plain read behind a barrier
  // would race with the next round's pushes)
  if (__syncthreads_or(s.n > kCap - kT)) sel_prune(s, k);
}

__device__ void sel_reset(Sel& s) {
  if (threadIdx.x == 0) { s.n = 0; s.has_thr = 0; }
}

// The sorted list -> row i of the outputs, pads behind it.  After sel_prune.
__device__ void sel_write(const Sel& s, int k, int64_t i, int64_t Di, const int64_t* __restrict__ D, int32_t* __restrict__ nbr_id,
                          float* __restrict__ nbr_w) {
  const int t = threadIdx.x;
  if (t >= k) return;
  int id = -1;
  float w = 0.f;
  if (t < s.n) {
    id = s.id[t];
    w = static_cast<float>(static_cast<double>(s.c[t]) * sqrt(static_cast<double>(Di + 1)) / static_cast<double>(Di) /
                           sqrt(static_cast<double>(D[id] + 1)));
  }
  nbr_id[i * k + t] = id;
  nbr_w[i * k + t] = w;
}

__device__ void write_pads(int k, int64_t i, int32_t* __restrict__ nbr_id, float* __restrict__ nbr_w) {
  if (static_cast<int>(threadIdx.x) < k) { nbr_id[i * k + threadIdx.x] = -1; nbr_w[i * k + threadIdx.x] = 0.f; }
}

// What a visit of the walk does with the item id it meets.
struct LdsInsert {                       // light tier: count in the LDS table
  int* t_id; int* t_c; int mask;
  static constexpr bool kRounds = false;
  __device__ __forceinline__ void operator()(int j) const {
    int slot = j & mask;
    for (int probes = 0; probes <= mask; ++probes) {           // load <= 1/2: an empty slot is met long before
      const int old = atomicCAS(&t_id[slot], -1, j);
      if (old == -1 || old == j) { atomicAdd(&t_c[slot], 1); return; }
      slot = (slot + 1) & mask;
    }
  }
};
struct RowAdd {                          // heavy tier, first walk
  int* row;
  static constexpr bool kRounds = false;
  __device__ __forceinline__ void operator()(int j) const { atomicAdd(&row[j], 1); }
};
struct RowTake {                         // heavy tier, second walk: the visit that gets the count back owns the candidate
  int* row; Sel* sel; const int64_t* D;
  static constexpr bool kRounds = true;
  __device__ __forceinline__ void operator()(int j) const {
    const int c = atomicExch(&row[j], 0);
    if (c > 0) sel_push(*sel, cooc_key(c, D[j]), j, c);
  }
};

// Every (user u, item j of u) pair once for the users iu_idx[u0 .. u1) of an item, kT pairs per round, kT users per group; `skip` (zero_diagonal: i itself,
// else -1) is passed over.  Visitors with kRounds end every round with sel_round.
template <class Visit>
__device__ void walk_users(const Csr& g, int64_t u0, int64_t u1, int skip, Group& grp, const Visit& visit, Sel* sel, int k) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  for (int64_t gb = u0; gb < u1; gb += kT) {
    const int nu = u1 - gb < kT ? static_cast<int>(u1 - gb) : kT;
    int64_t len = 0;
    if (tid < nu) {
      const int u = g.iu_idx[gb + tid];
      const int64_t p = g.ui_ptr[u];
      len = g.ui_ptr[u + 1] - p;
      grp.p0[tid] = p;
    }
    int64_t run = len;                   // inclusive scan over the block: wave by shuffles, then the wave totals
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
      const int64_t up = __shfl_up(run, m);
      if (lane >= m) run += up;
    }
    if (lane == kWave - 1) grp.wave_tot[w] = run;
    __syncthreads();
    for (int q = 0; q < w; ++q) run += grp.wave_tot[q];
    grp.end[tid] = run;
    __syncthreads();
    const int64_t total = grp.end[nu - 1];
    for (int64_t v0 = 0; v0 < total; v0 += kT) {
      const int64_t v = v0 + tid;
      if (v < total) {
        int lo = 0, hi = nu - 1;         // the first user whose running length exceeds v
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (grp.end[mid] > v) hi = mid; else lo = mid + 1;
        }
        const int64_t start = lo ? grp.end[lo - 1] : 0;
        const int j = g.ui_idx[grp.p0[lo] + (v - start)];
        if (j != skip) visit(j);
      }
      if (Visit::kRounds) sel_round(*sel, k);
    }
    __syncthreads();                     // the group's arrays are rewritten by the next one
  }
}

template <class Visit>
__device__ void walk(const Csr& g, int64_t i, int skip, Group& grp, const Visit& visit, Sel* sel, int k) {
  walk_users(g, g.iu_ptr[i], g.iu_ptr[i + 1], skip, grp, visit, sel, k);
}

__global__ __launch_bounds__(kT) void cooc_degree_kernel(const int64_t* __restrict__ iu_ptr, const int32_t* __restrict__ iu_idx,
                                                         const int64_t* __restrict__ ui_ptr, int64_t n_item, int zero_diagonal,
                                                         int64_t* __restrict__ D) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * (kT / kWave) + (threadIdx.x >> 6);
  if (i >= n_item) return;
  const int64_t u0 = iu_ptr[i], u1 = iu_ptr[i + 1];
  int64_t s = 0;
  for (int64_t p = u0 + lane; p < u1; p += kWave) {
    const int u = iu_idx[p];
    s += ui_ptr[u + 1] - ui_ptr[u];
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) s += __shfl_xor(s, m);
  if (lane == 0) D[i] = s - (zero_diagonal ? u1 - u0 : 0);
}

__global__ __launch_bounds__(kT) void cooc_light_kernel(Csr g, const int64_t* __restrict__ D, const int32_t* __restrict__ items,
                                                        int k, int zero_diagonal, int32_t* __restrict__ nbr_id,
                                                        float* __restrict__ nbr_w) {
  __shared__ int t_id[kTable];
  __shared__ int t_c[kTable];
  __shared__ Sel sel;
  __shared__ Group grp;
  const int64_t i = items[blockIdx.x];
  const int64_t Di = D[i];
  if (Di <= 0 || Di > kLdsLimit) {       // nothing to rank (an item above the limit is never listed by the host side)
    write_pads(k, i, nbr_id, nbr_w);
    return;
  }
  int tsize = kT;
  while (tsize < 2 * Di) tsize <<= 1;    // <= kTable
  for (int s = threadIdx.x; s < tsize; s += kT) { t_id[s] = -1; t_c[s] = 0; }
  sel_reset(sel);
  __syncthreads();
  walk(g, i, zero_diagonal ? static_cast<int>(i) : -1, grp, LdsInsert{t_id, t_c, tsize - 1}, static_cast<Sel*>(nullptr), k);
  __syncthreads();
  for (int base = 0; base < tsize; base += kT) {
    const int id = t_id[base + threadIdx.x];
    if (id >= 0) {
      const int c = t_c[base + threadIdx.x];
      sel_push(sel, cooc_key(c, D[id]), id, c);
    }
    sel_round(sel, k);
  }
  sel_prune(sel, k);
  sel_write(sel, k, i, Di, D, nbr_id, nbr_w);
}

__global__ __launch_bounds__(kT) void cooc_heavy_kernel(Csr g, const int64_t* __restrict__ D, const int32_t* __restrict__ items,
                                                        int64_t n_listed, int64_t n_item, int k, int zero_diagonal,
                                                        int* __restrict__ workspace, int32_t* __restrict__ nbr_id,
                                                        float* __restrict__ nbr_w) {
  __shared__ Sel sel;
  __shared__ Group grp;
  int* row = workspace + static_cast<int64_t>(blockIdx.x) * n_item;
  for (int64_t it = blockIdx.x; it < n_listed; it += gridDim.x) {
    const int64_t i = items[it];
    const int64_t Di = D[i];
    if (Di <= 0) {
      write_pads(k, i, nbr_id, nbr_w);
      continue;
    }
    const int skip = zero_diagonal ? static_cast<int>(i) : -1;
    sel_reset(sel);
    __syncthreads();
    walk(g, i, skip, grp, RowAdd{row}, static_cast<Sel*>(nullptr), k);
    __threadfence();                     // every add has landed before the first exchange
    __syncthreads();
    walk(g, i, skip, grp, RowTake{row, &sel, D}, &sel, k);
    sel_prune(sel, k);
    sel_write(sel, k, i, Di, D, nbr_id, nbr_w);
    __syncthreads();
  }
}

// Hub items (the largest D_i): ONE item's walk is cut into parts -- contiguous slices [part_u0, part_u1) of its user list -- and
// every part is a block.  All parts of a hub share the hub's counter row; the barrier between the add walk and the take walk is
// the boundary between two launches.  A candidate is still owned by the one visit that gets its count back, so the parts' lists
// are disjoint, each part keeps its own k best, and the hub's k best are among them: a third launch merges them.
struct HubParts {
  const int32_t* hub_items;        // [n_hub] item ids
  const int32_t* part_hub;         // [n_part] index into hub_items
  const int64_t* part_u0;          // [n_part] slice of iu_idx
  const int64_t* part_u1;
  const int64_t* hub_part_ptr;     // [n_hub + 1] the parts of a hub
};

__global__ __launch_bounds__(kT) void cooc_hub_add_kernel(Csr g, HubParts hp, int64_t n_item, int zero_diagonal,
                                                          int* __restrict__ workspace) {
  __shared__ Group grp;
  const int64_t p = blockIdx.x;
  const int h = hp.part_hub[p];
  const int i = hp.hub_items[h];
  walk_users(g, hp.part_u0[p], hp.part_u1[p], zero_diagonal ? i : -1, grp, RowAdd{workspace + static_cast<int64_t>(h) * n_item},
             static_cast<Sel*>(nullptr), 0);
}

__global__ __launch_bounds__(kT) void cooc_hub_take_kernel(Csr g, HubParts hp, const int64_t* __restrict__ D, int64_t n_item, int k,
                                                           int zero_diagonal, int* __restrict__ workspace,
                                                           int32_t* __restrict__ part_id, int32_t* __restrict__ part_c) {
  __shared__ Sel sel;
  __shared__ Group grp;
  const int64_t p = blockIdx.x;
  const int h = hp.part_hub[p];
  const int i = hp.hub_items[h];
  sel_reset(sel);
  __syncthreads();
  walk_users(g, hp.part_u0[p], hp.part_u1[p], zero_diagonal ? i : -1, grp,
             RowTake{workspace + static_cast<int64_t>(h) * n_item, &sel, D}, &sel, k);
  sel_prune(sel, k);
  const int t = threadIdx.x;
  if (t < k) {
    part_id[p * k + t] = t < sel.n ? sel.id[t] : -1;
    part_c[p * k + t] = t < sel.n ? sel.c[t] : 0;
  }
}

__global__ __launch_bounds__(kT) void cooc_hub_merge_kernel(HubParts hp, const int64_t* __restrict__ D, int k,
                                                            const int32_t* __restrict__ part_id, const int32_t* __restrict__ part_c,
                                                            int32_t* __restrict__ nbr_id, float* __restrict__ nbr_w) {
  __shared__ Sel sel;
  const int h = blockIdx.x;
  const int64_t i = hp.hub_items[h];
  const int64_t Di = D[i];
  if (Di <= 0) {
    write_pads(k, i, nbr_id, nbr_w);
    return;
  }
  const int64_t a = hp.hub_part_ptr[h] * k, b = hp.hub_part_ptr[h + 1] * k;
  sel_reset(sel);
  __syncthreads();
  for (int64_t base = a; base < b; base += kT) {
    const int64_t at = base + threadIdx.x;
    if (at < b) {
      const int id = part_id[at];
      if (id >= 0) sel_push(sel, cooc_key(part_c[at], D[id]), id, part_c[at]);
    }
    sel_round(sel, k);
  }
  sel_prune(sel, k);
  sel_write(sel, k, i, Di, D, nbr_id, nbr_w);
}

int check_csr(const char* what, const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, const int32_t* ui_idx) {
  if (!iu_ptr || !iu_idx || !ui_ptr || !ui_idx) return fail(TAGREC_E_INVALID, std::string(what) + ": null pointer");
  return TAGREC_OK;
}

}  // namespace

extern "C" int tagrec_cooc_lds_limit(void) { return kLdsLimit; }

extern "C" int tagrec_cooc_degree_i64(const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, int64_t n_item,
                                      int zero_diagonal, int64_t* D, void* stream) {
  TAGREC_REQUIRE(iu_ptr && iu_idx && ui_ptr && D, "cooc_degree: null pointer");
  TAGREC_REQUIRE(n_item >= 1 && n_item <= 2147483647ll, "cooc_degree: n_item must be in 1 .. 2^31 - 1");
  const int64_t blocks = (n_item + kT / kWave - 1) / (kT / kWave);
  cooc_degree_kernel<<<static_cast<unsigned>(blocks), kT, 0, static_cast<hipStream_t>(stream)>>>(iu_ptr, iu_idx, ui_ptr, n_item,
                                                                                                  zero_diagonal, D);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_cooc_topk_light_f32(const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, const int32_t* ui_idx,
                                          const int64_t* D, const int32_t* items, int64_t n_listed, int64_t n_item, int k,
                                          int zero_diagonal, int32_t* nbr_id, float* nbr_w, void* stream) {
  TAGREC_TRY(check_csr("cooc_topk_light", iu_ptr, iu_idx, ui_ptr, ui_idx));
  TAGREC_REQUIRE(D && nbr_id && nbr_w, "cooc_topk_light: null pointer");
  TAGREC_REQUIRE(k >= 1 && k <= kMaxK, "cooc_topk_light: k must be in 1 .. 64");
  TAGREC_REQUIRE(n_item >= 1 && n_item <= 2147483647ll && n_listed >= 0 && n_listed <= n_item, "cooc_topk_light: bad shape");
  if (n_listed == 0) return TAGREC_OK;
  TAGREC_REQUIRE(items, "cooc_topk_light: null item list");
  const Csr g{iu_ptr, iu_idx, ui_ptr, ui_idx};
  cooc_light_kernel<<<static_cast<unsigned>(n_listed), kT, 0, static_cast<hipStream_t>(stream)>>>(g, D, items, k, zero_diagonal,
                                                                                                   nbr_id, nbr_w);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_cooc_topk_heavy_f32(const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, const int32_t* ui_idx,
                                          const int64_t* D, const int32_t* items, int64_t n_listed, int64_t n_item, int k,
                                          int zero_diagonal, int32_t* workspace, int64_t rows, int32_t* nbr_id, float* nbr_w,
                                          void* stream) {
  TAGREC_TRY(check_csr("cooc_topk_heavy", iu_ptr, iu_idx, ui_ptr, ui_idx));
  TAGREC_REQUIRE(D && nbr_id && nbr_w, "cooc_topk_heavy: null pointer");
  TAGREC_REQUIRE(k >= 1 && k <= kMaxK, "cooc_topk_heavy: k must be in 1 .. 64");
  TAGREC_REQUIRE(n_item >= 1 && n_item <= 2147483647ll && n_listed >= 0 && n_listed <= n_item, "cooc_topk_heavy: bad shape");
  if (n_listed == 0) return TAGREC_OK;
  TAGREC_REQUIRE(items, "cooc_topk_heavy: null item list");
  TAGREC_REQUIRE(workspace && rows >= 1, "cooc_topk_heavy: the workspace must hold at least one zeroed counter row of n_item int32");
  const int64_t blocks = std::min<int64_t>(std::min<int64_t>(rows, n_listed), kMaxRows);
  const Csr g{iu_ptr, iu_idx, ui_ptr, ui_idx};
  cooc_heavy_kernel<<<static_cast<unsigned>(blocks), kT, 0, static_cast<hipStream_t>(stream)>>>(g, D, items, n_listed, n_item, k,
                                                                                                 zero_diagonal, workspace, nbr_id,
                                                                                                 nbr_w);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_cooc_topk_hub_f32(const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, const int32_t* ui_idx,
                                        const int64_t* D, const int32_t* hub_items, int64_t n_hub, const int32_t* part_hub,
                                        const int64_t* part_u0, const int64_t* part_u1, int64_t n_part, const int64_t* hub_part_ptr,
                                        int64_t n_item, int k, int zero_diagonal, int32_t* workspace, int32_t* part_id,
                                        int32_t* part_c, int32_t* nbr_id, float* nbr_w, void* stream) {
  TAGREC_TRY(check_csr("cooc_topk_hub", iu_ptr, iu_idx, ui_ptr, ui_idx));
  TAGREC_REQUIRE(D && nbr_id && nbr_w, "cooc_topk_hub: null pointer");
  TAGREC_REQUIRE(k >= 1 && k <= kMaxK, "cooc_topk_hub: k must be in 1 .. 64");
  TAGREC_REQUIRE(n_item >= 1 && n_item <= 2147483647ll && n_hub >= 0 && n_hub <= n_item, "cooc_topk_hub: bad shape");
  if (n_hub == 0) return TAGREC_OK;
  TAGREC_REQUIRE(n_part >= n_hub && n_part <= 2147483647ll, "cooc_topk_hub: every hub needs at least one part");
  TAGREC_REQUIRE(hub_items && part_hub && part_u0 && part_u1 && hub_part_ptr && workspace && part_id && part_c,
                 "cooc_topk_hub: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Csr g{iu_ptr, iu_idx, ui_ptr, ui_idx};
  const HubParts hp{hub_items, part_hub, part_u0, part_u1, hub_part_ptr};
  cooc_hub_add_kernel<<<static_cast<unsigned>(n_part), kT, 0, s>>>(g, hp, n_item, zero_diagonal, workspace);
  TAGREC_LAUNCH_CHECK();
  cooc_hub_take_kernel<<<static_cast<unsigned>(n_part), kT, 0, s>>>(g, hp, D, n_item, k, zero_diagonal, workspace, part_id, part_c);
  TAGREC_LAUNCH_CHECK();
  cooc_hub_merge_kernel<<<static_cast<unsigned>(n_hub), kT, 0, s>>>(hp, D, k, part_id, part_c, nbr_id, nbr_w);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_cooc_max_rows(void) { return kMaxRows; }

}  // namespace tagrec
