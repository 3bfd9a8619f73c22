// K24: row-sparse Adam that is the dense optimizer's, bit for bit.  A row without a gradient still moves under dense Adam --
// m and v decay, p follows the old m -- but that move, adam_update(g = 0), is a function of the row's own state and of two
// per-step scalars.  So the row is left alone (`last[r]` = the last optimizer step applied to it) and the skipped steps are
// replayed in registers, in order, when something next reads it:
//
//   ring    : float pairs (step_size_t, bc2_sqrt_t) of step t at entry t mod capacity, device memory, filled ahead by the host
//             in blocks (tagrec_adam_coef: the arithmetic of tagrec_adam_f32, common.h's adam_step_coef)
//   catch-up: the distinct rows of a row-list plan (rowlist.h) are replayed from last[r] + 1 to t_done      (forward pass)
//   apply   : the segment sums of the compact gradient, in row_scatter_ordered's documented order (scatter_column of
//             rowlist.h -- the same device code), go through ONE adam_update of step t = last[r] + 1        (optimizer step)
//   flush   : every row of the table with last[r] < t_done is replayed to t_done; a row that is current costs its 4 bytes of
//             `last`, and a lane whose m and v are all +0 bits skips its loop and its p (a zero-gradient step leaves such an
//             element as it is, exactly: this is every row that was never named)
//
// Ring reads.  The replay's step index differs from row to row of a wave, so it cannot be a scalar load; reading the ring
// from global memory would make every lane of every iteration a load of its own.  A block therefore copies the window of
// steps (t_floor, t_done] into LDS once -- t_floor: a lower bound of `last` that the caller keeps, the step of its last
// flush -- and walks over its rows grid-stride; an iteration reads one 8-byte LDS word, the same address within a lane
// group (a broadcast).  The apply kernel needs one entry, at an index formed from kernel arguments alone: a uniform load.
//
// No float atomics.  Nothing here reads the host.
#include "rowlist.h"

namespace tagrec {
namespace {

constexpr int kMaxWindow = 4096;         // steps a replay can span: 32 KB of LDS
constexpr int kMaxBlocks = 2048;         // grid-stride: a block stages the window once for all its rows

struct RowAdamTable {
  float* p; float* m; float* v;
  int64_t ld;                 // row stride (floats)
  int32_t* last;              // [n_rows]
  int64_t n_rows;
  int D;
  const float2* ring;         // [cap] (step_size, bc2_sqrt) of step t at t mod cap
  int64_t cap;
  float w1, b2, w2, eps;
};

__device__ __forceinline__ bool zero_bits(float m, float v) { return (__float_as_uint(m) | __float_as_uint(v)) == 0u; }
__device__ __forceinline__ bool zero_bits(const adam_f4& m, const adam_f4& v) {
  return ((__float_as_uint(m[0]) | __float_as_uint(m[1]) | __float_as_uint(m[2]) | __float_as_uint(m[3])) |
          (__float_as_uint(v[0]) | __float_as_uint(v[1]) | __float_as_uint(v[2]) | __float_as_uint(v[3]))) == 0u;
}
__device__ __forceinline__ float zero_grad_step(float& m, float& v, float p, const RowAdamTable& tb, const float2 c) {
  return adam_update1(m, v, p, 0.f, tb.w1, tb.b2, tb.w2, c.x, c.y, tb.eps);
}
__device__ __forceinline__ adam_f4 zero_grad_step(adam_f4& m, adam_f4& v, adam_f4 p, const RowAdamTable& tb, const float2 c) {
  const adam_f4 g = {0.f, 0.f, 0.f, 0.f};
  return adam_update(m, v, p, g, tb.w1, tb.b2, tb.w2, c.x, c.y, tb.eps);
}

// steps from + 1 .. t_done on one column (V = float) or one 16-byte column group (V = adam_f4); win[i] = step t_floor + 1 + i
template <typename V>
__device__ __forceinline__ void replay_column(V* __restrict__ p, V* __restrict__ m, V* __restrict__ v, const RowAdamTable& tb,
                                              const float2* win, int32_t from, int32_t t_floor, int32_t t_done) {
  V mi = *m, vi = *v;
  if (zero_bits(mi, vi)) return;
  V pi = *p;
  for (int32_t s = from; s < t_done; ++s) pi = zero_grad_step(mi, vi, pi, tb, win[s - t_floor]);
  *p = pi;
  *m = mi;
  *v = vi;
}

__device__ __forceinline__ void stage_window(const RowAdamTable& tb, float2* win, int32_t t_floor, int32_t t_done) {
  const int32_t W = t_done - t_floor;
  for (int32_t i = threadIdx.x; i < W; i += blockDim.x) win[i] = tb.ring[(static_cast<int64_t>(t_floor) + 1 + i) % tb.cap];
  __syncthreads();
}

// LISTED: entry idx of the plan's distinct rows (seg_row, counts); else row idx of the table.  -> the row, or -1: nothing to do
template <bool LISTED>
__device__ __forceinline__ int64_t replay_row(const RowAdamTable& tb, const int32_t* __restrict__ seg_row, int64_t idx) {
  if constexpr (!LISTED) return idx;
  const int64_t r = seg_row[idx];
  return r < tb.n_rows ? r : -1;
}

// Lane group q of a wave owns one row per pass of the grid-stride loop, lane c of the group its float4 column c.  Rows of a
// wave have different trip counts; a lane group's lanes share theirs.
template <int LPR, bool LISTED>
__global__ __launch_bounds__(kScatterWaves * kWave) void rowadam_replay_vec_kernel(RowAdamTable tb, const int32_t* __restrict__ seg_row,
                                                                                  const int32_t* __restrict__ counts, int32_t n_listed,
                                                                                  int32_t t_floor, int32_t t_done) {
  extern __shared__ float2 win[];
  stage_window(tb, win, t_floor, t_done);
  constexpr int NPI = kWave / LPR;
  constexpr int per_block = kScatterWaves * NPI;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = lane / LPR, c = lane % LPR;
  const int64_t n = LISTED ? static_cast<int64_t>(min(counts[kCountSegments], n_listed)) : tb.n_rows;
  const int64_t ld4 = tb.ld / 4;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * per_block + (threadIdx.x >> 6) * NPI + q; idx < n;
       idx += static_cast<int64_t>(gridDim.x) * per_block) {
    const int64_t r = replay_row<LISTED>(tb, seg_row, idx);
    if (r < 0) continue;
    const int32_t from = tb.last[r];
    if (from >= t_done) continue;                     // current: nothing of the row is read beyond `last`
    const int64_t at = r * ld4 + c;
    replay_column(reinterpret_cast<adam_f4*>(tb.p) + at, reinterpret_cast<adam_f4*>(tb.m) + at, reinterpret_cast<adam_f4*>(tb.v) + at,
                  tb, win, max(from, t_floor), t_floor, t_done);
    if (c == 0) tb.last[r] = t_done;                  // (after the group's lanes have read it: the loop above hangs on it)
  }
}

// Any width: one wavefront per row, lane c takes columns c, c + 64, ...
template <bool LISTED>
__global__ __launch_bounds__(kScatterWaves * kWave) void rowadam_replay_scalar_kernel(RowAdamTable tb, const int32_t* __restrict__ seg_row,
                                                                                     const int32_t* __restrict__ counts, int32_t n_listed,
                                                                                     int32_t t_floor, int32_t t_done) {
  extern __shared__ float2 win[];
  stage_window(tb, win, t_floor, t_done);
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t n = LISTED ? static_cast<int64_t>(min(counts[kCountSegments], n_listed)) : tb.n_rows;
  for (int64_t idx = static_cast<int64_t>(blockIdx.x) * kScatterWaves + (threadIdx.x >> 6); idx < n;
       idx += static_cast<int64_t>(gridDim.x) * kScatterWaves) {
    const int64_t r = replay_row<LISTED>(tb, seg_row, idx);
    if (r < 0) continue;
    const int32_t from = tb.last[r];
    if (from >= t_done) continue;
    for (int c = lane; c < tb.D; c += kWave) {
      const int64_t at = r * tb.ld + c;
      replay_column(tb.p + at, tb.m + at, tb.v + at, tb, win, max(from, t_floor), t_floor, t_done);
    }
    if (lane == 0) tb.last[r] = t_done;
  }
}

template <int LPR, bool LISTED>
int launch_replay_vec(const RowAdamTable& tb, const int32_t* seg_row, const int32_t* counts, int64_t n_bound, int32_t t_floor,
                      int32_t t_done, hipStream_t s) {
  constexpr int per_block = kScatterWaves * (kWave / LPR);
  const int64_t tiles = (n_bound + per_block - 1) / per_block;
  const unsigned blocks = static_cast<unsigned>(tiles < kMaxBlocks ? tiles : kMaxBlocks);
  const size_t lds = static_cast<size_t>(t_done - t_floor) * sizeof(float2);
  rowadam_replay_vec_kernel<LPR, LISTED><<<blocks, kScatterWaves * kWave, lds, s>>>(tb, seg_row, counts, LISTED ? static_cast<int32_t>(n_bound) : 0,
                                                                                   t_floor, t_done);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

template <bool LISTED>
int launch_replay(const RowAdamTable& tb, const int32_t* seg_row, const int32_t* counts, int64_t n_bound, int32_t t_floor, int32_t t_done,
                  hipStream_t s) {
  const bool vec = aligned16(tb.p) && aligned16(tb.m) && aligned16(tb.v) && tb.ld % 4 == 0;
  if (vec) {
    switch (tb.D) {
      case 8: return launch_replay_vec<2, LISTED>(tb, seg_row, counts, n_bound, t_floor, t_done, s);
      case 16: return launch_replay_vec<4, LISTED>(tb, seg_row, counts, n_bound, t_floor, t_done, s);
      case 32: return launch_replay_vec<8, LISTED>(tb, seg_row, counts, n_bound, t_floor, t_done, s);
      case 64: return launch_replay_vec<16, LISTED>(tb, seg_row, counts, n_bound, t_floor, t_done, s);
      case 128: return launch_replay_vec<32, LISTED>(tb, seg_row, counts, n_bound, t_floor, t_done, s);
      case 256: return launch_replay_vec<64, LISTED>(tb, seg_row, counts, n_bound, t_floor, t_done, s);
      default: break;
    }
  }
  const int64_t tiles = (n_bound + kScatterWaves - 1) / kScatterWaves;
  const unsigned blocks = static_cast<unsigned>(tiles < kMaxBlocks ? tiles : kMaxBlocks);
  const size_t lds = static_cast<size_t>(t_done - t_floor) * sizeof(float2);
  rowadam_replay_scalar_kernel<LISTED><<<blocks, kScatterWaves * kWave, lds, s>>>(tb, seg_row, counts, LISTED ? static_cast<int32_t>(n_bound) : 0,
                                                                                 t_floor, t_done);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

// ---- apply: where scatter_column's finished segment sum lands is Adam's update of that row ----
struct LandAdam {
  RowAdamTable tb;
  float2 coef;                // of step t
  int32_t t;
  int c;                      // this lane's column (float) or column group (float4); lane 0 of a row also stores `last`
  __device__ __forceinline__ void operator()(int64_t row, const float4& acc) const {
    const int64_t at = row * (tb.ld / 4) + c;
    adam_f4* p = reinterpret_cast<adam_f4*>(tb.p) + at;
    adam_f4* m = reinterpret_cast<adam_f4*>(tb.m) + at;
    adam_f4* v = reinterpret_cast<adam_f4*>(tb.v) + at;
    const adam_f4 g = {acc.x, acc.y, acc.z, acc.w};
    adam_f4 mi = *m, vi = *v;
    *p = adam_update(mi, vi, *p, g, tb.w1, tb.b2, tb.w2, coef.x, coef.y, tb.eps);
    *m = mi;
    *v = vi;
    if (c == 0) tb.last[row] = t;
  }
  __device__ __forceinline__ void operator()(int64_t row, const float& acc) const {
    const int64_t at = row * tb.ld + c;
    float mi = tb.m[at], vi = tb.v[at];
    tb.p[at] = adam_update1(mi, vi, tb.p[at], acc, tb.w1, tb.b2, tb.w2, coef.x, coef.y, tb.eps);
    tb.m[at] = mi;
    tb.v[at] = vi;
    if (c == 0) tb.last[row] = t;
  }
};

// the geometry of row_scatter_vec_kernel / row_scatter_scalar_kernel (rowscatter.hip): lane group q of a wave owns sorted
// position (wave * NPI + q)
template <int LPR, bool FOLD>
__global__ __launch_bounds__(kScatterWaves * kWave) void rowadam_apply_vec_kernel(ScatterPlan pl, const float* __restrict__ src, int64_t lds,
                                                                                 float* __restrict__ slab, RowAdamTable tb, int32_t t) {
  constexpr int NPI = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int q = lane / LPR, c = lane % LPR;
  const int64_t wv = static_cast<int64_t>(blockIdx.x) * kScatterWaves + (threadIdx.x >> 6);
  const int64_t i = wv * NPI + q;
  if (i >= pl.n_listed || i >= pl.counts[kCountValid]) return;
  const float2 coef = tb.ring[t % tb.cap];             // formed from kernel arguments alone: a uniform load
  scatter_column<float4, FOLD>(pl, static_cast<int32_t>(i), reinterpret_cast<const float4*>(src) + c, lds / 4,
                               reinterpret_cast<float4*>(slab) + c, LPR, tb.n_rows, LandAdam{tb, coef, t, c});
}

template <bool FOLD>
__global__ __launch_bounds__(kScatterWaves * kWave) void rowadam_apply_scalar_kernel(ScatterPlan pl, const float* __restrict__ src, int64_t lds,
                                                                                    float* __restrict__ slab, RowAdamTable tb, int32_t t) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kScatterWaves + (threadIdx.x >> 6);
  if (i >= pl.n_listed || i >= pl.counts[kCountValid]) return;
  const float2 coef = tb.ring[t % tb.cap];
  for (int c = lane; c < tb.D; c += kWave)
    scatter_column<float, FOLD>(pl, static_cast<int32_t>(i), src + c, lds, slab + c, tb.D, tb.n_rows, LandAdam{tb, coef, t, c});
}

template <int LPR>
int launch_apply_vec(const ScatterPlan& pl, const float* src, int64_t lds, float* slab, const RowAdamTable& tb, int32_t t, hipStream_t s) {
  constexpr int per_block = kScatterWaves * (kWave / LPR);
  const unsigned blocks = static_cast<unsigned>((pl.n_listed + per_block - 1) / per_block);
  rowadam_apply_vec_kernel<LPR, false><<<blocks, kScatterWaves * kWave, 0, s>>>(pl, src, lds, slab, tb, t);
  TAGREC_LAUNCH_CHECK();
  if (pl.n_listed > kScatterChunk) {                   // only then can a segment be long
    rowadam_apply_vec_kernel<LPR, true><<<blocks, kScatterWaves * kWave, 0, s>>>(pl, src, lds, slab, tb, t);
    TAGREC_LAUNCH_CHECK();
  }
  return TAGREC_OK;
}

int launch_apply_scalar(const ScatterPlan& pl, const float* src, int64_t lds, float* slab, const RowAdamTable& tb, int32_t t, hipStream_t s) {
  const unsigned blocks = static_cast<unsigned>((pl.n_listed + kScatterWaves - 1) / kScatterWaves);
  rowadam_apply_scalar_kernel<false><<<blocks, kScatterWaves * kWave, 0, s>>>(pl, src, lds, slab, tb, t);
  TAGREC_LAUNCH_CHECK();
  if (pl.n_listed > kScatterChunk) {
    rowadam_apply_scalar_kernel<true><<<blocks, kScatterWaves * kWave, 0, s>>>(pl, src, lds, slab, tb, t);
    TAGREC_LAUNCH_CHECK();
  }
  return TAGREC_OK;
}

int make_table(const char* who, float* p, float* m, float* v, int64_t ld, int64_t n_rows, int D, int32_t* last, const float* ring,
               int64_t ring_cap, float b1, float b2, float eps, RowAdamTable* tb) {
  const std::string w(who);
  TAGREC_REQUIRE(p && m && v && last && ring, w + ": null pointer");
  TAGREC_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31) - 1, w + ": the table holds 1 .. 2^31 - 2 rows");
  TAGREC_REQUIRE(D >= 1 && D <= (1 << 16) && ld >= D, w + ": D must be 1 .. 65536 and the row stride at least D");
  TAGREC_REQUIRE(ring_cap >= 1 && (reinterpret_cast<uintptr_t>(ring) & 7u) == 0, w + ": the ring holds >= 1 8-byte aligned pairs");
  *tb = RowAdamTable{p, m, v, ld, last, n_rows, D, reinterpret_cast<const float2*>(ring), ring_cap,
                     static_cast<float>(1.0 - static_cast<double>(b1)), b2, static_cast<float>(1.0 - static_cast<double>(b2)), eps};
  return TAGREC_OK;
}

int check_window(const char* who, int64_t ring_cap, int64_t t_floor, int64_t t_done) {
  const std::string w(who);
  TAGREC_REQUIRE(t_floor >= 0 && t_floor <= t_done && t_done < (1ll << 31) - 1, w + ": needs 0 <= t_floor <= t_done < 2^31 - 1");
  TAGREC_REQUIRE(t_done - t_floor <= ring_cap, w + ": the ring is shorter than the steps (t_floor, t_done]");
  TAGREC_REQUIRE(t_done - t_floor <= kMaxWindow, w + ": a replay spans at most 4096 steps");
  return TAGREC_OK;
}

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_adam_coef(double lr, double b1, double b2, int64_t t0, int64_t n, float* out) {
  TAGREC_REQUIRE(out != nullptr || n == 0, "adam_coef: null pointer");
  TAGREC_REQUIRE(t0 >= 1 && n >= 0, "adam_coef: steps are counted from 1");
  for (int64_t i = 0; i < n; ++i) adam_step_coef(lr, b1, b2, t0 + i, out + 2 * i, out + 2 * i + 1);
  return TAGREC_OK;
}

extern "C" int tagrec_rowadam_catchup_f32(const void* ws, int64_t ws_bytes, int64_t n_listed, int width, float* p, float* m, float* v,
                                          int64_t ld, int64_t n_rows, int D, int32_t* last, const float* ring, int64_t ring_cap,
                                          int64_t t_floor, int64_t t_done, float b1, float b2, float eps, void* stream) {
  TAGREC_REQUIRE(ws != nullptr, "rowadam_catchup: null pointer");
  TAGREC_TRY(check_list("rowadam_catchup", n_listed, width));
  RowAdamTable tb;
  TAGREC_TRY(make_table("rowadam_catchup", p, m, v, ld, n_rows, D, last, ring, ring_cap, b1, b2, eps, &tb));
  TAGREC_TRY(check_window("rowadam_catchup", ring_cap, t_floor, t_done));
  RowListLayout L;
  rowlist_layout_head(n_listed, width, &L);
  TAGREC_REQUIRE(ws_bytes >= static_cast<int64_t>(L.total), "rowadam_catchup: workspace smaller than tagrec_rowlist_workspace(...)");
  if (t_done == t_floor) return TAGREC_OK;             // every row is at t_floor or later: all current
  const ScatterPlan pl = scatter_plan(ws, L, n_listed);
  return launch_replay<true>(tb, pl.seg_row, pl.counts, n_listed, static_cast<int32_t>(t_floor), static_cast<int32_t>(t_done),
                             static_cast<hipStream_t>(stream));
}

extern "C" int tagrec_rowadam_flush_f32(float* p, float* m, float* v, int64_t ld, int64_t n_rows, int D, int32_t* last, const float* ring,
                                        int64_t ring_cap, int64_t t_floor, int64_t t_done, float b1, float b2, float eps, void* stream) {
  RowAdamTable tb;
  TAGREC_TRY(make_table("rowadam_flush", p, m, v, ld, n_rows, D, last, ring, ring_cap, b1, b2, eps, &tb));
  TAGREC_TRY(check_window("rowadam_flush", ring_cap, t_floor, t_done));
  if (t_done == t_floor) return TAGREC_OK;
  return launch_replay<false>(tb, nullptr, nullptr, n_rows, static_cast<int32_t>(t_floor), static_cast<int32_t>(t_done),
                              static_cast<hipStream_t>(stream));
}

extern "C" int tagrec_rowadam_apply_f32(const void* ws, int64_t ws_bytes, int64_t n_listed, int width, const float* src, int64_t lds,
                                        float* p, float* m, float* v, int64_t ld, int64_t n_rows, int D, int32_t* last, const float* ring,
                                        int64_t ring_cap, int64_t t, float b1, float b2, float eps, void* stream) {
  TAGREC_REQUIRE(ws != nullptr && src != nullptr, "rowadam_apply: null pointer");
  TAGREC_TRY(check_list("rowadam_apply", n_listed, width));
  RowAdamTable tb;
  TAGREC_TRY(make_table("rowadam_apply", p, m, v, ld, n_rows, D, last, ring, ring_cap, b1, b2, eps, &tb));
  TAGREC_REQUIRE(D <= width, "rowadam_apply: D must be 1 .. the width the plan's workspace was sized for");
  TAGREC_REQUIRE(lds >= D, "rowadam_apply: the gradient's row stride is smaller than D");
  TAGREC_REQUIRE(t >= 1 && t < (1ll << 31) - 1, "rowadam_apply: steps are counted from 1");
  RowListLayout L;
  rowlist_layout_head(n_listed, width, &L);
  TAGREC_REQUIRE(ws_bytes >= static_cast<int64_t>(L.total), "rowadam_apply: workspace smaller than tagrec_rowlist_workspace(...)");
  const ScatterPlan pl = scatter_plan(ws, L, n_listed);
  float* slab = reinterpret_cast<float*>(const_cast<char*>(static_cast<const char*>(ws)) + L.slab);   // one stream per plan
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int32_t t32 = static_cast<int32_t>(t);
  const bool vec = aligned16(src) && aligned16(p) && aligned16(m) && aligned16(v) && lds % 4 == 0 && ld % 4 == 0;
  if (vec) {
    switch (D) {
      case 8: return launch_apply_vec<2>(pl, src, lds, slab, tb, t32, s);
      case 16: return launch_apply_vec<4>(pl, src, lds, slab, tb, t32, s);
      case 32: return launch_apply_vec<8>(pl, src, lds, slab, tb, t32, s);
      case 64: return launch_apply_vec<16>(pl, src, lds, slab, tb, t32, s);
      case 128: return launch_apply_vec<32>(pl, src, lds, slab, tb, t32, s);
      case 256: return launch_apply_vec<64>(pl, src, lds, slab, tb, t32, s);
      default: break;
    }
  }
  return launch_apply_scalar(pl, src, lds, slab, tb, t32, s);
}
