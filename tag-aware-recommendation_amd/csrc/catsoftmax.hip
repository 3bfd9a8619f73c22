// Catalogue softmax: a fused rectangular B x N softmax cross-entropy whose logits are never stored (tagrec_catsoftmax_fwd_f32 /
// tagrec_catsoftmax_bwd_f32) -- the rectangular sibling of csrc/inbatch.hip, with csrc/eval.hip's walk over the whole table.
//
// Operands: Q (rows read at qrow[b]), T [N, D] the column table, target [B].  z_bn = Q[qrow_b] . T[n] / temperature.
// The tile scheme is the one of csrc/pairtile.h (owned tile x walked tile in LDS, score MFMA, running (maximum, sum), C fed
// straight to the second MFMA).  What is this loss's own:
//   * the long axis is N and IT is what the grid splits: the column tiles are cut into n_split contiguous ranges and one block
//     serves one (64-row tile of Q, range) pair.  The forward leaves a (maximum, sum) pair per row and range, merged in
//     ascending range order by cat_combine_kernel; the backward of Q leaves a partial row per range, summed in ascending
//     range order by cat_sum_kernel.  An empty range (more ranges than tiles) leaves (sentinel, 0) / a zero row.
//   * the walk is pipelined through registers: the global loads of the NEXT walked tile are issued before the MFMAs of the
//     current one (NF float4 per thread, NF = Dp / 16), and land in LDS after the barrier that ends the current tile.
//   * the backward of T is owned by a column tile that walks the B rows of Q (ascending b) and STORES its 64 rows of the dense
//     dT: no atomics anywhere, nothing reads the old contents, every order is a function of (B, N, D, n_split) only.
// The target logit zt[b] comes from the same MFMA tile that feeds the row sum (stored by the lane that meets column
// target_b), so lse_b >= zt_b holds in floating point: the maximum is exact, the term of the maximum is exactly 1.
//
// The MASKED form (tagrec_catsoftmax_masked_*): row b leaves the columns of a sorted list out of its softmax, all but its own
// target -- mask_ptr / mask_cols, a CSR over the rows of Q in csrc/eval.hip's conventions, row qrow[b].  It is a compile-time
// variant of the same body (the unmasked instantiations are the code they were): an excluded column is a select in the tile
// walk, never pushed onto the running pair in the forward and an exact 0.0f coefficient in both backward walks.
//   * owner = rows of Q (forward, dQ): a lane meets its columns in ascending order, so it keeps one cursor into its row's list
//     and the next excluded id in a register; a tile below that id costs one compare and no load.
//   * owner = rows of T (dT): the 64 threads that stage the walked rows' targets fold each row's entries inside the owned 64
//     columns into one 64-bit word, a ballot per column transposes the 64 words and they go to LDS (two buffers of 64
//     words): a lane of the walk reads the one word of its column.  The search for the NEXT walked tile is issued before the
//     current tile's MFMAs and written to the other buffer.
#include "pairtile.h"

namespace tagrec {
namespace {

constexpr int kCombineRows = 256;         // rows per block of cat_combine_kernel: `partials` holds two floats per block
constexpr int kMaxSplit = 65535;          // gridDim.y

struct CatArgs {
  Rows q, t;
  int64_t B, N;
  int D, Dk;                              // Dk = D rounded up to 16 (score loop); the LDS row width Dp = 16 NF >= Dk
  const int64_t* target;
  float inv_tau, inv_b;
  int64_t tiles_per_range;                // column tiles of one range; range y covers tiles y tpr .. (y + 1) tpr - 1
  float* pm;                              // forward: [n_split, B] maxima and sums, zt [B]
  float* ps;
  float* zt;
  const float* lse;                       // backward
  const float* g;
  float* dQpart;                          // [n_split, B, D] partial rows (dQ itself when n_split == 1)
  float* dT;
  int64_t lddt;
  const int64_t* mask_ptr;                // the masked form: CSR over the rows of Q (row qrow[b]) of the excluded columns,
  const int32_t* mask_cols;               // ascending and unique within a row; the row's own target stays live regardless
};

constexpr int64_t kNoCol = INT64_MAX;     // "no further excluded column" of a lane's cursor

// One row of the CSR as 32-bit state (a column id fits int32; a list longer than 2^31 - 1 entries is cut there).
struct MaskRow {
  const int32_t* cols;
  int n;
};
__device__ __forceinline__ MaskRow mask_row(const CatArgs& a, int64_t r) {
  const int64_t lo = a.mask_ptr[r], len = a.mask_ptr[r + 1] - lo;
  return {a.mask_cols + lo, len < 0 ? 0 : (len > INT32_MAX ? INT32_MAX : static_cast<int>(len))};
}

// first position in [0, n) whose column is >= col (n if none); every read lies inside the row whatever the list holds
__device__ __forceinline__ int mask_lower_bound(const MaskRow& m, int col) {
  int lo = 0, hi = m.n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (m.cols[mid] < col) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Is the row's target its ONLY live column (the list holds every other column)?  Then p_target = 1 and every coefficient of
// the row is 0; the backward walks take the target for excluded as well, so that the 0 is a stored one.  (Formed from the
// logits it would be expf(z - lse) - 1 with lse == zt bit for bit, where z - lse, contracted into one fma, sees the
// unrounded product and leaves the rounding residue of zt.)  The usual row fails the first compare.
__device__ __forceinline__ bool mask_single(const MaskRow& m, int64_t N, int64_t tgt) {
  if (m.n < N - 1) return false;
  const int c = mask_lower_bound(m, static_cast<int>(tgt));
  const bool has = c < m.n && m.cols[c] == tgt;
  return m.n - (has ? 1 : 0) == N - 1;
}

// MODE 2 of the masked form: bit d of the word = "column own0 + d is excluded for the walked row w" (the row's target never is)
__device__ __forceinline__ uint64_t mask_word(const CatArgs& a, int64_t w, int64_t own0) {
  if (w >= a.B) return 0;
  const MaskRow m = mask_row(a, a.q.idx ? a.q.idx[w] : w);
  const int first = static_cast<int>(own0);            // own0 < N <= 2^31 - 1
  uint64_t bits = 0;
  for (int c = mask_lower_bound(m, first); c < m.n; ++c) {
    const unsigned d = static_cast<unsigned>(m.cols[c]) - static_cast<unsigned>(first);
    if (d >= static_cast<unsigned>(kTile)) break;      // past the owned columns (or, in an unsorted list, before them)
    bits |= 1ull << d;
  }
  const int64_t tgt = a.target[w], dt = tgt - own0;
  if (dt >= 0 && dt < kTile) {
    bits &= ~(1ull << dt);
    if (mask_single(m, a.N, tgt)) bits |= 1ull << dt;
  }
  return bits;
}

// The first wavefront of a block (lane = walked row w0 + lane) turns its 64 row words into 64 COLUMN words -- bit i of dst[d] =
// "owned column own0 + d is excluded for walked row w0 + i" -- by one ballot per column, so that a lane of the tile walk reads
// the one word of its own column.  No entry in the whole 64 x 64 tile (the usual case at catalogue scale): one ballot.
__device__ __forceinline__ void stage_mask_words(uint64_t* dst, const CatArgs& a, int64_t w0, int64_t own0, int lane) {
  const uint64_t bits = mask_word(a, w0 + lane, own0);
  uint64_t mine = 0;
  if (__ballot(bits != 0) != 0) {
#pragma unroll 1
    for (int d = 0; d < kTile; ++d) {
      const uint64_t col = __ballot(static_cast<int>((bits >> d) & 1ull));
      if (lane == d) mine = col;
    }
  }
  dst[lane] = mine;
}

// MODE 0: forward (owner = 64 rows of Q, walks one column range).  MODE 1: backward of Q, the same roles.
// MODE 2: backward of T (owner = 64 rows of T, walks all B rows of Q).  MASKED: the lists of a.mask_ptr / a.mask_cols apply.
template <int MODE, int NF, bool MASKED>
__device__ __forceinline__ void cat_body(const CatArgs& a, unsigned char* smem) {
  constexpr int S = tile_stride(16 * NF);
  int64_t* sh_tgt = reinterpret_cast<int64_t*>(smem);  // MODE 2: targets and row log-sum-exps of the walked rows
  float* sh_lse = reinterpret_cast<float*>(sh_tgt + kTile);
  float* sh_own = sh_lse + kTile;
  float* sh_walk = sh_own + kTile * S;
  // MASKED, MODE 2: one 64-bit word per owned column (stage_mask_words), twice: the words of the next walked tile are written
  // while this one's are read
  uint64_t* sh_bits = reinterpret_cast<uint64_t*>(sh_walk + kTile * S);

  const PairLane ln = pair_lane();
  const int tid = threadIdx.x, wave = ln.wave, r = ln.r, q = ln.q;
  const Rows& own = MODE == 2 ? a.t : a.q;
  const Rows& walk = MODE == 2 ? a.q : a.t;
  const int64_t own_n = MODE == 2 ? a.N : a.B;
  const int64_t own0 = static_cast<int64_t>(blockIdx.x) * kTile;
  int64_t w_begin = 0, w_end = a.B;
  if (MODE != 2) {
    const int64_t t0 = static_cast<int64_t>(blockIdx.y) * a.tiles_per_range;
    w_begin = t0 * kTile;
    w_end = (t0 + a.tiles_per_range) * kTile;
    if (w_end > a.N) w_end = a.N;
    if (w_begin > w_end) w_begin = w_end;              // an empty range
  }

  f32x4 pre[NF];
  load_tile<NF>(pre, own, a.D, own0, own_n);
  store_tile<NF>(sh_own, pre);

  const int64_t o = own0 + 16 * wave + r;              // the owned row whose scores this lane ends up with
  const bool o_ok = o < own_n;
  const int64_t o_tgt = (MODE != 2 && o_ok) ? a.target[o] : -1;
  const float o_lse = (MODE == 1 && o_ok) ? a.lse[o] : 0.f;
  const float scale = MODE == 0 ? 0.f : ((a.g ? a.g[0] : 1.0f) * a.inv_tau) * a.inv_b;

  float run_m = kLowest, run_s = 0.f;                  // forward: this lane's columns only
  AccTiles<NF> acc;
  zero_acc(acc);

  // MASKED, MODE 0 / 1: the lane's cursor into the list of its row and the column it stands on (kNoCol: the list is spent)
  MaskRow m_row = {nullptr, 0};
  int m_cur = 0;
  int64_t m_next = kNoCol;
  bool m_single = false;                               // MODE 1: `mask_single` of the lane's row
  int m_buf = 0;                                       // MASKED, MODE 2: the half of sh_bits this tile reads
  if constexpr (MASKED && MODE != 2) {
    if (o_ok && w_begin < w_end) {
      m_row = mask_row(a, own.idx ? own.idx[o] : o);
      m_cur = mask_lower_bound(m_row, static_cast<int>(w_begin));                // a range starts mid-list
      if (m_cur < m_row.n) m_next = m_row.cols[m_cur];
      if (MODE == 1) m_single = mask_single(m_row, a.N, o_tgt);
    }
  }
  if constexpr (MASKED && MODE == 2) {
    if (tid < kTile) stage_mask_words(sh_bits, a, w_begin, own0, tid);         // the first barrier of the walk covers it
  }

  if (w_begin < w_end) load_tile<NF>(pre, walk, a.D, w_begin, w_end);
  for (int64_t w0 = w_begin; w0 < w_end; w0 += kTile) {
    __syncthreads();                                   // the previous walked tile has been consumed
    store_tile<NF>(sh_walk, pre);
    if (MODE == 2 && tid < kTile) {
      const int64_t w = w0 + tid;
      const bool ok = w < w_end;
      sh_tgt[tid] = ok ? a.target[w] : -1;
      sh_lse[tid] = ok ? a.lse[w] : 0.f;
    }
    __syncthreads();
    if (w0 + kTile < w_end) load_tile<NF>(pre, walk, a.D, w0 + kTile, w_end);   // in flight under this tile's MFMAs
    if constexpr (MASKED && MODE == 2) {               // and so is the search of the next walked rows' lists
      if (tid < kTile && w0 + kTile < w_end) stage_mask_words(sh_bits + kTile * (m_buf ^ 1), a, w0 + kTile, own0, tid);
    }

    // MASKED, MODE 0 / 1: bit 4 t + v = "column w0 + 16 t + 4 q + v is in the row's list".  The usual tile holds no entry:
    // one compare.  Otherwise every entry of the tile is passed once, whichever of the row's four lanes it belongs to.
    unsigned m_ex = 0;
    if constexpr (MASKED && MODE != 2) {
      while (m_next < w0 + kTile) {
        const int d = static_cast<int>(m_next - w0);
        if (d >= 0 && ((d >> 2) & 3) == q) m_ex |= 1u << (((d >> 4) << 2) | (d & 3));
        ++m_cur;
        m_next = m_cur < m_row.n ? m_row.cols[m_cur] : kNoCol;
      }
    }

    f32x4 sc[4];
    score_tile(sh_own, sh_walk, S, a.Dk, ln, sc);
    uint64_t m_col = 0;                                // MASKED, MODE 2: the word of this lane's column, walked row 4 q at bit 0
    if constexpr (MASKED && MODE == 2) m_col = sh_bits[kTile * m_buf + 16 * wave + r] >> (4 * q);
    // sc[t][v] = owned row o . walked row w0 + 16 t + 4 q + v
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int wl = 16 * t + 4 * q + v;
        const int64_t w = w0 + wl;
        bool live = o_ok && w < w_end;
        if constexpr (MASKED && MODE != 2) live = live && (w == o_tgt ? !m_single : ((m_ex >> (4 * t + v)) & 1u) == 0);
        if constexpr (MASKED && MODE == 2) live = live && ((m_col >> (16 * t + v)) & 1ull) == 0;
        const float z = sc[t][v] * a.inv_tau;          // one rounding, the same in every pass
        if (MODE == 0) {
          if (live) {
            lse_push(run_m, run_s, z);
            if (w == o_tgt) a.zt[o] = z;               // one lane of one block of the whole grid
          }
        } else {
          const float l = MODE == 1 ? o_lse : sh_lse[wl];
          const bool hit = MODE == 1 ? (w == o_tgt) : (sh_tgt[wl] == o);
          sc[t][v] = live ? scale * (expf(z - l) - (hit ? 1.0f : 0.0f)) : 0.0f;
        }
      }
    }
    if (MODE != 0) grad_tile<NF>(sh_walk, S, ln, sc, acc);
    if constexpr (MASKED && MODE == 2) m_buf ^= 1;
  }

  if (MODE == 0) {
    lse_merge_q(run_m, run_s);
    if (o_ok && q == 0) {
      const int64_t at = static_cast<int64_t>(blockIdx.y) * a.B + o;
      a.pm[at] = run_m;
      a.ps[at] = run_s;
    }
  } else {
    float* dst = MODE == 1 ? a.dQpart + static_cast<int64_t>(blockIdx.y) * a.B * a.D : a.dT;
    const int64_t ldd = MODE == 1 ? a.D : a.lddt;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int c = 16 * f + r;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t row = own0 + 16 * wave + 4 * q + v;
        if (row < own_n && c < a.D) dst[row * ldd + c] = acc.f[f][v];
      }
    }
  }
}

template <int NF>
__global__ __launch_bounds__(kThreads) void cat_fwd_kernel(CatArgs a) {
  extern __shared__ __align__(16) unsigned char cat_smem[];
  cat_body<0, NF, false>(a, cat_smem);
}

template <int NF>
__global__ __launch_bounds__(kThreads) void cat_dq_kernel(CatArgs a) {
  extern __shared__ __align__(16) unsigned char cat_smem[];
  cat_body<1, NF, false>(a, cat_smem);
}

template <int NF>
__global__ __launch_bounds__(kThreads) void cat_dt_kernel(CatArgs a) {
  extern __shared__ __align__(16) unsigned char cat_smem[];
  cat_body<2, NF, false>(a, cat_smem);
}

template <int NF>
__global__ __launch_bounds__(kThreads) void cat_fwd_masked_kernel(CatArgs a) {
  extern __shared__ __align__(16) unsigned char cat_smem[];
  cat_body<0, NF, true>(a, cat_smem);
}

template <int NF>
__global__ __launch_bounds__(kThreads) void cat_dq_masked_kernel(CatArgs a) {
  extern __shared__ __align__(16) unsigned char cat_smem[];
  cat_body<1, NF, true>(a, cat_smem);
}

// Left to itself the register allocator stops a few registers above the unmasked kernel's step at NF = 4 and 8 (a wave of
// occupancy each); asked for the unmasked kernel's waves per SIMD it fits every NF, still without scratch.
constexpr int dt_waves(int nf) { return nf <= 1 ? 6 : nf == 2 ? 5 : nf == 4 ? 4 : nf == 8 ? 3 : nf == 12 ? 2 : 1; }

template <int NF>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(dt_waves(NF)))) void cat_dt_masked_kernel(CatArgs a) {
  extern __shared__ __align__(16) unsigned char cat_smem[];
  cat_body<2, NF, true>(a, cat_smem);
}

struct RegArgs {
  const float* Qreg;
  const float* Treg;
  const int64_t* qrow;
  const int64_t* target;
  int64_t ldreg, N;
  int Dreg;
};

// row b of the two L2 operands; a target outside [0, N) is the caller's error and is clamped so that no read leaves Treg
__device__ __forceinline__ const float* reg_row(const RegArgs& x, int side, int64_t b) {
  if (side == 0) return x.Qreg + (x.qrow ? x.qrow[b] : b) * x.ldreg;
  int64_t t = x.target[b];
  t = t < 0 ? 0 : (t >= x.N ? x.N - 1 : t);
  return x.Treg + t * x.ldreg;
}

// lse[b] = merge of the row's (maximum, sum) pairs in ascending range order (a range that is empty, or in the masked form
// wholly excluded for the row, holds (sentinel, 0) and merges as nothing: its side of lse_merge is 0 * expf(<= 0)); partials[2 blk] = sum of (lse - zt) over the
// block's 256 rows (fixed tree), partials[2 blk + 1] = 0.5 sum |row|^2 of their L2 rows (one row per wavefront at a time)
__global__ __launch_bounds__(kThreads) void cat_combine_kernel(const float* pm, const float* ps, int n_split, int64_t B,
                                                               const float* zt, RegArgs x, float* lse_out, float* partials) {
  __shared__ float sh[kThreads];
  __shared__ float sh_reg[4];
  const PairLane ln = pair_lane();
  const int tid = threadIdx.x;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kCombineRows, b = b0 + tid;
  float loss = 0.f;
  if (b < B) {
    float m = kLowest, s = 0.f;
    for (int y = 0; y < n_split; ++y) lse_merge(m, s, pm[static_cast<int64_t>(y) * B + b], ps[static_cast<int64_t>(y) * B + b]);
    const float l = m + logf(s);                       // the target's range is live: m is a score, its term is 1, s >= 1
    lse_out[b] = l;
    loss = l - zt[b];
  }
  sh[tid] = loss;
  float reg = 0.f;
  if (x.Qreg) reg = l2_rows([&](int side, int64_t row) { return reg_row(x, side, row); }, b0, kCombineRows / 4, B, x.Dreg, ln);
  if (ln.lane == 0) sh_reg[ln.wave] = reg;
  __syncthreads();
  for (int off = kThreads / 2; off >= 1; off >>= 1) {
    if (tid < off) sh[tid] += sh[tid + off];
    __syncthreads();
  }
  if (tid == 0) {
    partials[2 * blockIdx.x] = sh[0];
    partials[2 * blockIdx.x + 1] = 0.5f * ((sh_reg[0] + sh_reg[1]) + (sh_reg[2] + sh_reg[3]));
  }
}

__global__ __launch_bounds__(kThreads) void cat_reduce_kernel(const float* partials, int64_t n, float inv_b, float* loss_out) {
  reduce_loss_pair(partials, n, inv_b, loss_out);
}

// dQ[b] = sum over ranges of part[y][b], ascending y
__global__ __launch_bounds__(kThreads) void cat_sum_kernel(const float* part, int n_split, int64_t BD, float* dQ) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= BD) return;
  float s = part[i];
  for (int y = 1; y < n_split; ++y) s += part[static_cast<int64_t>(y) * BD + i];
  dQ[i] = s;
}

// the compact L2 gradients: dQreg[b] = rscale Qreg[qrow_b], dTreg[b] = rscale Treg[target_b], rscale = g1 / B
__global__ __launch_bounds__(kThreads) void cat_reg_bwd_kernel(RegArgs x, int64_t B, const float* g, float inv_b, float* dQreg,
                                                               float* dTreg) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= B * x.Dreg) return;
  const int64_t b = i / x.Dreg;
  const int c = static_cast<int>(i - b * x.Dreg);
  const float rscale = (g ? g[1] : 1.0f) * inv_b;
  dQreg[i] = rscale * reg_row(x, 0, b)[c];
  dTreg[i] = rscale * reg_row(x, 1, b)[c];
}

size_t lds_bytes(int Dp, bool masked = false) {
  return kTile * sizeof(int64_t) + kTile * sizeof(float) + tiles_bytes(Dp) + (masked ? 2 * kTile * sizeof(uint64_t) : 0);
}

bool shape_ok(int64_t B, int64_t N, int D) { return D >= 8 && D <= 256 && (D & 3) == 0 && B >= 1 && B <= 65536 && N >= 1; }

int check_shape(const char* what, int64_t B, int64_t N, int D, int64_t ldq, int64_t ldt) {
  if (int rc = check_rows(what, B, 1, "", D)) return rc;
  if (N < 1) return fail(TAGREC_E_UNSUPPORTED, std::string(what) + ": N must be >= 1, got " + std::to_string(N));
  return check_stride(what, ldq < ldt ? ldq : ldt, D);
}

int64_t col_tiles(int64_t N) { return (N + kTile - 1) / kTile; }

// row tiles x ranges fill the 256 CUs about four times over, and a range keeps at least four column tiles (the owned tile
// is staged once per block)
int default_splits(int64_t B, int64_t N) {
  const int64_t row_tiles = (B + kTile - 1) / kTile;
  int64_t want = (1024 + row_tiles - 1) / row_tiles;
  const int64_t most = col_tiles(N) / 4;
  if (want > most) want = most;
  if (want > kMaxSplit) want = kMaxSplit;
  return want < 1 ? 1 : static_cast<int>(want);
}

int resolve_splits(const char* what, int64_t B, int64_t N, int n_split, int* out) {
  if (n_split < 0 || n_split > kMaxSplit)
    return fail(TAGREC_E_INVALID, std::string(what) + ": n_split must be in 0 .. 65535 (0: the default), got " + std::to_string(n_split));
  *out = n_split == 0 ? default_splits(B, N) : n_split;
  return TAGREC_OK;
}

int64_t combine_blocks(int64_t B) { return (B + kCombineRows - 1) / kCombineRows; }

// floats: the forward keeps pm | ps [n_split, B] each and two partials per combine block, the backward [n_split, B, D]
int64_t workspace_floats(int64_t B, int D, int n_split) {
  const int64_t fwd = 2 * static_cast<int64_t>(n_split) * B + 2 * combine_blocks(B);
  const int64_t bwd = static_cast<int64_t>(n_split) * B * D;
  return fwd > bwd ? fwd : bwd;
}

void fill_args(CatArgs& a, const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt, int64_t N, int D,
               const int64_t* target, int64_t B, float temperature, int n_split) {
  a.q.X = Q; a.q.ld = ldq; a.q.idx = qrow; a.q.vec = aligned16(Q) && (ldq & 3) == 0;
  a.t.X = T; a.t.ld = ldt; a.t.idx = nullptr; a.t.vec = aligned16(T) && (ldt & 3) == 0;
  a.B = B; a.N = N; a.D = D; a.Dk = round16(D);
  a.target = target;
  a.inv_tau = 1.0f / temperature; a.inv_b = 1.0f / static_cast<float>(B);
  a.tiles_per_range = (col_tiles(N) + n_split - 1) / n_split;
}

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_catsoftmax_splits(int64_t B, int64_t N, int D) {
  if (!shape_ok(B, N, D)) {
    fail(TAGREC_E_UNSUPPORTED, "catsoftmax_splits: D a multiple of 4 in 8 .. 256, B in 1 .. 65536 and N >= 1 expected");
    return TAGREC_E_UNSUPPORTED;
  }
  return default_splits(B, N);
}

extern "C" int64_t tagrec_catsoftmax_workspace(int64_t B, int64_t N, int D, int n_split) {
  if (!shape_ok(B, N, D) || n_split < 0 || n_split > kMaxSplit) {
    fail(TAGREC_E_UNSUPPORTED, "catsoftmax_workspace: D a multiple of 4 in 8 .. 256, B in 1 .. 65536, N >= 1 and n_split in "
                               "0 .. 65535 expected");
    return TAGREC_E_UNSUPPORTED;
  }
  return 4 * workspace_floats(B, D, n_split == 0 ? default_splits(B, N) : n_split);
}

// the two entry-point pairs; masked: the lists are required and a column id must fit mask_cols' int32
static int cat_check_mask(const std::string& what, bool masked, int64_t N, const int64_t* mask_ptr, const int32_t* mask_cols) {
  if (!masked) return TAGREC_OK;
  TAGREC_REQUIRE(mask_ptr && mask_cols, what + ": null mask_ptr / mask_cols (an empty list set still has its row pointers)");
  if (N > INT32_MAX) return fail(TAGREC_E_UNSUPPORTED, what + ": the masked form takes N <= 2^31 - 1, got " + std::to_string(N));
  return TAGREC_OK;
}

static int cat_fwd(const std::string& what, bool masked, const float* Q, int64_t ldq, const int64_t* qrow, const float* T,
                   int64_t ldt, int64_t N, int D, const int64_t* target, const int64_t* mask_ptr, const int32_t* mask_cols,
                   const float* Qreg, const float* Treg, int64_t ldreg, int Dreg, int64_t B, float temperature, int n_split,
                   void* workspace, int64_t workspace_bytes, float* lse, float* zt, float* loss_out, void* stream) {
  if (int rc = check_shape(what.c_str(), B, N, D, ldq, ldt)) return rc;
  TAGREC_REQUIRE(Q && T && target && workspace && lse && zt && loss_out, what + ": null pointer");
  if (int rc = cat_check_mask(what, masked, N, mask_ptr, mask_cols)) return rc;
  TAGREC_REQUIRE((Qreg == nullptr) == (Treg == nullptr), what + ": Qreg/Treg must both be given or both null");
  TAGREC_REQUIRE(!Qreg || (Dreg >= 1 && ldreg >= Dreg), what + ": bad reg shape");
  if (int rc = check_temperature(what, temperature)) return rc;
  int ns = 0;
  if (int rc = resolve_splits(what.c_str(), B, N, n_split, &ns)) return rc;
  TAGREC_REQUIRE(workspace_bytes >= 4 * workspace_floats(B, D, ns), what + ": the workspace is too small");
  CatArgs a = {};
  fill_args(a, Q, ldq, qrow, T, ldt, N, D, target, B, temperature, ns);
  a.mask_ptr = mask_ptr; a.mask_cols = mask_cols;
  float* ws = static_cast<float*>(workspace);
  a.pm = ws;
  a.ps = ws + static_cast<int64_t>(ns) * B;
  a.zt = zt;
  float* partials = ws + 2 * static_cast<int64_t>(ns) * B;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nf = pick_nf(D);
  const dim3 grid(static_cast<unsigned>((B + kTile - 1) / kTile), static_cast<unsigned>(ns));
  const size_t lds = lds_bytes(16 * nf, masked);
  if (int rc = dispatch_nf(nf, [&](auto n) {
        constexpr int NF = decltype(n)::value;
        return masked ? launch_lds<CatArgs, cat_fwd_masked_kernel<NF>>(grid, lds, a, s) : launch_lds<CatArgs, cat_fwd_kernel<NF>>(grid, lds, a, s);
      })) return rc;
  RegArgs x = {Qreg, Treg, qrow, target, ldreg, N, Dreg};
  const int64_t blocks = combine_blocks(B);
  cat_combine_kernel<<<static_cast<unsigned>(blocks), kThreads, 0, s>>>(a.pm, a.ps, ns, B, zt, x, lse, partials);
  TAGREC_LAUNCH_CHECK();
  cat_reduce_kernel<<<1, kThreads, 0, s>>>(partials, blocks, a.inv_b, loss_out);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

static int cat_bwd(const std::string& what, bool masked, const float* Q, int64_t ldq, const int64_t* qrow, const float* T,
                   int64_t ldt, int64_t N, int D, const int64_t* target, const int64_t* mask_ptr, const int32_t* mask_cols,
                   const float* Qreg, const float* Treg, int64_t ldreg, int Dreg, int64_t B, float temperature, int n_split,
                   void* workspace, int64_t workspace_bytes, const float* lse, const float* g, float* dT, int64_t lddt, float* dQ,
                   float* dQreg, float* dTreg, void* stream) {
  if (int rc = check_shape(what.c_str(), B, N, D, ldq, ldt)) return rc;
  TAGREC_REQUIRE(Q && T && target && workspace && lse, what + ": null pointer");
  if (int rc = cat_check_mask(what, masked, N, mask_ptr, mask_cols)) return rc;
  TAGREC_REQUIRE((dT == nullptr) == (dQ == nullptr), what + ": dT/dQ must both be given or both null (the L2 part only)");
  TAGREC_REQUIRE(dT || dQreg, what + ": nothing to write");
  TAGREC_REQUIRE(!dT || lddt >= D, what + ": row stride of dT below D");
  TAGREC_REQUIRE((dQreg == nullptr) == (dTreg == nullptr), what + ": dQreg/dTreg must both be given or both null");
  TAGREC_REQUIRE(!dQreg || (Qreg && Treg && Dreg >= 1 && ldreg >= Dreg), what + ": bad reg arguments");
  if (int rc = check_temperature(what, temperature)) return rc;
  int ns = 0;
  if (int rc = resolve_splits(what.c_str(), B, N, n_split, &ns)) return rc;
  TAGREC_REQUIRE(workspace_bytes >= 4 * workspace_floats(B, D, ns), what + ": the workspace is too small");
  CatArgs a = {};
  fill_args(a, Q, ldq, qrow, T, ldt, N, D, target, B, temperature, ns);
  a.mask_ptr = mask_ptr; a.mask_cols = mask_cols;
  a.lse = lse; a.g = g; a.dT = dT; a.lddt = lddt;
  a.dQpart = ns == 1 ? dQ : static_cast<float*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nf = pick_nf(D);
  const size_t lds = lds_bytes(16 * nf, masked);
  if (dT) {
    const dim3 grid_t(static_cast<unsigned>(col_tiles(N)));
    if (int rc = dispatch_nf(nf, [&](auto n) {
          constexpr int NF = decltype(n)::value;
          return masked ? launch_lds<CatArgs, cat_dt_masked_kernel<NF>>(grid_t, lds, a, s) : launch_lds<CatArgs, cat_dt_kernel<NF>>(grid_t, lds, a, s);
        })) return rc;
    const dim3 grid_q(static_cast<unsigned>((B + kTile - 1) / kTile), static_cast<unsigned>(ns));
    if (int rc = dispatch_nf(nf, [&](auto n) {
          constexpr int NF = decltype(n)::value;
          return masked ? launch_lds<CatArgs, cat_dq_masked_kernel<NF>>(grid_q, lds, a, s) : launch_lds<CatArgs, cat_dq_kernel<NF>>(grid_q, lds, a, s);
        })) return rc;
  }
  if (dT && ns > 1) {
    const int64_t BD = B * D;
    cat_sum_kernel<<<static_cast<unsigned>((BD + kThreads - 1) / kThreads), kThreads, 0, s>>>(a.dQpart, ns, BD, dQ);
    TAGREC_LAUNCH_CHECK();
  }
  if (dQreg) {
    RegArgs x = {Qreg, Treg, qrow, target, ldreg, N, Dreg};
    const int64_t n = B * Dreg;
    cat_reg_bwd_kernel<<<static_cast<unsigned>((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(x, B, g, a.inv_b, dQreg, dTreg);
    TAGREC_LAUNCH_CHECK();
  }
  return TAGREC_OK;
}

extern "C" int tagrec_catsoftmax_fwd_f32(const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt, int64_t N,
                                         int D, const int64_t* target, const float* Qreg, const float* Treg, int64_t ldreg,
                                         int Dreg, int64_t B, float temperature, int n_split, void* workspace,
                                         int64_t workspace_bytes, float* lse, float* zt, float* loss_out, void* stream) {
  return cat_fwd("catsoftmax_fwd", false, Q, ldq, qrow, T, ldt, N, D, target, nullptr, nullptr, Qreg, Treg, ldreg, Dreg, B,
                 temperature, n_split, workspace, workspace_bytes, lse, zt, loss_out, stream);
}

extern "C" int tagrec_catsoftmax_bwd_f32(const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt, int64_t N,
                                         int D, const int64_t* target, const float* Qreg, const float* Treg, int64_t ldreg,
                                         int Dreg, int64_t B, float temperature, int n_split, void* workspace,
                                         int64_t workspace_bytes, const float* lse, const float* g, float* dT, int64_t lddt,
                                         float* dQ, float* dQreg, float* dTreg, void* stream) {
  return cat_bwd("catsoftmax_bwd", false, Q, ldq, qrow, T, ldt, N, D, target, nullptr, nullptr, Qreg, Treg, ldreg, Dreg, B,
                 temperature, n_split, workspace, workspace_bytes, lse, g, dT, lddt, dQ, dQreg, dTreg, stream);
}

extern "C" int tagrec_catsoftmax_masked_fwd_f32(const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt,
                                                int64_t N, int D, const int64_t* target, const float* Qreg, const float* Treg,
                                                int64_t ldreg, int Dreg, int64_t B, float temperature, int n_split,
                                                void* workspace, int64_t workspace_bytes, float* lse, float* zt, float* loss_out,
                                                void* stream, const int64_t* mask_ptr, const int32_t* mask_cols) {
  return cat_fwd("catsoftmax_masked_fwd", true, Q, ldq, qrow, T, ldt, N, D, target, mask_ptr, mask_cols, Qreg, Treg, ldreg, Dreg,
                 B, temperature, n_split, workspace, workspace_bytes, lse, zt, loss_out, stream);
}

extern "C" int tagrec_catsoftmax_masked_bwd_f32(const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt,
                                                int64_t N, int D, const int64_t* target, const float* Qreg, const float* Treg,
                                                int64_t ldreg, int Dreg, int64_t B, float temperature, int n_split,
                                                void* workspace, int64_t workspace_bytes, const float* lse, const float* g,
                                                float* dT, int64_t lddt, float* dQ, float* dQreg, float* dTreg, void* stream,
                                                const int64_t* mask_ptr, const int32_t* mask_cols) {
  return cat_bwd("catsoftmax_masked_bwd", true, Q, ldq, qrow, T, ldt, N, D, target, mask_ptr, mask_cols, Qreg, Treg, ldreg, Dreg,
                 B, temperature, n_split, workspace, workspace_bytes, lse, g, dT, lddt, dQ, dQreg, dTreg, stream);
}
