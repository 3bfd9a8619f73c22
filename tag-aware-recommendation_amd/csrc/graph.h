// The CSR handle behind `tagrec_graph*`, the device-side views of it and the host-side launch helpers, shared by the
// kernels that walk adjacency rows (spmm.hip, routing.hip, batch_hop.hip).
#pragma once

#include <type_traits>

#include "common.h"

// Borrowed CSR arrays + the long-row work list built once by tagrec_graph_create (spmm.hip).
struct tagrec_graph {
  int64_t n_rows, n_cols, nnz;
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  int64_t n_long, n_chunks;
  int32_t* long_rows;
  int32_t* long_base;
  int2* chunk_desc;
  float* slab;                // n_chunks x kSlabWidth partial sums, allocated with the handle (scratch of the launch in
  size_t slab_floats;         // flight: one stream per handle)
  bool owns_long;             // false: long_rows / long_base / chunk_desc belong to the graph this one was created like,
                              // or live in a caller-provided workspace
  bool owns_slab;             // false: the slab lives in a caller-provided workspace
  bool deferred = false;      // n_long / n_chunks are upper bounds, unused slots of the work list hold -1 (no host read at creation)
};

namespace tagrec {

constexpr int kWavesPerBlock = 4;
constexpr int kLongRow = 1024;   // rows with more stored entries are cut into chunks
constexpr int kChunk = 512;      // entries per chunk (one wavefront each)
constexpr int kSlabWidth = 256;  // floats per chunk in the partial-sum slab = widest vector kernel

struct GraphView {
  int64_t n_rows;
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  int64_t n_cols;           // rows of the gathered operand: what the row flags of that operand are counted against
};

// The FIRST `chunk_blocks` blocks of a row-walking launch take the long-row chunks.
struct LongView {
  const int32_t* long_rows;
  const int2* chunk_desc;   // (index into long_rows, chunk number)
  int64_t n_chunks;
  float* slab;              // [n_chunks, width] partial results
  unsigned chunk_blocks;
};

// Check that g->slab (allocated at creation) holds n_chunks x width floats.
int ensure_slab(const tagrec_graph* g, int width);

// *count = number of non-zero bytes of flags[0..n) (rowops.hip)
int count_flags(const uint8_t* flags, int64_t n, unsigned* count, hipStream_t s);

// ---- host side: what every launch over a handle starts from ---------------------------------------------------------
inline GraphView view_of(const tagrec_graph* g) { return GraphView{g->n_rows, g->rowptr, g->col, g->val, g->n_cols}; }

// blocks of a grid that gives each of n rows one of the `per_block` slots of a block (default: one wavefront per row)
inline unsigned row_blocks(int64_t n, int per_block = kWavesPerBlock) { return static_cast<unsigned>((n + per_block - 1) / per_block); }

// The long-row part of a launch whose rows are `width` floats wide: empty when the graph has no long row.
inline int long_view(const tagrec_graph* g, int width, LongView* lv) {
  *lv = LongView{g->long_rows, g->chunk_desc, g->n_chunks, nullptr, 0};
  if (g->n_long > 0) {
    TAGREC_TRY(ensure_slab(g, width));
    lv->slab = g->slab;
    lv->chunk_blocks = row_blocks(g->n_chunks);
  }
  return TAGREC_OK;
}

// A row-walking launch and the fold of its long rows: main_launch(lv) puts lv.chunk_blocks blocks in front of its own
// grid, finish_launch() folds the slab into the g->n_long long rows and runs only when there are any.
template <typename Main, typename Finish>
int launch_with_long_rows(const tagrec_graph* g, int width, Main&& main_launch, Finish&& finish_launch) {
  LongView lv;
  TAGREC_TRY(long_view(g, width, &lv));
  main_launch(lv);
  TAGREC_LAUNCH_CHECK();
  if (g->n_long > 0) {
    finish_launch();
    TAGREC_LAUNCH_CHECK();
  }
  return TAGREC_OK;
}

// The vector kernels cover rows of D = 8 .. 256 floats, a power of two: LPR = D / 4 lanes hold one row as float4s.
inline bool is_vec_width(int D) { return D == 8 || D == 16 || D == 32 || D == 64 || D == 128 || D == 256; }

// Dispatch on D to a functor templated on LPR.
template <typename F>
int vec_width_dispatch(int D, const char* who, F&& f) {
  switch (D) {
    case 8: return f(std::integral_constant<int, 2>{});
    case 16: return f(std::integral_constant<int, 4>{});
    case 32: return f(std::integral_constant<int, 8>{});
    case 64: return f(std::integral_constant<int, 16>{});
    case 128: return f(std::integral_constant<int, 32>{});
    case 256: return f(std::integral_constant<int, 64>{});
    default: return fail(TAGREC_E_UNSUPPORTED, std::string(who) + ": D must be 8 .. 256, a power of two");
  }
}

}  // namespace tagrec
