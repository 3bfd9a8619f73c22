/* tagrec.h -- C ABI of libtagrec_hip.so (MI355X / gfx950 only).
 *
 * The reference (chenzheng5555/tag-aware-recommendation) has no FFI: its hot path
 * is in-process Python calling PyTorch operators.  Each entry point below replaces
 * the PyTorch operator sequence at the cited reference lines; the Python host in
 * `tag-aware-recommendation_amd/` mirrors the reference's operator / model / step
 * surface and binds these symbols with ctypes (binding shown in INTEGRATION.md).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (PyTorch storage);
 *     the library never frees caller memory.  Row-major, contiguous, fp32.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every call is asynchronous on that stream unless stated otherwise.
 *   - return value: 0 = TAGREC_OK, negative = TAGREC_E_*; the message for the last
 *     failing call of the calling thread is tagrec_last_error().  No C++ exception
 *     crosses the ABI.
 *   - a handle may be used from one thread AND one stream at a time (a graph handle owns the
 *     partial-sum scratch of the launch in flight; launches on one stream are ordered, two
 *     streams sharing a handle would race on it); distinct handles are independent.
 *   - no entry point that takes a `stream` allocates or frees device memory: scratch is
 *     either allocated when a handle is created or passed in by the caller (the
 *     `*_workspace` size queries), so every such call may be captured in a HIP graph.
 *   - D (row width) must be a multiple of 4 and rows 16-byte aligned for the vector
 *     kernels; other widths take a scalar kernel (correct, slower).
 */
#ifndef TAGREC_H
#define TAGREC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAGREC_OK 0
#define TAGREC_E_INVALID (-1)     /* bad argument (null pointer, negative size, bad enum) */
#define TAGREC_E_HIP (-2)         /* a HIP runtime call failed; message holds hipGetErrorString */
#define TAGREC_E_UNSUPPORTED (-3) /* shape outside what the kernels cover */
#define TAGREC_E_NOMEM (-4)

#define TAGREC_LOSS_SOFTPLUS 0    /* mean softplus(neg - pos)        (loss.py:11) */
#define TAGREC_LOSS_LOGSIGMOID 1  /* -mean logsigmoid(pos - neg)     (loss.py:9)  */
#define TAGREC_LOSS_SOFTMAX 2     /* sampled softmax over (pos, K negatives): tagrec_rank_fwd_f32 only */

#define TAGREC_ABI_VERSION 2

typedef struct tagrec_graph tagrec_graph;

int tagrec_abi_version(void);
const char* tagrec_last_error(void);
/* number of CUs / wavefront size / gcnArchName of the current device (synchronous) */
int tagrec_device_info(int* n_cu, int* wave_size, char* arch, int arch_len);

/* ---- sparse normalised adjacency ------------------------------------------------
 * A CSR matrix (int64 rowptr[n_rows+1], int32 colidx[nnz], fp32 vals[nnz]) as built by
 * model/help/adj.py:38-46 `creat_adj` (+ :144-150 `sp2tensor`).  The arrays are BORROWED:
 * they must outlive the handle.  Creation scans the row lengths once (synchronises the
 * stream) and splits rows longer than 1024 entries into 512-entry chunks that are
 * reduced in a fixed order, so results do not depend on scheduling.  The partial-sum
 * scratch of those chunks (256 floats per chunk) is allocated here, once. */
int tagrec_graph_create(tagrec_graph** out, int64_t n_rows, int64_t n_cols, int64_t nnz,
                        const int64_t* rowptr, const int32_t* colidx, const float* vals, void* stream);
/* A second matrix over the SAME row pointer (same rows, same entries per row) with its own column indices / values,
 * e.g. the two inverted neighbour tables of the TGCN attention backward: shares `like`'s long-row work list instead of
 * scanning again (no synchronisation).  `like` must outlive the new handle. */
int tagrec_graph_create_like(tagrec_graph** out, const tagrec_graph* like, int64_t n_cols, const int32_t* colidx,
                             const float* vals);
/* The same two constructors on a CALLER-PROVIDED workspace of tagrec_graph_workspace(nnz) bytes (256-byte aligned, must
 * outlive the handle): nothing is allocated or freed on the device -- for matrices built and dropped inside a training
 * step (the inverted neighbour tables of the TGCN attention backward, tgcn.py:20-37).  create_ws still reads two counters
 * back (one stream synchronisation); create_like_ws is asynchronous. */
int64_t tagrec_graph_workspace(int64_t nnz);
int tagrec_graph_create_ws(tagrec_graph** out, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* rowptr,
                           const int32_t* colidx, const float* vals, void* workspace, int64_t workspace_bytes, void* stream);
/* The same, without the host read of the long-row counters (a read waits for the stream: the TGCN step builds twelve
 * inverted tables per step).  The work list is sized by its upper bounds, unused slots are marked and skipped by the
 * kernels; accepted by the tagrec_spmm_*, tagrec_attn_pull_* entry points, refused by the tagrec_route_* ones. */
int tagrec_graph_create_ws_deferred(tagrec_graph** out, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* rowptr,
                                    const int32_t* colidx, const float* vals, void* workspace, int64_t workspace_bytes,
                                    void* stream);
int tagrec_graph_create_like_ws(tagrec_graph** out, const tagrec_graph* like, int64_t n_cols, const int32_t* colidx,
                                const float* vals, void* workspace, int64_t workspace_bytes);
int tagrec_graph_destroy(tagrec_graph* g);
int tagrec_graph_info(const tagrec_graph* g, int64_t* n_rows, int64_t* n_cols, int64_t* nnz,
                      int64_t* n_long_rows, int64_t* n_chunks);

/* Y[n_rows,D] = A @ X[n_cols,D]            -- `split_mm` / torch.sparse.mm, adj.py:158-167.
 * The autograd backward dX = A^T dY is the same call on the transposed graph
 * (bi_norm adjacency is symmetric: the same handle). */
int tagrec_spmm_f32(const tagrec_graph* g, const float* X, float* Y, int D, void* stream);

/* One LightGCN layer, fused (lightgcn.py:54-58 + the mean of :60):
 *   Y_raw = A @ X;  inv_norm[r] = 1 / max(||Y_raw[r]||_2, 1e-12);
 *   acc[r] += acc_scale * Y_raw[r] / max(||Y_raw[r]||_2, 1e-12)
 * Y_raw feeds the next layer; acc is the running layer mean. */
int tagrec_spmm_norm_acc_f32(const tagrec_graph* g, const float* X, float* Y_raw, float* inv_norm,
                             float* acc, float acc_scale, int D, void* stream);

/* Backward of one layer, fused:  G_out = A @ G_in + normalize_bwd(X_raw, inv_norm, d_scale * dZ)
 * where normalize_bwd is the gradient of F.normalize(p=2, eps=1e-12) (lightgcn.py:57) at X_raw. */
int tagrec_spmm_normbwd_f32(const tagrec_graph* g, const float* G_in, const float* X_raw,
                            const float* inv_norm, const float* dZ, float d_scale, float* G_out,
                            int D, void* stream);

/* G_out = A @ G_in + b_scale * B      (last backward hop into the ego table; NGCF dX = dX_direct + A^T dN) */
int tagrec_spmm_axpy_f32(const tagrec_graph* g, const float* G_in, const float* B, float b_scale,
                         float* G_out, int D, void* stream);

/* The forward / backward LightGCN layers with MESSAGE DROPOUT (F.dropout on the product, model/lightgcn.py:56) inside
 * the epilogue: Y_raw = mask * (A @ X) / (1 - p) before it is normalised and accumulated; in the backward layer the
 * same mask multiplies the gradient that leaves the layer.  Whether element i survives is a pure function of
 * (seed, i) (counter-based generator, csrc/common.h), so nothing is stored between the passes; the caller uses one
 * seed per layer and step.  tagrec_dropout_f32 applies the identical mask to a plain [n] buffer (n % 4 == 0): the
 * last layer's normalize-backward, NGCF / TGCN layer outputs, tests.  Training-mode parity with the reference is
 * statistical (it draws torch's generator). */
int tagrec_spmm_norm_acc_drop_f32(const tagrec_graph* g, const float* X, float* Y_raw, float* inv_norm,
                                  float* acc, float acc_scale, float drop_p, uint64_t seed, int D, void* stream);
int tagrec_spmm_normbwd_drop_f32(const tagrec_graph* g, const float* G_in, const float* X_raw,
                                 const float* inv_norm, const float* dZ, float d_scale, float drop_p,
                                 uint64_t seed, float* G_out, int D, void* stream);
int tagrec_dropout_f32(const float* x, float* out, int64_t n, float p, uint64_t seed, void* stream);
/* The same mask on a compact row list: element (j, c) of x [n_rows, D] takes the draw of element (rows[j], c) of the full
 * [N, D] layer output, so a node named by several list slots gets ONE mask (model/ngcf.py:85 drops the full output). */
int tagrec_dropout_rows_f32(const float* x, float* out, const int64_t* rows, int64_t n_rows, int D, float p, uint64_t seed,
                            void* stream);

/* Backward layers on a ROW-SPARSE gradient.  The gradient that enters the backward chain is non-zero on the <= 3 B rows
 * of the batch only, and one hop later on their neighbours, so most rows a backward product would gather are zero.
 * row_flags[c] (uint8) != 0 iff row c holds a non-zero; *count (uint32, device) = how many rows are flagged.  A product
 * given in_flags / in_count does not fetch rows flagged zero -- a x 0 adds exactly 0 -- and consults the flags only
 * while they cover less than 4/5 of the rows (decided on the device, no host read).  in_flags with in_count == NULL:
 * the flags are ALWAYS consulted, so rows flagged zero may hold anything (an operand written on a row subset only).
 *   rownorm_bwd_flags   : tagrec_rownorm_bwd_f32 + flags / count of its output rows (the head of the chain)
 *   spmm_normbwd_sparse : tagrec_spmm_normbwd_drop_f32 reading in_flags (may be NULL) and writing out_flags / out_count
 *                         (may be NULL).  row_mask (may be NULL): rows whose byte is 0 are left alone -- for a caller
 *                         who knows their result is zero (no flagged neighbour, and X_raw / inv_norm / dZ zero there, as
 *                         after the row-restricted forward) and has zeroed those rows of G_out / out_flags itself
 *   spmm_axpy_sparse    : tagrec_spmm_axpy_f32 reading in_flags (may be NULL)
 * dz_flags / b_flags (may be NULL): dz_flags[r] == 0 promises that row r of dZ (of B) is zero; the row's epilogue term
 * then vanishes and neither dZ nor X_raw is read for it.  The gradient of a BPR batch w.r.t. the layer mean is non-zero
 * on the <= 3 B batch rows only, so every backward layer skips 2 N D floats of epilogue reads.
 * A product given in_flags walks a row's entries 64 at a time, keeps the entries whose operand row is flagged (order
 * preserved) and gathers those alone. */
int tagrec_rownorm_bwd_flags_f32(const float* X_raw, const float* inv_norm, const float* dZ, int64_t lddz,
                                 float d_scale, float* dX, int accumulate, int64_t n_rows, int D,
                                 uint8_t* row_flags, unsigned* count, void* stream);
int tagrec_spmm_normbwd_sparse_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags,
                                   const unsigned* in_count, const float* X_raw, const float* inv_norm,
                                   const float* dZ, float d_scale, float drop_p, uint64_t seed, float* G_out,
                                   uint8_t* out_flags, unsigned* out_count, const uint8_t* row_mask,
                                   const uint8_t* dz_flags, int D, void* stream);
int tagrec_spmm_axpy_sparse_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags /* may be NULL */,
                                const unsigned* in_count, const float* B, float b_scale, float* G_out,
                                const uint8_t* row_mask /* may be NULL; as in spmm_normbwd_sparse */,
                                const uint8_t* b_flags, int D, void* stream);
/* G_out = A @ G_in on a row-sparse operand (in_flags / in_count as above; row_mask optional), writing the row flags of
 * the result (out_flags; out_count optional).  The backward hop of a column-sharded table, whose normalize-backward term
 * needs row dots over every rank's columns and is added on the batch rows by the caller. */
int tagrec_spmm_flags_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags, const unsigned* in_count,
                          float* G_out, uint8_t* out_flags, unsigned* out_count, const uint8_t* row_mask, int D, void* stream);
/* Forward layer on a SUBSET of the output rows.  The loss reads the propagated table at the batch rows only
 * (model/lightgcn.py:71-75), so the last layer is needed on those rows and the layer below it on their neighbours.
 *   graph_mark_rows   : flags[c] = 1 for every column index stored in the listed rows and for the rows themselves
 *                       (flags uint8 [n_rows], zeroed / pre-marked by the caller; square adjacency)
 *   spmm_norm_acc_rows: tagrec_spmm_norm_acc_drop_f32 for the rows with row_mask[r] != 0 (NULL = every row); the other
 *                       rows of Y_raw, inv_norm and acc are left untouched.  acc may be NULL: the layer mean is then
 *                       not accumulated (a caller that reads it at a few rows forms it there from Y_raw and inv_norm) */
int tagrec_graph_mark_rows_u8(const tagrec_graph* g, const int64_t* rows, int64_t n_listed, uint8_t* flags, void* stream);
/* the same for a rectangular matrix: flags (uint8 [n_cols]) of the columns stored in the listed rows, rows not marked */
int tagrec_graph_mark_cols_u8(const tagrec_graph* g, const int64_t* rows, int64_t n_listed, uint8_t* flags, void* stream);
int tagrec_spmm_norm_acc_rows_f32(const tagrec_graph* g, const float* X, float* Y_raw, float* inv_norm,
                                  float* acc, float acc_scale, const uint8_t* row_mask, float drop_p,
                                  uint64_t seed, int D, void* stream);
/* the plain product (NGCF) and the column-sharded forward product on the rows with row_mask[r] != 0 */
int tagrec_spmm_rows_f32(const tagrec_graph* g, const float* X, float* Y, const uint8_t* row_mask, int D, void* stream);
int tagrec_spmm_ss_rows_f32(const tagrec_graph* g, const float* X, float* Y, float* ss, const uint8_t* row_mask, int D,
                            void* stream);
/* The plain product on a short LIST of rows with a compact result: Y[k, :] = (A @ X)[rows[k], :], k < n_listed
 * (rows int64, may repeat; rows[k] is NOT range-checked on the device -- the caller guarantees 0 <= rows[k] < n_rows).
 * Every listed row is cut into 32 ranges summed by separate blocks (batch rows are popular items: 1e5 entries), partial
 * rows go to `ws` (tagrec_spmm_listed_workspace(n_listed, D) floats, caller-provided) and are added in a fixed order.
 * This is the top layer of a training step -- the loss reads it at the <= 3 B batch rows (model/lightgcn.py:71-75) -- and,
 * with A = the column slice A[:, rows_g] of a row-sharded table, rank g's share of it (the 1-D fold partition of
 * adj.py:114-140,158-164 in push form where the output is 3 B rows); the shares are summed by an all-reduce of [3 B, D]. */
int64_t tagrec_spmm_listed_workspace(int64_t n_listed, int D);
int tagrec_spmm_listed_f32(const tagrec_graph* g, const int64_t* rows, int64_t n_listed, const float* X, float* Y,
                           int D, float* ws, int64_t ws_floats, void* stream);
/* Edge dropout (`node_drop`, model/help/adj.py:170-191, used at model/lightgcn.py:50) evaluated INSIDE the products: no
 * dropped CSR is built, no mask is stored, nothing is sorted.  For the stored entry (i, j) of the forward matrix
 *     key  = (uint64(i) << 32) | uint32(j);   h = mix64(seed ^ mix64(key))      (the splitmix64 finaliser of the
 *     keep = (h >> 40) >= (unsigned)(p * 16777216.0f)                             message-dropout masks)
 * a kept entry contributes val / (1 - p) (a true fp32 division, as the reference divides), a dropped one nothing -- its
 * operand row is not fetched; (i, j) and (j, i) draw independently.  ed_transposed != 0: the handle holds the TRANSPOSE
 * of the matrix the mask is defined on (the symmetric bi_norm matrix itself, or an explicit transpose), so the entry met
 * as (row r, column c) takes the draw of (c, r): forward and backward of one step see the same dropped matrix.
 * The `_edrop` forms take the arguments of the product they are named after plus (ed_p, ed_seed, ed_transposed) and need
 * a vector-kernel width (D in {8, 16, 32, 64, 128, 256}, 16-byte aligned operands; anything else is TAGREC_E_UNSUPPORTED):
 *   spmm_edrop                : tagrec_spmm_f32
 *   spmm_norm_acc_rows_edrop  : tagrec_spmm_norm_acc_rows_f32 (row_mask NULL = every row, acc may be NULL)
 *   spmm_normbwd_sparse_edrop : tagrec_spmm_normbwd_sparse_f32 (in_flags NULL = dense operand)
 *   spmm_axpy_sparse_edrop    : tagrec_spmm_axpy_sparse_f32
 *   spmm_listed_edrop         : tagrec_spmm_listed_f32
 *   edge_drop_mask            : mask_out[e] = 1 iff stored entry e (CSR order) is kept -- for tests and for host helpers
 *                               that materialise the dropped matrix */
int tagrec_edge_drop_mask_u8(const tagrec_graph* g, float p, uint64_t seed, int transposed, uint8_t* mask_out, void* stream);
int tagrec_spmm_edrop_f32(const tagrec_graph* g, const float* X, float* Y, float ed_p, uint64_t ed_seed, int ed_transposed,
                          int D, void* stream);
int tagrec_spmm_norm_acc_rows_edrop_f32(const tagrec_graph* g, const float* X, float* Y_raw, float* inv_norm,
                                        float* acc, float acc_scale, const uint8_t* row_mask, float drop_p,
                                        uint64_t seed, float ed_p, uint64_t ed_seed, int ed_transposed, int D, void* stream);
int tagrec_spmm_normbwd_sparse_edrop_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags,
                                         const unsigned* in_count, const float* X_raw, const float* inv_norm,
                                         const float* dZ, float d_scale, float drop_p, uint64_t seed, float* G_out,
                                         uint8_t* out_flags, unsigned* out_count, const uint8_t* row_mask,
                                         const uint8_t* dz_flags, float ed_p, uint64_t ed_seed, int ed_transposed, int D,
                                         void* stream);
int tagrec_spmm_axpy_sparse_edrop_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags,
                                      const unsigned* in_count, const float* B, float b_scale, float* G_out,
                                      const uint8_t* row_mask, const uint8_t* b_flags, float ed_p, uint64_t ed_seed,
                                      int ed_transposed, int D, void* stream);
int tagrec_spmm_listed_edrop_f32(const tagrec_graph* g, const int64_t* rows, int64_t n_listed, const float* X, float* Y,
                                 int D, float* ws, int64_t ws_floats, float ed_p, uint64_t ed_seed, int ed_transposed,
                                 void* stream);
/* Noise perturbation of the SimGCL views (Yu et al., "Are Graph Augmentations Necessary?", SIGIR 2022) evaluated INSIDE the
 * layer kernels: no noise tensor is stored, and the all-rows product, the row-masked product and the compact top layer
 * perturb the same element the same way, because the direction is keyed by NODE ID, not by where the row is stored.
 * For row r (node id), float4 index c (0 <= c < D / 4) of layer `layer` (1-based) of view `view` under the step's `seed`
 *     key = mix64(seed ^ mix64((uint64(view) << 32) | uint32(layer)))            (mix64: the splitmix64 finaliser of the
 *     h   = mix64(key ^ mix64((uint64(r) << 8) | uint64(c)))                       dropout masks)
 *     u[4 c + j] = (((h >> 16 j) & 0xFFFF) + 1) * 2^-16,  j = 0 .. 3            (in (0, 1], exact in fp32)
 *     n(r) = u / ||u||_2     (||u||^2: per float4 fma(u0,u0, fma(u1,u1, fma(u2,u2, u3 u3))), then an xor butterfly over c)
 *     x'   = fma(eps sign(y), n(r), y),  sign(0) = 0       (an empty row stays zero; eps = 0: x' = y)
 * D in {8, 16, 32, 64, 128, 256}; anything else is TAGREC_E_UNSUPPORTED.  eps finite and >= 0, view / layer >= 0.
 *   spmm_norm_acc_noise : tagrec_spmm_norm_acc_rows_f32 (row_mask NULL = every row, rows outside the mask untouched, acc may
 *                         be NULL) with y = the product row replaced by x' BEFORE the sum of squares: Y_raw holds x' (what the
 *                         next layer gathers and what the unchanged backward kernels read), inv_norm = 1 / max(||x'||, 1e-12),
 *                         acc += acc_scale x' inv_norm.  A long row is perturbed once, where its chunks are folded.
 *   noise_rownorm_fwd   : rows of a COMPACT Y [n_rows, D] (e.g. from tagrec_spmm_listed_f32), row t being node node_ids[t]
 *                         (NULL: node t): Y[t] <- x' in place, Z[t] = x' / max(||x'||, 1e-12) (row stride ldz),
 *                         inv_norm[t] (may be NULL).  The same bits as spmm_norm_acc_noise gives for the same product row;
 *                         with eps = 0 the bits of tagrec_rownorm_fwd_f32.
 *   noise_dir           : out[t] = n(node_ids[t]) (NULL: n(t)), [n_rows, D] -- for tests and microbenchmarks; no training
 *                         step calls it. */
int tagrec_spmm_norm_acc_noise_f32(const tagrec_graph* g, const float* X, float* Y_raw, float* inv_norm, float* acc,
                                   float acc_scale, const uint8_t* row_mask, float eps, uint64_t seed, int view, int layer,
                                   int D, void* stream);
int tagrec_noise_rownorm_fwd_f32(float* Y, const int64_t* node_ids, int64_t n_rows, float eps, uint64_t seed, int view,
                                 int layer, float* Z, int64_t ldz, float* inv_norm, int D, void* stream);
int tagrec_noise_dir_f32(float* out, const int64_t* node_ids, int64_t n_rows, uint64_t seed, int view, int layer, int D,
                         void* stream);
/* The masked hop below the top layer of a restricted step, driven by an inverted list of the batch rows' entries instead
 * of a walk over every masked row: G_out[j] = sum_b A[j, b] G_in[b] over the listed rows b, for the rows j of row_mask.
 *   batch_hop_plan   : gt = the TRANSPOSE of A (A itself when A is symmetric); rows = the n_listed (<= 16384) batch rows,
 *                      int64, may repeat (a node counts once).  Builds, on the stream and without a host read, one record
 *                      (destination j, source b, weight) per stored entry of a listed row of gt, grouped by destination
 *                      and ordered by ascending source inside a destination (a counting sort by destination in LDS; the
 *                      order does not depend on its integer atomics), and the list of rows the hop visits: every destination with a record and every
 *                      listed row without one, each once, with its device-side length (the work of plan and hop follows
 *                      the records, not the rows of gt, which must be square with at most 2^24 rows).  `capacity` bounds the record count (the
 *                      sum of the n_listed largest row degrees
 *                      of gt always suffices); records beyond it are dropped -- never written -- and *err |= 1; a listed
 *                      id outside gt's rows is skipped and *err |= 2.  err is only ever set, the caller clears it.
 *                      ws: tagrec_batch_hop_workspace(n_rows, n_listed, capacity) bytes, 256-byte aligned.
 *   batch_hop_normbwd: tagrec_spmm_normbwd_sparse_f32(in_flags = the listed rows, in_count = NULL, row_mask) from that
 *                      plan.  A row of row_mask is written when it has a record, or is a listed row whose dz_flags byte is
 *                      set (NULL = every listed row); the others are left untouched, G_out and out_flags alike.  The launch
 *                      is a fixed grid that strides over the plan's row list, tagrec_batch_hop_grid_rows(D) rows per pass
 *                      (0: D not supported).  Rows of A with at most 1024 stored
 *                      entries get the bits of the masked kernel (the same fused multiply-adds in the same order); longer
 *                      rows are summed in ascending source order as well, in fp64 rounded once, where the masked kernel
 *                      folds chunk partials (last bits may differ; no further from the exact sum). */
int64_t tagrec_batch_hop_workspace(int64_t n_rows, int64_t n_listed, int64_t capacity);
int tagrec_batch_hop_grid_rows(int D);
/* where a built plan keeps its row list inside ws -- what = 0: byte offset of its device-side length (int32, may exceed the
 * capacity after an overflow), 1: byte offset of the list (four int32 per row: row id, start and length of its record
 * segment, unused), 2: its capacity in rows; -1: bad arguments */
int64_t tagrec_batch_hop_list_result(int64_t n_rows, int64_t n_listed, int64_t capacity, int what);
int tagrec_batch_hop_plan(const tagrec_graph* gt, const int64_t* rows, int64_t n_listed, int64_t capacity, void* ws,
                          int64_t ws_bytes, int32_t* err, void* stream);
int tagrec_batch_hop_normbwd_f32(const tagrec_graph* g, const void* ws, int64_t ws_bytes, int64_t n_listed, int64_t capacity,
                                 const float* G_in, const float* X_raw, const float* inv_norm, const float* dZ,
                                 float d_scale, float* G_out, uint8_t* out_flags, const uint8_t* row_mask,
                                 const uint8_t* dz_flags, int D, void* stream);
/* Fixed-order scatter of compact rows into a table, dst[rows[j]] (=|+=) src[j], for a row list that repeats ids: no float
 * atomics, the same bits on every run (config key `deterministic` of LightGCN / NGCF).
 *   rowlist_plan : rows = n_listed int64 ids (may repeat) into a table of n rows.  Builds in ws, on the stream and without a
 *                  host read: order (int32 [n_listed], the slots stably sorted by row id), seg_row (int32, the distinct
 *                  rows ascending), seg_ptr (int32, segment s = order[seg_ptr[s] .. seg_ptr[s + 1])) and counts (int32
 *                  [4]: segments, valid slots, ids outside [0, n), 0).  An id outside [0, n) is dropped from the plan and
 *                  counted.  ws: tagrec_rowlist_workspace(n_listed, width) bytes, 256-byte aligned, width = the widest row
 *                  the plan will scatter; part p of the plan (0 order, 1 seg_row, 2 seg_ptr, 3 counts) starts at byte
 *                  tagrec_rowlist_plan_result(n_listed, width, p).
 *   row_scatter_ordered : dst[seg_row[s]] = (accumulate ? dst[seg_row[s]] : 0) + sum of src[order[j]] over segment s.  src
 *                  [n_listed, D] with row stride lds, dst [n_dst >= n, D] with row stride ldd, D <= width.  The order of
 *                  the sum is part of the contract: ascending slot id; a segment of <= 1024 slots is one left-to-right
 *                  fp32 chain from its first term; a longer one is cut into consecutive 1024-slot chunks, each such a
 *                  chain, whose sums are added left to right.  dst is touched once per segment (a store, or one fp32 add
 *                  of the finished sum); rows outside the list are not touched.  D in {8, .., 256} with 16-byte aligned
 *                  rows takes D / 4 lanes x 16 bytes per row, anything else one lane per column.  A plan serves one
 *                  stream at a time (the chunk sums live in its workspace). */
int64_t tagrec_rowlist_workspace(int64_t n_listed, int width);
int64_t tagrec_rowlist_plan_result(int64_t n_listed, int width, int part);
int tagrec_rowlist_plan_i64(const int64_t* rows, int64_t n_listed, int64_t n, int width, void* ws, int64_t ws_bytes,
                            void* stream);
int tagrec_row_scatter_ordered_f32(const void* ws, int64_t ws_bytes, int64_t n_listed, int width, const float* src,
                                   int64_t lds, float* dst, int64_t ldd, int64_t n_dst, int D, int accumulate, void* stream);
/* tagrec_spmm_normbwd_dot_f32 (column-sharded tables) on a row-sparse G_in */
int tagrec_spmm_normbwd_dot_sparse_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags,
                                       const unsigned* in_count, const float* X_raw, const float* inv_norm,
                                       const float* dZ, const float* dot, float d_scale, float* G_out,
                                       uint8_t* out_flags, unsigned* out_count, const uint8_t* row_mask, int D,
                                       void* stream);
/* row_flags[r] = (row r of X [n_rows, D] holds a non-zero), *count = number of such rows: for operands whose producer
 * does not write flags itself (the NGCF backward's dN). */
int tagrec_row_flags_f32(const float* X, int64_t n_rows, int D, uint8_t* row_flags, unsigned* count, void* stream);

/* ---- column-sharded tables (feature sharding over GPUs: every rank holds D/G columns of every row) ---------------
 * Whatever reduces over a row's columns is split into a local part, an all-reduce done by the caller, and an apply:
 *   spmm_ss          : Y = A @ X;  ss[r] = sum_c Y[r,c]^2 over the local columns
 *   row_scale_acc    : acc[r,:] += s * inv[r] * Y[r,:]                          (inv from the all-reduced ss)
 *   row_dot          : out[r] = inv[r] * s * sum_c X[r,c] dZ[r,c]               (local part of z . (s dZ))
 *   rownorm_bwd_dot  : dX[r,:] = inv[r] * (s dZ[r,:] - X[r,:] inv[r] dot[r])    (dot all-reduced)
 *   spmm_normbwd_dot : G_out = A @ G_in + the same expression                   (fused backward layer)
 *   bpr_dots         : dots[b] = (u.p, u.n, 0.5(|u|^2+|p|^2+|n|^2)) over the local columns */
int tagrec_spmm_ss_f32(const tagrec_graph* g, const float* X, float* Y, float* ss, int D, void* stream);
int tagrec_spmm_normbwd_dot_f32(const tagrec_graph* g, const float* G_in, const float* X_raw, const float* inv_norm,
                                const float* dZ, const float* dot, float d_scale, float* G_out, int D, void* stream);
int tagrec_row_scale_acc_f32(const float* Y, const float* inv, float s, float* acc, int64_t n_rows, int D, void* stream);
int tagrec_row_dot_f32(const float* X, const float* inv, const float* dZ, float s, float* out, int64_t n_rows, int D,
                       void* stream);
int tagrec_rownorm_bwd_dot_f32(const float* X, const float* inv, const float* dZ, const float* dot, float s, float* dX,
                               int64_t n_rows, int D, void* stream);
int tagrec_bpr_dots_f32(const float* U, const float* I, int64_t ld, int D, const float* Ureg, const float* Ireg,
                        int64_t ldreg, int Dreg, const int64_t* trip, int64_t B, float* dots, void* stream);

/* ---- F.normalize(p=2, dim=1, eps=1e-12) as standalone kernels (ngcf.py:86, tgcn.py:220-222) ----
 * fwd: Z (row stride ldz floats, so it can write one slot of a concat buffer) and inv_norm.
 * bwd: dX = normalize_bwd(X_raw, inv_norm, d_scale * dZ); dZ has row stride lddz; if `accumulate`
 *      the result is added to dX. */
int tagrec_rownorm_fwd_f32(const float* X, float* Z, int64_t ldz, float* inv_norm, int64_t n_rows, int D, void* stream);
int tagrec_rownorm_bwd_f32(const float* X_raw, const float* inv_norm, const float* dZ, int64_t lddz,
                           float d_scale, float* dX, int accumulate, int64_t n_rows, int D, void* stream);

/* ---- BPR triplet loss (lightgcn.py:68-82, ngcf.py:95-105, loss.py:4-12, 27-32) -------------------
 * trip: int64 [B,3] = (user, pos_item, neg_item), item ids local to the item table.
 * U/I: propagated user/item tables (row stride ld floats, width D); Ureg/Ireg (stride ldreg, width Dreg):
 * the rows the L2 term reads (ego tables for LightGCN, the propagated ones for NGCF/TGCN).
 * fwd writes loss_out[0] = mul_loss, loss_out[1] = l2reg_loss (unweighted), and coef[b] =
 * d mul_loss_b / d(neg_b - pos_b) (a sigmoid) for the backward.  `partials` is scratch of
 * 2*ceil(B/4) floats (two per launched block, four triplets per block); the two-stage reduction is
 * deterministic. */
int tagrec_bpr_fwd_f32(const float* U, const float* I, int64_t ld, int D,
                       const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                       const int64_t* trip, int64_t B, int loss_kind,
                       float* coef, float* partials, float* loss_out, void* stream);
/* bwd scatter-adds (float atomics) into dU/dI (stride ld) and dUreg/dIreg (stride ldreg):
 *   dU[u] += g0*coef/B * (I[n]-I[p]);  dI[p] -= g0*coef/B * U[u];  dI[n] += g0*coef/B * U[u]
 *   dXreg[row] += g1 * reg / B * Xreg[row]     for the three rows of every triplet
 * g = device pointer to two floats (upstream gradients of the two loss parts) or NULL for (1,1).
 * Where the L2 part reads the main tables and shares their gradient buffers (Ureg == U, Ireg == I, dUreg == dU,
 * dIreg == dI, same stride and width) a slot adds its two terms as ONE value: a row that two triplets name is then a
 * sum of two additions, the same bits in either order.
 * Callers zero the gradient buffers.  dU = dI = NULL runs the L2 part only (so it can be added
 * after the propagation backward has overwritten the ego gradient). */
int tagrec_bpr_bwd_f32(const float* U, const float* I, int64_t ld, int D,
                       const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                       const int64_t* trip, int64_t B, const float* coef, const float* g, float reg,
                       float* dU, float* dI, float* dUreg, float* dIreg, void* stream);

/* ---- Multi-negative ranking losses on COMPACT (already gathered) rows: sampled softmax, K-negative BPR ----
 * A batch of B tuples (user, positive, K negatives), K in 1 .. 63 (the K + 1 scores of a tuple sit one per lane of a
 * wavefront).  Ub [B, D]: the user rows; Ib [(1 + K) B, D]: item j of tuple b is row j B + b, j = 0 the positive; both
 * with row stride ld floats.  Ureg [B, Dreg] / Ireg [(1 + K) B, Dreg] (stride ldreg): the rows the L2 term reads, in the
 * same slot order (both NULL: no L2 term).  No index array is read: no two slots share a row.
 * Scores s_j = Ub[b] . Ib[j B + b];  loss_b by loss_kind:
 *   TAGREC_LOSS_SOFTMAX                 logsumexp_j(s_j / temperature) - s_0 / temperature  (maximum subtracted)
 *   TAGREC_LOSS_SOFTPLUS / _LOGSIGMOID  mean over k = 1 .. K of the triplet loss's per-pair expression of (s_0, s_k),
 *                                       softplus's gradient pass-through past 20 included (temperature is not read)
 * fwd writes loss_out[0] = mean_b loss_b, loss_out[1] = 0.5 sum |row|^2 / B over all (2 + K) B L2 rows (unweighted), and
 * coef [B, K + 1] = d loss_b / d s_j (1 / temperature and 1 / K folded in; entry 0 is minus the sum of the others).
 * `partials`: scratch of 2*ceil(B/4) floats; the two-stage reduction is deterministic. */
int tagrec_rank_fwd_f32(const float* Ub, const float* Ib, int64_t ld, int D,
                        const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                        int64_t B, int K, int loss_kind, float temperature,
                        float* coef, float* partials, float* loss_out, void* stream);
/* bwd STORES (no atomics, no read of the old contents; a pure function of its inputs) every row of
 *   dUb[b]       = g0 / B * sum_j coef[b, j] * Ib[j B + b]     (ascending j)
 *   dIb[j B + b] = g0 / B * coef[b, j] * Ub[b]
 *   dXreg[row]   = g1 / B * Xreg[row]                          for the (2 + K) B L2 rows
 * g = device pointer to two floats (upstream gradients of the two loss parts) or NULL for (1, 1).  dUb = dIb = NULL runs
 * the L2 part only.  dUreg = dUb and dIreg = dIb (one buffer for both parts) is allowed when Ureg = Ub, Ireg = Ib with
 * the same stride and width: each row then receives the sum of its two terms in one store. */
int tagrec_rank_bwd_f32(const float* Ub, const float* Ib, int64_t ld, int D,
                        const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                        int64_t B, int K, const float* coef, const float* g,
                        float* dUb, float* dIb, float* dUreg, float* dIreg, void* stream);

/* ---- Weighted pointwise binary cross-entropy on COMPACT rows (UltraGCN; csrc/rowops.hip) ----
 * The slot layout of the rank kernels with S = 1 + K + M slots per tuple: Ub [B, D], Ib [S B, D], slot j of tuple b at row
 * j B + b; j = 0 the positive, 1 .. K the negatives, K + 1 .. K + M the positive's co-occurrence neighbours.  K >= 1,
 * M >= 0, S <= 4096 (the kernels loop over the slots).  Labels t_j = +1 for j = 0 and j > K, -1 for the negatives;
 * weight [B, S] (contiguous, >= 0).  With s_bj = Ub[b] . Ib[j B + b] and softplus(x) = max(x, 0) + log1p(exp(-|x|)):
 *   loss_out[0] = (1 / B) sum_b sum_j weight[b, j] softplus(-t_j s_bj)
 *   loss_out[1] = 0.5 (|Ureg[b]|^2 + sum_{j <= K} |Ireg[j B + b]|^2) / B summed over b (the neighbour slots carry no L2)
 *   coef [B, S] = -t_j weight[b, j] sigmoid(-t_j s_bj) / B         (1 / B folded in; a zero weight gives an exact zero)
 * `partials`: scratch of 2*ceil(B/4) floats; the two-stage reduction is deterministic. */
int tagrec_wbce_fwd_f32(const float* Ub, const float* Ib, int64_t ld, int D,
                        const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                        int64_t B, int K, int M, const float* weight,
                        float* coef, float* partials, float* loss_out, void* stream);
/* bwd STORES (no atomics, no read of the old contents) every row of
 *   dUb[b]       = g0 * sum_j coef[b, j] * Ib[j B + b]     (ascending j)
 *   dIb[j B + b] = g0 * coef[b, j] * Ub[b]
 *   dUreg[b] = g1 / B * Ureg[b];  dIreg[j B + b] = g1 / B * Ireg[j B + b] for j <= K and 0 for the neighbour slots
 * g, the NULL forms and the shared-buffer form (dUreg = dUb, dIreg = dIb with Ureg = Ub, Ireg = Ib) as in tagrec_rank_bwd_f32. */
int tagrec_wbce_bwd_f32(const float* Ub, const float* Ib, int64_t ld, int D,
                        const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                        int64_t B, int K, int M, const float* coef, const float* g,
                        float* dUb, float* dIb, float* dUreg, float* dIreg, void* stream);

/* ---- Item co-occurrence top-k: the k heaviest columns of every row of the sparse A^T A (csrc/cooc.hip) ----
 * A = the 0 / 1 user x item train matrix, given as two CSRs with sorted, duplicate-free rows: item -> users (iu_ptr
 * [n_item + 1], iu_idx) and user -> items (ui_ptr [n_user + 1], ui_idx); every id must lie inside its range (not checked on
 * the device).  c_ij = |N(i) n N(j)|, c_ii = deg(i), D_i = sum_j c_ij; zero_diagonal: c_ii counts as 0.
 *   tagrec_cooc_degree_i64     D [n_item] = sum_{u in N(i)} deg(u) [- deg(i)]
 *   tagrec_cooc_topk_*_f32     for every listed item i (items [n_listed], int32, no repeats): row i of nbr_id / nbr_w
 *                              [n_item, k] = the first k candidates j (c_ij > 0) in descending fp64 c_ij^2 / (D_j + 1), ties to
 *                              the lower id, padded with -1 / 0;  nbr_w = (float)(c_ij sqrt(D_i + 1) / D_i / sqrt(D_j + 1)),
 *                              formed in fp64.  1 <= k <= 64.  Rows of items that are not listed are not touched.
 * Counts are summed with integer atomics only: the outputs do not depend on the execution order.
 *   light: one block per listed item, counts in an LDS hash table; every listed item needs D_i <= tagrec_cooc_lds_limit()
 *          (an item above it gets an all-pad row).
 *   heavy: any D_i; `workspace` = rows x n_item int32, ALL ZERO on entry and all zero again on return; min(rows, n_listed,
 *          tagrec_cooc_max_rows()) blocks each own one counter row and take the listed items in turn.
 *   hub:   a listed item's walk cut into n_part parts (part p: hub part_hub[p], users iu_idx[part_u0[p] .. part_u1[p]); the parts of
 *          hub h are hub_part_ptr[h] .. hub_part_ptr[h + 1], contiguous, and cover its user list exactly once), one block per part;
 *          `workspace` = n_hub x n_item int32, all zero on entry and on return; part_id / part_c: scratch of n_part x k int32.
 *          Three launches: every part adds into its hub's row, every part exchanges and keeps its k best, one block per hub merges. */
int tagrec_cooc_lds_limit(void);
int tagrec_cooc_max_rows(void);
int tagrec_cooc_topk_hub_f32(const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, const int32_t* ui_idx,
                             const int64_t* D, const int32_t* hub_items, int64_t n_hub, const int32_t* part_hub,
                             const int64_t* part_u0, const int64_t* part_u1, int64_t n_part, const int64_t* hub_part_ptr,
                             int64_t n_item, int k, int zero_diagonal, int32_t* workspace, int32_t* part_id,
                             int32_t* part_c, int32_t* nbr_id, float* nbr_w, void* stream);
int tagrec_cooc_degree_i64(const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, int64_t n_item,
                           int zero_diagonal, int64_t* D, void* stream);
int tagrec_cooc_topk_light_f32(const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, const int32_t* ui_idx,
                               const int64_t* D, const int32_t* items, int64_t n_listed, int64_t n_item, int k,
                               int zero_diagonal, int32_t* nbr_id, float* nbr_w, void* stream);
int tagrec_cooc_topk_heavy_f32(const int64_t* iu_ptr, const int32_t* iu_idx, const int64_t* ui_ptr, const int32_t* ui_idx,
                               const int64_t* D, const int32_t* items, int64_t n_listed, int64_t n_item, int k,
                               int zero_diagonal, int32_t* workspace, int64_t rows, int32_t* nbr_id, float* nbr_w,
                               void* stream);

/* ---- In-batch sampled softmax on COMPACT rows: a fused B x B loss, the score matrix is never stored (csrc/inbatch.hip) ----
 * Ub [B, D] and Ib [B, D] (row stride ld floats): row b of Ib is the positive of row b of Ub, and every other row of Ib is
 * a negative of it.  The kernels do not know what the two operands stand for (users / items, or two views of one node set).
 * uid, iid: int64 [B], the ids behind the rows, read for the mask only (both NULL: nothing is masked).  col_bias: float [B]
 * or NULL.  Ureg / Ireg [B, Dreg] (stride ldreg): the rows the L2 term reads (both NULL: no L2 term).
 *   s_bj   = Ub[b] . Ib[j]                        (exact-fp32 MFMA 16x16x4, ascending feature blocks)
 *   z_bj   = s_bj / temperature - col_bias[j]     (every j, the diagonal included)
 *   masked   (b, j), j != b, with iid[j] == iid[b] (the row's own positive) or uid[j] == uid[b] (another positive of the same
 *            user): left out of the softmax entirely
 *   loss_b = logsumexp_{j unmasked} z_bj - z_bb   (running maximum; a row whose every other column is masked: exactly 0)
 * fwd writes loss_out[0] = mean_b loss_b, loss_out[1] = 0.5 sum |row|^2 / B over the 2 B L2 rows (unweighted) and
 * lse [B] = the row log-sum-exp the backward reads.  `partials`: scratch of 2*ceil(B/64) floats; the reduction over b runs
 * in a fixed order.  D must be a multiple of 4 in 8 .. 256 and 1 <= B <= 65536, anything else is TAGREC_E_UNSUPPORTED. */
int tagrec_inbatch_fwd_f32(const float* Ub, const float* Ib, int64_t ld, int D,
                           const int64_t* uid, const int64_t* iid, const float* col_bias,
                           const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                           int64_t B, float temperature,
                           float* lse, float* partials, float* loss_out, void* stream);
/* bwd STORES (no atomics, no read of the old contents; a pure function of its inputs, the summation order is a function of
 * (B, D) only) every row of
 *   dUb[b]     = sum_j C_bj Ib[j]                 (ascending j)
 *   dIb[j]     = sum_b C_bj Ub[b]                 (ascending b)
 *   C_bj       = g0 / (temperature B) * (exp(z_bj - lse[b]) - [b == j]), 0 where masked
 *   dXreg[row] = g1 / B * Xreg[row]               for the 2 B L2 rows (dUreg = dIreg = NULL: not written)
 * g = device pointer to two floats (upstream gradients of the two loss parts) or NULL for (1, 1).  dUreg = dUb and
 * dIreg = dIb (one buffer for both parts) is allowed when Ureg = Ub, Ireg = Ib with the same stride and width: each row
 * then receives the sum of its two terms in one store. */
int tagrec_inbatch_bwd_f32(const float* Ub, const float* Ib, int64_t ld, int D,
                           const int64_t* uid, const int64_t* iid, const float* col_bias,
                           const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                           int64_t B, float temperature, const float* lse, const float* g,
                           float* dUb, float* dIb, float* dUreg, float* dIreg, void* stream);

/* ---- Catalogue softmax: a fused rectangular B x N softmax cross-entropy, the logits are never stored (csrc/catsoftmax.hip) ----
 * Q: float rows (stride ldq), row b of the problem is Q[qrow[b]] (qrow int64 [B]; NULL: row b).  T [N, D] (stride ldt): the
 * column table.  target: int64 [B] in [0, N).  The kernels do not know what the operands stand for (users against the item
 * catalogue, nodes against a centroid table).  Qreg (read at qrow) / Treg (read at target), width Dreg, stride ldreg: the rows
 * the L2 term reads (both NULL: no L2 term); they may alias Q / T.
 *   z_bn   = Q[qrow_b] . T[n] / temperature       (exact-fp32 MFMA 16x16x4, ascending feature blocks; one rounding for 1 / t)
 *   loss_b = logsumexp_n z_bn - z_{b, target_b}   (>= 0 in floating point: zt comes from the tile that feeds the row sum)
 * The column tiles (64 rows of T) are cut into n_split contiguous ranges of ceil(tiles / n_split) tiles, one block per (64-row
 * tile of Q, range); a range past the last tile is empty.  n_split = 0: tagrec_catsoftmax_splits(B, N, D), the library's
 * default (a pure function, >= 1); any other value in 1 .. 65535 is forced.  workspace: tagrec_catsoftmax_workspace(B, N, D,
 * n_split) bytes, 4-byte aligned; nothing is kept in it between the forward and the backward.
 * fwd writes lse [B], zt [B] (the target logit), loss_out[0] = mean_b (lse_b - zt_b) and loss_out[1] = 0.5 sum_b (|Qreg row|^2
 * + |Treg row|^2) / B (unweighted; 0 without an L2 term).  Every row keeps a running (maximum, sum) per lane, started at a
 * finite sentinel; lanes, then ranges (ascending, an empty one is (sentinel, 0)) are merged by one rescale and add each.
 * D must be a multiple of 4 in 8 .. 256, 1 <= B <= 65536, N >= 1: anything else is TAGREC_E_UNSUPPORTED.  A target outside
 * [0, N) is the caller's error: no access leaves the operands (the L2 read is clamped), zt[b] is then left unwritten. */
int tagrec_catsoftmax_splits(int64_t B, int64_t N, int D);
int64_t tagrec_catsoftmax_workspace(int64_t B, int64_t N, int D, int n_split);
int tagrec_catsoftmax_fwd_f32(const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt, int64_t N, int D,
                              const int64_t* target, const float* Qreg, const float* Treg, int64_t ldreg, int Dreg,
                              int64_t B, float temperature, int n_split, void* workspace, int64_t workspace_bytes,
                              float* lse, float* zt, float* loss_out, void* stream);
/* bwd STORES (no atomics, no read of the old contents; the summation order is a function of (B, N, D, n_split) only)
 *   dT[n]      = sum_b C_bn Q[qrow_b]             every row of the dense [N, D] (stride lddt), ascending b
 *   dQ[b]      = sum_n C_bn T[n]                  every row of the compact, contiguous [B, D]: ascending n within a range
 *                                                 (partial rows in the workspace), then ascending ranges
 *   C_bn       = g0 / (temperature B) * (exp(z_bn - lse[b]) - [n == target_b])
 *   dQreg[b]   = g1 / B * Qreg[qrow_b], dTreg[b] = g1 / B * Treg[target_b]     compact, contiguous [B, Dreg] (both NULL: not written)
 * g = device pointer to two floats (upstream gradients of the two loss parts) or NULL for (1, 1).  dT = dQ = NULL: the L2
 * part only.  Repeated qrow ids and repeated targets are the caller's to fold. */
int tagrec_catsoftmax_bwd_f32(const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt, int64_t N, int D,
                              const int64_t* target, const float* Qreg, const float* Treg, int64_t ldreg, int Dreg,
                              int64_t B, float temperature, int n_split, void* workspace, int64_t workspace_bytes,
                              const float* lse, const float* g, float* dT, int64_t lddt, float* dQ, float* dQreg, float* dTreg,
                              void* stream);
/* The MASKED form: the two calls above with a list of excluded columns per row of Q, a CSR in the conventions of
 * tagrec_eval_topk_f32's train lists: mask_ptr int64 [rows of Q + 1], mask_cols int32, ascending and unique within a row;
 * batch row b uses CSR row qrow[b] (qrow NULL: row b).  With E_b = list(qrow_b) \ {target_b}
 *   loss_b = log sum_{n not in E_b} exp(z_bn) - z_{b, target_b},   C_bn = 0 EXACTLY for n in E_b
 * (an excluded column is never added to a row's running sum and its coefficient is a stored 0.0f, not a product); the target
 * column stays live whether or not the list names it.  A row whose only live column is its target has lse_b == zt_b bit
 * for bit, and the backward, which finds such a row by the length of its list, takes p_target = 1: the row's coefficients,
 * its dQ row and its share of dT are exactly 0 (formed from the logits they would be the rounding residue of zt).  Everything
 * else -- the split, the workspace (same size), the L2 part, the orders of summation, now a function of (B, N, D, n_split,
 * lists) -- is as above, and with every list empty the outputs are the unmasked calls' bits (N = 1 aside: there every
 * row is such a row).  N <= 2^31 - 1
 * (TAGREC_E_UNSUPPORTED otherwise); both pointers are required.  The lists are not validated: an unsorted list gives an
 * unspecified mask, but no read leaves [mask_ptr[r], mask_ptr[r + 1]) of mask_cols. */
int tagrec_catsoftmax_masked_fwd_f32(const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt, int64_t N,
                                     int D, const int64_t* target, const float* Qreg, const float* Treg, int64_t ldreg,
                                     int Dreg, int64_t B, float temperature, int n_split, void* workspace,
                                     int64_t workspace_bytes, float* lse, float* zt, float* loss_out, void* stream,
                                     const int64_t* mask_ptr, const int32_t* mask_cols);
int tagrec_catsoftmax_masked_bwd_f32(const float* Q, int64_t ldq, const int64_t* qrow, const float* T, int64_t ldt, int64_t N,
                                     int D, const int64_t* target, const float* Qreg, const float* Treg, int64_t ldreg,
                                     int Dreg, int64_t B, float temperature, int n_split, void* workspace,
                                     int64_t workspace_bytes, const float* lse, const float* g, float* dT, int64_t lddt,
                                     float* dQ, float* dQreg, float* dTreg, void* stream, const int64_t* mask_ptr,
                                     const int32_t* mask_cols);

/* ---- K22: nearest-centroid assignment, the E-step of k-means; the n x K distances are never stored (csrc/kmeans.hip) ----
 * X [n, D] (row stride ldx floats): the rows to assign.  C [K, D] (stride ldc): the centroids.  The tile scheme is the pair
 * kernels' (csrc/pairtile.h): a block owns 64 rows of X and walks every 64-row tile of C; there is no column split, so a call
 * with few rows and very many centroids walks serially.
 *   h_j    = 0.5 |c_j|^2                           (one fmaf chain over ascending d, then * 0.5f: the same expression for
 *                                                   every column, written to half_norm [K] -- scratch the caller provides)
 *   s_ij   = x_i . c_j - h_j                       (exact-fp32 MFMA 16x16x4, ascending feature blocks; one subtraction)
 *   assign[i] = argmax_j s_ij                      = the Euclidean nearest centroid; TIES GO TO THE LOWER ID
 *   best[i]   = s_{i, assign_i}                    (NULL: not written); the inertia is sum_i |x_i|^2 - 2 best_i
 * Two identical rows of C score bit-identically, so the lower of their ids wins every row.  A column past K is never admitted
 * (it would score 0), padded feature columns add exact zeros.  No atomics, nothing allocated: the outputs are a pure function
 * of the operands.  D must be a multiple of 4 in 8 .. 256, n >= 1 and 1 <= K <= 2^31 - 1: anything else is
 * TAGREC_E_UNSUPPORTED.  Rows that are 16-byte aligned with a stride that is a multiple of 4 are staged by float4 loads, any
 * other by scalar loads.  NaN / Inf operands give an unspecified assignment inside [0, K); no read leaves the operands. */
int tagrec_kmeans_assign_f32(const float* X, int64_t ldx, int64_t n, const float* C, int64_t ldc, int64_t K, int D,
                             float* half_norm, int64_t* assign, float* best, void* stream);

/* ---- DirectAU on COMPACT rows: alignment + uniformity on the unit sphere, fused B x B kernels (csrc/directau.hip) ----
 * Ub [B, D] and Ib [B, D] (row stride ld floats): row b of Ib is the positive of row b of Ub; repeated rows are kept.
 * Ureg / Ireg [B, Dreg] (stride ldreg): the rows the L2 term reads (both NULL: no L2 term).  x^ = x / max(|x|, 1e-12).
 *   align   = (1 / B) sum_b |u^_b - i^_b|^2                                   (difference form)
 *   S(X)    = sum_{i < j} expf(2 t (x^_i . x^_j - 1))                         (exact-fp32 MFMA 16x16x4 scores; = exp(-t |x^_i - x^_j|^2))
 *   unif(X) = logf(S(X)) + log(2 / (B (B - 1)))                               (the constant in double on the host)
 * fwd writes loss_out[0] = align + gamma (unif(U) + unif(I)) / 2, loss_out[1] = 0.5 sum |row|^2 / B over the 2 B L2 rows
 * (unweighted), parts[3] = [align, unif(U), unif(I)] and the state the backward reads: inv [2 B] (the inverse norms of the
 * rows of Ub, then of Ib) and ls [2] = logf(S) of the two sides.  `partials`: scratch of 2 ceil(B / 4) + 2 ceil(B / 64)
 * floats; every reduction runs in a fixed order (no atomics).  D must be a multiple of 4 in 8 .. 256 and 2 <= B <= 65536
 * (TAGREC_E_UNSUPPORTED otherwise); 0 < t <= 20 -- a term is then >= e^-80, a normal float, which is what lets the sum run
 * without a running maximum -- and gamma finite and >= 0 (TAGREC_E_INVALID otherwise). */
int tagrec_directau_fwd_f32(const float* Ub, const float* Ib, int64_t ld, int D,
                            const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                            int64_t B, float t, float gamma,
                            float* inv, float* ls, float* partials, float* parts, float* loss_out, void* stream);
/* bwd STORES (no atomics, no read of the old contents; the summation order is a function of (B, D) only) every row of the
 * gradients with respect to the RAW rows:
 *   G_i        = sum_{j != i} C_ij x^_j (ascending j) +- g0 (2 / B) (u^_b - i^_b),  C_ij = g0 gamma t expf(2 t (s_ij - 1) - ls)
 *   dX[i]      = inv_i (G_i - x^_i (x^_i . G_i))
 *   dXreg[row] = g1 / B * Xreg[row]               for the 2 B L2 rows (dUreg = dIreg = NULL: not written)
 * g = device pointer to two floats (upstream gradients of the two loss parts) or NULL for (1, 1).  dUreg = dUb and
 * dIreg = dIb (one buffer for both parts) is allowed when Ureg = Ub, Ireg = Ib with the same stride and width. */
int tagrec_directau_bwd_f32(const float* Ub, const float* Ib, int64_t ld, int D,
                            const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                            int64_t B, float t, float gamma, const float* inv, const float* ls, const float* g,
                            float* dUb, float* dIb, float* dUreg, float* dIreg, void* stream);

/* ---- N4: propagation with dynamic per-factor edge weights (DGCF model/dgcf.py:70-110, DisenGCN model/disengcn.py:23-46) --
 * The graph handle supplies the STRUCTURE (rowptr / colidx; its values are not read).  K factors own the column
 * slices [k D/K, (k+1) D/K) of an embedding row (torch.split / torch.cat along dim 1 in the reference).  Per-entry
 * data is factor-interleaved [nnz, K] in CSR entry order; per-node data [N, K].  D in {32,64,128,256}, K in {1,2,4,8},
 * D/K a multiple of 4.
 *   route_softmax      : w[j, :] = softmax(logits[j, :])                      (torch.softmax(A_values, dim=0))
 *   route_rowsum_rsqrt : d[r, k] = 1 / sqrt(sum_j w[j, k] over row r), inf -> 0  (dgcf.py:95-99)
 *   route_permute      : wt[j, :] = w[perm[j], :]                              (weights in the transposed matrix's order)
 *   route_spmm         : y[r, slice k] = post[r,k] * sum_j w[j,k] X[col_j, slice k] + self[r] + b_scale * B[r];
 *                        Y = y, Yn = y / max(||y slice||, 1e-12), inv[r,k] = 1 / max(||y slice||, 1e-12)
 *                        (post / self / B / Y / Yn / inv may each be NULL)
 *   route_score        : logits[j, k] (+)= < H[row_j, slice k], T[col_j, slice k] >
 *   slice_scale        : Y[r, slice k] = scale[r, k] * X[r, slice k]
 *   slice_norm_fwd     : Y = X / max(||X slice||, 1e-12) per slice (then tanh if apply_tanh); inv (may be NULL) as above
 *   slice_norm_bwd     : gradient of slice_norm_fwd (without tanh) given X_raw, inv and dZ
 *   row_softmax_fwd    : a[j] = softmax of logits over the stored entries of j's row (torch.sparse.softmax(adj, dim=1),
 *                        model/kgat.py:96);  row_softmax_bwd : dlogits = a * (da - sum_row(a * da))
 * D in {16,32,64,128,256} for the routed kernels. */
int tagrec_route_softmax_f32(const float* logits, float* w, int64_t nnz, int K, void* stream);
int tagrec_route_rowsum_rsqrt_f32(const tagrec_graph* g, const float* w, int K, float* d, void* stream);
int tagrec_route_permute_f32(const float* w, const int32_t* perm, float* wt, int64_t nnz, int K, void* stream);
int tagrec_route_spmm_f32(const tagrec_graph* g, const float* W, int K, const float* X, const float* post,
                          const float* self, const float* B, float b_scale, float* Y, float* Yn, float* inv,
                          int D, void* stream);
int tagrec_route_score_f32(const tagrec_graph* g, const float* H, const float* T, float* logits, int K,
                           int accumulate, int D, void* stream);
/* The same two with the restrictions of the plain products: row_mask (may be NULL) = output rows / entries' rows to
 * compute, the others are left untouched; in_flags / in_count (may be NULL) = rows of X that hold a non-zero. */
int tagrec_route_spmm_ex_f32(const tagrec_graph* g, const float* W, int K, const float* X, const float* post,
                             const float* self, const float* B, float b_scale, float* Y, float* Yn, float* inv,
                             const uint8_t* row_mask, const uint8_t* in_flags, const unsigned* in_count, int D,
                             void* stream);
int tagrec_route_score_rows_f32(const tagrec_graph* g, const float* H, const float* T, float* logits, int K,
                                int accumulate, const uint8_t* row_mask, int D, void* stream);
int tagrec_slice_scale_f32(const float* X, const float* scale, float* Y, int64_t n_rows, int D, int K, void* stream);
int tagrec_slice_norm_fwd_f32(const float* X, float* Y, float* inv, int64_t n_rows, int D, int K, int apply_tanh,
                              void* stream);
int tagrec_slice_norm_bwd_f32(const float* X_raw, const float* inv, const float* dZ, float* dX, int64_t n_rows, int D,
                              int K, void* stream);
int tagrec_row_softmax_fwd_f32(const tagrec_graph* g, const float* logits, float* a, void* stream);
int tagrec_row_softmax_bwd_f32(const tagrec_graph* g, const float* a, const float* da, float* dlogits, void* stream);

/* ---- DisenHAN relation attention (model/disenhan.py:28-97) ---------------------------------------------------------
 * A relation is a merged CSR (int64 rowptr[n_rows+1], int32 col[nnz], fp32 mult[nnz]: the number of times the (row, col)
 * pair occurs in the reference's uncoalesced COO), with row type a and column type b.  Per-node per-factor data
 * [n, K]; embeddings [n, D] with factor k in columns [k D/K, (k+1) D/K).  No float atomics: bit-reproducible.
 *   dh_edge_softmax_fwd : alpha[j] = softmax over row i's entries of  mult_j * sum_k r[i,k] relu(sL[i,k] + sR[col_j,k])
 *   dh_edge_softmax_bwd : given dalpha: g[j] = mult_j * alpha_j (dalpha_j - sum_row alpha dalpha) (scratch [nnz]),
 *                         dr / dsL [n_rows, K] (row sums), dsR [n_cols, K] (column sums over the transposed structure
 *                         rowptr_t / col_t = row ids / perm = index of the entry in the row-major order)
 *   dh_rel_epi_fwd      : Yl = leaky_0.2(Y);  Z[i, slice k] = Yl[i, slice k] W  (W [dk, dk]);
 *                         r[i, :] = softmax_k < tanh(Z[i, slice k]), q >  (q [dk])
 *   dh_rel_epi_bwd      : given dZ / dr (either may be NULL = 0): ds_k = r_k (dr_k - sum r dr),
 *                         dZt = dZ + ds_k q (1 - tanh(Z)^2), dY = (dZt_k W^T) * leaky'(Yl), dsT = ds_k tanh(Z)
 *                         (dW = Yl^T dZt and dq = column sums of dsT, both viewed [n K, dk], are left to the caller)
 *   dh_combine_fwd      : x = ego + r1 (.) Z1 + r2 (.) Z2 per slice;  y = x / max(||x slice||, 1e-12);  inv as slice_norm
 *   dh_combine_bwd      : dx = slice-norm backward of dy;  dZ_e = r_e (.) dx;  dr_e[i,k] = < Z_e[i, slice k], dx[i, slice k] >
 * K in {1,2,4,8}; the row passes need D in {16,32,64,128,256}. */
int tagrec_dh_edge_softmax_fwd_f32(const int64_t* rowptr, const int32_t* col, const float* mult, int64_t n_rows,
                                   const float* sL, const float* sR, const float* r, int K, float* alpha, void* stream);
int tagrec_dh_edge_softmax_bwd_f32(const int64_t* rowptr, const int32_t* col, const float* mult, int64_t n_rows,
                                   const int64_t* rowptr_t, const int32_t* col_t, const int32_t* perm, int64_t n_cols,
                                   const float* sL, const float* sR, const float* r, int K, const float* alpha,
                                   const float* dalpha, float* g, float* dr, float* dsL, float* dsR, void* stream);
int tagrec_dh_rel_epi_fwd_f32(const float* Y, const float* W, const float* q, int64_t n, int D, int K, float* Yl, float* Z,
                              float* r, void* stream);
int tagrec_dh_rel_epi_bwd_f32(const float* Yl, const float* Z, const float* r, const float* dZ, const float* dr,
                              const float* W, const float* q, int64_t n, int D, int K, float* dY, float* dZt, float* dsT,
                              void* stream);
int tagrec_dh_combine_fwd_f32(const float* ego, const float* Z1, const float* r1, const float* Z2, const float* r2,
                              int64_t n, int D, int K, float* x, float* y, float* inv, void* stream);
int tagrec_dh_combine_bwd_f32(const float* x, const float* inv, const float* dy, const float* Z1, const float* r1,
                              const float* Z2, const float* r2, int64_t n, int D, int K, float* dx, float* dZ1, float* dZ2,
                              float* dr1, float* dr2, void* stream);

/* ---- evaluation: sigmoid(U_b I^T) -> mask train positives -> top-K, fused (lightgcn.py:84-89, basic_test.py:36-50) --
 * U / I: propagated user / item tables, row-major [*, D].  users: int64 [n_users] ids to score.  train_ptr int64
 * [n_user_total + 1] / train_items int32: each user's train items, sorted (the rows basic_test.py:47 overwrites with
 * -1024; here they are simply never admitted).  top_idx int64 [n_users, K]: item ids by descending sigmoid score,
 * ties to the lower id, -1 if fewer than K items remain; top_val [n_users, K] (may be NULL): the scores.
 * D in {16,32,64,128,192,256,384,512}, K <= 64. */
int tagrec_eval_topk_f32(const float* U, const float* I, int64_t n_item, int D, const int64_t* users,
                         int64_t n_users, const int64_t* train_ptr, const int32_t* train_items, int K,
                         int64_t* top_idx, float* top_val, void* stream);

/* ---- evaluation with AUC: the same pass, plus each user's AUC over its un-masked items (basic_test.py:53,73) --------
 * test_ptr int64 [n_user_total + 1] / test_items int32: each user's test items, sorted (duplicates allowed).  valid =
 * not a train id; positives = unique test ids that are valid; negatives = the other valid items.  Per evaluated user:
 * n_pos / n_neg int64 [n_users], auc_num2 int64 [n_users] = sum over (positive p, negative x) of 2 [s_p > s_x] +
 * [s_p == s_x], with s = the fp32 sigmoid score the top-K ranks by; AUC = auc_num2 / (2 n_pos n_neg).  top_idx /
 * top_val exactly as tagrec_eval_topk_f32.  Same widths, K <= 64. */
int tagrec_eval_topk_auc_f32(const float* U, const float* I, int64_t n_item, int D, const int64_t* users,
                             int64_t n_users, const int64_t* train_ptr, const int32_t* train_items,
                             const int64_t* test_ptr, const int32_t* test_items, int K, int64_t* top_idx,
                             float* top_val, int64_t* auc_num2, int64_t* n_pos, int64_t* n_neg, void* stream);

/* ---- negative sampler (train_data/utils.py:19-28, 31-40) -------------------------------------------------------
 * For each of n_rows positive rows with left id left[e] (a user, or a (user, tag) pair id): one uniform draw in
 * [0, n_right), re-drawn while it is in the left id's sorted positive list cols[rowptr[l] .. rowptr[l+1]).
 * Draw t of row e is a pure function of (seed, e, t): reproducible whatever the launch geometry. */
int tagrec_sample_negative_i64(const int64_t* left, int64_t n_rows, const int64_t* rowptr, const int32_t* cols,
                               int64_t n_left, int64_t n_right, uint64_t seed, int64_t* neg, void* stream);

/* The same sampler with a choice of proposal and n_cand candidates per row (not in the reference, which draws uniformly).
 * With mix64 = the splitmix64 finaliser and base_0 = mix64(seed ^ mix64(e)), candidate c of row e runs the rejection loop
 * above (at most 4096 tries, the last one kept) on the stream base_c = base_0 for c = 0, mix64(base_0 + (c << 32)) else:
 *   uniform (alias_prob == NULL): try t draws umul64hi(mix64(base_c + t), n_right) -- candidate 0 is the draw of
 *     tagrec_sample_negative_i64;
 *   alias table (alias_prob float32 [n_right], alias_idx int32 [n_right], Vose): j = umul64hi(mix64(base_c + 2t), n_right),
 *     u = float(mix64(base_c + 2t + 1) >> 40) * 2^-24; the draw is j if u < alias_prob[j], else alias_idx[j].
 * Candidates are drawn with replacement.  n_cand == 1: neg[e] = candidate 0, no table is read (U, I, ld, D are ignored;
 * score_out must be NULL).  n_cand in 2 .. 16: score_c = sum_k U[left[e] * ld_u + k] * I[cand_c * ld_i + k] in fp32 and
 * neg[e] = the first arg-max in c order (a later candidate wins only with a strictly greater score: ties keep the
 * lowest c, a NaN score never replaces an earlier candidate).  D % 4 == 0, 8 <= D <= 1024, ld % 4 == 0, ld >= D, 16-byte
 * aligned tables; U must hold n_left rows and I n_right rows.  cand_out int64 [n_rows, n_cand] and score_out float32
 * [n_rows, n_cand] are optional.  A pure function of its arguments: no atomics, two launches give the same bits. */
int tagrec_sample_negative_ex_i64(const int64_t* left, int64_t n_rows, const int64_t* rowptr, const int32_t* cols,
                                  int64_t n_left, int64_t n_right, uint64_t seed, int n_cand, const float* alias_prob,
                                  const int32_t* alias_idx, const float* U, int64_t ld_u, const float* I, int64_t ld_i,
                                  int D, int64_t* neg, int64_t* cand_out, float* score_out, void* stream);

/* ---- TransTag phase of TGCN (tgcn.py:251-261, loss.py:35-41, 27-32) on the EGO tables -------------------------
 * quad: int64 [B,4] = (user, tag, pos_item, neg_item).  fwd: loss_out[0] = mean relu(margin + ||u+t-p|| - ||u+t-n||),
 * loss_out[1] = l2reg_loss(u, t, p, n) (unweighted); dist [B,2] keeps the two distances; partials: 2*ceil(B/4) floats.
 * bwd: float-atomic scatter-add of g[0]*d loss + g[1]*d reg into caller-zeroed dEu / dEi / dEt (g = two upstream
 * gradients on the device, NULL = (1,1)). */
int tagrec_transtag_fwd_f32(const float* Eu, const float* Ei, const float* Et, int64_t ld, int D,
                            const int64_t* quad, int64_t B, float margin, float* dist, float* partials,
                            float* loss_out, void* stream);
int tagrec_transtag_bwd_f32(const float* Eu, const float* Ei, const float* Et, int64_t ld, int D,
                            const int64_t* quad, int64_t B, float margin, const float* dist, const float* g,
                            float* dEu, float* dEi, float* dEt, void* stream);

/* ---- Adam (torch.optim.Adam defaults as used at com.py:14,25,69), one fused pass -----------------
 *   m += (1-b1)(g-m);  v = b2 v + (1-b2) g^2;  p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps) */
int tagrec_adam_f32(float* p, const float* g, float* m, float* v, int64_t n,
                    float lr, float b1, float b2, float eps, int64_t step, void* stream);
/* The same update for n_tensors (small) parameter tensors in one launch per 64 of them: host arrays of device pointers and
 * element counts (< 2^31 each), one step count for all. */
int tagrec_adam_multi_f32(int n_tensors, float* const* p, const float* const* g, float* const* m, float* const* v,
                          const int64_t* n, float lr, float b1, float b2, float eps, int64_t step, void* stream);
/* The same update with the step counter (int64[1]) and the two step-dependent factors (float[2], scratch) in DEVICE
 * memory: the call advances *step_dev itself, so a HIP graph that captured it replays as successive steps. */
int tagrec_adam_graph_f32(float* p, const float* g, float* m, float* v, int64_t n,
                          float lr, float b1, float b2, float eps, int64_t* step_dev, float* coef_dev, void* stream);

/* Row-sparse Adam that computes what tagrec_adam_f32 computes, bit for bit (train.RowAdam).  Under a zero gradient the update
 * of a row is a function of the row's own p / m / v and of two per-step scalars, so a row the step does not name is left
 * alone and the skipped steps are replayed, in order, when it is next read.  State per table p / m / v [n_rows, D] (row
 * stride ld): last (int32 [n_rows]) = the last optimizer step applied to each row, and a ring of cap float pairs in device
 * memory, (lr / (1 - b1^t), sqrt(1 - b2^t)) of step t at entry t mod cap.
 *   adam_coef : HOST ONLY, no stream.  Fills the host array out [2 n] with the pairs of steps t0 .. t0 + n - 1 (t0 >= 1) --
 *               the double-precision expressions of tagrec_adam_f32, each rounded to float once.  (tagrec_adam_f32 takes lr /
 *               b1 / b2 as floats and widens them: pass the widened values here to get its bits.)
 *   catchup   : every distinct row r of a built row-list plan (ws, n_listed, width as for tagrec_row_scatter_ordered_f32)
 *               takes the zero-gradient update of steps last[r] + 1 .. t_done, in order; p, m, v and last[r] = t_done are
 *               stored.  A row with last[r] == t_done is not read beyond `last`.
 *   apply     : the gradient of every distinct row is its segment's sum of src [n_listed, D] (row stride lds) in EXACTLY
 *               tagrec_row_scatter_ordered_f32's order (the same device code); one update of step t with the ring's pair of t;
 *               last[r] = t.  Requires last[r] == t - 1 on entry (run catchup to t - 1 first); not checked on the device.
 *   flush     : every row of the table with last[r] < t_done is replayed to t_done.  A row that is current costs its 4 bytes
 *               of `last`; a 16-byte column group whose m and v are all +0 bits is left as it is (exact: a zero gradient
 *               does not change it) and its p is not read.
 * t_floor (catchup, flush): a lower bound of last[] over the rows concerned, kept by the caller (the step of its last flush);
 * the ring entries of steps t_floor + 1 .. t_done must be filled, t_done - t_floor <= min(cap, 4096) (a block stages that
 * window in LDS).  A row whose `last` is below t_floor is replayed from t_floor.  D in {8, .., 256} with 16-byte aligned rows
 * takes D / 4 lanes x 16 bytes per row, anything else one lane per column.  No float atomics, no host read. */
int tagrec_adam_coef(double lr, double b1, double b2, int64_t t0, int64_t n, float* out);
int tagrec_rowadam_catchup_f32(const void* ws, int64_t ws_bytes, int64_t n_listed, int width, float* p, float* m, float* v,
                               int64_t ld, int64_t n_rows, int D, int32_t* last, const float* ring, int64_t ring_cap,
                               int64_t t_floor, int64_t t_done, float b1, float b2, float eps, void* stream);
int tagrec_rowadam_apply_f32(const void* ws, int64_t ws_bytes, int64_t n_listed, int width, const float* src, int64_t lds,
                             float* p, float* m, float* v, int64_t ld, int64_t n_rows, int D, int32_t* last, const float* ring,
                             int64_t ring_cap, int64_t t, float b1, float b2, float eps, void* stream);
int tagrec_rowadam_flush_f32(float* p, float* m, float* v, int64_t ld, int64_t n_rows, int D, int32_t* last, const float* ring,
                             int64_t ring_cap, int64_t t_floor, int64_t t_done, float b1, float b2, float eps, void* stream);

/* The last backward hop with the optimizer folded in (training/basic_train.py:19-25: backward() then opt.step()):
 * row r of A G_in + b_scale B is the gradient of parameter row r; torch.optim.Adam's update (defaults; the arithmetic of
 * tagrec_adam_f32 at step `step`, counted from 1) is applied to p / m / v [n_rows, D] in the epilogue and no gradient
 * tensor is written.  in_flags / in_count / b_flags as in tagrec_spmm_axpy_sparse_f32.  G_in must not alias p. */
int tagrec_spmm_axpy_adam_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags, const unsigned* in_count,
                              const float* B, float b_scale, const uint8_t* b_flags, float* p, float* m, float* v,
                              float lr, float b1, float b2, float eps, int64_t step, int D, void* stream);
/* The same with the optimizer's step counter (int64) and its two step-dependent factors ([lr / (1 - b1^t), sqrt(1 - b2^t)])
 * in DEVICE memory: tagrec_adam_advance moves them one step forward on the stream (a one-thread kernel); the product reads
 * the factors there.  Nothing step-dependent is baked into the launch, so a captured HIP graph of the whole training step
 * (loss, backward, optimizer) replays correctly (train.GraphedStep with Adam(capturable=True).fuse_into(model)). */
int tagrec_adam_advance(int64_t* step_dev, float* coef_dev, float lr, float b1, float b2, void* stream);
int tagrec_spmm_axpy_adam_graph_f32(const tagrec_graph* g, const float* G_in, const uint8_t* in_flags,
                                    const unsigned* in_count, const float* B, float b_scale, const uint8_t* b_flags,
                                    float* p, float* m, float* v, float lr, float b1, float b2, float eps,
                                    int64_t* step_dev, float* coef_dev, int D, void* stream);

/* out = srcs[0] + ... + srcs[n_srcs - 1] (1 <= n_srcs <= 8, n floats each, summed left to right) in one pass: the
 * gradient of a table that several consumers read (what autograd's pairwise accumulation does in 3 passes per extra
 * gradient).  `srcs` is a HOST array of device pointers; `out` may alias a source. */
int tagrec_sum_n_f32(float* out, const float* const* srcs, int n_srcs, int64_t n, void* stream);

/* The layer mean of a restricted LightGCN step on its n_listed batch rows, and their ego rows, in one launch:
 *   out_b[k] = s x0[rows[k]] + sum_l s y[l][rows[k]] inv[l][rows[k]] + s z_top[k],   ego_b[k] = x0[rows[k]]  (ego_b may be NULL)
 * x0, y[l]: [n_rows, D]; inv[l]: [n_rows]; z_top, out_b, ego_b: [n_listed, D]; D a multiple of 4; 0 <= n_layers <= 8.
 * `y` and `inv` are HOST arrays of device pointers.  Same operation order and roundings as torch's index_select, `* s`,
 * addcmul_(value = s) per layer and add_(alpha = s): the same bits.  A row id outside [0, n_rows) yields NaN rows. */
int tagrec_layer_mean_rows_f32(const float* x0, const int64_t* rows, int64_t n_listed, int64_t n_rows, const float* const* y,
                               const float* const* inv, int n_layers, const float* z_top, float s, float* out_b, float* ego_b,
                               int D, void* stream);

/* ---- NGCF layer, dense half (ngcf.py:77-86), exact-fp32 MFMA ------------------------------------------
 * Given N = A @ X (tagrec_spmm_f32) and W1p = W1 + b1, W2p = W2 + b2 (row-major [Din, Dout]; the
 * reference adds the 1 x Dout bias to the weight matrix, ngcf.py:78,82):
 *   fwd : Xp = LeakyReLU_0.2((N + X) W1p) + LeakyReLU_0.2((N * X) W2p);  inv_norm = 1/max(||Xp||, 1e-12);
 *         Z  = Xp / max(||Xp||, 1e-12) written with row stride ldz (one slot of the concat output)
 *   bwd : from dXp (gradient w.r.t. Xp): dP1, dP2 (pre-activation gradients), dN = dA1 + dA2 * X,
 *         dXd = dA1 + dA2 * N with dAi = dPi Wip^T.  The caller finishes dX = A^T dN + dXd
 *         (tagrec_spmm_axpy_f32).
 *   wgrad: dW1p = (N + X)^T dP1, dW2p = (N * X)^T dP2 (deterministic two-stage reduction; workspace of
 *         tagrec_ngcf_wgrad_workspace(Din, Dout) floats).  db = column sums of dWp (the bias broadcast).
 * Din, Dout in {16, 32, 64, 128} (128 -> 128 runs the backward kernels one matrix per launch: both LDS copies of both
 * matrices would not fit).
 * The *_rows_* forms serve the restricted training step (a layer whose output is needed on some rows only):
 *   row_mask (one byte per row, may be NULL = every row): rows whose byte is 0 are neither read nor written -- their
 *     slots in the outputs keep whatever they held, so every consumer must be handed the same mask (the weight gradient
 *     takes it too and counts such rows as zero);
 *   Z may be NULL (fwd): the normalised slot is not written (the step forms it on the batch rows from Xp and inv_norm);
 *   dz_flags (bwd, one byte per row, may be NULL): rows whose byte is 0 have dZ == 0; Xp, inv_norm and dZ are not read
 *     there (the concat gradient of a BPR step lives on the <= 3 B batch rows). */
int64_t tagrec_ngcf_wgrad_workspace(int Din, int Dout);
int tagrec_ngcf_dense_fwd_f32(const float* N, const float* X, const float* W1p, const float* W2p,
                              int64_t n_rows, int Din, int Dout, float* Xp, float* inv_norm, float* Z,
                              int64_t ldz, void* stream);
int tagrec_ngcf_dense_bwd_f32(const float* dXp, const float* N, const float* X, const float* W1p,
                              const float* W2p, int64_t n_rows, int Din, int Dout, float* dN, float* dXd,
                              float* dP1, float* dP2, void* stream);
/* bwd with the normalize-backward folded in: the gradient w.r.t. Xp is G (may be NULL; what the next layer sent
 * back) + normalize-backward(Xp, inv_norm, dZ), dZ = this layer's slot of the concat gradient, row stride ldz. */
int tagrec_ngcf_dense_bwd_norm_f32(const float* G, const float* Xp, const float* inv_norm, const float* dZ, int64_t ldz,
                                   const float* N, const float* X, const float* W1p, const float* W2p,
                                   int64_t n_rows, int Din, int Dout, float* dN, float* dXd, float* dP1,
                                   float* dP2, void* stream);
int tagrec_ngcf_wgrad_f32(const float* N, const float* X, const float* dP1, const float* dP2, int64_t n_rows,
                          int Din, int Dout, float* dW1p, float* dW2p, float* workspace,
                          int64_t workspace_floats, void* stream);
int tagrec_ngcf_dense_fwd_rows_f32(const float* N, const float* X, const float* W1p, const float* W2p,
                                   int64_t n_rows, int Din, int Dout, float* Xp, float* inv_norm, float* Z,
                                   int64_t ldz, const uint8_t* row_mask, void* stream);
int tagrec_ngcf_dense_bwd_rows_f32(const float* G, const float* Xp, const float* inv_norm, const float* dZ, int64_t ldz,
                                   const uint8_t* dz_flags, const float* N, const float* X, const float* W1p,
                                   const float* W2p, int64_t n_rows, int Din, int Dout, float* dN, float* dXd,
                                   float* dP1, float* dP2, const uint8_t* row_mask, void* stream);
int tagrec_ngcf_wgrad_rows_f32(const float* N, const float* X, const float* dP1, const float* dP2, int64_t n_rows,
                               int Din, int Dout, float* dW1p, float* dW2p, float* workspace,
                               int64_t workspace_floats, const uint8_t* row_mask, void* stream);

/* ---- TGCN neighbour-level attention (tgcn.py:20-37) over fixed-width neighbour tables (tgcn.py:194-202) ---
 * The caller forms the dense pieces with plain GEMMs:  P = ev W1[:D] + b  [n, A];  Q = ej W2  [m, A];
 * WT = cat(0, ew) W1[D:]  [n_wt, A] (row 0 = pad).  idx / widx: int32 [n, k], neighbour id + 1 and weight
 * index, 0 = pad (a zero row that still takes part in the softmax, as in the reference).
 *   fwd: attn[n,k] = softmax_k( relu(P[v] + WT[widx] + Q[idx-1]) . v );  out[v] = sum_k attn * Ej[idx-1]
 *   bwd: from dOut [n, D]: dP [n, A] (written), dWT [n_wt, A] and dv [A] (written; fixed-order fold of
 *        per-block partials, which are themselves summed by LDS float atomics in no fixed order: dWT and
 *        dv agree between runs to rounding, not bit for bit -- dP, dh and comp do bit for bit; workspace
 *        of tagrec_tgcn_attn_workspace(n_wt, A) floats), and EITHER
 *        dh = NULL: dQ [m, A] and dEj [m, D] by float-atomic scatter-add into caller-zeroed buffers, OR
 *        dh [n, k, A] (written): the per-(node, neighbour) pre-activation gradients; the caller then forms
 *        dQ = S dh and dEj = G dOut as pull products over the inverted neighbour table with tagrec_spmm_f32
 *        (S: unit values, columns = flat (node, slot) positions; G: values = attn, columns = source nodes).
 * D in {16,32,64,128,256}, A in {4,8,16,32,64}, k <= 64. */
int64_t tagrec_tgcn_attn_workspace(int n_wt, int A);
int tagrec_tgcn_attn_fwd_f32(const float* P, const float* Q, const float* WT, const float* v, const float* Ej,
                             const int32_t* idx, const int32_t* widx, int64_t n, int k, int D, int A,
                             float* attn, float* out, void* stream);
int tagrec_tgcn_attn_bwd_f32(const float* P, const float* Q, const float* WT, const float* v, const float* Ej,
                             const int32_t* idx, const int32_t* widx, const float* attn, const float* dOut,
                             int64_t n, int k, int D, int A, int n_wt, float* dP, float* dQ, float* dEj,
                             float* dh, float* dWT, float* dv, float* workspace, int64_t workspace_floats, void* stream);

/*   bwd, pull form without the dh round trip (three launches per relation over the relation's table inverted by
 *   destination: graph handle `inv` with rows = destinations, colidx = source rows, vals = attention weights):
 *     tagrec_attn_pull_da_f32 : dEj[j] = sum_p attn[p] dOut[p / k] (+ B[j]) and, on the way, da[p] = dOut[p / k] . Ej[j]
 *                               for every listed pair (the wave that walks row j holds both operands);
 *     tagrec_tgcn_attn_bwd_ds_f32 : from da: dP, dWT, dv as in attn_bwd, and comp [n k, 2] = (ds, relu bits of the A
 *                               pre-activations as an int32) per pair -- 8 bytes instead of dh's 4 A; no D-wide row is read;
 *                               w_major: a hint, the most frequent value of widx (its dWT row is summed in registers instead
 *                               of LDS atomics; any value, or -1, gives the same result);
 *     tagrec_attn_pull_dq_f32 : dQ[j] = v (.) sum_p ds[p] bits[p] (+ B[j]), over a handle whose colidx = PAIR ids.
 *   tagrec_attn_keys_i32: key[i] = idx[i] - 1, pads -> n_dst: the sort keys of the inversion.  A in {16, 32} (pull_dq). */
int tagrec_attn_pull_da_f32(const tagrec_graph* inv, const int32_t* pair, const float* dOut, const float* Ej,
                            const float* B, float* dEj, float* da, int D, void* stream);
/*   tagrec_attn_invert_fill: from the sort's permutation (int64 pair ids in destination order): pair (int32), src = pair / k,
 *   val = attn[pair] -- the colidx / vals of the inverted table that attn_pull_da walks (`inv`: rows = destinations,
 *   colidx = src, vals = val; `pair` rides along for the da store). */
int tagrec_attn_invert_fill(const int64_t* order, const float* attn, int k, int64_t n, int32_t* pair, int32_t* src, float* val,
                            void* stream);
int tagrec_tgcn_attn_bwd_ds_f32(const float* P, const float* Q, const float* WT, const float* v, const int32_t* idx,
                                const int32_t* widx, const float* attn, const float* da, int64_t n, int k, int A,
                                int n_wt, int w_major, float* dP, float* comp, float* dWT, float* dv, float* workspace,
                                int64_t workspace_floats, void* stream);
int tagrec_attn_pull_dq_f32(const tagrec_graph* inv, const float* comp, const float* v, int A, const float* B, float* dQ,
                            void* stream);
int tagrec_attn_keys_i32(const int32_t* idx, int64_t n, int32_t n_dst, int32_t* key, void* stream);
/*   tagrec_inv_filter_i32 : a step's inverted table WITHOUT a sort.  The neighbour tables are static (tgcn.py:194-202), so each
 *   relation's pair list sorted by destination is built once: perm_sorted (pair id v k + n of a non-pad slot) and dest_sorted
 *   (its destination id), n_entries of them.  A step computes a row subset: pos_src[v + 1] = 1 + position of source row v in
 *   it (0 = not computed; int32 [n_src + 1]); the entries of those rows are compacted IN ORDER into skey (destination,
 *   renumbered through pos_dst[d + 1] - 1 when pos_dst != NULL), pair (= position k + slot), src (= position) and val
 *   (= attn[pair]); skey[total .. capacity) is set to n_dst ("no entry").  capacity >= the number of listed entries (rows k
 *   is always enough).  workspace: tagrec_inv_filter_workspace(n_entries) int32, 8-byte aligned; workspace[1] = the total on
 *   return.  One pass over the static list (ticketed blocks, chained scan of their counts); k <= 64. */
int64_t tagrec_inv_filter_workspace(int64_t n_entries);
int tagrec_inv_filter_i32(const int32_t* perm_sorted, const int32_t* dest_sorted, int64_t n_entries, int k,
                          const int32_t* pos_src, const int32_t* pos_dst, const float* attn, int32_t n_dst,
                          int64_t capacity, int32_t* skey, int32_t* pair, int32_t* src, float* val,
                          int32_t* workspace, int64_t workspace_ints, void* stream);
/*   tagrec_nbr_gather_i32 : the neighbour tables of a ROW SUBSET in compact numbering (tgcn.py:194-202 restricted to the rows a
 *   mini-batch needs): out_idx[i, :] = pos[idx[rows[i], :]] (pos NULL: ids unchanged; pos[0] = 0 keeps the pad),
 *   out_widx[i, :] = widx[rows[i], :]. */
int tagrec_nbr_gather_i32(const int32_t* idx, const int32_t* widx, const int64_t* rows, const int32_t* pos, int64_t n_rows,
                          int k, int32_t* out_idx, int32_t* out_widx, void* stream);
/*     tagrec_attn_seg_dq_f32 : the same dQ from the pair list SORTED by destination (dest_sorted = the sorted keys, entries
 *                               with dest >= n_dst are the pads at the tail), as a balanced segmented sum: 256 entries per
 *                               wavefront, a finished segment ADDED to dQ by float atomics (the caller zeroes dQ; two relations
 *                               of one neighbour type add into the same buffer).  A in {4, 8, 16, 32}. */
int tagrec_attn_seg_dq_f32(const int32_t* dest_sorted, const int32_t* pair_sorted, int64_t n_entries, int32_t n_dst,
                           const float* comp, const float* v, int A, float* dQ, void* stream);

/* ---- the row plan of a restricted TGCN step (tgcn.py:236-249 reads the top layer at the batch rows only; the tables of
 *      tgcn.py:194-202 say which rows of the layer below those depend on) ---------------------------------------------
 * Node types 0, 1, 2 (user, item, tag) of sizes3[] nodes share one flag buffer: segment t starts at byte
 * tagrec_plan_segment_result(sizes3, t) (t = 3: the total = tagrec_plan_flags_workspace(sizes3) bytes) and holds n_t + 1
 * slots, slot 0 = the pad id of the neighbour tables, slot v + 1 = row v.
 *   plan_mark    : clears flags and counts, sets every row of a type with all3[t] != 0, then runs the descriptors
 *                  i < n_desc (at most 12): idx[i] == NULL -> flag rows[i][j * stride[i]] (j < n_rows[i]) of type
 *                  dst_type[i]; else flag idx[i][row, 0..k[i]) of type dst_type[i] for row = rows[i][j * stride[i]]
 *                  (rows[i] == NULL: row = j) < n_src[i].  Ids out of range are skipped and counted in counts[3].
 *   plan_compact : per type, the flagged rows in ascending order -> rows_out[row_base_t ..) (row_base = 0, n_0, n_0 + n_1;
 *                  capacity sum of sizes3), their number -> counts[t] (device int64 [4]), and the position map pos_out (int32,
 *                  the flag buffer's layout): pos_out[slot] = 1 + position of the row in its list, 0 if not flagged.
 *                  workspace: tagrec_plan_scan_workspace(sizes3) int32.
 *   plan_lookup  : out[i * out_stride] = pos[rows[i * stride] + 1] - 1 (a row id -> its position in a compact table). */
int64_t tagrec_plan_flags_workspace(const int64_t* sizes3);
int64_t tagrec_plan_segment_result(const int64_t* sizes3, int type);
int64_t tagrec_plan_scan_workspace(const int64_t* sizes3);
int tagrec_plan_mark_u8(int n_desc, const int32_t* const* idx, const int64_t* const* rows, const int64_t* stride,
                        const int64_t* n_rows, const int64_t* n_src, const int* k, const int* dst_type, const int* all3,
                        const int64_t* sizes3, uint8_t* flags, int64_t* counts, void* stream);
int tagrec_plan_compact_i64(const uint8_t* flags, const int64_t* sizes3, int64_t* rows_out, int32_t* pos_out, int64_t* counts,
                            int32_t* workspace, int64_t workspace_ints, void* stream);
int tagrec_plan_lookup_i64(const int32_t* pos, const int64_t* rows, int64_t stride, int64_t n, int64_t* out, int64_t out_stride,
                           void* stream);

/* ---- TGCN type-level attention + bit/vector convolutions + fusion layer, fused (tgcn.py:78-106) ------------
 * One node type per call.  T0/T1/T2 [n, D]: the (user-side, item-side, tag-side) vectors of each node, in
 * that order.  U [D, A], q [A], p [A]; wb [C, 3] (Conv2d(1,C,(3,1)) weight); w1 [V, D], w2 [V, 2, D],
 * w3 [V, 3, D] (Conv2d(1,V,(j,D)) weights); Wf [C*D + 6V, Dout], bf [Dout].
 *   fwd: out [n, Dout] = relu(y Wf + bf) with y the convolution features of e_j = softmax_j(relu(t_j U + q).p) t_j;
 *        bw_out [n, 3] = the softmax weights (kept for the backward pass).
 * Built for A = 32, C = 32, V = 8 (the reference's defaults) and D, Dout in {16, 32, 64, 128}. */
int tagrec_tgcn_fuse_fwd_f32(const float* T0, const float* T1, const float* T2, int64_t n, int D, int Dout,
                             int A, int C, int V, const float* U, const float* q, const float* p,
                             const float* wb, const float* w1, const float* w2, const float* w3,
                             const float* Wf, const float* bf, float* bw_out, float* out, void* stream);

/*   fwd with MESSAGE DROPOUT of the output (F.dropout on eu / ei / et, tgcn.py:217-219) in the epilogue: the n rows are up to
 *        three segments [0, lo1), [lo1, lo2), [lo2, n) -- the node types of a layer, merged into one launch -- each with its own
 *        seed (host array seeds3) and, when the launch computes a row subset, its node ids (rowsK, device int64; NULL = rows
 *        0 .. in order).  out = mask(seed, node id, column) relu(..) / (1 - p) with the counter-based mask of
 *        tagrec_dropout_rows_f32.  The backward entry points are used unchanged with out' = this output and dOut' =
 *        dOut / (1 - p): [out' > 0] = mask [out > 0]. */
int tagrec_tgcn_fuse_fwd_drop_f32(const float* T0, const float* T1, const float* T2, int64_t n, int D, int Dout,
                                  int A, int C, int V, const float* U, const float* q, const float* p,
                                  const float* wb, const float* w1, const float* w2, const float* w3,
                                  const float* Wf, const float* bf, float drop_p, const uint64_t* seeds3,
                                  const int64_t* rows0, const int64_t* rows1, const int64_t* rows2, int64_t lo1,
                                  int64_t lo2, float* bw_out, float* out, void* stream);

/*   bwd (data part): from dOut [n, Dout] and the forward's `out` (ReLU mask): dT0/dT1/dT2 [n, D]; yvec [n, 6V]
 *        (post-ReLU vector features) and dfeat [n, 6V] (their pre-activation gradients), dS [n, 3A] (type-attention
 *        pre-activation gradients) for the weight gradients; small [3C + 2A] = dwb | dq | dp
 *        (deterministic fold of per-block partials; workspace of tagrec_tgcn_fuse_bwd_workspace(Dout) floats). */
int64_t tagrec_tgcn_fuse_bwd_workspace(int Dout);
int tagrec_tgcn_fuse_bwd_f32(const float* T0, const float* T1, const float* T2, int64_t n, int D, int Dout,
                             int A, int C, int V, const float* U, const float* q, const float* p,
                             const float* wb, const float* w1, const float* w2, const float* w3,
                             const float* Wf, const float* out, const float* dOut, float* dT0, float* dT1,
                             float* dT2, float* yvec, float* dfeat, float* dS, float* small,
                             float* workspace, int64_t workspace_floats, void* stream);

/*   wf: every weight gradient that is a product over the NODE axis, in one launch.  result (of
 *        tagrec_tgcn_fuse_wf_result(D, Dout) floats) = [ dWf | G | dU ]:
 *          dWf [C*D + 6V, Dout] = y^T (dOut * [out > 0]), y re-formed on the fly from T0..T2, bw [n, 3], wb, yvec;
 *          G   [6V, 3, D]       = dfeat^T e_j  (the caller folds G into the Conv2d(1,V,(j,D)) weight gradients);
 *          dU  [D, A]           = sum_j t_j^T dS_j.
 *        workspace of tagrec_tgcn_fuse_wf_workspace(D, Dout) floats; deterministic fold of per-node-group partials. */
int64_t tagrec_tgcn_fuse_wf_result(int D, int Dout);
int64_t tagrec_tgcn_fuse_wf_workspace(int D, int Dout);
int tagrec_tgcn_fuse_wf_f32(const float* T0, const float* T1, const float* T2, const float* bw, const float* yvec,
                            const float* wb, const float* out, const float* dOut, const float* dfeat, const float* dS,
                            int64_t n, int D, int Dout, int C, int V, float* result, float* workspace,
                            int64_t workspace_floats, void* stream);

/* ---- tall-skinny dense products of the TGCN step (tgcn.py:20-37 after the split of the attention's matmuls) ----
 * exact-fp32 MFMA, HBM-bound: a node table times a small matrix, and the reverse products.  K, NO in {16, 32, 64, 128}.
 *   tall_mm : Y[n, NO] (+)= [X1 | X2][sel][n, K] W[K, NO] + bias.
 *             X2 != NULL: the tall operand is two tensors of K/2 columns each; sel (int64 [n], may be NULL) gathers its rows.
 *             W(k, c) = W1[k * w_sk + c * w_sc] (strides in floats: a transposed matrix is a stride pair); w_split = 1: W2
 *             holds the rows k >= K/2, w_split = 2: W2 holds the columns c >= NO/2 (same strides).
 *             Y2 != NULL: columns [NO/2, NO) go to Y2, both outputs with row stride NO/2 (b1 / b2: their biases, may be NULL).
 *             accumulate != 0: the product is added to what Y holds.
 *   tall_wgrad : dW[KI, NO] (+)= X^T [dY1 | dY2] and db1 / db2 (+)= column sums of dY1 / dY2 (any output may be NULL),
 *             contraction over the n rows; per-wave partials in `workspace` (tagrec_tall_wgrad_workspace(KI, NO) floats) folded
 *             in a fixed order.
 *   small_mm : C[M, N] (+)= A B with A(i, k) = A[i * sam + k * sak], B(k, j) = B[k * sbk + j * sbn] (look-up-table sized).
 *   row_add_at : dst[pos[i], :] += src[i, :] for DISTINCT positions (plain read-modify-write). */
int tagrec_tall_mm_f32(const float* X1, const float* X2, const int64_t* sel, int64_t n, int K, int NO, const float* W1,
                       const float* W2, int64_t w_sk, int64_t w_sc, int w_split, const float* b1, const float* b2,
                       float* Y1, float* Y2, int accumulate, void* stream);
/*   tall_mm_adam : the gradient G = G_in + X W (X [n, K], W(k, c) = W[k * w_sk + c * w_sc], G_in [n, NO] or NULL) of the
 *             embedding table p [n, NO] is not stored: torch.optim.Adam's update of p, exp_avg m and exp_avg_sq v (the arithmetic
 *             of tagrec_adam_f32, step = the number of this update) is applied in the product's epilogue -- the last term of
 *             a TGCN table's gradient is dQ W_2^T (tgcn.py:20-37), so the optimizer never reads a gradient tensor
 *             (training/basic_train.py:21,25). */
int tagrec_tall_mm_adam_f32(const float* X, int64_t n, int K, int NO, const float* W, int64_t w_sk, int64_t w_sc,
                            const float* G_in, float* p, float* m, float* v, float lr, float b1, float b2, float eps,
                            int64_t step, void* stream);
int64_t tagrec_tall_wgrad_workspace(int KI, int NO);
int tagrec_tall_wgrad_f32(const float* X, const float* dY1, const float* dY2, int64_t n, int KI, int NO, float* dW,
                          float* db1, float* db2, int acc_w, int acc_b, float* workspace, int64_t workspace_floats, void* stream);
int tagrec_small_mm_f32(const float* A, const float* B, float* C, int M, int N, int K, int64_t sam, int64_t sak,
                        int64_t sbk, int64_t sbn, int accumulate, void* stream);
int tagrec_row_add_at_f32(float* dst, const int64_t* pos, const float* src, int64_t n_rows, int D, void* stream);
/*   masked_colsum : result[D] = column sums of dOut (.) [out > 0] -- the bias gradient of a ReLU layer (dbf of the fusion
 *   layer, tgcn.py:104-106); per-block partials in `workspace` (tagrec_masked_colsum_workspace(D) floats), fixed-order fold. */
int64_t tagrec_masked_colsum_workspace(int D);
int tagrec_masked_colsum_f32(const float* dOut, const float* out, int64_t n_rows, int D, float* result, float* workspace,
                             int64_t workspace_floats, void* stream);

/* ---- distance-correlation loss between factor slices (model/help/loss.py:53-80; csrc/cor.hip) ----
 * X [n, D] (row stride ld floats, rows 16-byte aligned) is K column slices of width D / K; D in {8 .. 256}, K >= 2,
 * K | D, D / K >= 2, n >= 2.  The distances are recomputed from LDS tiles in every pass: nothing n x n is stored.
 *   fwd: loss[1] and, for the backward pass, rowsum [n, K] (sum_j d^f_ij), gsum [K] (their column sums) and
 *        coef [K, 3] (d loss / d d^f_ij = coef[f][0] A^{f-1} + coef[f][1] A^f + coef[f][2] A^{f+1}); part [n, 2K] and
 *        sums [2K] are scratch (per-row and total covariance sums).  All sums have a fixed order.
 *   bwd: dX [n, D] (row stride lddx) = g[0] * d loss / dX; every row is written once, no atomics. */
int tagrec_cor_fwd_f32(const float* X, int64_t ld, int64_t n, int D, int K, double* rowsum, double* gsum, double* part,
                       double* sums, float* loss, float* coef, void* stream);
int tagrec_cor_bwd_f32(const float* X, int64_t ld, int64_t n, int D, int K, const double* rowsum, const double* gsum,
                       const float* coef, const float* g, float* dX, int64_t lddx, void* stream);

/* ---- bandwidth probes (measured ceilings of the box next to the 8 TB/s specification) ----------------
 * a = b + s * c over n floats (stream triad; 12 bytes per element; c == NULL: copy a = b, 8 bytes per element; non_temporal
 * picks the load / store flavour), and a random whole-row gather with the access shape
 * of the SpMM's neighbour gather (64 rows of D floats per wavefront and index chunk, nothing else): sums of the gathered
 * rows land in out[tagrec_probe_gather_out_floats()], which exists only to keep the loads alive.  Indices are NOT
 * range-checked on the device: the caller guarantees 0 <= idx[i] < n_rows. */
int tagrec_probe_triad_f32(float* a, const float* b, const float* c, float s, int64_t n, int non_temporal, void* stream);
/* read-only stream over n floats; out holds tagrec_probe_gather_out_floats() floats (per-thread sums that keep the loads alive) */
int tagrec_probe_read_f32(const float* b, int64_t n, float* out, void* stream);
int64_t tagrec_probe_gather_out_floats(void);
int tagrec_probe_gather_rows_f32(const float* table, int64_t n_rows, int D, const int32_t* idx, int64_t n_idx, float* out,
                                 void* stream);
/* One wavefront spins for spin_us and returns out2 = {shader cycles, 100 MHz ticks}: launched on another stream before a
 * kernel, it measures the clock that kernel runs at (the peaks of the roofline are quoted at 2.4 GHz). */
int tagrec_probe_clock(int64_t spin_us, int64_t* out2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAGREC_H */
