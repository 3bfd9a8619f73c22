// In-batch sampled softmax on compact rows: a flash-style fused B x B loss (tagrec_inbatch_fwd_f32 / tagrec_inbatch_bwd_f32).
//
// The tile scheme (owned tile x walked tile in LDS, score MFMA, running (maximum, sum), C fed straight to the second MFMA)
// is the one of csrc/pairtile.h.  What is this loss's own: the diagonal is the positive and is never masked, so a row always
// has a live column; a column that repeats the row's user or item id is masked; the column bias joins the logit's one rounding.
// One templated body serves the three passes: the forward, the backward of the row operand (owner = Ub, walks Ib) and the
// backward of the column operand (owner = Ib, walks Ub; the row log-sum-exp is then indexed by the walked side and the column
// bias by the owned side).  Nothing in it knows what the two operands stand for.
#include "pairtile.h"

namespace tagrec {
namespace {

struct InbatchArgs {
  const float* X[2];                      // 0: Ub (rows of the score matrix), 1: Ib (columns)
  int64_t ld;
  int D, Dk, Dp;                          // Dk = D rounded up to 16 (score loop), Dp = 16 NF >= Dk (LDS row width)
  int vec;                                // both operands 16-byte aligned with ld % 4 == 0: float4 loads
  const int64_t* uid;
  const int64_t* iid;
  const float* col_bias;
  const float* Xreg[2];
  int64_t ldreg;
  int Dreg;
  int64_t B;
  float inv_tau, inv_b;
  float* lse_out;                         // forward
  float* partials;
  const float* lse;                       // backward
  const float* g;
  float* dX[2];
  float* dXreg[2];
};

// MODE 0: forward (owner = rows).  MODE 1: backward, owner = rows (dUb).  MODE 2: backward, owner = columns (dIb).
template <int MODE, int NF>
__device__ __forceinline__ void inbatch_body(const InbatchArgs& a, unsigned char* smem) {
  constexpr int OWN = MODE == 2 ? 1 : 0, WALK = 1 - OWN;
  int64_t* sh_uid = reinterpret_cast<int64_t*>(smem);
  int64_t* sh_iid = sh_uid + kTile;
  float* sh_bias = reinterpret_cast<float*>(sh_iid + kTile);
  float* sh_lse = sh_bias + kTile;
  float* sh_red = sh_lse + kTile;                      // 16 floats
  float* sh_own = sh_red + 16;
  const int S = tile_stride(a.Dp);
  float* sh_walk = sh_own + kTile * S;

  const PairLane ln = pair_lane();
  const int tid = threadIdx.x, wave = ln.wave, lane = ln.lane, r = ln.r, q = ln.q;
  const int64_t B = a.B, own0 = static_cast<int64_t>(blockIdx.x) * kTile;
  const bool vec = a.vec != 0;
  const bool ids = a.uid != nullptr;

  stage_tile<false>(sh_own, a.X[OWN], nullptr, a.ld, a.D, a.Dp, own0, B, vec);

  const int64_t o = own0 + 16 * wave + r;              // the owned row whose scores this lane ends up with
  const bool o_ok = o < B;
  const int64_t o_uid = (ids && o_ok) ? a.uid[o] : 0, o_iid = (ids && o_ok) ? a.iid[o] : 0;
  const float o_bias = (MODE == 2 && a.col_bias && o_ok) ? a.col_bias[o] : 0.f;
  const float o_lse = (MODE == 1 && o_ok) ? a.lse[o] : 0.f;
  const float scale = MODE == 0 ? 0.f : ((a.g ? a.g[0] : 1.0f) * a.inv_tau) * a.inv_b;

  float run_m = kLowest, run_s = 0.f, zd = 0.f;        // forward: this lane's columns only
  AccTiles<NF> acc;
  zero_acc(acc);

  for (int64_t w0 = 0; w0 < B; w0 += kTile) {
    __syncthreads();                                   // the previous walked tile has been consumed
    stage_tile<false>(sh_walk, a.X[WALK], nullptr, a.ld, a.D, a.Dp, w0, B, vec);
    if (tid < kTile) {
      const int64_t w = w0 + tid;
      const bool ok = w < B;
      if (ids) {
        sh_uid[tid] = ok ? a.uid[w] : 0;
        sh_iid[tid] = ok ? a.iid[w] : 0;
      }
      if (MODE != 2) sh_bias[tid] = (a.col_bias && ok) ? a.col_bias[w] : 0.f;
      if (MODE == 2) sh_lse[tid] = ok ? a.lse[w] : 0.f;
    }
    __syncthreads();

    f32x4 sc[4];
    score_tile(sh_own, sh_walk, S, a.Dk, ln, sc);
    // sc[t][v] = owned row o . walked row w0 + 16 t + 4 q + v
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int wl = 16 * t + 4 * q + v;
        const int64_t w = w0 + wl;
        const bool diag = w == o;
        bool live = o_ok && w < B;
        if (ids) live = live && (diag || (sh_iid[wl] != o_iid && sh_uid[wl] != o_uid));
        const float z = fmaf(sc[t][v], a.inv_tau, -(MODE == 2 ? o_bias : sh_bias[wl]));   // one rounding, the same in every pass
        if (MODE == 0) {
          if (live) {
            lse_push(run_m, run_s, z);
            if (diag) zd = z;
          }
        } else {
          const float l = MODE == 1 ? o_lse : sh_lse[wl];
          sc[t][v] = live ? scale * (expf(z - l) - (diag ? 1.0f : 0.0f)) : 0.0f;
        }
      }
    }
    if (MODE != 0) grad_tile<NF>(sh_walk, S, ln, sc, acc);
  }

  if (MODE == 0) {
    lse_merge_q(run_m, run_s);
    zd += __shfl_xor(zd, 16);                          // exactly one of the four lanes of a row holds the diagonal
    zd += __shfl_xor(zd, 32);
    float loss = 0.f;
    if (o_ok) {                                        // the diagonal is live: run_m is a score, run_s >= 1
      const float l = run_m + logf(run_s);
      loss = l - zd;
      if (q == 0) a.lse_out[o] = l;
    }
    if (q != 0) loss = 0.f;
    loss = wave_sum(loss);
    // 0.5 |row|^2 of the block's 2 x 64 L2 rows
    float reg = 0.f;
    if (a.Xreg[0]) reg = l2_rows([&](int side, int64_t row) { return a.Xreg[side] + row * a.ldreg; }, own0, 16, B, a.Dreg, ln);
    if (lane == 0) {
      sh_red[wave] = loss;
      sh_red[4 + wave] = reg;
    }
    __syncthreads();
    if (tid == 0) {
      a.partials[2 * blockIdx.x] = (sh_red[0] + sh_red[1]) + (sh_red[2] + sh_red[3]);
      a.partials[2 * blockIdx.x + 1] = 0.5f * ((sh_red[4] + sh_red[5]) + (sh_red[6] + sh_red[7]));
    }
  } else {
    float* dX = a.dX[OWN];
    float* dR = a.dXreg[OWN];
    const float* R = a.Xreg[OWN];
    const float rscale = (a.g ? a.g[1] : 1.0f) * a.inv_b;
    const bool shared = dR != nullptr && dR == dX;     // one buffer takes both parts (then Xreg = X, checked by the caller)
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int c = 16 * f + r;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t row = own0 + 16 * wave + 4 * q + v;
        if (row < B && c < a.D) {
          float val = acc.f[f][v];
          if (shared) val += rscale * R[row * a.ldreg + c];
          dX[row * a.ld + c] = val;
        }
      }
    }
    if (dR != nullptr && !shared) l2_grad_tail(dR, R, a.ldreg, a.Dreg, rscale, own0, B);
  }
}

__global__ __launch_bounds__(kThreads) void inbatch_fwd_kernel(InbatchArgs a) {
  extern __shared__ __align__(16) unsigned char inbatch_smem[];
  inbatch_body<0, 1>(a, inbatch_smem);
}

// blockIdx.y = 0: the row operand's gradient; 1: the column operand's (the same body, roles swapped)
template <int NF>
__global__ __launch_bounds__(kThreads) void inbatch_bwd_kernel(InbatchArgs a) {
  extern __shared__ __align__(16) unsigned char inbatch_smem[];
  if (blockIdx.y == 0)
    inbatch_body<1, NF>(a, inbatch_smem);
  else
    inbatch_body<2, NF>(a, inbatch_smem);
}

__global__ __launch_bounds__(kThreads) void inbatch_reduce_kernel(const float* __restrict__ partials, int64_t n, float inv_b,
                                                                  float* __restrict__ loss_out) {
  reduce_loss_pair(partials, n, inv_b, loss_out);
}

size_t lds_bytes(int Dp) {
  return 2 * kTile * sizeof(int64_t) + (2 * kTile + 16) * sizeof(float) + tiles_bytes(Dp);
}

int check_shape(const char* what, int64_t B, int D, int64_t ld) {
  if (int rc = check_rows(what, B, 1, "", D)) return rc;
  return check_stride(what, ld, D);
}

}  // namespace
}  // namespace tagrec

using namespace tagrec;

extern "C" int tagrec_inbatch_fwd_f32(const float* Ub, const float* Ib, int64_t ld, int D, const int64_t* uid, const int64_t* iid,
                                      const float* col_bias, const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                                      int64_t B, float temperature, float* lse, float* partials, float* loss_out, void* stream) {
  TAGREC_REQUIRE(Ub && Ib && lse && partials && loss_out, "inbatch_fwd: null pointer");
  TAGREC_REQUIRE((uid == nullptr) == (iid == nullptr), "inbatch_fwd: uid/iid must both be given or both null");
  TAGREC_REQUIRE((Ureg == nullptr) == (Ireg == nullptr), "inbatch_fwd: Ureg/Ireg must both be given or both null");
  TAGREC_REQUIRE(!Ureg || (Dreg >= 1 && ldreg >= Dreg), "inbatch_fwd: bad reg shape");
  if (int rc = check_temperature("inbatch_fwd", temperature)) return rc;
  if (int rc = check_shape("inbatch_fwd", B, D, ld)) return rc;
  InbatchArgs a = {};
  a.X[0] = Ub; a.X[1] = Ib; a.ld = ld; a.D = D; a.Dk = round16(D); a.Dp = a.Dk;
  a.vec = aligned16(Ub) && aligned16(Ib) && (ld & 3) == 0;
  a.uid = uid; a.iid = iid; a.col_bias = col_bias;
  a.Xreg[0] = Ureg; a.Xreg[1] = Ireg; a.ldreg = ldreg; a.Dreg = Dreg;
  a.B = B; a.inv_tau = 1.0f / temperature; a.inv_b = 1.0f / static_cast<float>(B);
  a.lse_out = lse; a.partials = partials;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t blocks = (B + kTile - 1) / kTile;
  if (int rc = launch_lds<InbatchArgs, inbatch_fwd_kernel>(dim3(static_cast<unsigned>(blocks)), lds_bytes(a.Dp), a, s)) return rc;
  inbatch_reduce_kernel<<<1, kThreads, 0, s>>>(partials, blocks, a.inv_b, loss_out);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
}

extern "C" int tagrec_inbatch_bwd_f32(const float* Ub, const float* Ib, int64_t ld, int D, const int64_t* uid, const int64_t* iid,
                                      const float* col_bias, const float* Ureg, const float* Ireg, int64_t ldreg, int Dreg,
                                      int64_t B, float temperature, const float* lse, const float* g, float* dUb, float* dIb,
                                      float* dUreg, float* dIreg, void* stream) {
  TAGREC_REQUIRE(Ub && Ib && lse && dUb && dIb, "inbatch_bwd: null pointer");
  TAGREC_REQUIRE((uid == nullptr) == (iid == nullptr), "inbatch_bwd: uid/iid must both be given or both null");
  TAGREC_REQUIRE((Ureg == nullptr) == (Ireg == nullptr) && (dUreg == nullptr) == (dIreg == nullptr),
                 "inbatch_bwd: Ureg/Ireg and dUreg/dIreg must both be given or both null");
  TAGREC_REQUIRE(!dUreg || (Ureg && Dreg >= 1 && ldreg >= Dreg), "inbatch_bwd: bad reg arguments");
  TAGREC_REQUIRE(!dUreg || ((dUreg == dUb) == (dIreg == dIb)), "inbatch_bwd: dUreg/dIreg must both alias dUb/dIb or neither");
  TAGREC_REQUIRE(!dUreg || dUreg != dUb || (Ureg == Ub && Ireg == Ib && ldreg == ld && Dreg == D),
                 "inbatch_bwd: a gradient buffer shared by both parts needs Ureg = Ub and Ireg = Ib");
  if (int rc = check_temperature("inbatch_bwd", temperature)) return rc;
  if (int rc = check_shape("inbatch_bwd", B, D, ld)) return rc;
  InbatchArgs a = {};
  const int nf = pick_nf(D);
  a.X[0] = Ub; a.X[1] = Ib; a.ld = ld; a.D = D; a.Dk = round16(D); a.Dp = 16 * nf;
  a.vec = aligned16(Ub) && aligned16(Ib) && (ld & 3) == 0;
  a.uid = uid; a.iid = iid; a.col_bias = col_bias;
  a.Xreg[0] = Ureg; a.Xreg[1] = Ireg; a.ldreg = ldreg; a.Dreg = Dreg;
  a.B = B; a.inv_tau = 1.0f / temperature; a.inv_b = 1.0f / static_cast<float>(B);
  a.lse = lse; a.g = g; a.dX[0] = dUb; a.dX[1] = dIb; a.dXreg[0] = dUreg; a.dXreg[1] = dIreg;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((B + kTile - 1) / kTile), 2);
  const size_t lds = lds_bytes(a.Dp);
  return dispatch_nf(nf, [&](auto n) { return launch_lds<InbatchArgs, inbatch_bwd_kernel<decltype(n)::value>>(grid, lds, a, s); });
}
