// In-batch sampled softmax on compact rows: a flash-style fused B x B loss (tagrec_inbatch_fwd_f32 / tagrec_inbatch_bwd_f32).
//
// The B x B score matrix is never stored.  One block of four wavefronts OWNS a tile of 64 rows of one operand and WALKS the
// other operand in tiles of 64 rows; both tiles sit in LDS (row stride Dp + 4 floats: the 16 rows a wavefront reads land on
// 16 distinct groups of four banks).  A wavefront holds 16 owned rows.  Its 16 x 64 score tile comes from the exact-fp32
// MFMA 16x16x4 (the one csrc/eval.hip uses): A = walked rows, B = owned rows, so lane (r = lane % 16, q = lane / 16) ends with
// the scores of owned row r against the walked rows 16 t + 4 q + v (t, v = 0 .. 3).
//   forward   every lane keeps a running (maximum, sum) of its own columns, rescaled when the maximum moves; the four lanes of
//             a row are merged once, after the walk.  The maximum starts at a finite sentinel and the diagonal is never masked,
//             so neither "-inf - (-inf)" nor log(0) can be formed.
//   backward  the score tile is recomputed, C = scale (exp(z - lse) - delta) is formed in registers and fed STRAIGHT to the
//             second MFMA as its A operand: the k index of an MFMA step may be any permutation of the walked rows as long as
//             the B operand (the walked tile read from LDS by row 16 t + 4 q + v, column 16 f + r) uses the same one, so no
//             hand-over of C through LDS is needed.  The accumulators (Dp / 16 tiles of 16 x 16) stay in registers over the
//             walk and every owned row is stored once: no atomics, and the order of every sum is a function of (B, D) only.
// One templated body serves the three passes: the forward, the backward of the row operand (owner = Ub, walks Ib) and the
// backward of the column operand (owner = Ib, walks Ub; the row log-sum-exp is then indexed by the walked side and the column
// bias by the owned side).  Nothing in it knows what the two operands stand for.
#include "common.h"

namespace tagrec {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kTile = 64;                 // rows of the owned tile = rows of a walked tile = 16 per wavefront
constexpr float kLowest = -3.0e38f;       // start of the running maximum: finite, below every score

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

// rows row0 .. row0 + 63 of X -> sh [64, Dp + 4]; rows past B and columns past D are zero
__device__ __forceinline__ void stage_tile(float* sh, const float* __restrict__ X, int64_t ld, int D, int Dp, int64_t row0,
                                           int64_t B, bool vec) {
  const int S = Dp + 4, c4n = Dp >> 2;
  for (int idx = threadIdx.x; idx < kTile * c4n; idx += kThreads) {
    const int row = idx / c4n, c = (idx - row * c4n) << 2;
    const int64_t gr = row0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (gr < B && c < D) {
      const float* p = X + gr * ld + c;
      if (vec) {
        v = *reinterpret_cast<const f32x4*>(p);
      } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
      }
    }
    *reinterpret_cast<f32x4*>(sh + row * S + c) = v;
  }
}

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
  const int S = a.Dp + 4;
  float* sh_walk = sh_own + kTile * S;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const int64_t B = a.B, own0 = static_cast<int64_t>(blockIdx.x) * kTile;
  const bool vec = a.vec != 0;
  const bool ids = a.uid != nullptr;

  stage_tile(sh_own, a.X[OWN], a.ld, a.D, a.Dp, own0, B, vec);

  const int64_t o = own0 + 16 * wave + r;              // the owned row whose scores this lane ends up with
  const bool o_ok = o < B;
  const int64_t o_uid = (ids && o_ok) ? a.uid[o] : 0, o_iid = (ids && o_ok) ? a.iid[o] : 0;
  const float o_bias = (MODE == 2 && a.col_bias && o_ok) ? a.col_bias[o] : 0.f;
  const float o_lse = (MODE == 1 && o_ok) ? a.lse[o] : 0.f;
  const float scale = MODE == 0 ? 0.f : ((a.g ? a.g[0] : 1.0f) * a.inv_tau) * a.inv_b;

  float run_m = kLowest, run_s = 0.f, zd = 0.f;        // forward: this lane's columns only
  f32x4 acc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t w0 = 0; w0 < B; w0 += kTile) {
    __syncthreads();                                   // the previous walked tile has been consumed
    stage_tile(sh_walk, a.X[WALK], a.ld, a.D, a.Dp, w0, B, vec);
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
#pragma unroll
    for (int t = 0; t < 4; ++t) sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* po = sh_own + (16 * wave + r) * S + 4 * q;
    const float* pw = sh_walk + r * S + 4 * q;
    for (int kk = 0; kk < a.Dk; kk += 16) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(po + kk);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(pw + t * 16 * S + kk);
#pragma unroll
        for (int c = 0; c < 4; ++c) sc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bv[c], sc[t], 0, 0, 0);
      }
    }
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
            if (z > run_m) {
              run_s = run_s * expf(run_m - z) + 1.0f;
              run_m = z;
            } else {
              run_s += expf(z - run_m);
            }
            if (diag) zd = z;
          }
        } else {
          const float l = MODE == 1 ? o_lse : sh_lse[wl];
          sc[t][v] = live ? scale * (expf(z - l) - (diag ? 1.0f : 0.0f)) : 0.0f;
        }
      }
    }
    if (MODE != 0) {
      // acc[f] += C [16 owned, 64 walked] . walked tile [64, 16 f .. 16 f + 15]; MFMA step (t, v) takes k = 16 t + 4 q + v
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float* pb = sh_walk + (16 * t + 4 * q + v) * S + r;
#pragma unroll
          for (int f = 0; f < NF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[t][v], pb[16 * f], acc[f], 0, 0, 0);
        }
      }
    }
  }

  if (MODE == 0) {
    // merge the four lanes of a row (q = 0 .. 3) in a fixed order; an empty lane holds (kLowest, 0)
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float m2 = __shfl_xor(run_m, off), s2 = __shfl_xor(run_s, off);
      const float mn = fmaxf(run_m, m2);
      run_s = run_s * expf(run_m - mn) + s2 * expf(m2 - mn);
      run_m = mn;
      zd += __shfl_xor(zd, off);                       // exactly one of the four lanes holds the diagonal
    }
    float loss = 0.f;
    if (o_ok) {                                        // the diagonal is live: run_m is a score, run_s >= 1
      const float l = run_m + logf(run_s);
      loss = l - zd;
      if (q == 0) a.lse_out[o] = l;
    }
    if (q != 0) loss = 0.f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) loss += __shfl_xor(loss, off);
    // 0.5 |row|^2 of the block's 2 x 64 L2 rows: one row per wavefront at a time, fixed order
    float reg = 0.f;
    if (a.Xreg[0]) {
      for (int side = 0; side < 2; ++side) {
        for (int i = 0; i < 16; ++i) {
          const int64_t row = own0 + 16 * wave + i;
          if (row >= B) break;
          const float* p = a.Xreg[side] + row * a.ldreg;
          float s = 0.f;
          for (int c = lane; c < a.Dreg; c += 64) s = fmaf(p[c], p[c], s);
#pragma unroll
          for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
          reg += s;
        }
      }
    }
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
    // acc[f][v] = d owned row 16 wave + 4 q + v, column 16 f + r
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int c = 16 * f + r;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t row = own0 + 16 * wave + 4 * q + v;
        if (row < B && c < a.D) {
          float val = acc[f][v];
          if (shared) val += rscale * R[row * a.ldreg + c];
          dX[row * a.ld + c] = val;
        }
      }
    }
    if (dR != nullptr && !shared) {
      for (int idx = tid; idx < kTile * a.Dreg; idx += kThreads) {
        const int row = idx / a.Dreg, c = idx - row * a.Dreg;
        const int64_t gr = own0 + row;
        if (gr < B) dR[gr * a.ldreg + c] = rscale * R[gr * a.ldreg + c];
      }
    }
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

// loss_out[k] = inv_b * sum over blocks of partials[2 i + k]: strided per-thread sums, then a fixed tree
__global__ __launch_bounds__(kThreads) void inbatch_reduce_kernel(const float* __restrict__ partials, int64_t n, float inv_b,
                                                                  float* __restrict__ loss_out) {
  __shared__ float sh[2][kThreads];
  float s0 = 0.f, s1 = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    s0 += partials[2 * i];
    s1 += partials[2 * i + 1];
  }
  sh[0][threadIdx.x] = s0;
  sh[1][threadIdx.x] = s1;
  __syncthreads();
  for (int off = kThreads / 2; off >= 1; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + off];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss_out[0] = sh[0][0] * inv_b;
    loss_out[1] = sh[1][0] * inv_b;
  }
}

size_t lds_bytes(int Dp) {
  return 2 * kTile * sizeof(int64_t) + (2 * kTile + 16) * sizeof(float) + 2 * static_cast<size_t>(kTile) * (Dp + 4) * sizeof(float);
}

// the accumulator tiles the backward is built for: the smallest NF with 16 NF >= D
int pick_nf(int D) {
  const int nfs[] = {1, 2, 4, 8, 12, 16};
  for (int nf : nfs)
    if (16 * nf >= D) return nf;
  return 0;
}

int check_shape(const char* what, int64_t B, int D, int64_t ld) {
  if (D < 8 || D > 256 || (D & 3) != 0)
    return fail(TAGREC_E_UNSUPPORTED, std::string(what) + ": D must be a multiple of 4 in 8 .. 256, got " + std::to_string(D));
  if (B < 1 || B > 65536)
    return fail(TAGREC_E_UNSUPPORTED, std::string(what) + ": B must be in 1 .. 65536, got " + std::to_string(B));
  if (ld < D) return fail(TAGREC_E_INVALID, std::string(what) + ": row stride below D");
  return TAGREC_OK;
}

// Dynamic LDS past the default 64 KB (D > 112) needs the function attribute: it is set once per kernel instantiation and
// device (the largest size asked for so far), so a later launch -- one inside a stream capture included -- makes no host call.
template <void (*KERN)(InbatchArgs)>
int launch(dim3 grid, size_t lds, const InbatchArgs& a, hipStream_t s) {
  constexpr int kMaxDevices = 64;
  static int granted[kMaxDevices] = {};
  if (lds > 64 * 1024) {
    int dev = 0;
    TAGREC_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices || granted[dev] < static_cast<int>(lds)) {
      TAGREC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
      if (dev >= 0 && dev < kMaxDevices) granted[dev] = static_cast<int>(lds);
    }
  }
  KERN<<<grid, kThreads, lds, s>>>(a);
  TAGREC_LAUNCH_CHECK();
  return TAGREC_OK;
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
  TAGREC_REQUIRE(temperature > 0.f && temperature <= 3.4028234e38f, "inbatch_fwd: the temperature must be finite and > 0");
  if (int rc = check_shape("inbatch_fwd", B, D, ld)) return rc;
  InbatchArgs a = {};
  a.X[0] = Ub; a.X[1] = Ib; a.ld = ld; a.D = D; a.Dk = (D + 15) & ~15; a.Dp = a.Dk;
  a.vec = aligned16(Ub) && aligned16(Ib) && (ld & 3) == 0;
  a.uid = uid; a.iid = iid; a.col_bias = col_bias;
  a.Xreg[0] = Ureg; a.Xreg[1] = Ireg; a.ldreg = ldreg; a.Dreg = Dreg;
  a.B = B; a.inv_tau = 1.0f / temperature; a.inv_b = 1.0f / static_cast<float>(B);
  a.lse_out = lse; a.partials = partials;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t blocks = (B + kTile - 1) / kTile;
  if (int rc = launch<inbatch_fwd_kernel>(dim3(static_cast<unsigned>(blocks)), lds_bytes(a.Dp), a, s)) return rc;
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
  TAGREC_REQUIRE(temperature > 0.f && temperature <= 3.4028234e38f, "inbatch_bwd: the temperature must be finite and > 0");
  if (int rc = check_shape("inbatch_bwd", B, D, ld)) return rc;
  InbatchArgs a = {};
  const int nf = pick_nf(D);
  a.X[0] = Ub; a.X[1] = Ib; a.ld = ld; a.D = D; a.Dk = (D + 15) & ~15; a.Dp = 16 * nf;
  a.vec = aligned16(Ub) && aligned16(Ib) && (ld & 3) == 0;
  a.uid = uid; a.iid = iid; a.col_bias = col_bias;
  a.Xreg[0] = Ureg; a.Xreg[1] = Ireg; a.ldreg = ldreg; a.Dreg = Dreg;
  a.B = B; a.inv_tau = 1.0f / temperature; a.inv_b = 1.0f / static_cast<float>(B);
  a.lse = lse; a.g = g; a.dX[0] = dUb; a.dX[1] = dIb; a.dXreg[0] = dUreg; a.dXreg[1] = dIreg;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>((B + kTile - 1) / kTile), 2);
  const size_t lds = lds_bytes(a.Dp);
  switch (nf) {
    case 1: return launch<inbatch_bwd_kernel<1>>(grid, lds, a, s);
    case 2: return launch<inbatch_bwd_kernel<2>>(grid, lds, a, s);
    case 4: return launch<inbatch_bwd_kernel<4>>(grid, lds, a, s);
    case 8: return launch<inbatch_bwd_kernel<8>>(grid, lds, a, s);
    case 12: return launch<inbatch_bwd_kernel<12>>(grid, lds, a, s);
    default: return launch<inbatch_bwd_kernel<16>>(grid, lds, a, s);
  }
}
