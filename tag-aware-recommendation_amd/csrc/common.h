// Shared host-side helpers of libtagrec_hip (error slot, HIP call checking).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "../../include/tagrec.h"

namespace tagrec {

void set_error(const std::string& msg);

inline int fail(int code, const std::string& msg) {
  set_error(msg);
  return code;
}

#define TAGREC_HIP(expr)                                                                   \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return ::tagrec::fail(TAGREC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

#define TAGREC_REQUIRE(cond, msg)                                        \
  do {                                                                   \
    if (!(cond)) return ::tagrec::fail(TAGREC_E_INVALID, std::string(msg)); \
  } while (0)

// hand a callee's refusal on as it is (its message is already in the error slot)
#define TAGREC_TRY(expr)              \
  do {                                \
    const int _rc = (expr);           \
    if (_rc != TAGREC_OK) return _rc; \
  } while (0)

#define TAGREC_LAUNCH_CHECK() TAGREC_HIP(hipGetLastError())

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

constexpr int kWave = 64;

// splitmix64 finaliser: the counter-based generator behind the negative sampler and the dropout masks
__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Message dropout (F.dropout on a layer's output, /root/reference/model/lightgcn.py:56): whether element `index` of
// the tensor drawn under `seed` survives is a pure function of (seed, index), so the backward pass re-creates the
// forward's mask instead of storing it.  Four consecutive elements (one float4) share one hash: 4 x 16 bits.
struct DropMask {
  float p;          // drop probability; 0 = off
  uint64_t seed;
};
__device__ __forceinline__ void drop4(const DropMask& m, int64_t float4_index, float& a, float& b, float& c, float& d) {
  if (m.p <= 0.f) return;
  const uint64_t h = mix64(m.seed ^ mix64(static_cast<uint64_t>(float4_index)));
  const unsigned thr = static_cast<unsigned>(m.p * 65536.0f);          // keep iff 16-bit draw >= p * 2^16
  const float keep = 1.0f / (1.0f - m.p);
  a = ((h >> 0) & 0xFFFFu) >= thr ? a * keep : 0.f;
  b = ((h >> 16) & 0xFFFFu) >= thr ? b * keep : 0.f;
  c = ((h >> 32) & 0xFFFFu) >= thr ? c * keep : 0.f;
  d = ((h >> 48) & 0xFFFFu) >= thr ? d * keep : 0.f;
}


// Edge dropout (`node_drop`, /root/reference/model/help/adj.py:170-191) evaluated inside the products: whether the stored
// entry (i, j) of the FORWARD matrix survives is a pure function of (seed, i, j), so no dropped CSR is built, no mask is
// stored and the backward pass re-creates the forward's mask.  (i, j) and (j, i) draw independently, as the reference
// drops COO entries one by one.  A product with the TRANSPOSE walks the row of j and meets column i: `transposed` swaps the
// hash arguments so that it evaluates the mask of (i, j).  A kept entry contributes val / (1 - p).
struct EdgeDrop {
  float p;          // drop probability; 0 = nothing dropped
  uint64_t seed;
  int transposed;   // the walked matrix is the transpose of the one the mask is defined on
};
__host__ __device__ inline bool edge_kept(const EdgeDrop& d, int64_t row, int col) {
  const uint64_t i = static_cast<uint64_t>(d.transposed ? static_cast<int64_t>(col) : row);
  const uint32_t j = static_cast<uint32_t>(d.transposed ? row : static_cast<int64_t>(col));
  const uint64_t h = mix64(d.seed ^ mix64((i << 32) | j));
  return (h >> 40) >= static_cast<unsigned>(d.p * 16777216.0f);     // keep iff the 24-bit draw >= p * 2^24
}

// Noise direction of the SimGCL views (Yu et al., SIGIR 2022; include/tagrec.h has the key formula): the random unit vector
// that perturbs row `node` of a layer's product is a pure function of (step seed, view, layer, NODE ID, float4 index within
// the row), so the all-rows product, the row-masked one and the compact top layer perturb the same element the same way and
// nothing is stored.  One hash per float4: four 16-bit fields -> u in (0, 1], exact in fp32.  Every kernel that applies the
// perturbation sums ||u||^2 in ONE order (noise_ss4 per float4, then an xor butterfly over the row's float4 indices) and
// goes through noise_apply, so that they give the same bits.
struct NoiseDir {
  float eps;        // length of the perturbation; 0 = the row passes unchanged
  uint64_t key;     // noise_key(seed, view, layer)
};
__host__ __device__ inline uint64_t noise_key(uint64_t seed, int view, int layer) {
  return mix64(seed ^ mix64((static_cast<uint64_t>(static_cast<uint32_t>(view)) << 32) | static_cast<uint32_t>(layer)));
}
__device__ __forceinline__ void noise_u4(uint64_t key, int64_t node, int c4, float& a, float& b, float& c, float& d) {
  const uint64_t h = mix64(key ^ mix64((static_cast<uint64_t>(node) << 8) | static_cast<uint64_t>(c4)));
  a = static_cast<float>(((h >> 0) & 0xFFFFu) + 1u) * (1.0f / 65536.0f);
  b = static_cast<float>(((h >> 16) & 0xFFFFu) + 1u) * (1.0f / 65536.0f);
  c = static_cast<float>(((h >> 32) & 0xFFFFu) + 1u) * (1.0f / 65536.0f);
  d = static_cast<float>(((h >> 48) & 0xFFFFu) + 1u) * (1.0f / 65536.0f);
}
__device__ __forceinline__ float noise_ss4(float a, float b, float c, float d) {
  return fmaf(a, a, fmaf(b, b, fmaf(c, c, d * d)));
}
// y + eps sign(y) u / ||u||, sign(0) = 0 (an empty row stays zero); eps = 0 returns y
__device__ __forceinline__ float noise_apply(float y, float u, float u_norm, float eps) {
  const float se = y > 0.f ? eps : (y < 0.f ? -eps : 0.f);
  return fmaf(se, u / u_norm, y);
}

// torch.optim.Adam's update (_single_tensor_adam: exp_avg.lerp_(grad, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(grad, grad,
// 1 - b2); param.addcdiv_(exp_avg, sqrt(exp_avg_sq) / sqrt(bc2) + eps, -step_size)), shared by the Adam kernels (rowops.hip)
// and the last backward hop's fused epilogue (spmm.hip).  The roundings are PINNED -- contraction off, the three fused
// multiply-adds written out -- so that every kernel that applies the update gives the same bits whatever surrounds the call
// (left to the compiler, the vector kernel and a scalar kernel contracted differently).
__device__ __forceinline__ float adam_update1(float& m, float& v, float p, const float g, float w1, float b2, float w2, float step_size,
                                              float bc2_sqrt, float eps) {
#pragma clang fp contract(off)
  m = fmaf(w1, g - m, m);
  v = fmaf(w2 * g, g, v * b2);
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  return fmaf(-step_size, m / denom, p);
}
typedef float adam_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ adam_f4 adam_update(adam_f4& mi, adam_f4& vi, adam_f4 pi, const adam_f4 gi, float w1, float b2, float w2,
                                               float step_size, float bc2_sqrt, float eps) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float m = mi[c], v = vi[c];
    pi[c] = adam_update1(m, v, pi[c], gi[c], w1, b2, w2, step_size, bc2_sqrt, eps);
    mi[c] = m;
    vi[c] = v;
  }
  return pi;
}
// The two step-dependent factors of that update, lr / (1 - b1^t) and sqrt(1 - b2^t): torch's host arithmetic (python
// floats = doubles), each rounded to float once.  The one statement of it: tagrec_adam_f32 and the coefficient ring of
// the row-sparse Adam (tagrec_adam_coef) must agree to the bit.
inline void adam_step_coef(double lr, double b1, double b2, int64_t step, float* step_size, float* bc2_sqrt) {
  const double bc1 = 1.0 - pow(b1, static_cast<double>(step));
  const double bc2 = 1.0 - pow(b2, static_cast<double>(step));
  *step_size = static_cast<float>(lr / bc1);
  *bc2_sqrt = static_cast<float>(sqrt(bc2));
}
// Optional Adam update in place of a gradient store (EpiArgs::adam): p == nullptr -> off
struct AdamRow {
  float* p; float* m; float* v;
  float w1, b2, w2, step_size, bc2_sqrt, eps;
  const float* coef = nullptr;     // device [step_size, bc2_sqrt] advanced on the device (graph replay); overrides the two floats
};

}  // namespace tagrec
