// hf_dense_act.h -- what the two dense kernel families (hf_dense.hip: batches <= 256 rows; hf_dense_tall.hip: 257 .. 8192
// rows) share: the limits of a split reduction, the predicated 16-byte / element load, the activation factor and the two
// elementwise passes that do not reduce over the rows (k_dense_act_tangent, k_dense_act_forward) with their validator.
// ONE copy of that arithmetic: each family's entry points differ in the row range they accept, nothing else.
#pragma once
#include "hf_common.h"

namespace {

constexpr int DENSE_MAX_SPLITS = 32;
constexpr int64_t DENSE_MAX_C = 1 << 20;

inline bool quad_ok(const void* p, int64_t pitch) { return aligned16(p) && (pitch & 3) == 0; }

struct Quad { float e[4]; };

// p[k .. k+3] of a row that ends at `end`; `ok` = the row exists.  Entries outside read as zero and are not touched.
template <bool ALIGNED>
__device__ __forceinline__ Quad ld_quad(const float* __restrict__ p, int k, int end, bool ok) {
  Quad q;
  if (ALIGNED && ok && k + 4 <= end) {
    const F4 v = ld4(p + k);
#pragma unroll
    for (int e = 0; e < 4; ++e) q.e[e] = v.e[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) q.e[e] = (ok && k + e < end) ? p[k + e] : 0.0f;
  }
  return q;
}

// ---- activation factor ---------------------------------------------------------------------------------------------
enum { ACT_IDENTITY = 0, ACT_RELU = 1, ACT_TANH = 2 };

// s * act'(y): relu  y > 0 ? s : 0  (as k_chan_affine);  tanh  s * (1 - y*y)  (three roundings)
__device__ __forceinline__ float act_apply(float s, const float* __restrict__ y, int idx, int act) {
  if (act == ACT_RELU) return y[idx] > 0.0f ? s : 0.0f;
  if (act == ACT_TANH) {
    const float yy = y[idx];
    return s * (1.0f - yy * yy);
  }
  return s;
}

// one entry of an activation adjoint: (sum of slabs) * act'(y); CURV adds the tanh curvature term (hf_dense.hip,
// k_dense_act_adjoint: the order of the roundings is documented there)
template <bool CURV>
__device__ __forceinline__ float act_adjoint_value(const float* __restrict__ slabs, int idx, int splits, long long stride,
                                                   const float* __restrict__ y, int act, const float* __restrict__ ty,
                                                   const float* __restrict__ h1) {
  const float s = slab_sum<4>(slabs[idx], slabs, idx, splits, stride);
  float gv = act_apply(s, y, idx, act);
  if (CURV) gv = fmaf((-2.0f * y[idx]) * ty[idx], h1[idx], gv);
  return gv;
}

// t_y = (sum of slabs + v_b[col]) * act'(y)
__global__ __launch_bounds__(BLOCK) void k_dense_act_tangent(float* __restrict__ ty, const float* __restrict__ slabs,
                                                             int splits, long long stride, const float* __restrict__ vb,
                                                             const float* __restrict__ y, int act, int total, int c) {
  const int idx = blockIdx.x * BLOCK + threadIdx.x;
  if (idx >= total) return;
  float s = slab_sum<4>(slabs[idx], slabs, idx, splits, stride);
  if (vb) s += vb[idx % c];
  ty[idx] = act_apply(s, y, idx, act);
}

// ---- forward pass of a layer: y = act(sum of slabs + b[col]) ------------------------------------------------------
// The slab sum and the bias addition are k_dense_act_tangent's; then relu  s <= 0 ? +0 : s  (a NaN stays a NaN, as in
// ATen's relu: a trial point whose hidden layer is NaN must not report a finite loss) or  tanhf(s).
__global__ __launch_bounds__(BLOCK) void k_dense_act_forward(float* __restrict__ y, const float* __restrict__ slabs,
                                                             int splits, long long stride, const float* __restrict__ b,
                                                             int act, int total, int c) {
  const int idx = blockIdx.x * BLOCK + threadIdx.x;
  if (idx >= total) return;
  float s = slab_sum<4>(slabs[idx], slabs, idx, splits, stride);
  if (b) s += b[idx % c];
  if (act == ACT_RELU) s = s <= 0.0f ? 0.0f : s;
  if (act == ACT_TANH) s = tanhf(s);
  y[idx] = s;
}

// the operands of an elementwise pass over `splits` slabs of [rows, c], rows in [rows_lo, rows_hi]
inline bool act_args_in(const void* slabs, int splits, int64_t slab_stride, const void* y, int act, int64_t rows,
                        int64_t c, int dtype, int64_t rows_lo, int64_t rows_hi) {
  if (dtype != HF_F32 || !slabs) return false;
  if (rows < rows_lo || rows > rows_hi || c < 1 || c > DENSE_MAX_C) return false;
  if (splits < 1 || splits > DENSE_MAX_SPLITS) return false;
  if (splits > 1 && slab_stride < rows * c) return false;
  if (act < ACT_IDENTITY || act > ACT_TANH) return false;
  if (act != ACT_IDENTITY && !y) return false;
  return true;
}

// the curvature term's operands: tanh needs the tangent output and the first-order cotangent (act'' = 0 otherwise)
inline bool act_curv_args_ok(int act, const void* t_y, const void* h) { return act != ACT_TANH || (t_y && h); }

// hf_dense_act_tangent / hf_dense_tall_act_tangent: one validator sequence and one launch, the row range is the caller's
inline int dense_act_tangent_launch(void* t_y, const void* slabs, int splits, int64_t slab_stride, const void* v_b,
                                    const void* y, int act, int64_t rows, int64_t c, int dtype, void* stream,
                                    int64_t rows_lo, int64_t rows_hi) {
  if (!t_y || !act_args_in(slabs, splits, slab_stride, y, act, rows, c, dtype, rows_lo, rows_hi)) return HF_ERR_ARG;
  if (rows * c >= ((int64_t)1 << 31)) return HF_ERR_ARG;
  const int total = (int)(rows * c);
  k_dense_act_tangent<<<(total + BLOCK - 1) / BLOCK, BLOCK, 0, (hipStream_t)stream>>>(
      (float*)t_y, (const float*)slabs, splits, (long long)slab_stride, (const float*)v_b, (const float*)y, act, total,
      (int)c);
  return (int)hipGetLastError();
}

// hf_dense_act_forward / hf_dense_tall_act_forward
inline int dense_act_forward_launch(void* y, const void* slabs, int splits, int64_t slab_stride, const void* b, int act,
                                    int64_t rows, int64_t c, int dtype, void* stream, int64_t rows_lo, int64_t rows_hi) {
  if (!y || !act_args_in(slabs, splits, slab_stride, y, act, rows, c, dtype, rows_lo, rows_hi)) return HF_ERR_ARG;
  if (rows * c >= ((int64_t)1 << 31)) return HF_ERR_ARG;
  const int total = (int)(rows * c);
  k_dense_act_forward<<<(total + BLOCK - 1) / BLOCK, BLOCK, 0, (hipStream_t)stream>>>(
      (float*)y, (const float*)slabs, splits, (long long)slab_stride, (const float*)b, act, total, (int)c);
  return (int)hipGetLastError();
}

}  // namespace
