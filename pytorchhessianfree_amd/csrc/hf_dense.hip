// hf_dense.hip -- fully-connected layers inside the GGN product (the dense-stack curvature engine, engine/dense.py):
// skinny fp32 GEMMs (batch rows <= 256) on __builtin_amdgcn_mfma_f32_32x32x2f32 that read the weight [c_out, c_in] and
// the matching slice of the CG vector IN PLACE in the flat vectors -- no [W | v_W] copy, no transposed copy, no gather
// afterwards -- plus the two elementwise passes between them, the diagonal of the empirical Fisher of the same layers
// (the weight-gradient GEMM on squared operands, a column sum of squares), and the second-order adjoint sweep of the
// Hessian product (forward over reverse: the two-term forms hf_dense_wgrad2 / hf_dense_dgrad2_slabs of the W and D GEMMs
// and the tanh curvature term of hf_dense_act_adjoint2 -- each the body of its sibling under a template flag), and what a
// persistent session replays per step and per trial point: the forward pass's slab sum + bias + activation
// (hf_dense_act_forward) and the loss head on the logits (hf_dense_loss_head: softmax cross-entropy or mean-squared error).
// fp32, wave64, no atomics; partial results of a split
// reduction leave as slabs that the consumer adds by the rule of hf_common.h::slab_sum; every kernel sums in one fixed
// order, so two launches on the same operands agree bitwise.
//
// Fragment layout of the 32x32x2 MFMA (wave64): lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31];
// accumulator register q of lane l is C[(q & 3) + 8 * (q >> 2) + 4 * (l >> 5)][l & 31].  The reduction index may be
// visited in any order as long as A and B agree, so a lane takes FOUR consecutive k (one 16-byte load where the operand
// allows it) and feeds them to four MFMAs; likewise four consecutive output columns per lane where the OUTPUT is the
// wide operand (hf_dense_wgrad).
//
// Operands may sit anywhere in a flat parameter vector (4-byte aligned, row lengths that are no multiple of 4): the host
// picks the 16-byte form only when base pointers and row pitches allow it, else the kernels load element by element.
// Every load is predicated on its row and column: nothing outside rows x c is ever read.
#include "hf_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DENSE_MAX_ROWS = 256;
constexpr int DENSE_MAX_SPLITS = 32;
constexpr int64_t DENSE_MAX_C = 1 << 20;
constexpr int DENSE_KSTEP = 32;        // reduction entries one pass of a workgroup consumes: 4 waves x 8
constexpr int DENSE_TARGET_BLOCKS = 512;

// ---- the plan: ONE definition, run by hf_dense_plan and by every launching entry point ----------------------------
inline bool dense_dims_ok(int64_t rows, int64_t c_in, int64_t c_out) {
  return rows >= 1 && rows <= DENSE_MAX_ROWS && c_in >= 1 && c_in <= DENSE_MAX_C && c_out >= 1 && c_out <= DENSE_MAX_C;
}

// reduction entries per split: a multiple of DENSE_KSTEP
inline int64_t dense_kper(int64_t len, int splits) {
  const int64_t per = (len + splits - 1) / splits;
  return (per + DENSE_KSTEP - 1) / DENSE_KSTEP * DENSE_KSTEP;
}

// a split count the kernels accept for a reduction of `len` entries: no split may start behind the end
inline bool dense_split_ok(int64_t len, int splits) {
  if (splits < 1 || splits > DENSE_MAX_SPLITS) return false;
  return (int64_t)(splits - 1) * dense_kper(len, splits) < len;
}

// the planned count: about DENSE_TARGET_BLOCKS workgroups of one 32-column tile each
inline int dense_planned_splits(int64_t len, int64_t out_cols) {
  const int64_t tiles = (out_cols + 31) / 32;
  int64_t want = (DENSE_TARGET_BLOCKS + tiles - 1) / tiles;
  if (want > DENSE_MAX_SPLITS) want = DENSE_MAX_SPLITS;
  int s = (int)want;
  while (s > 1 && !dense_split_ok(len, s)) --s;
  return s;
}

struct DensePlan {
  int splits_t, splits_d;
};

inline int dense_plan(int64_t rows, int64_t c_in, int64_t c_out, DensePlan* p) {
  if (!dense_dims_ok(rows, c_in, c_out)) return HF_ERR_ARG;
  p->splits_t = dense_planned_splits(c_in, c_out);   // T: reduction over c_in, output [rows, c_out]
  p->splits_d = dense_planned_splits(c_out, c_in);   // D: reduction over c_out, output [rows, c_in]
  return HF_OK;
}

inline bool quad_ok(const void* p, int64_t pitch) { return aligned16(p) && (pitch & 3) == 0; }

// ---- device helpers ------------------------------------------------------------------------------------------------
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

// The four waves of a workgroup hold partial sums of the same 32x32 tile (each took every fourth 8-entry step of the
// split's range): added in wave order ((w0 + w1) + w2) + w3 through LDS and written to out[row0 + .][col0 + .].
__device__ __forceinline__ void store_tile_sum(float (*red)[1024], const f32x16& acc, float* __restrict__ out, int row0,
                                               int rows, int col0, int cols) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (the previous tile's readers are done)
#pragma unroll
  for (int q = 0; q < 16; ++q) red[wave][q * 64 + lane] = acc[q];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = threadIdx.x + 256 * u, q = e >> 6, ln = e & 63;
    float s = red[0][e];
    s += red[1][e];
    s += red[2][e];
    s += red[3][e];
    const int r = row0 + (q & 3) + 8 * (q >> 2) + 4 * (ln >> 5), c = col0 + (ln & 31);
    if (r < rows && c < cols) out[(size_t)r * cols + c] = s;
  }
}

// ---- T: slab s of  t_x . W^T + x . V^T  over the split's share of c_in ------------------------------------------
// grid (ceil(c_out / 32), splits); per lane one row of W / V (c_in contiguous) and one row of t_x / x per row tile.
// Order of the additions into one accumulator: k ascending within the wave's steps, per k first t_x*W then x*V.
template <int MT, bool ALIGNED>
__global__ __launch_bounds__(BLOCK) void k_dense_tangent(float* __restrict__ out, const float* __restrict__ tx,
                                                         const float* __restrict__ x, const float* __restrict__ W,
                                                         const float* __restrict__ V, int rows, int c_in, int c_out,
                                                         int ld_x, int kper, long long slab_stride) {
  __shared__ float red[WAVES][1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const int o = blockIdx.x * 32 + j;
  const bool o_ok = o < c_out;
  const int kb = blockIdx.y * kper, ke = min(kb + kper, c_in);
  const float* wrow = W + (size_t)(o_ok ? o : 0) * c_in;
  const float* vrow = V ? V + (size_t)(o_ok ? o : 0) * c_in : nullptr;
  f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[m][q] = 0.0f;
  for (int k0 = kb + 8 * wave; k0 < ke; k0 += DENSE_KSTEP) {
    const int k = k0 + 4 * h;
    Quad w4 = {}, v4 = {};
    if (tx) w4 = ld_quad<ALIGNED>(wrow, k, ke, o_ok);
    if (V) v4 = ld_quad<ALIGNED>(vrow, k, ke, o_ok);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int r = 32 * m + j;
      const bool r_ok = r < rows;
      const size_t ro = (size_t)(r_ok ? r : 0) * ld_x;
      Quad t4 = {}, x4 = {};
      if (tx) t4 = ld_quad<ALIGNED>(tx + ro, k, ke, r_ok);
      if (V) x4 = ld_quad<ALIGNED>(x + ro, k, ke, r_ok);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        if (tx) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(t4.e[s], w4.e[s], acc[m], 0, 0, 0);
        if (V) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(x4.e[s], v4.e[s], acc[m], 0, 0, 0);
      }
    }
  }
  float* slab = out + (long long)blockIdx.y * slab_stride;
#pragma unroll
  for (int m = 0; m < MT; ++m) store_tile_sum(red, acc[m], slab, 32 * m, rows, blockIdx.x * 32, c_out);
}

// ---- D: slab s of  g_a . W  (TWO: + g . V)  over the split's share of c_out -------------------------------------
// grid (ceil(c_in / 32), splits); B[k][j] = W[k][i0 + j]: 128 contiguous bytes per weight row and load, no transposed
// copy.  Order of the additions: k ascending within the wave's steps; TWO (hf_dense_dgrad2_slabs, the Hessian product's
// data gradient): per k first g_a*W, then g*V -- the T kernel's rule.
template <int MT, bool ALIGNED, bool TWO>
__global__ __launch_bounds__(BLOCK) void k_dense_dgrad(float* __restrict__ out, const float* __restrict__ g,
                                                       const float* __restrict__ W, const float* __restrict__ g2,
                                                       const float* __restrict__ V, int rows, int c_in, int c_out,
                                                       int kper, long long slab_stride) {
  __shared__ float red[WAVES][1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const int i = blockIdx.x * 32 + j;
  const bool i_ok = i < c_in;
  const int kb = blockIdx.y * kper, ke = min(kb + kper, c_out);
  f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[m][q] = 0.0f;
  for (int k0 = kb + 8 * wave; k0 < ke; k0 += DENSE_KSTEP) {
    const int k = k0 + 4 * h;
    float w[4], v[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bool ok = i_ok && k + s < ke;
      w[s] = ok ? W[(size_t)(k + s) * c_in + i] : 0.0f;
      if (TWO) v[s] = ok ? V[(size_t)(k + s) * c_in + i] : 0.0f;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int r = 32 * m + j;
      const bool r_ok = r < rows;
      const size_t ro = (size_t)(r_ok ? r : 0) * c_out;
      const Quad g4 = ld_quad<ALIGNED>(g + ro, k, ke, r_ok);
      Quad h4 = {};
      if (TWO) h4 = ld_quad<ALIGNED>(g2 + ro, k, ke, r_ok);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(g4.e[s], w[s], acc[m], 0, 0, 0);
        if (TWO) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(h4.e[s], v[s], acc[m], 0, 0, 0);
      }
    }
  }
  float* slab = out + (long long)blockIdx.y * slab_stride;
#pragma unroll
  for (int m = 0; m < MT; ++m) store_tile_sum(red, acc[m], slab, 32 * m, rows, blockIdx.x * 32, c_in);
}

// ---- W: out[o][i] = scale * sum_r g_a[r][o] * x[r][i], written once ----------------------------------------------
// grid (ceil(c_in / 128), ceil(c_out / 128)); wave w owns output rows o0 + 32 w .. + 31 and 128 columns, lane column j
// holding the four consecutive columns i0 + 4 j + u in accumulators u = 0..3 (one 16-byte store per output row where the
// destination allows it).  The reduction runs over the batch rows in ascending order; `scale` multiplies the finished
// sum (one more rounding).  WGRAD_SQ: both operands are squared after the load (one rounding each) -- the diagonal of the
// empirical Fisher of the layer's weight, sum_r (g_a[r][o] x[r][i])^2, without a per-sample gradient (hf_dense_sq_wgrad).
// WGRAD_TWO: a second pair, sum_r g[r][o] x[r][i] + sum_r g2[r][o] x2[r][i] -- the Hessian product's weight gradient
// (hf_dense_wgrad2): each pair has its own chain over the rows (two independent accumulators: no longer chain than the
// sibling's, and the two MFMA streams do not wait for each other), the chains are added once, then `scale`.
enum { WGRAD_PLAIN = 0, WGRAD_SQ = 1, WGRAD_TWO = 2 };
template <bool ALIGNED, int MODE>
__global__ __launch_bounds__(BLOCK) void k_dense_wgrad(float* __restrict__ out, const float* __restrict__ g,
                                                       const float* __restrict__ x, const float* __restrict__ g2,
                                                       const float* __restrict__ x2, int rows, int c_in, int c_out,
                                                       float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const int o0 = blockIdx.y * 128 + 32 * wave, i0 = blockIdx.x * 128 + 4 * j;
  if (o0 >= c_out) return;  // (no barrier in this kernel)
  const int o = o0 + j;
  const bool o_ok = o < c_out;
  f32x16 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[u][q] = 0.0f;
  constexpr int N2 = MODE == WGRAD_TWO ? 4 : 1;  // (the second pair's accumulators exist in that form only)
  f32x16 acc2[N2];
#pragma unroll
  for (int u = 0; u < N2; ++u)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc2[u][q] = 0.0f;
  for (int r0 = 0; r0 < rows; r0 += 2) {
    const int r = r0 + h;
    const bool r_ok = r < rows;
    float a = (r_ok && o_ok) ? g[(size_t)r * c_out + o] : 0.0f;
    Quad b4 = ld_quad<ALIGNED>(x + (size_t)(r_ok ? r : 0) * c_in, i0, c_in, r_ok);
    if (MODE == WGRAD_SQ) {
      a *= a;
#pragma unroll
      for (int u = 0; u < 4; ++u) b4.e[u] *= b4.e[u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b4.e[u], acc[u], 0, 0, 0);
    if (MODE == WGRAD_TWO) {
      const float a2 = (r_ok && o_ok) ? g2[(size_t)r * c_out + o] : 0.0f;
      const Quad c4 = ld_quad<ALIGNED>(x2 + (size_t)(r_ok ? r : 0) * c_in, i0, c_in, r_ok);
#pragma unroll
      for (int u = 0; u < N2; ++u) acc2[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, c4.e[u], acc2[u], 0, 0, 0);
    }
  }
  if (MODE == WGRAD_TWO) {
#pragma unroll
    for (int u = 0; u < N2; ++u)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[u][q] += acc2[u][q];
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int oo = o0 + (q & 3) + 8 * (q >> 2) + 4 * h;
    if (oo >= c_out) continue;
    float* dst = out + (size_t)oo * c_in + i0;
    if (ALIGNED && i0 + 4 <= c_in) {
      F4 v;
#pragma unroll
      for (int u = 0; u < 4; ++u) v.e[u] = acc[u][q] * scale;
      *reinterpret_cast<F4*>(dst) = v;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u < c_in) dst[u] = acc[u][q] * scale;
    }
  }
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

// g_a = (sum of slabs) * act'(y);  g_b[col] = scale * sum_rows g_a -- one thread per column walks the rows in order,
// the column sum is kept in fp64 and rounded to fp32 once, then multiplied by `scale`.
// CURV (hf_dense_act_adjoint2 with tanh; the adjoint of the Hessian product, where act' itself has a tangent):
// g_a = fmaf((-2 y) * t_y, h, (sum of slabs) * act'(y)) -- t_y is the layer's tangent OUTPUT (it carries 1 - y*y), h the
// first-order cotangent of the layer's output, so act'' is never formed: the doubling is exact, then one rounding for
// the product with t_y and one for the fused multiply-add.
constexpr int ADJ_BLOCK = 64;
template <bool CURV>
__global__ __launch_bounds__(ADJ_BLOCK) void k_dense_act_adjoint(float* __restrict__ ga, float* __restrict__ gb,
                                                                 const float* __restrict__ slabs, int splits,
                                                                 long long stride, const float* __restrict__ y, int act,
                                                                 const float* __restrict__ ty, const float* __restrict__ h1,
                                                                 int rows, int c, float scale) {
  const int col = blockIdx.x * ADJ_BLOCK + threadIdx.x;
  if (col >= c) return;
  double sum = 0.0;
  for (int r = 0; r < rows; ++r) {
    const int idx = r * c + col;
    const float s = slab_sum<4>(slabs[idx], slabs, idx, splits, stride);
    float gv = act_apply(s, y, idx, act);
    if (CURV) gv = fmaf((-2.0f * y[idx]) * ty[idx], h1[idx], gv);
    ga[idx] = gv;
    sum += (double)gv;
  }
  if (gb) gb[col] = (float)sum * scale;
}

// out[col] = scale * sum_rows g_a^2 -- the rule of k_dense_act_adjoint's bias sum: one thread per column walks the rows in
// order, the squares (exact in fp64) are summed in fp64, the sum is rounded to fp32 once, then multiplied by `scale`.
__global__ __launch_bounds__(ADJ_BLOCK) void k_dense_sq_colsum(float* __restrict__ out, const float* __restrict__ ga,
                                                               int rows, int c, float scale) {
  const int col = blockIdx.x * ADJ_BLOCK + threadIdx.x;
  if (col >= c) return;
  double sum = 0.0;
  for (int r = 0; r < rows; ++r) {
    const double gv = (double)ga[(size_t)r * c + col];
    sum += gv * gv;
  }
  out[col] = (float)sum * scale;
}

inline bool act_args_ok(const void* slabs, int splits, int64_t slab_stride, const void* y, int act, int64_t rows,
                        int64_t c, int dtype) {
  if (dtype != HF_F32 || !slabs) return false;
  if (rows < 1 || rows > DENSE_MAX_ROWS || c < 1 || c > DENSE_MAX_C) return false;
  if (splits < 1 || splits > DENSE_MAX_SPLITS) return false;
  if (splits > 1 && slab_stride < rows * c) return false;
  if (act < ACT_IDENTITY || act > ACT_TANH) return false;
  if (act != ACT_IDENTITY && !y) return false;
  return true;
}

// the curvature term's operands: tanh needs the tangent output and the first-order cotangent (act'' = 0 otherwise)
inline bool act_curv_args_ok(int act, const void* t_y, const void* h) { return act != ACT_TANH || (t_y && h); }

// hf_dense_act_adjoint (second = false) and hf_dense_act_adjoint2: one validator sequence, one launch.  Identity and relu
// have no curvature term: they take the sibling's instantiation, which never sees t_y / h.
int dense_act_adjoint_launch(bool second, void* g_a, void* g_b_out, const void* slabs, int splits, int64_t slab_stride,
                             const void* y, int act, const void* t_y, const void* h, int64_t rows, int64_t c,
                             double scale, int dtype, void* stream) {
  if (!g_a || !act_args_ok(slabs, splits, slab_stride, y, act, rows, c, dtype)) return HF_ERR_ARG;
  if (second && !act_curv_args_ok(act, t_y, h)) return HF_ERR_ARG;
  if (!(scale == scale)) return HF_ERR_ARG;
  const unsigned grid = (unsigned)((c + ADJ_BLOCK - 1) / ADJ_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  if (second && act == ACT_TANH)
    k_dense_act_adjoint<true><<<grid, ADJ_BLOCK, 0, st>>>((float*)g_a, (float*)g_b_out, (const float*)slabs, splits,
                                                          (long long)slab_stride, (const float*)y, act, (const float*)t_y,
                                                          (const float*)h, (int)rows, (int)c, (float)scale);
  else
    k_dense_act_adjoint<false><<<grid, ADJ_BLOCK, 0, st>>>((float*)g_a, (float*)g_b_out, (const float*)slabs, splits,
                                                           (long long)slab_stride, (const float*)y, act, nullptr, nullptr,
                                                           (int)rows, (int)c, (float)scale);
  return (int)hipGetLastError();
}

// hf_dense_wgrad (WGRAD_PLAIN), hf_dense_sq_wgrad (WGRAD_SQ) and hf_dense_wgrad2 (WGRAD_TWO): one validator, one launch
template <int MODE>
int dense_wgrad_launch(void* out, const void* g_a, const void* x, const void* g2, const void* x2, int64_t rows,
                       int64_t c_in, int64_t c_out, double scale, int dtype, void* stream) {
  DensePlan p;
  if (dense_plan(rows, c_in, c_out, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out || !g_a || !x) return HF_ERR_ARG;
  if (MODE == WGRAD_TWO && (!g2 || !x2)) return HF_ERR_ARG;
  if (!(scale == scale)) return HF_ERR_ARG;
  const bool al = quad_ok(out, c_in) && quad_ok(x, c_in) && (MODE != WGRAD_TWO || quad_ok(x2, c_in));
  const dim3 grid((unsigned)((c_in + 127) / 128), (unsigned)((c_out + 127) / 128));
  hipStream_t st = (hipStream_t)stream;
  if (al)
    k_dense_wgrad<true, MODE><<<grid, BLOCK, 0, st>>>((float*)out, (const float*)g_a, (const float*)x, (const float*)g2,
                                                      (const float*)x2, (int)rows, (int)c_in, (int)c_out, (float)scale);
  else
    k_dense_wgrad<false, MODE><<<grid, BLOCK, 0, st>>>((float*)out, (const float*)g_a, (const float*)x, (const float*)g2,
                                                       (const float*)x2, (int)rows, (int)c_in, (int)c_out, (float)scale);
  return (int)hipGetLastError();
}

#define DENSE_MT_SWITCH(mt, CALL) \
  switch (mt) {                   \
    case 1: CALL(1); break;       \
    case 2: CALL(2); break;       \
    case 3: CALL(3); break;       \
    case 4: CALL(4); break;       \
    case 5: CALL(5); break;       \
    case 6: CALL(6); break;       \
    case 7: CALL(7); break;       \
    default: CALL(8); break;      \
  }

// hf_dense_dgrad_slabs (TWO = false) and hf_dense_dgrad2_slabs (TWO = true): one validator, one launch
template <bool TWO>
int dense_dgrad_launch(void* out_slabs, const void* g_a, const void* W, const void* g, const void* V, int64_t rows,
                       int64_t c_in, int64_t c_out, int splits, int64_t slab_stride, int dtype, void* stream) {
  DensePlan p;
  if (dense_plan(rows, c_in, c_out, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out_slabs || !g_a || !W) return HF_ERR_ARG;
  if (TWO && (!g || !V)) return HF_ERR_ARG;
  if (!dense_split_ok(c_out, splits)) return HF_ERR_ARG;
  if (splits > 1 && slab_stride < rows * c_in) return HF_ERR_ARG;
  const bool al = quad_ok(g_a, c_out) && (!TWO || quad_ok(g, c_out));
  const int mt = (int)((rows + 31) / 32), kper = (int)dense_kper(c_out, splits);
  const dim3 grid((unsigned)((c_in + 31) / 32), (unsigned)splits);
  hipStream_t st = (hipStream_t)stream;
#define CALL_D(MT)                                                                                                     \
  do {                                                                                                                 \
    if (al)                                                                                                            \
      k_dense_dgrad<MT, true, TWO><<<grid, BLOCK, 0, st>>>((float*)out_slabs, (const float*)g_a, (const float*)W,      \
                                                           (const float*)g, (const float*)V, (int)rows, (int)c_in,     \
                                                           (int)c_out, kper, (long long)slab_stride);                  \
    else                                                                                                               \
      k_dense_dgrad<MT, false, TWO><<<grid, BLOCK, 0, st>>>((float*)out_slabs, (const float*)g_a, (const float*)W,     \
                                                            (const float*)g, (const float*)V, (int)rows, (int)c_in,    \
                                                            (int)c_out, kper, (long long)slab_stride);                 \
  } while (0)
  DENSE_MT_SWITCH(mt, CALL_D)
#undef CALL_D
  return (int)hipGetLastError();
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

// ---- the loss head on logits [rows, c] --------------------------------------------------------------------------------
enum { LOSS_CE = 0, LOSS_MSE = 1 };
constexpr int LOSS_CE_MAX_C = 1024;          // 4 columns per thread of one workgroup
constexpr int LOSS_WORK_DOUBLES = 512;       // the workspace: row terms + row marks (ce), block partials (mse)

// max over the workgroup, the same value in every thread
__device__ __forceinline__ float block_max(float v, float* lds /*WAVES*/) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  float m = lds[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) m = fmaxf(m, lds[w]);
  __syncthreads();
  return m;
}

// One workgroup per row: m = row maximum; e = expf(x - m); S = sum of the e in fp64 (per thread its columns ascending,
// then the fixed tree of block_allreduce); p = e / (float)S; d = p - onehot (rounded), dl = d * scale_g (rounded),
// dl_ps = d * scale_ps (rounded).  The row's loss term log(S) - (x[t] - m) in fp64 goes to work[r], its mark (target
// outside [0, c): no one in onehot, term 0) to work[rows + r].
__global__ __launch_bounds__(BLOCK) void k_dense_ce_rows(const float* __restrict__ logits,
                                                         const long long* __restrict__ targets, float* __restrict__ p,
                                                         float* __restrict__ dl, float* __restrict__ dl_ps,
                                                         double* __restrict__ work, float scale_g, float scale_ps,
                                                         int rows, int c) {
  __shared__ float lds_m[WAVES];
  __shared__ double lds_s[WAVES];
  const int r = blockIdx.x;
  const float* x = logits + (size_t)r * c;
  float xv[4], m = -INFINITY;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = threadIdx.x + BLOCK * u;
    xv[u] = col < c ? x[col] : -INFINITY;
    m = fmaxf(m, xv[u]);
  }
  m = block_max(m, lds_m);
  float e[4];
  double part[1] = {0.0};
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = threadIdx.x + BLOCK * u;
    e[u] = col < c ? expf(xv[u] - m) : 0.0f;
    part[0] += (double)e[u];
  }
  block_allreduce<1>(part, lds_s);
  const float sf = (float)part[0];
  const long long t = targets[r];
  const bool ok = t >= 0 && t < (long long)c;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int col = threadIdx.x + BLOCK * u;
    if (col >= c) continue;
    const size_t idx = (size_t)r * c + col;
    const float pv = e[u] / sf;
    const float d = pv - ((ok && (long long)col == t) ? 1.0f : 0.0f);
    p[idx] = pv;
    dl[idx] = d * scale_g;
    if (dl_ps) dl_ps[idx] = d * scale_ps;
  }
  if (threadIdx.x == 0) {
    work[r] = ok ? log(part[0]) - ((double)x[t] - (double)m) : 0.0;
    work[rows + r] = ok ? 0.0 : 1.0;
  }
}

// d = out - t (rounded), dl = d * scale_g, dl_ps = d * scale_ps; the squares d*d (exact in fp64) are summed in fp64: per
// thread over its grid-stride elements in ascending order, then the fixed tree of block_allreduce -> work[block].
__global__ __launch_bounds__(BLOCK) void k_dense_mse_part(const float* __restrict__ out, const float* __restrict__ tg,
                                                          float* __restrict__ dl, float* __restrict__ dl_ps,
                                                          double* __restrict__ work, float scale_g, float scale_ps,
                                                          long long total) {
  __shared__ double lds_s[WAVES];
  double part[1] = {0.0};
  const long long step = (long long)gridDim.x * BLOCK;
  for (long long idx = (long long)blockIdx.x * BLOCK + threadIdx.x; idx < total; idx += step) {
    const float d = out[idx] - tg[idx];
    dl[idx] = d * scale_g;
    if (dl_ps) dl_ps[idx] = d * scale_ps;
    part[0] += (double)d * (double)d;
  }
  block_allreduce<1>(part, lds_s);
  if (threadIdx.x == 0) work[blockIdx.x] = part[0];
}

// The loss value and the flag: one thread adds work[0 .. n-1] in ascending order in fp64.  ce: loss = (float)(sum * coef),
// flag = some row mark work[n .. 2n-1] is set; mse: loss = (float)sum * (float)coef, flag = 0.
__global__ __launch_bounds__(BLOCK) void k_dense_loss_finish(const double* __restrict__ work, int n, int kind, double coef,
                                                             float* __restrict__ loss, int* __restrict__ flag) {
  __shared__ double terms[LOSS_WORK_DOUBLES];
  const int have = kind == LOSS_CE ? 2 * n : n;
  for (int i = threadIdx.x; i < have; i += BLOCK) terms[i] = work[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int i = 0; i < n; ++i) sum += terms[i];
  int bad = 0;
  if (kind == LOSS_CE) {
    for (int i = n; i < 2 * n; ++i) bad |= terms[i] != 0.0;
    *loss = (float)(sum * coef);
  } else {
    *loss = (float)sum * (float)coef;
  }
  *flag = bad;
}

// workgroups of the mse pass: 1024 elements each at first, at most LOSS_WORK_DOUBLES
inline int mse_blocks(int64_t total) {
  const int64_t g = (total + 4 * BLOCK - 1) / (4 * BLOCK);
  return (int)(g < 1 ? 1 : g > LOSS_WORK_DOUBLES ? LOSS_WORK_DOUBLES : g);
}

}  // namespace

extern "C" {

int hf_dense_plan(int64_t rows, int64_t c_in, int64_t c_out, int* splits_t, int* splits_d) {
  DensePlan p;
  if (!splits_t || !splits_d) return HF_ERR_ARG;
  const int rc = dense_plan(rows, c_in, c_out, &p);
  if (rc != HF_OK) return rc;
  *splits_t = p.splits_t;
  *splits_d = p.splits_d;
  return HF_OK;
}

int hf_dense_tangent_slabs(void* out_slabs, const void* t_x, const void* x, const void* W, const void* V, int64_t rows,
                           int64_t c_in, int64_t c_out, int64_t ld_x, int splits, int64_t slab_stride, int dtype,
                           void* stream) {
  DensePlan p;
  if (dense_plan(rows, c_in, c_out, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out_slabs) return HF_ERR_ARG;
  if (!t_x && !V) return HF_ERR_ARG;           // nothing to compute
  if ((t_x && !W) || (V && !x)) return HF_ERR_ARG;
  if (ld_x == 0) ld_x = c_in;
  if (ld_x < c_in || ld_x > DENSE_MAX_C) return HF_ERR_ARG;
  if (!dense_split_ok(c_in, splits)) return HF_ERR_ARG;
  if (splits > 1 && slab_stride < rows * c_out) return HF_ERR_ARG;
  const bool al = (!t_x || (quad_ok(t_x, ld_x) && quad_ok(W, c_in))) && (!V || (quad_ok(x, ld_x) && quad_ok(V, c_in)));
  const int mt = (int)((rows + 31) / 32), kper = (int)dense_kper(c_in, splits);
  const dim3 grid((unsigned)((c_out + 31) / 32), (unsigned)splits);
  hipStream_t st = (hipStream_t)stream;
#define CALL_T(MT)                                                                                                     \
  do {                                                                                                                 \
    if (al)                                                                                                            \
      k_dense_tangent<MT, true><<<grid, BLOCK, 0, st>>>((float*)out_slabs, (const float*)t_x, (const float*)x,         \
                                                        (const float*)W, (const float*)V, (int)rows, (int)c_in,        \
                                                        (int)c_out, (int)ld_x, kper, (long long)slab_stride);          \
    else                                                                                                               \
      k_dense_tangent<MT, false><<<grid, BLOCK, 0, st>>>((float*)out_slabs, (const float*)t_x, (const float*)x,        \
                                                         (const float*)W, (const float*)V, (int)rows, (int)c_in,       \
                                                         (int)c_out, (int)ld_x, kper, (long long)slab_stride);         \
  } while (0)
  DENSE_MT_SWITCH(mt, CALL_T)
#undef CALL_T
  return (int)hipGetLastError();
}

int hf_dense_dgrad_slabs(void* out_slabs, const void* g_a, const void* W, int64_t rows, int64_t c_in, int64_t c_out,
                         int splits, int64_t slab_stride, int dtype, void* stream) {
  return dense_dgrad_launch<false>(out_slabs, g_a, W, nullptr, nullptr, rows, c_in, c_out, splits, slab_stride, dtype,
                                   stream);
}

int hf_dense_dgrad2_slabs(void* out_slabs, const void* g_a, const void* W, const void* g, const void* V, int64_t rows,
                          int64_t c_in, int64_t c_out, int splits, int64_t slab_stride, int dtype, void* stream) {
  return dense_dgrad_launch<true>(out_slabs, g_a, W, g, V, rows, c_in, c_out, splits, slab_stride, dtype, stream);
}

int hf_dense_wgrad(void* out, const void* g_a, const void* x, int64_t rows, int64_t c_in, int64_t c_out, double scale,
                   int dtype, void* stream) {
  return dense_wgrad_launch<WGRAD_PLAIN>(out, g_a, x, nullptr, nullptr, rows, c_in, c_out, scale, dtype, stream);
}

int hf_dense_sq_wgrad(void* out, const void* g_a, const void* x, int64_t rows, int64_t c_in, int64_t c_out, double scale,
                      int dtype, void* stream) {
  return dense_wgrad_launch<WGRAD_SQ>(out, g_a, x, nullptr, nullptr, rows, c_in, c_out, scale, dtype, stream);
}

int hf_dense_wgrad2(void* out, const void* g1, const void* x1, const void* g2, const void* x2, int64_t rows, int64_t c_in,
                    int64_t c_out, double scale, int dtype, void* stream) {
  return dense_wgrad_launch<WGRAD_TWO>(out, g1, x1, g2, x2, rows, c_in, c_out, scale, dtype, stream);
}

int hf_dense_sq_colsum(void* out, const void* g_a, int64_t rows, int64_t c, double scale, int dtype, void* stream) {
  if (!dense_dims_ok(rows, c, c)) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out || !g_a) return HF_ERR_ARG;
  if (!(scale == scale)) return HF_ERR_ARG;
  k_dense_sq_colsum<<<(unsigned)((c + ADJ_BLOCK - 1) / ADJ_BLOCK), ADJ_BLOCK, 0, (hipStream_t)stream>>>(
      (float*)out, (const float*)g_a, (int)rows, (int)c, (float)scale);
  return (int)hipGetLastError();
}

int hf_dense_act_tangent(void* t_y, const void* slabs, int splits, int64_t slab_stride, const void* v_b, const void* y,
                         int act, int64_t rows, int64_t c, int dtype, void* stream) {
  if (!t_y || !act_args_ok(slabs, splits, slab_stride, y, act, rows, c, dtype)) return HF_ERR_ARG;
  const int total = (int)(rows * c);
  k_dense_act_tangent<<<(total + BLOCK - 1) / BLOCK, BLOCK, 0, (hipStream_t)stream>>>(
      (float*)t_y, (const float*)slabs, splits, (long long)slab_stride, (const float*)v_b, (const float*)y, act, total,
      (int)c);
  return (int)hipGetLastError();
}

int hf_dense_act_adjoint(void* g_a, void* g_b_out, const void* slabs, int splits, int64_t slab_stride, const void* y,
                         int act, int64_t rows, int64_t c, double scale, int dtype, void* stream) {
  return dense_act_adjoint_launch(false, g_a, g_b_out, slabs, splits, slab_stride, y, act, nullptr, nullptr, rows, c,
                                  scale, dtype, stream);
}

int hf_dense_act_adjoint2(void* g_a, void* g_b_out, const void* slabs, int splits, int64_t slab_stride, const void* y,
                          int act, const void* t_y, const void* h, int64_t rows, int64_t c, double scale, int dtype,
                          void* stream) {
  return dense_act_adjoint_launch(true, g_a, g_b_out, slabs, splits, slab_stride, y, act, t_y, h, rows, c, scale, dtype,
                                  stream);
}

int hf_dense_act_forward(void* y, const void* slabs, int splits, int64_t slab_stride, const void* b, int act,
                         int64_t rows, int64_t c, int dtype, void* stream) {
  if (!y || !act_args_ok(slabs, splits, slab_stride, y, act, rows, c, dtype)) return HF_ERR_ARG;
  const int total = (int)(rows * c);
  k_dense_act_forward<<<(total + BLOCK - 1) / BLOCK, BLOCK, 0, (hipStream_t)stream>>>(
      (float*)y, (const float*)slabs, splits, (long long)slab_stride, (const float*)b, act, total, (int)c);
  return (int)hipGetLastError();
}

int hf_dense_loss_head(int kind, const void* logits, const void* targets, void* p, void* dl, void* dl_ps, void* loss,
                       void* flag, void* work, double scale_g, double scale_ps, double coef, int64_t rows, int64_t c,
                       int dtype, void* stream) {
  if (dtype != HF_F32 || (kind != LOSS_CE && kind != LOSS_MSE)) return HF_ERR_ARG;
  if (!logits || !targets || !dl || !loss || !flag || !work || (kind == LOSS_CE && !p)) return HF_ERR_ARG;
  if ((((uintptr_t)work) & 7) != 0 || (kind == LOSS_CE && (((uintptr_t)targets) & 7) != 0)) return HF_ERR_ARG;
  if (rows < 1 || rows > DENSE_MAX_ROWS || c < 1 || c > (kind == LOSS_CE ? (int64_t)LOSS_CE_MAX_C : DENSE_MAX_C))
    return HF_ERR_ARG;
  if (!(scale_g == scale_g) || !(scale_ps == scale_ps) || !(coef == coef)) return HF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  int n;
  if (kind == LOSS_CE) {
    n = (int)rows;
    k_dense_ce_rows<<<(unsigned)rows, BLOCK, 0, st>>>((const float*)logits, (const long long*)targets, (float*)p,
                                                      (float*)dl, (float*)dl_ps, (double*)work, (float)scale_g,
                                                      (float)scale_ps, (int)rows, (int)c);
  } else {
    n = mse_blocks(rows * c);
    k_dense_mse_part<<<(unsigned)n, BLOCK, 0, st>>>((const float*)logits, (const float*)targets, (float*)dl,
                                                    (float*)dl_ps, (double*)work, (float)scale_g, (float)scale_ps,
                                                    (long long)(rows * c));
  }
  HF_HIP(hipGetLastError());
  k_dense_loss_finish<<<1, BLOCK, 0, st>>>((const double*)work, n, kind, coef, (float*)loss, (int*)flag);
  return (int)hipGetLastError();
}

}  // extern "C"
