// hf_ln.hip -- LayerNorm layers of the dense-stack engine (engine/linear.py): Linear(+bias) -> LayerNorm(affine) ->
// [ReLU | Tanh] as ONE layer of the dense chain.  Forward, tangent and adjoint of the normalisation are one launch each,
// the parameter sums (scale, shift, the Linear's bias -- or their squares, for the diagonal empirical Fisher) one more.
// fp32, wave64, activations [rows <= 256, c <= 16 384], statistics per ROW.  Plain C++/HIP, no atomics, no cooperative
// launch: every order depends on the shape alone, two launches on the same operands agree bitwise.
//
// Why a design of its own.  The dense chain's elementwise passes (hf_dense_act.h) own one ELEMENT per thread and its
// adjoint one COLUMN per thread: neither sees a row.  A LayerNorm statistic belongs to one row of c features -- the
// ownership hf_gn.hip gives a (sample, group) block: one owner sums the split-K slabs of its row once, keeps the row on
// chip and takes every reduction from it.  A row is read from HBM once per launch and never re-read.
//
// Work split (row kernels), chosen on the host by c; a row's features are taken as nq = ceil(c / 4) QUADS, quad q the
// columns 4q .. 4q+3:
//   wave per row, c <= 1024.  Four rows per 256-thread workgroup, row = 4 * block + wave.  Lane l owns the quads
//     l, l + 64, l + 128, l + 192 (instantiations for 1, 2 and 4 quads per lane) and keeps them in REGISTERS: no LDS,
//     no barrier; a wave whose row does not exist leaves at once.
//   workgroup per row, 1024 < c <= 16 384.  Thread t owns the quads t, t + 256, .. (at most 16) and stages what it
//     summed in LDS (one tile of 16 384 floats for the forward pass, two -- the summed operand and x_hat / y's factor --
//     for tangent and adjoint: 128 KB of gfx950's 160 KB); per-wave partials are combined through LDS in wave order.
// Loads: c % 4 == 0 takes 16-byte loads and stores of the row maps (which then must sit on the 16-byte grid:
// HF_ERR_ALIGN otherwise), any other c element loads, predicated on the column; per-column vectors (the biases, gamma,
// beta and the CG vector's slices) sit on any 4-byte boundary of a flat vector and are read element by element.
//
// Reductions (the means of a row).  A lane keeps FOUR fp32 partial sums, one per column of its quads, each a chain over
// its quads in ascending order: L = ceil(nq / 64) <= 4 terms (wave form), ceil(nq / 256) <= 16 terms (workgroup form).
// Everything behind that is fp64: the four partials are added ((s0 + s1) + s2) + s3, the 64 lanes of a wave by an xor
// butterfly (offsets 32 .. 1: every lane holds the same bits), the four waves of the workgroup form in wave order.  The
// two means of the tangent and the two of the adjoint are taken in ONE round.
//
// Arithmetic chains (one fp32 rounding per named step unless it says fp64; -ffp-contract=off: no step is fused)
//   sum      = slab 0 + slab 1 + .. (split order: hf_common.h's slab_sum)                 splits - 1 roundings
// hf_ln_act_forward
//   a        = sum [+ b[col]]                                                            [1]
//   mu       = fp32( fp64 sum of the lanes' chains of a / c )                             chain, then ONE rounding
//   d        = a - mu;  the lanes' chains of d * d                                        (exact two-pass variance)
//   rstd     = fp32( 1 / sqrt( fp64 sum / c + eps ) )                                     all fp64, ONE rounding
//   xh       = d * rstd                                                                   1 behind d, rstd
//   r        = gamma[col] * xh + beta[col]                                                2
//   y        = r (identity) | r <= 0 ? +0 : r (relu: a NaN stays a NaN) | tanhf(r)
// hf_ln_act_tangent  (xh, rstd, y: the forward launch's, as given)
//   t        = sum [+ v_b[col]]                                                           [1]
//   m1       = fp32( fp64 sum of the chains of t / c );  mx = fp32( .. of the chains of xh * t .. )
//   tx       = rstd * ((t - m1) - xh * mx)                                                4 behind t, m1, mx
//   r        = gamma[col] * tx  (1)  [+ v_gamma[col] * xh  (2)]  [+ v_beta[col]  (1)]
//   t_y      = act_apply(r, y): r | y > 0 ? r : 0 | r * (1 - y * y)  (3)                   hf_dense_act.h
// hf_ln_act_adjoint
//   s        = act_apply(sum, y)                                                          0 | 0 | 3
//   q        = gamma[col] * s                                                             1
//   m1       = fp32( fp64 sum of the chains of q / c );  mx = fp32( .. of the chains of q * xh .. )
//   g_a      = rstd * ((q - m1) - xh * mx)                                                4 behind q, m1, mx
// hf_ln_param_sums  (s, xh, g_a as given; one thread per column, consecutive threads consecutive columns; wave w of the
//                    workgroup takes the rows w * ceil(rows / 4) .. in ascending order, the waves are added in wave order:
//                    the rows in row order, all in fp64)
//   o_gamma  = fp32( fp64 sum_r fp32(s * xh) ) * scale                                    1 + 1 + 1
//   o_beta   = fp32( fp64 sum_r s ) * scale;   o_b = fp32( fp64 sum_r g_a ) * scale       1 + 1
//   squared  : the terms fp32(s * xh)^2, s^2, g_a^2 -- the squares exact in fp64 -- instead
#include "hf_dense_act.h"

#include <math.h>

#include <initializer_list>

namespace {

constexpr int LN_MAX_ROWS = 256;   // the skinny dense chain's
constexpr int LN_WAVE_C = 1024;    // wave form: four quads per lane
constexpr int LN_MAX_C = 16384;    // workgroup form: the LDS tile (hf_gn.hip's block limit)
constexpr int LN_COLS = 64;        // columns of one workgroup of the column kernel

// ---- what a thread owns ------------------------------------------------------------------------------------------------
// NJ > 0: the wave form with NJ quads per lane; NJ == 0: the workgroup form (a run-time count of quads per thread)
struct LnGeo {
  int row, lt, nq, nj;
  long long base;  // float index of the row's first column in a dense [rows, c] map
};

template <int NJ>
__device__ __forceinline__ LnGeo ln_geo(int c) {
  LnGeo g;
  g.nq = (c + 3) >> 2;
  if (NJ) {
    g.row = blockIdx.x * WAVES + (threadIdx.x >> 6);
    g.lt = threadIdx.x & 63;
    g.nj = NJ;
  } else {
    g.row = blockIdx.x;
    g.lt = threadIdx.x;
    g.nj = (g.nq + BLOCK - 1) / BLOCK;
  }
  g.base = (long long)g.row * c;
  return g;
}

// the thread's quads of one row-sized operand: registers (wave form) or its own places of an LDS tile
template <int NJ>
struct LnRow {
  F4 v[NJ];
  __device__ __forceinline__ explicit LnRow(F4*) {}
  __device__ __forceinline__ F4 get(int j) const { return v[j]; }
  __device__ __forceinline__ void set(int j, const F4& x) { v[j] = x; }
};
template <>
struct LnRow<0> {
  F4* t;
  __device__ __forceinline__ explicit LnRow(F4* tile) : t(tile) {}
  __device__ __forceinline__ F4 get(int j) const { return t[threadIdx.x + BLOCK * j]; }
  __device__ __forceinline__ void set(int j, const F4& x) { t[threadIdx.x + BLOCK * j] = x; }
};

#define LN_T (NJ ? 64 : BLOCK)
#define LN_FOR_QUADS _Pragma("unroll NJ ? NJ : 4") for (int j = 0; j < (NJ ? NJ : g.nj); ++j)
#define LN_ZERO (F4{{0.f, 0.f, 0.f, 0.f}})

// column 4q + k of the row exists (VEC: whole quads)
template <bool VEC>
__device__ __forceinline__ bool ln_on(int q, int k, int nq, int c) { return VEC ? q < nq : 4 * q + k < c; }

// quad q of a per-column vector; zeros behind the row's end
__device__ __forceinline__ F4 ln_cols(const float* __restrict__ p, int q, int c) {
  F4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v.e[k] = 4 * q + k < c ? p[4 * q + k] : 0.f;
  return v;
}

// quad q of a row of a dense map (`row`: its first column); zeros behind the row's end
template <bool VEC>
__device__ __forceinline__ F4 ln_map(const float* __restrict__ row, int q, int nq, int c) {
  if (VEC) return q < nq ? ld4(row + 4 * q) : LN_ZERO;
  return ln_cols(row, q, c);
}

// the same of the sum of `splits` slabs
template <bool VEC>
__device__ __forceinline__ F4 ln_slabs(const float* __restrict__ slabs, long long base, int q, int nq, int c, int splits,
                                       long long stride) {
  F4 v = LN_ZERO;
  if (VEC) {
    const long long off = base + 4 * q;
    if (q < nq) v = slab_sum<4>(ld4(slabs + off), slabs, off, splits, stride);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long off = base + 4 * q + k;
      if (4 * q + k < c) v.e[k] = slab_sum<4>(slabs[off], slabs, off, splits, stride);
    }
  }
  return v;
}

template <bool VEC>
__device__ __forceinline__ void ln_store(float* __restrict__ row, int q, int nq, int c, const F4& v) {
  if (VEC) {
    if (q < nq) chain_store4<HF_WT_ELEM != 0>(row + 4 * q, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * q + k < c) chain_store<HF_WT_ELEM != 0>(row + 4 * q + k, v.e[k]);
  }
}

__device__ __forceinline__ double ln_quad_sum(const F4& s) {
  return (((double)s.e[0] + (double)s.e[1]) + (double)s.e[2]) + (double)s.e[3];
}

// the row's sums in every lane of its owner: the butterfly over a wave; workgroup form: the waves in wave order
template <int K, int NJ>
__device__ __forceinline__ void ln_row_sum(double (&v)[K], double* red /*K * WAVES*/) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  }
  if (NJ == 0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) red[k * WAVES + wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = red[k * WAVES];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) s += red[k * WAVES + w];
      v[k] = s;
    }
    __syncthreads();
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------
template <int NJ, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_ln_forward(float* __restrict__ y, float* __restrict__ xh_out,
                                                      float* __restrict__ rstd_out, const float* __restrict__ slabs,
                                                      int splits, long long stride, const float* __restrict__ b,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      double eps, int act, int rows, int c) {
  __shared__ F4 tile[NJ ? 1 : LN_MAX_C / 4];
  __shared__ double red[WAVES];
  const LnGeo g = ln_geo<NJ>(c);
  if (g.row >= rows) return;  // (wave form only: a whole wave, and no barrier follows)
  LnRow<NJ> a(tile);
  F4 p = LN_ZERO;
  LN_FOR_QUADS {
    const int q = g.lt + LN_T * j;
    F4 v = ln_slabs<VEC>(slabs, g.base, q, g.nq, c, splits, stride);
    if (b) {
      const F4 bb = ln_cols(b, q, c);
#pragma unroll
      for (int k = 0; k < 4; ++k) v.e[k] += bb.e[k];
    }
    a.set(j, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) p.e[k] += v.e[k];
  }
  double m[1] = {ln_quad_sum(p)};
  ln_row_sum<1, NJ>(m, red);
  const float mu = (float)(m[0] / (double)c);
  p = LN_ZERO;
  LN_FOR_QUADS {
    const int q = g.lt + LN_T * j;
    const F4 v = a.get(j);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float d = ln_on<VEC>(q, k, g.nq, c) ? v.e[k] - mu : 0.f;
      p.e[k] += d * d;
    }
  }
  m[0] = ln_quad_sum(p);
  ln_row_sum<1, NJ>(m, red);
  const float rs = (float)(1.0 / sqrt(m[0] / (double)c + eps));
  LN_FOR_QUADS {
    const int q = g.lt + LN_T * j;
    if (q >= g.nq) continue;
    const F4 v = a.get(j), ga = ln_cols(gamma, q, c), be = ln_cols(beta, q, c);
    F4 xo, yo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xv = (v.e[k] - mu) * rs;
      float r = ga.e[k] * xv + be.e[k];
      if (act == ACT_RELU) r = r <= 0.0f ? 0.0f : r;
      if (act == ACT_TANH) r = tanhf(r);
      xo.e[k] = xv;
      yo.e[k] = r;
    }
    ln_store<VEC>(xh_out + g.base, q, g.nq, c, xo);
    ln_store<VEC>(y + g.base, q, g.nq, c, yo);
  }
  if (g.lt == 0) rstd_out[g.row] = rs;
}

// ---- tangent -------------------------------------------------------------------------------------------------------------
template <int NJ, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_ln_tangent(float* __restrict__ ty, const float* __restrict__ slabs, int splits,
                                                      long long stride, const float* __restrict__ vb,
                                                      const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma, const float* __restrict__ vgamma,
                                                      const float* __restrict__ vbeta, const float* __restrict__ y, int act,
                                                      int rows, int c) {
  __shared__ F4 tile_t[NJ ? 1 : LN_MAX_C / 4], tile_x[NJ ? 1 : LN_MAX_C / 4];
  __shared__ double red[2 * WAVES];
  const LnGeo g = ln_geo<NJ>(c);
  if (g.row >= rows) return;
  LnRow<NJ> t(tile_t), xh(tile_x);
  F4 p1 = LN_ZERO, p2 = LN_ZERO;
  LN_FOR_QUADS {
    const int q = g.lt + LN_T * j;
    F4 v = ln_slabs<VEC>(slabs, g.base, q, g.nq, c, splits, stride);
    if (vb) {
      const F4 bb = ln_cols(vb, q, c);
#pragma unroll
      for (int k = 0; k < 4; ++k) v.e[k] += bb.e[k];
    }
    const F4 x = ln_map<VEC>(xhat + g.base, q, g.nq, c);
    t.set(j, v);
    xh.set(j, x);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p1.e[k] += v.e[k];
      p2.e[k] += x.e[k] * v.e[k];
    }
  }
  double m[2] = {ln_quad_sum(p1), ln_quad_sum(p2)};
  ln_row_sum<2, NJ>(m, red);
  const float m1 = (float)(m[0] / (double)c), mx = (float)(m[1] / (double)c), rs = rstd[g.row];
  LN_FOR_QUADS {
    const int q = g.lt + LN_T * j;
    if (q >= g.nq) continue;
    const F4 v = t.get(j), x = xh.get(j), ga = ln_cols(gamma, q, c);
    const F4 yq = act != ACT_IDENTITY ? ln_map<VEC>(y + g.base, q, g.nq, c) : LN_ZERO;
    const F4 vg = vgamma ? ln_cols(vgamma, q, c) : LN_ZERO, vbe = vbeta ? ln_cols(vbeta, q, c) : LN_ZERO;
    F4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float tx = rs * ((v.e[k] - m1) - x.e[k] * mx);
      float r = ga.e[k] * tx;
      if (vgamma) r += vg.e[k] * x.e[k];
      if (vbeta) r += vbe.e[k];
      o.e[k] = act_apply(r, yq.e, k, act);
    }
    ln_store<VEC>(ty + g.base, q, g.nq, c, o);
  }
}

// ---- adjoint, row launch ---------------------------------------------------------------------------------------------------
template <int NJ, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_ln_adjoint(float* __restrict__ ga_out, float* __restrict__ s_out,
                                                      const float* __restrict__ slabs, int splits, long long stride,
                                                      const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma, const float* __restrict__ y, int act,
                                                      int rows, int c) {
  __shared__ F4 tile_q[NJ ? 1 : LN_MAX_C / 4], tile_x[NJ ? 1 : LN_MAX_C / 4];
  __shared__ double red[2 * WAVES];
  const LnGeo g = ln_geo<NJ>(c);
  if (g.row >= rows) return;
  LnRow<NJ> qr(tile_q), xh(tile_x);
  F4 p1 = LN_ZERO, p2 = LN_ZERO;
  LN_FOR_QUADS {
    const int q = g.lt + LN_T * j;
    const F4 v = ln_slabs<VEC>(slabs, g.base, q, g.nq, c, splits, stride);
    const F4 yq = act != ACT_IDENTITY ? ln_map<VEC>(y + g.base, q, g.nq, c) : LN_ZERO;
    const F4 x = ln_map<VEC>(xhat + g.base, q, g.nq, c), gm = ln_cols(gamma, q, c);
    F4 s, qv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s.e[k] = act_apply(v.e[k], yq.e, k, act);
      qv.e[k] = gm.e[k] * s.e[k];
      p1.e[k] += qv.e[k];
      p2.e[k] += qv.e[k] * x.e[k];
    }
    ln_store<VEC>(s_out + g.base, q, g.nq, c, s);
    qr.set(j, qv);
    xh.set(j, x);
  }
  double m[2] = {ln_quad_sum(p1), ln_quad_sum(p2)};
  ln_row_sum<2, NJ>(m, red);
  const float m1 = (float)(m[0] / (double)c), mx = (float)(m[1] / (double)c), rs = rstd[g.row];
  LN_FOR_QUADS {
    const int q = g.lt + LN_T * j;
    if (q >= g.nq) continue;
    const F4 qv = qr.get(j), x = xh.get(j);
    F4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.e[k] = rs * ((qv.e[k] - m1) - x.e[k] * mx);
    ln_store<VEC>(ga_out + g.base, q, g.nq, c, o);
  }
}

// ---- adjoint, column launch ------------------------------------------------------------------------------------------------
template <bool SQ>
__device__ __forceinline__ double ln_term(float v) { return SQ ? (double)v * (double)v : (double)v; }

template <bool SQ>
__global__ __launch_bounds__(BLOCK) void k_ln_param_sums(float* __restrict__ o_gamma, float* __restrict__ o_beta,
                                                         float* __restrict__ o_b, const float* __restrict__ s,
                                                         const float* __restrict__ xh, const float* __restrict__ ga,
                                                         int rows, int c, float scale) {
  __shared__ double red[3][WAVES][LN_COLS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = blockIdx.x * LN_COLS + lane;
  const int chunk = (rows + WAVES - 1) / WAVES, r0 = wave * chunk, r1 = min(rows, r0 + chunk);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  if (col < c) {
    for (int r = r0; r < r1; ++r) {
      const int idx = r * c + col;
      if (o_gamma || o_beta) {
        const float sv = s[idx];
        if (o_gamma) a0 += ln_term<SQ>(sv * xh[idx]);
        if (o_beta) a1 += ln_term<SQ>(sv);
      }
      if (o_b) a2 += ln_term<SQ>(ga[idx]);
    }
  }
  red[0][wave][lane] = a0;
  red[1][wave][lane] = a1;
  red[2][wave][lane] = a2;
  __syncthreads();
  if (wave != 0 || col >= c) return;
  float* const outs[3] = {o_gamma, o_beta, o_b};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (!outs[k]) continue;
    double sum = red[k][0][lane];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) sum += red[k][w][lane];
    outs[k][col] = (float)sum * scale;
  }
}

// ---- validators ------------------------------------------------------------------------------------------------------------
inline bool ln_dims_ok(int64_t rows, int64_t c, int dtype) {
  return dtype == HF_F32 && rows >= 1 && rows <= LN_MAX_ROWS && c >= 1 && c <= LN_MAX_C;
}

inline bool ln_slabs_ok(const void* slabs, int splits, int64_t stride, int64_t rows, int64_t c) {
  return slabs && splits >= 1 && splits <= DENSE_MAX_SPLITS && (splits == 1 || stride >= rows * c);
}

// c % 4 == 0: the 16-byte form, so every row map (and the distance between two slabs) sits on the 16-byte grid
inline int ln_align(int64_t c, std::initializer_list<const void*> maps, int splits, int64_t stride) {
  if (c & 3) return HF_OK;
  for (const void* p : maps)
    if (p && !aligned16(p)) return HF_ERR_ALIGN;
  return splits > 1 && (stride & 3) ? HF_ERR_ALIGN : HF_OK;
}

// one row kernel on its form: wave per row (1, 2 or 4 quads per lane) or workgroup per row; 16-byte or element loads
#define LN_LAUNCH(KERNEL, NJ, GRID, ...)                                                      \
  do {                                                                                        \
    if ((c & 3) == 0) KERNEL<NJ, true><<<(unsigned)(GRID), BLOCK, 0, st>>>(__VA_ARGS__);      \
    else KERNEL<NJ, false><<<(unsigned)(GRID), BLOCK, 0, st>>>(__VA_ARGS__);                  \
  } while (0)
#define LN_DISPATCH(KERNEL, ...)                                                              \
  do {                                                                                        \
    hipStream_t st = (hipStream_t)stream;                                                     \
    const int64_t per_lane = ((c + 3) / 4 + 63) / 64, wgs = (rows + WAVES - 1) / WAVES;       \
    if (c > LN_WAVE_C) LN_LAUNCH(KERNEL, 0, rows, __VA_ARGS__);                               \
    else if (per_lane == 1) LN_LAUNCH(KERNEL, 1, wgs, __VA_ARGS__);                           \
    else if (per_lane == 2) LN_LAUNCH(KERNEL, 2, wgs, __VA_ARGS__);                           \
    else LN_LAUNCH(KERNEL, 4, wgs, __VA_ARGS__);                                              \
  } while (0)

}  // namespace

extern "C" {

int hf_ln_act_forward(void* y, void* xhat, void* rstd, const void* slabs, int splits, int64_t slab_stride, const void* b,
                      const void* gamma, const void* beta, double eps, int act, int64_t rows, int64_t c, int dtype,
                      void* stream) {
  if (!ln_dims_ok(rows, c, dtype) || !ln_slabs_ok(slabs, splits, slab_stride, rows, c)) return HF_ERR_ARG;
  if (!y || !xhat || !rstd || !gamma || !beta || act < ACT_IDENTITY || act > ACT_TANH || !(eps >= 0.0)) return HF_ERR_ARG;
  const int al = ln_align(c, {y, xhat, slabs}, splits, slab_stride);
  if (al != HF_OK) return al;
  LN_DISPATCH(k_ln_forward, (float*)y, (float*)xhat, (float*)rstd, (const float*)slabs, splits, (long long)slab_stride,
              (const float*)b, (const float*)gamma, (const float*)beta, eps, act, (int)rows, (int)c);
  return (int)hipGetLastError();
}

int hf_ln_act_tangent(void* t_y, const void* slabs, int splits, int64_t slab_stride, const void* v_b, const void* xhat,
                      const void* rstd, const void* gamma, const void* v_gamma, const void* v_beta, const void* y, int act,
                      int64_t rows, int64_t c, int dtype, void* stream) {
  if (!ln_dims_ok(rows, c, dtype) || !ln_slabs_ok(slabs, splits, slab_stride, rows, c)) return HF_ERR_ARG;
  if (!t_y || !xhat || !rstd || !gamma || act < ACT_IDENTITY || act > ACT_TANH) return HF_ERR_ARG;
  if (act != ACT_IDENTITY && !y) return HF_ERR_ARG;
  const int al = ln_align(c, {t_y, slabs, xhat, act != ACT_IDENTITY ? y : nullptr}, splits, slab_stride);
  if (al != HF_OK) return al;
  LN_DISPATCH(k_ln_tangent, (float*)t_y, (const float*)slabs, splits, (long long)slab_stride, (const float*)v_b,
              (const float*)xhat, (const float*)rstd, (const float*)gamma, (const float*)v_gamma, (const float*)v_beta,
              (const float*)y, act, (int)rows, (int)c);
  return (int)hipGetLastError();
}

int hf_ln_act_adjoint(void* g_a, void* s, const void* slabs, int splits, int64_t slab_stride, const void* xhat,
                      const void* rstd, const void* gamma, const void* y, int act, int64_t rows, int64_t c, int dtype,
                      void* stream) {
  if (!ln_dims_ok(rows, c, dtype) || !ln_slabs_ok(slabs, splits, slab_stride, rows, c)) return HF_ERR_ARG;
  if (!g_a || !s || !xhat || !rstd || !gamma || act < ACT_IDENTITY || act > ACT_TANH) return HF_ERR_ARG;
  if (act != ACT_IDENTITY && !y) return HF_ERR_ARG;
  const int al = ln_align(c, {g_a, s, slabs, xhat, act != ACT_IDENTITY ? y : nullptr}, splits, slab_stride);
  if (al != HF_OK) return al;
  LN_DISPATCH(k_ln_adjoint, (float*)g_a, (float*)s, (const float*)slabs, splits, (long long)slab_stride,
              (const float*)xhat, (const float*)rstd, (const float*)gamma, (const float*)y, act, (int)rows, (int)c);
  return (int)hipGetLastError();
}

int hf_ln_param_sums(void* o_gamma, void* o_beta, void* o_b, const void* s, const void* xhat, const void* g_a, int squared,
                     double scale, int64_t rows, int64_t c, int dtype, void* stream) {
  if (!ln_dims_ok(rows, c, dtype) || (squared != 0 && squared != 1) || !(scale == scale)) return HF_ERR_ARG;
  if (!o_gamma && !o_beta && !o_b) return HF_ERR_ARG;  // nothing to compute
  if (((o_gamma || o_beta) && !s) || (o_gamma && !xhat) || (o_b && !g_a)) return HF_ERR_ARG;
  const int al = ln_align(c, {s, xhat, g_a}, 1, 0);  // (the family's one rule for row maps; the outputs sit anywhere)
  if (al != HF_OK) return al;
  const unsigned grid = (unsigned)((c + LN_COLS - 1) / LN_COLS);
  hipStream_t st = (hipStream_t)stream;
  if (squared)
    k_ln_param_sums<true><<<grid, BLOCK, 0, st>>>((float*)o_gamma, (float*)o_beta, (float*)o_b, (const float*)s,
                                                  (const float*)xhat, (const float*)g_a, (int)rows, (int)c, (float)scale);
  else
    k_ln_param_sums<false><<<grid, BLOCK, 0, st>>>((float*)o_gamma, (float*)o_beta, (float*)o_b, (const float*)s,
                                                   (const float*)xhat, (const float*)g_a, (int)rows, (int)c, (float)scale);
  return (int)hipGetLastError();
}

}  // extern "C"
