// hf_head.hip -- the small non-convolution stages of the curvature engine's sweeps (gfx950):
// the max-pool behind a ResNet stem and the classifier head (linear layer + softmax
// cross-entropy Hessian).  Each of these was 2-6 ATen / rocBLAS launches of ~5 us inside
// every GGN product (BackPACK's R-op / L-op through them, optimizer.py:461); here each is ONE
// launch, with fixed summation orders (no atomics: the product stays bitwise repeatable).
//
// All tensors fp32, activations NHWC.

#include "hf_common.h"

namespace {

constexpr int HB = 256;

// ---------------------------------------------------------------------------------------
// max-pool, tangent:   out[n,oy,ox,c] = t[n, idx[n,oy,ox,c], c]
// idx = flat position (y*W + x) of the window's maximum in the forward pass (what
// max_pool2d_with_indices returns), stored NHWC int32.  `out` may be the first-channels slice
// of a wider NHWC buffer (out_ld floats per pixel).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB) void k_maxpool_tangent(float* __restrict__ out, const float* __restrict__ t,
                                                        const int* __restrict__ idx, unsigned total,
                                                        unsigned C, unsigned out_ld, unsigned opix, unsigned ipix) {
  const unsigned i = blockIdx.x * HB + threadIdx.x;
  if (i >= total) return;
  const unsigned c = i % C, pix = i / C, n = pix / opix;
  const float v = t[((size_t)n * ipix + (unsigned)idx[i]) * C + c];
  chain_store<HF_WT_ELEM>(&out[(size_t)pix * out_ld + c], v);
}

// ---------------------------------------------------------------------------------------
// max-pool, adjoint, in gather form (no zero-fill, no atomics):
//   g[n,y,x,c] = sum over the windows (oy,ox) that contain (y,x) and whose maximum sits at (y,x)
//                of  (sum_s A[s][n,oy,ox,c] + sum_s B[s][n,oy,ox,c])
// A, B: the cotangents of the pooled map from its two consumers (the first residual block's
// convolution and identity branch), each possibly split-K slabs that are summed here in split
// order.  Windows are visited in (oy, ox) order.
// ---------------------------------------------------------------------------------------
struct PoolGeo {
  int H, W, OH, OW, kh, kw, sh, sw, ph, pw;
};

__global__ __launch_bounds__(HB) void k_maxpool_adjoint(float* __restrict__ g, const float* __restrict__ A,
                                                        int a_splits, long long a_slab,
                                                        const float* __restrict__ B, int b_splits,
                                                        long long b_slab, const int* __restrict__ idx,
                                                        unsigned total, unsigned C, PoolGeo q) {
  const unsigned i = blockIdx.x * HB + threadIdx.x;
  if (i >= total) return;
  const unsigned c = i % C;
  unsigned pix = i / C;
  const int x = pix % q.W; pix /= q.W;
  const int y = pix % q.H;
  const int n = pix / q.H;
  const int self = y * q.W + x;
  // windows containing (y, x): oy*sh - ph <= y <= oy*sh - ph + kh - 1
  int oy0 = y + q.ph - q.kh + 1; oy0 = oy0 > 0 ? (oy0 + q.sh - 1) / q.sh : 0;
  int oy1 = (y + q.ph) / q.sh;   oy1 = oy1 < q.OH - 1 ? oy1 : q.OH - 1;
  int ox0 = x + q.pw - q.kw + 1; ox0 = ox0 > 0 ? (ox0 + q.sw - 1) / q.sw : 0;
  int ox1 = (x + q.pw) / q.sw;   ox1 = ox1 < q.OW - 1 ? ox1 : q.OW - 1;
  float acc = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      const size_t o = ((size_t)(n * q.OH + oy) * q.OW + ox) * C + c;
      if (idx[o] != self) continue;
      // slabs in batches of eight, all in flight before the first addition (one at a time is a dependent round
      // trip per slab: the first block's data gradient arrives as ~15 of them); same order of additions
      float v = A[o];
      const float w = B ? B[o] : 0.f;
      v = slab_sum<8>(v, A, o, a_splits, a_slab);
      if (B) v = v + slab_sum<8>(w, B, o, b_splits, b_slab);
      acc += v;
    }
  chain_store<HF_WT_ELEM>(&g[i], acc);
}

// max-pool, forward with positions (ATen's rule: first maximum in scan order, NaN wins)
__global__ __launch_bounds__(HB) void k_maxpool_forward(float* __restrict__ out, float* __restrict__ out2,
                                                        unsigned out2_ld, int* __restrict__ idx,
                                                        const float* __restrict__ x, unsigned total, unsigned C,
                                                        PoolGeo q) {
  const unsigned i = blockIdx.x * HB + threadIdx.x;
  if (i >= total) return;
  const unsigned c = i % C;
  unsigned pix = i / C;
  const unsigned opix = pix;
  const int ox = pix % q.OW; pix /= q.OW;
  const int oy = pix % q.OH;
  const int n = pix / q.OH;
  int y0 = oy * q.sh - q.ph, x0 = ox * q.sw - q.pw;
  const int y1 = y0 + q.kh < q.H ? y0 + q.kh : q.H, x1 = x0 + q.kw < q.W ? x0 + q.kw : q.W;
  y0 = y0 > 0 ? y0 : 0; x0 = x0 > 0 ? x0 : 0;
  float best = -__builtin_inff();
  int bi = y0 * q.W + x0;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) {
      const float v = x[((size_t)(n * q.H + yy) * q.W + xx) * C + c];
      if (v > best || v != v) { best = v; bi = yy * q.W + xx; }
    }
  if (out) out[i] = best;
  if (out2) out2[(size_t)opix * out2_ld + c] = best;
  idx[i] = bi;
}

// ---------------------------------------------------------------------------------------
// bias / ReLU / max-pool of a plain stack's pooled layer in ONE launch per direction.  ReLU masks and pool positions
// are piecewise constant, so with  y_pool = max_pool(relu(a + b))  and idx the windows' positions
//   tangent:  t_pool[n,oy,ox,c] = (y_pool > 0) * (t_a[n, idx, c] + v_b[c])
//   adjoint:  g_a[n,y,x,c]      = sum over the windows whose idx is (y,x) of (y_pool > 0) * g_pool[n,oy,ox,c]
// (a window's maximum of relu(.) is positive exactly where the pre-activation at idx is): neither sweep needs the
// full-resolution tangent map, the mask comes from the pooled map.  A thread owns W consecutive channels of a pixel
// (W = 4: 16-byte loads of idx / y_pool / cotangents, 16-byte stores; W = 1: any channel count and alignment).
// ---------------------------------------------------------------------------------------
// A pooled BatchNorm unit  y_pool = max_pool(relu?(xhat*w + b)),  xhat = (a - mean)*rstd  (eval mode), is the same pair
// of kernels under the flag BN, with these operands (the bias instantiations carry them unread and keep their bits):
//   tangent:  t_pool = m * (t_a[idx]*(w*rstd) + xhat[idx]*v_w + v_b)    -- hf_chan_affine_ex's rounding sequence
//   adjoint:  g = the bias form's g_a (unscaled, masked);  g_a = g*(w*rstd);  gb = sum g,  gw = sum g*xhat
struct PoolBn {
  const float *a, *mean, *rstd, *w, *vw;
};

template <int W, bool BN>
__global__ __launch_bounds__(HB) void k_pool_act_tangent(float* __restrict__ out, const float* __restrict__ slabs,
                                                         int splits, long long slab_stride,
                                                         const float* __restrict__ vb, const int* __restrict__ idx,
                                                         const float* __restrict__ ypool, unsigned total,
                                                         unsigned CQ, unsigned out_ld, unsigned opix, unsigned ipix,
                                                         const PoolBn bn) {
  using VF = ColOf<float, W>;
  using VI = ColOf<int, W>;
  const unsigned i = blockIdx.x * HB + threadIdx.x;
  if (i >= total) return;
  const unsigned cq = i % CQ, pix = i / CQ, n = pix / opix, C = CQ * W, c0 = cq * W;
  const unsigned e = pix * C + c0;
  const VI ix = *reinterpret_cast<const VI*>(idx + e);
  VF m, b, s;
  if (ypool) m = *reinterpret_cast<const VF*>(ypool + e);
  if (vb) {  // (a slice of the flat vector: on any 4-byte boundary)
#pragma unroll
    for (int k = 0; k < W; ++k) b.e[k] = vb[c0 + k];
  }
  VF sc, rs, mu, q, av;  // (BN) per channel: w*rstd, rstd, mean, v_w; the convolution output at the position
  if constexpr (BN) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      rs.e[k] = bn.rstd[c0 + k];
      sc.e[k] = bn.w[c0 + k] * rs.e[k];
      if (bn.vw) { mu.e[k] = bn.mean[c0 + k]; q.e[k] = bn.vw[c0 + k]; }
    }
  }
  unsigned off[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    // (a position outside the plane would be a read outside the slabs: clamped, never followed)
    const unsigned p = (unsigned)ix.e[k] < ipix ? (unsigned)ix.e[k] : ipix - 1;
    off[k] = (n * ipix + p) * C + c0 + k;
    s.e[k] = slabs[off[k]];
    if constexpr (BN) {
      if (bn.vw) av.e[k] = bn.a[off[k]];
    }
  }
  // slab_sum, for the W channels together: one batch of all of them in flight, each channel added in split order
  for (int sp = 1; sp < splits; sp += 8) {
    float v[W][8];
#pragma unroll
    for (int k = 0; k < W; ++k) slab_issue(v[k], slabs, off[k], sp, splits, slab_stride);
#pragma unroll
    for (int k = 0; k < W; ++k) slab_add<false>(s.e[k], v[k], sp, splits);
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    float t = s.e[k];
    if constexpr (BN) {
      t = t * sc.e[k];
      if (bn.vw) t = t + ((av.e[k] - mu.e[k]) * rs.e[k]) * q.e[k];
    }
    if (vb) t = t + b.e[k];
    if (ypool) t = m.e[k] > 0.f ? t : 0.f;
    s.e[k] = t;
  }
  chain_store_col<HF_WT_ELEM>(out + (size_t)pix * out_ld + c0, s);
}

// g_a of W channels of the full-resolution pixel (n, y, x): windows in (oy, ox) order, each one's slabs in split order
template <int W>
__device__ __forceinline__ ColOf<float, W> pool_act_adjoint_at(const float* __restrict__ gy, int splits,
                                                               long long slab, const int* __restrict__ idx,
                                                               const float* __restrict__ ypool, unsigned C,
                                                               unsigned c0, int n, int y, int x, const PoolGeo& q) {
  using VF = ColOf<float, W>;
  using VI = ColOf<int, W>;
  const int self = y * q.W + x;
  // windows containing (y, x): oy*sh - ph <= y <= oy*sh - ph + kh - 1
  int oy0 = y + q.ph - q.kh + 1; oy0 = oy0 > 0 ? (oy0 + q.sh - 1) / q.sh : 0;
  int oy1 = (y + q.ph) / q.sh;   oy1 = oy1 < q.OH - 1 ? oy1 : q.OH - 1;
  int ox0 = x + q.pw - q.kw + 1; ox0 = ox0 > 0 ? (ox0 + q.sw - 1) / q.sw : 0;
  int ox1 = (x + q.pw) / q.sw;   ox1 = ox1 < q.OW - 1 ? ox1 : q.OW - 1;
  VF acc;
#pragma unroll
  for (int k = 0; k < W; ++k) acc.e[k] = 0.f;
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      const unsigned o = (unsigned)((n * q.OH + oy) * q.OW + ox) * C + c0;
      const VI ix = *reinterpret_cast<const VI*>(idx + o);
      bool any = false;
#pragma unroll
      for (int k = 0; k < W; ++k) any = any || ix.e[k] == self;
      if (!any) continue;
      VF v = *reinterpret_cast<const VF*>(gy + o);
      VF m;
      if (ypool) m = *reinterpret_cast<const VF*>(ypool + o);
      v = slab_sum<8>(v, gy, o, splits, slab);
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const bool on = ix.e[k] == self && (!ypool || m.e[k] > 0.f);
        acc.e[k] += on ? v.e[k] : 0.f;
      }
    }
  return acc;
}

// (BN) g_a = g * (w*rstd), w*rstd formed first: hf_bn_adjoint_v4's rounding
template <int W>
__device__ __forceinline__ ColOf<float, W> pool_bn_scale(const ColOf<float, W>& g, const PoolBn& bn, unsigned c0) {
  ColOf<float, W> o;
#pragma unroll
  for (int k = 0; k < W; ++k) o.e[k] = g.e[k] * (bn.w[c0 + k] * bn.rstd[c0 + k]);
  return o;
}

// without per-channel sums: one pixel's W channels per thread
template <int W, bool BN>
__global__ __launch_bounds__(HB) void k_pool_act_adjoint(float* __restrict__ ga, float* __restrict__ g,
                                                         const float* __restrict__ gy, int splits, long long slab,
                                                         const int* __restrict__ idx,
                                                         const float* __restrict__ ypool, unsigned total,
                                                         unsigned CQ, PoolGeo q, const PoolBn bn) {
  const unsigned i = blockIdx.x * HB + threadIdx.x;
  if (i >= total) return;
  const unsigned cq = i % CQ, C = CQ * W;
  unsigned pix = i / CQ;
  const unsigned row = pix;
  const int x = pix % q.W; pix /= q.W;
  const int y = pix % q.H;
  const int n = pix / q.H;
  const ColOf<float, W> v = pool_act_adjoint_at<W>(gy, splits, slab, idx, ypool, C, cq * W, n, y, x, q);
  if constexpr (BN) {
    if (g) chain_store_col<HF_WT_ELEM>(g + (size_t)row * C + cq * W, v);
    chain_store_col<HF_WT_ELEM>(ga + (size_t)row * C + cq * W, pool_bn_scale<W>(v, bn, cq * W));
  } else {
    chain_store_col<HF_WT_ELEM>(ga + (size_t)row * C + cq * W, v);
  }
}

// with per-channel sums: workgroup b owns the full-resolution rows [b*per, (b+1)*per) and all channels, as the row-major
// BatchNorm adjoint (hf_bn.hip) does; thread (tx, ty) walks channel column tx of every G-th row of the share and keeps
// its sum in fp64; the G sums of a column are added in ty order and rounded once -> gb[b*C + channel]
// (BN: a second sum per channel, of g * xhat with xhat rounded to fp32 first -> gw[b*C + channel]; either is nullable)
// (GA = false, BN only: the reduction pass of a TRAIN-mode unit -- g and the sums; no ga = g*(w*rstd), which batch
// statistics would throw away: the store is compiled out, `ga` is not touched)
template <int W, bool BN, bool GA = true>
__global__ __launch_bounds__(HB) void k_pool_act_adjoint_rows(float* __restrict__ ga, float* __restrict__ g,
                                                              float* __restrict__ gw, float* __restrict__ gb,
                                                              const float* __restrict__ gy, int splits,
                                                              long long slab, const int* __restrict__ idx,
                                                              const float* __restrict__ ypool, unsigned rows,
                                                              unsigned per, unsigned CQ, PoolGeo q, const PoolBn bn) {
  constexpr int S = BN ? 2 : 1;  // sums per channel
  __shared__ double red[HB * W * S];
  const unsigned C = CQ * W, cols = CQ < HB ? CQ : HB, G = HB / cols;
  const unsigned tx = threadIdx.x % cols, ty = threadIdx.x / cols;
  const unsigned lo = blockIdx.x * per, hi = lo + per < rows ? lo + per : rows;
  for (unsigned cb = 0; cb < CQ; cb += cols) {
    const unsigned cq = cb + tx;
    const bool live = ty < G && cq < CQ;
    double acc[W * S];
#pragma unroll
    for (int k = 0; k < W * S; ++k) acc[k] = 0.0;
    if (live) {
      float rs[W], mu[W];
      if constexpr (BN) {
        if (gw) {
#pragma unroll
          for (int k = 0; k < W; ++k) { rs[k] = bn.rstd[cq * W + k]; mu[k] = bn.mean[cq * W + k]; }
        }
      }
      for (unsigned r = lo + ty; r < hi; r += G) {
        unsigned pix = r;
        const int x = pix % q.W; pix /= q.W;
        const int y = pix % q.H;
        const int n = pix / q.H;
        ColOf<float, W> av;
        if constexpr (BN) {
          if (gw) av = *reinterpret_cast<const ColOf<float, W>*>(bn.a + (size_t)r * C + cq * W);
        }
        const ColOf<float, W> v = pool_act_adjoint_at<W>(gy, splits, slab, idx, ypool, C, cq * W, n, y, x, q);
        if constexpr (BN) {
          if (g) chain_store_col<HF_WT_ELEM>(g + (size_t)r * C + cq * W, v);
          if constexpr (GA) chain_store_col<HF_WT_ELEM>(ga + (size_t)r * C + cq * W, pool_bn_scale<W>(v, bn, cq * W));
          if (gw) {
#pragma unroll
            for (int k = 0; k < W; ++k) acc[W + k] += (double)v.e[k] * (double)(float)((av.e[k] - mu[k]) * rs[k]);
          }
        } else {
          chain_store_col<HF_WT_ELEM>(ga + (size_t)r * C + cq * W, v);
        }
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += (double)v.e[k];
      }
#pragma unroll
      for (int k = 0; k < W * S; ++k) red[(ty * cols + tx) * W * S + k] = acc[k];
    }
    __syncthreads();
    if (ty == 0 && cq < CQ) {
#pragma unroll
      for (int k = 0; k < W * S; ++k) {
        float* dst = k < W ? gb : gw;
        double sum = 0.0;
        for (unsigned t = 0; t < G; ++t) sum += red[(t * cols + tx) * W * S + k];
        const float f = (float)sum;
        if (dst) chain_store<HF_WT_ELEM>(&dst[(size_t)blockIdx.x * C + cq * W + (k < W ? k : k - W)], f);
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------
// Classifier head of the GGN product in one launch:
//   Jv   = t_feat W^T + feat V_W^T + v_b          tangent of the logits        [B, K]
//   HJv  = scale * p * (Jv - <p, Jv>)             softmax-CE Hessian, row-wise [B, K]
//   g_feat = HJv W    [B, F],   g_W = HJv^T feat  [K, F],   g_b = sum_b HJv    [K]
// One workgroup per HEAD_R rows, one wave per row.  ONE round of global loads: W and V_W go to
// LDS, every wave keeps its row's features and feature tangents in registers; everything after
// the barrier reads LDS.  The sums over the rows (g_W, g_b) are left to the consumer: workgroup
// g writes the partial sums of ITS rows to slab g, hf_pack_ex adds the slabs up in order (as
// it does for split-K weight gradients).  Measured on the way here: a single workgroup that went
// back to L2 for every class 26 us (twelve dependent round trips); a single workgroup with
// everything in LDS 19-20 us (2.7 MB of LDS reads through ONE CU's 128 B/clk); this form spreads
// them over ceil(B / HEAD_R) CUs.
// ---------------------------------------------------------------------------------------
constexpr int HEAD_R = 4, HEAD_T = 64 * HEAD_R, KB = 5;

template <int CH>  // float4 chunks per lane: F <= 256*CH
__global__ __launch_bounds__(HEAD_T) void k_linear_ce_head(
    float* __restrict__ g_feat, float* __restrict__ g_w, float* __restrict__ g_b,
    const float* __restrict__ t_feat, const float* __restrict__ feat, const float* __restrict__ W,
    const float* __restrict__ VW, const float* __restrict__ vb, const float* __restrict__ p, float scale,
    int B, int F, int K) {
  extern __shared__ float lds[];
  const int F4 = F >> 2;
  float4* s_w = reinterpret_cast<float4*>(lds);   // [K][F]
  float4* s_vw = s_w + K * F4;                    // [K][F]
  float4* s_feat = s_vw + K * F4;                 // [HEAD_R][F]
  float* s_h = reinterpret_cast<float*>(s_feat + HEAD_R * F4);  // [HEAD_R][K]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * HEAD_R + wave;
  const bool row = b < B;
  // ---- the only round of global loads ----
  for (int e = threadIdx.x; e < K * F4; e += HEAD_T) {
    s_w[e] = reinterpret_cast<const float4*>(W)[e];
    s_vw[e] = reinterpret_cast<const float4*>(VW)[e];
  }
  float4 tf[CH], ff[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    const int j = lane + 64 * u;
    tf[u] = ff[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row && j < F4) {
      tf[u] = reinterpret_cast<const float4*>(t_feat + (size_t)b * F)[j];
      ff[u] = reinterpret_cast<const float4*>(feat + (size_t)b * F)[j];
    }
    if (j < F4) s_feat[wave * F4 + j] = ff[u];  // (zeros for a row past the end)
  }
  const float pk = (row && lane < K) ? p[(size_t)b * K + lane] : 0.f;
  const float bias = (vb && lane < K) ? vb[lane] : 0.f;
  __syncthreads();
  // ---- the row: logits' tangent, KB classes per pass (their wave reductions interleave) ----
  float jv = 0.f;  // lane k keeps Jv[b][k]
  for (int k0 = 0; k0 < K; k0 += KB) {
    float part[KB];
#pragma unroll
    for (int r = 0; r < KB; ++r) {
      const int k = k0 + r < K ? k0 + r : K - 1;  // (clamped: the surplus sums are discarded)
      float p0 = 0.f, p1 = 0.f;
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const int j = lane + 64 * u;
        if (j < F4) {
          const float4 w = s_w[k * F4 + j], v = s_vw[k * F4 + j];
          // (explicit fma: the file is built with -ffp-contract=off)
          p0 = fmaf(tf[u].x, w.x, p0); p1 = fmaf(tf[u].y, w.y, p1);
          p0 = fmaf(tf[u].z, w.z, p0); p1 = fmaf(tf[u].w, w.w, p1);
          p0 = fmaf(ff[u].x, v.x, p0); p1 = fmaf(ff[u].y, v.y, p1);
          p0 = fmaf(ff[u].z, v.z, p0); p1 = fmaf(ff[u].w, v.w, p1);
        }
      }
      part[r] = p0 + p1;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int r = 0; r < KB; ++r) part[r] += __shfl_xor(part[r], off, 64);
    }
#pragma unroll
    for (int r = 0; r < KB; ++r)
      if (lane == k0 + r && k0 + r < K) jv = part[r] + bias;
  }
  double d = (double)pk * (double)jv;  // <p, Jv> in fp64, as hf_softmax_ce_hvp
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
  const float h = row ? scale * (pk * (jv - (float)d)) : 0.f;
  if (lane < K) s_h[wave * K + lane] = h;
  // ---- the row's data gradient ----
  float4 acc[CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k0 = 0; k0 < K; k0 += KB) {
#pragma unroll
    for (int r = 0; r < KB; ++r) {
      const int k = k0 + r < K ? k0 + r : K - 1;
      const float hk = k0 + r < K ? __shfl(h, k, 64) : 0.f;
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const int j = lane + 64 * u;
        if (j < F4) {
          const float4 w = s_w[k * F4 + j];
          acc[u].x = fmaf(hk, w.x, acc[u].x); acc[u].y = fmaf(hk, w.y, acc[u].y);
          acc[u].z = fmaf(hk, w.z, acc[u].z); acc[u].w = fmaf(hk, w.w, acc[u].w);
        }
      }
    }
  }
  if (row) {
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int j = lane + 64 * u;
      if (j < F4) chain_store16<HF_WT_ELEM>(&reinterpret_cast<float4*>(g_feat + (size_t)b * F)[j], acc[u]);
    }
  }
  __syncthreads();
  // ---- this workgroup's share of the weight / bias gradient (its rows, in order) -> slab ----
  float* gw = g_w + (size_t)blockIdx.x * K * F;
  for (int e = threadIdx.x; e < K * F4; e += HEAD_T) {
    const int k = e / F4, j = e % F4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int r = 0; r < HEAD_R; ++r) {
      const float hb = s_h[r * K + k];
      const float4 f = s_feat[r * F4 + j];
      s.x = fmaf(hb, f.x, s.x); s.y = fmaf(hb, f.y, s.y); s.z = fmaf(hb, f.z, s.z); s.w = fmaf(hb, f.w, s.w);
    }
    chain_store16<HF_WT_ELEM>(&reinterpret_cast<float4*>(gw)[e], s);
  }
  if (g_b && threadIdx.x < K) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < HEAD_R; ++r) s += s_h[r * K + threadIdx.x];
    chain_store<HF_WT_ELEM>(&g_b[(size_t)blockIdx.x * K + threadIdx.x], s);
  }
}

// ---------------------------------------------------------------------------------------
// Head of a network ending in global average pooling, inside J^T H_L J v (one workgroup per sample):
//   Jv[k] = mean_hw t[hw][k];  h = scale * p * (Jv - <p, Jv>);  g[hw][k] = h[k] / hw
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(HB) void k_pool_ce_head(float* __restrict__ g, float* __restrict__ jv_out,
                                                     const float* __restrict__ t, const float* __restrict__ p,
                                                     float scale, int HW, int K) {
  __shared__ double red[HB / 64];
  __shared__ float s_h[1024];
  const int n = blockIdx.x;
  const float* tn = t + (size_t)n * HW * K;
  double part = 0.0;
  float jv_mine[4];  // K <= 1024: up to 4 classes per thread
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = threadIdx.x + u * HB;
    float s = 0.f;
    if (k < K) {
      for (int q = 0; q < HW; ++q) s += tn[(size_t)q * K + k];
      s = s / (float)HW;
      if (jv_out) chain_store<HF_WT_ELEM>(&jv_out[(size_t)n * K + k], s);
      part += (double)p[(size_t)n * K + k] * (double)s;
    }
    jv_mine[u] = s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
  __syncthreads();
  double d = red[0];
#pragma unroll
  for (int w = 1; w < HB / 64; ++w) d += red[w];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = threadIdx.x + u * HB;
    if (k < K) s_h[k] = (scale * (p[(size_t)n * K + k] * (jv_mine[u] - (float)d))) / (float)HW;
  }
  __syncthreads();
  float* gn = g + (size_t)n * HW * K;
  for (int e = threadIdx.x; e < HW * K; e += HB) {
    const float h = s_h[e % K];
    chain_store<HF_WT_ELEM>(&gn[e], h);
  }
}

// ---------------------------------------------------------------------------------------
// The boundary between a conv stack (NHWC maps) and a classifier tail behind nn.Flatten (rows whose features run
// (c, h, w), the order the first Linear's weight is read in): a per-sample hw x c transpose, both directions.
//   flatten:    out[r][ch*hw + p] = in[(r*hw + p)*in_ld + ch]
//   unflatten:  out[(r*hw + p)*c + ch] = sum_s slabs[s][r][ch*hw + p]          (slab_sum: slab 0, then 1 .. n-1)
// One workgroup per FT x FT tile of one sample through LDS, so both global sides run contiguously: 16 bytes per lane
// along c on the NHWC side (lane = (pixel t/8, channel quad t%8)), 4 bytes per lane along p on the row side (lane =
// (channel t/32 + 8k, pixel t%32): hw is arbitrary, rows start on any 4-byte boundary).  The tile lies [channel][pixel]
// with a pitch of FT + 1 dwords.  Row side: a 32-lane half is one channel and 32 consecutive pixels -> 32 banks.
// NHWC side, component j: dword (4q + j)*33 + p, bank (4q + j + p) % 32 with q = 0..7 and four consecutive p per half
// -> 4q + (p - p_lo) covers 0..31 once.  Conflict-free on both sides (ds_write_b32 / ds_read_b32 bank as (a/4) % 32 per
// 32-lane half).
// ---------------------------------------------------------------------------------------
constexpr int FT = 32, FPITCH = FT + 1;

__global__ __launch_bounds__(HB) void k_flatten_rows(float* __restrict__ out, const float* __restrict__ in,
                                                     unsigned out_ld, unsigned in_ld, unsigned hw, unsigned c,
                                                     unsigned tiles_p, unsigned tiles_c) {
  __shared__ float tile[FT * FPITCH];
  unsigned b = blockIdx.x;
  const unsigned c0 = (b % tiles_c) * FT; b /= tiles_c;
  const unsigned p0 = (b % tiles_p) * FT;
  const unsigned r = b / tiles_p;
  {
    const unsigned q = threadIdx.x % 8, p = threadIdx.x / 8;
    if (p0 + p < hw && c0 + 4 * q < c) {
      const F4 v = ld4(in + ((size_t)r * hw + p0 + p) * in_ld + c0 + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[(4 * q + j) * FPITCH + p] = v.e[j];
    }
  }
  __syncthreads();
  const unsigned p = threadIdx.x % FT;
  if (p0 + p >= hw) return;
#pragma unroll
  for (int k = 0; k < FT / 8; ++k) {
    const unsigned ch = threadIdx.x / FT + 8 * k;
    if (c0 + ch < c)
      chain_store<HF_WT_ELEM>(&out[(size_t)r * out_ld + (size_t)(c0 + ch) * hw + p0 + p], tile[ch * FPITCH + p]);
  }
}

__global__ __launch_bounds__(HB) void k_unflatten_slabs(float* __restrict__ out, const float* __restrict__ slabs,
                                                        int splits, long long slab_stride, unsigned hw, unsigned c,
                                                        unsigned tiles_p, unsigned tiles_c) {
  __shared__ float tile[FT * FPITCH];
  unsigned b = blockIdx.x;
  const unsigned c0 = (b % tiles_c) * FT; b /= tiles_c;
  const unsigned p0 = (b % tiles_p) * FT;
  const unsigned r = b / tiles_p;
  {
    const unsigned p = threadIdx.x % FT;
    if (p0 + p < hw) {
#pragma unroll
      for (int k = 0; k < FT / 8; ++k) {
        const unsigned ch = threadIdx.x / FT + 8 * k;
        if (c0 + ch < c) {
          const size_t off = ((size_t)r * c + c0 + ch) * hw + p0 + p;
          tile[ch * FPITCH + p] = slab_sum<8>(slabs[off], slabs, off, splits, slab_stride);
        }
      }
    }
  }
  __syncthreads();
  const unsigned q = threadIdx.x % 8, p = threadIdx.x / 8;
  if (p0 + p < hw && c0 + 4 * q < c) {
    F4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v.e[j] = tile[(4 * q + j) * FPITCH + p];
    chain_store4<HF_WT_ELEM>(out + ((size_t)r * hw + p0 + p) * c + c0 + 4 * q, v);
  }
}

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// what the two boundary kernels share: extents, the dense kernels' feature limit, the tile grid
inline int flatten_grid(int64_t n, int64_t hw, int64_t c, int dtype, unsigned* tiles_p, unsigned* tiles_c,
                        unsigned* blocks) {
  if (dtype != HF_F32 || n < 1 || hw < 1 || c < 1 || c % 4) return HF_ERR_ARG;
  const int64_t lim = 1LL << 31;
  if (n >= lim || hw > HF_FLATTEN_MAX_FEATURES || c > HF_FLATTEN_MAX_FEATURES || c * hw > HF_FLATTEN_MAX_FEATURES)
    return HF_ERR_ARG;
  const int64_t tp = (hw + FT - 1) / FT, tc = (c + FT - 1) / FT;
  if (n * tp * tc >= lim) return HF_ERR_ARG;
  *tiles_p = (unsigned)tp; *tiles_c = (unsigned)tc; *blocks = (unsigned)(n * tp * tc);
  return HF_OK;
}

// the two pooled-unit entry points of each direction share everything but the BatchNorm operands (bn: NULL = a bias unit)
int pool_act_tangent(void* out, int64_t out_ld, const void* slabs, int splits, int64_t slab_stride, const void* v_b,
                     const void* idx, const void* y_pool, int relu, int64_t n, int64_t h, int64_t w, int64_t oh,
                     int64_t ow, int64_t c, int dtype, void* stream, const PoolBn* bn) {
  if (dtype != HF_F32 || !out || !slabs || !idx || (relu && !y_pool)) return HF_ERR_ARG;
  if (n < 1 || h < 1 || w < 1 || oh < 1 || ow < 1 || c < 1) return HF_ERR_ARG;
  if (splits < 1 || splits > HF_POOL_ACT_MAX_SPLITS) return HF_ERR_ARG;
  if (out_ld == 0) out_ld = c;
  if (out_ld < c) return HF_ERR_ARG;
  // (every factor below 2^31 first: the products cannot wrap)
  const int64_t lim = 1LL << 31;
  if (n >= lim || h >= lim || w >= lim || oh >= lim || ow >= lim || c >= lim || out_ld >= lim) return HF_ERR_ARG;
  if (h * w >= lim || oh * ow >= lim || n * (h * w) >= lim || n * (oh * ow) >= lim) return HF_ERR_ARG;
  const int64_t full = n * h * w * c, total = n * oh * ow * c;
  if (full >= lim || total >= lim || n * oh * ow * out_ld >= lim) return HF_ERR_ARG;
  if (splits > 1 && slab_stride < full) return HF_ERR_ARG;  // (slabs would overlap)
  const float* yp = relu ? (const float*)y_pool : nullptr;
  const bool quad = c % 4 == 0 && out_ld % 4 == 0 && al16(out) && al16(idx) && (!yp || al16(yp));
  const unsigned cq = (unsigned)(quad ? c / 4 : c), items = (unsigned)(total / (quad ? 4 : 1));
  const PoolBn ops = bn ? *bn : PoolBn{};
#define HF_PAT(W, BN)                                                                                              \
  hipLaunchKernelGGL((k_pool_act_tangent<W, BN>), dim3((items + HB - 1) / HB), dim3(HB), 0, (hipStream_t)stream,  \
                     (float*)out, (const float*)slabs, splits, (long long)slab_stride, (const float*)v_b,         \
                     (const int*)idx, yp, items, cq, (unsigned)out_ld, (unsigned)(oh * ow), (unsigned)(h * w), ops)
  if (bn) { if (quad) HF_PAT(4, true); else HF_PAT(1, true); }
  else if (quad) HF_PAT(4, false);
  else HF_PAT(1, false);
#undef HF_PAT
  return (int)hipGetLastError();
}

int pool_act_adjoint(void* ga, void* g, void* gw, void* gb, int row_blocks, const void* gy, int gy_splits, int64_t gy_slab,
                     const void* idx, const void* y_pool, int relu, int64_t n, int64_t h, int64_t w, int64_t oh,
                     int64_t ow, int64_t c, int64_t kh, int64_t kw, int64_t stride_h, int64_t stride_w, int64_t pad_h,
                     int64_t pad_w, int dtype, void* stream, const PoolBn* bn, bool reduce = false) {
  // (reduce: a train-mode unit's reduction pass -- no ga; g and both sum rows are what it is for)
  if (reduce ? (ga || !g || !gw || !gb || !bn) : !ga) return HF_ERR_ARG;
  if (dtype != HF_F32 || !gy || !idx || (relu && !y_pool)) return HF_ERR_ARG;
  if (n < 1 || h < 1 || w < 1 || oh < 1 || ow < 1 || c < 1) return HF_ERR_ARG;
  if (kh < 1 || kw < 1 || stride_h < 1 || stride_w < 1 || pad_h < 0 || pad_w < 0) return HF_ERR_ARG;
  if (gy_splits < 1 || gy_splits > HF_POOL_ACT_MAX_SPLITS) return HF_ERR_ARG;
  const int64_t lim = 1LL << 31;
  if (n >= lim || h >= lim || w >= lim || oh >= lim || ow >= lim || c >= lim) return HF_ERR_ARG;
  if (kh >= lim || kw >= lim || stride_h >= lim || stride_w >= lim || pad_h >= lim || pad_w >= lim) return HF_ERR_ARG;
  // the pooled extent of a max-pool without dilation / ceil_mode
  if (h + 2 * pad_h < kh || w + 2 * pad_w < kw) return HF_ERR_ARG;
  if (oh != (h + 2 * pad_h - kh) / stride_h + 1 || ow != (w + 2 * pad_w - kw) / stride_w + 1) return HF_ERR_ARG;
  if (h * w >= lim || oh * ow >= lim || n * (h * w) >= lim || n * (oh * ow) >= lim) return HF_ERR_ARG;
  const int64_t rows = n * h * w, full = rows * c, pooled = n * oh * ow * c;
  if (full >= lim || pooled >= lim) return HF_ERR_ARG;
  if (gy_splits > 1 && gy_slab < pooled) return HF_ERR_ARG;  // (slabs would overlap)
  int64_t per = 0;
  if (gb || gw) {
    if (row_blocks < 1) return HF_ERR_ARG;
    per = (rows + row_blocks - 1) / row_blocks;
    if ((int64_t)(row_blocks - 1) * per >= rows) return HF_ERR_ARG;  // an empty share
  }
  const float* yp = relu ? (const float*)y_pool : nullptr;
  const bool quad = c % 4 == 0 && al16(ga) && al16(gy) && al16(idx) && (!yp || al16(yp)) &&
                    (gy_splits == 1 || gy_slab % 4 == 0) && al16(g) && (!bn || al16(bn->a));
  const unsigned cq = (unsigned)(quad ? c / 4 : c);
  PoolGeo q{(int)h, (int)w, (int)oh, (int)ow, (int)kh, (int)kw, (int)stride_h, (int)stride_w, (int)pad_h, (int)pad_w};
  hipStream_t s = (hipStream_t)stream;
  const PoolBn ops = bn ? *bn : PoolBn{};
  if (gb || gw) {
#define HF_PAA(W, BN, GA)                                                                                          \
  hipLaunchKernelGGL((k_pool_act_adjoint_rows<W, BN, GA>), dim3((unsigned)row_blocks), dim3(HB), 0, s, (float*)ga, \
                     (float*)g, (float*)gw, (float*)gb, (const float*)gy, gy_splits, (long long)gy_slab,          \
                     (const int*)idx, yp, (unsigned)rows, (unsigned)per, cq, q, ops)
    if (reduce) { if (quad) HF_PAA(4, true, false); else HF_PAA(1, true, false); }
    else if (bn) { if (quad) HF_PAA(4, true, true); else HF_PAA(1, true, true); }
    else if (quad) HF_PAA(4, false, true);
    else HF_PAA(1, false, true);
#undef HF_PAA
  } else {
    const unsigned items = (unsigned)(rows * cq);
#define HF_PAE(W, BN)                                                                                              \
  hipLaunchKernelGGL((k_pool_act_adjoint<W, BN>), dim3((items + HB - 1) / HB), dim3(HB), 0, s, (float*)ga,        \
                     (float*)g, (const float*)gy, gy_splits, (long long)gy_slab, (const int*)idx, yp, items, cq, q, \
                     ops)
    if (bn) { if (quad) HF_PAE(4, true); else HF_PAE(1, true); }
    else if (quad) HF_PAE(4, false);
    else HF_PAE(1, false);
#undef HF_PAE
  }
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int hf_maxpool_tangent_nhwc(void* out, const void* t, const void* idx, int64_t n, int64_t h, int64_t w,
                            int64_t oh, int64_t ow, int64_t c, int64_t out_ld, int dtype, void* stream) {
  if (dtype != HF_F32 || !out || !t || !idx || n < 1 || c < 1) return -1;
  const int64_t total = n * oh * ow * c;
  if (total >= (1LL << 31) || n * h * w * c >= (1LL << 31)) return -1;
  if (out_ld == 0) out_ld = c;
  if (out_ld < c) return -1;
  hipLaunchKernelGGL(k_maxpool_tangent, dim3((unsigned)((total + HB - 1) / HB)), dim3(HB), 0,
                     (hipStream_t)stream, (float*)out, (const float*)t, (const int*)idx, (unsigned)total,
                     (unsigned)c, (unsigned)out_ld, (unsigned)(oh * ow), (unsigned)(h * w));
  return (int)hipGetLastError();
}

int hf_maxpool_forward_nhwc(void* out, void* out2, int64_t out2_ld, void* idx, const void* x, int64_t n,
                            int64_t h, int64_t w, int64_t oh, int64_t ow, int64_t c, int64_t kh, int64_t kw,
                            int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int dtype,
                            void* stream) {
  if (dtype != HF_F32 || !idx || !x || (!out && !out2) || n < 1 || c < 1 || oh < 1 || ow < 1) return -1;
  if (kh < 1 || kw < 1 || stride_h < 1 || stride_w < 1 || pad_h < 0 || pad_w < 0) return -1;
  const int64_t total = n * oh * ow * c;
  if (total >= (1LL << 31) || n * h * w * c >= (1LL << 31)) return -1;
  if (out2 && out2_ld < c) return -1;
  if (n * oh * ow * (out2 ? out2_ld : c) >= (1LL << 31)) return -1;
  PoolGeo q{(int)h, (int)w, (int)oh, (int)ow, (int)kh, (int)kw, (int)stride_h, (int)stride_w, (int)pad_h, (int)pad_w};
  hipLaunchKernelGGL(k_maxpool_forward, dim3((unsigned)((total + HB - 1) / HB)), dim3(HB), 0,
                     (hipStream_t)stream, (float*)out, (float*)out2, (unsigned)out2_ld, (int*)idx,
                     (const float*)x, (unsigned)total, (unsigned)c, q);
  return (int)hipGetLastError();
}

int hf_maxpool_adjoint_nhwc(void* g, const void* gy_a, int a_splits, int64_t a_slab, const void* gy_b,
                            int b_splits, int64_t b_slab, const void* idx, int64_t n, int64_t h, int64_t w,
                            int64_t oh, int64_t ow, int64_t c, int64_t kh, int64_t kw, int64_t stride_h,
                            int64_t stride_w, int64_t pad_h, int64_t pad_w, int dtype, void* stream) {
  if (dtype != HF_F32 || !g || !gy_a || !idx || n < 1 || c < 1 || a_splits < 1 || (gy_b && b_splits < 1)) return -1;
  if (kh < 1 || kw < 1 || stride_h < 1 || stride_w < 1 || pad_h < 0 || pad_w < 0) return -1;
  const int64_t total = n * h * w * c;
  if (total >= (1LL << 31)) return -1;
  PoolGeo q{(int)h, (int)w, (int)oh, (int)ow, (int)kh, (int)kw, (int)stride_h, (int)stride_w, (int)pad_h, (int)pad_w};
  // (a variant that issued the slab loads of all matching windows before the first addition --
  // two dependent round trips instead of five -- was measured slower, 17.7 vs 13.4 us: 138 VGPRs
  // and 32 loads per match instead of 11)
  hipLaunchKernelGGL(k_maxpool_adjoint, dim3((unsigned)((total + HB - 1) / HB)), dim3(HB), 0,
                     (hipStream_t)stream, (float*)g, (const float*)gy_a, a_splits, (long long)a_slab,
                     (const float*)gy_b, b_splits, (long long)b_slab, (const int*)idx, (unsigned)total,
                     (unsigned)c, q);
  return (int)hipGetLastError();
}

int hf_pool_act_tangent_nhwc(void* out, int64_t out_ld, const void* slabs, int splits, int64_t slab_stride,
                             const void* v_b, const void* idx, const void* y_pool, int relu, int64_t n, int64_t h,
                             int64_t w, int64_t oh, int64_t ow, int64_t c, int dtype, void* stream) {
  return pool_act_tangent(out, out_ld, slabs, splits, slab_stride, v_b, idx, y_pool, relu, n, h, w, oh, ow, c, dtype,
                          stream, nullptr);
}

int hf_pool_bn_act_tangent_nhwc(void* out, int64_t out_ld, const void* slabs, int splits, int64_t slab_stride,
                                const void* a, const void* mean, const void* rstd, const void* w, const void* v_w,
                                const void* v_b, const void* idx, const void* y_pool, int relu, int64_t n, int64_t h,
                                int64_t w_, int64_t oh, int64_t ow, int64_t c, int dtype, void* stream) {
  if (!a || !mean || !rstd || !w) return HF_ERR_ARG;
  const PoolBn bn{(const float*)a, (const float*)mean, (const float*)rstd, (const float*)w, (const float*)v_w};
  return pool_act_tangent(out, out_ld, slabs, splits, slab_stride, v_b, idx, y_pool, relu, n, h, w_, oh, ow, c, dtype,
                          stream, &bn);
}

int hf_pool_act_adjoint_nhwc(void* ga, void* gb, int row_blocks, const void* gy, int gy_splits, int64_t gy_slab,
                             const void* idx, const void* y_pool, int relu, int64_t n, int64_t h, int64_t w,
                             int64_t oh, int64_t ow, int64_t c, int64_t kh, int64_t kw, int64_t stride_h,
                             int64_t stride_w, int64_t pad_h, int64_t pad_w, int dtype, void* stream) {
  return pool_act_adjoint(ga, nullptr, nullptr, gb, row_blocks, gy, gy_splits, gy_slab, idx, y_pool, relu, n, h, w, oh,
                          ow, c, kh, kw, stride_h, stride_w, pad_h, pad_w, dtype, stream, nullptr);
}

int hf_pool_bn_act_adjoint_nhwc(void* ga, void* g, void* gw, void* gb, int row_blocks, const void* gy, int gy_splits,
                                int64_t gy_slab, const void* a, const void* mean, const void* rstd, const void* w,
                                const void* idx, const void* y_pool, int relu, int64_t n, int64_t h, int64_t w_,
                                int64_t oh, int64_t ow, int64_t c, int64_t kh, int64_t kw, int64_t stride_h,
                                int64_t stride_w, int64_t pad_h, int64_t pad_w, int dtype, void* stream) {
  if (!a || !mean || !rstd || !w) return HF_ERR_ARG;
  const PoolBn bn{(const float*)a, (const float*)mean, (const float*)rstd, (const float*)w, nullptr};
  return pool_act_adjoint(ga, g, gw, gb, row_blocks, gy, gy_splits, gy_slab, idx, y_pool, relu, n, h, w_, oh, ow, c, kh,
                          kw, stride_h, stride_w, pad_h, pad_w, dtype, stream, &bn);
}

int hf_pool_bn_act_adjoint_reduce_nhwc(void* g, void* gw, void* gb, int row_blocks, const void* gy, int gy_splits,
                                       int64_t gy_slab, const void* a, const void* mean, const void* rstd, const void* w,
                                       const void* idx, const void* y_pool, int relu, int64_t n, int64_t h, int64_t w_,
                                       int64_t oh, int64_t ow, int64_t c, int64_t kh, int64_t kw, int64_t stride_h,
                                       int64_t stride_w, int64_t pad_h, int64_t pad_w, int dtype, void* stream) {
  if (!a || !mean || !rstd || !w) return HF_ERR_ARG;
  const PoolBn bn{(const float*)a, (const float*)mean, (const float*)rstd, (const float*)w, nullptr};
  return pool_act_adjoint(nullptr, g, gw, gb, row_blocks, gy, gy_splits, gy_slab, idx, y_pool, relu, n, h, w_, oh, ow, c,
                          kh, kw, stride_h, stride_w, pad_h, pad_w, dtype, stream, &bn, true);
}

int hf_linear_ce_head(void* g_feat, void* g_w, void* g_b, const void* t_feat, const void* feat, const void* w,
                      const void* v_w, const void* v_b, const void* p, double scale, int64_t rows,
                      int64_t features, int64_t classes, int dtype, void* stream) {
  if (dtype != HF_F32 || !g_feat || !g_w || !t_feat || !feat || !w || !v_w || !p) return -1;
  if (rows < 1 || rows > 4096 || classes < 1 || classes > 64 || features < 4 || features % 4 || features > 512)
    return -1;
  const size_t lds = (size_t)(2 * classes * features + HEAD_R * features + HEAD_R * classes) * sizeof(float);
  if (lds > 64 * 1024) return -1;  // W, V_W and the workgroup's rows must fit the default LDS allowance
  if (!al16(g_feat) || !al16(g_w) || !al16(t_feat) || !al16(feat) || !al16(w) || !al16(v_w)) return -1;
  const int ch = (int)((features / 4 + 63) / 64);
  const unsigned groups = (unsigned)((rows + HEAD_R - 1) / HEAD_R);
  hipStream_t s = (hipStream_t)stream;
#define HF_HEAD(CH)                                                                                        \
  hipLaunchKernelGGL((k_linear_ce_head<CH>), dim3(groups), dim3(HEAD_T), lds, s, (float*)g_feat,           \
                     (float*)g_w, (float*)g_b, (const float*)t_feat, (const float*)feat, (const float*)w,  \
                     (const float*)v_w, (const float*)v_b, (const float*)p, (float)scale, (int)rows,       \
                     (int)features, (int)classes)
  if (ch <= 1) HF_HEAD(1);
  else HF_HEAD(2);
#undef HF_HEAD
  return (int)hipGetLastError();
}

int hf_pool_ce_head(void* g, void* jv_out, const void* t, const void* p, double scale, int64_t n, int64_t hw,
                    int64_t k, int dtype, void* stream) {
  if (dtype != HF_F32 || !g || !t || !p || n < 1 || hw < 1 || k < 1 || k > 1024) return -1;
  if (n * hw * k >= (1LL << 31)) return -1;
  hipLaunchKernelGGL(k_pool_ce_head, dim3((unsigned)n), dim3(HB), 0, (hipStream_t)stream, (float*)g,
                     (float*)jv_out, (const float*)t, (const float*)p, (float)scale, (int)hw, (int)k);
  return (int)hipGetLastError();
}

int hf_flatten_nhwc_rows(void* out, int64_t out_ld, const void* in, int64_t in_ld, int64_t n, int64_t hw, int64_t c,
                         int dtype, void* stream) {
  unsigned tiles_p, tiles_c, blocks;
  if (!out || !in) return HF_ERR_ARG;
  if (const int rc = flatten_grid(n, hw, c, dtype, &tiles_p, &tiles_c, &blocks)) return rc;
  const int64_t lim = 1LL << 31;
  if (in_ld < c || in_ld % 4 || in_ld >= lim || out_ld < c * hw || out_ld >= lim) return HF_ERR_ARG;
  if (n * hw * in_ld >= lim || n * out_ld >= lim) return HF_ERR_ARG;
  if (!al16(in)) return HF_ERR_ALIGN;
  hipLaunchKernelGGL(k_flatten_rows, dim3(blocks), dim3(HB), 0, (hipStream_t)stream, (float*)out, (const float*)in,
                     (unsigned)out_ld, (unsigned)in_ld, (unsigned)hw, (unsigned)c, tiles_p, tiles_c);
  return (int)hipGetLastError();
}

int hf_unflatten_slabs_nhwc(void* out, const void* slabs, int splits, int64_t slab_stride, int64_t n, int64_t hw,
                            int64_t c, int dtype, void* stream) {
  unsigned tiles_p, tiles_c, blocks;
  if (!out || !slabs) return HF_ERR_ARG;
  if (const int rc = flatten_grid(n, hw, c, dtype, &tiles_p, &tiles_c, &blocks)) return rc;
  if (splits < 1 || splits > HF_POOL_ACT_MAX_SPLITS) return HF_ERR_ARG;
  if (n * c * hw >= (1LL << 31)) return HF_ERR_ARG;
  if (splits > 1 && slab_stride < n * c * hw) return HF_ERR_ARG;  // (slabs would overlap)
  if (!al16(out)) return HF_ERR_ALIGN;
  hipLaunchKernelGGL(k_unflatten_slabs, dim3(blocks), dim3(HB), 0, (hipStream_t)stream, (float*)out,
                     (const float*)slabs, splits, (long long)slab_stride, (unsigned)hw, (unsigned)c, tiles_p, tiles_c);
  return (int)hipGetLastError();
}

int hf_linear_ce_head_slabs(int64_t rows) { return rows < 1 ? 0 : (int)((rows + HEAD_R - 1) / HEAD_R); }

}  // extern "C"
