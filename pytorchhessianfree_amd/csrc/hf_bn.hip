// hf_bn.hip -- BatchNorm / bias (+ residual, + ReLU) as per-channel affine maps inside the curvature sweeps and the
// engine's own forward pass (gfx950): forward, tangent, adjoint; eval mode and train mode (batch statistics whose
// per-channel finalisation runs in the prologue of the launch that consumes it); the softmax-CE Hessian rows.
// Reference: what BackPACK's R-op / L-op differentiate through, hessianfree/optimizer.py:450-462.
#include "hf_common.h"

namespace {

// ---------------------------------------------------------------------------
// eval-mode BatchNorm (+ residual add, + ReLU) as a per-channel affine map, fused
// (curvature-product path).   xhat = (x - mean[c]) * rstd[c]
//   k_chan_affine     : t = a*(w[c]*rstd[c]) + xhat*q[c] + r[c] + add   (each term optional)
//                       out = relu_self ? max(t, 0) : (mask_src ? (mask_src > 0 ? t : 0) : t)
//       forward  y = act(xhat*w + b + res)      (q = w, r = b, add = res, relu_self)
//       tangent / transpose of the backward map (a = v_gx, q = v_gw, r = v_gb,
//                                                add = v_gres, mask_src = y)
//   k_chan_affine_bwd : g = mask_src ? gy*(mask_src > 0) : gy
//                       gx = g*w[c]*rstd[c] ; gw[c] = sum g*xhat ; gb[c] = sum g ; gres = g
// One launch each instead of the ~16 small ATen kernels autograd's generic
// double-backward of batch_norm (+2 for the add, +2 for the ReLU) issues per layer
// and product.  NCHW-contiguous.
// ---------------------------------------------------------------------------
// I = unsigned (tensors < 2^31 elements: 32-bit index arithmetic, the per-element
// division is what these tiny kernels spend their time on) or long long.
template <typename T, typename I>
__device__ __forceinline__ void chan_affine_body(
    T* __restrict__ out, const T* __restrict__ a, const T* __restrict__ x,
    const T* __restrict__ mean, const T* __restrict__ rstd, const T* __restrict__ w,
    const T* __restrict__ q, const T* __restrict__ r, const T* __restrict__ add,
    const T* __restrict__ mask_src, int relu_self, I total, I C, I HW, int nhwc, I out_ld,
    I add_ld, int a_splits, long long a_slab, I bid, I nblocks) {
  // out_ld / add_ld != 0: that operand is the first-C-channels slice of a wider buffer --
  // NHWC: element (row, c) at row*ld + c; NCHW: (n, c, hw) at n*ld + c*HW + hw.
  const I CHW = C * HW;
  for (I i = bid * BLOCK + threadIdx.x; i < total; i += nblocks * BLOCK) {
    const I c = (nhwc || HW == 1 ? i : i / HW) % C;  // NHWC: the channel is the fastest index
    const T rs = rstd ? rstd[c] : (T)1;  // (no BatchNorm: conv + bias layers of plain stacks)
    T acc = (T)0;
    if (a) {
      const T av = slab_sum<8>(a[i], a, i, a_splits, a_slab);  // split-K slabs: eight loads in flight
      acc = av * ((w ? w[c] : (T)1) * rs);
    }
    if (q) acc += ((x[i] - mean[c]) * rs) * q[c];
    if (r) acc += r[c];
    I outer = 0;
    if (out_ld | add_ld) outer = nhwc ? i / C : i / CHW;  // row resp. sample
    if (add) acc += add[add_ld ? i + outer * (add_ld - (nhwc ? C : CHW)) : i];
    if (relu_self) acc = acc > (T)0 ? acc : (T)0;
    else if (mask_src) acc = mask_src[i] > (T)0 ? acc : (T)0;
    chain_store<HF_WT_ELEM>(&out[out_ld ? i + outer * (out_ld - (nhwc ? C : CHW)) : i], acc);
  }
}

// fp32 NHWC, C % 4 == 0, every operand 16-byte aligned: one 16-byte channel quad per thread, and EVERY load
// of the quad -- per-channel vectors, x / add / mask, up to 17 split-K slabs -- issued before the first use.
// These launches move a few MB and take ~5 us: what they cost is dependent round trips (~0.6 us each from the
// memory-side cache the producer's slabs sit in), not bytes; the scalar walk above paid one per slab batch of
// eight, one for w[c], one for x / q / r, one for add, one for the mask.  Same expressions, same order of
// additions: bitwise the scalar walk's results.
__device__ __forceinline__ void chan_affine_v4_body(
    float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ w,
    const float* __restrict__ q, const float* __restrict__ r, const float* __restrict__ add,
    const float* __restrict__ mask_src, int relu_self, unsigned total, unsigned C, unsigned out_ld,
    unsigned add_ld, int a_splits, long long a_slab, unsigned bid, unsigned nblocks) {
  const unsigned quads = total >> 2;
  for (unsigned v = bid * BLOCK + threadIdx.x; v < quads; v += nblocks * BLOCK) {
    const unsigned i = v << 2;
    const unsigned row = i / C, c = i - row * C;
    F4 rs4, w4, q4, r4, mu4, xv, addv, mv, av;
    if (rstd) rs4 = ld4(rstd + c);
    if (w) w4 = ld4(w + c);
    if (q) { q4 = ld4(q + c); mu4 = ld4(mean + c); xv = ld4(x + i); }
    if (r) r4 = ld4(r + c);
    if (add) addv = ld4(add + (add_ld ? row * add_ld + c : i));
    if (mask_src && !relu_self) mv = ld4(mask_src + i);
    if (a) av = slab_sum<16>(ld4(a + i), a, i, a_splits, a_slab);  // split-K slabs: sixteen loads in flight
    F4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float rs = rstd ? rs4.e[k] : 1.f;
      float acc = 0.f;
      if (a) acc = av.e[k] * ((w ? w4.e[k] : 1.f) * rs);
      if (q) acc += ((xv.e[k] - mu4.e[k]) * rs) * q4.e[k];
      if (r) acc += r4.e[k];
      if (add) acc += addv.e[k];
      if (relu_self) acc = acc > 0.f ? acc : 0.f;
      else if (mask_src) acc = mv.e[k] > 0.f ? acc : 0.f;
      o.e[k] = acc;
    }
    chain_store4<HF_WT_ELEM>(out + (out_ld ? row * out_ld + c : i), o);
  }
}

__global__ __launch_bounds__(BLOCK) void k_chan_affine_v4(
    float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ w,
    const float* __restrict__ q, const float* __restrict__ r, const float* __restrict__ add,
    const float* __restrict__ mask_src, int relu_self, unsigned total, unsigned C, unsigned out_ld,
    unsigned add_ld, int a_splits, long long a_slab) {
  chan_affine_v4_body(out, a, x, mean, rstd, w, q, r, add, mask_src, relu_self, total, C, out_ld, add_ld, a_splits,
                      a_slab, blockIdx.x, gridDim.x);
}

template <typename T, typename I>
__global__ __launch_bounds__(BLOCK) void k_chan_affine(
    T* __restrict__ out, const T* __restrict__ a, const T* __restrict__ x,
    const T* __restrict__ mean, const T* __restrict__ rstd, const T* __restrict__ w,
    const T* __restrict__ q, const T* __restrict__ r, const T* __restrict__ add,
    const T* __restrict__ mask_src, int relu_self, I total, I C, I HW, int nhwc, I out_ld,
    I add_ld, int a_splits, long long a_slab) {
  chan_affine_body<T, I>(out, a, x, mean, rstd, w, q, r, add, mask_src, relu_self, total, C, HW, nhwc, out_ld,
                         add_ld, a_splits, a_slab, (I)blockIdx.x, (I)gridDim.x);
}

// Two independent layers (a residual block's first BatchNorm and its downsample branch's) in ONE
// launch: the first `blocks_a` workgroups run problem A.  fp32, 32-bit indices.
struct AffArgs {
  float* out;
  const float *a, *x, *mean, *rstd, *w, *q, *r, *add, *mask_src;
  int relu_self;
  unsigned total, C, HW;
  int nhwc;
  unsigned out_ld, add_ld;
  int a_splits;
  long long a_slab;
  int vec4;  // eligible for the quad-per-thread walk (alignment checked on the host)
};

__global__ __launch_bounds__(BLOCK) void k_chan_affine_pair(const AffArgs A, const AffArgs B, unsigned blocks_a) {
  const bool first = blockIdx.x < blocks_a;
  const AffArgs& p = first ? A : B;
  if (p.vec4) {
    chan_affine_v4_body(p.out, p.a, p.x, p.mean, p.rstd, p.w, p.q, p.r, p.add, p.mask_src, p.relu_self, p.total,
                        p.C, p.out_ld, p.add_ld, p.a_splits, p.a_slab, first ? blockIdx.x : blockIdx.x - blocks_a,
                        first ? blocks_a : gridDim.x - blocks_a);
    return;
  }
  chan_affine_body<float, unsigned>(p.out, p.a, p.x, p.mean, p.rstd, p.w, p.q, p.r, p.add, p.mask_src, p.relu_self,
                                    p.total, p.C, p.HW, p.nhwc, p.out_ld, p.add_ld, p.a_splits, p.a_slab,
                                    first ? blockIdx.x : blockIdx.x - blocks_a,
                                    first ? blocks_a : gridDim.x - blocks_a);
}

// One channel per GROUP of TPC threads (TPC = 64: one wave per channel, 4 channels
// per block, no LDS / barrier -- for the late layers where a channel has only
// N*HW <= 256 elements; TPC = 256: one block per channel).
template <typename T, typename I, int TPC>
__global__ __launch_bounds__(BLOCK) void k_chan_affine_bwd(
    T* __restrict__ gx, T* __restrict__ gw, T* __restrict__ gb, T* __restrict__ gres,
    const T* __restrict__ gy, const T* __restrict__ gy2, const T* __restrict__ x,
    const T* __restrict__ mean, const T* __restrict__ rstd, const T* __restrict__ w,
    const T* __restrict__ mask_src, I N, I C, I HW, int s1 = 1, long long l1 = 0, int s2 = 1,
    long long l2 = 0) {
  __shared__ double lds[2 * WAVES];
  constexpr int GROUPS = BLOCK / TPC;
  const I c = (I)blockIdx.x * GROUPS + threadIdx.x / TPC;
  const int lane = threadIdx.x % TPC;
  const bool live = c < C;
  double acc[2] = {0.0, 0.0};
  if (live) {
    const T rs = rstd ? rstd[c] : (T)1, mu = mean ? mean[c] : (T)0;
    const T s = (w ? w[c] : (T)1) * rs;
    const I per = N * HW;
    if (per <= (I)TPC) {
      // at most ONE element per lane (the 32-row maps of the last stage, whose cotangents arrive as ~32 slabs):
      // sixteen slabs in flight per pass -- one at a time is a dependent round trip per slab, ~5 us per launch
      if ((I)lane < per) {
        const I n = HW == 1 ? (I)lane : (I)lane / HW;
        const I idx = (n * C + c) * HW + ((I)lane - n * HW);
        T g = gy[idx], h = gy2 ? gy2[idx] : (T)0;
        const T m = mask_src ? mask_src[idx] : (T)1, xv = x ? x[idx] : (T)0;
        // (written out, not slab_sum<16>: through the helper the fp64 instantiations got 8-16 instructions more)
        for (int sp = 1; sp < s1; sp += 16) {
          T v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = gy[(long long)(sp + u < s1 ? sp + u : 0) * l1 + idx];
#pragma unroll
          for (int u = 0; u < 16; ++u) g += sp + u < s1 ? v[u] : (T)0;
        }
        if (gy2) {
          for (int sp = 1; sp < s2; sp += 16) {
            T v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = gy2[(long long)(sp + u < s2 ? sp + u : 0) * l2 + idx];
#pragma unroll
            for (int u = 0; u < 16; ++u) h += sp + u < s2 ? v[u] : (T)0;
          }
        }
        T gg = g;
        if (gy2) gg = gg + h;
        if (mask_src) gg = m > (T)0 ? gg : (T)0;
        if (gx) { const T o = gg * s; chain_store<HF_WT_ELEM>(&gx[idx], o); }
        if (gres) chain_store<HF_WT_ELEM>(&gres[idx], gg);
        if (x) acc[0] += (double)gg * (double)(T)((xv - mu) * rs);
        acc[1] += (double)gg;
      }
    } else {
    // ITER elements per thread with all loads issued before the first use (latency-bound)
    constexpr int ITER = 8;
    for (I e0 = lane; e0 < per; e0 += (I)TPC * ITER) {
      I idx[ITER];
      T g[ITER], h[ITER], xv[ITER], m[ITER];
#pragma unroll
      for (int t = 0; t < ITER; ++t) {
        const I e = e0 + (I)t * TPC;
        idx[t] = 0;
        if (e < per) {
          const I n = HW == 1 ? e : e / HW;
          idx[t] = (n * C + c) * HW + (e - n * HW);
          g[t] = gy[idx[t]];
          if (gy2) h[t] = gy2[idx[t]];
          if (mask_src) m[t] = mask_src[idx[t]];
          if (x) xv[t] = x[idx[t]];
        }
      }
      // split-K slabs, added in split order (batching eight slabs of every element per pass was measured: no
      // gain on these 32-row maps, 252 instead of 58 VGPRs)
#pragma unroll
      for (int t = 0; t < ITER; ++t) {
        if (e0 + (I)t * TPC < per) {
          // (depth 1, unpredicated, written out: slab_sum<1> laid these loops out with 13-36 instructions more)
          for (int sp = 1; sp < s1; ++sp) g[t] += gy[(long long)sp * l1 + idx[t]];
          if (gy2)
            for (int sp = 1; sp < s2; ++sp) h[t] += gy2[(long long)sp * l2 + idx[t]];
        }
      }
#pragma unroll
      for (int t = 0; t < ITER; ++t) {
        if (e0 + (I)t * TPC < per) {
          T gg = g[t];
          if (gy2) gg = gg + h[t];  // the cotangents of the output's two consumers
          if (mask_src) gg = m[t] > (T)0 ? gg : (T)0;
          if (gx) { const T o = gg * s; chain_store<HF_WT_ELEM>(&gx[idx[t]], o); }
          if (gres) chain_store<HF_WT_ELEM>(&gres[idx[t]], gg);
          if (x) acc[0] += (double)gg * (double)(T)((xv[t] - mu) * rs);
          acc[1] += (double)gg;
        }
      }
    }
    }
  }
  if (TPC == 64) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      acc[0] += __shfl_down(acc[0], off, 64);
      acc[1] += __shfl_down(acc[1], off, 64);
    }
  } else {
    block_allreduce<2>(acc, lds);
  }
  if (live && lane == 0) {
    if (gw) { const T sw = (T)acc[0]; chain_store<HF_WT_ELEM>(&gw[c], sw); }
    if (gb) { const T sb = (T)acc[1]; chain_store<HF_WT_ELEM>(&gb[c], sb); }
  }
}

// first + slabs 1..n-1 of a W-wide column, eight loads in flight, added in split order.  (k_chan_affine_bwd_nhwc's own
// copy of hf_common.h's slab_sum<8, true>: with that one the W = 4 kernels, which keep SGPRs in VGPR lanes, came out
// 44-101 instructions longer)
template <typename T, typename Col, int W>
__device__ __forceinline__ Col col_slab_sum(Col first, const T* p, int n, long long stride) {
  for (int sp = 1; sp < n; sp += 8) {
    Col v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int q = sp + u < n ? sp + u : 0;  // slab 0 is valid memory; its value is discarded
      v[u] = *reinterpret_cast<const Col*>(p + (long long)q * stride);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (sp + u < n) {
#pragma unroll
        for (int k = 0; k < W; ++k) first.e[k] += v[u].e[k];
      }
    }
  }
  return first;
}

// NHWC variant: element (row, c) at row*C + c, row = n*HW + hw.  A block owns W
// adjacent channels (W = 4: one 16-byte column) and spreads the rows over its 256
// threads, so the per-channel sums need no cross-block step (deterministic, no
// workspace) and C/W blocks are in flight; the tensors of this path are a few MB
// and L2-resident, the strided 16-byte reads cost less than a second launch would.
template <typename T, typename I, int W, int BS>
__global__ __launch_bounds__(BS) void k_chan_affine_bwd_nhwc(
    T* __restrict__ gx, T* __restrict__ gw, T* __restrict__ gb, T* __restrict__ gres,
    const T* __restrict__ gy, const T* __restrict__ gy2, const T* __restrict__ x,
    const T* __restrict__ mean, const T* __restrict__ rstd, const T* __restrict__ w,
    const T* __restrict__ mask_src, I rows, I C, int s1 = 1, long long l1 = 0, int s2 = 1,
    long long l2 = 0, int row_blocks = 1) {
  __shared__ double lds[2 * W * (BS / 64)];
  using Col = ColOf<T, W>;
  // row_blocks > 1: block (q, rb) owns channel column q and the rb-th share of the rows and
  // writes its per-channel partial sums to gw/gb + rb*C (hf_pack_ex adds the shares up)
  const I cq = (I)blockIdx.x % (C / W), rb = (I)blockIdx.x / (C / W);
  const I c0 = cq * W;
  const I rpb = (rows + (I)row_blocks - 1) / (I)row_blocks;
  const I row_lo = rb * rpb, row_hi = (row_lo + rpb < rows) ? row_lo + rpb : rows;
  T rs[W], mu[W], sc[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    rs[k] = rstd ? rstd[c0 + k] : (T)1;
    mu[k] = mean ? mean[c0 + k] : (T)0;
    sc[k] = (w ? w[c0 + k] : (T)1) * rs[k];
  }
  double acc[2 * W];
#pragma unroll
  for (int k = 0; k < 2 * W; ++k) acc[k] = 0.0;
  // rows are visited ITER at a time with all loads issued before the first use: these
  // activation-sized kernels are latency-bound, one round trip per 8 rows instead of one each
  constexpr int ITER = 8;
  for (I r0 = row_lo + threadIdx.x; r0 < row_hi; r0 += (I)BS * ITER) {
    Col g[ITER], h[ITER], xv[ITER], m[ITER];
#pragma unroll
    for (int t = 0; t < ITER; ++t) {
      const I r = r0 + (I)t * BS;
      if (r < row_hi) {
        const I idx = r * C + c0;
        // every first load is issued before any slab is summed (a sum waits for its loads)
        g[t] = *reinterpret_cast<const Col*>(gy + idx);
        if (gy2) h[t] = *reinterpret_cast<const Col*>(gy2 + idx);
        if (x) xv[t] = *reinterpret_cast<const Col*>(x + idx);
        if (mask_src) m[t] = *reinterpret_cast<const Col*>(mask_src + idx);
      }
    }
    if (s1 > 1 || s2 > 1) {
#pragma unroll
      for (int t = 0; t < ITER; ++t) {
        const I r = r0 + (I)t * BS;
        if (r < row_hi) {
          const I idx = r * C + c0;
          // split-K slabs: batches of eight, the last one predicated instead of a one-by-one tail (a tail of
          // dependent load-add pairs costs a round trip each)
          if (s1 > 1) g[t] = col_slab_sum<T, Col, W>(g[t], gy + idx, s1, l1);
          if (gy2 && s2 > 1) h[t] = col_slab_sum<T, Col, W>(h[t], gy2 + idx, s2, l2);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < ITER; ++t) {
      const I r = r0 + (I)t * BS;
      if (r < row_hi) {
        const I idx = r * C + c0;
        if (gy2) {
#pragma unroll
          for (int k = 0; k < W; ++k) g[t].e[k] = g[t].e[k] + h[t].e[k];
        }
        if (mask_src) {
#pragma unroll
          for (int k = 0; k < W; ++k) g[t].e[k] = m[t].e[k] > (T)0 ? g[t].e[k] : (T)0;
        }
        if (gres) chain_store_col<HF_WT_ELEM>(gres + idx, g[t]);
        if (gx) {
          Col o;
#pragma unroll
          for (int k = 0; k < W; ++k) o.e[k] = g[t].e[k] * sc[k];
          chain_store_col<HF_WT_ELEM>(gx + idx, o);
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
          if (x) acc[2 * k] += (double)g[t].e[k] * (double)(T)((xv[t].e[k] - mu[k]) * rs[k]);
          acc[2 * k + 1] += (double)g[t].e[k];
        }
      }
    }
  }
  block_allreduce<2 * W, BS / 64>(acc, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if (gw) { const T sw = (T)acc[2 * k]; chain_store<HF_WT_ELEM>(&gw[rb * C + c0 + k], sw); }
      if (gb) { const T sb = (T)acc[2 * k + 1]; chain_store<HF_WT_ELEM>(&gb[rb * C + c0 + k], sb); }
    }
  }
}

// Cross-row sums of a ROW-MAJOR thread map (thread (ty, tx) = (threadIdx.x / quads, threadIdx.x % quads), ty < RP, holds
// eight sums of its rows in acc): red[k][ty][tx] (consecutive lanes -> consecutive words: no bank conflicts), then
// 8*quads threads each add one (k, tx) column over ty in a fixed order and hand it to sink(k, tx, sum).  (The first
// version let the `quads` threads of ty == 0 walk all 8 sums serially: 8*RP dependent LDS reads per thread behind
// 8-way bank conflicts -- 72 % of the adjoint kernel's LDS cycles were conflict cycles,
// profiles/r03_engine_kernel_counters.json.)  Same summation order, bitwise the same sums.
// Contract: a BLOCK-thread workgroup calls it with all its threads and passes its own map (tx, ty, live == ty < RP;
// RP * quads <= BLOCK, threads that are not live hold nothing); red holds 8 * RP * quads <= 8 * BLOCK doubles and must
// be free on entry.  There is one barrier, between the stores and the column sums, and none at the end: a caller that
// reuses red, or reads from other threads what sink wrote, puts its own __syncthreads after the call.
template <typename Sink>
__device__ __forceinline__ void cross_row_sums(const double (&acc)[8], double* red, unsigned RP, unsigned quads,
                                               unsigned tx, unsigned ty, bool live, Sink&& sink) {
  if (live) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[(k * RP + ty) * quads + tx] = acc[k];
  }
  __syncthreads();
  for (unsigned idx = threadIdx.x; idx < 8 * quads; idx += BLOCK) {
    const unsigned k = idx / quads, col = idx - k * quads;
    double sum = 0.0;
    for (unsigned t = 0; t < RP; ++t) sum += red[(k * RP + t) * quads + col];  // fixed order over ty
    sink(k, col, sum);
  }
}

// BatchNorm adjoint, NHWC fp32, ROW-MAJOR thread map: thread (ty, tx) owns the 16-byte channel
// column tx of rows ty, ty + RP, ... of its block's row share, so that a wave reads whole
// contiguous rows (the column-per-block kernel above reads 16 bytes every C*4 bytes: one cache
// line per lane).  Per-channel sums: per thread over its rows, then over ty through LDS in a
// fixed order; every block writes its partial sums to gw / gb + blockIdx.x*C (hf_pack_ex adds
// the row shares up).  Cotangents may arrive as split-K slabs.
__device__ __forceinline__ void bn_adjoint_rows_body(
    float* __restrict__ gx, float* __restrict__ gw, float* __restrict__ gb, float* __restrict__ gres,
    const float* __restrict__ gy, int s1, long long l1, const float* __restrict__ gy2, int s2, long long l2,
    const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ w, const float* __restrict__ mask_src, unsigned rows, unsigned C,
    unsigned rows_per_block, unsigned bid, double* red) {
  const unsigned quads = C / 4, RP = BLOCK / quads;
  const unsigned tx = threadIdx.x % quads, ty = threadIdx.x / quads;
  const unsigned c0 = tx * 4;
  const bool live = ty < RP;
  float rs[4], mu[4], sc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rs[k] = rstd ? rstd[c0 + k] : 1.f;
    mu[k] = mean ? mean[c0 + k] : 0.f;
    sc[k] = (w ? w[c0 + k] : 1.f) * rs[k];
  }
  double acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.0;
  const unsigned row_lo = bid * rows_per_block;
  const unsigned row_hi = row_lo + rows_per_block < rows ? row_lo + rows_per_block : rows;
  if (live) {
    // two rows per pass: their first loads and their slab batches are all in flight together
    for (unsigned r = row_lo + ty; r < row_hi; r += 2 * RP) {
      const bool two = r + RP < row_hi;
      const unsigned idx0 = r * C + c0, idx1 = (two ? r + RP : r) * C + c0;
      F4 g0 = ld4(gy + idx0), g1 = ld4(gy + idx1);
      F4 h0, h1, x0, x1, m0, m1;
      if (gy2) { h0 = ld4(gy2 + idx0); h1 = ld4(gy2 + idx1); }
      if (x) { x0 = ld4(x + idx0); x1 = ld4(x + idx1); }
      if (mask_src) { m0 = ld4(mask_src + idx0); m1 = ld4(mask_src + idx1); }
      // split-K slabs of both rows and both cotangents: one loop, 8 slabs x up to 4 columns in flight per
      // pass (each column still adds its slabs in split order: bitwise the one-column-at-a-time sums, which
      // cost a round trip per column and batch)
      // (sixteen slabs x two columns per pass was measured slower: 272 VGPRs; the first batch as straight-line code
      // behind the row loads with its first addition pinned behind its last load -- 43 loads before the first wait, 256
      // VGPRs -- measured +0.5 % on ResNet-18, -1.5 % on All-CNN-C's large maps: profiles/r04_rows_straight_rejected.jsonl)
      const int smax = (gy2 && s2 > s1) ? s2 : s1;
      for (int sp = 1; sp < smax; sp += 8) {
        // (written out, not slab_issue / slab_add: those issue one row's eight loads back to back, this loop the two rows'
        // loads of a slab next to each other -- another load order, 4 VGPRs and 58 instructions more)
        F4 vg0[8], vg1[8], vh0[8], vh1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const long long o1 = (long long)(sp + u < s1 ? sp + u : 0) * l1;
          vg0[u] = ld4(gy + o1 + idx0);
          vg1[u] = ld4(gy + o1 + idx1);
        }
        if (gy2 && s2 > 1) {
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const long long o2 = (long long)(sp + u < s2 ? sp + u : 0) * l2;
            vh0[u] = ld4(gy2 + o2 + idx0);
            vh1[u] = ld4(gy2 + o2 + idx1);
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (sp + u < s1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { g0.e[k] += vg0[u].e[k]; g1.e[k] += vg1[u].e[k]; }
          }
        }
        if (gy2 && s2 > 1) {
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (sp + u < s2) {
#pragma unroll
              for (int k = 0; k < 4; ++k) { h0.e[k] += vh0[u].e[k]; h1.e[k] += vh1[u].e[k]; }
            }
          }
        }
      }
      F4 o0, o1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float a0 = gy2 ? g0.e[k] + h0.e[k] : g0.e[k], a1 = gy2 ? g1.e[k] + h1.e[k] : g1.e[k];
        if (mask_src) { a0 = m0.e[k] > 0.f ? a0 : 0.f; a1 = m1.e[k] > 0.f ? a1 : 0.f; }
        g0.e[k] = a0; g1.e[k] = a1;
        o0.e[k] = a0 * sc[k]; o1.e[k] = a1 * sc[k];
        if (x) acc[2 * k] += (double)a0 * (double)(float)((x0.e[k] - mu[k]) * rs[k]);
        acc[2 * k + 1] += (double)a0;
        if (two) {
          if (x) acc[2 * k] += (double)a1 * (double)(float)((x1.e[k] - mu[k]) * rs[k]);
          acc[2 * k + 1] += (double)a1;
        }
      }
      if (gres) { chain_store4<HF_WT_ELEM>(gres + idx0, g0); if (two) chain_store4<HF_WT_ELEM>(gres + idx1, g1); }
      if (gx) { chain_store4<HF_WT_ELEM>(gx + idx0, o0); if (two) chain_store4<HF_WT_ELEM>(gx + idx1, o1); }
    }
  }
  cross_row_sums(acc, red, RP, quads, tx, ty, live, [&](unsigned k, unsigned col, double sum) {
    float* dst = (k & 1) ? gb : gw;
    if (dst) { const float v = (float)sum; chain_store<HF_WT_ELEM>(&dst[bid * C + col * 4 + (k >> 1)], v); }
  });
}

__global__ __launch_bounds__(BLOCK) void k_bn_adjoint_rows(
    float* __restrict__ gx, float* __restrict__ gw, float* __restrict__ gb, float* __restrict__ gres,
    const float* __restrict__ gy, int s1, long long l1, const float* __restrict__ gy2, int s2, long long l2,
    const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ w, const float* __restrict__ mask_src, unsigned rows, unsigned C,
    unsigned rows_per_block) {
  __shared__ double red[BLOCK * 8];
  bn_adjoint_rows_body(gx, gw, gb, gres, gy, s1, l1, gy2, s2, l2, x, mean, rstd, w, mask_src, rows, C,
                       rows_per_block, blockIdx.x, red);
}

// Both column sums in one pass (all loads of both partial-row sets in flight together).  scratch: 8 * BLOCK doubles.
// `between()` runs right after the first batch of partial-row loads is issued: the caller's own independent loads go
// there, so that one round trip covers both.
// HF_FCS_BATCH: how many partial rows of each set a thread keeps in flight per round trip.  The rows come out of the
// memory-side cache (~0.6-1 us per dependent round trip); the consumers of a train-mode BatchNorm add up 64 ... 256 rows
// per channel, i.e. 16 ... 32 per thread: 4 per batch = 4 ... 8 dependent round trips in the prologue of a launch that
// otherwise takes ~4.6 us.  The order of the additions does not depend on it (bitwise the same sums).  Measured, same box
// (profiles/r06_fcs_batch_ab.jsonl, bench.py --bn train): 4 -> 1 174 / 1 190, 8 -> 1 211 / 1 208, 16 -> 1 201 / 1 202
// matvecs/s.  (A column-blocked workgroup mapping -- 64 rows x 16 channels, a quarter ... a 32nd of the redundant
// partial-row traffic and one round trip -- was built and measured at NO gain: 1 196-1 199 against 1 200,
// profiles/r06_colblock_rejected.jsonl; removed.)
#ifndef HF_FCS_BATCH
#define HF_FCS_BATCH 8
#endif
template <typename Between>
__device__ __forceinline__ void final_column_sums2(const float* __restrict__ rows_a, const float* __restrict__ rows_b,
                                                   unsigned nrows, unsigned C, double* scratch, double* out_a,
                                                   double* out_b, Between&& between) {
  const unsigned quads = C / 4, G = BLOCK / quads;
  const unsigned tx = threadIdx.x % quads, ty = threadIdx.x / quads;
  const bool live = ty < G;
  double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  constexpr int NB = HF_FCS_BATCH;  // partial rows of each set in flight per thread and round trip
  F4 va[NB], vb[NB];
  auto issue = [&](unsigned p0) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const unsigned p = p0 + u * G < nrows ? p0 + u * G : 0u;
      va[u] = ld4(rows_a + (size_t)p * C + 4 * tx);
      vb[u] = ld4(rows_b + (size_t)p * C + 4 * tx);
    }
  };
  auto add = [&](unsigned p0) {  // NB partial rows of each set, added in row order
#pragma unroll
    for (int u = 0; u < NB; ++u)
      if (p0 + u * G < nrows) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] += (double)va[u].e[k]; a[4 + k] += (double)vb[u].e[k]; }
      }
  };
  const bool first = live && ty < nrows;
  issue(ty);  // (unconditional, out-of-range rows read row 0: a branch here makes the compiler shuffle -- and wait for --
              // the loaded registers at its join)
  between();
  if (first) {
    // (pins the first use of the rows BEHIND the caller's loads: without it the compiler adds them up -- and waits
    // for them -- before it issues those)
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      asm volatile("" : "+v"(va[u].e[0]), "+v"(va[u].e[1]), "+v"(va[u].e[2]), "+v"(va[u].e[3]) : : "memory");
      asm volatile("" : "+v"(vb[u].e[0]), "+v"(vb[u].e[1]), "+v"(vb[u].e[2]), "+v"(vb[u].e[3]) : : "memory");
    }
    add(ty);
  }
  if (live) {
    for (unsigned p0 = ty + NB * G; p0 < nrows; p0 += NB * G) { issue(p0); add(p0); }
    // (cross_row_sums written out: its stores belong into this `if (live)`; as a call behind it the train kernels changed)
#pragma unroll
    for (int k = 0; k < 8; ++k) scratch[(k * G + ty) * quads + tx] = a[k];
  }
  __syncthreads();
  for (unsigned idx = threadIdx.x; idx < 8 * quads; idx += BLOCK) {
    const unsigned k = idx / quads, col = idx - k * quads;
    double sum = 0.0;
    for (unsigned t = 0; t < G; ++t) sum += scratch[(k * G + t) * quads + col];
    (k < 4 ? out_a : out_b)[col * 4 + (k & 3)] = sum;
  }
  __syncthreads();
}

// ---- train-mode BatchNorm: the per-channel finalisation in the CONSUMER's prologue ---------------------------
// k_chan_affine_v4 whose workgroups first add the reduction launch's partial rows up themselves (plain loads: the
// rows come from the PREVIOUS launch; every workgroup the same fixed order, so the same q / r everywhere) --
//   q = vq - w*rstd*S_x/m,  r = vr - w*rstd*S_1/m,  then  out = mask(a*(w*rstd) + xhat*q + r + add).
// The redundant sums cost each workgroup one more round trip (nparts * C * 8 bytes out of L2); the finalisation as the
// reduction launch's tail would cost a ticket, a drain and a one-workgroup re-read, as its own launch a launch boundary
// more.
struct AffTrainArgs {
  float* out;
  const float *a, *x, *mean, *rstd, *w, *part_x, *part_1;
  unsigned nparts;
  const float *vq, *vr;
  float inv_m;
  const float *add, *mask_src;
  unsigned total, C, out_ld, add_ld;
  int a_splits;
  long long a_slab;
};

template <bool SLABS, bool ADD, bool MASK>
__device__ __forceinline__ void affine_train_body(const AffTrainArgs& p, unsigned bid, unsigned nblocks,
                                                  double* scratch, double* fin, float* qs, float* rsh) {
  const float* __restrict__ a = p.a;
  const float* __restrict__ x = p.x;
  const float* __restrict__ mean = p.mean;
  const float* __restrict__ rstd = p.rstd;
  const float* __restrict__ w = p.w;
  const float* __restrict__ add = p.add;
  const float* __restrict__ mask_src = p.mask_src;
  float* __restrict__ out = p.out;
  const unsigned total = p.total, C = p.C, out_ld = p.out_ld, add_ld = p.add_ld;
  const int a_splits = p.a_splits;
  const long long a_slab = p.a_slab;
  // this thread's element quad: every load of it issued right behind the first partial-row loads and BEFORE those are
  // added up (none depends on the sums): one round trip for both
  const unsigned quads_total = total >> 2;
  const unsigned v = bid * BLOCK + threadIdx.x;
  const bool have = v < quads_total;
  const unsigned i = v << 2;
  const unsigned row = i / C, c = i - row * C;
  F4 rs4, w4, mu4, xv, addv, mv, av, t[16];
  final_column_sums2(p.part_x, p.part_1, p.nparts, C, scratch, fin, fin + 4 * BLOCK, [&]() {
    // (no run-time branches around these loads -- optional operands are template flags, threads past the end read
    // element 0: at a branch's join the compiler copies the loaded registers, which waits for them right here)
    const unsigned ii = have ? i : 0u, cc = have ? c : 0u, rr = have ? row : 0u;
    rs4 = ld4(rstd + cc);
    mu4 = ld4(mean + cc);
    xv = ld4(x + ii);
    w4 = ld4(w + cc);
    if (ADD) addv = ld4(add + (add_ld ? rr * add_ld + cc : ii));
    if (MASK) mv = ld4(mask_src + ii);
    av = ld4(a + ii);
    if (SLABS) {  // the first batch: added behind the finalisation.  (This and the loop below are written out: through
                  // slab_issue / slab_add the slab variants of the train kernels came out 42-99 instructions shorter)
#pragma unroll
      for (int u = 0; u < 16; ++u) t[u] = ld4(a + (long long)(1 + u < a_splits ? 1 + u : 0) * a_slab + ii);
    }
  });
  for (unsigned ch = threadIdx.x; ch < C; ch += BLOCK) {
    const float k = w[ch] * rstd[ch] * p.inv_m;
    qs[ch] = (p.vq ? p.vq[ch] : 0.f) - k * (float)fin[ch];
    rsh[ch] = (p.vr ? p.vr[ch] : 0.f) - k * (float)fin[4 * BLOCK + ch];
  }
  __syncthreads();
  if (have) {
    if (SLABS) {  // (slabs in split order, as chan_affine_v4_body)
#pragma unroll
      for (int u = 0; u < 16; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) av.e[k] += 1 + u < a_splits ? t[u].e[k] : 0.f;
      for (int sp = 17; sp < a_splits; sp += 16) {
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = ld4(a + (long long)(sp + u < a_splits ? sp + u : 0) * a_slab + i);
#pragma unroll
        for (int u = 0; u < 16; ++u)
#pragma unroll
          for (int k = 0; k < 4; ++k) av.e[k] += sp + u < a_splits ? t[u].e[k] : 0.f;
      }
    }
    F4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float rs = rs4.e[k];
      float acc = av.e[k] * (w4.e[k] * rs);
      acc += ((xv.e[k] - mu4.e[k]) * rs) * qs[c + k];
      acc += rsh[c + k];
      if (ADD) acc += addv.e[k];
      if (MASK) acc = mv.e[k] > 0.f ? acc : 0.f;
      o.e[k] = acc;
    }
    chain_store4<HF_WT_ELEM>(out + (out_ld ? row * out_ld + c : i), o);
  }
  // (a grid capped below one quad per thread: the rest by the plain walk)
  if (nblocks * BLOCK < quads_total)
    chan_affine_v4_body(out, a, x, mean, rstd, w, qs, rsh, add, mask_src, 0, total, C, out_ld, add_ld, a_splits,
                        a_slab, bid + nblocks, nblocks);
}

template <bool SLABS, bool ADD, bool MASK>
__global__ __launch_bounds__(BLOCK) void k_chan_affine_v4_train(const AffTrainArgs p) {
  __shared__ double scratch[8 * BLOCK];
  __shared__ double fin[2 * 4 * BLOCK];
  __shared__ float qs[4 * BLOCK], rsh[4 * BLOCK];
  affine_train_body<SLABS, ADD, MASK>(p, blockIdx.x, gridDim.x, scratch, fin, qs, rsh);
}

// Two independent train-mode layers (a residual block's first BatchNorm and its downsample branch's) in ONE launch:
// the first `blocks_a` workgroups run problem A.  No residual operand in either (template flags: slabs / mask of A, B).
template <bool SA, bool MA, bool SB, bool MB>
__global__ __launch_bounds__(BLOCK) void k_chan_affine_v4_train_pair(const AffTrainArgs A, const AffTrainArgs B,
                                                                     unsigned blocks_a) {
  __shared__ double scratch[8 * BLOCK];
  __shared__ double fin[2 * 4 * BLOCK];
  __shared__ float qs[4 * BLOCK], rsh[4 * BLOCK];
  if (blockIdx.x < blocks_a) affine_train_body<SA, false, MA>(A, blockIdx.x, blocks_a, scratch, fin, qs, rsh);
  else affine_train_body<SB, false, MB>(B, blockIdx.x - blocks_a, gridDim.x - blocks_a, scratch, fin, qs, rsh);
}

// ---- a plain stack's POOLED train-mode BatchNorm unit: the tangent at the windows' positions ----------------------------
// k_chan_affine_v4_train's prologue (the same partial rows added in the same order: the same q / r in every workgroup),
// then hf_head.hip's pooled BatchNorm tangent with q / r in place of v_w / v_b: with p = idx[n,oy,ox,c]
//   out[n,oy,ox,c] = m * (T[p]*(w*rstd) + xhat[p]*q + r),   T[p]: the tangent convolution's slabs at p, in split order
// -- bitwise the train kernel's unmasked dense output gathered at idx; the full-resolution tangent is never formed (its
// sums S_x / S_1 came from the convolution's epilogue or one reduction launch over the slabs).  A thread owns W consecutive
// channels of a pooled pixel (W = 4: 16-byte loads of idx / y_pool, 16-byte stores; W = 1: any alignment of those).
struct PoolTrainArgs {
  float* out;
  const float *slabs, *a, *mean, *rstd, *w, *part_x, *part_1, *vq, *vr, *ypool;
  const int* idx;
  unsigned nparts;
  float inv_m;
  unsigned items, CQ, out_ld, opix, ipix;
  int splits;
  long long slab_stride;
};

template <int W>
__global__ __launch_bounds__(BLOCK) void k_pool_bn_act_tangent_train(const PoolTrainArgs p) {
  __shared__ double scratch[8 * BLOCK];
  __shared__ double fin[2 * 4 * BLOCK];
  __shared__ float qs[4 * BLOCK], rsh[4 * BLOCK];
  using VF = ColOf<float, W>;
  using VI = ColOf<int, W>;
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  const bool have = v < p.items;
  const unsigned i = have ? v : 0u;  // (threads past the end read item 0 and store nothing: they serve the prologue)
  const unsigned C = p.CQ * W, cq = i % p.CQ, pix = i / p.CQ, n = pix / p.opix, c0 = cq * W;
  const unsigned e = pix * C + c0;
  const float* __restrict__ ypool = p.ypool;
  VI ix;
  VF m;
  final_column_sums2(p.part_x, p.part_1, p.nparts, C, scratch, fin, fin + 4 * BLOCK, [&]() {
    // the element's own first round trip (positions, mask) rides with the partial rows'
    ix = *reinterpret_cast<const VI*>(p.idx + e);
    if (ypool) m = *reinterpret_cast<const VF*>(ypool + e);
  });
  for (unsigned ch = threadIdx.x; ch < C; ch += BLOCK) {  // (k_chan_affine_v4_train's finalisation, to the letter)
    const float k = p.w[ch] * p.rstd[ch] * p.inv_m;
    qs[ch] = (p.vq ? p.vq[ch] : 0.f) - k * (float)fin[ch];
    rsh[ch] = (p.vr ? p.vr[ch] : 0.f) - k * (float)fin[4 * BLOCK + ch];
  }
  __syncthreads();
  if (!have) return;
  const float* __restrict__ slabs = p.slabs;
  VF s, av;
  unsigned off[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    // (a position outside the plane would be a read outside the slabs: clamped, never followed)
    const unsigned pos = (unsigned)ix.e[k] < p.ipix ? (unsigned)ix.e[k] : p.ipix - 1;
    off[k] = (n * p.ipix + pos) * C + c0 + k;
    s.e[k] = slabs[off[k]];
    av.e[k] = p.a[off[k]];
  }
  // (the W channels' slabs: one batch of all of them in flight, each channel added in split order)
  for (int sp = 1; sp < p.splits; sp += 8) {
    float t[W][8];
#pragma unroll
    for (int k = 0; k < W; ++k) slab_issue(t[k], slabs, off[k], sp, p.splits, p.slab_stride);
#pragma unroll
    for (int k = 0; k < W; ++k) slab_add<false>(s.e[k], t[k], sp, p.splits);
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const float rs = p.rstd[c0 + k];
    float acc = s.e[k] * (p.w[c0 + k] * rs);
    acc += ((av.e[k] - p.mean[c0 + k]) * rs) * qs[c0 + k];
    acc += rsh[c0 + k];
    if (ypool) acc = m.e[k] > 0.f ? acc : 0.f;
    s.e[k] = acc;
  }
  chain_store_col<HF_WT_ELEM>(p.out + (size_t)pix * p.out_ld + c0, s);
}

// One-pass batch statistics of a train-mode BatchNorm's forward: sums the convolution's split-K slabs into
// a_out (row-major walk as k_bn_adjoint_rows), per-channel sum a and sum a^2 in fp64 per thread / block.
// part: [gridDim.x, 2, C] doubles; the normalising launch (k_bn_forward_train) adds the rows up in its prologue:
// mean, biased variance = E[a^2] - mean^2 (fp64: 1e-16 * mean^2/var relative, far below fp32 for any layer a network
// can train), rstd, running statistics.
__global__ __launch_bounds__(BLOCK) void k_bn_stats_rows(
    float* __restrict__ a_out, const float* __restrict__ a, int splits, long long slab, double* part,
    unsigned rows, unsigned C, unsigned rows_per_block) {
  __shared__ double red[BLOCK * 8];
  const unsigned quads = C / 4, RP = BLOCK / quads;
  const unsigned tx = threadIdx.x % quads, ty = threadIdx.x / quads;
  const unsigned c0 = tx * 4;
  const bool live = ty < RP;
  double acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.0;
  const unsigned row_lo = blockIdx.x * rows_per_block;
  const unsigned row_hi = row_lo + rows_per_block < rows ? row_lo + rows_per_block : rows;
  if (live) {
    for (unsigned r = row_lo + ty; r < row_hi; r += RP) {
      const unsigned idx = r * C + c0;
      F4 v = ld4(a + idx);
      // (written out: slab_sum<8> cost this kernel two instructions more)
      for (int sp = 1; sp < splits; sp += 8) {  // eight slabs in flight, added in split order
        F4 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
          t[u] = ld4(a + (long long)(sp + u < splits ? sp + u : 0) * slab + idx);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int k = 0; k < 4; ++k) v.e[k] += sp + u < splits ? t[u].e[k] : 0.f;
      }
      if (a_out) *reinterpret_cast<F4*>(a_out + idx) = v;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        acc[2 * k] += (double)v.e[k];
        acc[2 * k + 1] += (double)v.e[k] * (double)v.e[k];
      }
    }
  }
  cross_row_sums(acc, red, RP, quads, tx, ty, live, [&](unsigned k, unsigned col, double sum) {
    part[((size_t)blockIdx.x * 2 + (k & 1)) * C + col * 4 + (k >> 1)] = sum;
  });
}

// Two independent layers' adjoints in ONE launch (see k_chan_affine_pair).
struct BnAdjArgs {
  float *gx, *gw, *gb, *gres;
  const float* gy;
  int s1;
  long long l1;
  const float* gy2;
  int s2;
  long long l2;
  const float *x, *mean, *rstd, *w, *mask_src;
  unsigned rows, C, rows_per_block;
};

__global__ __launch_bounds__(BLOCK) void k_bn_adjoint_rows_pair(const BnAdjArgs A, const BnAdjArgs B,
                                                                unsigned blocks_a) {
  __shared__ double red[BLOCK * 8];
  const bool first = blockIdx.x < blocks_a;
  const BnAdjArgs& p = first ? A : B;
  bn_adjoint_rows_body(p.gx, p.gw, p.gb, p.gres, p.gy, p.s1, p.l1, p.gy2, p.s2, p.l2, p.x, p.mean, p.rstd, p.w,
                       p.mask_src, p.rows, p.C, p.rows_per_block, first ? blockIdx.x : blockIdx.x - blocks_a, red);
}

// Adjoint pre-pass of a fused eval-BatchNorm(+add+ReLU) layer in NHWC [rows, C], elementwise:
//   g  = (sum_s gyA[s] + sum_s gyB[s]) * [mask_src > 0]      (the two consumers' cotangents,
//                                                              each possibly split-K slabs)
//   g_out = g (the residual branch's cotangent, and what the per-channel sums are taken of)
//   ga_out = g * w[c]*rstd[c]                                 (cotangent of the convolution output)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_bn_adjoint_pre(
    T* __restrict__ g_out, T* __restrict__ ga_out, const T* __restrict__ gyA, int a_splits,
    long long a_slab, const T* __restrict__ gyB, int b_splits, long long b_slab,
    const T* __restrict__ mask_src, const T* __restrict__ w, const T* __restrict__ rstd,
    unsigned total, unsigned C) {
  for (unsigned i = blockIdx.x * BLOCK + threadIdx.x; i < total; i += gridDim.x * BLOCK) {
    T g = gyA[i];  // (depth 1, unpredicated, written out: slab_sum<1> cost two instructions and two SGPRs more)
    for (int sp = 1; sp < a_splits; ++sp) g += gyA[(long long)sp * a_slab + i];
    if (gyB) {
      T h = gyB[i];
      for (int sp = 1; sp < b_splits; ++sp) h += gyB[(long long)sp * b_slab + i];
      g = g + h;
    }
    if (mask_src) g = mask_src[i] > (T)0 ? g : (T)0;
    if (g_out) g_out[i] = g;
    if (ga_out) {
      const unsigned c = i % C;
      ga_out[i] = g * ((w ? w[c] : (T)1) * rstd[c]);
    }
  }
}

// The same pre-pass in the shape of chan_affine_v4_body (fp32, C % 4 == 0, every operand 16-byte aligned): one channel
// quad per thread, every load -- both cotangents' slab 0, the mask, w, rstd, sixteen slabs of each cotangent -- issued
// before the first use.  This is what the adjoint CHAIN needs of a BatchNorm unit; the per-channel sums of g (the
// parameters' gradient, read by hf_pack_ex only) are taken off the chain by k_bn_sums_multi below.  Expressions and order
// are bn_adjoint_rows_body's -- slabs of each cotangent in split order (guarded additions, not + 0), g + h, the mask,
// g * (w*rstd) with w*rstd formed first: bitwise that kernel's gres / gx.
struct BnAdjV4Args {
  float *g_out, *ga_out;
  const float* gy;
  int s1;
  long long l1;
  const float* gy2;
  int s2;
  long long l2;
  const float *mask_src, *w, *rstd;
  unsigned total, C;
};

__device__ __forceinline__ void bn_adjoint_v4_body(
    float* __restrict__ g_out, float* __restrict__ ga_out, const float* __restrict__ gy, int s1, long long l1,
    const float* __restrict__ gy2, int s2, long long l2, const float* __restrict__ mask_src,
    const float* __restrict__ w, const float* __restrict__ rstd, unsigned total, unsigned C, unsigned bid,
    unsigned nblocks) {
  const unsigned quads = total >> 2;
  for (unsigned v = bid * BLOCK + threadIdx.x; v < quads; v += nblocks * BLOCK) {
    const unsigned i = v << 2;
    const unsigned c = i % C;
    F4 g = ld4(gy + i), h, mv, rs4, w4;
    if (gy2) h = ld4(gy2 + i);
    if (mask_src) mv = ld4(mask_src + i);
    if (rstd) rs4 = ld4(rstd + c);
    if (w) w4 = ld4(w + c);
    const bool hs = gy2 && s2 > 1;
    const int smax = (hs && s2 > s1) ? s2 : s1;
    for (int sp = 1; sp < smax; sp += 16) {
      F4 vg[16], vh[16];
      slab_issue(vg, gy, i, sp, s1, l1);
      if (hs) slab_issue(vh, gy2, i, sp, s2, l2);
      slab_add<true>(g, vg, sp, s1);
      if (hs) slab_add<true>(h, vh, sp, s2);
    }
    F4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float a = gy2 ? g.e[k] + h.e[k] : g.e[k];
      if (mask_src) a = mv.e[k] > 0.f ? a : 0.f;
      g.e[k] = a;
      o.e[k] = a * ((w ? w4.e[k] : 1.f) * (rstd ? rs4.e[k] : 1.f));
    }
    if (g_out) chain_store4<HF_WT_ELEM>(g_out + i, g);
    if (ga_out) chain_store4<HF_WT_ELEM>(ga_out + i, o);
  }
}

__global__ __launch_bounds__(BLOCK) void k_bn_adjoint_v4(const BnAdjV4Args p) {
  bn_adjoint_v4_body(p.g_out, p.ga_out, p.gy, p.s1, p.l1, p.gy2, p.s2, p.l2, p.mask_src, p.w, p.rstd, p.total, p.C,
                     blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(BLOCK) void k_bn_adjoint_v4_pair(const BnAdjV4Args A, const BnAdjV4Args B,
                                                              unsigned blocks_a) {
  const bool first = blockIdx.x < blocks_a;
  const BnAdjV4Args& p = first ? A : B;
  bn_adjoint_v4_body(p.g_out, p.ga_out, p.gy, p.s1, p.l1, p.gy2, p.s2, p.l2, p.mask_src, p.w, p.rstd, p.total, p.C,
                     first ? blockIdx.x : blockIdx.x - blocks_a, first ? blocks_a : gridDim.x - blocks_a);
}

// The per-channel sums gw = sum g*xhat, gb = sum g of SEVERAL units' stored masked cotangents in ONE launch, off the
// adjoint chain: workgroup b of the launch finds its problem in a table in device memory (entries [first, first + count),
// in adjoint-sweep order; block0 = the running sum of the row-block counts from entry 0) and runs bn_adjoint_rows_body on
// its row share -- one slab, no second cotangent, no mask, nothing elementwise stored: the thread map, the two-rows-per-
// pass order and cross_row_sums of the fused launch, bitwise its partial rows.  The table is read, not passed by value:
// one vector load per lane and a ballot find the entry, whose fields then arrive by uniform loads.
__global__ __launch_bounds__(BLOCK) void k_bn_sums_multi(const hf_bn_sums_problem* __restrict__ tab, int first,
                                                         int count, unsigned base) {
  __shared__ double red[BLOCK * 8];
  const unsigned b = blockIdx.x + base;
  const int lane = threadIdx.x & 63;
  unsigned b0 = 0xffffffffu;
  if (lane < count) b0 = tab[first + lane].block0;
  const int p = __builtin_amdgcn_readfirstlane(first + __popcll(__ballot(b0 <= b)) - 1);  // block0[first] == base <= b
  const hf_bn_sums_problem& e = tab[p];
  bn_adjoint_rows_body(nullptr, (float*)e.gw, (float*)e.gb, nullptr, (const float*)e.g, 1, 0, nullptr, 1, 0,
                       (const float*)e.x, (const float*)e.mean, (const float*)e.rstd, nullptr, nullptr, e.rows, e.c,
                       e.rows_per_block, b - e.block0, red);
}

// Forward of conv -> (eval-BatchNorm | bias) (+ residual) (+ ReLU) from the convolution's split-K slabs,
// NHWC [rows, C]; one element per thread (activation-sized, latency-bound).  The rounding sequence
// is chan_affine_body's forward: ((s - mean)*rstd)*w, + b, + res.
__global__ __launch_bounds__(BLOCK) void k_bn_forward(
    float* __restrict__ y, float* __restrict__ y2, unsigned y2_ld, float* a_out,
    const float* a, int splits, long long slab, const float* __restrict__ mean,  // (a_out may alias a: in place)
    const float* __restrict__ rstd, const float* __restrict__ w, const float* __restrict__ b,
    const float* __restrict__ res, unsigned res_ld, int relu, unsigned total, unsigned C) {
  for (unsigned i = blockIdx.x * BLOCK + threadIdx.x; i < total; i += gridDim.x * BLOCK) {
  const unsigned c = i % C, row = i / C;
  const float av = slab_sum<8>(a[i], a, i, splits, slab);  // eight slabs in flight
  if (a_out) a_out[i] = av;
  float t = av;
  if (rstd) t = ((av - mean[c]) * rstd[c]) * w[c];
  if (b) t += b[c];
  if (res) t += res[res_ld ? (size_t)row * res_ld + c : i];
  if (relu) t = t > 0.f ? t : 0.f;
  if (y) y[i] = t;
  if (y2) y2[(size_t)row * y2_ld + c] = t;
  }
}

// Forward of a TRAIN-mode BatchNorm (+ residual, + ReLU) whose workgroups first add the one-pass statistics' partial
// rows up themselves (k_bn_stats_rows without its tail: part [nparts][2][C] doubles = sum a, sum a^2 per row block) --
// mean, biased variance = E[a^2] - mean^2, rstd exactly as that tail computes them; workgroup 0 also writes mean /
// rstd (the sweeps read them) and moves the running statistics.  fp32 NHWC, C % 4 == 0, `a` already summed.
__global__ __launch_bounds__(BLOCK) void k_bn_forward_train(
    float* __restrict__ y, float* __restrict__ y2, unsigned y2_ld, const float* __restrict__ a,
    const double* __restrict__ part, unsigned nparts, float* __restrict__ mean_out, float* __restrict__ rstd_out,
    float* __restrict__ run_mean, float* __restrict__ run_var, double count, float eps, float momentum,
    const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ res, unsigned res_ld,
    int relu, unsigned total, unsigned C) {
  struct alignas(16) D2 { double e[2]; };
  __shared__ D2 scratch[2 * BLOCK];  // [row group][column pair], C <= 2 * BLOCK column pairs
  __shared__ double fin[8 * BLOCK];   // sum a | sum a^2, C <= 4 * BLOCK each
  __shared__ float mus[4 * BLOCK], rss[4 * BLOCK];
  // this thread's element quad first (independent of the statistics)
  const unsigned quads_total = total >> 2;
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  const bool have = v < quads_total;
  const unsigned i = have ? v << 2 : 0u;
  const unsigned row = i / C, c = i - row * C;
  const F4 av = ld4(a + i);
  const F4 w4 = ld4(w + c);
  F4 b4, r4;
  if (b) b4 = ld4(b + c);
  if (res) r4 = ld4(res + (res_ld ? row * res_ld + c : i));
  // column sums of the [nparts][2C] matrix of doubles, as pairs: thread (tx, ty) adds rows ty, ty + G, ... of column
  // pair tx (+ lanes, ...), four rows in flight, fixed order; the row groups are combined through LDS
  const unsigned CP = C;  // pairs of doubles per row
  const unsigned lanes = CP < BLOCK ? CP : BLOCK, G = BLOCK / lanes;
  const unsigned tx = threadIdx.x % lanes, ty = threadIdx.x / lanes;
  const D2* rows2 = reinterpret_cast<const D2*>(part);
  for (unsigned col = tx; col < CP; col += lanes) {
    D2 acc = {{0.0, 0.0}};
    if (ty < G) {
      for (unsigned p0 = ty; p0 < nparts; p0 += 4 * G) {
        D2 t4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t4[u] = rows2[(size_t)(p0 + u * G < nparts ? p0 + u * G : p0) * CP + col];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (p0 + u * G < nparts) { acc.e[0] += t4[u].e[0]; acc.e[1] += t4[u].e[1]; }
      }
      if (G > 1) scratch[ty * lanes + col] = acc;
      else { fin[2 * col] = acc.e[0]; fin[2 * col + 1] = acc.e[1]; }
    }
  }
  __syncthreads();
  if (G > 1) {
    for (unsigned j = threadIdx.x; j < 2 * C; j += BLOCK) {
      double sum = 0.0;
      for (unsigned t = 0; t < G; ++t) sum += scratch[t * lanes + (j >> 1)].e[j & 1];
      fin[j] = sum;
    }
    __syncthreads();
  }
  for (unsigned ch = threadIdx.x; ch < C; ch += BLOCK) {
    const double m = fin[ch] / count;
    double var = fin[C + ch] / count - m * m;
    if (var < 0.0) var = 0.0;
    const float mf = (float)m, rf = (float)(1.0 / sqrt(var + (double)eps));
    mus[ch] = mf;
    rss[ch] = rf;
    if (blockIdx.x == 0) {
      mean_out[ch] = mf;
      rstd_out[ch] = rf;
      if (momentum >= 0.f && run_mean && run_var) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        run_mean[ch] = (float)((1.0 - (double)momentum) * (double)run_mean[ch] + (double)momentum * (double)mf);
        run_var[ch] = (float)((1.0 - (double)momentum) * (double)run_var[ch] + (double)momentum * unbiased);
      }
    }
  }
  __syncthreads();
  if (!have) return;
  F4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float t = ((av.e[k] - mus[c + k]) * rss[c + k]) * w4.e[k];
    if (b) t += b4.e[k];
    if (res) t += r4.e[k];
    if (relu) t = t > 0.f ? t : 0.f;
    o.e[k] = t;
  }
  if (y) *reinterpret_cast<F4*>(y + i) = o;
  if (y2) *reinterpret_cast<F4*>(y2 + (size_t)row * y2_ld + c) = o;
}

// Hessian of a softmax cross-entropy w.r.t. the logits, applied to v, row by row:
//   out[r, :] = scale * p[r, :] * (v[r, :] - <p[r, :], v[r, :]>)      (p = softmax(logits))
// One block per row; the dot product is accumulated in fp64.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_softmax_ce_hvp(T* __restrict__ out,
                                                          const T* __restrict__ p,
                                                          const T* __restrict__ v, T scale,
                                                          int cols) {
  __shared__ double lds[WAVES];
  const long long base = (long long)blockIdx.x * cols;
  double acc[1] = {0.0};
  for (int j = threadIdx.x; j < cols; j += BLOCK) acc[0] += (double)p[base + j] * (double)v[base + j];
  block_allreduce<1>(acc, lds);
  const T d = (T)acc[0];
  for (int j = threadIdx.x; j < cols; j += BLOCK)
    out[base + j] = scale * (p[base + j] * (v[base + j] - d));
}

// ---- Hessian product through a TRAIN-mode BatchNorm (forward-over-reverse, optimizer.py:450-455) --------------
// z = gamma * xhat + beta, xhat = (a - mean(a)) * rstd(a).  With the step's first-order cotangents g_z (masked), g_a
// and the tangent sweep's a' (dot quantities: derivatives along v; m = rows):
//   S1 = mean(a'),  Sx = mean(a' xhat),  xhat' = rstd (a' - S1 - xhat Sx),  rstd'/rstd = -rstd Sx
//   g_gamma' = sum(g_z' xhat + g_z xhat') = sum(g_z' xhat) + rstd sum(g_z a') - rstd (S1 g_beta + Sx g_gamma)
//   g_a'     = (rstd'/rstd) g_a + rstd [ G' - mean(G') - xhat' mean(G xhat) - xhat mean(G' xhat + G xhat') ],
//              G = gamma g_z,  G' = v_gamma g_z + gamma g_z'
//            = c0 g_a + c1 g_z + c2 g_z' + c3 a' + c4 xhat + c5          (per-channel c0 ... c5, below)
// k_bn_train_hessian_coeffs adds the partial rows of the five row reductions up (fp64, row order) and writes the six
// coefficient vectors and the closed-form share of g_gamma' as one more partial row for the gather;
// k_bn_train_hessian_apply is the elementwise pass (a' arrives as the tangent convolution's split-K slabs).
__global__ __launch_bounds__(BLOCK) void k_bn_train_hessian_coeffs(
    float* __restrict__ coef, float* __restrict__ gw_corr, const float* __restrict__ sum_gx2,
    const float* __restrict__ sum_g2, const float* __restrict__ sum_ga, const float* __restrict__ sum_tx,
    const float* __restrict__ sum_t1, int nparts, int nparts_t, const float* __restrict__ g_gamma1,
    const float* __restrict__ g_beta1, const float* __restrict__ gamma, const float* __restrict__ v_gamma,
    const float* __restrict__ rstd, double count, int C) {
  // 8 channels x 32 row lanes per workgroup: lane rl adds rows rl, rl + 32, ... (fp64, increasing), the 32 shares are
  // combined in lane order -- a fixed summation order, and at most nparts / 32 dependent round trips instead of nparts
  // (one thread per channel walking up to 256 rows: 530 matvecs/s on the train-mode ResNet-18; 8 row lanes: 628)
  constexpr int CH = 8, RL = BLOCK / CH;
  __shared__ double red[5][RL][CH];
  const int cl = threadIdx.x % CH, rl = threadIdx.x / CH, c = blockIdx.x * CH + cl;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  if (c < C) {
    for (int p = rl; p < nparts; p += RL) {
      s[0] += (double)sum_gx2[(size_t)p * C + c];
      s[1] += (double)sum_g2[(size_t)p * C + c];
      s[2] += (double)sum_ga[(size_t)p * C + c];
    }
    for (int p = rl; p < nparts_t; p += RL) {  // (the tangent sweep's sums: a reduction launch's or the convolution epilogue's)
      s[3] += (double)sum_tx[(size_t)p * C + c];
      s[4] += (double)sum_t1[(size_t)p * C + c];
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][rl][cl] = s[k];
  __syncthreads();
  if (rl != 0 || c >= C) return;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double t = red[k][0][cl];
    for (int j = 1; j < RL; ++j) t += red[k][j][cl];
    s[k] = t;
  }
  const double s_gx = s[0], s_g = s[1], s_ga = s[2], s_tx = s[3], s_t1 = s[4];
  const double r = rstd[c], gam = gamma[c], dgam = v_gamma[c], gg = g_gamma1[c], gb = g_beta1[c];
  const double S1 = s_t1 / count, Sx = s_tx / count;
  const double corr = -r * (S1 * gb + Sx * gg);
  const double dgg = s_gx + s_ga + corr;                  // g_gamma'
  const double mG = (dgam * gb + gam * s_g) / count;      // mean(G')
  const double m2 = (dgam * gg + gam * dgg) / count;      // mean(G' xhat + G xhat')
  const double mGx = gam * gg / count;                    // mean(G xhat)
  coef[0 * C + c] = (float)(-r * Sx);
  coef[1 * C + c] = (float)(r * dgam);
  coef[2 * C + c] = (float)(r * gam);
  coef[3 * C + c] = (float)(-r * r * mGx);
  coef[4 * C + c] = (float)(r * r * mGx * Sx - r * m2);
  coef[5 * C + c] = (float)(-r * mG + r * r * mGx * S1);
  gw_corr[c] = (float)corr;
}

__global__ __launch_bounds__(BLOCK) void k_bn_train_hessian_apply(
    float* __restrict__ out, const float* __restrict__ ga1, const float* __restrict__ gz1,
    const float* __restrict__ gz2, const float* __restrict__ t, int t_splits, long long t_slab,
    const float* __restrict__ a, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ coef, unsigned total4, unsigned C) {
  for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < total4; q += gridDim.x * BLOCK) {
    const unsigned i = 4 * q, c = i % C;
    F4 k0 = ld4(coef + c), k1 = ld4(coef + C + c), k2 = ld4(coef + 2 * C + c), k3 = ld4(coef + 3 * C + c),
       k4 = ld4(coef + 4 * C + c), k5 = ld4(coef + 5 * C + c);
    const F4 mu = ld4(mean + c), rs = ld4(rstd + c);
    const F4 va = ld4(ga1 + i), v1 = ld4(gz1 + i), v2 = ld4(gz2 + i), xa = ld4(a + i);
    F4 ta = ld4(t + i);
    // (written out: slab_sum<8, true> cost this kernel three instructions and two VGPRs more)
    for (int sp = 1; sp < t_splits; sp += 8) {  // the tangent convolution's slabs: eight in flight, added in split order
      F4 sl[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) sl[u] = ld4(t + (long long)(sp + u < t_splits ? sp + u : 0) * t_slab + i);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (sp + u < t_splits) {
#pragma unroll
          for (int e = 0; e < 4; ++e) ta.e[e] += sl[u].e[e];
        }
    }
    F4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (xa.e[e] - mu.e[e]) * rs.e[e];
      o.e[e] = ((k0.e[e] * va.e[e] + k1.e[e] * v1.e[e]) + (k2.e[e] * v2.e[e] + k3.e[e] * ta.e[e])) +
               (k4.e[e] * xh + k5.e[e]);
    }
    *reinterpret_cast<F4*>(out + i) = o;
  }
}

// hf_chan_sqsum: sum over the samples of the SQUARED per-sample scale / shift (bias) gradient, NHWC [n*hw, c].
// A workgroup takes 64 channels (one wave reads 64 consecutive channels of a row) and the samples of row share
// blockIdx.y; the four waves split a sample's hw rows (row j to wave j % 4) and each wave keeps four fp64 sums (its
// rows in turn: four independent loads in flight), added as (s0 + s1) + (s2 + s3).  Per sample: the four waves' shares
// added through LDS in wave order, rounded once to fp32; then t = pre * sum, acc += t * t in fp32, the samples in
// ascending order.  One fixed order: two launches give the same bits.
constexpr int SQ_CH = 64, SQ_PARTS = BLOCK / SQ_CH;
__global__ __launch_bounds__(BLOCK) void k_chan_sqsum(float* __restrict__ gw2, float* __restrict__ gb2,
                                                      const float* __restrict__ g, const float* __restrict__ x,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      unsigned n, unsigned c, unsigned hw, unsigned per, float pre) {
  __shared__ double red[2][SQ_PARTS][SQ_CH];
  const unsigned cl = threadIdx.x % SQ_CH, part = threadIdx.x / SQ_CH, ch = blockIdx.x * SQ_CH + cl;
  const bool cok = ch < c;
  const unsigned i0 = blockIdx.y * per, i1 = i0 + per < n ? i0 + per : n;
  const float mu = (x && cok) ? mean[ch] : 0.f, rs = (x && cok) ? rstd[ch] : 0.f;
  float qw = 0.f, qb = 0.f;
  for (unsigned i = i0; i < i1; ++i) {
    double s1 = 0.0, sx = 0.0;
    if (cok) {
      double a1[4] = {0.0, 0.0, 0.0, 0.0}, ax[4] = {0.0, 0.0, 0.0, 0.0};
      const size_t e0 = (size_t)i * hw * c + ch;
      unsigned j = part;
      for (; j + 3 * SQ_PARTS < hw; j += 4 * SQ_PARTS) {  // (every load first)
        float gv[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const size_t e = e0 + (size_t)(j + u * SQ_PARTS) * c;
          gv[u] = g[e];
          xv[u] = x ? x[e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          a1[u] += (double)gv[u];
          if (x) ax[u] += (double)gv[u] * (double)(float)((xv[u] - mu) * rs);
        }
      }
      for (; j < hw; j += SQ_PARTS) {
        const size_t e = e0 + (size_t)j * c;
        const float gv = g[e];
        a1[0] += (double)gv;
        if (x) ax[0] += (double)gv * (double)(float)((x[e] - mu) * rs);
      }
      s1 = (a1[0] + a1[1]) + (a1[2] + a1[3]);
      sx = (ax[0] + ax[1]) + (ax[2] + ax[3]);
    }
    red[0][part][cl] = s1;
    red[1][part][cl] = sx;
    __syncthreads();
    if (part == 0) {
      const double t1 = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
      const double tx = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
      const float b = pre * (float)t1, wv = pre * (float)tx;
      qb += b * b;
      qw += wv * wv;
    }
    __syncthreads();
  }
  if (part == 0 && cok) {
    if (gw2) gw2[(size_t)blockIdx.y * c + ch] = qw;
    if (gb2) gb2[(size_t)blockIdx.y * c + ch] = qb;
  }
}
static_assert(SQ_PARTS == 4, "k_chan_sqsum adds four waves' shares");

}  // namespace

int hf_chan_sqsum(void* gw2, void* gb2, const void* g, const void* x, const void* mean, const void* rstd, int64_t n,
                  int64_t c, int64_t hw, float pre, int row_blocks, int dtype, void* stream) {
  if (!g || (!gw2 && !gb2) || n <= 0 || c <= 0 || hw <= 0 || row_blocks < 1 || dtype != HF_F32) return HF_ERR_ARG;
  if (!(pre - pre == 0.f)) return HF_ERR_ARG;                       // (NaN / infinity)
  if ((x || mean || rstd) && !(x && mean && rstd)) return HF_ERR_ARG;  // xhat needs all three
  if (gw2 && !x) return HF_ERR_ARG;
  if (n > 0x7fffffffLL || c > 0x7fffffffLL || hw > 0x7fffffffLL || n * hw > 0x7fffffffLL) return HF_ERR_ARG;
  const int64_t per = (n + row_blocks - 1) / row_blocks;
  if (row_blocks > 65535 || (int64_t)(row_blocks - 1) * per >= n) return HF_ERR_ARG;  // an empty share
  const dim3 grid((unsigned)((c + SQ_CH - 1) / SQ_CH), (unsigned)row_blocks);
  hipLaunchKernelGGL(k_chan_sqsum, grid, dim3(BLOCK), 0, (hipStream_t)stream, (float*)gw2, (float*)gb2,
                     (const float*)g, (const float*)x, (const float*)mean, (const float*)rstd, (unsigned)n, (unsigned)c,
                     (unsigned)hw, (unsigned)per, pre);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_bn_adjoint_pre(void* g_out, void* ga_out, const void* gy_a, int a_splits, int64_t a_slab,
                      const void* gy_b, int b_splits, int64_t b_slab, const void* mask_src, const void* w,
                      const void* rstd, int64_t rows, int64_t c, int dtype, void* stream) {
  if (!gy_a || (!g_out && !ga_out) || rows <= 0 || c <= 0 || a_splits < 1 || b_splits < 1) return HF_ERR_ARG;
  if (ga_out && !rstd) return HF_ERR_ARG;
  if ((a_splits > 1 && a_slab <= 0) || (gy_b && b_splits > 1 && b_slab <= 0)) return HF_ERR_ARG;
  const long long total = (long long)rows * c;
  if (total > 0x7fffffffLL) return HF_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HF_F32)
    hipLaunchKernelGGL((k_bn_adjoint_pre<float>), dim3(wide_grid(total)), dim3(BLOCK), 0, s, (float*)g_out,
                       (float*)ga_out, (const float*)gy_a, a_splits, (long long)a_slab, (const float*)gy_b,
                       b_splits, (long long)b_slab, (const float*)mask_src, (const float*)w, (const float*)rstd,
                       (unsigned)total, (unsigned)c);
  else if (dtype == HF_F64)
    hipLaunchKernelGGL((k_bn_adjoint_pre<double>), dim3(wide_grid(total)), dim3(BLOCK), 0, s, (double*)g_out,
                       (double*)ga_out, (const double*)gy_a, a_splits, (long long)a_slab, (const double*)gy_b,
                       b_splits, (long long)b_slab, (const double*)mask_src, (const double*)w,
                       (const double*)rstd, (unsigned)total, (unsigned)c);
  else
    return HF_ERR_ARG;
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_bn_forward(void* y, void* y2, int64_t y2_ld, void* a_out, const void* a, int splits, int64_t slab_stride,
                  const void* mean, const void* rstd, const void* w, const void* b, const void* res,
                  int64_t res_ld, int relu, int64_t rows, int64_t c, int dtype, void* stream) {
  if (dtype != HF_F32 || !a || (!y && !y2) || rows <= 0 || c <= 0 || splits < 1) return HF_ERR_ARG;
  if (splits > 1 && slab_stride < rows * c) return HF_ERR_ARG;
  if (rstd && (!mean || !w)) return HF_ERR_ARG;
  if ((y2 && y2_ld < c) || (res && res_ld && res_ld < c)) return HF_ERR_ARG;
  const long long total = (long long)rows * c;
  const long long widest = (long long)rows * (y2_ld > res_ld ? (y2_ld > c ? y2_ld : c) : (res_ld > c ? res_ld : c));
  if (total > 0x7fffffffLL || widest > 0x7fffffffLL || y2_ld > 0x3fffffffLL || res_ld > 0x3fffffffLL) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_bn_forward, dim3(wide_grid(total)), dim3(BLOCK), 0, (hipStream_t)stream, (float*)y,
                     (float*)y2, (unsigned)y2_ld, (float*)a_out, (const float*)a, splits, (long long)slab_stride,
                     (const float*)mean, (const float*)rstd, (const float*)w, (const float*)b, (const float*)res,
                     (unsigned)res_ld, relu, (unsigned)total, (unsigned)c);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_bn_forward_train(void* y, void* y2, int64_t y2_ld, const void* a, const void* part, int nparts, void* mean,
                        void* rstd, void* running_mean, void* running_var, double count, double eps, double momentum,
                        const void* w, const void* b, const void* res, int64_t res_ld, int relu, int64_t rows,
                        int64_t c, int dtype, void* stream) {
  if (dtype != HF_F32 || !a || (!y && !y2) || !part || nparts < 1 || !mean || !rstd || !w || count <= 0.0 ||
      rows <= 0 || c <= 0)
    return HF_ERR_ARG;
  if (!(c % 4 == 0 && c / 4 <= BLOCK)) return HF_ERR_ARG;
  if ((y2 && (y2_ld < c || (y2_ld & 3))) || (res && res_ld && (res_ld < c || (res_ld & 3)))) return HF_ERR_ARG;
  const long long total = (long long)rows * c;
  const long long widest = (long long)rows * (y2_ld > res_ld ? (y2_ld > c ? y2_ld : c) : (res_ld > c ? res_ld : c));
  if (total > 0x7fffffffLL || widest > 0x7fffffffLL) return HF_ERR_ARG;
  const void* al[] = {y, y2, a, part, w, b, res};
  for (const void* p : al)
    if (p && !aligned16(p)) return HF_ERR_ALIGN;
  // (the grid covers every quad: one per thread, as the prologue's sums are per workgroup anyway)
  const long long wgs = (total / 4 + BLOCK - 1) / BLOCK;
  if (wgs > 0x7fffffLL) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_bn_forward_train, dim3((unsigned)wgs), dim3(BLOCK), 0, (hipStream_t)stream, (float*)y,
                     (float*)y2, (unsigned)y2_ld, (const float*)a, (const double*)part, (unsigned)nparts, (float*)mean,
                     (float*)rstd, (float*)running_mean, (float*)running_var, count, (float)eps, (float)momentum,
                     (const float*)w, (const float*)b, (const float*)res, (unsigned)res_ld, relu, (unsigned)total,
                     (unsigned)c);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_softmax_ce_hvp(void* out, const void* p, const void* v, double scale, int64_t rows,
                      int64_t cols, int dtype, void* stream) {
  if (!out || !p || !v || rows <= 0 || cols <= 0 || cols > 0x7fffffffLL || rows > 0x7fffffffLL)
    return HF_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HF_F32)
    hipLaunchKernelGGL((k_softmax_ce_hvp<float>), dim3((unsigned)rows), dim3(BLOCK), 0, s, (float*)out,
                       (const float*)p, (const float*)v, (float)scale, (int)cols);
  else if (dtype == HF_F64)
    hipLaunchKernelGGL((k_softmax_ce_hvp<double>), dim3((unsigned)rows), dim3(BLOCK), 0, s,
                       (double*)out, (const double*)p, (const double*)v, scale, (int)cols);
  else
    return HF_ERR_ARG;
  HF_HIP(hipGetLastError());
  return HF_OK;
}

// The host functions below take a problem as the public struct that names its fields (include/hf_pcg.h); the positional
// entry points fill that struct and run what the two-problem entry points run.

// The quad-per-thread walk of the affine kernels: every operand given (`ptrs`) 16-byte aligned, NHWC, strides in quads.
template <size_t N>
static bool affine_vec4_ok(const void* const (&ptrs)[N], long long total, long long c, int nhwc, long long out_ld,
                           long long add_ld, long long a_slab) {
  for (const void* p : ptrs)
    if (p && !aligned16(p)) return false;
  return nhwc && c % 4 == 0 && out_ld % 4 == 0 && add_ld % 4 == 0 && a_slab % 4 == 0 && 2 * total < 0x7fffffffLL;
}

// One problem of hf_chan_affine_ex / hf_chan_affine_pair, any dtype and size: the refusals, and whether the
// quad-per-thread walk may run.
static int check_aff(bool& vec4, const hf_affine_problem& p, int channels_last) {
  if (p.a_splits < 1 || (p.a_splits > 1 && (!p.a || p.a_slab <= 0))) return HF_ERR_ARG;
  if (!p.out || p.n <= 0 || p.c <= 0 || p.hw <= 0) return HF_ERR_ARG;
  if (p.q && (!p.x || !p.mean || !p.rstd)) return HF_ERR_ARG;
  // a leading dimension is that of a buffer with MORE channels: >= 2x would be the
  // tangent buffers' case, anything above the dense one is accepted
  const int64_t dense = channels_last ? p.c : p.c * p.hw;
  if ((p.out_ld && p.out_ld < dense) || (p.add_ld && (p.add_ld < dense || !p.add)) ||
      p.out_ld > 0x3fffffffLL || p.add_ld > 0x3fffffffLL)
    return HF_ERR_ARG;
  const void* const ptrs[] = {p.out, p.a, p.x, p.mean, p.rstd, p.w, p.q, p.r, p.add, p.mask_src};
  vec4 = affine_vec4_ok(ptrs, (long long)p.n * p.c * p.hw, p.c, channels_last || p.hw == 1, p.out_ld, p.add_ld,
                        p.a_slab);
  return HF_OK;
}

// The same problem as the fp32 kernel arguments with 32-bit sizes, which hold while 2 * total < 2^31: larger problems
// are refused, so a filled AffArgs is always valid.
static int fill_aff(AffArgs& k, const hf_affine_problem& p, int channels_last) {
  bool vec4 = false;
  const int rc = check_aff(vec4, p, channels_last);
  if (rc) return rc;
  const long long total = (long long)p.n * p.c * p.hw;
  if (2 * total >= 0x7fffffffLL) return HF_ERR_ARG;
  k = AffArgs{(float*)p.out, (const float*)p.a, (const float*)p.x, (const float*)p.mean, (const float*)p.rstd,
              (const float*)p.w, (const float*)p.q, (const float*)p.r, (const float*)p.add, (const float*)p.mask_src,
              p.relu_self, (unsigned)total, (unsigned)p.c, (unsigned)p.hw, channels_last, (unsigned)p.out_ld,
              (unsigned)p.add_ld, p.a_splits, (long long)p.a_slab, vec4 ? 1 : 0};
  return HF_OK;
}

template <typename T>
static void launch_chan_affine(hipStream_t s, const hf_affine_problem& p, int nhwc, bool vec4) {
  const long long total = (long long)p.n * p.c * p.hw, c = p.c, hw = p.hw, out_ld = p.out_ld, add_ld = p.add_ld,
                  a_slab = p.a_slab;
  if (sizeof(T) == 4 && vec4)
    hipLaunchKernelGGL(k_chan_affine_v4, dim3(wide_grid(total / 4)), dim3(BLOCK), 0, s, (float*)p.out,
                       (const float*)p.a, (const float*)p.x, (const float*)p.mean, (const float*)p.rstd,
                       (const float*)p.w, (const float*)p.q, (const float*)p.r, (const float*)p.add,
                       (const float*)p.mask_src, p.relu_self, (unsigned)total, (unsigned)c, (unsigned)out_ld,
                       (unsigned)add_ld, p.a_splits, a_slab);
  else if (2 * total < 0x7fffffffLL)  // strided operands reach at most 2*total
    hipLaunchKernelGGL((k_chan_affine<T, unsigned>), dim3(wide_grid(total)), dim3(BLOCK), 0, s,
                       (T*)p.out, (const T*)p.a, (const T*)p.x, (const T*)p.mean, (const T*)p.rstd,
                       (const T*)p.w, (const T*)p.q, (const T*)p.r, (const T*)p.add, (const T*)p.mask_src,
                       p.relu_self, (unsigned)total, (unsigned)c, (unsigned)hw, nhwc,
                       (unsigned)out_ld, (unsigned)add_ld, p.a_splits, a_slab);
  else
    hipLaunchKernelGGL((k_chan_affine<T, long long>), dim3(wide_grid(total)), dim3(BLOCK), 0, s,
                       (T*)p.out, (const T*)p.a, (const T*)p.x, (const T*)p.mean, (const T*)p.rstd,
                       (const T*)p.w, (const T*)p.q, (const T*)p.r, (const T*)p.add, (const T*)p.mask_src,
                       p.relu_self, total, c, hw, nhwc, out_ld, add_ld, p.a_splits, a_slab);
}

int hf_chan_affine(void* out, const void* a, const void* x, const void* mean, const void* rstd,
                   const void* w, const void* q, const void* r, const void* add,
                   const void* mask_src, int relu_self, int64_t n, int64_t c, int64_t hw,
                   int channels_last, int64_t out_ld, int64_t add_ld, int dtype, void* stream) {
  return hf_chan_affine_ex(out, a, x, mean, rstd, w, q, r, add, mask_src, relu_self, n, c, hw, channels_last,
                           out_ld, add_ld, 1, 0, dtype, stream);
}

int hf_chan_affine_ex(void* out, const void* a, const void* x, const void* mean, const void* rstd,
                      const void* w, const void* q, const void* r, const void* add,
                      const void* mask_src, int relu_self, int64_t n, int64_t c, int64_t hw,
                      int channels_last, int64_t out_ld, int64_t add_ld, int a_splits, int64_t a_slab,
                      int dtype, void* stream) {
  const hf_affine_problem p = {.out = out, .a = a, .x = x, .mean = mean, .rstd = rstd, .w = w, .q = q, .r = r,
                               .add = add, .mask_src = mask_src, .relu_self = relu_self, .n = n, .c = c, .hw = hw,
                               .out_ld = out_ld, .add_ld = add_ld, .a_splits = a_splits, .a_slab = a_slab};
  bool vec4 = false;
  const int rc = check_aff(vec4, p, channels_last);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HF_F32)
    launch_chan_affine<float>(s, p, channels_last, vec4);
  else if (dtype == HF_F64)
    launch_chan_affine<double>(s, p, channels_last, false);
  else
    return HF_ERR_ARG;
  HF_HIP(hipGetLastError());
  return HF_OK;
}

// One problem of hf_chan_affine_train / hf_chan_affine_train_pair; `add_ld`: the one argument the struct lacks.
static int fill_aff_train(AffTrainArgs& q, const hf_affine_train_problem& p, int64_t add_ld, int dtype) {
  if (!p.out || !p.a || !p.x || !p.mean || !p.rstd || !p.w || !p.part_x || !p.part_1 || p.nparts < 1 ||
      p.count <= 0.0 || p.n <= 0 || p.c <= 0 || p.hw <= 0 || p.a_splits < 1 || (p.a_splits > 1 && p.a_slab <= 0) ||
      dtype != HF_F32)
    return HF_ERR_ARG;
  if (!(p.c % 4 == 0 && p.c / 4 <= BLOCK)) return HF_ERR_ARG;
  if ((p.out_ld && p.out_ld < p.c) || (add_ld && (add_ld < p.c || !p.add)) || p.out_ld > 0x3fffffffLL ||
      add_ld > 0x3fffffffLL)
    return HF_ERR_ARG;
  const long long total = (long long)p.n * p.c * p.hw;
  const void* const ptrs[] = {p.out, p.a, p.x, p.mean, p.rstd, p.w, p.add, p.mask_src};
  if (!affine_vec4_ok(ptrs, total, p.c, 1, p.out_ld, add_ld, p.a_slab) || !aligned16(p.part_x) || !aligned16(p.part_1))
    return HF_ERR_ALIGN;
  q = AffTrainArgs{(float*)p.out, (const float*)p.a, (const float*)p.x, (const float*)p.mean, (const float*)p.rstd,
                   (const float*)p.w, (const float*)p.part_x, (const float*)p.part_1, (unsigned)p.nparts,
                   (const float*)p.vq, (const float*)p.vr, (float)(1.0 / p.count), (const float*)p.add,
                   (const float*)p.mask_src, (unsigned)total, (unsigned)p.c, (unsigned)p.out_ld, (unsigned)add_ld,
                   p.a_splits, (long long)p.a_slab};
  return HF_OK;
}

int hf_chan_affine_train(void* out, const void* a, const void* x, const void* mean, const void* rstd, const void* w,
                         const void* part_x, const void* part_1, int nparts, const void* vq, const void* vr,
                         double count, const void* add, const void* mask_src, int64_t n, int64_t c, int64_t hw,
                         int64_t out_ld, int64_t add_ld, int a_splits, int64_t a_slab, int dtype, void* stream) {
  const hf_affine_train_problem p = {.out = out, .a = a, .x = x, .mean = mean, .rstd = rstd, .w = w, .part_x = part_x,
                                     .part_1 = part_1, .nparts = nparts, .vq = vq, .vr = vr, .count = count,
                                     .add = add, .mask_src = mask_src, .n = n, .c = c, .hw = hw, .out_ld = out_ld,
                                     .a_splits = a_splits, .a_slab = a_slab};
  AffTrainArgs q;
  const int rc = fill_aff_train(q, p, add_ld, dtype);
  if (rc) return rc;
  typedef void (*Kern)(AffTrainArgs);
  static const Kern kerns[8] = {
      k_chan_affine_v4_train<false, false, false>, k_chan_affine_v4_train<true, false, false>,
      k_chan_affine_v4_train<false, true, false>,  k_chan_affine_v4_train<true, true, false>,
      k_chan_affine_v4_train<false, false, true>,  k_chan_affine_v4_train<true, false, true>,
      k_chan_affine_v4_train<false, true, true>,   k_chan_affine_v4_train<true, true, true>};
  hipLaunchKernelGGL(kerns[(a_splits > 1 ? 1 : 0) | (add ? 2 : 0) | (mask_src ? 4 : 0)],
                     dim3(wide_grid(q.total / 4)), dim3(BLOCK), 0, (hipStream_t)stream, q);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_chan_affine_train_pair(const hf_affine_train_problem* problems, int dtype, void* stream) {
  if (!problems) return HF_ERR_ARG;
  AffTrainArgs q[2];
  for (int i = 0; i < 2; ++i) {
    const hf_affine_train_problem& p = problems[i];
    if (p.add) return HF_ERR_ARG;  // (no residual operand in the paired form)
    const int rc = fill_aff_train(q[i], p, 0, dtype);
    if (rc) return rc;
  }
  typedef void (*Kern)(AffTrainArgs, AffTrainArgs, unsigned);
#define HF_ATP(SA, MA, SB, MB) k_chan_affine_v4_train_pair<SA, MA, SB, MB>
  static const Kern kerns[16] = {
      HF_ATP(false, false, false, false), HF_ATP(true, false, false, false), HF_ATP(false, true, false, false),
      HF_ATP(true, true, false, false),   HF_ATP(false, false, true, false), HF_ATP(true, false, true, false),
      HF_ATP(false, true, true, false),   HF_ATP(true, true, true, false),   HF_ATP(false, false, false, true),
      HF_ATP(true, false, false, true),   HF_ATP(false, true, false, true),  HF_ATP(true, true, false, true),
      HF_ATP(false, false, true, true),   HF_ATP(true, false, true, true),   HF_ATP(false, true, true, true),
      HF_ATP(true, true, true, true)};
#undef HF_ATP
  const unsigned ba = (unsigned)wide_grid(q[0].total / 4), bb = (unsigned)wide_grid(q[1].total / 4);
  const int idx = (q[0].a_splits > 1 ? 1 : 0) | (q[0].mask_src ? 2 : 0) | (q[1].a_splits > 1 ? 4 : 0) |
                  (q[1].mask_src ? 8 : 0);
  hipLaunchKernelGGL(kerns[idx], dim3(ba + bb), dim3(BLOCK), 0, (hipStream_t)stream, q[0], q[1], ba);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_chan_affine_pair(const hf_affine_problem* problems, int dtype, void* stream) {
  if (!problems || dtype != HF_F32) return HF_ERR_ARG;
  AffArgs q[2];
  unsigned blocks[2];
  for (int i = 0; i < 2; ++i) {
    const hf_affine_problem& p = problems[i];
    const int rc = fill_aff(q[i], p, 1 /* NHWC */);
    if (rc) return rc;
    blocks[i] = (unsigned)wide_grid(q[i].vec4 ? q[i].total / 4 : q[i].total);
  }
  hipLaunchKernelGGL(k_chan_affine_pair, dim3(blocks[0] + blocks[1]), dim3(BLOCK), 0, (hipStream_t)stream, q[0],
                     q[1], blocks[0]);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

// One problem of the row-share form (hf_chan_affine_bwd_ex with row_blocks > 1, hf_chan_affine_bwd_pair; fp32 NHWC).
// What the row-major adjoint kernel needs beyond its shape limits: every workgroup's row share starts
// inside the tensor (share i covers rows [i*per, (i+1)*per), per = ceil(rows / row_blocks): an empty share would be a
// partial row of zeros the caller did not plan for), slab strides that keep the 16-byte loads aligned, and the
// statistics whenever the scale's gradient is asked for (without x the kernel would leave gw = 0).
static int fill_bn_adj_rows(BnAdjArgs& k, const hf_bn_adjoint_problem& p) {
  if (!p.gy || p.n <= 0 || p.c <= 0 || p.hw <= 0 || p.gy_splits < 1 || p.gy2_splits < 1 || p.row_blocks < 2)
    return HF_ERR_ARG;
  if (!(p.c % 4 == 0 && p.c / 4 <= BLOCK)) return HF_ERR_ARG;
  const int64_t rows = p.n * p.hw, per = (rows + p.row_blocks - 1) / p.row_blocks;
  if ((int64_t)(p.row_blocks - 1) * per >= rows) return HF_ERR_ARG;
  if (p.gy_splits > 1 && (p.gy_slab <= 0 || (p.gy_slab & 3))) return HF_ERR_ARG;
  if (p.gy2 && p.gy2_splits > 1 && (p.gy2_slab <= 0 || (p.gy2_slab & 3))) return HF_ERR_ARG;
  if (p.gw && (!p.x || !p.mean || !p.rstd)) return HF_ERR_ARG;
  if (rows * p.c > 0x7fffffffLL || !aligned16(p.gy) || (p.gy2 && !aligned16(p.gy2)) || (p.x && !aligned16(p.x)) ||
      (p.mask_src && !aligned16(p.mask_src)) || (p.gx && !aligned16(p.gx)) || (p.gres && !aligned16(p.gres)))
    return HF_ERR_ALIGN;
  k = BnAdjArgs{(float*)p.gx, (float*)p.gw, (float*)p.gb, (float*)p.gres, (const float*)p.gy, p.gy_splits,
                (long long)p.gy_slab, (const float*)p.gy2, p.gy2_splits, (long long)p.gy2_slab, (const float*)p.x,
                (const float*)p.mean, (const float*)p.rstd, (const float*)p.w, (const float*)p.mask_src, (unsigned)rows,
                (unsigned)p.c, (unsigned)per};
  return HF_OK;
}

int hf_chan_affine_bwd_pair(const hf_bn_adjoint_problem* problems, int dtype, void* stream) {
  if (!problems || dtype != HF_F32) return HF_ERR_ARG;
  BnAdjArgs q[2];
  unsigned blocks[2];
  for (int i = 0; i < 2; ++i) {
    const hf_bn_adjoint_problem& p = problems[i];
    const int rc = fill_bn_adj_rows(q[i], p);
    if (rc) return rc;
    blocks[i] = (unsigned)p.row_blocks;
  }
  hipLaunchKernelGGL(k_bn_adjoint_rows_pair, dim3(blocks[0] + blocks[1]), dim3(BLOCK), 0, (hipStream_t)stream,
                     q[0], q[1], blocks[0]);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

template <typename T>
static void launch_chan_affine_bwd(hipStream_t s, const hf_bn_adjoint_problem& p, int nhwc) {
  const long long n = p.n, c = p.c, hw = p.hw, total = n * c * hw, l1 = p.gy_slab, l2 = p.gy2_slab;
  const int s1 = p.gy_splits, s2 = p.gy2_splits;
  if (nhwc && hw > 1) {
    const bool vec = c % 4 == 0 && aligned16(p.gy) && (!p.gy2 || aligned16(p.gy2)) && (!p.x || aligned16(p.x)) &&
                     (!p.mask_src || aligned16(p.mask_src)) &&
                     (!p.gx || aligned16(p.gx)) && (!p.gres || aligned16(p.gres)) && sizeof(T) == 4;
#define HF_BWD_CL(I, W, BS)                                                                        \
  hipLaunchKernelGGL((k_chan_affine_bwd_nhwc<T, I, W, BS>), dim3((unsigned)(c / W * p.row_blocks)), dim3(BS), 0, s, \
                     (T*)p.gx, (T*)p.gw, (T*)p.gb, (T*)p.gres, (const T*)p.gy, (const T*)p.gy2, (const T*)p.x,    \
                     (const T*)p.mean, (const T*)p.rstd, (const T*)p.w, (const T*)p.mask_src, (I)(n * hw), (I)c,  \
                     s1, l1, s2, l2, p.row_blocks)
    // (512- and 1024-thread blocks for the early layers' tall reductions were measured: no
    // gain; a row-major kernel with a two-level reduction (block partials + last-ticket block)
    // was correct but slower end to end (885 vs 915 matvecs/s): its extra dependent round
    // trips cost more than the coalescing wins on tensors this small)
    if (total < 0x7fffffffLL) {
      if (vec) HF_BWD_CL(unsigned, 4, BLOCK); else HF_BWD_CL(unsigned, 1, BLOCK);
    } else {
      if (vec) HF_BWD_CL(long long, 4, BLOCK); else HF_BWD_CL(long long, 1, BLOCK);
    }
#undef HF_BWD_CL
    return;
  }
  const bool small = n * hw <= 256;
#define HF_BWD(I, TPC, GRID)                                                                    \
  hipLaunchKernelGGL((k_chan_affine_bwd<T, I, TPC>), dim3((unsigned)(GRID)), dim3(BLOCK), 0, s,  \
                     (T*)p.gx, (T*)p.gw, (T*)p.gb, (T*)p.gres, (const T*)p.gy, (const T*)p.gy2, (const T*)p.x,  \
                     (const T*)p.mean, (const T*)p.rstd, (const T*)p.w, (const T*)p.mask_src, (I)n, (I)c, (I)hw,  \
                     s1, l1, s2, l2)
  if (total < 0x7fffffffLL) {
    if (small) HF_BWD(unsigned, 64, (c + 3) / 4); else HF_BWD(unsigned, 256, c);
  } else {
    HF_BWD(long long, 256, c);
  }
#undef HF_BWD
}

int hf_chan_affine_bwd(void* gx, void* gw, void* gb, void* gres, const void* gy, const void* gy2,
                       const void* x, const void* mean, const void* rstd, const void* w,
                       const void* mask_src, int64_t n, int64_t c, int64_t hw, int channels_last,
                       int dtype, void* stream) {
  return hf_chan_affine_bwd_ex(gx, gw, gb, gres, gy, 1, 0, gy2, 1, 0, x, mean, rstd, w, mask_src, n, c, hw,
                               channels_last, 1, dtype, stream);
}

int hf_chan_affine_bwd_ex(void* gx, void* gw, void* gb, void* gres, const void* gy, int gy_splits,
                          int64_t gy_slab, const void* gy2, int gy2_splits, int64_t gy2_slab,
                          const void* x, const void* mean, const void* rstd, const void* w,
                          const void* mask_src, int64_t n, int64_t c, int64_t hw, int channels_last,
                          int row_blocks, int dtype, void* stream) {
  if (!gy || n <= 0 || c <= 0 || hw <= 0 || gy_splits < 1 || gy2_splits < 1 || row_blocks < 1) return HF_ERR_ARG;
  hf_bn_adjoint_problem p = {.gx = gx, .gw = gw, .gb = gb, .gres = gres, .gy = gy, .gy_splits = gy_splits,
                             .gy_slab = gy_slab, .gy2 = gy2, .gy2_splits = gy2_splits, .gy2_slab = gy2_slab, .x = x,
                             .mean = mean, .rstd = rstd, .w = w, .mask_src = mask_src, .n = n, .c = c, .hw = hw,
                             .row_blocks = row_blocks};
  // row shares: the row-major NHWC fp32 kernel
  if (row_blocks > 1) {
    if (!(channels_last && dtype == HF_F32)) return HF_ERR_ARG;
    BnAdjArgs k;
    const int rc = fill_bn_adj_rows(k, p);
    if (rc) return rc;
    hipLaunchKernelGGL(k_bn_adjoint_rows, dim3((unsigned)row_blocks), dim3(BLOCK), 0, (hipStream_t)stream, k.gx, k.gw,
                       k.gb, k.gres, k.gy, k.s1, k.l1, k.gy2, k.s2, k.l2, k.x, k.mean, k.rstd, k.w, k.mask_src, k.rows,
                       k.C, k.rows_per_block);
    HF_HIP(hipGetLastError());
    return HF_OK;
  }
  if ((gy_splits > 1 && gy_slab <= 0) || (gy2 && gy2_splits > 1 && gy2_slab <= 0)) return HF_ERR_ARG;
  if ((gy_splits > 1 || gy2_splits > 1) && !(channels_last || hw == 1)) return HF_ERR_ARG;
  if (gw && (!x || !mean || !rstd)) return HF_ERR_ARG;  // (rstd == NULL: no BatchNorm, gx = g * w or g)
  if (!gw) p.x = nullptr;  // plain per-channel sums (a conv layer's bias gradient)
  hipStream_t s = (hipStream_t)stream;
  if (dtype == HF_F32)
    launch_chan_affine_bwd<float>(s, p, channels_last);
  else if (dtype == HF_F64)
    launch_chan_affine_bwd<double>(s, p, channels_last);
  else
    return HF_ERR_ARG;
  HF_HIP(hipGetLastError());
  return HF_OK;
}

// One problem of the elementwise adjoint (hf_bn_adjoint_v4, hf_bn_adjoint_v4_pair): the quad walk's conditions are
// refusals here, there is no scalar form behind it.
// Of the struct it reads gres (-> g_out), gx (-> ga_out), the cotangents, mask_src, w, rstd and rows = n * hw, c.
static int fill_bn_adj_v4(BnAdjV4Args& k, const hf_bn_adjoint_problem& p) {
  if (p.n <= 0 || p.hw <= 0) return HF_ERR_ARG;
  const int64_t rows = p.n * p.hw;
  if (!p.gy || (!p.gres && !p.gx) || rows <= 0 || p.c <= 0 || p.c % 4 || p.gy_splits < 1 || p.gy2_splits < 1)
    return HF_ERR_ARG;
  if (p.gy_splits > 1 && (p.gy_slab <= 0 || (p.gy_slab & 3))) return HF_ERR_ARG;
  if (p.gy2 && p.gy2_splits > 1 && (p.gy2_slab <= 0 || (p.gy2_slab & 3))) return HF_ERR_ARG;
  if (rows * p.c > 0x7fffffffLL) return HF_ERR_ARG;
  const void* ptrs[] = {p.gres, p.gx, p.gy, p.gy2, p.mask_src, p.w, p.rstd};
  for (const void* q : ptrs)
    if (q && !aligned16(q)) return HF_ERR_ARG;
  k = BnAdjV4Args{(float*)p.gres, (float*)p.gx, (const float*)p.gy, p.gy_splits, (long long)p.gy_slab,
                  (const float*)p.gy2, p.gy2 ? p.gy2_splits : 1, (long long)p.gy2_slab, (const float*)p.mask_src,
                  (const float*)p.w, (const float*)p.rstd, (unsigned)(rows * p.c), (unsigned)p.c};
  return HF_OK;
}

int hf_bn_adjoint_v4(void* g_out, void* ga_out, const void* gy, int gy_splits, int64_t gy_slab, const void* gy2,
                     int gy2_splits, int64_t gy2_slab, const void* mask_src, const void* w, const void* rstd,
                     int64_t rows, int64_t c, int dtype, void* stream) {
  if (dtype != HF_F32) return HF_ERR_ARG;
  const hf_bn_adjoint_problem p = {.gx = ga_out, .gres = g_out, .gy = gy, .gy_splits = gy_splits, .gy_slab = gy_slab,
                                   .gy2 = gy2, .gy2_splits = gy2_splits, .gy2_slab = gy2_slab, .rstd = rstd, .w = w,
                                   .mask_src = mask_src, .n = rows, .c = c, .hw = 1};
  BnAdjV4Args k;
  const int rc = fill_bn_adj_v4(k, p);
  if (rc) return rc;
  hipLaunchKernelGGL(k_bn_adjoint_v4, dim3(wide_grid(k.total / 4)), dim3(BLOCK), 0, (hipStream_t)stream, k);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_bn_adjoint_v4_pair(const hf_bn_adjoint_problem* problems, int dtype, void* stream) {
  if (!problems || dtype != HF_F32) return HF_ERR_ARG;
  BnAdjV4Args q[2];
  unsigned blocks[2];
  for (int i = 0; i < 2; ++i) {
    const hf_bn_adjoint_problem& p = problems[i];
    const int rc = fill_bn_adj_v4(q[i], p);
    if (rc) return rc;
    blocks[i] = (unsigned)wide_grid(q[i].total / 4);
  }
  hipLaunchKernelGGL(k_bn_adjoint_v4_pair, dim3(blocks[0] + blocks[1]), dim3(BLOCK), 0, (hipStream_t)stream, q[0],
                     q[1], blocks[0]);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

// One entry of a sums table: what bn_adjoint_rows_body needs of it (fill_bn_adj_rows's conditions for one slab and no
// elementwise output).  hf_bn_sums_table and hf_bn_sums_multi both run it.
static int check_bn_sums(const hf_bn_sums_problem& p, uint32_t& per) {
  if (!p.g || (!p.gw && !p.gb) || p.rows == 0 || p.c == 0 || p.row_blocks < 1) return HF_ERR_ARG;
  if (!(p.c % 4 == 0 && p.c / 4 <= BLOCK)) return HF_ERR_ARG;
  per = (p.rows + p.row_blocks - 1) / p.row_blocks;
  if ((uint64_t)(p.row_blocks - 1) * per >= p.rows) return HF_ERR_ARG;  // an empty share
  if (p.gw && (!p.x || !p.mean || !p.rstd)) return HF_ERR_ARG;
  if ((uint64_t)p.rows * p.c > 0x7fffffffULL) return HF_ERR_ARG;
  if (!aligned16(p.g) || (p.x && !aligned16(p.x))) return HF_ERR_ARG;
  return HF_OK;
}

int64_t hf_bn_sums_table(hf_bn_sums_problem* problems, int count) {
  if (!problems || count < 1) return HF_ERR_ARG;
  uint64_t blocks = 0;
  for (int i = 0; i < count; ++i) {
    uint32_t per;
    const int rc = check_bn_sums(problems[i], per);
    if (rc) return rc;
    if (!problems[i].gw) problems[i].x = nullptr;  // plain column sums (a bias gradient)
    problems[i].rows_per_block = per;
    problems[i].block0 = (uint32_t)blocks;
    blocks += problems[i].row_blocks;
    if (blocks > 0x7fffffffULL) return HF_ERR_ARG;
  }
  return (int64_t)blocks;
}

int hf_bn_sums_multi(const void* table_dev, const hf_bn_sums_problem* table, int table_count, int first, int count,
                     int dtype, void* stream) {
  if (!table_dev || !table || dtype != HF_F32 || table_count < 1 || first < 0 || count < 1 ||
      count > HF_BN_SUMS_MAX || first > table_count - count)
    return HF_ERR_ARG;
  uint64_t blocks = 0;
  for (int i = first; i < first + count; ++i) {
    uint32_t per;
    const int rc = check_bn_sums(table[i], per);
    if (rc) return rc;
    // (the derived fields as hf_bn_sums_table left them: the device copy was made from them)
    if (table[i].rows_per_block != per || table[i].block0 != table[first].block0 + blocks) return HF_ERR_ARG;
    blocks += table[i].row_blocks;
  }
  hipLaunchKernelGGL(k_bn_sums_multi, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream,
                     (const hf_bn_sums_problem*)table_dev, first, count, table[first].block0);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_bn_stats_rows(void* a_out, const void* a, int splits, int64_t slab_stride, void* part, int64_t rows, int64_t c,
                     int row_blocks, int dtype, void* stream) {
  if (!a || !part || splits < 1 || (splits > 1 && slab_stride <= 0) || rows <= 0 || c <= 0 || row_blocks < 1 ||
      dtype != HF_F32)
    return HF_ERR_ARG;
  if (!(c % 4 == 0 && c / 4 <= BLOCK) || rows * c > 0x7fffffffLL) return HF_ERR_ARG;
  if (!aligned16(a) || (a_out && !aligned16(a_out)) || (slab_stride & 3)) return HF_ERR_ALIGN;
  const unsigned rpb = (unsigned)((rows + row_blocks - 1) / row_blocks);
  hipLaunchKernelGGL(k_bn_stats_rows, dim3((unsigned)row_blocks), dim3(BLOCK), 0, (hipStream_t)stream,
                     (float*)a_out, (const float*)a, splits, (long long)slab_stride, (double*)part, (unsigned)rows,
                     (unsigned)c, rpb);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_bn_train_hessian_coeffs(void* coef, void* gw_corr, const void* sum_gx2, const void* sum_g2, const void* sum_ga,
                               int nparts, const void* sum_tx, const void* sum_t1, int nparts_t, const void* g_gamma1,
                               const void* g_beta1, const void* gamma, const void* v_gamma, const void* rstd,
                               double count, int64_t c, int dtype, void* stream) {
  if (!coef || !gw_corr || !sum_gx2 || !sum_g2 || !sum_ga || !sum_tx || !sum_t1 || nparts < 1 || nparts_t < 1 || !g_gamma1 ||
      !g_beta1 || !gamma || !v_gamma || !rstd || !(count > 0.0) || c <= 0 || c > 0x7fffffffLL || dtype != HF_F32)
    return HF_ERR_ARG;
  hipLaunchKernelGGL(k_bn_train_hessian_coeffs, dim3((unsigned)((c + 7) / 8)), dim3(BLOCK), 0,
                     (hipStream_t)stream, (float*)coef, (float*)gw_corr, (const float*)sum_gx2, (const float*)sum_g2,
                     (const float*)sum_ga, (const float*)sum_tx, (const float*)sum_t1, nparts, nparts_t,
                     (const float*)g_gamma1,
                     (const float*)g_beta1, (const float*)gamma, (const float*)v_gamma, (const float*)rstd, count,
                     (int)c);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_bn_train_hessian_apply(void* out, const void* ga1, const void* gz1, const void* gz2, const void* t, int t_splits,
                              int64_t t_slab, const void* a, const void* mean, const void* rstd, const void* coef,
                              int64_t rows, int64_t c, int dtype, void* stream) {
  if (!out || !ga1 || !gz1 || !gz2 || !t || t_splits < 1 || (t_splits > 1 && t_slab <= 0) || !a || !mean || !rstd ||
      !coef || rows <= 0 || c <= 0 || c % 4 || rows * c > 0x7fffffffLL || dtype != HF_F32)
    return HF_ERR_ARG;
  if (!aligned16(out) || !aligned16(ga1) || !aligned16(gz1) || !aligned16(gz2) || !aligned16(t) || !aligned16(a) ||
      !aligned16(mean) || !aligned16(rstd) || !aligned16(coef) || (t_slab & 3))
    return HF_ERR_ALIGN;
  const int64_t total4 = rows * c / 4;
  hipLaunchKernelGGL(k_bn_train_hessian_apply, dim3(wide_grid(total4)), dim3(BLOCK), 0, (hipStream_t)stream,
                     (float*)out, (const float*)ga1, (const float*)gz1, (const float*)gz2, (const float*)t, t_splits,
                     (long long)t_slab, (const float*)a, (const float*)mean, (const float*)rstd, (const float*)coef,
                     (unsigned)total4, (unsigned)c);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_pool_bn_act_tangent_train_nhwc(void* out, int64_t out_ld, const void* slabs, int splits, int64_t slab_stride,
                                      const void* a, const void* mean, const void* rstd, const void* w, const void* v_w,
                                      const void* v_b, const void* part_x, const void* part_1, int nparts, double count,
                                      const void* idx, const void* y_pool, int relu, int64_t n, int64_t h, int64_t w_,
                                      int64_t oh, int64_t ow, int64_t c, int dtype, void* stream) {
  // hf_pool_bn_act_tangent_nhwc's refusals ...
  if (dtype != HF_F32 || !out || !slabs || !idx || (relu && !y_pool) || !a || !mean || !rstd || !w) return HF_ERR_ARG;
  if (n < 1 || h < 1 || w_ < 1 || oh < 1 || ow < 1 || c < 1) return HF_ERR_ARG;
  if (splits < 1 || splits > HF_POOL_ACT_MAX_SPLITS) return HF_ERR_ARG;
  // ... and the prologue's
  if (!part_x || !part_1 || nparts < 1 || !(count > 0.0) || c % 4 || c / 4 > BLOCK) return HF_ERR_ARG;
  if (out_ld == 0) out_ld = c;
  if (out_ld < c) return HF_ERR_ARG;
  // (every factor below 2^31 first: the products cannot wrap)
  const int64_t lim = 1LL << 31;
  if (n >= lim || h >= lim || w_ >= lim || oh >= lim || ow >= lim || out_ld >= lim) return HF_ERR_ARG;
  if (h * w_ >= lim || oh * ow >= lim || n * (h * w_) >= lim || n * (oh * ow) >= lim) return HF_ERR_ARG;
  const int64_t full = n * h * w_ * c, total = n * oh * ow * c;
  if (full >= lim || total >= lim || n * oh * ow * out_ld >= lim) return HF_ERR_ARG;
  if (splits > 1 && slab_stride < full) return HF_ERR_ARG;  // (slabs would overlap)
  if (!aligned16(part_x) || !aligned16(part_1)) return HF_ERR_ALIGN;  // (the prologue reads the rows by quads)
  const float* yp = relu ? (const float*)y_pool : nullptr;
  const bool quad = out_ld % 4 == 0 && aligned16(out) && aligned16(idx) && (!yp || aligned16(yp));
  const unsigned items = (unsigned)(total / (quad ? 4 : 1));
  const PoolTrainArgs q{(float*)out, (const float*)slabs, (const float*)a, (const float*)mean, (const float*)rstd,
                        (const float*)w, (const float*)part_x, (const float*)part_1, (const float*)v_w, (const float*)v_b,
                        yp, (const int*)idx, (unsigned)nparts, (float)(1.0 / count), items,
                        (unsigned)(quad ? c / 4 : c), (unsigned)out_ld, (unsigned)(oh * ow), (unsigned)(h * w_), splits,
                        (long long)slab_stride};
  const dim3 grid((items + BLOCK - 1) / BLOCK);
  if (quad) hipLaunchKernelGGL(k_pool_bn_act_tangent_train<4>, grid, dim3(BLOCK), 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL(k_pool_bn_act_tangent_train<1>, grid, dim3(BLOCK), 0, (hipStream_t)stream, q);
  HF_HIP(hipGetLastError());
  return HF_OK;
}
