// hf_common.h -- what the translation units of libhfpcg.so share: workgroup size, 16-byte vector types, the
// fixed-order block reduction, the split-K slab sum, error / alignment / grid helpers.  gfx950 (wave64) only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "hf_pcg.h"
#include "hf_store.h"
#include "hf_unpack.h"

#define HF_HIP(expr)                         \
  do {                                       \
    hipError_t e_ = (expr);                  \
    if (e_ != hipSuccess) return (int)e_;    \
  } while (0)

namespace {

constexpr int BLOCK = 256;          // 4 waves of 64
constexpr int WAVES = BLOCK / 64;

using hf_shared::VecOf;
using hf_shared::VU;

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// one element per thread: these activation-sized kernels (<= a few hundred thousand
// elements) are latency-bound, every extra grid-stride iteration adds a full round trip
inline int wide_grid(int64_t n) {
  int64_t g = (n + BLOCK - 1) / BLOCK;
  if (g < 1) g = 1;
  if (g > 16384) g = 16384;
  return (int)g;
}

inline int small_grid(int64_t n) {
  int64_t g = (n + BLOCK * 4 - 1) / (BLOCK * 4);
  if (g < 1) g = 1;
  if (g > 2048) g = 2048;
  return (int)g;
}

// ---------------------------------------------------------------------------
// reductions: 64-lane __shfl_down tree -> LDS partial per wave -> fixed-order sum
// ---------------------------------------------------------------------------
template <int K, int NW = WAVES>
__device__ __forceinline__ void block_allreduce(double (&v)[K], double* lds /*K*NW*/) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[k * NW + wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = lds[k * NW];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += lds[k * NW + w];
    v[k] = s;
  }
  __syncthreads();
}

// Every block re-reduces the previous kernel's per-block partials (layout
// part[k*stride + block]) in the same order.
template <int K>
__device__ __forceinline__ void reduce_partials(const double* __restrict__ part, int nparts,
                                                int stride, double (&out)[K], double* lds) {
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.0;
  for (int i = threadIdx.x; i < nparts; i += BLOCK) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] += part[k * stride + i];
  }
  block_allreduce<K>(out, lds);
}

// ---------------------------------------------------------------------------
// split-K slabs.  A producer leaves n slabs `stride` elements apart; every consumer adds them up as
//   first (slab 0), then slabs 1 .. n-1 in split order,
// NB loads in flight per round trip (all issued before the first addition), a load past the last slab reads slab 0
// (valid memory) and is discarded.  The order of the additions does not depend on NB: bitwise the same sums.
// V is what a thread owns of each slab: a scalar T or a W-wide aligned column of T.
// ---------------------------------------------------------------------------
template <typename T, int W>
struct alignas(sizeof(T) * W) ColOf { T e[W]; };
using F4 = ColOf<float, 4>;  // the 16-byte quad of floats

__device__ __forceinline__ F4 ld4(const float* p) { return *reinterpret_cast<const F4*>(p); }

using hf_shared::chain_store;
using hf_shared::chain_store16;
template <bool WT>
__device__ __forceinline__ void chain_store4(float* p, const F4& v) { chain_store16<WT>(reinterpret_cast<F4*>(p), v); }
// a W-wide column of any element type: one scalar, or whole 16-byte pieces
template <bool WT, typename T, int W>
__device__ __forceinline__ void chain_store_col(T* p, const ColOf<T, W>& v) {
  if constexpr (!WT) {
    *reinterpret_cast<ColOf<T, W>*>(p) = v;
  } else if constexpr (W == 1) {
    chain_store<true>(p, v.e[0]);
  } else {
    constexpr int PW = 16 / sizeof(T);
    static_assert(W % PW == 0, "whole 16-byte pieces");
#pragma unroll
    for (int k = 0; k < W / PW; ++k) {
      ColOf<T, PW> piece;
#pragma unroll
      for (int e = 0; e < PW; ++e) piece.e[e] = v.e[k * PW + e];
      chain_store16<true>(reinterpret_cast<ColOf<T, PW>*>(p) + k, piece);
    }
  }
}

// s += v where `on`.  BRANCH picks the spelling: a select (the additions are straight-line code) or a branch around
// them; the sums are the same, the register allocation of the kernel around them is not, so each site says which.
template <bool BRANCH, typename T>
__device__ __forceinline__ void add_where(T& s, const T& v, bool on) {
  if (BRANCH) { if (on) s += v; }
  else s += on ? v : (T)0;
}
template <bool BRANCH, typename T, int W>
__device__ __forceinline__ void add_where(ColOf<T, W>& s, const ColOf<T, W>& v, bool on) {
  if (BRANCH) {
    if (on) {
#pragma unroll
      for (int k = 0; k < W; ++k) s.e[k] += v.e[k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) s.e[k] += on ? v.e[k] : (T)0;
  }
}

// first half: issue the loads of slabs sp .. sp+NB-1 (this thread's part of a slab starts `off` elements into it)
template <int NB, typename V, typename T, typename I>
__device__ __forceinline__ void slab_issue(V (&v)[NB], const T* p, I off, int sp, int n, long long stride) {
#pragma unroll
  for (int u = 0; u < NB; ++u)
    v[u] = *reinterpret_cast<const V*>(p + (long long)(sp + u < n ? sp + u : 0) * stride + off);
}

// second half: add that batch in split order, predicated
template <bool BRANCH, int NB, typename V>
__device__ __forceinline__ void slab_add(V& s, const V (&v)[NB], int sp, int n) {
#pragma unroll
  for (int u = 0; u < NB; ++u) add_where<BRANCH>(s, v[u], sp + u < n);
}

// first + slabs 1 .. n-1
template <int NB, bool BRANCH = false, typename V, typename T, typename I>
__device__ __forceinline__ V slab_sum(V first, const T* p, I off, int n, long long stride) {
  for (int sp = 1; sp < n; sp += NB) {
    V v[NB];
    slab_issue(v, p, off, sp, n, stride);
    slab_add<BRANCH>(first, v, sp, n);
  }
  return first;
}

template <int K>
__device__ __forceinline__ void write_partials(double* __restrict__ part, int stride,
                                               double (&v)[K], double* lds) {
  block_allreduce<K>(v, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) part[k * stride + blockIdx.x] = v[k];
  }
}

}  // namespace
