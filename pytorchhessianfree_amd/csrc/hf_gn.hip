// hf_gn.hip -- GroupNorm units of the plain-stack engine (engine/plain.py): conv -> GroupNorm(affine) -> [ReLU].  Forward,
// tangent and adjoint of the normalisation are ONE launch each -- the adjoint's own tangent, a Hessian product's second-order
// half, included -- and the per-sample parameter rows of the adjoint make the diagonal empirical Fisher one more.  fp32, wave64, NHWC [rows = n*hw, c], `groups` groups of cg = c / groups channels,
// cg % 4 == 0; statistics mean / rstd [n, groups].  Plain C++/HIP, no atomics: two launches on the same operands agree bitwise.
//
// Why a design of its own.  hf_bn.hip reduces per CHANNEL over all rows: its workgroups share a channel column and a
// grid-wide sum stands between the two passes of a train-mode unit (5-6 launches).  A GroupNorm statistic belongs to one
// (sample, group): hw pixels x cg channels, at most a few thousand numbers.  One workgroup can hold all of them, so every
// reduction of the unit is taken inside the launch that also applies the elementwise part.
//
// Work split.  A workgroup (256 lanes) owns one sample x one SPAN of whole groups: gps consecutive groups, span = gps * cg
// channels (the last span of a sample may hold fewer groups).  hf_gn_plan chooses gps: enough groups that a pixel's span is
// GN_SEG = 64 channels (a wave's 16-byte loads then form 256-byte segments; cg = 4 takes 16 groups), capped by the LDS
// block of GN_LDS_FLOATS = 16 384 floats (hw * span), then halved while the launch has fewer than 256 workgroups and a
// pixel's span stays >= 32 channels.  Grid (spans, n).
//
// Data movement.  The workgroup sums the split-K slabs of its hw x span block ONCE into LDS (slab 0, then slabs 1 .. n-1
// in split order: hf_common.h's slab_sum), tile[pixel][span channel], written as whole quads in thread order (lane q owns
// quads q, q + 256, ..: linear LDS addresses, 16-byte global loads along the pixel's span).  Every reduction reads that
// resident block; the elementwise part reads it again and leaves with 16-byte stores.  The recorded map `a` (x_hat's
// operand in tangent and adjoint) is read from global memory where it is needed: the sample's block is L2-resident.
//
// Reductions (group statistics).  The four waves form TEAMS: one group in the span -> one team of four waves, two groups
// -> two teams of two waves, three or more -> four teams of one wave; team t takes the span's groups t, t + teams, ...
// Lane l of a team of T lanes owns the group's quads l, l + T, .. (quad e = pixel e / (cg/4), channel quad e % (cg/4)) and
// keeps FOUR fp32 partial sums, one per channel of the quad, each a chain over its quads in ascending order: at most
// ceil(hw * cg / 256) terms (T >= 64).  Everything behind that is fp64: the four partials are added ((s0 + s1) + s2) + s3,
// the 64 lanes of a wave by a __shfl_down tree (offsets 32 .. 1), the waves of a team in wave order through LDS.  The
// order depends on the shape alone.
// Reductions (per-sample parameter rows, adjoint).  The lanes are laid out as slots x columns, columns = min(span / 4, 256)
// channel quads, slots = 256 / columns: lane (slot, j) owns channel quad j at the pixels slot, slot + slots, .. -- four fp32
// chains of at most ceil(hw / slots) terms -- and the slots are added in fp64 in slot order through LDS; one rounding to
// fp32 at the store.  (span / 4 > 256: passes of 256 columns, slots = 1.)
//
// Arithmetic chains (one fp32 rounding per named step unless it says fp64; -ffp-contract=off: no step is fused).
//   s        = slab 0 + slab 1 + .. (split order) [+ conv_bias[c]]                      splits - 1 [+ 1] roundings
// hf_gn_forward
//   mu       = fp32( fp64 sum of the lanes' chains of s / (hw*cg) )                     chain, then ONE rounding
//   d        = s - mu;  q = d * d;  the lanes' chains of q
//   rstd     = fp32( 1 / sqrt( fp64 sum / (hw*cg) + eps ) )                             all fp64, ONE rounding
//              (exact two-pass variance: the mean first, then sum (s - mu)^2; no E[x^2] - mu^2)
//   y        = act( ((s - mu) * rstd) * gamma[c] + beta[c] )                            4 roundings behind s, mu, rstd
// hf_gn_act_tangent  (mu, rstd: the forward launch's, as given)
//   t        = s of the tangent convolution's slabs [+ v_conv_bias[c]]
//   xh       = (a - mu) * rstd                                                          2
//   m1       = fp32( fp64 sum of the chains of t / (hw*cg) );  mx = fp32( .. of the chains of xh * t .. )
//   r        = (gamma[c] * rstd) * ((t - m1) - xh * mx)                                 5 behind t, xh, m1, mx
//   r       += v_gamma[c] * xh  (2);   r += v_beta[c]  (1);   t_y = (y > 0 | no ReLU) ? r : 0
// hf_gn_act_adjoint
//   g        = (y > 0 | no ReLU) ? s of the consumer's data-gradient slabs : 0
//   p        = gamma[c] * g                                                             1
//   m1       = fp32( fp64 sum of the chains of p / (hw*cg) );  mx = fp32( .. of the chains of p * xh .. )
//   ga       = rstd * ((p - m1) - xh * mx)                                              4 behind p, xh, m1, mx
//   gb_rows[n][c] = fp32( fp64 sum over the slots of the chains of g ),  gw_rows: of g * xh (1 more),  gcb_rows: of ga
// hf_gn_act_adjoint2  (the tangent of hf_gn_act_adjoint inside a Hessian product; mu, rstd and g -- the step's first-order
//                      masked cotangent -- as given; g and a are read from global memory in every pass)
//   g'       = (y > 0 | no ReLU) ? s of the second sweep's cotangent slabs : 0          resident block 1
//   t        = s of the tangent convolution's slabs [+ v_conv_bias[c]]                  resident block 2
//   xh       = (a - mu) * rstd  (2);   p = gamma[c] * g  (1);   p' = gamma[c] * g'  (1)  [p' = v_gamma[c] * g + p'  (2)]
//   round 1:   T1, Tx, P1, Px, Q1, Qx = fp32( fp64 sum of the chains of t, xh * t, p, p * xh, p', p' * xh / (hw*cg) )
//   tau      = (t - T1) - xh * Tx                                                        3 behind t, xh, T1, Tx
//   round 2:   Qt = rstd * fp32( fp64 sum of the chains of p * tau / (hw*cg) )          (taken directly: no cancelling form)
//   Qs       = Qx + Qt  (1);   rT = rstd * Tx  (1);   rt = rstd * tau  (1);   ga = rstd * ((p - P1) - xh * Px)  (4)
//   ga'      = rstd * (((p' - Q1) - xh * Qs) - rt * Px) - rT * ga                        8 behind p', xh, rt, ga, Q1, Qs, Px, rT
//   gb_rows[n][c] = fp32( fp64 sum over the slots of the chains of g' ),  gw_rows: of g' * xh + g * rt (3 more),
//   gcb_rows: of ga'
//   Two blocks resident (g' and t), so the LDS is sized to the launch: instantiations for blocks of up to 2 048, 8 192 and
//   16 384 floats (25 / 73 / 137 KB with the reductions' scratch; gfx950 has 160 KB per CU), static, the smallest that holds
//   the plan's hw x span.
// hf_gn_rows_sqsum
//   out[c]   =fp32( fp64 sum over the samples, ascending, of fp32(t * t),  t = fp32(pre * rows[n][c]) )
#include "hf_common.h"

#include <math.h>

namespace {

constexpr int GN_LDS_FLOATS = 16384;  // the resident block: 64 KB
constexpr int GN_SEG = 64;            // channels of a pixel's span the plan aims at
constexpr int GN_MIN_SEG = 32;        // ... and does not go below when it trades span for workgroups
constexpr int GN_TARGET_WGS = 256;
constexpr int GN_MAX_GPS = GN_SEG / 4;  // groups per span (cg >= 4)

// ---- the plan: ONE definition, run by hf_gn_plan and by every launching entry point --------------------------------
struct GnPlan {
  int n, hw, c, groups, cg, gps, spans;
};

inline int gn_plan(GnPlan& p, int64_t n, int64_t hw, int64_t c, int64_t groups) {
  if (n <= 0 || hw <= 0 || c <= 0 || groups <= 0 || c % groups) return HF_ERR_ARG;
  const int64_t cg = c / groups;
  if (cg % 4 || hw * cg > GN_LDS_FLOATS || n > 65535 || n * hw * c > 0x7fffffffLL) return HF_ERR_ARG;
  int64_t gps = (GN_SEG + cg - 1) / cg;
  if (gps > groups) gps = groups;
  if (gps > GN_LDS_FLOATS / (hw * cg)) gps = GN_LDS_FLOATS / (hw * cg);
  while (gps > 1 && n * ((groups + gps - 1) / gps) < GN_TARGET_WGS && ((gps + 1) / 2) * cg >= GN_MIN_SEG) gps = (gps + 1) / 2;
  p = GnPlan{(int)n, (int)hw, (int)c, (int)groups, (int)cg, (int)gps, (int)((groups + gps - 1) / gps)};
  return HF_OK;
}

// ---- what a workgroup owns, and its lanes' places in the two reductions ------------------------------------------------
struct GnBlock {
  int nb, g0, ng, ch0, sq, nq, qpg;  // sample, first group, groups, first channel, quads per pixel, quads, quads per group and pixel
  long long base;                    // float index of (sample, pixel 0, channel ch0) in a dense [rows, c] map
  int wpt, nteams, team, lt, T, iters;
};

__device__ __forceinline__ GnBlock gn_block(int hw, int c, int groups, int cg, int gps) {
  GnBlock b;
  b.nb = blockIdx.y;
  b.g0 = blockIdx.x * gps;
  b.ng = groups - b.g0 < gps ? groups - b.g0 : gps;
  b.ch0 = b.g0 * cg;
  b.qpg = cg >> 2;
  b.sq = b.ng * b.qpg;
  b.nq = hw * b.sq;
  b.base = (long long)b.nb * hw * c + b.ch0;
  b.wpt = b.ng == 1 ? WAVES : b.ng == 2 ? WAVES / 2 : 1;
  b.nteams = WAVES / b.wpt;
  b.T = b.wpt * 64;
  b.team = threadIdx.x / b.T;
  b.lt = threadIdx.x - b.team * b.T;
  b.iters = (b.ng + b.nteams - 1) / b.nteams;
  return b;
}

__device__ __forceinline__ double quad_sum(const F4& s) { return (((double)s.e[0] + (double)s.e[1]) + (double)s.e[2]) + (double)s.e[3]; }

// the teams' sums: a wave's lanes by the tree, a team's waves in wave order; every lane of a team gets its team's sums.
// Called by all 256 lanes (a team without a group adds zeros).  red: K * WAVES doubles.
template <int K>
__device__ __forceinline__ void gn_team_sum(double (&v)[K], double* red, const GnBlock& b) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k * WAVES + wave] = v[k];
  }
  __syncthreads();
  const int w0 = b.team * b.wpt;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = red[k * WAVES + w0];
    for (int w = 1; w < b.wpt; ++w) s += red[k * WAVES + w0 + w];
    v[k] = s;
  }
  __syncthreads();
}

// four consecutive per-channel values (the model's parameters and the CG vector's slices sit on any 4-byte boundary)
__device__ __forceinline__ F4 ld4s(const float* p) { return F4{{p[0], p[1], p[2], p[3]}}; }

// the block's slabs summed into LDS, thread order; `extra` (nullable): a per-channel vector added behind the slab sum
__device__ __forceinline__ void gn_stage(F4* tile, const GnBlock& b, const float* src, int splits, long long slab,
                                         const float* extra, float* copy, int c) {
  for (int q = threadIdx.x; q < b.nq; q += BLOCK) {
    const int p = q / b.sq, j = q - p * b.sq;
    const long long gi = b.base + (long long)p * c + 4 * j;
    F4 v = slab_sum<8>(ld4(src + gi), src, gi, splits, slab);
    if (extra) {
      const F4 e = ld4s(extra + b.ch0 + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) v.e[k] += e.e[k];
    }
    if (copy) *reinterpret_cast<F4*>(copy + gi) = v;
    tile[q] = v;
  }
}

// the same for a cotangent: g = mask * (sum of the slabs), `mask_src` (nullable): the unit's output, y > 0
__device__ __forceinline__ void gn_stage_masked(F4* tile, const GnBlock& b, const float* gy, int splits, long long slab,
                                                const float* mask_src, int c) {
  for (int q = threadIdx.x; q < b.nq; q += BLOCK) {
    const int p = q / b.sq, j = q - p * b.sq;
    const long long gi = b.base + (long long)p * c + 4 * j;
    F4 v = slab_sum<8>(ld4(gy + gi), gy, gi, splits, slab);
    if (mask_src) {
      const F4 m = ld4(mask_src + gi);
#pragma unroll
      for (int k = 0; k < 4; ++k) v.e[k] = m.e[k] > 0.f ? v.e[k] : 0.f;
    }
    tile[q] = v;
  }
}

__global__ __launch_bounds__(BLOCK) void k_gn_forward(
    float* __restrict__ y, float* __restrict__ y2, unsigned y2_ld, float* a_out, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, const float* a, int splits, long long slab, const float* __restrict__ cbias,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu, int hw, int c, int groups, int cg,
    int gps) {
  __shared__ F4 tile[GN_LDS_FLOATS / 4];
  __shared__ double red[WAVES];
  __shared__ float smu[GN_MAX_GPS], srs[GN_MAX_GPS];
  const GnBlock b = gn_block(hw, c, groups, cg, gps);
  gn_stage(tile, b, a, splits, slab, cbias, a_out, c);
  __syncthreads();
  const double cnt = (double)hw * (double)cg;
  for (int it = 0; it < b.iters; ++it) {
    const int gl = b.team + it * b.nteams;
    const bool on = gl < b.ng;
    const int gq = on ? hw * b.qpg : 0;
    F4 s = {{0.f, 0.f, 0.f, 0.f}};
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg;
      const F4 x = tile[p * b.sq + gl * b.qpg + jj];
#pragma unroll
      for (int k = 0; k < 4; ++k) s.e[k] += x.e[k];
    }
    double v[1] = {quad_sum(s)};
    gn_team_sum<1>(v, red, b);
    const float mu = (float)(v[0] / cnt);
    s = F4{{0.f, 0.f, 0.f, 0.f}};
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg;
      const F4 x = tile[p * b.sq + gl * b.qpg + jj];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = x.e[k] - mu;
        s.e[k] += d * d;
      }
    }
    v[0] = quad_sum(s);
    gn_team_sum<1>(v, red, b);
    const float rs = (float)(1.0 / sqrt(v[0] / cnt + (double)eps));
    if (on && b.lt == 0) {
      smu[gl] = mu;
      srs[gl] = rs;
      mean_out[(long long)b.nb * groups + b.g0 + gl] = mu;
      rstd_out[(long long)b.nb * groups + b.g0 + gl] = rs;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < b.nq; q += BLOCK) {
    const int p = q / b.sq, j = q - p * b.sq, gl = j / b.qpg;
    const float mu = smu[gl], rs = srs[gl];
    const F4 x = tile[q], w = ld4s(gamma + b.ch0 + 4 * j);
    F4 t;
#pragma unroll
    for (int k = 0; k < 4; ++k) t.e[k] = ((x.e[k] - mu) * rs) * w.e[k];
    if (beta) {
      const F4 bq = ld4s(beta + b.ch0 + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) t.e[k] += bq.e[k];
    }
    if (relu) {
#pragma unroll
      for (int k = 0; k < 4; ++k) t.e[k] = t.e[k] > 0.f ? t.e[k] : 0.f;
    }
    const long long row = (long long)b.nb * hw + p;
    if (y) *reinterpret_cast<F4*>(y + row * c + b.ch0 + 4 * j) = t;
    if (y2) *reinterpret_cast<F4*>(y2 + row * y2_ld + b.ch0 + 4 * j) = t;
  }
}

__global__ __launch_bounds__(BLOCK) void k_gn_act_tangent(
    float* __restrict__ out, unsigned out_ld, const float* __restrict__ ta, int splits, long long slab,
    const float* __restrict__ v_cb, const float* __restrict__ a, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ v_gamma,
    const float* __restrict__ v_beta, const float* __restrict__ mask_src, int hw, int c, int groups, int cg, int gps) {
  __shared__ F4 tile[GN_LDS_FLOATS / 4];
  __shared__ double red[2 * WAVES];
  __shared__ float sm1[GN_MAX_GPS], smx[GN_MAX_GPS];
  const GnBlock b = gn_block(hw, c, groups, cg, gps);
  gn_stage(tile, b, ta, splits, slab, v_cb, nullptr, c);
  __syncthreads();
  const double cnt = (double)hw * (double)cg;
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  for (int it = 0; it < b.iters; ++it) {
    const int gl = b.team + it * b.nteams;
    const bool on = gl < b.ng;
    const int gq = on ? hw * b.qpg : 0;
    const float mu = on ? stat_mu[gl] : 0.f, rs = on ? stat_rs[gl] : 0.f;
    F4 s1 = {{0.f, 0.f, 0.f, 0.f}}, sx = {{0.f, 0.f, 0.f, 0.f}};
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg, j = gl * b.qpg + jj;
      const F4 t = tile[p * b.sq + j], x = ld4(a + b.base + (long long)p * c + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xh = (x.e[k] - mu) * rs;
        s1.e[k] += t.e[k];
        sx.e[k] += xh * t.e[k];
      }
    }
    double v[2] = {quad_sum(s1), quad_sum(sx)};
    gn_team_sum<2>(v, red, b);
    if (on && b.lt == 0) {
      sm1[gl] = (float)(v[0] / cnt);
      smx[gl] = (float)(v[1] / cnt);
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < b.nq; q += BLOCK) {
    const int p = q / b.sq, j = q - p * b.sq, gl = j / b.qpg;
    const float mu = stat_mu[gl], rs = stat_rs[gl], m1 = sm1[gl], mx = smx[gl];
    const long long row = (long long)b.nb * hw + p, gi = row * c + b.ch0 + 4 * j;
    const F4 t = tile[q], x = ld4(a + gi), w = ld4s(gamma + b.ch0 + 4 * j);
    F4 xh, r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xh.e[k] = (x.e[k] - mu) * rs;
      r.e[k] = (w.e[k] * rs) * ((t.e[k] - m1) - xh.e[k] * mx);
    }
    if (v_gamma) {
      const F4 vg = ld4s(v_gamma + b.ch0 + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) r.e[k] += vg.e[k] * xh.e[k];
    }
    if (v_beta) {
      const F4 vb = ld4s(v_beta + b.ch0 + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) r.e[k] += vb.e[k];
    }
    if (mask_src) {
      const F4 m = ld4(mask_src + gi);
#pragma unroll
      for (int k = 0; k < 4; ++k) r.e[k] = m.e[k] > 0.f ? r.e[k] : 0.f;
    }
    *reinterpret_cast<F4*>(out + row * out_ld + b.ch0 + 4 * j) = r;
  }
}

// one table's rows: the slots' partial quads added in slot order (fp64), rounded once, stored by slot 0
__device__ __forceinline__ void gn_row_store(float* rows, const F4& part, double* rsum, int slots, int cols, int slot, int jl,
                                             bool act, long long at) {
  if (slots > 1) {
    if (act) {
#pragma unroll
      for (int k = 0; k < 4; ++k) rsum[(slot * cols + jl) * 4 + k] = (double)part.e[k];
    }
    __syncthreads();
  }
  if (act && slot == 0) {
    F4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double s = (double)part.e[k];
      for (int sl = 1; sl < slots; ++sl) s += rsum[(sl * cols + jl) * 4 + k];
      o.e[k] = (float)s;
    }
    *reinterpret_cast<F4*>(rows + at) = o;
  }
  if (slots > 1) __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void k_gn_act_adjoint(
    float* __restrict__ ga_out, float* __restrict__ g_out, float* __restrict__ gw_rows, float* __restrict__ gb_rows,
    float* __restrict__ gcb_rows, const float* __restrict__ gy, int splits, long long slab, const float* __restrict__ a,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ mask_src, int hw, int c, int groups, int cg, int gps) {
  __shared__ F4 tile[GN_LDS_FLOATS / 4];
  __shared__ double red[2 * WAVES];
  __shared__ double rsum[BLOCK * 4];
  __shared__ float sm1[GN_MAX_GPS], smx[GN_MAX_GPS];
  const GnBlock b = gn_block(hw, c, groups, cg, gps);
  gn_stage_masked(tile, b, gy, splits, slab, mask_src, c);  // g, resident
  __syncthreads();
  const double cnt = (double)hw * (double)cg;
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  for (int it = 0; it < b.iters; ++it) {
    const int gl = b.team + it * b.nteams;
    const bool on = gl < b.ng;
    const int gq = on ? hw * b.qpg : 0;
    const float mu = on ? stat_mu[gl] : 0.f, rs = on ? stat_rs[gl] : 0.f;
    F4 s1 = {{0.f, 0.f, 0.f, 0.f}}, sx = {{0.f, 0.f, 0.f, 0.f}};
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg, j = gl * b.qpg + jj;
      const F4 g = tile[p * b.sq + j], x = ld4(a + b.base + (long long)p * c + 4 * j), w = ld4s(gamma + b.ch0 + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xh = (x.e[k] - mu) * rs, pg = w.e[k] * g.e[k];
        s1.e[k] += pg;
        sx.e[k] += pg * xh;
      }
    }
    double v[2] = {quad_sum(s1), quad_sum(sx)};
    gn_team_sum<2>(v, red, b);
    if (on && b.lt == 0) {
      sm1[gl] = (float)(v[0] / cnt);
      smx[gl] = (float)(v[1] / cnt);
    }
  }
  __syncthreads();
  // the elementwise part and the per-sample rows: lane (slot, column) walks its channel quad down the pixels
  const int cols = b.sq < BLOCK ? b.sq : BLOCK, slots = BLOCK / cols;
  const int slot = threadIdx.x / cols, jl = threadIdx.x - slot * cols;
  for (int j0 = 0; j0 < b.sq; j0 += cols) {
    const int j = j0 + jl;
    const bool act = slot < slots && j < b.sq;
    F4 sb = {{0.f, 0.f, 0.f, 0.f}}, sw = {{0.f, 0.f, 0.f, 0.f}}, sc = {{0.f, 0.f, 0.f, 0.f}};
    if (act) {
      const int gl = j / b.qpg;
      const float mu = stat_mu[gl], rs = stat_rs[gl], m1 = sm1[gl], mx = smx[gl];
      const F4 w = ld4s(gamma + b.ch0 + 4 * j);
      for (int p = slot; p < hw; p += slots) {
        const long long gi = b.base + (long long)p * c + 4 * j;
        const F4 g = tile[p * b.sq + j], x = ld4(a + gi);
        F4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float xh = (x.e[k] - mu) * rs, pg = w.e[k] * g.e[k];
          o.e[k] = rs * ((pg - m1) - xh * mx);
          sb.e[k] += g.e[k];
          sw.e[k] += g.e[k] * xh;
          sc.e[k] += o.e[k];
        }
        *reinterpret_cast<F4*>(ga_out + gi) = o;
        if (g_out) *reinterpret_cast<F4*>(g_out + gi) = g;
      }
    }
    const long long at = (long long)b.nb * c + b.ch0 + 4 * j;
    if (gw_rows) gn_row_store(gw_rows, sw, rsum, slots, cols, slot, jl, act, at);
    if (gb_rows) gn_row_store(gb_rows, sb, rsum, slots, cols, slot, jl, act, at);
    if (gcb_rows) gn_row_store(gcb_rows, sc, rsum, slots, cols, slot, jl, act, at);
  }
}

// ---- the tangent of the adjoint (a Hessian product's second sweep): TWO resident blocks ---------------------------------
// what the three passes of k_gn_act_adjoint2 share per element: xh, p = gamma g and p' = v_gamma g + gamma g'
struct Gn2Point {
  float xh, p, pp;
};

__device__ __forceinline__ Gn2Point gn2_point(float x, float g, float gp, float w, float vg, bool has_vg, float mu, float rs) {
  Gn2Point o;
  o.xh = (x - mu) * rs;
  o.p = w * g;
  o.pp = w * gp;
  if (has_vg) o.pp = vg * g + o.pp;
  return o;
}

// per-group results of the two rounds, as the elementwise part reads them
enum { G2_T1, G2_TX, G2_P1, G2_PX, G2_Q1, G2_QS, G2_RT, G2_STATS };

// FLOATS: the floats of ONE resident block this instantiation reserves (hw * span <= FLOATS); the launch takes the smallest
template <int FLOATS>
__global__ __launch_bounds__(BLOCK) void k_gn_act_adjoint2(
    float* __restrict__ ga2_out, float* __restrict__ gw_rows, float* __restrict__ gb_rows, float* __restrict__ gcb_rows,
    const float* __restrict__ gy2, int splits, long long slab, const float* __restrict__ ta, int t_splits, long long t_slab,
    const float* __restrict__ v_cb, const float* __restrict__ a, const float* __restrict__ g1,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ v_gamma, const float* __restrict__ mask_src, int hw, int c, int groups, int cg, int gps) {
  __shared__ F4 tg[FLOATS / 4];  // g' = mask * (sum of the second sweep's cotangent slabs)
  __shared__ F4 tt[FLOATS / 4];  // t  = sum of the tangent convolution's slabs [+ v_conv_bias]
  __shared__ double red[6 * WAVES];
  __shared__ double rsum[BLOCK * 4];
  __shared__ float stats[G2_STATS][GN_MAX_GPS];
  const GnBlock b = gn_block(hw, c, groups, cg, gps);
  gn_stage_masked(tg, b, gy2, splits, slab, mask_src, c);
  gn_stage(tt, b, ta, t_splits, t_slab, v_cb, nullptr, c);
  __syncthreads();
  const double cnt = (double)hw * (double)cg;
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  const bool has_vg = v_gamma != nullptr;
  const F4 zero = {{0.f, 0.f, 0.f, 0.f}};
  for (int it = 0; it < b.iters; ++it) {
    const int gl = b.team + it * b.nteams;
    const bool on = gl < b.ng;
    const int gq = on ? hw * b.qpg : 0;
    const float mu = on ? stat_mu[gl] : 0.f, rs = on ? stat_rs[gl] : 0.f;
    // round 1: T1, Tx, P1, Px, Q1, Qx
    F4 s[6] = {zero, zero, zero, zero, zero, zero};
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg, j = gl * b.qpg + jj;
      const long long gi = b.base + (long long)p * c + 4 * j;
      const F4 gp = tg[p * b.sq + j], t = tt[p * b.sq + j], x = ld4(a + gi), g = ld4(g1 + gi);
      const F4 w = ld4s(gamma + b.ch0 + 4 * j), vg = has_vg ? ld4s(v_gamma + b.ch0 + 4 * j) : zero;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const Gn2Point o = gn2_point(x.e[k], g.e[k], gp.e[k], w.e[k], vg.e[k], has_vg, mu, rs);
        s[0].e[k] += t.e[k];
        s[1].e[k] += o.xh * t.e[k];
        s[2].e[k] += o.p;
        s[3].e[k] += o.p * o.xh;
        s[4].e[k] += o.pp;
        s[5].e[k] += o.pp * o.xh;
      }
    }
    double v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = quad_sum(s[i]);
    gn_team_sum<6>(v, red, b);
    const float T1 = (float)(v[0] / cnt), Tx = (float)(v[1] / cnt);
    // round 2: E[p * tau], from the resident block, T1 and Tx known (no E[p t] - T1 P1 - Tx Px: that form cancels)
    F4 s2 = zero;
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg, j = gl * b.qpg + jj;
      const long long gi = b.base + (long long)p * c + 4 * j;
      const F4 t = tt[p * b.sq + j], x = ld4(a + gi), g = ld4(g1 + gi), w = ld4s(gamma + b.ch0 + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float xh = (x.e[k] - mu) * rs, tau = (t.e[k] - T1) - xh * Tx;
        s2.e[k] += (w.e[k] * g.e[k]) * tau;
      }
    }
    double v2[1] = {quad_sum(s2)};
    gn_team_sum<1>(v2, red, b);
    if (on && b.lt == 0) {
      const float Qt = rs * (float)(v2[0] / cnt);
      stats[G2_T1][gl] = T1;
      stats[G2_TX][gl] = Tx;
      stats[G2_P1][gl] = (float)(v[2] / cnt);
      stats[G2_PX][gl] = (float)(v[3] / cnt);
      stats[G2_Q1][gl] = (float)(v[4] / cnt);
      stats[G2_QS][gl] = (float)(v[5] / cnt) + Qt;
      stats[G2_RT][gl] = rs * Tx;
    }
  }
  __syncthreads();
  // the elementwise part and the per-sample rows, laid out as in k_gn_act_adjoint
  const int cols = b.sq < BLOCK ? b.sq : BLOCK, slots = BLOCK / cols;
  const int slot = threadIdx.x / cols, jl = threadIdx.x - slot * cols;
  for (int j0 = 0; j0 < b.sq; j0 += cols) {
    const int j = j0 + jl;
    const bool act = slot < slots && j < b.sq;
    F4 sb = zero, sw = zero, sc = zero;
    if (act) {
      const int gl = j / b.qpg;
      const float mu = stat_mu[gl], rs = stat_rs[gl];
      const float T1 = stats[G2_T1][gl], Tx = stats[G2_TX][gl], P1 = stats[G2_P1][gl], Px = stats[G2_PX][gl];
      const float Q1 = stats[G2_Q1][gl], Qs = stats[G2_QS][gl], rT = stats[G2_RT][gl];
      const F4 w = ld4s(gamma + b.ch0 + 4 * j), vg = has_vg ? ld4s(v_gamma + b.ch0 + 4 * j) : zero;
      for (int p = slot; p < hw; p += slots) {
        const long long gi = b.base + (long long)p * c + 4 * j;
        const F4 gp = tg[p * b.sq + j], t = tt[p * b.sq + j], x = ld4(a + gi), g = ld4(g1 + gi);
        F4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const Gn2Point e = gn2_point(x.e[k], g.e[k], gp.e[k], w.e[k], vg.e[k], has_vg, mu, rs);
          const float rt = rs * ((t.e[k] - T1) - e.xh * Tx);
          const float ga = rs * ((e.p - P1) - e.xh * Px);
          o.e[k] = rs * (((e.pp - Q1) - e.xh * Qs) - rt * Px) - rT * ga;
          sb.e[k] += gp.e[k];
          sw.e[k] += gp.e[k] * e.xh + g.e[k] * rt;
          sc.e[k] += o.e[k];
        }
        *reinterpret_cast<F4*>(ga2_out + gi) = o;
      }
    }
    const long long at = (long long)b.nb * c + b.ch0 + 4 * j;
    if (gw_rows) gn_row_store(gw_rows, sw, rsum, slots, cols, slot, jl, act, at);
    if (gb_rows) gn_row_store(gb_rows, sb, rsum, slots, cols, slot, jl, act, at);
    if (gcb_rows) gn_row_store(gcb_rows, sc, rsum, slots, cols, slot, jl, act, at);
  }
}

// out[c] = sum_n (pre * rows[n][c])^2 for up to three tables (blockIdx.y), one lane per channel
struct GnSqTables {
  float* out[3];
  const float* rows[3];
};

__global__ __launch_bounds__(BLOCK) void k_gn_rows_sqsum(GnSqTables tabs, float pre, int n, int c) {
  float* out = tabs.out[blockIdx.y];
  const float* rows = tabs.rows[blockIdx.y];
  const int ch = blockIdx.x * BLOCK + threadIdx.x;
  if (!out || ch >= c) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    const float t = pre * rows[(long long)i * c + ch];
    s += (double)(t * t);
  }
  out[ch] = (float)s;
}

// ---- validators: everything a launch assumes, checked before anything is touched ------------------------------------
inline bool gn_ld_ok(int64_t ld, const GnPlan& p) {
  return ld == 0 || (ld >= p.c && (ld & 3) == 0 && (int64_t)p.n * p.hw * ld <= 0x7fffffffLL);
}

inline int gn_slabs_ok(const void* slabs, int splits, int64_t slab_stride, const GnPlan& p) {
  if (!slabs || splits < 1) return HF_ERR_ARG;
  if (splits > 1 && (slab_stride < (int64_t)p.n * p.hw * p.c || (slab_stride & 3))) return HF_ERR_ARG;
  return HF_OK;
}

template <size_t N>
inline int gn_aligned(const void* const (&ptrs)[N]) {
  for (const void* q : ptrs)
    if (q && !aligned16(q)) return HF_ERR_ARG;
  return HF_OK;
}

}  // namespace

int hf_gn_plan(int64_t n, int64_t hw, int64_t c, int64_t groups) {
  GnPlan p;
  const int rc = gn_plan(p, n, hw, c, groups);
  return rc != HF_OK ? rc : p.gps * p.cg;
}

int hf_gn_forward(void* y, void* y2, int64_t y2_ld, void* a_out, void* mean, void* rstd, const void* a, int splits,
                  int64_t slab_stride, const void* conv_bias, const void* gamma, const void* beta, double eps, int relu,
                  int64_t n, int64_t hw, int64_t c, int64_t groups, int dtype, void* stream) {
  GnPlan p;
  if (dtype != HF_F32 || gn_plan(p, n, hw, c, groups) != HF_OK) return HF_ERR_ARG;
  if ((!y && !y2) || !mean || !rstd || !gamma || !(eps >= 0.0) || !(eps - eps == 0.0)) return HF_ERR_ARG;
  if (gn_slabs_ok(a, splits, slab_stride, p) != HF_OK || (y2 && (y2_ld == 0 || !gn_ld_ok(y2_ld, p)))) return HF_ERR_ARG;
  const void* al[] = {y, y2, a_out, a};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_forward, dim3(p.spans, p.n), dim3(BLOCK), 0, (hipStream_t)stream, (float*)y, (float*)y2,
                     (unsigned)y2_ld, (float*)a_out, (float*)mean, (float*)rstd, (const float*)a, splits,
                     (long long)slab_stride, (const float*)conv_bias, (const float*)gamma, (const float*)beta, (float)eps,
                     relu, p.hw, p.c, p.groups, p.cg, p.gps);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_act_tangent(void* out, int64_t out_ld, const void* t_a, int splits, int64_t slab_stride, const void* v_conv_bias,
                      const void* a, const void* mean, const void* rstd, const void* gamma, const void* v_gamma,
                      const void* v_beta, const void* mask_src, int64_t n, int64_t hw, int64_t c, int64_t groups, int dtype,
                      void* stream) {
  GnPlan p;
  if (dtype != HF_F32 || gn_plan(p, n, hw, c, groups) != HF_OK) return HF_ERR_ARG;
  if (!out || !a || !mean || !rstd || !gamma || !gn_ld_ok(out_ld, p)) return HF_ERR_ARG;
  if (gn_slabs_ok(t_a, splits, slab_stride, p) != HF_OK) return HF_ERR_ARG;
  const void* al[] = {out, t_a, a, mask_src};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_act_tangent, dim3(p.spans, p.n), dim3(BLOCK), 0, (hipStream_t)stream, (float*)out,
                     (unsigned)(out_ld ? out_ld : c), (const float*)t_a, splits, (long long)slab_stride,
                     (const float*)v_conv_bias, (const float*)a, (const float*)mean, (const float*)rstd,
                     (const float*)gamma, (const float*)v_gamma, (const float*)v_beta, (const float*)mask_src, p.hw, p.c,
                     p.groups, p.cg, p.gps);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_act_adjoint(void* ga, void* g, void* gw_rows, void* gb_rows, void* gcb_rows, const void* gy, int splits,
                      int64_t slab_stride, const void* a, const void* mean, const void* rstd, const void* gamma,
                      const void* mask_src, int64_t n, int64_t hw, int64_t c, int64_t groups, int dtype, void* stream) {
  GnPlan p;
  if (dtype != HF_F32 || gn_plan(p, n, hw, c, groups) != HF_OK) return HF_ERR_ARG;
  if (!ga || !a || !mean || !rstd || !gamma) return HF_ERR_ARG;
  if (gn_slabs_ok(gy, splits, slab_stride, p) != HF_OK) return HF_ERR_ARG;
  const void* al[] = {ga, g, gw_rows, gb_rows, gcb_rows, gy, a, mask_src};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_act_adjoint, dim3(p.spans, p.n), dim3(BLOCK), 0, (hipStream_t)stream, (float*)ga, (float*)g,
                     (float*)gw_rows, (float*)gb_rows, (float*)gcb_rows, (const float*)gy, splits, (long long)slab_stride,
                     (const float*)a, (const float*)mean, (const float*)rstd, (const float*)gamma, (const float*)mask_src,
                     p.hw, p.c, p.groups, p.cg, p.gps);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_act_adjoint2(void* ga2, void* gw_rows, void* gb_rows, void* gcb_rows, const void* gy2, int splits,
                       int64_t slab_stride, const void* t_a, int t_splits, int64_t t_slab_stride, const void* v_conv_bias,
                       const void* a, const void* g, const void* mean, const void* rstd, const void* gamma,
                       const void* v_gamma, const void* mask_src, int64_t n, int64_t hw, int64_t c, int64_t groups, int dtype,
                       void* stream) {
  GnPlan p;
  if (dtype != HF_F32 || gn_plan(p, n, hw, c, groups) != HF_OK) return HF_ERR_ARG;
  if (!ga2 || !a || !g || !mean || !rstd || !gamma) return HF_ERR_ARG;
  if (gn_slabs_ok(gy2, splits, slab_stride, p) != HF_OK || gn_slabs_ok(t_a, t_splits, t_slab_stride, p) != HF_OK)
    return HF_ERR_ARG;
  const void* al[] = {ga2, gw_rows, gb_rows, gcb_rows, gy2, t_a, a, g, mask_src};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  // LDS sized to the launch: three instantiations with static LDS (2 blocks of 8 / 32 / 64 KB + 9 KB of scratch), the
  // smallest that holds the plan's block hw * span -- nothing to set at run time, and nothing a graph capture could meet
  const int block = p.hw * p.gps * p.cg;
  auto kernel = block <= GN_LDS_FLOATS / 8   ? k_gn_act_adjoint2<GN_LDS_FLOATS / 8>
                : block <= GN_LDS_FLOATS / 2 ? k_gn_act_adjoint2<GN_LDS_FLOATS / 2>
                                             : k_gn_act_adjoint2<GN_LDS_FLOATS>;
  hipLaunchKernelGGL(kernel, dim3(p.spans, p.n), dim3(BLOCK), 0, (hipStream_t)stream, (float*)ga2, (float*)gw_rows,
                     (float*)gb_rows, (float*)gcb_rows, (const float*)gy2, splits, (long long)slab_stride, (const float*)t_a,
                     t_splits, (long long)t_slab_stride, (const float*)v_conv_bias, (const float*)a, (const float*)g,
                     (const float*)mean, (const float*)rstd, (const float*)gamma, (const float*)v_gamma,
                     (const float*)mask_src, p.hw, p.c, p.groups, p.cg, p.gps);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_rows_sqsum(void* out_w, const void* rows_w, void* out_b, const void* rows_b, void* out_cb, const void* rows_cb,
                     double pre, int64_t n, int64_t c, int dtype, void* stream) {
  if (dtype != HF_F32 || n <= 0 || c <= 0 || n * c > 0x7fffffffLL || !(pre - pre == 0.0)) return HF_ERR_ARG;
  if ((!out_w && !out_b && !out_cb) || (out_w && !rows_w) || (out_b && !rows_b) || (out_cb && !rows_cb)) return HF_ERR_ARG;
  GnSqTables tabs = {{(float*)out_w, (float*)out_b, (float*)out_cb},
                     {(const float*)rows_w, (const float*)rows_b, (const float*)rows_cb}};
  hipLaunchKernelGGL(k_gn_rows_sqsum, dim3((unsigned)((c + BLOCK - 1) / BLOCK), 3), dim3(BLOCK), 0, (hipStream_t)stream,
                     tabs, (float)pre, (int)n, (int)c);
  HF_HIP(hipGetLastError());
  return HF_OK;
}
