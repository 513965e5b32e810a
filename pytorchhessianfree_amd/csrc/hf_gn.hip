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
//
// Split family (hf_gn_split_*): blocks beyond one workgroup's LDS -- GroupNorm(1, C), large maps; any hw * cg with
// cg <= 16 384.  A bigger tile would not do (160 KB of LDS per CU: 2.4 x the limit), so the work is split differently:
//
// Work split.  A (sample, group) block is cut along the PIXELS into `parts` ranges of part_pixels pixels, the last one
// what is left.  A workgroup owns sample x span of whole groups x one part: a GnBlock with a pixel offset and a pixel
// count, part_pixels * span <= GN_LDS_FLOATS, so the part is resident exactly as a whole block is above -- the same staging
// helpers, teams and slots x columns layout, over the part's pixels.  Grid (parts, spans, n).  gn_split_plan: the span aims
// at GN_SEG channels and is not traded for workgroups; part_pixels is (halved while the launch has fewer than 256 workgroups
// and a part keeps GN_PART_FLOOR = 4 096 floats).
//
// Two ordinary launches per direction, in stream order: a REDUCE launch stages the part once, writes what the apply
// launch reads back (the summed map, the raw tangent, the masked cotangent) and leaves two fp64 partial sums per (sample,
// group, part) in the caller's table [n, groups, parts, 2]; every workgroup of the APPLY launch adds the partials of its
// groups itself (lane gl < groups of the span, part order, fp64) and does the elementwise part from global memory -- it
// keeps no tile (128 B - 8 KB of LDS), the part is L2-resident from the launch before.  No cooperative launch, no waiting
// of one workgroup on another, no atomics: every order depends on the shape alone, two launches agree bitwise.
//
// Arithmetic chains (n_i = pixels of part i x cg, N = hw * cg; "chains" = the lanes' fp32 chains over the PART, at most
// ceil(part_pixels * cg / 256) terms, added in fp64 as above; everything over the parts is fp64)
// hf_gn_split_stats
//   s        = slab 0 + slab 1 + .. [+ conv_bias[c]]  -> a_out                           as above
//   S_i      = fp64 sum of the chains of s
//   c_i      = fp32( S_i / n_i )                                                         the part's own centre, ONE rounding
//   Q_i      = fp64 sum of the chains of q,  d = s - c_i;  q = d * d                     (a shifted sum about the part's own
//              mean: no E[x^2] - mu^2)
// hf_gn_split_forward
//   m        = (S_0 + S_1 + ..) / N;   c_i = fp32( S_i / n_i ) again: the same number
//   M2       = sum_i (Q_i - n_i (S_i/n_i - c_i)^2) + sum_i n_i (S_i/n_i - m)^2            the two sums apart, each in part
//              order; exact for any c_i; a constant block gives 0 + 0, clamped at 0
//   mu       = fp32( m );   rstd = fp32( 1 / sqrt( M2 / N + eps ) )                       ONE rounding each
//   y        = act( ((s - mu) * rstd) * gamma[c] + beta[c] )                              hf_gn_forward's chain, s from the map
// hf_gn_split_tangent_sums
//   t        = s of the tangent convolution's slabs [+ v_conv_bias[c]]  -> out (raw, pitch out_ld)
//   xh       = (a - mu) * rstd                                                            2
//   partials = fp64 sums of the chains of t and of xh * t
// hf_gn_split_act_tangent  (t: read back from out by the lane that rewrites it)
//   m1, mx   = fp32( fp64 sum of the parts' partials / N )
//   r        = (gamma[c] * rstd) * ((t - m1) - xh * mx);  += v_gamma[c] * xh;  += v_beta[c];  the mask       hf_gn_act_tangent's
// hf_gn_split_adjoint_sums
//   g        = (y > 0 | no ReLU) ? s of the consumer's data-gradient slabs : 0  -> g
//   p        = gamma[c] * g  (1);   partials = fp64 sums of the chains of p and of p * xh
//   gb_rows[n * parts + part][c] = fp32( fp64 sum over the slots of the chains of g down the part's pixels ),  gw_rows: of g * xh
// hf_gn_split_act_adjoint  (g: read back; it may be ga's own buffer)
//   m1, mx   = fp32( fp64 sum of the parts' partials / N )
//   ga       = rstd * ((p - m1) - xh * mx)                                                hf_gn_act_adjoint's
//   gcb_rows[n * parts + part][c] = fp32( fp64 sum over the slots of the chains of ga )
// hf_gn_split_adjoint2_sums  (the split form of hf_gn_act_adjoint2; mu, rstd, g as there.  ONE reduce launch although Qt's
//                      mean needs T1 and Tx first: they are the tangent sweep's -- hf_gn_split_tangent_sums left sum t and
//                      sum xh * t of the SAME t per part in its table, and nothing between that sweep and this one of the same
//                      product writes it -- so tau is formed here and p * tau is reduced directly: five sums, no cancelling
//                      E[p t] - T1 P1 - Tx Px)
//   g'       = (y > 0 | no ReLU) ? s of the second sweep's cotangent slabs : 0  -> gp     resident block 1
//   t        = s of the tangent convolution's slabs [+ v_conv_bias[c]]  -> t              resident block 2 (the tangent sweep
//              rewrote its operand in place: the raw t is summed again, the same additions in the same order)
//   T1, Tx   = fp32( fp64 sum of the tangent table's partials, part order / N )           hf_gn_split_act_tangent's m1, mx
//   xh, p, p' as in hf_gn_act_adjoint2;   tau = (t - T1) - xh * Tx                        3 behind t, xh, T1, Tx
//   partials = fp64 sums of the chains of p, p * xh, p', p' * xh, p * tau                 [n, groups, parts, 5]
//   gb_rows[n * parts + part][c] = fp32( fp64 sum over the slots of the chains of g' down the part's pixels ),
//   gw_rows: of g' * xh + g * rt,  rt = rstd * tau  (3 more)
//   Both blocks resident as in hf_gn_act_adjoint2: instantiations for parts of up to 8 192 and 16 384 floats (73 / 137 KB).
//   Bytes per element: this launch reads 4 (s2 + sT) of slabs [+ 4: the mask] + 8 (a, g; again from L2 in the rows' pass) and
//   writes 8 (g', t); the apply launch reads 16 (g', t, a, g) and writes 4.  Summing the slabs again in the apply launch would
//   trade those 8 + 8 for 4 (s2 + sT) [+ 4] more reads: no gain from s2 + sT = 3 [4] on, and a Hessian product's cotangent
//   alone arrives in two slabs or more wherever the consumer is a dense convolution (its extras are more slabs).
// hf_gn_split_act_adjoint2  (g': read back; it may be ga2's own buffer)
//   P1, Px, Q1, Qx = fp32( fp64 sum of the parts' partials / N );  Qt = rstd * fp32( .. of p * tau .. );  T1, Tx as above
//   Qs, rT, rt, ga, ga'                                                                    hf_gn_act_adjoint2's, per element
//   gcb_rows[n * parts + part][c] = fp32( fp64 sum over the slots of the chains of ga' )
// hf_gn_split_rows_sqsum
//   row      = fp32( fp64 sum over the sample's parts, part order, of rows[n * parts + part][c] )      ONE rounding
//   out[c]   = fp32( fp64 sum over the samples, ascending, of fp32(t * t),  t = fp32(pre * row) )
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

// ---- the split family's plan: ONE definition, run by hf_gn_split_plan and by every launching entry point of the family ---
// The span as above (GN_SEG channels of a pixel, whole groups; never traded for workgroups: the parts are).  A part:
// part_pixels = min(hw, GN_LDS_FLOATS / span) pixels, halved (rounded up) while the launch has fewer than 256 workgroups
// and a part keeps at least GN_PART_FLOOR = 4 096 floats -- four quads per lane: below that the staging loop is one or two
// passes and a workgroup's fixed cost (the teams' trees, the barriers) outweighs what it moves.  parts = ceil(hw /
// part_pixels) <= hw; the last part takes what is left.
constexpr int GN_PART_FLOOR = 4096;

struct GnSplitPlan {
  GnPlan g;       // hw, c, groups, cg, gps, spans as in the one-launch family
  int parts, pp;  // parts per (sample, group) block, pixels of a part
};

inline int gn_split_plan(GnSplitPlan& s, int64_t n, int64_t hw, int64_t c, int64_t groups) {
  if (n <= 0 || hw <= 0 || c <= 0 || groups <= 0 || c % groups) return HF_ERR_ARG;
  const int64_t cg = c / groups;
  if (cg % 4 || cg > GN_LDS_FLOATS || n > 65535 || n * hw * c > 0x7fffffffLL) return HF_ERR_ARG;
  int64_t gps = (GN_SEG + cg - 1) / cg;
  if (gps > groups) gps = groups;
  const int64_t span = gps * cg, spans = (groups + gps - 1) / gps;  // span <= max(cg, 2 * GN_SEG) <= GN_LDS_FLOATS
  if (spans > 65535) return HF_ERR_ARG;
  int64_t pp = GN_LDS_FLOATS / span;
  if (pp > hw) pp = hw;
  while (n * spans * ((hw + pp - 1) / pp) < GN_TARGET_WGS && ((pp + 1) / 2) * span >= GN_PART_FLOOR) pp = (pp + 1) / 2;
  s.g = GnPlan{(int)n, (int)hw, (int)c, (int)groups, (int)cg, (int)gps, (int)spans};
  s.parts = (int)((hw + pp - 1) / pp);
  s.pp = (int)pp;
  return HF_OK;
}

// ---- what a workgroup owns, and its lanes' places in the two reductions ------------------------------------------------
struct GnBlock {
  int nb, g0, ng, ch0, sq, nq, qpg;  // sample, first group, groups, first channel, quads per pixel, quads, quads per group and pixel
  int p0, np;                        // first pixel and pixels of the block (a whole sample: 0, hw; a part of the split family: its range)
  long long row0, base;              // row of pixel p0, and the float index of (that row, channel ch0), in a dense [rows, c] map
  int wpt, nteams, team, lt, T, iters;
};

// sample nb, span sx, the pixels p0 .. p0 + np - 1
__device__ __forceinline__ GnBlock gn_block_of(int nb, int sx, int p0, int np, int hw, int c, int groups, int cg, int gps) {
  GnBlock b;
  b.nb = nb;
  b.g0 = sx * gps;
  b.ng = groups - b.g0 < gps ? groups - b.g0 : gps;
  b.ch0 = b.g0 * cg;
  b.qpg = cg >> 2;
  b.sq = b.ng * b.qpg;
  b.p0 = p0;
  b.np = np;
  b.nq = np * b.sq;
  b.row0 = (long long)nb * hw + p0;
  b.base = b.row0 * c + b.ch0;
  b.wpt = b.ng == 1 ? WAVES : b.ng == 2 ? WAVES / 2 : 1;
  b.nteams = WAVES / b.wpt;
  b.T = b.wpt * 64;
  b.team = threadIdx.x / b.T;
  b.lt = threadIdx.x - b.team * b.T;
  b.iters = (b.ng + b.nteams - 1) / b.nteams;
  return b;
}

// one-launch family, grid (spans, n): the whole (sample, span) block
__device__ __forceinline__ GnBlock gn_block(int hw, int c, int groups, int cg, int gps) {
  return gn_block_of(blockIdx.y, blockIdx.x, 0, hw, hw, c, groups, cg, gps);
}

// split family, grid (parts, spans, n): part blockIdx.x of the block, pp pixels (the last part: what is left)
__device__ __forceinline__ GnBlock gn_part(int hw, int c, int groups, int cg, int gps, int pp) {
  const int p0 = blockIdx.x * pp;
  return gn_block_of(blockIdx.z, blockIdx.y, p0, hw - p0 < pp ? hw - p0 : pp, hw, c, groups, cg, gps);
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

// the block's slabs summed into LDS, thread order; `extra` (nullable): a per-channel vector added behind the slab sum;
// `copy` (nullable): the sum also goes to a [rows, copy_ld] map
__device__ __forceinline__ void gn_stage(F4* tile, const GnBlock& b, const float* src, int splits, long long slab,
                                         const float* extra, float* copy, int c, long long copy_ld) {
  for (int q = threadIdx.x; q < b.nq; q += BLOCK) {
    const int p = q / b.sq, j = q - p * b.sq;
    const long long gi = b.base + (long long)p * c + 4 * j;
    F4 v = slab_sum<8>(ld4(src + gi), src, gi, splits, slab);
    if (extra) {
      const F4 e = ld4s(extra + b.ch0 + 4 * j);
#pragma unroll
      for (int k = 0; k < 4; ++k) v.e[k] += e.e[k];
    }
    if (copy) *reinterpret_cast<F4*>(copy + (b.row0 + p) * copy_ld + b.ch0 + 4 * j) = v;
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
  gn_stage(tile, b, a, splits, slab, cbias, a_out, c, c);
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
  gn_stage(tile, b, ta, splits, slab, v_cb, nullptr, c, c);
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

// ga' of one element from the group's seven numbers; rt = rstd * tau on the way (the scale's row reads it)
__device__ __forceinline__ float gn2_ga2(const Gn2Point& e, float t, float rs, float T1, float Tx, float P1, float Px,
                                         float Q1, float Qs, float rT, float& rt) {
  rt = rs * ((t - T1) - e.xh * Tx);
  const float ga = rs * ((e.p - P1) - e.xh * Px);
  return rs * (((e.pp - Q1) - e.xh * Qs) - rt * Px) - rT * ga;
}

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
  gn_stage(tt, b, ta, t_splits, t_slab, v_cb, nullptr, c, c);
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
          float rt;
          o.e[k] = gn2_ga2(e, t.e[k], rs, T1, Tx, P1, Px, Q1, Qs, rT, rt);
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

// ---- the split family: blocks beyond one workgroup's LDS, a reduce and an apply launch per direction -------------------
// (the header's "Split family" section: work split, partials table, arithmetic chains)

// the partials of (sample, group gl of the block's span): [parts][K] doubles of the table [n, groups, parts, K]
template <typename D>
__device__ __forceinline__ D* gn_tab(D* tab, const GnBlock& b, int groups, int gl, int K = 2) {
  return tab + ((long long)b.nb * groups + b.g0 + gl) * gridDim.x * K;
}

// apply launches: lane gl < ng adds the two partial sums of its group over the parts, in part order, and leaves their
// means over the whole block (one rounding each) in sm1 / smx; ends with a barrier
__device__ __forceinline__ void gn_parts_means(float* sm1, float* smx, const double* tab, const GnBlock& b, int groups,
                                               double cnt) {
  if ((int)threadIdx.x < b.ng) {
    const double* t = gn_tab(tab, b, groups, threadIdx.x);
    double s1 = 0.0, sx = 0.0;
    for (int i = 0; i < (int)gridDim.x; ++i) {
      s1 += t[2 * i];
      sx += t[2 * i + 1];
    }
    sm1[threadIdx.x] = (float)(s1 / cnt);
    smx[threadIdx.x] = (float)(sx / cnt);
  }
  __syncthreads();
}

__global__ __launch_bounds__(BLOCK) void k_gn_split_stats(float* a_out, double* __restrict__ tab, const float* a, int splits,
                                                          long long slab, const float* __restrict__ cbias, int hw, int c,
                                                          int groups, int cg, int gps, int pp) {
  __shared__ F4 tile[GN_LDS_FLOATS / 4];
  __shared__ double red[WAVES];
  const GnBlock b = gn_part(hw, c, groups, cg, gps, pp);
  gn_stage(tile, b, a, splits, slab, cbias, a_out, c, c);
  __syncthreads();
  const double cnt = (double)b.np * (double)cg;  // n_i
  for (int it = 0; it < b.iters; ++it) {
    const int gl = b.team + it * b.nteams;
    const bool on = gl < b.ng;
    const int gq = on ? b.np * b.qpg : 0;
    F4 s = {{0.f, 0.f, 0.f, 0.f}};
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg;
      const F4 x = tile[p * b.sq + gl * b.qpg + jj];
#pragma unroll
      for (int k = 0; k < 4; ++k) s.e[k] += x.e[k];
    }
    double v[1] = {quad_sum(s)};
    gn_team_sum<1>(v, red, b);
    const double S = v[0];
    const float ci = (float)(S / cnt);  // the part's own centre: the apply launch takes the same number from S and n_i
    s = F4{{0.f, 0.f, 0.f, 0.f}};
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg;
      const F4 x = tile[p * b.sq + gl * b.qpg + jj];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = x.e[k] - ci;
        s.e[k] += d * d;
      }
    }
    v[0] = quad_sum(s);
    gn_team_sum<1>(v, red, b);
    if (on && b.lt == 0) {
      double* o = gn_tab(tab, b, groups, gl) + 2 * blockIdx.x;
      o[0] = S;
      o[1] = v[0];
    }
  }
}

__global__ __launch_bounds__(BLOCK) void k_gn_split_forward(
    float* __restrict__ y, float* __restrict__ y2, unsigned y2_ld, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, const float* __restrict__ s_map, const double* __restrict__ tab,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu, int hw, int c, int groups, int cg,
    int gps, int pp) {
  __shared__ float smu[GN_MAX_GPS], srs[GN_MAX_GPS];
  const GnBlock b = gn_part(hw, c, groups, cg, gps, pp);
  if ((int)threadIdx.x < b.ng) {  // Chan's combination of the parts' (S_i, Q_i about c_i), all fp64, part order
    const double* t = gn_tab(tab, b, groups, threadIdx.x);
    const int parts = gridDim.x;
    const double cnt = (double)hw * (double)cg;
    double S = 0.0;
    for (int i = 0; i < parts; ++i) S += t[2 * i];
    const double m = S / cnt;
    double within = 0.0, between = 0.0;
    for (int i = 0; i < parts; ++i) {
      const int np = hw - i * pp < pp ? hw - i * pp : pp;
      const double ni = (double)np * (double)cg, mi = t[2 * i] / ni;
      const double dc = mi - (double)(float)mi, dm = mi - m;
      within += t[2 * i + 1] - ni * (dc * dc);
      between += ni * (dm * dm);
    }
    double M2 = within + between;
    M2 = M2 > 0.0 ? M2 : 0.0;
    const float mu = (float)m, rs = (float)(1.0 / sqrt(M2 / cnt + (double)eps));
    smu[threadIdx.x] = mu;
    srs[threadIdx.x] = rs;
    if (blockIdx.x == 0) {
      mean_out[(long long)b.nb * groups + b.g0 + threadIdx.x] = mu;
      rstd_out[(long long)b.nb * groups + b.g0 + threadIdx.x] = rs;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < b.nq; q += BLOCK) {
    const int p = q / b.sq, j = q - p * b.sq, gl = j / b.qpg;
    const float mu = smu[gl], rs = srs[gl];
    const F4 x = ld4(s_map + b.base + (long long)p * c + 4 * j), w = ld4s(gamma + b.ch0 + 4 * j);
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
    const long long row = b.row0 + p;
    if (y) *reinterpret_cast<F4*>(y + row * c + b.ch0 + 4 * j) = t;
    if (y2) *reinterpret_cast<F4*>(y2 + row * y2_ld + b.ch0 + 4 * j) = t;
  }
}

__global__ __launch_bounds__(BLOCK) void k_gn_split_tangent_sums(
    float* __restrict__ out, unsigned out_ld, double* __restrict__ tab, const float* __restrict__ ta, int splits,
    long long slab, const float* __restrict__ v_cb, const float* __restrict__ a, const float* __restrict__ mean,
    const float* __restrict__ rstd, int hw, int c, int groups, int cg, int gps, int pp) {
  __shared__ F4 tile[GN_LDS_FLOATS / 4];
  __shared__ double red[2 * WAVES];
  const GnBlock b = gn_part(hw, c, groups, cg, gps, pp);
  gn_stage(tile, b, ta, splits, slab, v_cb, out, c, out_ld);  // t, resident, and raw into the destination
  __syncthreads();
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  for (int it = 0; it < b.iters; ++it) {
    const int gl = b.team + it * b.nteams;
    const bool on = gl < b.ng;
    const int gq = on ? b.np * b.qpg : 0;
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
      double* o = gn_tab(tab, b, groups, gl) + 2 * blockIdx.x;
      o[0] = v[0];
      o[1] = v[1];
    }
  }
}

// (out: read and rewritten in place, each element by the lane that read it -- no __restrict__)
__global__ __launch_bounds__(BLOCK) void k_gn_split_act_tangent(
    float* out, unsigned out_ld, const double* __restrict__ tab, const float* __restrict__ a,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ v_gamma, const float* __restrict__ v_beta, const float* __restrict__ mask_src, int hw, int c,
    int groups, int cg, int gps, int pp) {
  __shared__ float sm1[GN_MAX_GPS], smx[GN_MAX_GPS];
  const GnBlock b = gn_part(hw, c, groups, cg, gps, pp);
  gn_parts_means(sm1, smx, tab, b, groups, (double)hw * (double)cg);
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  for (int q = threadIdx.x; q < b.nq; q += BLOCK) {
    const int p = q / b.sq, j = q - p * b.sq, gl = j / b.qpg;
    const float mu = stat_mu[gl], rs = stat_rs[gl], m1 = sm1[gl], mx = smx[gl];
    const long long row = b.row0 + p, gi = row * c + b.ch0 + 4 * j;
    float* dst = out + row * out_ld + b.ch0 + 4 * j;
    const F4 t = ld4(dst), x = ld4(a + gi), w = ld4s(gamma + b.ch0 + 4 * j);
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
    *reinterpret_cast<F4*>(dst) = r;
  }
}

__global__ __launch_bounds__(BLOCK) void k_gn_split_adjoint_sums(
    float* __restrict__ g_out, double* __restrict__ tab, float* __restrict__ gw_rows, float* __restrict__ gb_rows,
    const float* __restrict__ gy, int splits, long long slab, const float* __restrict__ a, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ mask_src, int hw, int c,
    int groups, int cg, int gps, int pp) {
  __shared__ F4 tile[GN_LDS_FLOATS / 4];
  __shared__ double red[2 * WAVES];
  __shared__ double rsum[BLOCK * 4];
  const GnBlock b = gn_part(hw, c, groups, cg, gps, pp);
  gn_stage_masked(tile, b, gy, splits, slab, mask_src, c);  // g, resident
  __syncthreads();
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  for (int it = 0; it < b.iters; ++it) {
    const int gl = b.team + it * b.nteams;
    const bool on = gl < b.ng;
    const int gq = on ? b.np * b.qpg : 0;
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
      double* o = gn_tab(tab, b, groups, gl) + 2 * blockIdx.x;
      o[0] = v[0];
      o[1] = v[1];
    }
  }
  // g leaves, and the part's rows of scale and shift: lane (slot, column) walks its channel quad down the part's pixels
  const int cols = b.sq < BLOCK ? b.sq : BLOCK, slots = BLOCK / cols;
  const int slot = threadIdx.x / cols, jl = threadIdx.x - slot * cols;
  for (int j0 = 0; j0 < b.sq; j0 += cols) {
    const int j = j0 + jl;
    const bool act = slot < slots && j < b.sq;
    F4 sb = {{0.f, 0.f, 0.f, 0.f}}, sw = {{0.f, 0.f, 0.f, 0.f}};
    if (act) {
      const int gl = j / b.qpg;
      const float mu = stat_mu[gl], rs = stat_rs[gl];
      for (int p = slot; p < b.np; p += slots) {
        const long long gi = b.base + (long long)p * c + 4 * j;
        const F4 g = tile[p * b.sq + j], x = ld4(a + gi);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float xh = (x.e[k] - mu) * rs;
          sb.e[k] += g.e[k];
          sw.e[k] += g.e[k] * xh;
        }
        *reinterpret_cast<F4*>(g_out + gi) = g;
      }
    }
    const long long at = ((long long)b.nb * gridDim.x + blockIdx.x) * c + b.ch0 + 4 * j;
    if (gw_rows) gn_row_store(gw_rows, sw, rsum, slots, cols, slot, jl, act, at);
    if (gb_rows) gn_row_store(gb_rows, sb, rsum, slots, cols, slot, jl, act, at);
  }
}

// (g may be ga_out itself: read and rewritten in place, each element by the lane that read it -- no __restrict__)
__global__ __launch_bounds__(BLOCK) void k_gn_split_act_adjoint(
    float* ga_out, float* __restrict__ gcb_rows, const float* g_in, const double* __restrict__ tab,
    const float* __restrict__ a, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, int hw, int c, int groups, int cg, int gps, int pp) {
  __shared__ double rsum[BLOCK * 4];
  __shared__ float sm1[GN_MAX_GPS], smx[GN_MAX_GPS];
  const GnBlock b = gn_part(hw, c, groups, cg, gps, pp);
  gn_parts_means(sm1, smx, tab, b, groups, (double)hw * (double)cg);
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  const int cols = b.sq < BLOCK ? b.sq : BLOCK, slots = BLOCK / cols;
  const int slot = threadIdx.x / cols, jl = threadIdx.x - slot * cols;
  for (int j0 = 0; j0 < b.sq; j0 += cols) {
    const int j = j0 + jl;
    const bool act = slot < slots && j < b.sq;
    F4 sc = {{0.f, 0.f, 0.f, 0.f}};
    if (act) {
      const int gl = j / b.qpg;
      const float mu = stat_mu[gl], rs = stat_rs[gl], m1 = sm1[gl], mx = smx[gl];
      const F4 w = ld4s(gamma + b.ch0 + 4 * j);
      for (int p = slot; p < b.np; p += slots) {
        const long long gi = b.base + (long long)p * c + 4 * j;
        const F4 g = ld4(g_in + gi), x = ld4(a + gi);
        F4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float xh = (x.e[k] - mu) * rs, pg = w.e[k] * g.e[k];
          o.e[k] = rs * ((pg - m1) - xh * mx);
          sc.e[k] += o.e[k];
        }
        *reinterpret_cast<F4*>(ga_out + gi) = o;
      }
    }
    const long long at = ((long long)b.nb * gridDim.x + blockIdx.x) * c + b.ch0 + 4 * j;
    if (gcb_rows) gn_row_store(gcb_rows, sc, rsum, slots, cols, slot, jl, act, at);
  }
}

// ---- the tangent of the split adjoint (a Hessian product's second sweep through a split unit) ---------------------------
// the five partial sums per (sample, group, part): of p, p * xh, p', p' * xh and p * tau
enum { S2_P1, S2_PX, S2_Q1, S2_QX, S2_PT, S2_K };

// FLOATS: the floats of ONE resident block (part_pixels * span <= FLOATS), as for k_gn_act_adjoint2
template <int FLOATS>
__global__ __launch_bounds__(BLOCK) void k_gn_split_adjoint2_sums(
    float* __restrict__ gp_out, float* __restrict__ t_out, double* __restrict__ tab, float* __restrict__ gw_rows,
    float* __restrict__ gb_rows, const float* __restrict__ gy2, int splits, long long slab, const float* __restrict__ ta,
    int t_splits, long long t_slab, const float* __restrict__ v_cb, const double* __restrict__ t_tab,
    const float* __restrict__ a, const float* __restrict__ g1, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ v_gamma,
    const float* __restrict__ mask_src, int hw, int c, int groups, int cg, int gps, int pp) {
  __shared__ F4 tg[FLOATS / 4];  // g' of the part
  __shared__ F4 tt[FLOATS / 4];  // t of the part
  __shared__ double red[S2_K * WAVES];
  __shared__ double rsum[BLOCK * 4];
  __shared__ float sT1[GN_MAX_GPS], sTx[GN_MAX_GPS];
  const GnBlock b = gn_part(hw, c, groups, cg, gps, pp);
  gn_parts_means(sT1, sTx, t_tab, b, groups, (double)hw * (double)cg);  // T1, Tx: the tangent sweep's partials
  gn_stage_masked(tg, b, gy2, splits, slab, mask_src, c);
  gn_stage(tt, b, ta, t_splits, t_slab, v_cb, t_out, c, c);  // t, resident, and out for the apply launch
  __syncthreads();
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  const bool has_vg = v_gamma != nullptr;
  const F4 zero = {{0.f, 0.f, 0.f, 0.f}};
  for (int it = 0; it < b.iters; ++it) {
    const int gl = b.team + it * b.nteams;
    const bool on = gl < b.ng;
    const int gq = on ? b.np * b.qpg : 0;
    const float mu = on ? stat_mu[gl] : 0.f, rs = on ? stat_rs[gl] : 0.f;
    const float T1 = on ? sT1[gl] : 0.f, Tx = on ? sTx[gl] : 0.f;
    F4 s[S2_K] = {zero, zero, zero, zero, zero};
    for (int e = b.lt; e < gq; e += b.T) {
      const int p = e / b.qpg, jj = e - p * b.qpg, j = gl * b.qpg + jj;
      const long long gi = b.base + (long long)p * c + 4 * j;
      const F4 gp = tg[p * b.sq + j], t = tt[p * b.sq + j], x = ld4(a + gi), g = ld4(g1 + gi);
      const F4 w = ld4s(gamma + b.ch0 + 4 * j), vg = has_vg ? ld4s(v_gamma + b.ch0 + 4 * j) : zero;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const Gn2Point o = gn2_point(x.e[k], g.e[k], gp.e[k], w.e[k], vg.e[k], has_vg, mu, rs);
        const float tau = (t.e[k] - T1) - o.xh * Tx;
        s[S2_P1].e[k] += o.p;
        s[S2_PX].e[k] += o.p * o.xh;
        s[S2_Q1].e[k] += o.pp;
        s[S2_QX].e[k] += o.pp * o.xh;
        s[S2_PT].e[k] += o.p * tau;
      }
    }
    double v[S2_K];
#pragma unroll
    for (int i = 0; i < S2_K; ++i) v[i] = quad_sum(s[i]);
    gn_team_sum<S2_K>(v, red, b);
    if (on && b.lt == 0) {
      double* o = gn_tab(tab, b, groups, gl, S2_K) + S2_K * blockIdx.x;
#pragma unroll
      for (int i = 0; i < S2_K; ++i) o[i] = v[i];
    }
  }
  // g' leaves, and the part's rows of scale and shift: lane (slot, column) walks its channel quad down the part's pixels
  const int cols = b.sq < BLOCK ? b.sq : BLOCK, slots = BLOCK / cols;
  const int slot = threadIdx.x / cols, jl = threadIdx.x - slot * cols;
  for (int j0 = 0; j0 < b.sq; j0 += cols) {
    const int j = j0 + jl;
    const bool act = slot < slots && j < b.sq;
    F4 sb = zero, sw = zero;
    if (act) {
      const int gl = j / b.qpg;
      const float mu = stat_mu[gl], rs = stat_rs[gl], T1 = sT1[gl], Tx = sTx[gl];
      for (int p = slot; p < b.np; p += slots) {
        const long long gi = b.base + (long long)p * c + 4 * j;
        const F4 gp = tg[p * b.sq + j], t = tt[p * b.sq + j], x = ld4(a + gi), g = ld4(g1 + gi);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float xh = (x.e[k] - mu) * rs, rt = rs * ((t.e[k] - T1) - xh * Tx);
          sb.e[k] += gp.e[k];
          sw.e[k] += gp.e[k] * xh + g.e[k] * rt;
        }
        *reinterpret_cast<F4*>(gp_out + gi) = gp;
      }
    }
    const long long at = ((long long)b.nb * gridDim.x + blockIdx.x) * c + b.ch0 + 4 * j;
    if (gw_rows) gn_row_store(gw_rows, sw, rsum, slots, cols, slot, jl, act, at);
    if (gb_rows) gn_row_store(gb_rows, sb, rsum, slots, cols, slot, jl, act, at);
  }
}

// (gp may be ga2_out itself: read and rewritten in place, each element by the lane that read it -- no __restrict__)
__global__ __launch_bounds__(BLOCK) void k_gn_split_act_adjoint2(
    float* ga2_out, float* __restrict__ gcb_rows, const float* gp_in, const float* __restrict__ t_map,
    const double* __restrict__ tab, const double* __restrict__ t_tab, const float* __restrict__ a,
    const float* __restrict__ g1, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ v_gamma, int hw, int c, int groups, int cg, int gps, int pp) {
  __shared__ double rsum[BLOCK * 4];
  __shared__ float stats[G2_STATS][GN_MAX_GPS];
  const GnBlock b = gn_part(hw, c, groups, cg, gps, pp);
  const float* stat_mu = mean + (long long)b.nb * groups + b.g0;
  const float* stat_rs = rstd + (long long)b.nb * groups + b.g0;
  if ((int)threadIdx.x < b.ng) {  // the group's seven numbers from the parts' partials, part order, fp64
    const double* q = gn_tab(tab, b, groups, threadIdx.x, S2_K);
    const double* tq = gn_tab(t_tab, b, groups, threadIdx.x);
    const double cnt = (double)hw * (double)cg;
    double v[S2_K] = {0.0, 0.0, 0.0, 0.0, 0.0}, t1 = 0.0, tx = 0.0;
    for (int i = 0; i < (int)gridDim.x; ++i) {
#pragma unroll
      for (int k = 0; k < S2_K; ++k) v[k] += q[S2_K * i + k];
      t1 += tq[2 * i];
      tx += tq[2 * i + 1];
    }
    const float rs = stat_rs[threadIdx.x], Tx = (float)(tx / cnt), Qt = rs * (float)(v[S2_PT] / cnt);
    stats[G2_T1][threadIdx.x] = (float)(t1 / cnt);
    stats[G2_TX][threadIdx.x] = Tx;
    stats[G2_P1][threadIdx.x] = (float)(v[S2_P1] / cnt);
    stats[G2_PX][threadIdx.x] = (float)(v[S2_PX] / cnt);
    stats[G2_Q1][threadIdx.x] = (float)(v[S2_Q1] / cnt);
    stats[G2_QS][threadIdx.x] = (float)(v[S2_QX] / cnt) + Qt;
    stats[G2_RT][threadIdx.x] = rs * Tx;
  }
  __syncthreads();
  const bool has_vg = v_gamma != nullptr;
  const F4 zero = {{0.f, 0.f, 0.f, 0.f}};
  const int cols = b.sq < BLOCK ? b.sq : BLOCK, slots = BLOCK / cols;
  const int slot = threadIdx.x / cols, jl = threadIdx.x - slot * cols;
  for (int j0 = 0; j0 < b.sq; j0 += cols) {
    const int j = j0 + jl;
    const bool act = slot < slots && j < b.sq;
    F4 sc = zero;
    if (act) {
      const int gl = j / b.qpg;
      const float mu = stat_mu[gl], rs = stat_rs[gl];
      const float T1 = stats[G2_T1][gl], Tx = stats[G2_TX][gl], P1 = stats[G2_P1][gl], Px = stats[G2_PX][gl];
      const float Q1 = stats[G2_Q1][gl], Qs = stats[G2_QS][gl], rT = stats[G2_RT][gl];
      const F4 w = ld4s(gamma + b.ch0 + 4 * j), vg = has_vg ? ld4s(v_gamma + b.ch0 + 4 * j) : zero;
      for (int p = slot; p < b.np; p += slots) {
        const long long gi = b.base + (long long)p * c + 4 * j;
        const F4 gp = ld4(gp_in + gi), t = ld4(t_map + gi), x = ld4(a + gi), g = ld4(g1 + gi);
        F4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const Gn2Point e = gn2_point(x.e[k], g.e[k], gp.e[k], w.e[k], vg.e[k], has_vg, mu, rs);
          float rt;
          o.e[k] = gn2_ga2(e, t.e[k], rs, T1, Tx, P1, Px, Q1, Qs, rT, rt);
          sc.e[k] += o.e[k];
        }
        *reinterpret_cast<F4*>(ga2_out + gi) = o;
      }
    }
    const long long at = ((long long)b.nb * gridDim.x + blockIdx.x) * c + b.ch0 + 4 * j;
    if (gcb_rows) gn_row_store(gcb_rows, sc, rsum, slots, cols, slot, jl, act, at);
  }
}

// out[c] = sum_n (pre * row[n][c])^2, row[n] = the sample's `parts` partial rows added in part order (fp64, one rounding)
__global__ __launch_bounds__(BLOCK) void k_gn_split_rows_sqsum(GnSqTables tabs, float pre, int n, int parts, int c) {
  float* out = tabs.out[blockIdx.y];
  const float* rows = tabs.rows[blockIdx.y];
  const int ch = blockIdx.x * BLOCK + threadIdx.x;
  if (!out || ch >= c) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    double r = 0.0;
    for (int pt = 0; pt < parts; ++pt) r += (double)rows[((long long)i * parts + pt) * c + ch];
    const float t = pre * (float)r;
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

// ---- the split family's entry points ------------------------------------------------------------------------------------
namespace {

// what every launching entry point of the family checks first: the plan, and the fp64 partials table
inline int gn_split_ok(GnSplitPlan& s, const void* partials, int64_t n, int64_t hw, int64_t c, int64_t groups, int dtype) {
  if (dtype != HF_F32 || gn_split_plan(s, n, hw, c, groups) != HF_OK) return HF_ERR_ARG;
  return partials && ((uintptr_t)partials & 7) == 0 ? HF_OK : HF_ERR_ARG;
}

inline dim3 gn_split_grid(const GnSplitPlan& s) { return dim3(s.parts, s.g.spans, s.g.n); }

}  // namespace

int hf_gn_split_plan(int64_t n, int64_t hw, int64_t c, int64_t groups, int* span, int* parts, int* part_pixels) {
  GnSplitPlan s;
  if (!span || !parts || !part_pixels || gn_split_plan(s, n, hw, c, groups) != HF_OK) return HF_ERR_ARG;
  *span = s.g.gps * s.g.cg;
  *parts = s.parts;
  *part_pixels = s.pp;
  return HF_OK;
}

int hf_gn_split_stats(void* a_out, void* partials, const void* a, int splits, int64_t slab_stride, const void* conv_bias,
                      int64_t n, int64_t hw, int64_t c, int64_t groups, int dtype, void* stream) {
  GnSplitPlan s;
  if (gn_split_ok(s, partials, n, hw, c, groups, dtype) != HF_OK) return HF_ERR_ARG;
  if (gn_slabs_ok(a, splits, slab_stride, s.g) != HF_OK) return HF_ERR_ARG;
  const void* al[] = {a_out, a};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_split_stats, gn_split_grid(s), dim3(BLOCK), 0, (hipStream_t)stream, (float*)a_out,
                     (double*)partials, (const float*)a, splits, (long long)slab_stride, (const float*)conv_bias, s.g.hw,
                     s.g.c, s.g.groups, s.g.cg, s.g.gps, s.pp);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_split_forward(void* y, void* y2, int64_t y2_ld, void* mean, void* rstd, const void* s_map, const void* partials,
                        const void* gamma, const void* beta, double eps, int relu, int64_t n, int64_t hw, int64_t c,
                        int64_t groups, int dtype, void* stream) {
  GnSplitPlan s;
  if (gn_split_ok(s, partials, n, hw, c, groups, dtype) != HF_OK) return HF_ERR_ARG;
  if ((!y && !y2) || !mean || !rstd || !s_map || !gamma || !(eps >= 0.0) || !(eps - eps == 0.0)) return HF_ERR_ARG;
  if (y2 && (y2_ld == 0 || !gn_ld_ok(y2_ld, s.g))) return HF_ERR_ARG;
  const void* al[] = {y, y2, s_map};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_split_forward, gn_split_grid(s), dim3(BLOCK), 0, (hipStream_t)stream, (float*)y, (float*)y2,
                     (unsigned)y2_ld, (float*)mean, (float*)rstd, (const float*)s_map, (const double*)partials,
                     (const float*)gamma, (const float*)beta, (float)eps, relu, s.g.hw, s.g.c, s.g.groups, s.g.cg, s.g.gps,
                     s.pp);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_split_tangent_sums(void* out, int64_t out_ld, void* partials, const void* t_a, int splits, int64_t slab_stride,
                             const void* v_conv_bias, const void* a, const void* mean, const void* rstd, int64_t n,
                             int64_t hw, int64_t c, int64_t groups, int dtype, void* stream) {
  GnSplitPlan s;
  if (gn_split_ok(s, partials, n, hw, c, groups, dtype) != HF_OK) return HF_ERR_ARG;
  if (!out || !a || !mean || !rstd || !gn_ld_ok(out_ld, s.g)) return HF_ERR_ARG;
  if (gn_slabs_ok(t_a, splits, slab_stride, s.g) != HF_OK) return HF_ERR_ARG;
  const void* al[] = {out, t_a, a};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_split_tangent_sums, gn_split_grid(s), dim3(BLOCK), 0, (hipStream_t)stream, (float*)out,
                     (unsigned)(out_ld ? out_ld : c), (double*)partials, (const float*)t_a, splits, (long long)slab_stride,
                     (const float*)v_conv_bias, (const float*)a, (const float*)mean, (const float*)rstd, s.g.hw, s.g.c,
                     s.g.groups, s.g.cg, s.g.gps, s.pp);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_split_act_tangent(void* out, int64_t out_ld, const void* partials, const void* a, const void* mean,
                            const void* rstd, const void* gamma, const void* v_gamma, const void* v_beta,
                            const void* mask_src, int64_t n, int64_t hw, int64_t c, int64_t groups, int dtype,
                            void* stream) {
  GnSplitPlan s;
  if (gn_split_ok(s, partials, n, hw, c, groups, dtype) != HF_OK) return HF_ERR_ARG;
  if (!out || !a || !mean || !rstd || !gamma || !gn_ld_ok(out_ld, s.g)) return HF_ERR_ARG;
  const void* al[] = {out, a, mask_src};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_split_act_tangent, gn_split_grid(s), dim3(BLOCK), 0, (hipStream_t)stream, (float*)out,
                     (unsigned)(out_ld ? out_ld : c), (const double*)partials, (const float*)a, (const float*)mean,
                     (const float*)rstd, (const float*)gamma, (const float*)v_gamma, (const float*)v_beta,
                     (const float*)mask_src, s.g.hw, s.g.c, s.g.groups, s.g.cg, s.g.gps, s.pp);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_split_adjoint_sums(void* g, void* partials, void* gw_rows, void* gb_rows, const void* gy, int splits,
                             int64_t slab_stride, const void* a, const void* mean, const void* rstd, const void* gamma,
                             const void* mask_src, int64_t n, int64_t hw, int64_t c, int64_t groups, int dtype,
                             void* stream) {
  GnSplitPlan s;
  if (gn_split_ok(s, partials, n, hw, c, groups, dtype) != HF_OK) return HF_ERR_ARG;
  if (!g || !a || !mean || !rstd || !gamma || (int64_t)s.g.n * s.parts * s.g.c > 0x7fffffffLL) return HF_ERR_ARG;
  if (gn_slabs_ok(gy, splits, slab_stride, s.g) != HF_OK) return HF_ERR_ARG;
  const void* al[] = {g, gw_rows, gb_rows, gy, a, mask_src};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_split_adjoint_sums, gn_split_grid(s), dim3(BLOCK), 0, (hipStream_t)stream, (float*)g,
                     (double*)partials, (float*)gw_rows, (float*)gb_rows, (const float*)gy, splits, (long long)slab_stride,
                     (const float*)a, (const float*)mean, (const float*)rstd, (const float*)gamma, (const float*)mask_src,
                     s.g.hw, s.g.c, s.g.groups, s.g.cg, s.g.gps, s.pp);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_split_act_adjoint(void* ga, void* gcb_rows, const void* g, const void* partials, const void* a, const void* mean,
                            const void* rstd, const void* gamma, int64_t n, int64_t hw, int64_t c, int64_t groups,
                            int dtype, void* stream) {
  GnSplitPlan s;
  if (gn_split_ok(s, partials, n, hw, c, groups, dtype) != HF_OK) return HF_ERR_ARG;
  if (!ga || !g || !a || !mean || !rstd || !gamma || (int64_t)s.g.n * s.parts * s.g.c > 0x7fffffffLL) return HF_ERR_ARG;
  const void* al[] = {ga, gcb_rows, g, a};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_split_act_adjoint, gn_split_grid(s), dim3(BLOCK), 0, (hipStream_t)stream, (float*)ga,
                     (float*)gcb_rows, (const float*)g, (const double*)partials, (const float*)a, (const float*)mean,
                     (const float*)rstd, (const float*)gamma, s.g.hw, s.g.c, s.g.groups, s.g.cg, s.g.gps, s.pp);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_split_adjoint2_sums(void* gp, void* t, void* partials, void* gw_rows, void* gb_rows, const void* gy2, int splits,
                              int64_t slab_stride, const void* t_a, int t_splits, int64_t t_slab_stride,
                              const void* v_conv_bias, const void* t_partials, const void* a, const void* g, const void* mean,
                              const void* rstd, const void* gamma, const void* v_gamma, const void* mask_src, int64_t n,
                              int64_t hw, int64_t c, int64_t groups, int dtype, void* stream) {
  GnSplitPlan s;
  if (gn_split_ok(s, partials, n, hw, c, groups, dtype) != HF_OK) return HF_ERR_ARG;
  if (!t_partials || ((uintptr_t)t_partials & 7) || t_partials == partials) return HF_ERR_ARG;
  if (!gp || !t || gp == t || !a || !g || !mean || !rstd || !gamma || (int64_t)s.g.n * s.parts * s.g.c > 0x7fffffffLL)
    return HF_ERR_ARG;
  if (gn_slabs_ok(gy2, splits, slab_stride, s.g) != HF_OK || gn_slabs_ok(t_a, t_splits, t_slab_stride, s.g) != HF_OK)
    return HF_ERR_ARG;
  const void* al[] = {gp, t, gw_rows, gb_rows, gy2, t_a, a, g, mask_src};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  // two resident blocks, static LDS sized to the plan's part (as hf_gn_act_adjoint2; a part keeps at least 4 096 floats
  // wherever the plan could choose, so the smallest size there has no use here)
  auto kernel = s.pp * s.g.gps * s.g.cg <= GN_LDS_FLOATS / 2 ? k_gn_split_adjoint2_sums<GN_LDS_FLOATS / 2>
                                                             : k_gn_split_adjoint2_sums<GN_LDS_FLOATS>;
  hipLaunchKernelGGL(kernel, gn_split_grid(s), dim3(BLOCK), 0, (hipStream_t)stream, (float*)gp, (float*)t,
                     (double*)partials, (float*)gw_rows, (float*)gb_rows, (const float*)gy2, splits, (long long)slab_stride,
                     (const float*)t_a, t_splits, (long long)t_slab_stride, (const float*)v_conv_bias,
                     (const double*)t_partials, (const float*)a, (const float*)g, (const float*)mean, (const float*)rstd,
                     (const float*)gamma, (const float*)v_gamma, (const float*)mask_src, s.g.hw, s.g.c, s.g.groups, s.g.cg,
                     s.g.gps, s.pp);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_split_act_adjoint2(void* ga2, void* gcb_rows, const void* gp, const void* t, const void* partials,
                             const void* t_partials, const void* a, const void* g, const void* mean, const void* rstd,
                             const void* gamma, const void* v_gamma, int64_t n, int64_t hw, int64_t c, int64_t groups,
                             int dtype, void* stream) {
  GnSplitPlan s;
  if (gn_split_ok(s, partials, n, hw, c, groups, dtype) != HF_OK) return HF_ERR_ARG;
  if (!t_partials || ((uintptr_t)t_partials & 7)) return HF_ERR_ARG;
  if (!ga2 || !gp || !t || t == ga2 || !a || !g || !mean || !rstd || !gamma ||
      (int64_t)s.g.n * s.parts * s.g.c > 0x7fffffffLL)
    return HF_ERR_ARG;
  const void* al[] = {ga2, gcb_rows, gp, t, a, g};
  if (gn_aligned(al) != HF_OK) return HF_ERR_ARG;
  hipLaunchKernelGGL(k_gn_split_act_adjoint2, gn_split_grid(s), dim3(BLOCK), 0, (hipStream_t)stream, (float*)ga2,
                     (float*)gcb_rows, (const float*)gp, (const float*)t, (const double*)partials,
                     (const double*)t_partials, (const float*)a, (const float*)g, (const float*)mean, (const float*)rstd,
                     (const float*)gamma, (const float*)v_gamma, s.g.hw, s.g.c, s.g.groups, s.g.cg, s.g.gps, s.pp);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_gn_split_rows_sqsum(void* out_w, const void* rows_w, void* out_b, const void* rows_b, void* out_cb,
                           const void* rows_cb, double pre, int64_t n, int64_t parts, int64_t c, int dtype, void* stream) {
  if (dtype != HF_F32 || n <= 0 || parts <= 0 || c <= 0 || n * parts * c > 0x7fffffffLL || !(pre - pre == 0.0))
    return HF_ERR_ARG;
  if ((!out_w && !out_b && !out_cb) || (out_w && !rows_w) || (out_b && !rows_b) || (out_cb && !rows_cb)) return HF_ERR_ARG;
  GnSqTables tabs = {{(float*)out_w, (float*)out_b, (float*)out_cb},
                     {(const float*)rows_w, (const float*)rows_b, (const float*)rows_cb}};
  hipLaunchKernelGGL(k_gn_split_rows_sqsum, dim3((unsigned)((c + BLOCK - 1) / BLOCK), 3), dim3(BLOCK), 0,
                     (hipStream_t)stream, tabs, (float)pre, (int)n, (int)parts, (int)c);
  HF_HIP(hipGetLastError());
  return HF_OK;
}
