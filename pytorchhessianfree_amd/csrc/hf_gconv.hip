// hf_gconv.hip -- grouped convolutions (Conv2d(c_in -> c_out, groups = G), group widths cg_in = c_in / G and cg_out =
// c_out / G both multiples of 4 and <= 64) of the plain-stack engine (engine/plain.py): the tangent / forward map, and the
// data + weight gradient of one cotangent in ONE launch; the two-term form of the latter (a Hessian product's second-order
// backward) and the squared per-sample weight gradient summed over the batch (diag_ef), one launch each.  fp32, wave64,
// NHWC, r*s <= 49 taps, per-axis stride and padding, dilation 1, zero padding.  No atomics; every output is summed in one
// fixed order (below), so two launches on the same operands agree bitwise.
//
// Why a design of its own.  A grouped layer's reduction is r*s*cg_in long and block-diagonal over the channels.  The 64x64
// MFMA tiles of hf_conv.hip would be 1/16 .. 1/4 full per group and need one launch per group; the depthwise kernels have no
// reduction over channels.  v_mfma_f32_4x4x1_16b_f32 is sixteen independent 4x4 outer products per issue: one issue is
// 4 pixels x 64 consecutive output channels whatever the group width, block b owning the channel quad 4b .. 4b+3 and
// reading the input channels of THAT quad's group.  Both widths are multiples of 4, so a quad never straddles a group; a
// group may straddle a 64-channel span (cg_out = 12).  No multiply is wasted but in a partial last span.
// Lane maps of the instruction (block = lane / 4):  A: lane -> (block, row i = lane % 4);  B: lane -> (block, column
// j = lane % 4);  D: register i, lane j + 4 * block.  One k per issue: every accumulator is a chain of single products.
//
// Work split, tangent and data gradient.  A workgroup (4 waves) owns (sample, tile of th x 8 OUTPUT pixels (tangent) or
// INPUT pixels (data gradient), span of 64 channels of that map).  A pixel quad is 4 consecutive pixels of a tile row; a
// wave owns th/2 quads (th = 8: 4 quads = 16 accumulator registers), so one B word (a weight) is reused th/2 times and an
// issue costs one A word (an activation) per lane from LDS; the blocks of one group read the same A address (a broadcast).
// The reduction runs in chunks of ck channels per group (ck % 4 == 0): per chunk the workgroup stages ONCE
//   the tile of its span's groups, [(th-1)*stride_h + r] x [7*stride_w + s] pixels x (groups of the span) x ck channels,
//     padding and everything outside the map as zeros in LDS (no tap predicates a global load), pixel pitch
//     ng*ck + 1 words (odd: the four pixels of a quad fall into different banks);
//   the span's weights of the chunk: per output channel ONE contiguous run of ck*r*s floats of the parameter, read
//     coalesced, kept as [k = (channel of the chunk, tap)][64 channels of the span] at a pitch of 65 words, which is the
//     order the B lanes read them (one conflict-free row per k) and lets the transposing stores spread over the banks.
// The data gradient is the same loop with the widths' roles swapped: spans of 64 INPUT channels, the reduction over
// (output channel of the group, tap), the weight gathered transposed within the group; the cotangent tile is
// [(th + r - 2) / stride_h + 1] x [(8 + s - 2) / stride_w + 1] pixels.  A tap whose division by the stride is not exact is
// skipped where that is uniform for the quad (rows) and fed as a zero where it is per lane (columns); a cotangent pixel
// outside the map is a zero in LDS.
// Design points changed from the first sketch: (1) the two-term tangent runs its terms one after the other (all of
// t_x * W, then all of x * V) through ONE staging area instead of feeding both products of a k from two: it halves the
// LDS and is what lets th = 8 stand at stride 1 for every width; (2) the tile height th (8, 4 or 2) shrinks before the plan
// refuses a geometry -- with 16 groups per span (width 4) a stride-2 halo of 17 x 17 pixels x 64 channels is 75 KB;
// (3) the weight gradient needs no cross-wave reduction (below).
//
// Weight gradient.  gw[co][ci][tap] = sum_p ga[p][co] * x[pix(p, tap)][g*cg_in + ci]: the reduction index is the pixel,
// a block owns the 4x4 patch (output-channel quad) x (input-channel quad) of one tap.  A workgroup owns (run of units,
// span of 64 output channels, pass); a pass is a chunk of ck <= cg_in input channels per group with r*s*ck/4 <= 64 SLOTS
// (tap, input-channel quad); wave w owns the slots w, w+4, ...: at most 16 accumulators = 64 registers, kept over the
// whole run.  Per pixel a lane reads ONE A word (ga[p][ch0 + lane], the same for every slot) and one B word per issue.
// Every (channel, channel, tap) entry has exactly one owner lane: no shuffles, no LDS reduction.  The (sample, output
// tile) units in ascending order are cut into splits_w consecutive runs of `per` units (the last may be shorter); run s
// leaves slab s, [c_out*cg_in*r*s] in PARAMETER order, and hf_pack_ex adds the slabs in split order.
//
// LDS (<= 64 KB; words of 4 bytes; P = groups per span * ck + 1) and accumulator registers per wave:
//   tangent          halo * P + ck*r*s * 65          data gradient   cot * P + ck*r*s * 65        both: 4 * th/2 registers
//   weight gradient  halo * P + th*8 * 65                                                         4 * min(16, slots/4)
//   3x3, stride 1, widths 4 -> 4, >= 16 groups:  ck = 4, th = 8: 100*65 + 36*65 = 8 840 words = 35.4 KB (tangent and data
//     gradient), 100*65 + 64*65 = 42.6 KB with 9 slots = 12 registers (weight gradient); 16 accumulator registers.
//   the same at stride 2: the 17x17 halo needs th = 4 (9*17*65 + 36*65 = 49.1 KB), 8 registers.
//   3x3, stride 1, widths 16 -> 16: 4 groups per span, ck = 16: 100*65 + 144*65 = 63.4 KB; weight gradient 36 slots = 36
//     registers.   widths 64 -> 64: one group per span, ck = 20 (four chunks): 100*21 + 180*65 = 55.2 KB; the weight
//     gradient takes ck = 28 (63 slots, 64 registers; 100*29 + 64*65 = 28.2 KB) in 3 passes.
//
// Addition orders (each accumulator starts at zero and takes one product per issue).
//   tangent:        first the term t_x * W, then x * V; per term the chunks of input channels ascending, inside a chunk
//                   the channel ascending, inside a channel the taps ascending (i, j).
//   data gradient:  chunks of the group's output channels ascending, channel ascending, taps ascending (i, j); the
//                   skipped row taps add nothing, the zero-fed column taps and out-of-map pixels add an exact zero.
//   weight gradient: units of the run ascending, inside a unit the tile's pixels in row-major order (pixels outside
//                   the map: an exact zero); hf_pack_ex then adds the slabs in split order.
//
// The two-term backward (hf_gconv2d_nhwc_backward2_slabs): dx = D(g', W) + D(g, V), slabs = W(x, g') + W(t_x, g), the
// tangent of the backward sweep in ONE launch -- the same device functions under a template flag (TWO), by design point
// (1): the terms one after the other through ONE staging area.  A data-gradient block runs its chunk loop over (g', W),
// then over (g, V), through the same cotangent tile and weight table into the same acc[]; a weight-gradient block stages
// per unit the x halo and the g' tile, runs the pixel loop, and behind a barrier stages the t_x halo and the g tile and
// runs it again, the slot accumulators kept over both and over the run.  LDS words and accumulator registers are
// therefore the one-term launch's: the same gc_plan, the same split count, the same grid.
//   data gradient:  all of g' * W (co ascending, per co the taps ascending (i, j)), then all of g * V in that order.
//   weight gradient: per unit the pixels of (g', x) in row-major order, then those of (g, t_x); units ascending.
//
// The squared sum (hf_gconv2d_nhwc_sqsum_slabs): out[co][ci][tap] = sum_m (pre * gw_m[co][ci][tap])^2 over the per-sample
// weight gradients gw_m.  It is the weight-gradient loop (flag SQ) with a sample boundary in it: a workgroup owns (split of
// the SAMPLES, pass, span of 64 output channels), runs a sample's output tiles in ascending order into the slot
// accumulators, and at the sample's last tile every lane folds the entries it owns, in registers:  t = acc * pre (one
// rounding), sq += t * t (two roundings), acc = 0; samples ascending; sq goes to the split's slab in parameter order, every
// entry of it.  One owner lane per entry: no shuffle, no LDS, no per-sample gradient in memory.  The samples are cut into
// min(n, 64, ceil(target / (spans * passes))) runs of ceil(n / runs) samples, none empty.  The running sums double the
// accumulator registers (16 slots per wave: 64 + 64); the slot cap stays 16 -- the compiler's figures show no scratch.
//
// Resource usage (gfx950, -O3, the compiler's remarks; LDS is dynamic, the weight gradient's words above -- 3x3 stride 1:
// width 4 42.6 KB, width 16 42.6 KB (100*65 + 64*65), width 64 28.2 KB -- for the two-term form and the squared sum alike):
//                                                            VGPRs   AGPRs   scratch
//   k_gc_tangent   (every form)                             50-52       4         0
//   k_gc_backward  (one term and TWO: the same figures)        92      64         0
//   k_gc_sqsum                                                176      64         0     (2 waves per SIMD)
#include "hf_common.h"

namespace {

typedef float gc_v4 __attribute__((ext_vector_type(4)));

constexpr int GC_TW = 8;                    // tile width, pixels (two pixel quads)
constexpr int GC_SPAN = 64;                 // channels per issue: 16 blocks x 4
constexpr int GC_WP = GC_SPAN + 1;          // LDS pitch of a row of 64 channels
constexpr int GC_MAX_TAPS = 49;
constexpr int GC_MAX_STRIDE = 8;
constexpr int GC_MAX_WIDTH = 64;            // channels per group
constexpr int GC_LDS_WORDS = 16 * 1024;     // 64 KB
constexpr int GC_QW = 4;                    // most pixel quads per wave (th = 8)
constexpr int GC_WSLOTS = 16;               // most weight-gradient slots per wave
constexpr int GC_TARGET_BLOCKS = 512;       // weight-gradient workgroups the plan aims at (2 per CU)
constexpr int GC_MAX_SPLITS = 64;
constexpr bool GC_WT = HF_WT_CONV != 0;

// ---- the plan: ONE definition, run by hf_gconv2d_nhwc_plan and by every launching entry point ------------------------
struct GcDir {
  int th, ck, pitch;     // tile rows; channels per group and chunk; LDS words per staged pixel
  int tiles_y, sh_, sw_; // tiles along the rows; staged pixels per tile (rows, columns)
};
struct GcPlan {
  int n, h, w, ci, co, groups, cgi, cgo, r, s, sh, sw, ph, pw, oh, ow;
  int tiles_x, dtiles_x, ospans, ispans;
  GcDir t, d, g;                 // tangent, data gradient, weight gradient
  int passes, units, per, splits_w;
};

// the most groups a span of 64 channels of a map with c channels in groups of cg touches
inline int gc_span_groups(int c, int cg) {
  int most = 0;
  for (int c0 = 0; c0 < c; c0 += GC_SPAN) {
    const int c1 = c0 + GC_SPAN < c ? c0 + GC_SPAN : c;
    const int ng = (c1 - 1) / cg - c0 / cg + 1;
    if (ng > most) most = ng;
  }
  return most;
}

inline int64_t gc_lds_words(const GcDir& d, int table_rows) {
  return (int64_t)d.sh_ * d.sw_ * d.pitch + (int64_t)table_rows * GC_WP;
}

// The largest tile height, then the largest chunk, whose LDS fits.  dir: 0 tangent, 1 data gradient, 2 weight gradient.
inline bool gc_fit(const GcPlan& p, int dir, GcDir* d) {
  const int rs = p.r * p.s;
  const int ng = dir == 1 ? gc_span_groups(p.ci, p.cgi) : gc_span_groups(p.co, p.cgo);
  int ck_max = dir == 1 ? p.cgo : p.cgi;
  if (dir == 2 && ck_max > (GC_WSLOTS * WAVES / rs) * 4) ck_max = (GC_WSLOTS * WAVES / rs) * 4;  // (rs <= 49: >= 4)
  for (int th = 8; th >= 2; th /= 2) {
    d->th = th;
    if (dir == 1) d->sh_ = (th + p.r - 2) / p.sh + 1, d->sw_ = (GC_TW + p.s - 2) / p.sw + 1;
    else d->sh_ = (th - 1) * p.sh + p.r, d->sw_ = (GC_TW - 1) * p.sw + p.s;
    for (int ck = ck_max; ck >= 4; ck -= 4) {
      d->ck = ck, d->pitch = ng * ck + 1;
      if (gc_lds_words(*d, dir == 2 ? th * GC_TW : ck * rs) <= GC_LDS_WORDS) return true;
    }
  }
  return false;
}

inline int gc_plan(int64_t n, int64_t h, int64_t w, int64_t ci, int64_t co, int64_t groups, int64_t r, int64_t s,
                   int64_t sh, int64_t sw, int64_t ph, int64_t pw, GcPlan* p) {
  if (n < 1 || h < 1 || w < 1 || groups < 1 || ci < 4 || co < 4 || r < 1 || s < 1 || r * s > GC_MAX_TAPS) return HF_ERR_ARG;
  const int64_t cgi = ci / groups, cgo = co / groups;
  if (cgi * groups != ci || cgo * groups != co) return HF_ERR_ARG;
  if (cgi < 4 || cgo < 4 || (cgi & 3) || (cgo & 3) || cgi > GC_MAX_WIDTH || cgo > GC_MAX_WIDTH) return HF_ERR_ARG;
  if (sh < 1 || sw < 1 || sh > GC_MAX_STRIDE || sw > GC_MAX_STRIDE || ph < 0 || pw < 0 || ph >= r || pw >= s)
    return HF_ERR_ARG;
  if (h + 2 * ph < r || w + 2 * pw < s) return HF_ERR_ARG;
  const int64_t oh = (h + 2 * ph - r) / sh + 1, ow = (w + 2 * pw - s) / sw + 1;
  // (2 * ci: the widest pixel pitch the engine reads an input at)
  if (n * h * w * 2 * ci >= (1LL << 31) || n * oh * ow * co >= (1LL << 31) || co * cgi * r * s >= (1LL << 31))
    return HF_ERR_ARG;
  p->n = (int)n, p->h = (int)h, p->w = (int)w, p->ci = (int)ci, p->co = (int)co, p->groups = (int)groups;
  p->cgi = (int)cgi, p->cgo = (int)cgo, p->r = (int)r, p->s = (int)s, p->sh = (int)sh, p->sw = (int)sw;
  p->ph = (int)ph, p->pw = (int)pw, p->oh = (int)oh, p->ow = (int)ow;
  p->tiles_x = (int)((ow + GC_TW - 1) / GC_TW), p->dtiles_x = (int)((w + GC_TW - 1) / GC_TW);
  p->ospans = (int)((co + GC_SPAN - 1) / GC_SPAN), p->ispans = (int)((ci + GC_SPAN - 1) / GC_SPAN);
  if (!gc_fit(*p, 0, &p->t) || !gc_fit(*p, 1, &p->d) || !gc_fit(*p, 2, &p->g)) return HF_ERR_ARG;
  p->t.tiles_y = (p->oh + p->t.th - 1) / p->t.th;
  p->d.tiles_y = (p->h + p->d.th - 1) / p->d.th;
  p->g.tiles_y = (p->oh + p->g.th - 1) / p->g.th;
  p->passes = (p->cgi + p->g.ck - 1) / p->g.ck;
  if (n * p->t.tiles_y * p->tiles_x * p->ospans >= (1LL << 30) || n * p->d.tiles_y * p->dtiles_x * p->ispans >= (1LL << 30))
    return HF_ERR_ARG;
  const int64_t units = n * p->g.tiles_y * p->tiles_x;
  if (units >= (1LL << 30)) return HF_ERR_ARG;
  const int64_t wg = (int64_t)p->ospans * p->passes;  // workgroups per run of units
  int64_t want = (GC_TARGET_BLOCKS + wg - 1) / wg;
  if (want > GC_MAX_SPLITS) want = GC_MAX_SPLITS;
  if (want > units) want = units;
  const int64_t per = (units + want - 1) / want;
  p->units = (int)units, p->per = (int)per, p->splits_w = (int)((units + per - 1) / per);  // (no empty split)
  return HF_OK;
}

inline bool quad_ok(const void* p, int64_t pitch) { return aligned16(p) && (pitch & 3) == 0; }

// ---- device helpers ------------------------------------------------------------------------------------------------
template <bool AL>
__device__ __forceinline__ F4 gc_ld_quad(const float* __restrict__ p) {
  if constexpr (AL) {
    return ld4(p);
  } else {
    F4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v.e[k] = p[k];
    return v;
  }
}

__device__ __forceinline__ int gc_floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

__device__ __forceinline__ gc_v4 gc_mfma(float a, float b, gc_v4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}

// Rows y0 .. y0+ny-1 x columns x0 .. x0+nx-1 of sample `img` of an NHWC map [., H, W, .] with pixel pitch ld: of each of
// the groups g0 .. g0+ng-1 (cg channels wide) the channels c0 .. c0+cke-1, into dst[(py*nx + px) * pitch + gl*ck + cl].
// A pixel outside the map is a zero in LDS and is not read.
template <bool AL>
__device__ __forceinline__ void gc_stage(float* dst, const float* __restrict__ src, int64_t ld, int img, int H, int W,
                                         int cg, int g0, int ng, int c0, int cke, int ck, int y0, int x0, int ny, int nx,
                                         int pitch) {
  const int qpg = cke >> 2, total = ny * nx * ng * qpg;
  for (int idx = threadIdx.x; idx < total; idx += BLOCK) {
    const int qd = idx % qpg, t = idx / qpg;
    const int gl = t % ng, p = t / ng;
    const int py = p / nx, px = p - py * nx;
    const int y = y0 + py, x = x0 + px;
    F4 v;
    v.e[0] = v.e[1] = v.e[2] = v.e[3] = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W)
      v = gc_ld_quad<AL>(src + ((int64_t)(img * H + y) * W + x) * ld + (g0 + gl) * cg + c0 + 4 * qd);
    float* to = dst + p * pitch + gl * ck + 4 * qd;
#pragma unroll
    for (int e = 0; e < 4; ++e) to[e] = v.e[e];
  }
}

extern __shared__ __align__(16) float gc_lds[];

// what a lane is inside its span of 64 channels of a map with c channels in groups of cg
struct GcLane {
  int lane, wave, blk, li;
  int c0, ce, g0, ng, gl;   // span: first channel, channels, first group, groups; the block's group (local)
};
__device__ __forceinline__ GcLane gc_lane(int span, int c, int cg) {
  GcLane l;
  l.lane = threadIdx.x & 63, l.wave = threadIdx.x >> 6, l.blk = l.lane >> 2, l.li = l.lane & 3;
  l.c0 = span * GC_SPAN, l.ce = min(GC_SPAN, c - l.c0);
  l.g0 = l.c0 / cg, l.ng = (l.c0 + l.ce - 1) / cg - l.g0 + 1;
  const int cq = l.c0 + 4 * l.blk;
  l.gl = cq < c ? cq / cg - l.g0 : 0;  // (a block past the last channel computes on group 0 and stores nothing)
  return l;
}

// ---- tangent / forward: one workgroup per (sample, th x 8 output tile, span of 64 output channels) --------------------
// MODE 0: t_x * W + x * V;  1: t_x * W (V == NULL);  2: x * V (t_x == NULL; the forward pass with V = W)
template <bool AL, int MODE>
__global__ void __launch_bounds__(BLOCK)
k_gc_tangent(float* __restrict__ out, const float* __restrict__ tx, const float* __restrict__ x, int64_t ld,
             const float* __restrict__ W, const float* __restrict__ V, const GcPlan g) {
  const GcDir d = g.t;
  const int rs = g.r * g.s, qw = d.th >> 1;
  int b = blockIdx.x;
  const int span = b % g.ospans;
  b /= g.ospans;
  const int tix = b % g.tiles_x;
  b /= g.tiles_x;
  const int tiy = b % d.tiles_y, img = b / d.tiles_y;
  const GcLane l = gc_lane(span, g.co, g.cgo);
  float* tile = gc_lds;                           // [sh_ * sw_][pitch]
  float* wl = gc_lds + d.sh_ * d.sw_ * d.pitch;   // [ck * rs][GC_WP]
  const int oy0 = tiy * d.th, ox0 = tix * GC_TW;
  int base[GC_QW];
  gc_v4 acc[GC_QW];
#pragma unroll
  for (int q = 0; q < GC_QW; ++q) {
    const int qi = l.wave * qw + q;  // (q >= qw: not used)
    base[q] = q < qw ? (((qi >> 1) * g.sh) * d.sw_ + (4 * (qi & 1) + l.li) * g.sw) * d.pitch + l.gl * d.ck : 0;
    acc[q] = gc_v4{0.f, 0.f, 0.f, 0.f};
  }
  for (int term = (MODE == 2 ? 1 : 0); term < (MODE == 1 ? 1 : 2); ++term) {
    const float* __restrict__ act = term ? x : tx;
    const float* __restrict__ mat = term ? V : W;
    for (int c0 = 0; c0 < g.cgi; c0 += d.ck) {
      const int cke = min(d.ck, g.cgi - c0);
      __syncthreads();  // (the previous chunk's readers are done)
      gc_stage<AL>(tile, act, ld, img, g.h, g.w, g.cgi, l.g0, l.ng, c0, cke, d.ck, oy0 * g.sh - g.ph, ox0 * g.sw - g.pw,
                   d.sh_, d.sw_, d.pitch);
      // per channel of the span one contiguous run of cke * rs floats; a channel past the last reads as zero
      for (int idx = threadIdx.x; idx < GC_SPAN * cke * rs; idx += BLOCK) {
        const int chl = idx / (cke * rs), rr = idx - chl * (cke * rs);
        wl[rr * GC_WP + chl] = chl < l.ce ? mat[((int64_t)(l.c0 + chl) * g.cgi + c0) * rs + rr] : 0.f;
      }
      __syncthreads();
      for (int cl = 0; cl < cke; ++cl) {
        for (int i = 0; i < g.r; ++i) {
          for (int j = 0; j < g.s; ++j) {
            const float bv = wl[(cl * rs + i * g.s + j) * GC_WP + l.lane];
            const int off = (i * d.sw_ + j) * d.pitch + cl;
#pragma unroll
            for (int q = 0; q < GC_QW; ++q)
              if (q < qw) acc[q] = gc_mfma(tile[base[q] + off], bv, acc[q]);
          }
        }
      }
    }
  }
  const int ch = l.c0 + l.lane;  // (D: register i = the quad's pixel, lane = 4 * block + j = the span's channel)
#pragma unroll
  for (int q = 0; q < GC_QW; ++q) {
    if (q >= qw) continue;
    const int qi = l.wave * qw + q, oy = oy0 + (qi >> 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ox = ox0 + 4 * (qi & 1) + i;
      if (oy < g.oh && ox < g.ow && ch < g.co)
        chain_store<GC_WT>(out + ((int64_t)(img * g.oh + oy) * g.ow + ox) * g.co + ch, acc[q][i]);
    }
  }
}

// ---- data gradient: one workgroup per (sample, th x 8 tile of INPUT pixels, span of 64 input channels) ----------------
// TWO: D(ga, W) + D(ga1, V) -- the chunk loop once per term through the same cotangent tile and weight table, one acc[]
template <bool AL, bool TWO>
__device__ __forceinline__ void gc_dgrad(float* __restrict__ dx, const float* __restrict__ ga, const float* __restrict__ ga1,
                                         const float* __restrict__ W, const float* __restrict__ V, const GcPlan& g, int b) {
  const GcDir d = g.d;
  const int rs = g.r * g.s, qw = d.th >> 1;
  const int span = b % g.ispans;
  b /= g.ispans;
  const int tix = b % g.dtiles_x;
  b /= g.dtiles_x;
  const int tiy = b % d.tiles_y, img = b / d.tiles_y;
  const GcLane l = gc_lane(span, g.ci, g.cgi);
  float* cot = gc_lds;                            // [sh_ * sw_][pitch]
  float* wl = gc_lds + d.sh_ * d.sw_ * d.pitch;   // [ck * rs][GC_WP]
  const int h0 = tiy * d.th, w0 = tix * GC_TW;
  // the first cotangent row / column any tap of the tile can meet: ceil((h0 + pad - (r - 1)) / stride)
  const int gy0 = gc_floordiv(h0 + g.ph - (g.r - 1) + g.sh - 1, g.sh);
  const int gx0 = gc_floordiv(w0 + g.pw - (g.s - 1) + g.sw - 1, g.sw);
  gc_v4 acc[GC_QW];
#pragma unroll
  for (int q = 0; q < GC_QW; ++q) acc[q] = gc_v4{0.f, 0.f, 0.f, 0.f};
  for (int term = 0; term < (TWO ? 2 : 1); ++term) {
    const float* __restrict__ cog = term ? ga1 : ga;
    const float* __restrict__ mat = term ? V : W;
    for (int o0 = 0; o0 < g.cgo; o0 += d.ck) {
      const int cke = min(d.ck, g.cgo - o0);
      __syncthreads();
      gc_stage<AL>(cot, cog, g.co, img, g.oh, g.ow, g.cgo, l.g0, l.ng, o0, cke, d.ck, gy0, gx0, d.sh_, d.sw_, d.pitch);
      // W[group's output channel o0 + ol][input channel of the span][tap] -> wl[(ol, tap)][input channel]: consecutive
      // channels of one group are one contiguous run of the parameter
      for (int idx = threadIdx.x; idx < cke * GC_SPAN * rs; idx += BLOCK) {
        const int tap = idx % rs, t = idx / rs;
        const int cl = t % GC_SPAN, ol = t / GC_SPAN;
        const int c = l.c0 + cl;
        float v = 0.f;
        if (c < g.ci) {
          const int grp = c / g.cgi, cil = c - grp * g.cgi;
          v = mat[((int64_t)(grp * g.cgo + o0 + ol) * g.cgi + cil) * rs + tap];
        }
        wl[(ol * rs + tap) * GC_WP + cl] = v;
      }
      __syncthreads();
      for (int ol = 0; ol < cke; ++ol) {
        for (int i = 0; i < g.r; ++i) {
          for (int j = 0; j < g.s; ++j) {
            const float bv = wl[(ol * rs + i * g.s + j) * GC_WP + l.lane];
#pragma unroll
            for (int q = 0; q < GC_QW; ++q) {
              if (q >= qw) continue;
              const int qi = l.wave * qw + q;
              const int t = h0 + (qi >> 1) + g.ph - i;  // (uniform for the quad)
              if (t < 0 || t % g.sh) continue;
              const int ly = t / g.sh - gy0;   // 0 <= ly < sh_: (t_max - t_min) / stride <= (th + r - 2) / stride
              const int u = w0 + 4 * (qi & 1) + l.li + g.pw - j;
              const bool on = u >= 0 && u % g.sw == 0;
              const int lx = on ? u / g.sw - gx0 : 0;
              const float av = cot[(ly * d.sw_ + lx) * d.pitch + l.gl * d.ck + ol];
              acc[q] = gc_mfma(on ? av : 0.f, bv, acc[q]);
            }
          }
        }
      }
    }
  }
  const int ch = l.c0 + l.lane;
#pragma unroll
  for (int q = 0; q < GC_QW; ++q) {
    if (q >= qw) continue;
    const int qi = l.wave * qw + q, hy = h0 + (qi >> 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int wx = w0 + 4 * (qi & 1) + i;
      if (hy < g.h && wx < g.w && ch < g.ci)
        chain_store<GC_WT>(dx + ((int64_t)(img * g.h + hy) * g.w + wx) * g.ci + ch, acc[q][i]);
    }
  }
}

// ---- weight gradient: one workgroup per (run of units, pass, span of 64 output channels) -------------------------------
// TWO: W(x, ga) + W(tx, ga1) -- per unit the halo of x and the tile of ga, the pixel loop, then the halo of tx and the tile
// of ga1 through the same staging area, the pixel loop again; the slot accumulators are kept over both.
// SQ (the squared sum): a run is `per` SAMPLES; at a sample's last tile every lane folds the entries it owns.
template <bool AL, bool TWO, bool SQ>
__device__ __forceinline__ void gc_wgrad(float* __restrict__ gw, const float* __restrict__ ga, const float* __restrict__ ga1,
                                         const float* __restrict__ x, const float* __restrict__ tx, int64_t ld,
                                         int64_t slab_stride, float pre, const GcPlan& g, int b) {
  const GcDir d = g.g;
  const int rs = g.r * g.s, npix = d.th * GC_TW;
  const int span = b % g.ospans;
  b /= g.ospans;
  const int pass = b % g.passes, split = b / g.passes;
  const GcLane l = gc_lane(span, g.co, g.cgo);
  const int c0 = pass * d.ck, cke = min(d.ck, g.cgi - c0), qk = cke >> 2, nslots = rs * qk;
  float* xt = gc_lds;                             // [sh_ * sw_][pitch]
  float* gt = gc_lds + d.sh_ * d.sw_ * d.pitch;   // [th * 8][GC_WP]
  int soff[GC_WSLOTS];                            // the slot's offset from a pixel's first word of the halo tile
  gc_v4 acc[GC_WSLOTS];
  gc_v4 sq[SQ ? GC_WSLOTS : 1];                   // SQ: the run's sums of squares, entry for entry as acc[]
#pragma unroll
  for (int m = 0; m < GC_WSLOTS; ++m) {
    const int sl = l.wave + WAVES * m, tap = sl / qk, ciq = sl - tap * qk;
    soff[m] = sl < nslots ? ((tap / g.s) * d.sw_ + tap % g.s) * d.pitch + 4 * ciq : 0;
    acc[m] = gc_v4{0.f, 0.f, 0.f, 0.f};
    if constexpr (SQ) sq[m] = gc_v4{0.f, 0.f, 0.f, 0.f};
  }
  const int tiles = g.tiles_x * d.tiles_y;  // (units per sample)
  const int u0 = split * g.per * (SQ ? tiles : 1);
  const int u1 = SQ ? min(g.n, (split + 1) * g.per) * tiles : min(g.units, u0 + g.per);
  for (int u = u0; u < u1; ++u) {
    const int tix = u % g.tiles_x, tiy = (u / g.tiles_x) % d.tiles_y, img = u / tiles;
    for (int term = 0; term < (TWO ? 2 : 1); ++term) {
      const float* __restrict__ act = term ? tx : x;
      const float* __restrict__ cog = term ? ga1 : ga;
      __syncthreads();  // (the previous unit's or term's readers are done)
      gc_stage<AL>(xt, act, ld, img, g.h, g.w, g.cgi, l.g0, l.ng, c0, cke, d.ck, tiy * d.th * g.sh - g.ph,
                   tix * GC_TW * g.sw - g.pw, d.sh_, d.sw_, d.pitch);
      // the cotangent tile, zeros outside the map and past the last channel
      for (int idx = threadIdx.x; idx < npix * (GC_SPAN / 4); idx += BLOCK) {
        const int qd = idx % (GC_SPAN / 4), p = idx / (GC_SPAN / 4);
        const int oy = tiy * d.th + p / GC_TW, ox = tix * GC_TW + p % GC_TW, ch = l.c0 + 4 * qd;
        F4 v;
        v.e[0] = v.e[1] = v.e[2] = v.e[3] = 0.f;
        if (oy < g.oh && ox < g.ow && ch < g.co)
          v = gc_ld_quad<AL>(cog + ((int64_t)(img * g.oh + oy) * g.ow + ox) * g.co + ch);
#pragma unroll
        for (int e = 0; e < 4; ++e) gt[p * GC_WP + 4 * qd + e] = v.e[e];
      }
      __syncthreads();
      for (int p = 0; p < npix; ++p) {
        const float av = gt[p * GC_WP + l.lane];  // (A: block = output-channel quad, row i = its channel)
        const int base = ((p / GC_TW) * g.sh * d.sw_ + (p % GC_TW) * g.sw) * d.pitch + l.gl * d.ck + l.li;
#pragma unroll
        for (int m = 0; m < GC_WSLOTS; ++m)
          if (l.wave + WAVES * m < nslots) acc[m] = gc_mfma(av, xt[base + soff[m]], acc[m]);
      }
    }
    if constexpr (SQ) {
      if ((u + 1) % tiles == 0) {  // the sample boundary: registers only, each entry by its one owner lane
#pragma unroll
        for (int m = 0; m < GC_WSLOTS; ++m) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float t = acc[m][i] * pre;  // (one rounding; then two)
            sq[m][i] += t * t;
          }
          acc[m] = gc_v4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  }
  // D: register i = channel i of the block's output quad, lane's column j = channel j of the slot's input quad
  float* slab = gw + (int64_t)split * slab_stride;
#pragma unroll
  for (int m = 0; m < GC_WSLOTS; ++m) {
    const int sl = l.wave + WAVES * m;
    if (sl >= nslots) continue;
    const int tap = sl / qk, ciq = sl - tap * qk;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = l.c0 + 4 * l.blk + i;
      if (co < g.co)
        chain_store<GC_WT>(slab + ((int64_t)co * g.cgi + c0 + 4 * ciq + l.li) * rs + tap, SQ ? sq[m][i] : acc[m][i]);
    }
  }
}

// the one grid of a backward launch: data-gradient blocks first, then the weight-gradient blocks
template <bool AL, bool TWO>
__global__ void __launch_bounds__(BLOCK)
k_gc_backward(float* __restrict__ dx, float* __restrict__ gw, const float* __restrict__ ga, const float* __restrict__ ga1,
              const float* __restrict__ x, const float* __restrict__ tx, int64_t ld, const float* __restrict__ W,
              const float* __restrict__ V, int64_t slab_stride, int d_blocks, const GcPlan g) {
  const int b = blockIdx.x;
  if (b < d_blocks) gc_dgrad<AL, TWO>(dx, ga, ga1, W, V, g, b);
  else gc_wgrad<AL, TWO, false>(gw, ga, ga1, x, tx, ld, slab_stride, 0.f, g, b - d_blocks);
}

// ---- squared sum: one workgroup per (split of the samples, pass, span of 64 output channels); g.per = samples per split
template <bool AL>
__global__ void __launch_bounds__(BLOCK)
k_gc_sqsum(float* __restrict__ out, const float* __restrict__ ga, const float* __restrict__ x, int64_t ld, float pre,
           int64_t slab_stride, const GcPlan g) {
  gc_wgrad<AL, false, true>(out, ga, nullptr, x, nullptr, ld, slab_stride, pre, g, blockIdx.x);
}

// The squared sum's plan: gc_plan, then the split of the SAMPLES towards `target` workgroups (0: GC_TARGET_BLOCKS).
inline int gc_sq_plan(int64_t n, int64_t h, int64_t w, int64_t ci, int64_t co, int64_t groups, int64_t r, int64_t s,
                      int64_t sh, int64_t sw, int64_t ph, int64_t pw, int target, GcPlan* p) {
  if (target < 0 || gc_plan(n, h, w, ci, co, groups, r, s, sh, sw, ph, pw, p) != HF_OK) return HF_ERR_ARG;
  const int64_t wg = (int64_t)p->ospans * p->passes;  // workgroups per split
  int64_t want = ((target ? target : GC_TARGET_BLOCKS) + wg - 1) / wg;
  if (want > GC_MAX_SPLITS) want = GC_MAX_SPLITS;
  if (want > n) want = n;
  const int64_t per = (n + want - 1) / want;
  p->per = (int)per, p->splits_w = (int)((n + per - 1) / per);  // (no split without a sample)
  return HF_OK;
}

// The backward launch of both forms.  terms == 1: ga1, tx and V are NULL; dx may be NULL (W is then not read).
int gc_backward_launch(int terms, void* dx, void* gw_slabs, const void* ga, const void* ga1, const void* x, const void* tx,
                       int64_t act_ld, const void* W, const void* V, int64_t n, int64_t h, int64_t w, int64_t c_in,
                       int64_t c_out, int64_t groups, int64_t r, int64_t s, int64_t stride_h, int64_t stride_w,
                       int64_t pad_h, int64_t pad_w, int splits_w, int64_t slab_stride, int dtype, void* stream) {
  GcPlan p;
  if (gc_plan(n, h, w, c_in, c_out, groups, r, s, stride_h, stride_w, pad_h, pad_w, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !gw_slabs || !ga || !x) return HF_ERR_ARG;
  if (terms == 2 && (!dx || !ga1 || !tx || !W || !V)) return HF_ERR_ARG;
  if (dx && !W) return HF_ERR_ARG;
  if (splits_w != p.splits_w) return HF_ERR_ARG;
  if (splits_w > 1 && slab_stride < (int64_t)p.co * p.cgi * p.r * p.s) return HF_ERR_ARG;
  if (act_ld == 0) act_ld = c_in;
  if (act_ld < c_in || act_ld > 2 * c_in) return HF_ERR_ARG;
  const bool al = quad_ok(x, act_ld) && aligned16(ga) && (terms == 1 || (quad_ok(tx, act_ld) && aligned16(ga1)));
  const int d_blocks = dx ? p.n * p.d.tiles_y * p.dtiles_x * p.ispans : 0;
  const unsigned grid = (unsigned)(d_blocks + p.ospans * p.passes * p.splits_w);
  int64_t words = gc_lds_words(p.g, p.g.th * GC_TW);
  if (dx && gc_lds_words(p.d, p.d.ck * p.r * p.s) > words) words = gc_lds_words(p.d, p.d.ck * p.r * p.s);
  hipStream_t st = (hipStream_t)stream;
#define HF_GC_B(AL, TWO)                                                                                               \
  k_gc_backward<AL, TWO><<<grid, BLOCK, (size_t)words * 4, st>>>(                                                      \
      (float*)dx, (float*)gw_slabs, (const float*)ga, (const float*)ga1, (const float*)x, (const float*)tx, act_ld,    \
      (const float*)W, (const float*)V, slab_stride, d_blocks, p)
  if (terms == 2) {
    if (al) HF_GC_B(true, true);
    else HF_GC_B(false, true);
  } else {
    if (al) HF_GC_B(true, false);
    else HF_GC_B(false, false);
  }
#undef HF_GC_B
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int hf_gconv2d_nhwc_plan(int64_t n, int64_t h, int64_t w, int64_t c_in, int64_t c_out, int64_t groups, int64_t r, int64_t s,
                         int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w) {
  GcPlan p;
  if (gc_plan(n, h, w, c_in, c_out, groups, r, s, stride_h, stride_w, pad_h, pad_w, &p) != HF_OK) return HF_ERR_ARG;
  return p.splits_w;
}

int hf_gconv2d_nhwc_tangent(void* out, const void* t_x, const void* x, int64_t act_ld, const void* W, const void* V,
                            int64_t n, int64_t h, int64_t w, int64_t c_in, int64_t c_out, int64_t groups, int64_t r,
                            int64_t s, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int dtype,
                            void* stream) {
  GcPlan p;
  if (gc_plan(n, h, w, c_in, c_out, groups, r, s, stride_h, stride_w, pad_h, pad_w, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out) return HF_ERR_ARG;
  if (!t_x && !V) return HF_ERR_ARG;  // nothing to compute
  if ((t_x && !W) || (V && !x)) return HF_ERR_ARG;
  if (act_ld == 0) act_ld = c_in;
  if (act_ld < c_in || act_ld > 2 * c_in) return HF_ERR_ARG;
  const bool al = (!t_x || quad_ok(t_x, act_ld)) && (!V || quad_ok(x, act_ld));
  const int mode = (t_x && V) ? 0 : (t_x ? 1 : 2);
  const unsigned grid = (unsigned)((int64_t)p.n * p.t.tiles_y * p.tiles_x * p.ospans);
  const size_t lds = (size_t)gc_lds_words(p.t, p.t.ck * p.r * p.s) * 4;
  hipStream_t st = (hipStream_t)stream;
#define HF_GC_T(AL, MODE)                                                                                              \
  k_gc_tangent<AL, MODE><<<grid, BLOCK, lds, st>>>((float*)out, (const float*)t_x, (const float*)x, act_ld,          \
                                                    (const float*)W, (const float*)V, p)
  if (al) {
    if (mode == 0) HF_GC_T(true, 0);
    else if (mode == 1) HF_GC_T(true, 1);
    else HF_GC_T(true, 2);
  } else {
    if (mode == 0) HF_GC_T(false, 0);
    else if (mode == 1) HF_GC_T(false, 1);
    else HF_GC_T(false, 2);
  }
#undef HF_GC_T
  return (int)hipGetLastError();
}

int hf_gconv2d_nhwc_backward_slabs(void* dx, void* gw_slabs, const void* ga, const void* x, int64_t act_ld, const void* W,
                                   int64_t n, int64_t h, int64_t w, int64_t c_in, int64_t c_out, int64_t groups, int64_t r,
                                   int64_t s, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w,
                                   int splits_w, int64_t slab_stride, int dtype, void* stream) {
  return gc_backward_launch(1, dx, gw_slabs, ga, nullptr, x, nullptr, act_ld, W, nullptr, n, h, w, c_in, c_out, groups, r, s,
                            stride_h, stride_w, pad_h, pad_w, splits_w, slab_stride, dtype, stream);
}

int hf_gconv2d_nhwc_backward2_slabs(void* dx, void* gw_slabs, const void* ga_t, const void* ga, const void* x,
                                    const void* t_x, int64_t act_ld, const void* W, const void* V, int64_t n, int64_t h,
                                    int64_t w, int64_t c_in, int64_t c_out, int64_t groups, int64_t r, int64_t s,
                                    int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int splits_w,
                                    int64_t slab_stride, int dtype, void* stream) {
  return gc_backward_launch(2, dx, gw_slabs, ga_t, ga, x, t_x, act_ld, W, V, n, h, w, c_in, c_out, groups, r, s, stride_h,
                            stride_w, pad_h, pad_w, splits_w, slab_stride, dtype, stream);
}

int hf_gconv2d_nhwc_sqsum_plan(int64_t n, int64_t h, int64_t w, int64_t c_in, int64_t c_out, int64_t groups, int64_t r,
                               int64_t s, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w,
                               int target_blocks) {
  GcPlan p;
  if (gc_sq_plan(n, h, w, c_in, c_out, groups, r, s, stride_h, stride_w, pad_h, pad_w, target_blocks, &p) != HF_OK)
    return HF_ERR_ARG;
  return p.splits_w;
}

int hf_gconv2d_nhwc_sqsum_slabs(void* out, const void* ga, const void* x, int64_t act_ld, int64_t n, int64_t h, int64_t w,
                                int64_t c_in, int64_t c_out, int64_t groups, int64_t r, int64_t s, int64_t stride_h,
                                int64_t stride_w, int64_t pad_h, int64_t pad_w, float pre, int splits, int64_t slab_stride,
                                int dtype, void* stream) {
  GcPlan p;
  if (gc_sq_plan(n, h, w, c_in, c_out, groups, r, s, stride_h, stride_w, pad_h, pad_w, 0, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out || !ga || !x) return HF_ERR_ARG;
  if (!(pre - pre == 0.f)) return HF_ERR_ARG;  // (NaN / infinity)
  if (splits < 1 || splits > n) return HF_ERR_ARG;
  const int per = (int)((n + splits - 1) / splits);
  if ((int64_t)(splits - 1) * per >= n) return HF_ERR_ARG;  // (a split without a sample)
  if (splits > 1 && slab_stride < (int64_t)p.co * p.cgi * p.r * p.s) return HF_ERR_ARG;
  if (act_ld == 0) act_ld = c_in;
  if (act_ld < c_in || act_ld > 2 * c_in) return HF_ERR_ARG;
  p.per = per, p.splits_w = splits;
  const unsigned grid = (unsigned)((int64_t)p.ospans * p.passes * splits);
  const size_t lds = (size_t)gc_lds_words(p.g, p.g.th * GC_TW) * 4;
  hipStream_t st = (hipStream_t)stream;
  if (quad_ok(x, act_ld) && aligned16(ga))
    k_gc_sqsum<true><<<grid, BLOCK, lds, st>>>((float*)out, (const float*)ga, (const float*)x, act_ld, pre, slab_stride, p);
  else
    k_gc_sqsum<false><<<grid, BLOCK, lds, st>>>((float*)out, (const float*)ga, (const float*)x, act_ld, pre, slab_stride, p);
  return (int)hipGetLastError();
}

}  // extern "C"
