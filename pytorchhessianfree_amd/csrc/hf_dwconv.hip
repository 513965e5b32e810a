// hf_dwconv.hip -- depthwise convolutions (groups == c_in == c_out == c) of the plain-stack engine (engine/plain.py):
// the tangent / forward map, the data + weight gradient of one cotangent in ONE launch, the tangent of that backward sweep
// (a Hessian product's two-term form) in ONE launch, and the sum over the samples of the squared per-sample weight gradient
// (the batched diagonal empirical Fisher) in ONE launch.  fp32, wave64, NHWC, c % 4 == 0,
// r*s <= 49 taps, per-axis stride and padding, dilation 1.  Plain C++/HIP, no atomics; every output is summed in one fixed
// order (below), so two launches on the same operands agree bitwise.
//
// Why a design of its own.  A depthwise convolution has no reduction over channels: an implicit GEMM has nothing to
// multiply.  It does 2*r*s flop per output element against >= 8 bytes moved (18 flop / 8 B for 3x3: far below the ~20
// flop/B at which fp32 FMA meets 8 TB/s), so the design is about bytes and LDS reuse, not about the MFMA.
//
// Work split.  A lane owns 4 consecutive channels (one 16-byte load / store wherever base and pixel pitch allow; the
// host picks the aligned or the element-wise form, as quad_ok does in hf_dense.hip).  A workgroup (256 lanes) owns a
// channel block of cb <= 32 channels (cb/4 quads) x an 8x8 tile of OUTPUT pixels (tangent, weight gradient) or INPUT
// pixels (data gradient): lane = pixel slot * (cb/4) + quad, so with cb = 32 a wave covers one tile row of 8 pixels x 128
// contiguous bytes each -- its LDS reads are 1 KB contiguous for stride 1, conflict-free -- and a lane computes two pixels.
// The workgroup stages, ONCE, the halo tile of its channels, ((8-1)*stride_h + r) x ((8-1)*stride_w + s) pixels, into LDS;
// padding becomes zeros in LDS at staging time, so no tap carries a predicate on a global load.  The taps of the channel
// block are ONE contiguous run of the parameter ([c, 1, r, s]: cb*r*s floats from ch0*r*s): read in place, coalesced, and
// kept transposed in LDS as [tap][channel], so a lane's four weights of a tap are one 16-byte LDS read (a broadcast across
// the pixels of the wave).  The weight's tangent V is read the same way from the CG vector's slice.  No [W | v_W] operand,
// no transposed copy, no scatter.
//
// Sizes.  cb is the smallest of 4, 8, 16, 32 that is >= min(c, 32), halved while the LDS of any of the three directions
// would exceed 64 KB (two-term tangent: 2 * (halo + r*s) * cb * 4 bytes -- 3x3 stride 1: 100 + 9 pixels -> 27.9 KB at
// cb = 32, five workgroups per CU; 7x7 stride 1: 196 + 49 -> 62.7 KB, two per CU; 7x7 stride 2 halves cb to 16).  8x8 tiles:
// the halo re-reads 100/64 = 1.56x of the input for 3x3 stride 1, i.e. (2 * 1.56 + 1) * 4 = 16.5 bytes per output element
// of the two-term tangent against 12 algorithmic; 16x16 tiles would bring 1.27x but quarter the workgroups, and the maps of
// a CIFAR-sized net need them: batch 32, 32x32x32 -> 512 workgroups of 256 lanes (2 per CU); 16x16x128 -> 512; 8x8x256 ->
// 256; 4x4x512 -> 512 workgroups whose tile is a quarter full (a 4x4 map IS the tile: latency-bound, nothing to reuse).
//
// Addition orders (fmaf chains from zero: one rounding per product-and-add).
//   tangent:        taps ascending (i, j); within a tap first t_x * W, then x * V.
//   data gradient:  taps ascending (i, j) over the taps whose division is exact; a cotangent pixel outside the map is a
//                   zero in LDS (adding it is exact).
//   weight gradient: the (sample, output tile) units in ascending order are cut into splits_w consecutive runs of `per`
//                   units (the last may be shorter); run s leaves slab s, [c*r*s] in PARAMETER order.  Per unit and tap: a
//                   lane's chain over its pixels (ascending), the 64/(cb/4) pixel slots of a wave joined by a
//                   __shfl_down tree (offsets 32, 16, .. cb/4), the four waves added in wave order through LDS, and that
//                   sum added to the run's accumulator (units ascending).  hf_pack_ex adds the slabs in split order.
//
// The two-term backward (hf_dwconv2d_nhwc_backward2_slabs): dx = D(g', W) + D(g, V), slabs = W(x, g') + W(t_x, g) -- the same
// kernels under a template flag (TWO), not a second launch into "extras" slabs: a bandwidth-bound layer would write dx twice,
// have its consumer read it twice and double the weight-gradient slabs.  Each staging step loads both operands of a pair
// (g' / g: both dense; x / t_x: one pitch) from ONE index computation into two LDS tiles, and a lane feeds both products of
// a pixel into the SAME accumulator.  The LDS need roughly doubles, so the form has a plan of its own (terms = 2: cb may be
// smaller, and with it the split count may differ):
//   data gradient 2 * (r*s + cot) * cb * 4 bytes;  weight gradient ((2*halo + 2*64 + WAVES*DW_TAPCH + r*s) * cb + DW_TOFF) * 4.
//   3x3 stride 1: cb = 32, weight gradient 2*100 + 128 + 36 + 9 = 373 pixels-or-taps -> 48 000 B (data gradient 27 904 B);
//   5x5 stride 1: cb = 32, 2*144 + 128 + 36 + 25 = 477 -> 61 312 B (data gradient 43 264 B);
//   7x7 stride 1: cb = 32 would need 77 696 B -> cb = 16, 2*196 + 128 + 36 + 49 = 605 -> 38 976 B (data gradient 31 360 B).
// Addition orders of the two-term form:
//   data gradient:  taps ascending (i, j) as above; within a tap first g' * W, then g * V.
//   weight gradient: per pixel first g' * x, then g * t_x, into the lane's one chain; then the same wave tree, wave order
//                   and unit order as the one-term kernel.
//
// The squared sum (hf_dwconv2d_nhwc_sqsum_slabs): out[ch][tap] = sum_i (pre * gw_i[ch][tap])^2 over the per-sample weight
// gradients gw_i.  It is the weight-gradient loop with a sample boundary in it: a workgroup owns (split of the SAMPLES,
// channel block), runs the one-term unit loop over a sample's output tiles (ascending) into the LDS accumulator [tap][cb],
// and at the sample's end folds it:  t = acc * pre (one rounding), sq += t * t (two roundings), acc = 0; samples ascending;
// sq [tap][cb] (r*s*cb more LDS words) goes to the split's slab in parameter order.  Its plan (terms = DW_SQSUM) takes the
// largest cb whose LDS fits, then halves it while cb > 16 and n * channel blocks < 512: with cb = 16 a workgroup's 64
// pixel slots are exactly the 64 pixels of a tile (every lane still has work; below 16 lanes idle), and a batch of 32
// samples x 128 channels goes from 32 * 4 = 128 to 32 * 8 = 256 workgroups, one per CU.  The samples are cut into
// min(n, 64, ceil(target / channel blocks)) runs of ceil(n / runs) samples, none empty.
#include "hf_common.h"

namespace {

constexpr int DW_TILE = 8;                  // tile edge, pixels
constexpr int DW_PIX = DW_TILE * DW_TILE;
constexpr int DW_CB = 32;                   // most channels per workgroup: 8 quads
constexpr int DW_MAX_TAPS = 49;
constexpr int DW_MAX_STRIDE = 8;
constexpr int DW_TAPCH = 9;                 // taps a lane accumulates at once in the weight gradient (36 registers)
constexpr int DW_LDS_BYTES = 64 * 1024;
constexpr int DW_TARGET_BLOCKS = 512;       // weight-gradient workgroups the plan aims at (2 per CU)
constexpr int DW_MAX_SPLITS = 64;
constexpr int DW_TOFF = 64;                 // LDS words of the tap-offset table (>= DW_MAX_TAPS, 16-byte multiple)
constexpr int DW_SQSUM = 0;                 // dw_plan's `terms` for the squared-sum launch (one term, splits over the samples)
constexpr int DW_SQ_MIN_CB = 16;            // the squared sum trades channels per workgroup for workgroups down to here

// ---- the plan: ONE definition, run by hf_dwconv2d_nhwc_plan and by every launching entry point ----------------------
struct DwPlan {
  int n, h, w, c, r, s, sh, sw, ph, pw, oh, ow;
  int cb, cblocks;                          // channels per workgroup, channel blocks
  int tiles_y, tiles_x, halo_h, halo_w;     // output tiles; staged input pixels per output tile
  int dtiles_y, dtiles_x, cot_h, cot_w;     // input tiles; staged cotangent pixels per input tile
  int units, per, splits_w;                 // weight gradient: (sample, output tile) units, units per split, splits
};                                          // (the squared sum: the units are the samples)

inline int64_t dw_lds_tangent(const DwPlan& p, int terms) {
  return (int64_t)terms * (p.r * p.s + p.halo_h * p.halo_w) * p.cb * 4;
}
inline int64_t dw_lds_dgrad(const DwPlan& p, int terms) {
  return (int64_t)terms * (p.r * p.s + p.cot_h * p.cot_w) * p.cb * 4;
}
// (sq: the squared sum keeps a second [tap][cb] table)
inline int64_t dw_lds_wgrad(const DwPlan& p, int terms, bool sq = false) {
  const int64_t per_ch = terms * (p.halo_h * p.halo_w + DW_PIX) + WAVES * DW_TAPCH + (sq ? 2 : 1) * p.r * p.s;
  return (per_ch * p.cb + DW_TOFF) * 4;
}
// what the launches planned with `terms` need: 1 = tangent (both terms), data and weight gradient of one cotangent;
// 2 = the two-term backward; DW_SQSUM = the squared sum
inline bool dw_lds_fits(const DwPlan& p, int terms) {
  if (terms == DW_SQSUM) return dw_lds_wgrad(p, 1, true) <= DW_LDS_BYTES;
  if (terms == 2) return dw_lds_dgrad(p, 2) <= DW_LDS_BYTES && dw_lds_wgrad(p, 2) <= DW_LDS_BYTES;
  return dw_lds_tangent(p, 2) <= DW_LDS_BYTES && dw_lds_dgrad(p, 1) <= DW_LDS_BYTES && dw_lds_wgrad(p, 1) <= DW_LDS_BYTES;
}

// terms: 1, 2 or DW_SQSUM (above); target: the workgroups the split count aims at (0: DW_TARGET_BLOCKS)
inline int dw_plan(int64_t n, int64_t h, int64_t w, int64_t c, int64_t r, int64_t s, int64_t sh, int64_t sw, int64_t ph,
                   int64_t pw, int terms, int target, DwPlan* p) {
  if (target < 0) return HF_ERR_ARG;
  if (n < 1 || h < 1 || w < 1 || c < 4 || (c & 3) || r < 1 || s < 1 || r * s > DW_MAX_TAPS) return HF_ERR_ARG;
  if (sh < 1 || sw < 1 || sh > DW_MAX_STRIDE || sw > DW_MAX_STRIDE || ph < 0 || pw < 0 || ph >= r || pw >= s)
    return HF_ERR_ARG;
  if (h + 2 * ph < r || w + 2 * pw < s) return HF_ERR_ARG;
  const int64_t oh = (h + 2 * ph - r) / sh + 1, ow = (w + 2 * pw - s) / sw + 1;
  if (n * h * w * c >= (1LL << 31) || n * oh * ow * c >= (1LL << 31)) return HF_ERR_ARG;
  p->n = (int)n, p->h = (int)h, p->w = (int)w, p->c = (int)c, p->r = (int)r, p->s = (int)s;
  p->sh = (int)sh, p->sw = (int)sw, p->ph = (int)ph, p->pw = (int)pw, p->oh = (int)oh, p->ow = (int)ow;
  p->tiles_y = (int)((oh + DW_TILE - 1) / DW_TILE), p->tiles_x = (int)((ow + DW_TILE - 1) / DW_TILE);
  p->dtiles_y = (int)((h + DW_TILE - 1) / DW_TILE), p->dtiles_x = (int)((w + DW_TILE - 1) / DW_TILE);
  p->halo_h = (DW_TILE - 1) * p->sh + p->r, p->halo_w = (DW_TILE - 1) * p->sw + p->s;
  p->cot_h = (DW_TILE + p->r - 2) / p->sh + 1, p->cot_w = (DW_TILE + p->s - 2) / p->sw + 1;
  int cb = DW_CB;
  while (cb / 2 >= c) cb /= 2;
  for (;; cb /= 2) {
    if (cb < 4) return HF_ERR_ARG;
    p->cb = cb;
    if (dw_lds_fits(*p, terms)) break;
  }
  if (terms == DW_SQSUM)
    while (cb > DW_SQ_MIN_CB && n * ((c + cb - 1) / cb) < DW_TARGET_BLOCKS) cb /= 2;
  p->cb = cb;
  p->cblocks = (int)((c + cb - 1) / cb);
  if (n * p->tiles_y * p->tiles_x * p->cblocks >= (1LL << 31) || n * p->dtiles_y * p->dtiles_x * p->cblocks >= (1LL << 30))
    return HF_ERR_ARG;
  const int64_t units = terms == DW_SQSUM ? n : n * p->tiles_y * p->tiles_x;
  int64_t want = ((target ? target : DW_TARGET_BLOCKS) + p->cblocks - 1) / p->cblocks;
  if (want > DW_MAX_SPLITS) want = DW_MAX_SPLITS;
  if (want > units) want = units;
  const int64_t per = (units + want - 1) / want;
  p->units = (int)units, p->per = (int)per, p->splits_w = (int)((units + per - 1) / per);  // (no empty split)
  return HF_OK;
}

inline bool quad_ok(const void* p, int64_t pitch) { return aligned16(p) && (pitch & 3) == 0; }

// ---- device helpers ------------------------------------------------------------------------------------------------
constexpr bool DW_WT = HF_WT_CONV != 0;

__device__ __forceinline__ F4 zero4() {
  F4 z;
  z.e[0] = z.e[1] = z.e[2] = z.e[3] = 0.f;
  return z;
}

template <bool AL>
__device__ __forceinline__ F4 ld_quad(const float* __restrict__ p) {
  if constexpr (AL) {
    return ld4(p);
  } else {
    F4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v.e[k] = p[k];
    return v;
  }
}

template <bool AL>
__device__ __forceinline__ void st_quad(float* __restrict__ p, const F4& v) {
  if constexpr (AL) {
    chain_store4<DW_WT>(p, v);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) chain_store<DW_WT>(p + k, v.e[k]);
  }
}

__device__ __forceinline__ F4 lds4(const float* p) { return *reinterpret_cast<const F4*>(p); }

// acc = a * b + acc, per channel: one rounding each
__device__ __forceinline__ void fma4(F4& acc, const F4& a, const F4& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) acc.e[k] = fmaf(a.e[k], b.e[k], acc.e[k]);
}

__device__ __forceinline__ int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// Rows y0 .. y0+ny-1 x columns x0 .. x0+nx-1 of image `img` of an NHWC map [., H, W, .] with pixel pitch ld, channels
// ch0 .. ch0+cb-1, into dst[(py * pitch_w + px) * cb + channel].  A pixel outside the map and a channel >= c is a zero
// in LDS and is not read.  TWO: the same pixels of a second map src2 of the SAME shape and pitch into dst2, both loads
// and both stores from one index computation.
template <bool AL, bool TWO = false>
__device__ __forceinline__ void dw_stage(float* dst, const float* __restrict__ src, int64_t ld, int img, int H, int W,
                                         int c, int ch0, int cb, int y0, int x0, int ny, int nx, int pitch_w,
                                         float* dst2 = nullptr, const float* __restrict__ src2 = nullptr) {
  const int qb = cb >> 2, total = ny * nx * qb;
  for (int idx = threadIdx.x; idx < total; idx += BLOCK) {
    const int q = idx % qb, p = idx / qb;
    const int py = p / nx, px = p - py * nx;
    const int y = y0 + py, x = x0 + px, ch = ch0 + 4 * q;
    F4 v = zero4(), v2 = zero4();
    if (y >= 0 && y < H && x >= 0 && x < W && ch < c) {
      const int64_t at = ((int64_t)(img * H + y) * W + x) * ld + ch;
      v = ld_quad<AL>(src + at);
      if constexpr (TWO) v2 = ld_quad<AL>(src2 + at);
    }
    const int to = (py * pitch_w + px) * cb + 4 * q;
    *reinterpret_cast<F4*>(dst + to) = v;
    if constexpr (TWO) *reinterpret_cast<F4*>(dst2 + to) = v2;
  }
}

// The channel block's taps, cbe * rs contiguous floats of the parameter from ch0 * rs, transposed into wl[tap][cb];
// channels >= cbe read as zero.  TWO: the same run of V into wl2.
template <bool TWO = false>
__device__ __forceinline__ void dw_stage_taps(float* wl, const float* __restrict__ W, int ch0, int cbe, int cb, int rs,
                                              float* wl2 = nullptr, const float* __restrict__ V = nullptr) {
  for (int idx = threadIdx.x; idx < cb * rs; idx += BLOCK) {
    const int chl = idx / rs, tap = idx - chl * rs;
    const int64_t at = (int64_t)ch0 * rs + idx;
    wl[tap * cb + chl] = chl < cbe ? W[at] : 0.f;
    if constexpr (TWO) wl2[tap * cb + chl] = chl < cbe ? V[at] : 0.f;
  }
}

extern __shared__ __align__(16) float dw_lds[];

// ---- tangent / forward -----------------------------------------------------------------------------------------------
// MODE 0: t_x * W + x * V;  1: t_x * W (V == NULL);  2: x * V (t_x == NULL; the forward pass with V = W)
template <bool AL, int MODE>
__global__ void __launch_bounds__(BLOCK)
k_dw_tangent(float* __restrict__ out, const float* __restrict__ tx, const float* __restrict__ x, int64_t ld,
             const float* __restrict__ W, const float* __restrict__ V, const DwPlan g) {
  constexpr int NT = MODE == 0 ? 2 : 1;
  const int rs = g.r * g.s, cb = g.cb, qb = cb >> 2, halo = g.halo_h * g.halo_w;
  int b = blockIdx.x;
  const int cblk = b % g.cblocks;
  b /= g.cblocks;
  const int tix = b % g.tiles_x;
  b /= g.tiles_x;
  const int tiy = b % g.tiles_y, img = b / g.tiles_y;
  const int ch0 = cblk * cb, cbe = min(cb, g.c - ch0);
  float* wl = dw_lds;                  // [term][tap][cb]
  float* tile = wl + NT * rs * cb;     // [term][halo_h * halo_w][cb]
  float* wl2 = wl + (NT - 1) * rs * cb;
  float* tile2 = tile + (NT - 1) * halo * cb;
  const int oy0 = tiy * DW_TILE, ox0 = tix * DW_TILE;
  const int ny = min(DW_TILE, g.oh - oy0), nx = min(DW_TILE, g.ow - ox0);
  const int sy = (ny - 1) * g.sh + g.r, sx = (nx - 1) * g.sw + g.s;  // what the tile's outputs read of the halo
  if (MODE != 2) {
    dw_stage_taps(wl, W, ch0, cbe, cb, rs);
    dw_stage<AL>(tile, tx, ld, img, g.h, g.w, g.c, ch0, cb, oy0 * g.sh - g.ph, ox0 * g.sw - g.pw, sy, sx, g.halo_w);
  }
  if (MODE != 1) {
    dw_stage_taps(wl2, V, ch0, cbe, cb, rs);
    dw_stage<AL>(tile2, x, ld, img, g.h, g.w, g.c, ch0, cb, oy0 * g.sh - g.ph, ox0 * g.sw - g.pw, sy, sx, g.halo_w);
  }
  __syncthreads();
  const int q = threadIdx.x % qb, ps = threadIdx.x / qb, pp = BLOCK / qb, ch = ch0 + 4 * q;
  for (int o = ps; o < DW_PIX; o += pp) {
    const int oy = o / DW_TILE, ox = o % DW_TILE;
    if (oy >= ny || ox >= nx || ch >= g.c) continue;
    F4 acc = zero4();
    const int base = oy * g.sh * g.halo_w + ox * g.sw;
    for (int i = 0; i < g.r; ++i) {
      for (int j = 0; j < g.s; ++j) {
        const int pix = (base + i * g.halo_w + j) * cb + 4 * q, tp = (i * g.s + j) * cb + 4 * q;
        if (MODE != 2) fma4(acc, lds4(tile + pix), lds4(wl + tp));
        if (MODE != 1) fma4(acc, lds4(tile2 + pix), lds4(wl2 + tp));
      }
    }
    st_quad<AL>(out + ((int64_t)(img * g.oh + oy0 + oy) * g.ow + ox0 + ox) * g.c + ch, acc);
  }
}

// ---- data gradient: one workgroup per (image, 8x8 tile of INPUT pixels, channel block) -------------------------------
// TWO: D(ga, W) + D(ga1, V) -- two tap tables, two cotangent tiles, one accumulator (ga = g', ga1 = g)
template <bool AL, bool TWO>
__device__ __forceinline__ void dw_dgrad(float* __restrict__ dx, const float* __restrict__ ga,
                                         const float* __restrict__ ga1, const float* __restrict__ W,
                                         const float* __restrict__ V, const DwPlan& g, int b) {
  constexpr int NT = TWO ? 2 : 1;
  const int rs = g.r * g.s, cb = g.cb, qb = cb >> 2, cots = g.cot_h * g.cot_w;
  const int cblk = b % g.cblocks;
  b /= g.cblocks;
  const int tix = b % g.dtiles_x;
  b /= g.dtiles_x;
  const int tiy = b % g.dtiles_y, img = b / g.dtiles_y;
  const int ch0 = cblk * cb, cbe = min(cb, g.c - ch0);
  float* wl = dw_lds;               // [term][tap][cb]
  float* cot = wl + NT * rs * cb;   // [term][cot_h * cot_w][cb]
  float* wl2 = wl + (NT - 1) * rs * cb;
  float* cot2 = cot + (NT - 1) * cots * cb;
  const int h0 = tiy * DW_TILE, w0 = tix * DW_TILE;
  // the first cotangent row / column any tap of the tile can meet: ceil((h0 + pad - (r - 1)) / stride)
  const int gy0 = floordiv(h0 + g.ph - (g.r - 1) + g.sh - 1, g.sh), gx0 = floordiv(w0 + g.pw - (g.s - 1) + g.sw - 1, g.sw);
  dw_stage_taps<TWO>(wl, W, ch0, cbe, cb, rs, wl2, V);
  dw_stage<AL, TWO>(cot, ga, g.c, img, g.oh, g.ow, g.c, ch0, cb, gy0, gx0, g.cot_h, g.cot_w, g.cot_w, cot2, ga1);
  __syncthreads();
  const int q = threadIdx.x % qb, ps = threadIdx.x / qb, pp = BLOCK / qb, ch = ch0 + 4 * q;
  for (int o = ps; o < DW_PIX; o += pp) {
    const int hy = h0 + o / DW_TILE, wx = w0 + o % DW_TILE;
    if (hy >= g.h || wx >= g.w || ch >= g.c) continue;
    F4 acc = zero4();
    for (int i = 0; i < g.r; ++i) {
      const int t = hy + g.ph - i;
      if (t < 0 || t % g.sh) continue;
      const int ly = t / g.sh - gy0;   // 0 <= ly < cot_h: (t_max - t_min) / stride <= (DW_TILE + r - 2) / stride
      for (int j = 0; j < g.s; ++j) {
        const int u = wx + g.pw - j;
        if (u < 0 || u % g.sw) continue;
        const int lx = u / g.sw - gx0;
        const int pix = (ly * g.cot_w + lx) * cb + 4 * q, tp = (i * g.s + j) * cb + 4 * q;
        fma4(acc, lds4(cot + pix), lds4(wl + tp));
        if constexpr (TWO) fma4(acc, lds4(cot2 + pix), lds4(wl2 + tp));
      }
    }
    st_quad<AL>(dx + ((int64_t)(img * g.h + hy) * g.w + wx) * g.c + ch, acc);
  }
}

// ---- weight gradient: one workgroup per (split, channel block) -------------------------------------------------------
// The LDS of a weight-gradient workgroup.  TWO: a second halo tile (t_x beside x) and a second cotangent tile (g beside g').
struct DwWgLds {
  int* toff;     // [tap]: its pixel offset inside the halo tile
  float* xt;     // [halo_h * halo_w][cb]  (TWO: xt2 behind it)
  float* xt2;
  float* gt;     // [8 * 8][cb]            (TWO: gt2 behind it)
  float* gt2;
  float* red;    // [wave][DW_TAPCH][cb]
  float* accl;   // [tap][cb]: the running sums (behind it, the squared sum's second table [tap][cb])
};

template <bool TWO>
__device__ __forceinline__ DwWgLds dw_wg_lds(const DwPlan& g) {
  const int cb = g.cb, halo = g.halo_h * g.halo_w;
  DwWgLds l;
  l.toff = reinterpret_cast<int*>(dw_lds);
  l.xt = dw_lds + DW_TOFF;
  l.xt2 = l.xt + (TWO ? halo * cb : 0);
  l.gt = l.xt2 + halo * cb;
  l.gt2 = l.gt + (TWO ? DW_PIX * cb : 0);
  l.red = l.gt2 + DW_PIX * cb;
  l.accl = l.red + WAVES * DW_TAPCH * cb;
  return l;
}

// the tap offsets, and `tables` zeroed [tap][cb] tables from accl on (the next unit's first barrier publishes them)
__device__ __forceinline__ void dw_wg_init(const DwWgLds& l, const DwPlan& g, int tables) {
  const int rs = g.r * g.s;
  for (int idx = threadIdx.x; idx < rs; idx += BLOCK) l.toff[idx] = (idx / g.s) * g.halo_w + idx % g.s;
  for (int idx = threadIdx.x; idx < tables * rs * g.cb; idx += BLOCK) l.accl[idx] = 0.f;
}

// One (sample, output tile) unit added to accl: the tile loop the weight gradient, its two-term form and the squared sum
// share.  TWO: per pixel first ga * x, then ga1 * tx, into the same chain.  Begins and ends with a barrier.
template <bool AL, bool TWO>
__device__ __forceinline__ void dw_wgrad_unit(const DwWgLds& l, const float* __restrict__ ga,
                                              const float* __restrict__ ga1, const float* __restrict__ x,
                                              const float* __restrict__ tx, int64_t ld, const DwPlan& g, int ch0, int img,
                                              int tiy, int tix) {
  const int rs = g.r * g.s, cb = g.cb, qb = cb >> 2;
  const int q = threadIdx.x % qb, ps = threadIdx.x / qb, pp = BLOCK / qb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (the previous unit's readers are done; the first time: toff / accl are written)
  // the WHOLE halo and the whole 8x8 cotangent tile, zeros outside the maps: every lane then runs the same loop
  dw_stage<AL, TWO>(l.xt, x, ld, img, g.h, g.w, g.c, ch0, cb, tiy * DW_TILE * g.sh - g.ph, tix * DW_TILE * g.sw - g.pw,
                    g.halo_h, g.halo_w, g.halo_w, l.xt2, tx);
  dw_stage<AL, TWO>(l.gt, ga, g.c, img, g.oh, g.ow, g.c, ch0, cb, tiy * DW_TILE, tix * DW_TILE, DW_TILE, DW_TILE, DW_TILE,
                    l.gt2, ga1);
  __syncthreads();
  for (int tap0 = 0; tap0 < rs; tap0 += DW_TAPCH) {
    F4 acc[DW_TAPCH];
#pragma unroll
    for (int k = 0; k < DW_TAPCH; ++k) acc[k] = zero4();
    for (int o = ps; o < DW_PIX; o += pp) {
      const F4 gq = lds4(l.gt + o * cb + 4 * q);
      F4 gq1 = zero4();
      if constexpr (TWO) gq1 = lds4(l.gt2 + o * cb + 4 * q);
      const int base = (o / DW_TILE) * g.sh * g.halo_w + (o % DW_TILE) * g.sw;
#pragma unroll
      for (int k = 0; k < DW_TAPCH; ++k)
        if (tap0 + k < rs) {
          const int pix = (base + l.toff[tap0 + k]) * cb + 4 * q;
          fma4(acc[k], gq, lds4(l.xt + pix));
          if constexpr (TWO) fma4(acc[k], gq1, lds4(l.xt2 + pix));
        }
    }
    // the wave's pixel slots of one quad: lanes q, q + qb, q + 2 qb, ...
    for (int off = 32; off >= qb; off >>= 1) {
#pragma unroll
      for (int k = 0; k < DW_TAPCH; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k].e[e] += __shfl_down(acc[k].e[e], off, 64);
      }
    }
    if (lane < qb) {
#pragma unroll
      for (int k = 0; k < DW_TAPCH; ++k) *reinterpret_cast<F4*>(l.red + (wave * DW_TAPCH + k) * cb + 4 * lane) = acc[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < DW_TAPCH * qb) {
      const int k = threadIdx.x / qb, qq = threadIdx.x % qb, tap = tap0 + k;
      if (tap < rs) {
        F4 sum = lds4(l.red + k * cb + 4 * qq);
#pragma unroll
        for (int wv = 1; wv < WAVES; ++wv) {
          const F4 part = lds4(l.red + (wv * DW_TAPCH + k) * cb + 4 * qq);
#pragma unroll
          for (int e = 0; e < 4; ++e) sum.e[e] += part.e[e];
        }
        float* dst = l.accl + tap * cb + 4 * qq;
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[e] += sum.e[e];
      }
    }
    __syncthreads();
  }
}

// a [tap][cb] table to the channel block's run of a slab in parameter order, [channel][tap]
__device__ __forceinline__ void dw_store_slab(float* __restrict__ slab, const float* tab, int cbe, int cb, int rs) {
  for (int idx = threadIdx.x; idx < cbe * rs; idx += BLOCK) {
    const int chl = idx / rs, tap = idx - chl * rs;
    chain_store<DW_WT>(slab + idx, tab[tap * cb + chl]);
  }
}

// TWO: W(x, ga) + W(tx, ga1)
template <bool AL, bool TWO>
__device__ __forceinline__ void dw_wgrad(float* __restrict__ gw, const float* __restrict__ ga,
                                         const float* __restrict__ ga1, const float* __restrict__ x,
                                         const float* __restrict__ tx, int64_t ld, int64_t slab_stride, const DwPlan& g,
                                         int b) {
  const int rs = g.r * g.s, cb = g.cb;
  const int cblk = b % g.cblocks, split = b / g.cblocks;
  const int ch0 = cblk * cb, cbe = min(cb, g.c - ch0);
  const DwWgLds l = dw_wg_lds<TWO>(g);
  dw_wg_init(l, g, 1);
  const int u0 = split * g.per, u1 = min(g.units, u0 + g.per);
  for (int u = u0; u < u1; ++u)
    dw_wgrad_unit<AL, TWO>(l, ga, ga1, x, tx, ld, g, ch0, u / (g.tiles_x * g.tiles_y), (u / g.tiles_x) % g.tiles_y,
                           u % g.tiles_x);
  __syncthreads();
  dw_store_slab(gw + (int64_t)split * slab_stride + (int64_t)ch0 * rs, l.accl, cbe, cb, rs);
}

// the one grid of a backward launch: data-gradient blocks first, then (split, channel block) weight-gradient blocks
template <bool AL, bool TWO>
__global__ void __launch_bounds__(BLOCK)
k_dw_backward(float* __restrict__ dx, float* __restrict__ gw, const float* __restrict__ ga, const float* __restrict__ ga1,
              const float* __restrict__ x, const float* __restrict__ tx, int64_t ld, const float* __restrict__ W,
              const float* __restrict__ V, int64_t slab_stride, int d_blocks, const DwPlan g) {
  const int b = blockIdx.x;
  if (b < d_blocks) dw_dgrad<AL, TWO>(dx, ga, ga1, W, V, g, b);
  else dw_wgrad<AL, TWO>(gw, ga, ga1, x, tx, ld, slab_stride, g, b - d_blocks);
}

// ---- squared sum: one workgroup per (split of the samples, channel block) ----------------------------------------------
template <bool AL>
__global__ void __launch_bounds__(BLOCK)
k_dw_sqsum(float* __restrict__ out, const float* __restrict__ ga, const float* __restrict__ x, int64_t ld, float pre,
           int64_t slab_stride, const DwPlan g) {
  const int rs = g.r * g.s, cb = g.cb, tiles = g.tiles_y * g.tiles_x;
  const int cblk = blockIdx.x % g.cblocks, split = blockIdx.x / g.cblocks;
  const int ch0 = cblk * cb, cbe = min(cb, g.c - ch0);
  const DwWgLds l = dw_wg_lds<false>(g);
  float* sq = l.accl + rs * cb;  // [tap][cb]: the split's sum of squares
  dw_wg_init(l, g, 2);
  const int i0 = split * g.per, i1 = min(g.n, i0 + g.per);
  for (int img = i0; img < i1; ++img) {
    for (int t = 0; t < tiles; ++t)
      dw_wgrad_unit<AL, false>(l, ga, nullptr, x, nullptr, ld, g, ch0, img, t / g.tiles_x, t % g.tiles_x);
    // the sample boundary (the unit's last barrier stands behind its additions; the next unit's first one, or the one
    // below, behind these): each entry by the one lane that owns it
    for (int idx = threadIdx.x; idx < rs * cb; idx += BLOCK) {
      const float t = l.accl[idx] * pre;
      sq[idx] += t * t;
      l.accl[idx] = 0.f;
    }
  }
  __syncthreads();
  dw_store_slab(out + (int64_t)split * slab_stride + (int64_t)ch0 * rs, sq, cbe, cb, rs);
}

// The backward launch of both forms.  terms == 1: ga1, tx and V are NULL; dx may be NULL (W is then not read).
int dw_backward_launch(int terms, void* dx, void* gw_slabs, const void* ga, const void* ga1, const void* x, const void* tx,
                       int64_t act_ld, const void* W, const void* V, int64_t n, int64_t h, int64_t w, int64_t c, int64_t r,
                       int64_t s, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int splits_w,
                       int64_t slab_stride, int dtype, void* stream) {
  DwPlan p;
  if (dw_plan(n, h, w, c, r, s, stride_h, stride_w, pad_h, pad_w, terms, 0, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !gw_slabs || !ga || !x) return HF_ERR_ARG;
  if (terms == 2 && (!dx || !ga1 || !tx || !W || !V)) return HF_ERR_ARG;
  if (dx && !W) return HF_ERR_ARG;
  if (splits_w != p.splits_w) return HF_ERR_ARG;
  if (splits_w > 1 && slab_stride < c * r * s) return HF_ERR_ARG;
  if (act_ld == 0) act_ld = c;
  if (act_ld < c) return HF_ERR_ARG;
  const bool al = quad_ok(x, act_ld) && aligned16(ga) && (!dx || aligned16(dx)) &&
                  (terms == 1 || (quad_ok(tx, act_ld) && aligned16(ga1)));
  const int d_blocks = dx ? p.n * p.dtiles_y * p.dtiles_x * p.cblocks : 0;
  const unsigned grid = (unsigned)(d_blocks + p.cblocks * p.splits_w);
  int64_t lds = dw_lds_wgrad(p, terms);
  if (dx && dw_lds_dgrad(p, terms) > lds) lds = dw_lds_dgrad(p, terms);
  hipStream_t st = (hipStream_t)stream;
#define HF_DW_B(AL, TWO)                                                                                               \
  k_dw_backward<AL, TWO><<<grid, BLOCK, (size_t)lds, st>>>(                                                            \
      (float*)dx, (float*)gw_slabs, (const float*)ga, (const float*)ga1, (const float*)x, (const float*)tx, act_ld,    \
      (const float*)W, (const float*)V, slab_stride, d_blocks, p)
  if (terms == 2) {
    if (al) HF_DW_B(true, true);
    else HF_DW_B(false, true);
  } else {
    if (al) HF_DW_B(true, false);
    else HF_DW_B(false, false);
  }
#undef HF_DW_B
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int hf_dwconv2d_nhwc_plan(int64_t n, int64_t h, int64_t w, int64_t c, int64_t r, int64_t s, int64_t stride_h,
                          int64_t stride_w, int64_t pad_h, int64_t pad_w) {
  DwPlan p;
  if (dw_plan(n, h, w, c, r, s, stride_h, stride_w, pad_h, pad_w, 1, 0, &p) != HF_OK) return HF_ERR_ARG;
  return p.splits_w;
}

int hf_dwconv2d_nhwc_plan2(int64_t n, int64_t h, int64_t w, int64_t c, int64_t r, int64_t s, int64_t stride_h,
                           int64_t stride_w, int64_t pad_h, int64_t pad_w) {
  DwPlan p;
  if (dw_plan(n, h, w, c, r, s, stride_h, stride_w, pad_h, pad_w, 2, 0, &p) != HF_OK) return HF_ERR_ARG;
  return p.splits_w;
}

int hf_dwconv2d_nhwc_sqsum_plan(int64_t n, int64_t h, int64_t w, int64_t c, int64_t r, int64_t s, int64_t stride_h,
                                int64_t stride_w, int64_t pad_h, int64_t pad_w, int target_blocks) {
  DwPlan p;
  if (dw_plan(n, h, w, c, r, s, stride_h, stride_w, pad_h, pad_w, DW_SQSUM, target_blocks, &p) != HF_OK) return HF_ERR_ARG;
  return p.splits_w;
}

int hf_dwconv2d_nhwc_tangent(void* out, const void* t_x, const void* x, int64_t act_ld, const void* W, const void* V,
                             int64_t n, int64_t h, int64_t w, int64_t c, int64_t r, int64_t s, int64_t stride_h,
                             int64_t stride_w, int64_t pad_h, int64_t pad_w, int dtype, void* stream) {
  DwPlan p;
  if (dw_plan(n, h, w, c, r, s, stride_h, stride_w, pad_h, pad_w, 1, 0, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out) return HF_ERR_ARG;
  if (!t_x && !V) return HF_ERR_ARG;  // nothing to compute
  if ((t_x && !W) || (V && !x)) return HF_ERR_ARG;
  if (act_ld == 0) act_ld = c;
  if (act_ld < c) return HF_ERR_ARG;
  const bool al = aligned16(out) && (!t_x || quad_ok(t_x, act_ld)) && (!V || quad_ok(x, act_ld));
  const int mode = (t_x && V) ? 0 : (t_x ? 1 : 2);
  const unsigned grid = (unsigned)((int64_t)p.n * p.tiles_y * p.tiles_x * p.cblocks);
  const size_t lds = (size_t)dw_lds_tangent(p, mode == 0 ? 2 : 1);
  hipStream_t st = (hipStream_t)stream;
#define HF_DW_T(AL, MODE)                                                                                              \
  k_dw_tangent<AL, MODE><<<grid, BLOCK, lds, st>>>((float*)out, (const float*)t_x, (const float*)x, act_ld,          \
                                                    (const float*)W, (const float*)V, p)
  if (al) {
    if (mode == 0) HF_DW_T(true, 0);
    else if (mode == 1) HF_DW_T(true, 1);
    else HF_DW_T(true, 2);
  } else {
    if (mode == 0) HF_DW_T(false, 0);
    else if (mode == 1) HF_DW_T(false, 1);
    else HF_DW_T(false, 2);
  }
#undef HF_DW_T
  return (int)hipGetLastError();
}

int hf_dwconv2d_nhwc_backward_slabs(void* dx, void* gw_slabs, const void* ga, const void* x, int64_t act_ld, const void* W,
                                    int64_t n, int64_t h, int64_t w, int64_t c, int64_t r, int64_t s, int64_t stride_h,
                                    int64_t stride_w, int64_t pad_h, int64_t pad_w, int splits_w, int64_t slab_stride,
                                    int dtype, void* stream) {
  return dw_backward_launch(1, dx, gw_slabs, ga, nullptr, x, nullptr, act_ld, W, nullptr, n, h, w, c, r, s, stride_h,
                            stride_w, pad_h, pad_w, splits_w, slab_stride, dtype, stream);
}

int hf_dwconv2d_nhwc_backward2_slabs(void* dx, void* gw_slabs, const void* ga_t, const void* ga, const void* x,
                                     const void* t_x, int64_t act_ld, const void* W, const void* V, int64_t n, int64_t h,
                                     int64_t w, int64_t c, int64_t r, int64_t s, int64_t stride_h, int64_t stride_w,
                                     int64_t pad_h, int64_t pad_w, int splits_w, int64_t slab_stride, int dtype,
                                     void* stream) {
  return dw_backward_launch(2, dx, gw_slabs, ga_t, ga, x, t_x, act_ld, W, V, n, h, w, c, r, s, stride_h, stride_w, pad_h,
                            pad_w, splits_w, slab_stride, dtype, stream);
}

int hf_dwconv2d_nhwc_sqsum_slabs(void* out, const void* ga, const void* x, int64_t act_ld, int64_t n, int64_t h, int64_t w,
                                 int64_t c, int64_t r, int64_t s, int64_t stride_h, int64_t stride_w, int64_t pad_h,
                                 int64_t pad_w, float pre, int splits, int64_t slab_stride, int dtype, void* stream) {
  DwPlan p;
  if (dw_plan(n, h, w, c, r, s, stride_h, stride_w, pad_h, pad_w, DW_SQSUM, 0, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out || !ga || !x) return HF_ERR_ARG;
  if (!(pre - pre == 0.f)) return HF_ERR_ARG;  // (NaN / infinity)
  if (splits < 1 || splits > n) return HF_ERR_ARG;
  const int per = (int)((n + splits - 1) / splits);
  if ((int64_t)(splits - 1) * per >= n) return HF_ERR_ARG;  // (an empty split)
  if (splits > 1 && slab_stride < c * r * s) return HF_ERR_ARG;
  if (act_ld == 0) act_ld = c;
  if (act_ld < c) return HF_ERR_ARG;
  p.per = per, p.splits_w = splits;
  const unsigned grid = (unsigned)((int64_t)p.cblocks * splits);
  const size_t lds = (size_t)dw_lds_wgrad(p, 1, true);
  hipStream_t st = (hipStream_t)stream;
  if (quad_ok(x, act_ld) && aligned16(ga))
    k_dw_sqsum<true><<<grid, BLOCK, lds, st>>>((float*)out, (const float*)ga, (const float*)x, act_ld, pre, slab_stride, p);
  else
    k_dw_sqsum<false><<<grid, BLOCK, lds, st>>>((float*)out, (const float*)ga, (const float*)x, act_ld, pre, slab_stride, p);
  return (int)hipGetLastError();
}

}  // extern "C"
