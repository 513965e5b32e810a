// hf_conv.hip -- implicit-GEMM convolution kernels for the curvature product's conv
// layers on SMALL feature maps (gfx950, fp32 MFMA, NHWC), deterministic split-K.
//
// Why these exist.  A GGN product of a ResNet-18 on 28x28 inputs runs 48 convolutions
// (tangent, data-gradient and weight-gradient of 16 layers) whose GEMM view has a tiny
// M (N*OH*OW = 32..1568 rows) and a long K (9*Cin up to 4608).  The only way to fill
// 256 CUs is to split K.  MIOpen's kernels do that with a zero-fill launch in front
// and atomic accumulation: 48 extra launches per product (16 % of the GPU time) and a
// product that is not bitwise repeatable.  Here every K-split writes its partial tile
// to a workspace and the LAST workgroup to arrive at a tile (ticket counter) sums the
// partials in split order: one launch, no zero-fill, no float atomics, bitwise
// deterministic.  Taps of the kernel window that can never meet data (3x3 kernels on
// 1x1 / 2x2 maps) are dropped on the host, so such layers cost what a GEMM costs.
//
// Three directions, all "activation rows gathered on the fly" (implicit im2col):
//   F  out[m=(n,oh,ow)][k]  = sum_{tap,c} X[n, oh*s-p+r, ow*s-p+q][c] * Wt[k][tap][c]
//   D  dX [m=(n,ih,iw)][c]  = sum_{tap,k} dY[n,(ih+p-r)/s,(iw+p-q)/s][k] * WT[c][tap][k]
//   W  dW [k][tap][c]       = sum_{m}     dY[m][k] * X[pix(m,tap)][c]
// F and D are one kernel (operands contiguous along the reduction index: "NT"); W reduces
// over the rows ("TN").  v_mfma_f32_32x32x2_f32, 64x64 block tiles, 4 waves of 32x32,
// BK = 32, double-buffered LDS, a hand-counted register ring of global loads in front of it: three steps deep in
// the NT body and in the 128-wide configurations, two deep in the 64x64 TN body, whose loop is software-pipelined
// (pipelined_share).  Measured per wave on MI355X (profiles/r19_conv_step_attribution.json): ~4 us of waiting in
// front of the first MFMA whatever the step count (kernel arguments, then the first operands), then ~0.55 us per
// step, 0.43 us of it the sixteen dependent MFMAs.
//
// MFMA operand maps (cdna_hip_programming.md section 3): lane l supplies A[i=l&31][k=l>>5],
// B[k=l>>5][j=l&31]; C/D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
// The 32 k of a step are assigned as k = 16*(l>>5) + step (A and B alike), so that a lane's
// 16 operands are 64 contiguous bytes of an LDS row.

#include "hf_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CT = 256;            // threads per block
#ifndef HF_CONV_BK
#define HF_CONV_BK 32
#endif
constexpr int MAX_TAPS = 64;
#ifndef HF_CONV_FLAT96
#define HF_CONV_FLAT96 1  // (A/B knob of round 5: 0 builds without the 96 x 128 weight-gradient configuration)
#endif
#ifndef HF_DCLASS_NOSPLIT
#define HF_DCLASS_NOSPLIT 1
#endif
#ifndef HF_FLAT96_MIN_WORK
#define HF_FLAT96_MIN_WORK 2048  // (tiles x K-steps from which a weight gradient takes Flat96; A/B: 6144 = the Big rule)
#endif

// Tile configuration: 4 waves as WM x WN, each wave owns TM x TN MFMA tiles of 32x32 (block tile
// 32*WM*TM x 32*WN*TN), BK reduction elements per step.  Three configurations are built:
//   Small (2x2 waves, 1x1 tiles, BK 32): 64x64 -- the latency-bound small-map problems of the ResNet-18
//     product (a few K-steps per workgroup; BK = 64 measured the same);
//   Big   (2x2 waves, 2x2 tiles, BK 16): 128x128, four accumulators per wave -- problems with thousands
//     of GEMM rows (All-CNN-C, ResNet-50-size maps), where the 64x64 kernel is issue-bound: per K-step
//     it feeds 16 MFMAs per wave from 2+2 staged float4 per thread, this one 32 MFMAs from the same 2+2;
//   Big96 (4x1 waves, 1x3 tiles, BK 16): 128x96 -- the same for column counts that are multiples of 96
//     (All-CNN-C's 96 / 192 channels would waste a quarter of every 128-wide tile).  Staged like Big
//     (128 LDS rows per operand, the last 32 of B unused).
// All stage 2 + 2 float4 per thread and step, so the hand-counted prefetch ring below is shared.
template <int WM_, int WN_, int TM_, int TN_, int BK_>
struct Cfg {
  static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_, BK = BK_;
  static constexpr int BM = 32 * WM * TM, BN = 32 * WN * TN;
  static constexpr int SM = (BM + 63) / 64 * 64, SN = (BN + 63) / 64 * 64;  // staged rows / columns per operand
  static constexpr int KQ = BK / 4;          // float4 per row of a k-contiguous tile
  static constexpr int RPT = CT / KQ;        // NT: rows covered per pass of the staging threads
  static constexpr int HK = BK / 2;          // k per lane half
  static constexpr int LDK = BK + 4;         // NT: LDS row stride (floats): 16-B aligned, conflict-free b128 reads
  static constexpr int LDA = SM + 4, LDB = SN + 4;  // TN: LDS row strides
  static constexpr int NT_FLOATS = 2 * (SM + SN) * LDK;
  static constexpr int TN_FLOATS = 2 * BK * (LDA + LDB);
  static constexpr int LDS_FLOATS = (NT_FLOATS > TN_FLOATS ? NT_FLOATS : TN_FLOATS) + 4;  // + the last-arriver flag
  static_assert(WM * WN == 4, "four waves");
  static_assert(SM / RPT == 2 && SN / RPT == 2, "the hand-counted prefetch ring assumes 2 + 2 loads per step (NT)");
  static_assert(SM == SN, "both operands are staged at the same width");
  static_assert(LDS_FLOATS * 4 <= 64 * 1024, "static LDS limit");
};
typedef Cfg<2, 2, 1, 1, HF_CONV_BK> Small;
typedef Cfg<2, 2, 2, 2, 16> Big;
typedef Cfg<4, 1, 1, 3, 16> Big96;
// Flat96 (1x4 waves, 3x1 tiles, BK 16): 96 x 128 -- WEIGHT GRADIENTS whose dY channel count is a multiple of 96
// (All-CNN-C's 96 / 192): the 96 output rows fill the tile exactly, and the output COLUMNS are enumerated flat over
// (kernel tap, input channel) -- dW[k][tap][c] is one contiguous [k][taps * c] matrix when every tap is live -- so a
// 128-wide column tile may straddle taps (each staging thread keeps its own tap) and only the last of the
// ceil(taps * c / 128) tiles is partial: 9 x 96 = 864 columns fill 96.4 % of seven tiles, where the per-tap
// enumeration of the other configurations fills 75 % (128 x 96 rows x columns for 96 x 96).  Staged like Big.
typedef Cfg<1, 4, 3, 1, 16> Flat96;

// Division by a launch constant as multiply-high + shift (Granlund-Montgomery, n < 2^31): the host fills
// (mul, shift) per divisor.  The prologue of a convolution workgroup decodes its tile, its K range and the
// (n, y, x) of its staged rows with ~12 divisions by runtime values; as emulated 32-bit divisions (~35 VALU
// instructions each, the uniform ones included: there is no scalar divide) they were ~40 % of the ~800
// instructions in front of the first load of launches that take 7-10 us in all.
struct FastDiv {
  unsigned mul, shift;
};
__host__ __device__ __forceinline__ unsigned fdiv(unsigned n, FastDiv f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (__umulhi(n, f.mul) + n) >> f.shift;
#else
  return (unsigned)((((unsigned long long)n * f.mul) >> 32) + n) >> f.shift;
#endif
}

struct ConvArgs {
  const float* src;    // gathered activations (F: X, D: dY, W: X)
  const float* mat;    // F: Wt [Nout][RS][Cs]; D: WT [Nout][RS][Cs]; W: dY [M][Kout]
  float* out;
  float* ws;           // split-K partial tiles
  int* tickets;        // one counter per output tile, zero between launches
  int dgrad;           // gather rule: 0 = forward window, 1 = transposed (data gradient)
  // geometry of the gathered tensor and of the row index space
  int rows;            // M: F: N*OH*OW, D: N*H*W, W: N*OH*OW
  int rh, rw;          // spatial extent the row index decodes over (F/W: OH,OW; D: H,W)
  int sh_, sw_;        // spatial extent of the gathered tensor (F/W: H,W; D: OH,OW)
  int cs, cs_ld;       // channels gathered per pixel, pixel stride of src
  int mat_ld;          // NT: floats between consecutive taps of `mat` (>= cs: `mat` may be the first-channels
                       //     slice of a wider [Nout][RS][mat_ld] buffer -- the W half of a [W | v_W] operand)
  int nout, ldc;       // output columns (F: K, D: C, W: unused), output row stride
  int kout;            // W: number of dY channels (output rows of dW)
  int R, S, stride_h, stride_w, pad_h, pad_w;
  int ntaps;           // live taps
  // live taps as (r | s << 8).  DWORDS on purpose: a dynamically indexed BYTE array in the kernel arguments
  // compiles to global_load_ubyte + s_waitcnt vmcnt(0) (gfx950 has no scalar byte load), which drained the
  // three-deep prefetch ring at every step; a dword is one s_load on the scalar (lgkm) counter
  int tap_rs[MAX_TAPS];
  int tiles_m, tiles_n, splits, steps;  // steps = reduction steps in total
  int scalar;          // 1: channel counts not multiples of 4 -> element-wise gathers
  int shift_h, shift_w;  // log2 of the strides when both are powers of two, else -1
  int out_c;           // W: channels of X that get an output column (<= cs: X may be zero-padded)
  int slabs;           // 1: split s writes its partial result, in the output's own layout, to
  long long slab_stride;  //    out + s*slab_stride; the CONSUMER kernel sums the slabs in its prologue
  int big;             // tile configuration this problem was set up for (0: Small, 1: Big, 2: Big96, 3: Flat96)
  // Data gradient of a STRIDED convolution, decomposed by residue class of the input pixel: pixel (y, x) only
  // receives the taps with (y + pad - r) % stride == 0, so rows are enumerated class by class ((y % sh, x % sw)
  // fixed within a row tile) and every tile loops over ITS taps only -- a stride-2 3x3 layer does 9/4 taps per
  // pixel instead of 9, of which 3/4 would gather nothing.  ncls == 0: plain enumeration.
  int ncls;
  int cls_tile0[5];    // first row tile of class i ([ncls] = tiles_m)
  int cls_tap0[5];     // taps of class i: tap_r/tap_s[cls_tap0[i] .. cls_tap0[i+1])
  int cls_h[4], cls_w[4], cls_py[4], cls_px[4];  // pixels of the class: y = y'*stride_h + py, y' < cls_h
  // launch constants as divisors (filled by seal() right before the launch)
  FastDiv fd_tiles_n, fd_tiles_m, fd_splits, fd_rw, fd_rh, fd_csteps, fd_cblocks, fd_cs;
  // BNSUM instantiations (tangent convolution in front of a TRAIN-mode BatchNorm): per-channel partial sums of this
  // workgroup's tile, sum(t) and sum(t * xhat), xhat = (bn_x - bn_mean) * bn_rstd, to row (tile_m * splits + split)
  // of bn_part_1 / bn_part_x ([tiles_m * splits][nout]) -- what the reduction launch between the convolution and the
  // elementwise pass computed (hf_chan_affine_bwd_ex with gx = NULL); the elementwise pass adds the rows up
  const float *bn_x, *bn_mean, *bn_rstd;
  float *bn_part_x, *bn_part_1;
};

// One scalar load per 64-byte line of the argument block, all in flight together, before anything else: the
// compiler loads kernel arguments where they are first used -- a chain of ~5 dependent scalar-cache misses
// (~0.5 us each) through a ~650-byte block in the prologue of launches that take 7-10 us.  After this the
// later loads hit the scalar cache.
__device__ __forceinline__ void touch_args(const ConvArgs& a) {
  const int* ka = reinterpret_cast<const int*>(&a);
  int sink = 0;
#pragma unroll
  for (unsigned l = 0; l < (sizeof(ConvArgs) + 63) / 64; ++l) {
    const unsigned w = l * 16 < sizeof(ConvArgs) / 4 ? l * 16 : (unsigned)(sizeof(ConvArgs) / 4 - 1);
    sink ^= ka[w];
  }
  asm volatile("" ::"s"(sink));
}

// Pixel index into the gathered tensor for row coordinates (n, y, x) and tap (r, q); `valid` is
// false for padding.  Branch-free on purpose (selects only): the staging loads must not sit
// behind per-lane branches, or hipcc stops pipelining them.
__device__ __forceinline__ int gather_pixel(const ConvArgs& a, int n, int y, int x, int r, int q, bool& valid) {
  int sy, sx;
  bool v = true;
  if (!a.dgrad) {  // (uniform: a scalar branch)
    sy = y * a.stride_h - a.pad_h + r;
    sx = x * a.stride_w - a.pad_w + q;
  } else {
    const int ty = y + a.pad_h - r, tx = x + a.pad_w - q;
    if (a.shift_h >= 0) { sy = ty >> a.shift_h; sx = tx >> a.shift_w; }  // power-of-two strides
    else { sy = ty / a.stride_h; sx = tx / a.stride_w; }
    v = (ty >= 0) & (tx >= 0) & (sy * a.stride_h == ty) & (sx * a.stride_w == tx);
  }
  v = v & ((unsigned)sy < (unsigned)a.sh_) & ((unsigned)sx < (unsigned)a.sw_);
  valid = v;
  return v ? (n * a.sh_ + sy) * a.sw_ + sx : 0;
}

// The forward rule alone (weight gradients gather through the forward window), for the pipelined K loop: no branch
// on the direction, and the geometry held in scalar registers for the whole loop -- read through ConvArgs the compiler
// re-loads a field from the kernel arguments wherever it is used, a scalar load and a wait inside the MFMA chain.
struct Geom {
  int sth, stw, ph, pw, sh, sw;
};
__device__ __forceinline__ void pin(int& v) { asm volatile("" : "+s"(v)); }
__device__ __forceinline__ void pin(unsigned& v) { asm volatile("" : "+s"(v)); }
__device__ __forceinline__ Geom make_geom(const ConvArgs& a) {
  Geom g = {a.stride_h, a.stride_w, a.pad_h, a.pad_w, a.sh_, a.sw_};
  pin(g.sth); pin(g.stw); pin(g.ph); pin(g.pw); pin(g.sh); pin(g.sw);
  return g;
}
__device__ __forceinline__ int gather_pixel_fwd(const Geom& g, int n, int y, int x, int r, int q, bool& valid) {
  const int sy = y * g.sth - g.ph + r, sx = x * g.stw - g.pw + q;
  const bool v = ((unsigned)sy < (unsigned)g.sh) & ((unsigned)sx < (unsigned)g.sw);
  valid = v;
  return v ? (n * g.sh + sy) * g.sw + sx : 0;
}

__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// Staging loads the compiler does not see as loads: hipcc schedules the first use of a loaded
// register right behind the load (and waits there), which serialises the three-deep prefetch
// ring below.  Issued as inline asm they stay in flight until the matching HF_WAIT_SLOT, whose
// "+v" operands tie every later use of the registers to the wait (cdna_hip_programming.md
// section 5.7: count the queue by hand).
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void gload4(f32x4& dst, const float* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
#define HF_WAIT_SLOT(N, A, B) \
  asm volatile("s_waitcnt vmcnt(" #N ")" : "+v"(A[0]), "+v"(A[1]), "+v"(B[0]), "+v"(B[1]) : : "memory")

// ---------------------------------------------------------------------------------
// K loop of the 64x64 configuration (one accumulator per wave), software-pipelined.
// ---------------------------------------------------------------------------------
// A workgroup of these launches walks 1-6 steps with ONE wave per SIMD, so whatever is not issued between the
// sixteen dependent MFMAs of a step (16 x 64 cycles) sits serially in front of them.  Here step j's MFMAs carry,
// one piece per MFMA: the wait for and the LDS stash of step j+1 (into the other buffer), the address arithmetic
// and issue of the next fetch, the step's one barrier, and step j+1's fragment reads (into the other fragment
// registers).  The register ring is RING steps deep: a share of up to RING steps has every load in flight before
// the first wait, longer shares refill a slot as soon as it is stashed.  What a wave does in front of its first wait
// is NOT hidden -- the ring's slots are filled there, dead ones included -- and the weight-gradient shares of the
// ResNet-18 product are 1-3 steps: measured (profiles/r19_tn_ring_depth.jsonl), a ring of 6 / 4 / 2 gives
// 1 638 / 1 663 / 1 689 matvecs/s against 1 656 of the three-deep plain ring, so the ring is two deep.
//   prep(live)            uniform part of the next fetch (and advance to the one after); !live: a step past the
//                         share's end -- its loads read a dummy address and are stashed as zeros, never multiplied
//   load(piece, dst)      piece 0..3 = A row 0, B row 0, A row 1, B row 1 of the staging thread: issues ONE
//                         global_load_dwordx4 (unconditionally: the queue is counted by hand) and returns its ok bit
//   stash(buf, u, a, b, ok), frag(buf, piece, av, bv): LDS writes of staged row u; a quarter of the fragment reads
// The order of additions is the plain loop's: steps ascending, MFMA 0..15 of a step on the one accumulator.
#ifndef HF_CONV_RING
#define HF_CONV_RING 2  // (A/B knob: depth of the register ring of the pipelined loop; even)
#endif
constexpr int RING = HF_CONV_RING;
#define HF_WAIT_RING(A, B)                                                              \
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(A[0]), "+v"(A[1]), "+v"(B[0]), "+v"(B[1]) \
               : [n] "n"(4 * (RING - 1)) : "memory")
#define HF_DRAIN_RING(A, B) \
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(A[0]), "+v"(A[1]), "+v"(B[0]), "+v"(B[1]) : : "memory")

template <typename Prep, typename Load, typename Stash, typename Frag>
__device__ __forceinline__ void pipelined_share(int j0, int j1, f32x16& acc, Prep&& prep, Load&& load, Stash&& stash,
                                                Frag&& frag) {
  static_assert(RING % 2 == 0 && RING >= 2 && RING <= 14,
                "LDS buffer and fragment set of a step are compile-time in the unrolled ring; vmcnt counts to 63");
  f32x4 ra[RING][2], rb[RING][2];
  unsigned ok[RING];
  float av[2][16], bv[2][16];
  if (j0 >= j1) return;
  // No control flow around a load, anywhere: the compiler does not know that the ring's registers are pending until
  // the matching wait, and a copy it places at a join of two paths would read them before the data has landed.
#pragma unroll
  for (int s = 0; s < RING; ++s) {
    prep(j0 + s < j1);
    ok[s] = load(0, ra[s][0]);
    ok[s] |= load(1, rb[s][0]);
    ok[s] |= load(2, ra[s][1]);
    ok[s] |= load(3, rb[s][1]);
  }
  HF_WAIT_RING(ra[0], rb[0]);
  stash(0, 0, ra[0][0], rb[0][0], ok[0]);
  stash(0, 1, ra[0][1], rb[0][1], ok[0]);
  prep(j0 + RING < j1);
  ok[0] = load(0, ra[0][0]);
  ok[0] |= load(1, rb[0][0]);
  ok[0] |= load(2, ra[0][1]);
  ok[0] |= load(3, rb[0][1]);
  __syncthreads();
#pragma unroll
  for (int piece = 0; piece < 4; ++piece) frag(0, piece, av[0], bv[0]);
#define HF_STEP_MFMA(K) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[p][K], bv[p][K], acc, 0, 0, 0)
#define HF_SCHED_FENCE __builtin_amdgcn_sched_barrier(0)
  for (int j = j0; j < j1; j += RING) {
#pragma unroll
    for (int s = 0; s < RING; ++s) {
      if (j + s >= j1) break;  // (uniform)
      // step j+s: fragments p, staged in LDS buffer p; next step: ring slot n, LDS buffer / fragments q.  Past the
      // share's end the "next step" is a dead slot: zeros are stashed and read, never multiplied.
      const int p = s & 1, q = p ^ 1, n = (s + 1) % RING;
      HF_SCHED_FENCE;
      HF_STEP_MFMA(0);
      HF_WAIT_RING(ra[n], rb[n]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(1);
      stash(q, 0, ra[n][0], rb[n][0], ok[n]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(2);
      stash(q, 1, ra[n][1], rb[n][1], ok[n]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(3);
      prep(j + s + 1 + RING < j1);
      unsigned k = load(0, ra[n][0]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(4);
      k |= load(1, rb[n][0]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(5);
      k |= load(2, ra[n][1]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(6);
      k |= load(3, rb[n][1]);
      ok[n] = k;
      HF_SCHED_FENCE;
      HF_STEP_MFMA(7);
      __syncthreads();
      HF_SCHED_FENCE;
      HF_STEP_MFMA(8);
      frag(q, 0, av[q], bv[q]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(9);
      frag(q, 1, av[q], bv[q]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(10);
      frag(q, 2, av[q], bv[q]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(11);
      frag(q, 3, av[q], bv[q]);
      HF_SCHED_FENCE;
      HF_STEP_MFMA(12);
      HF_STEP_MFMA(13);
      HF_STEP_MFMA(14);
      HF_STEP_MFMA(15);
      HF_SCHED_FENCE;
    }
  }
#undef HF_STEP_MFMA
#undef HF_SCHED_FENCE
#pragma unroll
  for (int s = 0; s < RING; ++s) HF_DRAIN_RING(ra[s], rb[s]);  // the registers may be reused from here on
}

// four consecutive floats of which only the first `valid` exist, no alignment assumed
// (channel counts that are not multiples of 4: the 49-tap im2col of a 1-channel stem)
__device__ __forceinline__ float4 ldg4s(const float* p, int valid) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid > 0) v.x = p[0];
  if (valid > 1) v.y = p[1];
  if (valid > 2) v.z = p[2];
  if (valid > 3) v.w = p[3];
  return v;
}

// Last-arriver reduction of the split-K partials of one block tile (fixed order).  The wave at
// (wm, wn) holds TM x TN MFMA tiles: tile (im, in) covers rows wm*32*TM + im*32 .., cols likewise.
template <typename C, bool CLS = false, bool BNSUM = false>
__device__ __forceinline__ void finish_tile(const ConvArgs& a, const f32x16 (&acc)[C::TM][C::TN], int tile, int split,
                                            int wm, int wn, int lane, float* out_tile_base,
                                            int row0, int col0, int row_lim, int col_lim, int ldc,
                                            int* flag_lds, int cls = -1, float* lds = nullptr) {
  constexpr int BM = C::BM, BN = C::BN;
  const int i = lane & 31, h = lane >> 5;
  if constexpr (BNSUM) {
    static_assert(C::TM == 1 && C::TN == 1 && !CLS, "per-tile column sums: 64x64 tiles, plain row enumeration");
    // column `col` of this tile: 2 waves (wm) x 2 lane halves (h) x 16 accumulator rows each.  Every load first
    // (the tile's xhat operand), fp64 sums per lane, the four shares combined through LDS in a fixed order.
    const int col = wn * 32 + i, gcol = col0 + col;
    const bool cok = gcol < col_lim;
    const float mu = cok ? a.bn_mean[gcol] : 0.f, rs = cok ? a.bn_rstd[gcol] : 0.f;
    float xv[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int orow = row0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      xv[reg] = (cok && orow < row_lim) ? a.bn_x[(size_t)orow * ldc + gcol] : mu;
    }
    double s1 = 0.0, sx = 0.0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int orow = row0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (cok && orow < row_lim) {
        const float v = acc[0][0][reg];
        s1 += (double)v;
        sx += (double)v * (double)(float)((xv[reg] - mu) * rs);
      }
    }
    double* red = reinterpret_cast<double*>(lds);  // [2][4][BN]; the caller synchronised after its last LDS read
    red[(0 * 4 + wm * 2 + h) * BN + col] = s1;
    red[(1 * 4 + wm * 2 + h) * BN + col] = sx;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 2 * BN) {
      const int kind = t / BN, c = t - kind * BN;
      const double sum = ((red[(kind * 4 + 0) * BN + c] + red[(kind * 4 + 1) * BN + c]) +
                          red[(kind * 4 + 2) * BN + c]) + red[(kind * 4 + 3) * BN + c];
      const int tile_m = (int)fdiv((unsigned)tile, a.fd_tiles_n);
      if (col0 + c < col_lim) {
        const float part = (float)sum;
        chain_store<HF_WT_CONV>(&(kind ? a.bn_part_x : a.bn_part_1)[(size_t)(tile_m * a.splits + split) * a.nout + col0 + c], part);
      }
    }
  }
  if (a.splits == 1 || a.slabs) {
    float* dst = out_tile_base + (a.slabs ? (size_t)split * (size_t)a.slab_stride : 0);
#pragma unroll
    for (int im = 0; im < C::TM; ++im)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = (wm * C::TM + im) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        int orow = row0 + row;  // output row (= pixel index) of this accumulator row
        bool rok = orow < row_lim;
        if (CLS && cls >= 0) {  // (uniform) class-major enumeration: row -> (n, y', x') -> pixel (n, y'*sh + py, x'*sw + px)
          const int wc = a.cls_w[cls], hc = a.cls_h[cls];
          const int xq = orow % wc, tq = orow / wc;
          const int yq = tq % hc, nq = tq / hc;
          orow = (nq * a.rh + yq * a.stride_h + a.cls_py[cls]) * a.rw + xq * a.stride_w + a.cls_px[cls];
        }
#pragma unroll
        for (int in = 0; in < C::TN; ++in) {
          const int col = (wn * C::TN + in) * 32 + i;
          // (the accumulator layout gives a lane 4 bytes per row: its natural store width)
          if (rok && col0 + col < col_lim) chain_store<HF_WT_CONV>(&dst[(size_t)orow * ldc + col0 + col], acc[im][in][reg]);
        }
      }
    return;
  }
  const int tiles = a.tiles_m * a.tiles_n;
  float* mine = a.ws + ((size_t)split * tiles + tile) * (BM * BN);
#pragma unroll
  for (int im = 0; im < C::TM; ++im)
#pragma unroll
    for (int in = 0; in < C::TN; ++in)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = (wm * C::TM + im) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const int col = (wn * C::TN + in) * 32 + i;
        // write-through (sc1) store: visible device-wide once drained, no release fence needed
        __hip_atomic_store(mine + row * BN + col, acc[im][in][reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
  // publish (cdna_hip_programming.md, in-launch split-K reduction, write-through form):
  // every wave drains its sc1 stores, ONE lane draws the ticket; the last arriver's lane 0
  // acquires once (drops stale lines), then all its waves read the slabs with plain loads
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(a.tickets + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == a.splits - 1;
    if (last) {
      __hip_atomic_store(a.tickets + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *flag_lds = last;
  }
  __syncthreads();
  if (!*flag_lds) return;
  const float* base = a.ws + (size_t)tile * (BM * BN);
  const size_t slab = (size_t)tiles * (BM * BN);
  for (int e = threadIdx.x; e < BM * BN / 4; e += CT) {
    float4 s = *reinterpret_cast<const float4*>(base + 4 * e);
    int sp = 1;
    for (; sp + 4 <= a.splits; sp += 4) {  // four slabs in flight, summed in split order
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(base + (sp + u) * slab + 4 * e);
#pragma unroll
      for (int u = 0; u < 4; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
    }
    for (; sp < a.splits; ++sp) {
      const float4 v = *reinterpret_cast<const float4*>(base + sp * slab + 4 * e);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const int row = (4 * e) / BN, col = (4 * e) % BN;
    if (row0 + row < row_lim) {
      float* o = out_tile_base + (size_t)(row0 + row) * ldc + col0 + col;
      const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (col0 + col + c < col_lim) o[c] = v[c];
    }
  }
}

// ---------------------------------------------------------------------------------
// NT kernel: F and D.   out[m][j] = sum_{tap, c} src[pix(m,tap)][c] * mat[j][tap][c]
// ---------------------------------------------------------------------------------
// CLS: the instantiation that understands the residue-class enumeration of strided data gradients (ConvArgs::ncls);
// the plain one keeps the prologue of the latency-bound small-map launches short (+1 us per launch otherwise).
template <bool SCALAR, typename C, bool CLS = false, bool BNSUM = false>
__device__ __forceinline__ void conv_nt_body(const ConvArgs& a, float* lds, int bid) {
  constexpr int BM = C::BM, BN = C::BN, BK = C::BK, KQ = C::KQ, RPT = C::RPT, HK = C::HK, LDK = C::LDK;
  constexpr int NU = 2;
  constexpr int SM = C::SM, SN = C::SN;
  float (*As)[SM][LDK] = reinterpret_cast<float (*)[SM][LDK]>(lds);
  float (*Bs)[SN][LDK] = reinterpret_cast<float (*)[SN][LDK]>(lds + 2 * SM * LDK);
  int& flag = *reinterpret_cast<int*>(lds + C::LDS_FLOATS - 4);
  touch_args(a);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave / C::WN, wn = wave % C::WN;
  const int bq = (int)fdiv((unsigned)bid, a.fd_tiles_n), tile_n = bid - bq * a.tiles_n;
  const int split = (int)fdiv((unsigned)bq, a.fd_tiles_m), tile_m = bq - split * a.tiles_m;
  const int tile = tile_m * a.tiles_n + tile_n;
  const int csteps = (a.cs + BK - 1) / BK;
  // residue class of this row tile (strided data gradients, see ConvArgs): its rows, taps and step count
  int cls = -1, row_base = tile_m * BM, rows_c = a.rows, tap0 = 0, steps = a.steps;
  if (CLS && a.ncls > 0) {  // (uniform)
    cls = 0;
    while (cls + 1 < a.ncls && tile_m >= a.cls_tile0[cls + 1]) ++cls;
    row_base = (tile_m - a.cls_tile0[cls]) * BM;
    rows_c = (a.rows / (a.rh * a.rw)) * a.cls_h[cls] * a.cls_w[cls];  // images x pixels of the class
    tap0 = a.cls_tap0[cls];
    steps = (a.cls_tap0[cls + 1] - tap0) * csteps;
  }
  const int per = (int)fdiv((unsigned)(steps + a.splits - 1), a.fd_splits);
  const int j0 = split * per < steps ? split * per : steps, j1 = (j0 + per < steps) ? j0 + per : steps;

  // staging assignment: thread -> rows lr + RPT*u and the float4 at k offset 4*kq
  const int lr = t / KQ, kq = t % KQ;
  int rn[NU], ry[NU], rx[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int m = row_base + lr + RPT * u;
    if (m < rows_c) {
      if (CLS && cls >= 0) {
        const int wc = a.cls_w[cls], hc = a.cls_h[cls];
        const int xx = m % wc, tq = m / wc;
        rx[u] = xx * a.stride_w + a.cls_px[cls]; ry[u] = (tq % hc) * a.stride_h + a.cls_py[cls]; rn[u] = tq / hc;
      } else {
        const int tq = (int)fdiv((unsigned)m, a.fd_rw), xx = m - tq * a.rw;
        rn[u] = (int)fdiv((unsigned)tq, a.fd_rh);
        rx[u] = xx; ry[u] = tq - rn[u] * a.rh;
      }
    } else {
      rn[u] = -1; ry[u] = rx[u] = 0;
    }
  }
  const int RS = a.R * a.S;
  const float* brow[NU];
  bool bok[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int j = tile_n * BN + lr + RPT * u;
    bok[u] = (j < a.nout) & (lr + RPT * u < BN);  // (rows past BN belong to the next column tile)
    brow[u] = a.mat + (size_t)(bok[u] ? j : 0) * RS * a.mat_ld;
  }

  // Global -> register -> LDS staging with THREE steps of loads in flight: these kernels run
  // one or two workgroups per CU on operands that the previous launch has just written (cold
  // in this XCD's L2), so a step is bound by the ~2 us round trip unless several are
  // outstanding.  LDS stays double-buffered; the register ring is three deep.
  // (loads are issued UNCONDITIONALLY -- an out-of-range element reads a valid dummy address
  // and is zeroed when the registers are written to LDS: a branch around a load makes hipcc
  // drain the whole queue, vmcnt(0), before the next use; cdna_hip_programming.md trap 4c)
  auto fetch = [&](int step, float4 (&ra)[NU], float4 (&rb)[NU]) -> unsigned {
    const int tl = step / csteps, c = (step - tl * csteps) * BK + 4 * kq, ti = tap0 + tl;
    const int rs_ = a.tap_rs[ti], r = rs_ & 255, q = rs_ >> 8;
    const bool cok = c < a.cs;
    unsigned ok = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      bool va;
      const int pix = gather_pixel(a, rn[u], ry[u], rx[u], r, q, va);
      va = va & cok & (rn[u] >= 0);
      const bool vb = cok & bok[u];
      const float* pa = a.src + (va ? (size_t)pix * a.cs_ld + c : 0);
      const float* pb = vb ? brow[u] + (size_t)(r * a.S + q) * a.mat_ld + c : a.mat;
      ra[u] = ldg4s(pa, va ? a.cs - c : 0);
      rb[u] = ldg4s(pb, vb ? a.cs - c : 0);
      ok |= (va ? 1u : 0u) << (2 * u) | (vb ? 2u : 0u) << (2 * u);
    }
    return ok;
  };
  auto stash = [&](int buf, const float4 (&ra)[NU], const float4 (&rb)[NU], unsigned ok) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      *reinterpret_cast<float4*>(&As[buf][lr + RPT * u][4 * kq]) = (ok >> (2 * u)) & 1u ? ra[u] : zero;
      *reinterpret_cast<float4*>(&Bs[buf][lr + RPT * u][4 * kq]) = (ok >> (2 * u)) & 2u ? rb[u] : zero;
    }
  };

  f32x16 acc[C::TM][C::TN];
#pragma unroll
  for (int im = 0; im < C::TM; ++im)
#pragma unroll
    for (int in = 0; in < C::TN; ++in)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[im][in][r] = 0.f;
  const int i = lane & 31, h = lane >> 5;
  auto compute = [&](int cur) {
    float av[C::TM][HK], bv[C::TN][HK];
#pragma unroll
    for (int im = 0; im < C::TM; ++im) {
      const float* ap = &As[cur][(wm * C::TM + im) * 32 + i][HK * h];
#pragma unroll
      for (int v = 0; v < HK / 4; ++v)
        *reinterpret_cast<float4*>(av[im] + 4 * v) = *reinterpret_cast<const float4*>(ap + 4 * v);
    }
#pragma unroll
    for (int in = 0; in < C::TN; ++in) {
      const float* bp = &Bs[cur][(wn * C::TN + in) * 32 + i][HK * h];
#pragma unroll
      for (int v = 0; v < HK / 4; ++v)
        *reinterpret_cast<float4*>(bv[in] + 4 * v) = *reinterpret_cast<const float4*>(bp + 4 * v);
    }
#pragma unroll
    for (int s = 0; s < HK; ++s)
#pragma unroll
      for (int im = 0; im < C::TM; ++im)
#pragma unroll
        for (int in = 0; in < C::TN; ++in)
          acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[im][s], bv[in][s], acc[im][in], 0, 0, 0);
  };
  const int jl = j1 - 1;
  int cur = 0;
  if (!SCALAR) {
    // hand-counted ring: always three steps (12 loads) in flight; steps beyond the split's range
    // re-fetch step j1-1 and are never written to LDS, so the count at every wait is 8
    // steps are fetched in increasing order (the clamped re-fetches at the end repeat the last
    // one): the (tap, channel block) of the next fetch is kept incrementally -- no division per step
    int f_step = j0, f_ti = (int)fdiv((unsigned)j0, a.fd_csteps), f_cb = j0 - f_ti * csteps;
    // the tap table entry of the NEXT tap is loaded when a tap begins: the scalar load (a dynamic index into
    // the kernel arguments) has a whole tap's steps to land instead of stalling the step that needs it
    auto tap_at = [&](int ti) { return a.tap_rs[ti < MAX_TAPS ? ti : MAX_TAPS - 1]; };
    int f_rs = tap_at(tap0 + f_ti), f_rs_next = tap_at(tap0 + f_ti + 1);
    auto fetch_v = [&](int step, f32x4 (&ra)[NU], f32x4 (&rb)[NU]) -> unsigned {
      if (step > f_step) {  // (uniform; steps advance by one)
        f_step = step;
        if (++f_cb == csteps) {
          f_cb = 0;
          ++f_ti;
          f_rs = f_rs_next;
          f_rs_next = tap_at(tap0 + f_ti + 1);
        }
      }
      const int c = f_cb * BK + 4 * kq;
      const int rs_ = f_rs, r = rs_ & 255, q = rs_ >> 8;
      const bool cok = c < a.cs;
      unsigned ok = 0;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        bool va;
        const int pix = gather_pixel(a, rn[u], ry[u], rx[u], r, q, va);
        va = va & cok & (rn[u] >= 0);
        const bool vb = cok & bok[u];
        gload4(ra[u], a.src + (va ? (size_t)pix * a.cs_ld + c : 0));
        gload4(rb[u], vb ? brow[u] + (size_t)(r * a.S + q) * a.mat_ld + c : a.mat);
        ok |= (va ? 1u : 0u) << (2 * u) | (vb ? 2u : 0u) << (2 * u);
      }
      return ok;
    };
    auto stash_v = [&](int buf, const f32x4 (&ra)[NU], const f32x4 (&rb)[NU], unsigned ok) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        *reinterpret_cast<f32x4*>(&As[buf][lr + RPT * u][4 * kq]) = (ok >> (2 * u)) & 1u ? ra[u] : zero;
        *reinterpret_cast<f32x4*>(&Bs[buf][lr + RPT * u][4 * kq]) = (ok >> (2 * u)) & 2u ? rb[u] : zero;
      }
    };
    f32x4 a0[NU], b0[NU], a1[NU], b1[NU], a2[NU], b2[NU];
    unsigned k0 = 0, k1 = 0, k2 = 0;
    if (j0 < j1) {
      k0 = fetch_v(j0, a0, b0);
      k1 = fetch_v(j0 + 1 < j1 ? j0 + 1 : jl, a1, b1);
      k2 = fetch_v(j0 + 2 < j1 ? j0 + 2 : jl, a2, b2);
      for (int j = j0; j < j1; j += 3) {
        HF_WAIT_SLOT(8, a0, b0);
        stash_v(cur, a0, b0, k0);
        __syncthreads();
        k0 = fetch_v(j + 3 < j1 ? j + 3 : jl, a0, b0);
        compute(cur);
        cur ^= 1;
        HF_WAIT_SLOT(8, a1, b1);
        if (j + 1 < j1) {
          stash_v(cur, a1, b1, k1);
          __syncthreads();
          compute(cur);
          cur ^= 1;
        }
        k1 = fetch_v(j + 4 < j1 ? j + 4 : jl, a1, b1);
        HF_WAIT_SLOT(8, a2, b2);
        if (j + 2 < j1) {
          stash_v(cur, a2, b2, k2);
          __syncthreads();
          compute(cur);
          cur ^= 1;
        }
        k2 = fetch_v(j + 5 < j1 ? j + 5 : jl, a2, b2);
      }
      HF_WAIT_SLOT(0, a0, b0);  // drain: the registers may be reused from here on
      HF_WAIT_SLOT(0, a1, b1);
      HF_WAIT_SLOT(0, a2, b2);
    }
  } else {
    float4 a0[NU], b0[NU];
    for (int j = j0; j < j1; ++j) {  // element-wise gathers: plain one-step loop
      const unsigned k0 = fetch(j, a0, b0);
      stash(cur, a0, b0, k0);
      __syncthreads();
      compute(cur);
      cur ^= 1;
    }
  }
  __syncthreads();  // the LDS array is reused below (last-arriver flag)
  finish_tile<C, CLS, BNSUM>(a, acc, tile, split, wm, wn, lane, a.out, row_base, tile_n * BN, rows_c, a.nout, a.ldc,
                             &flag, cls, lds);
}

// ---------------------------------------------------------------------------------
// TN kernel: W.   dW[k][tap][c] = sum_m dY[m][k] * X[pix(m,tap)][c]
//   tile_m over k (dY channels), tile_n over (live tap, BN-channel block of X)
// ---------------------------------------------------------------------------------
// FLAT: the output columns are enumerated flat over (tap, channel) (see Flat96): column tile tile_n covers the
// flattened columns [tile_n * BN, ...), every staging thread decodes the tap of ITS column quad once.
// PIPE: the pipelined K loop (64x64 tiles); the launches that mix tile configurations (ANYBIG) keep the plain ring
// for their 64x64 problems, and with it the register count their 128-wide problems' occupancy depends on.
template <bool SCALAR, typename C, bool FLAT = false, bool PIPE = true>
__device__ __forceinline__ void conv_tn_body(const ConvArgs& a, float* lds, int bid) {
  constexpr int BM = C::BM, BN = C::BN, BK = C::BK, HK = C::HK, LDA = C::LDA, LDB = C::LDB;
  float (*As)[BK][LDA] = reinterpret_cast<float (*)[BK][LDA]>(lds);
  float (*Bs)[BK][LDB] = reinterpret_cast<float (*)[BK][LDB]>(lds + 2 * BK * LDA);
  int& flag = *reinterpret_cast<int*>(lds + C::LDS_FLOATS - 4);
  touch_args(a);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave / C::WN, wn = wave % C::WN;
  const int bq = (int)fdiv((unsigned)bid, a.fd_tiles_n), tile_n = bid - bq * a.tiles_n;
  const int split = (int)fdiv((unsigned)bq, a.fd_tiles_m), tile_m = bq - split * a.tiles_m;
  const int tile = tile_m * a.tiles_n + tile_n;
  const int per = (int)fdiv((unsigned)(a.steps + a.splits - 1), a.fd_splits);
  const int j0 = split * per, j1 = (j0 + per < a.steps) ? j0 + per : a.steps;

  const int cblocks = (a.cs + BN - 1) / BN;
  int ti, c0;
  if constexpr (FLAT) { ti = 0; c0 = tile_n * BN; }
  else { ti = (int)fdiv((unsigned)tile_n, a.fd_cblocks); c0 = (tile_n - ti * cblocks) * BN; }

  // staging: thread -> rows kr, kr + RP of the step and the float4 at column 4*cq
  constexpr int CQ = C::SM / 4;     // float4 per staged row (both operands are staged SM == SN wide)
  constexpr int RP = CT / CQ;       // rows per pass
  constexpr int TU = BK / RP;       // passes
  static_assert(TU == 2, "the hand-counted prefetch ring assumes 2 + 2 loads per step (TN)");
  const int kr = t / CQ, cq = t % CQ;
  const int ka = tile_m * BM + 4 * cq;  // dY channel
  int cb = c0 + 4 * cq;                 // X channel
  bool bkok = (cb < a.cs) & (4 * cq < BN);
  if constexpr (FLAT) {                 // (flattened column -> this thread's tap and channel; quads never straddle taps)
    const int jq = c0 + 4 * cq;
    bkok = (jq < a.ntaps * a.cs) & (4 * cq < BN);
    ti = bkok ? (int)fdiv((unsigned)jq, a.fd_cs) : 0;
    cb = jq - ti * a.cs;
  }
  const int rs_ = a.tap_rs[ti], r = rs_ & 255, q = rs_ >> 8;
  const bool aok = (ka < a.kout) & (4 * cq < BM);

  auto fetch = [&](int step, float4 (&ra)[TU], float4 (&rb)[TU]) -> unsigned {
    unsigned ok = 0;
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      const int m = step * BK + kr + RP * u;
      const bool mok = m < a.rows;
      const int mm = mok ? m : 0;
      const int xx = mm % a.rw, tq = mm / a.rw;
      bool vb;
      const int pix = gather_pixel(a, tq / a.rh, tq % a.rh, xx, r, q, vb);
      vb = vb & mok & bkok;
      const bool va = mok & aok;
      const float* pa = a.mat + (va ? (size_t)m * a.kout + ka : 0);
      const float* pb = a.src + (vb ? (size_t)pix * a.cs_ld + cb : 0);
      ra[u] = ldg4s(pa, va ? a.kout - ka : 0);
      rb[u] = ldg4s(pb, vb ? a.cs - cb : 0);
      ok |= (va ? 1u : 0u) << (2 * u) | (vb ? 2u : 0u) << (2 * u);
    }
    return ok;
  };
  auto stash = [&](int buf, const float4 (&ra)[TU], const float4 (&rb)[TU], unsigned ok) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      *reinterpret_cast<float4*>(&As[buf][kr + RP * u][4 * cq]) = (ok >> (2 * u)) & 1u ? ra[u] : zero;
      *reinterpret_cast<float4*>(&Bs[buf][kr + RP * u][4 * cq]) = (ok >> (2 * u)) & 2u ? rb[u] : zero;
    }
  };

  f32x16 acc[C::TM][C::TN];
#pragma unroll
  for (int im = 0; im < C::TM; ++im)
#pragma unroll
    for (int in = 0; in < C::TN; ++in)
#pragma unroll
      for (int x = 0; x < 16; ++x) acc[im][in][x] = 0.f;
  const int i = lane & 31, h = lane >> 5;
  auto compute = [&](int cur) {
    float av[C::TM][HK], bv[C::TN][HK];
#pragma unroll
    for (int s = 0; s < HK; ++s) {
#pragma unroll
      for (int im = 0; im < C::TM; ++im) av[im][s] = As[cur][HK * h + s][(wm * C::TM + im) * 32 + i];
#pragma unroll
      for (int in = 0; in < C::TN; ++in) bv[in][s] = Bs[cur][HK * h + s][(wn * C::TN + in) * 32 + i];
    }
#pragma unroll
    for (int s = 0; s < HK; ++s)
#pragma unroll
      for (int im = 0; im < C::TM; ++im)
#pragma unroll
        for (int in = 0; in < C::TN; ++in)
          acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[im][s], bv[in][s], acc[im][in], 0, 0, 0);
  };
  const int jl = j1 - 1;
  int cur = 0;
  if constexpr (!SCALAR && PIPE && C::TM * C::TN == 1 && !FLAT) {
    // 64x64 tiles: the pipelined loop (pipelined_share).  (n, y, x) of a staged row comes from two multiply-high
    // divisions per load -- branch-free, where the incremental form below walks rw-sized strides in a per-lane loop
    // (32 trips per step on a 1x1 map, in front of the loads it feeds)
    const Geom g = make_geom(a);
    int g_rows = a.rows, g_kout = a.kout, g_cs_ld = a.cs_ld, g_rw = a.rw, g_rh = a.rh;
    pin(g_rows); pin(g_kout); pin(g_cs_ld); pin(g_rw); pin(g_rh);
    FastDiv g_frw = a.fd_rw, g_frh = a.fd_rh;
    pin(g_frw.mul); pin(g_frw.shift); pin(g_frh.mul); pin(g_frh.shift);
    const float *g_src = a.src, *g_mat = a.mat;
    int f_m0 = j0 * BK + kr;
    int p_m0 = 0;
    bool p_live = false;
    auto prep = [&](bool live) {
      p_m0 = f_m0;
      p_live = live;
      f_m0 += BK;
    };
    auto load = [&](int piece, f32x4& dst) -> unsigned {
      const int u = piece >> 1;
      const int m = p_m0 + RP * u;
      const bool mok = (m < g_rows) & p_live;
      if (!(piece & 1)) {
        const bool va = mok & aok;
        gload4(dst, g_mat + (va ? (size_t)m * g_kout + ka : 0));
        return (va ? 1u : 0u) << (2 * u);
      }
      const int mm = mok ? m : 0;
      const int tq = (int)fdiv((unsigned)mm, g_frw), xx = mm - tq * g_rw;
      const int nn = (int)fdiv((unsigned)tq, g_frh), yy = tq - nn * g_rh;
      bool vb;
      const int pix = gather_pixel_fwd(g, nn, yy, xx, r, q, vb);
      vb = vb & mok & bkok;
      gload4(dst, g_src + (vb ? (size_t)pix * g_cs_ld + cb : 0));
      return (vb ? 2u : 0u) << (2 * u);
    };
    auto stash_u = [&](int buf, int u, const f32x4& ra, const f32x4& rb, unsigned ok) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(&As[buf][kr + RP * u][4 * cq]) = (ok >> (2 * u)) & 1u ? ra : zero;
      *reinterpret_cast<f32x4*>(&Bs[buf][kr + RP * u][4 * cq]) = (ok >> (2 * u)) & 2u ? rb : zero;
    };
    auto frag = [&](int buf, int piece, float (&av)[HK], float (&bv)[HK]) {
      static_assert(HK == 16, "four fragment pieces of eight elements each");
      const int s0 = 8 * (piece & 1);
#pragma unroll
      for (int s = s0; s < s0 + 8; ++s) {
        if (piece < 2) av[s] = As[buf][HK * h + s][wm * 32 + i];
        else bv[s] = Bs[buf][HK * h + s][wn * 32 + i];
      }
    };
    pipelined_share(j0, j1, acc[0][0], prep, load, stash_u, frag);
  } else if (!SCALAR) {
    // the rows of consecutive steps advance by BK: (n, y, x) of each staged row is kept
    // incrementally (the per-step divisions were ~300 VALU instructions per thread and step)
    int f_step = j0, fn_[TU], fy_[TU], fx_[TU];
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      const int m = j0 * BK + kr + RP * u;
      const int tq = (int)fdiv((unsigned)m, a.fd_rw), xx = m - tq * a.rw;
      fn_[u] = (int)fdiv((unsigned)tq, a.fd_rh);
      fx_[u] = xx; fy_[u] = tq - fn_[u] * a.rh;
    }
    auto fetch_v = [&](int step, f32x4 (&ra)[TU], f32x4 (&rb)[TU]) -> unsigned {
      if (step > f_step) {  // (uniform; steps advance by one)
        f_step = step;
#pragma unroll
        for (int u = 0; u < TU; ++u) {
          fx_[u] += BK;
          while (fx_[u] >= a.rw) { fx_[u] -= a.rw; if (++fy_[u] == a.rh) { fy_[u] = 0; ++fn_[u]; } }
        }
      }
      unsigned ok = 0;
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        const int m = step * BK + kr + RP * u;
        const bool mok = m < a.rows;
        bool vb;
        const int pix = gather_pixel(a, fn_[u], fy_[u], fx_[u], r, q, vb);
        vb = vb & mok & bkok;
        const bool va = mok & aok;
        gload4(ra[u], a.mat + (va ? (size_t)m * a.kout + ka : 0));
        gload4(rb[u], a.src + (vb ? (size_t)pix * a.cs_ld + cb : 0));
        ok |= (va ? 1u : 0u) << (2 * u) | (vb ? 2u : 0u) << (2 * u);
      }
      return ok;
    };
    auto stash_v = [&](int buf, const f32x4 (&ra)[TU], const f32x4 (&rb)[TU], unsigned ok) {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < TU; ++u) {
        *reinterpret_cast<f32x4*>(&As[buf][kr + RP * u][4 * cq]) = (ok >> (2 * u)) & 1u ? ra[u] : zero;
        *reinterpret_cast<f32x4*>(&Bs[buf][kr + RP * u][4 * cq]) = (ok >> (2 * u)) & 2u ? rb[u] : zero;
      }
    };
    f32x4 a0[TU], b0[TU], a1[TU], b1[TU], a2[TU], b2[TU];
    unsigned k0 = 0, k1 = 0, k2 = 0;
    if (j0 < j1) {
      k0 = fetch_v(j0, a0, b0);
      k1 = fetch_v(j0 + 1 < j1 ? j0 + 1 : jl, a1, b1);
      k2 = fetch_v(j0 + 2 < j1 ? j0 + 2 : jl, a2, b2);
      for (int j = j0; j < j1; j += 3) {
        HF_WAIT_SLOT(8, a0, b0);
        stash_v(cur, a0, b0, k0);
        __syncthreads();
        k0 = fetch_v(j + 3 < j1 ? j + 3 : jl, a0, b0);
        compute(cur);
        cur ^= 1;
        HF_WAIT_SLOT(8, a1, b1);
        if (j + 1 < j1) {
          stash_v(cur, a1, b1, k1);
          __syncthreads();
          compute(cur);
          cur ^= 1;
        }
        k1 = fetch_v(j + 4 < j1 ? j + 4 : jl, a1, b1);
        HF_WAIT_SLOT(8, a2, b2);
        if (j + 2 < j1) {
          stash_v(cur, a2, b2, k2);
          __syncthreads();
          compute(cur);
          cur ^= 1;
        }
        k2 = fetch_v(j + 5 < j1 ? j + 5 : jl, a2, b2);
      }
      HF_WAIT_SLOT(0, a0, b0);
      HF_WAIT_SLOT(0, a1, b1);
      HF_WAIT_SLOT(0, a2, b2);
    }
  } else {
    float4 a0[TU], b0[TU];
    for (int j = j0; j < j1; ++j) {
      const unsigned k0 = fetch(j, a0, b0);
      stash(cur, a0, b0, k0);
      __syncthreads();
      compute(cur);
      cur ^= 1;
    }
  }
  __syncthreads();
  // output element (k, tap, c) at (k*RS + tap)*cs + c: rows = k, "columns" = c within this tap
  if constexpr (FLAT) {
    // every tap live and out_c == cs: the columns ARE the flattened (tap, c) index.  A zero-padded operand
    // (out_c < cs) is only let through with a single tap (apply_out_c): the columns are then the channels, and the
    // padded ones are cut off here -- with several taps they would land in the next tap's / row's first entries
    finish_tile<C>(a, acc, tile, split, wm, wn, lane, a.out, tile_m * BM, c0, a.kout,
                   a.ntaps == 1 ? a.out_c : a.ntaps * a.cs, a.R * a.S * a.out_c, &flag);
  } else {
    float* base = a.out + (size_t)(r * a.S + q) * a.out_c;
    finish_tile<C>(a, acc, tile, split, wm, wn, lane, base, tile_m * BM, c0, a.kout, a.out_c,
                   a.R * a.S * a.out_c, &flag);
  }
}

// ---------------------------------------------------------------------------------
// Squared-sum sibling of the TN kernel (hf_conv2d_nhwc_sqsum_slabs):
//   out[k][tap][c] = sum_i ( pre * sum_{m in sample i} dY[m][k] * X[pix(m,tap)][c] )^2
// ---------------------------------------------------------------------------------
// The tile, the staging map, the LDS layout and the epilogue (finish_tile in slab mode) are conv_tn_body's in the 64x64
// configuration; what differs is the reduction.  The splits run over SAMPLES: split s takes samples
// [s*per, min(n, (s+1)*per)) and walks them as GROUPS of rows, each in ceil(glen / BK) steps whose staged rows are masked
// on the GROUP's end (a group's last step is partial whenever glen % BK != 0, so no step ever mixes two groups):
//   per-sample form (OUTER = false, P = oh*ow > 1): a group is one sample's P rows.  After its last step
//     t = acc * pre (one rounding), sq += t * t (two roundings), acc = 0: 16 more accumulator registers per wave.
//   squared-operand form (OUTER = true, P == 1): the per-sample gradient is the outer product dY_i[k] * X_i[c], so the
//     share is ONE group of rows with both operands squared after the load (one rounding each) and the result
//     acc * (pre * pre).
// The loop is the plain one with one step of loads in flight (the next step's loads are issued in front of this step's
// MFMAs); LDS is double-buffered with one barrier per step.
struct SqArgs {
  float pre;
  int n, P, per;  // samples, rows per sample, samples per split
};

template <bool SCALAR, bool OUTER>
__device__ __forceinline__ void conv_tn_sq_body(const ConvArgs& a, const SqArgs q, float* lds, int bid) {
  typedef Small C;
  constexpr int BM = C::BM, BN = C::BN, BK = C::BK, HK = C::HK, LDA = C::LDA, LDB = C::LDB;
  float (*As)[BK][LDA] = reinterpret_cast<float (*)[BK][LDA]>(lds);
  float (*Bs)[BK][LDB] = reinterpret_cast<float (*)[BK][LDB]>(lds + 2 * BK * LDA);
  int& flag = *reinterpret_cast<int*>(lds + C::LDS_FLOATS - 4);
  touch_args(a);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave / C::WN, wn = wave % C::WN;
  const int bq = (int)fdiv((unsigned)bid, a.fd_tiles_n), tile_n = bid - bq * a.tiles_n;
  const int split = (int)fdiv((unsigned)bq, a.fd_tiles_m), tile_m = bq - split * a.tiles_m;
  const int tile = tile_m * a.tiles_n + tile_n;
  const int s0 = split * q.per < q.n ? split * q.per : q.n, s1 = s0 + q.per < q.n ? s0 + q.per : q.n;
  const int glen = OUTER ? s1 - s0 : q.P, ngroups = OUTER ? (s1 > s0 ? 1 : 0) : s1 - s0;
  const int gsteps = (glen + BK - 1) / BK, total = ngroups * gsteps;

  const int cblocks = (a.cs + BN - 1) / BN;
  const int ti = (int)fdiv((unsigned)tile_n, a.fd_cblocks), c0 = (tile_n - ti * cblocks) * BN;
  constexpr int CQ = C::SM / 4, RP = CT / CQ, TU = BK / RP;
  const int kr = t / CQ, cq = t % CQ;
  const int ka = tile_m * BM + 4 * cq;  // dY channel
  const int cb = c0 + 4 * cq;           // X channel
  const bool bkok = (cb < a.cs) & (4 * cq < BN);
  const int rs_ = a.tap_rs[ti], r = rs_ & 255, tq_ = rs_ >> 8;
  const bool aok = (ka < a.kout) & (4 * cq < BM);

  // step jj of group gi: rows base + jj*BK + kr + RP*u, those past the group's end masked
  auto fetch = [&](int gi, int jj, float4 (&ra)[TU], float4 (&rb)[TU]) -> unsigned {
    const int base = OUTER ? s0 : (s0 + gi) * q.P;
    unsigned ok = 0;
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      const int local = jj * BK + kr + RP * u;
      const bool mok = local < glen;
      const int m = mok ? base + local : 0;
      const int tq = (int)fdiv((unsigned)m, a.fd_rw), xx = m - tq * a.rw;
      const int nn = (int)fdiv((unsigned)tq, a.fd_rh), yy = tq - nn * a.rh;
      bool vb;
      const int pix = gather_pixel(a, nn, yy, xx, r, tq_, vb);
      vb = vb & mok & bkok;
      const bool va = mok & aok;
      const float* pa = a.mat + (va ? (size_t)m * a.kout + ka : 0);
      const float* pb = a.src + (vb ? (size_t)pix * a.cs_ld + cb : 0);
      if (SCALAR) {
        ra[u] = ldg4s(pa, va ? a.kout - ka : 0);
        rb[u] = ldg4s(pb, vb ? a.cs - cb : 0);
      } else {  // (unconditional: a masked element reads a valid dummy address and is stashed as zero)
        ra[u] = ldg4(pa);
        rb[u] = ldg4(pb);
      }
      ok |= (va ? 1u : 0u) << (2 * u) | (vb ? 2u : 0u) << (2 * u);
    }
    return ok;
  };
  auto sqr = [](const float4& v) { return OUTER ? make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w) : v; };
  auto stash = [&](int buf, const float4 (&ra)[TU], const float4 (&rb)[TU], unsigned ok) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      *reinterpret_cast<float4*>(&As[buf][kr + RP * u][4 * cq]) = (ok >> (2 * u)) & 1u ? sqr(ra[u]) : zero;
      *reinterpret_cast<float4*>(&Bs[buf][kr + RP * u][4 * cq]) = (ok >> (2 * u)) & 2u ? sqr(rb[u]) : zero;
    }
  };

  f32x16 acc, sq[1][1];
#pragma unroll
  for (int x = 0; x < 16; ++x) acc[x] = sq[0][0][x] = 0.f;
  const int i = lane & 31, h = lane >> 5;
  auto compute = [&](int cur) {
    float av[HK], bv[HK];
#pragma unroll
    for (int s = 0; s < HK; ++s) {
      av[s] = As[cur][HK * h + s][wm * 32 + i];
      bv[s] = Bs[cur][HK * h + s][wn * 32 + i];
    }
#pragma unroll
    for (int s = 0; s < HK; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
  };
  const float pre2 = q.pre * q.pre;
  float4 ra[TU], rb[TU];
  unsigned ok = 0;
  int fg = 0, fj = 0;  // (group, step) of the loads in flight
  int cj = 0, cur = 0;
  if (total > 0) ok = fetch(0, 0, ra, rb);
  for (int st = 0; st < total; ++st) {
    stash(cur, ra, rb, ok);
    __syncthreads();
    if (st + 1 < total) {  // (uniform) -- the last step re-fetches itself: loaded, never stashed
      if (++fj == gsteps) { fj = 0; ++fg; }
    }
    ok = fetch(fg, fj, ra, rb);
    compute(cur);
    cur ^= 1;
    if (++cj == gsteps) {  // (uniform) the group's last step
      cj = 0;
#pragma unroll
      for (int x = 0; x < 16; ++x) {
        if (OUTER) {
          sq[0][0][x] = acc[x] * pre2;
        } else {
          const float tt = acc[x] * q.pre;
          sq[0][0][x] += tt * tt;
          acc[x] = 0.f;
        }
      }
    }
  }
  __syncthreads();
  float* base = a.out + (size_t)(r * a.S + tq_) * a.out_c;
  finish_tile<C>(a, sq, tile, split, wm, wn, lane, base, tile_m * BM, c0, a.kout, a.out_c, a.R * a.S * a.out_c, &flag);
}

template <bool SCALAR, bool OUTER>
__global__ __launch_bounds__(CT) void k_conv_tn_sq(const ConvArgs a, const SqArgs q) {
  __shared__ __attribute__((aligned(16))) float lds[Small::LDS_FLOATS];
  conv_tn_sq_body<SCALAR, OUTER>(a, q, lds, blockIdx.x);
}

template <bool SCALAR, typename C, bool CLS = false, bool BNSUM = false>
__global__ __launch_bounds__(CT) void k_conv_nt(const ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[C::LDS_FLOATS];
  conv_nt_body<SCALAR, C, CLS, BNSUM>(a, lds, blockIdx.x);
}

// A forward / tangent convolution whose launch CARRIES the tangent sweep's weight scatter (hf_unpack_weights) as
// extra workgroups behind its own: the stem's convolution does not read any scattered operand (its v_W is a slice
// of the vector itself), the scatter only has to land before the NEXT launch -- as one launch the 14 us scatter
// hides behind the 12 us latency-bound convolution (they were 26 us in sequence).
template <bool SCALAR, typename C>
__global__ __launch_bounds__(CT) void k_conv_nt_unpack(const ConvArgs a, const hf_shared::UnpackArgs u,
                                                       const float* __restrict__ usrc, int conv_blocks) {
  __shared__ __attribute__((aligned(16))) float lds[C::LDS_FLOATS];
  if ((int)blockIdx.x < conv_blocks) conv_nt_body<SCALAR, C, false>(a, lds, blockIdx.x);
  else hf_shared::unpack_block<float>(usrc, u, blockIdx.x - (unsigned)conv_blocks);
}

template <bool SCALAR, typename C, bool FLAT = false>
__global__ __launch_bounds__(CT) void k_conv_tn(const ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[C::LDS_FLOATS];
  conv_tn_body<SCALAR, C, FLAT>(a, lds, blockIdx.x);
}

// Data gradient AND weight gradient of one layer in ONE launch: both read the same dY,
// neither depends on the other; the first `nblocks_d` workgroups run the NT body.
// ANYBIG: some problem of the launch runs in the Big configuration (decided per problem, `a.big`); the
// all-Small instantiation keeps the register allocation of the small-map launches what it was.
template <bool ANYBIG, bool CLS = false>
__global__ __launch_bounds__(CT) void k_conv_dw(const ConvArgs d, const ConvArgs w, int nblocks_d) {
  constexpr int LDSB = Big::LDS_FLOATS > Big96::LDS_FLOATS ? Big::LDS_FLOATS : Big96::LDS_FLOATS;
  constexpr int LDSF = ANYBIG ? (LDSB > Small::LDS_FLOATS ? LDSB : Small::LDS_FLOATS) : Small::LDS_FLOATS;
  __shared__ __attribute__((aligned(16))) float lds[LDSF];
  if ((int)blockIdx.x < nblocks_d) {
    if (ANYBIG && d.big == 1) conv_nt_body<false, Big, CLS>(d, lds, blockIdx.x);
    else if (ANYBIG && d.big == 2) conv_nt_body<false, Big96, CLS>(d, lds, blockIdx.x);
    else conv_nt_body<false, Small, CLS>(d, lds, blockIdx.x);
  } else {
    if (ANYBIG && w.big == 1) conv_tn_body<false, Big>(w, lds, blockIdx.x - nblocks_d);
    else if (ANYBIG && w.big == 2) conv_tn_body<false, Big96>(w, lds, blockIdx.x - nblocks_d);
    else if (ANYBIG && w.big == 3) conv_tn_body<false, Flat96, true>(w, lds, blockIdx.x - nblocks_d);
    else conv_tn_body<false, Small, false, !ANYBIG>(w, lds, blockIdx.x - nblocks_d);
  }
}

// Up to GROUP_MAX independent convolutions (any mix of directions) in ONE launch: workgroups
// [start[p], start[p+1]) run problem p.  The curvature engine uses it where two layers read the
// same tensor (a residual block's first convolution and its downsample branch): one launch for
// both tangent convolutions, one for both layers' data + weight gradients.
constexpr int GROUP_MAX = 4;
// (the problems arrive as SEPARATE by-value arguments: indexing an array of them inside one by-value
// struct made hipcc copy all 1.2 KB to scratch memory, and every field read in the K loops a scratch
// load -- measured 3x on the 128-wide configurations)
struct GroupMeta {
  int tn[GROUP_MAX];       // 1: weight gradient (TN body), 0: forward / data gradient (NT body)
  int start[GROUP_MAX + 1];
  int n;
};

template <bool ANYBIG, bool CLS, bool BNSUM = false>
__device__ __forceinline__ void group_run(const ConvArgs& a, int tn, float* lds, int local) {
  if constexpr (BNSUM) {  // (tangent convolutions on 64x64 tiles only: checked on the host)
    if (a.bn_part_1) conv_nt_body<false, Small, false, true>(a, lds, local);
    else conv_nt_body<false, Small, false, false>(a, lds, local);
    return;
  }
  if (tn) {
    if (ANYBIG && a.big == 1) conv_tn_body<false, Big>(a, lds, local);
    else if (ANYBIG && a.big == 2) conv_tn_body<false, Big96>(a, lds, local);
    else if (ANYBIG && a.big == 3) conv_tn_body<false, Flat96, true>(a, lds, local);
    else conv_tn_body<false, Small, false, !ANYBIG>(a, lds, local);
  } else {
    if (ANYBIG && a.big == 1) conv_nt_body<false, Big, CLS>(a, lds, local);
    else if (ANYBIG && a.big == 2) conv_nt_body<false, Big96, CLS>(a, lds, local);
    else conv_nt_body<false, Small, CLS>(a, lds, local);
  }
}

template <bool ANYBIG, bool CLS = false, bool BNSUM = false>
__global__ __launch_bounds__(CT) void k_conv_group(const ConvArgs a0, const ConvArgs a1, const ConvArgs a2,
                                                   const ConvArgs a3, const GroupMeta m) {
  constexpr int LDSB = Big::LDS_FLOATS > Big96::LDS_FLOATS ? Big::LDS_FLOATS : Big96::LDS_FLOATS;
  constexpr int LDSF = ANYBIG ? (LDSB > Small::LDS_FLOATS ? LDSB : Small::LDS_FLOATS) : Small::LDS_FLOATS;
  __shared__ __attribute__((aligned(16))) float lds[LDSF];
  const int b = (int)blockIdx.x;
  if (b < m.start[1]) group_run<ANYBIG, CLS, BNSUM>(a0, m.tn[0], lds, b);
  else if (b < m.start[2]) group_run<ANYBIG, CLS, BNSUM>(a1, m.tn[1], lds, b - m.start[1]);
  else if (b < m.start[3]) group_run<ANYBIG, CLS, BNSUM>(a2, m.tn[2], lds, b - m.start[2]);
  else group_run<ANYBIG, CLS, BNSUM>(a3, m.tn[3], lds, b - m.start[3]);
}

}  // namespace

namespace {

// Number of K-splits.  target_blocks > 0: split until about that many workgroups exist
// (>= 2 steps per split).  Otherwise a cost model in microseconds: a split run pays ~3 us to
// publish and collect tickets plus ~0.15 us per slab the last arriver sums; workgroups beyond
// two per CU queue.  Its per-step term (0.6 + 0.014 * BK: ~1.0 us at BK = 32) dates from the
// one-step prefetch and is kept because the split counts it yields are pinned
// (tests/golden/conv_plan.npz); behind the register rings a wave's step was measured at ~0.55 us
// at BK = 32 (0.43 us of it MFMA), in front of a fixed ~4 us wait for the kernel arguments and
// the first operands (profiles/r19_conv_step_attribution.json).
#ifndef HF_BIG_TARGET_BLOCKS
#define HF_BIG_TARGET_BLOCKS 512  // (whole-bench A/B, profiles/r05_big_target_blocks_ab*.jsonl: 256 / 384 / 512 / 768 / 1024 ->
#endif                            //  configs[3] 576 / 579 / 601 / 582 / 544, All-CNN-C GGN 761 / 782 / 817 / 817 / 754)
#ifndef HF_BIG_MIN_WORK
#define HF_BIG_MIN_WORK 6144  // (output tiles x K-steps from which a problem takes a 128-wide configuration)
#endif
constexpr int64_t BIG_TARGET_BLOCKS = HF_BIG_TARGET_BLOCKS;  // workgroups a 128-wide launch is split towards (measured: below)
constexpr int64_t FEW_TILES = 8;            // up to this many output tiles ...
constexpr int64_t FEW_TILES_CAP = 96;       // ... a weight gradient may be split this deep (default measured on ResNet-18)

int choose_splits(int64_t tiles, int64_t steps, int target_blocks, int64_t ws_bytes, bool slabs = false,
                  int bk = Small::BK, int64_t tile_elems = Small::BM * Small::BN) {
  int64_t best = 1;
  if (slabs && target_blocks <= 0) {
    // no in-launch reduction: a split costs its consumer one more read per element; split
    // until one workgroup per CU exists (measured in the ResNet-18 product: 256 beats 384,
    // 512 and 768 -- the prefetch ring keeps a workgroup with several steps busy) or a split
    // is down to 2 steps
    // The 128-wide configurations (bk == 16) run one MFMA-heavy workgroup per CU at 256: a second and
    // third resident workgroup fill the matrix pipe while the first stages its next tile (measured on
    // the All-CNN-C shapes, scripts/conv_kernel_bench.py --big 1: 256 / 512 / 768 workgroups ->
    // tangent 76 / 93 / 99, data gradient 68 / 83 / 87, weight gradient 39 / 52 / 65 TFLOP/s stand-alone.  INSIDE the
    // product every further split is one more slab for the consumer kernel to read, and a Hessian product runs a
    // second launch on a parallel graph branch: the whole bench prefers 512 to 768 -- HF_BIG_TARGET_BLOCKS)
    const bool big = bk != Small::BK;
    best = ((big ? BIG_TARGET_BLOCKS : 256) + tiles - 1) / tiles;
    if (big && best > steps / 8) best = steps / 8;  // (>= 8 steps per workgroup)
    if (best > steps / 2) best = steps / 2;
    // (one or two output tiles -- the stem's weight gradient: 6272 rows into a 64 x 52 matrix --
    // would leave most of the chip idle at 32 splits)
    // (FEW_TILES: up to how many output tiles the larger cap applies.  Measured, round 4,
    // profiles/r04_conv_few_tiles.jsonl: 2 / 4 / 8 tiles -> ResNet-50 topology 314 / 323 / 323 matvecs/s,
    // ResNet-18 1507 / 1512 / 1507, All-CNN-C 742 / 751 / 755.)
    const int64_t cap = tiles <= FEW_TILES ? FEW_TILES_CAP : (big ? 128 : 32);
    if (best > cap) best = cap;
    if (best < 1) best = 1;
    while (best > 1 && ((steps + best - 1) / best) * (best - 1) >= steps) --best;
    return (int)best;
  }
  if (target_blocks > 0) {
    best = (target_blocks + tiles - 1) / tiles;
    if (best > steps / 2) best = steps / 2;
    if (best < 1) best = 1;
  } else {
    double best_cost = 1e30;
    const int64_t cap = steps < 64 ? steps : 64;
    for (int64_t sp = 1; sp <= cap; ++sp) {
      const int64_t per = (steps + sp - 1) / sp;
      if (sp > 1 && per * (sp - 1) >= steps) continue;  // would leave a split empty
      const double rounds = (double)(tiles * sp) / 512.0;
      double cost = (0.6 + 0.014 * bk) * (double)per * (rounds > 1.0 ? rounds : 1.0);
      if (sp > 1) cost += 3.0 + 0.15 * (double)sp;
      if (cost < best_cost - 1e-9) { best_cost = cost; best = sp; }
    }
  }
  while (!slabs && best > 1 && best * tiles * tile_elems * (int64_t)sizeof(float) > ws_bytes) --best;
  while (best > 1 && ((steps + best - 1) / best) * (best - 1) >= steps) --best;
  return (int)best;
}

FastDiv make_fastdiv(int64_t d) {
  if (d < 1) d = 1;
  unsigned l = 0;
  while ((1LL << l) < d) ++l;  // ceil(log2 d)
  FastDiv f;
  f.mul = (unsigned)((((unsigned long long)((1ULL << l) - (unsigned long long)d)) << 32) / (unsigned long long)d + 1);
  f.shift = l;
  return f;
}

// the divisors of the kernels' prologues (see FastDiv); called on the copy that is handed to the launch
void seal(ConvArgs& a) {
  const int bk = a.big ? Big::BK : Small::BK;
  const int bn = a.big == 1 ? Big::BN : a.big == 2 ? Big96::BN : Small::BN;
  a.fd_tiles_n = make_fastdiv(a.tiles_n);
  a.fd_tiles_m = make_fastdiv(a.tiles_m);
  a.fd_splits = make_fastdiv(a.splits);
  a.fd_rw = make_fastdiv(a.rw);
  a.fd_rh = make_fastdiv(a.rh);
  a.fd_csteps = make_fastdiv((a.cs + bk - 1) / bk);
  a.fd_cblocks = make_fastdiv((a.cs + bn - 1) / bn);
  a.fd_cs = make_fastdiv(a.cs);
}

// ---- one launcher per kernel family: each seals its copies and owns the choice of the instantiation ----
void launch_one(int direction, const ConvArgs& a_in, int64_t blocks, hipStream_t stream) {
  ConvArgs a = a_in;
  seal(a);
  const dim3 grid((unsigned)blocks), block(CT);
  if (direction <= 1) {
    if (a.scalar) hipLaunchKernelGGL((k_conv_nt<true, Small>), grid, block, 0, stream, a);
    else if (a.ncls > 0 && a.big == 1) hipLaunchKernelGGL((k_conv_nt<false, Big, true>), grid, block, 0, stream, a);
    else if (a.ncls > 0 && a.big == 2) hipLaunchKernelGGL((k_conv_nt<false, Big96, true>), grid, block, 0, stream, a);
    else if (a.ncls > 0) hipLaunchKernelGGL((k_conv_nt<false, Small, true>), grid, block, 0, stream, a);
    else if (a.big == 1) hipLaunchKernelGGL((k_conv_nt<false, Big>), grid, block, 0, stream, a);
    else if (a.big == 2) hipLaunchKernelGGL((k_conv_nt<false, Big96>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_conv_nt<false, Small>), grid, block, 0, stream, a);
  } else {
    if (a.scalar) hipLaunchKernelGGL((k_conv_tn<true, Small>), grid, block, 0, stream, a);
    else if (a.big == 1) hipLaunchKernelGGL((k_conv_tn<false, Big>), grid, block, 0, stream, a);
    else if (a.big == 2) hipLaunchKernelGGL((k_conv_tn<false, Big96>), grid, block, 0, stream, a);
    else if (a.big == 3) hipLaunchKernelGGL((k_conv_tn<false, Flat96, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_conv_tn<false, Small>), grid, block, 0, stream, a);
  }
}

void launch_dw(const ConvArgs& d_in, const ConvArgs& w_in, int64_t bd, int64_t bw, hipStream_t stream) {
  ConvArgs d = d_in, w = w_in;
  seal(d);
  seal(w);
  const dim3 grid((unsigned)(bd + bw)), block(CT);
  const bool big = d.big || w.big, cls = d.ncls > 0;
  if (big && cls) hipLaunchKernelGGL((k_conv_dw<true, true>), grid, block, 0, stream, d, w, (int)bd);
  else if (big) hipLaunchKernelGGL((k_conv_dw<true, false>), grid, block, 0, stream, d, w, (int)bd);
  else if (cls) hipLaunchKernelGGL((k_conv_dw<false, true>), grid, block, 0, stream, d, w, (int)bd);
  else hipLaunchKernelGGL((k_conv_dw<false, false>), grid, block, 0, stream, d, w, (int)bd);
}

// (64x64 tiles, no residue classes: the planner has refused everything else)
void launch_unpack(const ConvArgs& a_in, int64_t blocks, const hf_shared::UnpackArgs& u, const float* usrc,
                   int ublocks, hipStream_t stream) {
  ConvArgs a = a_in;
  seal(a);
  const dim3 grid((unsigned)(blocks + ublocks)), block(CT);
  if (a.scalar) hipLaunchKernelGGL((k_conv_nt_unpack<true, Small>), grid, block, 0, stream, a, u, usrc, (int)blocks);
  else hipLaunchKernelGGL((k_conv_nt_unpack<false, Small>), grid, block, 0, stream, a, u, usrc, (int)blocks);
}

// Problem i of a grouped launch takes the next `blocks` workgroups (`m` zeroed before the first; the unused slots
// stay empty ranges at the end).
int group_add(GroupMeta& m, int i, bool tn, int64_t blocks) {
  const int64_t end = m.start[i] + blocks;
  if (end > 0x7fffffffLL) return HF_ERR_ARG;
  m.tn[i] = tn;
  for (int j = i + 1; j <= GROUP_MAX; ++j) m.start[j] = (int)end;
  m.n = i + 1;
  return HF_OK;
}

// `a`: GROUP_MAX problems, those from m.n on zeroed.  bnsum: the instantiations whose epilogue writes the BatchNorm
// partial sums (tangent convolutions on 64x64 tiles only: the planner has refused everything else).
void launch_group(ConvArgs (&a)[GROUP_MAX], const GroupMeta& m, bool bnsum, hipStream_t st) {
  bool big = false, cls = false;
  for (int i = 0; i < m.n; ++i) {
    big = big || a[i].big;
    cls = cls || a[i].ncls > 0;
    seal(a[i]);
  }
  const dim3 grid((unsigned)m.start[GROUP_MAX]), block(CT);
  if (bnsum && m.n == 1 && a[0].bn_part_1)
    hipLaunchKernelGGL((k_conv_nt<false, Small, false, true>), grid, block, 0, st, a[0]);
  else if (bnsum) hipLaunchKernelGGL((k_conv_group<false, false, true>), grid, block, 0, st, a[0], a[1], a[2], a[3], m);
  else if (big && cls) hipLaunchKernelGGL((k_conv_group<true, true>), grid, block, 0, st, a[0], a[1], a[2], a[3], m);
  else if (big) hipLaunchKernelGGL((k_conv_group<true, false>), grid, block, 0, st, a[0], a[1], a[2], a[3], m);
  else if (cls) hipLaunchKernelGGL((k_conv_group<false, true>), grid, block, 0, st, a[0], a[1], a[2], a[3], m);
  else hipLaunchKernelGGL((k_conv_group<false, false>), grid, block, 0, st, a[0], a[1], a[2], a[3], m);
}

// Which tile configuration a problem runs in: a pure function of its geometry.  Big (128x128) needs both output
// dimensions to fill most of a tile and enough GEMM rows that the 64x64 kernel would be issue-bound.
int want_big(int direction, int64_t rows, int64_t dim_m, int64_t dim_n, int64_t red, int64_t mult, bool scalar,
             bool all_taps = false, bool slab_mode = false) {
  // dim_m x dim_n: the output matrix (NT: rows x nout; TN: kout x cs per tap, `mult` = live taps of them);
  // red: length of the reduction; rows: GEMM rows of the layer.
  // Returns 0 (Small), 1 (Big: 128x128) or 2 (Big96: 128x96), whichever wastes less of its tiles.
  if (scalar) return 0;
  auto fill = [](int64_t d, int64_t t) { return (double)d / (double)(((d + t - 1) / t) * t); };
  const double f128 = fill(dim_m, 128) * fill(dim_n, 128), f96 = fill(dim_m, 128) * fill(dim_n, 96);
  int kind = f96 > f128 + 1e-9 ? 2 : 1;
  double fbest = kind == 2 ? f96 : f128;
  // weight gradients with every tap live and a dY channel count that is a multiple of 96: Flat96 (see its typedef)
  int64_t flat_tiles = 0;
  if (HF_CONV_FLAT96 && direction == 2 && all_taps && dim_m % 96 == 0 && dim_n % 4 == 0) {
    const double fflat = fill(mult * dim_n, 128);
    if (fflat > fbest + 0.05) { kind = 3; fbest = fflat; flat_tiles = (dim_m / 96) * ((mult * dim_n + 127) / 128); }
  }
  const bool fits = fbest >= 0.7;
  // ... and only where the launch has enough work to give ~3 workgroups per CU a K loop of >= 8 steps of 16 each
  // (a looser rule -- any reduction of >= 64 steps, splits capped at 8 steps per workgroup -- was measured to put
  // ResNet-50 layers on the 128-wide tiles and lose: 289 -> 268 matvecs/s): with a handful of steps per workgroup the 128-wide
  // tiles lose to the 64x64 ones, whose prologue / epilogue are a quarter the size (ResNet-50 on 64x64
  // images, batch 32: 260 matvecs/s with the 64x64 tiles everywhere, 228 -> 198 with the 128-wide ones wherever
  // they fit; All-CNN-C's 8192-row layers, 9 steps per workgroup: 128x96 tiles 37 us, 64x64 tiles 64 us)
  const int64_t tiles = kind == 3 ? flat_tiles
                                  : ((dim_m + 127) / 128) * ((dim_n + (kind == 2 ? 95 : 127)) / (kind == 2 ? 96 : 128)) * mult;
  const int64_t steps = (red + Big::BK - 1) / Big::BK;
  // (Flat96 weight gradients: a third of that work already pays -- All-CNN-C's stride-2 layers, 8192 / 2048 output rows,
  // ran 58 / 35 us on 36 / 72 64x64 tiles with 8 / 4 splits against MIOpen's 24 / 23 us)
  // (slab mode only: with the in-launch ticket reduction of the stand-alone calls a deep split makes the last
  // arriver's sum the longest chain of the launch -- 52 -> 87 us measured)
  const int64_t least = (kind == 3 && slab_mode) ? HF_FLAT96_MIN_WORK : HF_BIG_MIN_WORK;
  return (fits && rows >= 2048 && tiles * steps >= least) ? kind : 0;
}

// The `out_c` of a weight-gradient problem (X zero-padded to cs channels, dW has out_c <= cs of them) is applied AFTER
// setup() has chosen the tile configuration: Flat96 enumerates its output columns flat over (tap, channel), which a
// padded operand breaks unless there is a single tap (the padded columns of one row raced with the next
// row's first entries and the last row wrote past the slab) -- refused, loudly, instead.
static int apply_out_c(ConvArgs& a, int64_t out_c) {
  if (!out_c) return HF_OK;
  if (a.big == 3 && out_c != a.cs && a.ntaps != 1) return HF_ERR_ARG;
  a.out_c = (int)out_c;
  return HF_OK;
}

// What the stand-alone calls with the in-launch (ticket) reduction bring along; the slab-mode calls have none.
struct Scratch {
  float* ws;
  int64_t ws_bytes;
  int* tickets;
  int64_t n_tickets;
  int target_blocks;  // (<= 0: the split count comes from the cost model)
};

// Fill `a` for problem `p`; returns the number of workgroups (<= 0: error code).  `tickets`: ticket mode on the
// scratch `sc`; else slab mode with p.splits splits (0: the plan -- choose them, towards sc->target_blocks workgroups
// if `sc` names a count > 0).
int64_t setup(ConvArgs& a, const hf_conv_problem& p, const Scratch* sc, bool tickets, bool force_small = false) {
  const int direction = p.direction, slab_splits = tickets ? -1 : p.splits, target_blocks = sc ? sc->target_blocks : 0;
  const int64_t n = p.n, h = p.h, w = p.w, c = p.c, k = p.k, r = p.r, s = p.s, stride_h = p.stride_h,
                stride_w = p.stride_w, pad_h = p.pad_h, pad_w = p.pad_w;
  const int64_t oh = (h + 2 * pad_h - r) / stride_h + 1, ow = (w + 2 * pad_w - s) / stride_w + 1;
  memset(&a, 0, sizeof(a));
  a.src = (const float*)p.act;
  a.mat = (const float*)p.mat;
  a.out = (float*)p.out;
  a.ws = sc ? sc->ws : nullptr;
  a.tickets = sc ? sc->tickets : nullptr;
  a.R = (int)r; a.S = (int)s;
  a.stride_h = (int)stride_h; a.stride_w = (int)stride_w; a.pad_h = (int)pad_h; a.pad_w = (int)pad_w;
  a.shift_h = a.shift_w = -1;
  if ((stride_h & (stride_h - 1)) == 0 && (stride_w & (stride_w - 1)) == 0) {
    a.shift_h = a.shift_w = 0;
    while ((1 << a.shift_h) < stride_h) ++a.shift_h;
    while ((1 << a.shift_w) < stride_w) ++a.shift_w;
  }
  // taps that meet data for at least one output position
  for (int rr = 0; rr < r; ++rr) {
    bool live_r = false;
    for (int64_t y = 0; y < oh && !live_r; ++y) { const int64_t iy = y * stride_h - pad_h + rr; live_r = iy >= 0 && iy < h; }
    if (!live_r) continue;
    for (int qq = 0; qq < s; ++qq) {
      bool live_q = false;
      for (int64_t x = 0; x < ow && !live_q; ++x) { const int64_t ix = x * stride_w - pad_w + qq; live_q = ix >= 0 && ix < w; }
      if (live_q) { a.tap_rs[a.ntaps] = rr | (qq << 8); a.ntaps++; }
    }
  }
  if (a.ntaps == 0) return HF_ERR_ARG;
  int64_t rows, red_steps;
  if (direction == 0) {        // F: act = X [n,h,w,c] (pixel stride act_ld), mat = Wt [k][r*s][c], out [n,oh,ow,k]
    a.dgrad = 0; rows = n * oh * ow; a.rh = (int)oh; a.rw = (int)ow; a.sh_ = (int)h; a.sw_ = (int)w;
    a.cs = (int)c; a.nout = (int)k; a.ldc = (int)k;
  } else if (direction == 1) { // D: act = dY [n,oh,ow,k], mat = WT [c][r*s][k], out = dX [n,h,w,c]
    a.dgrad = 1; rows = n * h * w; a.rh = (int)h; a.rw = (int)w; a.sh_ = (int)oh; a.sw_ = (int)ow;
    a.cs = (int)k; a.nout = (int)c; a.ldc = (int)c;
  } else {                     // W: act = X [n,h,w,c], mat = dY [n*oh*ow][k], out = dW [k][r*s][c]
    a.dgrad = 0; rows = n * oh * ow; a.rh = (int)oh; a.rw = (int)ow; a.sh_ = (int)h; a.sw_ = (int)w;
    a.cs = (int)c; a.kout = (int)k;
  }
  a.out_c = a.cs;
  a.rows = (int)rows;
  a.cs_ld = (int)(p.act_ld > 0 ? p.act_ld : a.cs);
  a.mat_ld = (int)(p.mat_ld > 0 ? p.mat_ld : a.cs);
  a.scalar = ((c % 4) || (k % 4) || (a.cs_ld % 4) || (a.mat_ld % 4)) ? 1 : 0;
  if (a.cs_ld < a.cs || a.mat_ld < a.cs || (p.mat_ld > 0 && direction == 2)) return HF_ERR_ARG;
  // strided data gradient in slab mode: residue classes of the input pixel (see ConvArgs; 1 268 -> 1 292 matvecs/s,
  // round 3)
  int cls_taps_max = a.ntaps;
  // (large maps only: on ResNet-18's <= 1568-row layers the launch is latency-bound either way and the extra
  // partially-filled row tiles cost ~1 % of the bench)
  const bool classes = direction == 1 && slab_splits >= 0 && (stride_h > 1 || stride_w > 1) &&
                       stride_h * stride_w <= 4 && !a.scalar && n * h * w >= 2048;
  struct { int py, px, hc, wc, ntaps; unsigned char r[MAX_TAPS], q[MAX_TAPS]; } cl[4];
  int ncls = 0;
  if (classes) {
    cls_taps_max = 0;
    for (int py = 0; py < stride_h; ++py)
      for (int px = 0; px < stride_w; ++px) {
        const int hc = (int)((h - py + stride_h - 1) / stride_h), wc = (int)((w - px + stride_w - 1) / stride_w);
        if (hc <= 0 || wc <= 0) continue;
        auto& c_ = cl[ncls];
        c_.py = py; c_.px = px; c_.hc = hc; c_.wc = wc; c_.ntaps = 0;
        for (int t_ = 0; t_ < a.ntaps; ++t_) {
          const int rr = a.tap_rs[t_] & 255, qq = a.tap_rs[t_] >> 8;
          const int64_t dy = py + pad_h - rr, dx = px + pad_w - qq;
          if (((dy % stride_h) + stride_h) % stride_h == 0 && ((dx % stride_w) + stride_w) % stride_w == 0) {
            c_.r[c_.ntaps] = (unsigned char)rr; c_.q[c_.ntaps] = (unsigned char)qq; c_.ntaps++;
          }
        }
        if (c_.ntaps > cls_taps_max) cls_taps_max = c_.ntaps;
        ++ncls;
      }
  }
  a.big = force_small      ? 0
          : direction <= 1 ? want_big(direction, rows, rows, a.nout, (int64_t)cls_taps_max * a.cs, 1, a.scalar)
                           : want_big(direction, rows, a.kout, a.cs, rows, a.ntaps, a.scalar, a.ntaps == (int)(r * s),
                                      slab_splits >= 0);
  const int BM = a.big == 3 ? Flat96::BM : a.big ? Big::BM : Small::BM;
  const int BN = a.big == 2 ? Big96::BN : a.big ? Big::BN : Small::BN;
  const int BK = a.big ? Big::BK : Small::BK;
  if (direction <= 1) {
    a.tiles_m = (int)((rows + BM - 1) / BM);
    a.tiles_n = (a.nout + BN - 1) / BN;
    red_steps = (int64_t)cls_taps_max * ((a.cs + BK - 1) / BK);
    if (ncls > 0) {  // rows class by class, taps reordered class-major
      a.ncls = ncls;
      int tile0 = 0, tap0 = 0;
      for (int i = 0; i < ncls; ++i) {
        a.cls_tile0[i] = tile0; a.cls_tap0[i] = tap0;
        a.cls_h[i] = cl[i].hc; a.cls_w[i] = cl[i].wc; a.cls_py[i] = cl[i].py; a.cls_px[i] = cl[i].px;
        for (int t_ = 0; t_ < cl[i].ntaps; ++t_) a.tap_rs[tap0 + t_] = cl[i].r[t_] | (cl[i].q[t_] << 8);
        tap0 += cl[i].ntaps;
        tile0 += (int)((n * cl[i].hc * cl[i].wc + BM - 1) / BM);
      }
      a.cls_tile0[ncls] = tile0; a.cls_tap0[ncls] = tap0;
      a.tiles_m = tile0;
      if (red_steps < 1) red_steps = 1;
    }
  } else {
    a.tiles_m = (a.kout + BM - 1) / BM;
    a.tiles_n = a.big == 3 ? (a.ntaps * a.cs + BN - 1) / BN : a.ntaps * ((a.cs + BN - 1) / BN);
    red_steps = (rows + BK - 1) / BK;
  }
  a.steps = (int)red_steps;
  const int64_t tiles = (int64_t)a.tiles_m * a.tiles_n;
  if (slab_splits >= 0) {  // consumer-side reduction: no workspace, no tickets
    a.slabs = 1;
    a.slab_stride = p.slab_stride;
    int sp = slab_splits > 0 ? slab_splits : choose_splits(tiles, red_steps, target_blocks, 0, true, BK);
    // strided data gradients by residue class: the classes' K loops differ by up to 4x (1 ... 4 taps of a 3x3 / stride 2
    // kernel) and a uniform split leaves the short ones with 2 steps per workgroup -- with one workgroup per CU already
    // there, do not split (A/B knob HF_DCLASS_NOSPLIT)
    if (HF_DCLASS_NOSPLIT && slab_splits == 0 && ncls > 0 && a.big && tiles >= 256) sp = 1;
    if (sp > red_steps) sp = (int)red_steps;
    while (sp > 1 && ((red_steps + sp - 1) / sp) * (sp - 1) >= red_steps) --sp;
    a.splits = sp < 1 ? 1 : sp;
    return tiles * a.splits;
  }
  // more output tiles than ticket counters (large batches / maps): such a launch fills the chip
  // without a K split, and an unsplit launch draws no tickets
  a.splits = tiles > sc->n_tickets ? 1 : choose_splits(tiles, red_steps, target_blocks, sc->ws_bytes, false, BK,
                                                        (int64_t)BM * BN);
  return tiles * a.splits;
}

// what a LAUNCH needs on top of the field ranges: pointers, their alignment, 32-bit index space
int check_common(const hf_conv_problem& p, int64_t oh, int64_t ow, int dtype, const Scratch* sc) {
  if (!p.out || !p.act || !p.mat || (sc && (!sc->ws || !sc->tickets))) return HF_ERR_ARG;
  if (dtype != HF_F32) return HF_ERR_ARG;
  // (channel counts that are not multiples of 4 run the element-wise gather variant)
  if ((sc && !aligned16(sc->ws)) || (((p.c % 4) == 0 && (p.k % 4) == 0) &&
                                     (!aligned16(p.out) || !aligned16(p.act) || !aligned16(p.mat))))
    return HF_ERR_ALIGN;
  const int64_t ck = p.c > p.k ? p.c : p.k;
  if (p.n * p.h * p.w * ck > 0x7fffffffLL || p.n * oh * ow * ck > 0x7fffffffLL || p.k * p.r * p.s * p.c > 0x7fffffffLL)
    return HF_ERR_ARG;
  return HF_OK;
}

// THE planner: the one place that turns a problem description into kernel arguments, for hf_conv2d_nhwc_plan and
// for every launching entry point alike -- what the plan answers and what a launch runs cannot drift apart.  In
// this order (it fixes which code a call with several faults returns):
//   1. field ranges, the out_c rule included;  2. check_common (launches only);  3. setup;
//   4. the planned split count is the caller's (slab-mode launches: ask hf_conv2d_nhwc_plan first);
//   5. what the caller's launch form cannot run (`allow`);  6. apply_out_c.
// `sc`: ticket mode.  PLAN_ONLY: no launch follows -- no pointers, no 2^31 limits, p.splits == 0 means "choose", and
// `sc` (nullable) only carries target_blocks -- unless PLAN_TICKETS asks for the plan of a ticket-mode launch on the
// sizes `sc` names (hf_conv2d_nhwc_plan_info).
enum : unsigned {
  ALLOW_SCALAR = 1,  // the form has the element-wise gather variant (channel counts not multiples of 4)
  ALLOW_BIG = 2,     // ... the 128-wide tile configurations
  ALLOW_CLS = 4,     // ... the residue-class enumeration of strided data gradients
  ALLOW_ALL = 7,
  PLAN_ONLY = 8,
  PLAN_TICKETS = 16,
  FORCE_SMALL = 32,  // the 64x64 configuration whatever the geometry (the squared-sum kernel has no other)
};

int plan_problem(const hf_conv_problem& p, int dtype, const Scratch* sc, unsigned allow, ConvArgs& a, int64_t& blocks) {
  const bool plan = allow & PLAN_ONLY, tickets = sc && (!plan || (allow & PLAN_TICKETS)), slab_launch = !sc && !plan;
  if (p.direction < 0 || p.direction > 2 || (slab_launch && p.splits < 1) || p.slab_stride < 0 || p.mat_ld < 0)
    return HF_ERR_ARG;
  if (p.out_c < 0 || p.out_c > p.c || (p.out_c && p.direction != 2)) return HF_ERR_ARG;
  if (p.n <= 0 || p.h <= 0 || p.w <= 0 || p.c <= 0 || p.k <= 0 || p.r <= 0 || p.s <= 0 || p.stride_h <= 0 ||
      p.stride_w <= 0 || p.pad_h < 0 || p.pad_w < 0 || p.r * p.s > MAX_TAPS)
    return HF_ERR_ARG;
  const int64_t oh = (p.h + 2 * p.pad_h - p.r) / p.stride_h + 1, ow = (p.w + 2 * p.pad_w - p.s) / p.stride_w + 1;
  if (oh <= 0 || ow <= 0) return HF_ERR_ARG;
  if (!plan) {
    const int rc = check_common(p, oh, ow, dtype, sc);
    if (rc) return rc;
  }
  blocks = setup(a, p, sc, tickets, allow & FORCE_SMALL);
  if (blocks <= 0) return (int)blocks;
  if (slab_launch && a.splits != p.splits) return HF_ERR_ARG;
  if ((a.scalar && !(allow & ALLOW_SCALAR)) || (a.big && !(allow & ALLOW_BIG)) || (a.ncls > 0 && !(allow & ALLOW_CLS)))
    return HF_ERR_ARG;
  return apply_out_c(a, p.out_c);
}

// One problem, every variant.
int launch_single(const hf_conv_problem& p, int dtype, const Scratch* sc, void* stream) {
  ConvArgs a;
  int64_t blocks;
  const int rc = plan_problem(p, dtype, sc, ALLOW_ALL, a, blocks);
  if (rc) return rc;
  launch_one(p.direction, a, blocks, (hipStream_t)stream);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

// One forward / data-gradient problem and one weight-gradient problem in one launch (16-byte gathers only).
int launch_pair(const hf_conv_problem& d, const hf_conv_problem& w, int dtype, const Scratch* sd, const Scratch* sw,
                void* stream) {
  ConvArgs a[2];
  int64_t blocks[2];
  int rc = plan_problem(d, dtype, sd, ALLOW_BIG | ALLOW_CLS, a[0], blocks[0]);
  if (!rc) rc = plan_problem(w, dtype, sw, ALLOW_BIG | ALLOW_CLS, a[1], blocks[1]);
  if (rc) return rc;
  launch_dw(a[0], a[1], blocks[0], blocks[1], (hipStream_t)stream);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

}  // namespace

// C linkage comes from hf_pcg.h.  The positional entry points describe their problem as an hf_conv_problem
// {direction, out, act, mat, n .. pad_w, act_ld, out_c, splits, slab_stride, mat_ld} and go the way of the struct ones.
int hf_conv2d_nhwc(int direction, void* out, const void* act, const void* mat, int64_t n,
                   int64_t h, int64_t w, int64_t c, int64_t k, int64_t r, int64_t s,
                   int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w,
                   int64_t act_ld, void* workspace, int64_t workspace_bytes, void* tickets,
                   int64_t n_tickets, int target_blocks, int dtype, void* stream) {
  const hf_conv_problem p = {direction, out, act, mat, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w,
                             act_ld, 0, 0, 0, 0};
  const Scratch sc = {(float*)workspace, workspace_bytes, (int*)tickets, n_tickets, target_blocks};
  return launch_single(p, dtype, &sc, stream);
}

int hf_conv2d_nhwc_backward(void* dx, void* dw, const void* dy, const void* x, const void* w_t, int64_t n,
                            int64_t h, int64_t w, int64_t c, int64_t k, int64_t r, int64_t s,
                            int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w,
                            void* workspace, int64_t workspace_bytes, void* tickets, int64_t n_tickets,
                            int target_blocks, int dtype, void* stream) {
  if (!dx || !dw) return HF_ERR_ARG;  // (ahead of any alignment verdict on the other operands, as ever)
  const hf_conv_problem d = {1, dx, dy, w_t, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w, 0, 0, 0, 0, 0};
  const hf_conv_problem g = {2, dw, x, dy, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w, 0, 0, 0, 0, 0};
  // the two halves get disjoint halves of the scratch (they run concurrently)
  const int64_t half_ws = (workspace_bytes / 2) & ~(int64_t)15, half_t = n_tickets / 2;
  const Scratch sd = {(float*)workspace, half_ws, (int*)tickets, half_t, target_blocks};
  const Scratch sw = {workspace ? (float*)((char*)workspace + half_ws) : nullptr, half_ws,
                      tickets ? (int*)tickets + half_t : nullptr, half_t, target_blocks};
  return launch_pair(d, g, dtype, &sd, &sw, stream);
}

// ---- consumer-side reduction ("slab") variants ---------------------------------------
// Split s writes its partial result, in the output's own layout, to out + s*slab_stride and
// the launch ends there: the kernel that consumes the tensor sums the `splits` slabs in its
// prologue (hf_chan_affine_ex, hf_bn_adjoint_pre, hf_pack_ex).  No workspace, no tickets, no
// fences: the launch boundary publishes the slabs.
int hf_conv2d_nhwc_plan(int direction, int64_t n, int64_t h, int64_t w, int64_t c, int64_t k, int64_t r,
                        int64_t s, int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w,
                        int target_blocks) {
  const hf_conv_problem p = {direction, nullptr, nullptr, nullptr, n, h, w, c, k, r, s, stride_h, stride_w, pad_h,
                             pad_w, 0, 0, 0, 0, 0};
  const Scratch sc = {nullptr, 0, nullptr, 0, target_blocks};
  ConvArgs a;
  int64_t blocks;
  const int rc = plan_problem(p, HF_F32, &sc, ALLOW_ALL | PLAN_ONLY, a, blocks);
  return rc ? rc : a.splits;
}

int hf_conv2d_nhwc_plan_info(const hf_conv_problem* p, int ticket_mode, int64_t ws_bytes, int64_t n_tickets,
                             int target_blocks, hf_conv_plan_info* out) {
  if (!p || !out || (ticket_mode && (ws_bytes < 0 || n_tickets < 0))) return HF_ERR_ARG;
  const Scratch sc = {nullptr, ws_bytes, nullptr, n_tickets, target_blocks};
  ConvArgs a;
  int64_t blocks;
  const int rc = plan_problem(*p, HF_F32, &sc, ALLOW_ALL | PLAN_ONLY | (ticket_mode ? PLAN_TICKETS : 0), a, blocks);
  if (rc) return rc;
  memset(out, 0, sizeof(*out));
  out->config = a.big;
  out->scalar = a.scalar;
  out->ncls = a.ncls;
  for (int i = 0; i < a.ncls; ++i) out->cls_taps[i] = a.cls_tap0[i + 1] - a.cls_tap0[i];
  out->live_taps = a.ntaps;
  out->tiles_m = a.tiles_m;
  out->tiles_n = a.tiles_n;
  out->steps = a.steps;
  out->splits = a.splits;
  out->blocks = blocks;
  return HF_OK;
}

int hf_conv2d_nhwc_slabs(int direction, void* out, const void* act, const void* mat, int64_t n, int64_t h,
                         int64_t w, int64_t c, int64_t k, int64_t r, int64_t s, int64_t stride_h,
                         int64_t stride_w, int64_t pad_h, int64_t pad_w, int64_t act_ld, int64_t mat_ld,
                         int64_t out_c, int splits, int64_t slab_stride, int dtype, void* stream) {
  const hf_conv_problem p = {direction, out, act, mat, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w,
                             act_ld, out_c, splits, slab_stride, mat_ld};
  return launch_single(p, dtype, nullptr, stream);
}

int hf_conv2d_nhwc_slabs_unpack(void* out, const void* act, const void* mat, int64_t n, int64_t h, int64_t w,
                                int64_t c, int64_t k, int64_t r, int64_t s, int64_t stride_h, int64_t stride_w,
                                int64_t pad_h, int64_t pad_w, int64_t act_ld, int64_t mat_ld, int splits,
                                int64_t slab_stride, const void* usrc, void* const* udsts, const int64_t* usrc_offs,
                                const int64_t* unumels, const int64_t* uslabs, const int64_t* uinners,
                                const int64_t* ulive, const int64_t* uhalves, int n_tensors, int dtype,
                                void* stream) {
  return hf_conv2d_nhwc_slabs_unpack_compact(out, act, mat, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w, act_ld,
                                             mat_ld, splits, slab_stride, usrc, udsts, usrc_offs, unumels, uslabs,
                                             uinners, ulive, uhalves, nullptr, n_tensors, dtype, stream);
}

int hf_conv2d_nhwc_slabs_unpack_compact(void* out, const void* act, const void* mat, int64_t n, int64_t h, int64_t w,
                                        int64_t c, int64_t k, int64_t r, int64_t s, int64_t stride_h, int64_t stride_w,
                                        int64_t pad_h, int64_t pad_w, int64_t act_ld, int64_t mat_ld, int splits,
                                        int64_t slab_stride, const void* usrc, void* const* udsts,
                                        const int64_t* usrc_offs, const int64_t* unumels, const int64_t* uslabs,
                                        const int64_t* uinners, const int64_t* ulive, const int64_t* uhalves,
                                        const int64_t* ucompact, int n_tensors, int dtype, void* stream) {
  if (!usrc || !udsts || !usrc_offs || !unumels || !uslabs || !uinners || n_tensors < 1) return HF_ERR_ARG;
  if (uhalves)  // (transposed copies run as LDS-tiled workgroups of hf_unpack_weights' own kernel only)
    for (int t_ = 0; t_ < n_tensors; ++t_)
      if (uhalves[t_] == 2) return HF_ERR_ARG;
  const hf_conv_problem p = {0, out, act, mat, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w,
                             act_ld, 0, splits, slab_stride, mat_ld};
  ConvArgs a;
  int64_t blocks;
  const int rc = plan_problem(p, dtype, nullptr, ALLOW_SCALAR, a, blocks);  // (small-map launches only)
  if (rc) return rc;
  hf_shared::UnpackArgs u;
  int ublocks = 0;
  const int next = hf_shared::fill_unpack_args<float>(u, &ublocks, 0, udsts, usrc_offs, unumels, uslabs, uinners,
                                                      ulive, uhalves, ucompact, n_tensors,
                                                      /*allow_transposed=*/false);
  if (next < 0) return next;
  if (next != n_tensors || ublocks < 1) return HF_ERR_ARG;  // more tensors than one argument block holds
  launch_unpack(a, blocks, u, (const float*)usrc, ublocks, (hipStream_t)stream);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_conv2d_nhwc_backward_slabs(void* dx, void* dw, const void* dy, const void* x, const void* w_t,
                                  int64_t n, int64_t h, int64_t w, int64_t c, int64_t k, int64_t r,
                                  int64_t s, int64_t stride_h, int64_t stride_w, int64_t pad_h,
                                  int64_t pad_w, int splits_d, int64_t slab_stride_d, int splits_w,
                                  int64_t slab_stride_w, int dtype, void* stream) {
  if (!dx || !dw || !x || splits_d < 1 || splits_w < 1) return HF_ERR_ARG;  // (ahead of any alignment verdict, as ever)
  const hf_conv_problem d = {1, dx, dy, w_t, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w,
                             0, 0, splits_d, slab_stride_d, 0};
  const hf_conv_problem g = {2, dw, x, dy, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w,
                             0, 0, splits_w, slab_stride_w, 0};
  return launch_pair(d, g, dtype, nullptr, nullptr, stream);
}

int hf_conv2d_nhwc_dw_slabs(const hf_conv_problem* d, const hf_conv_problem* w, int dtype, void* stream) {
  if (!d || !w || d->direction > 1 || w->direction != 2) return HF_ERR_ARG;
  return launch_pair(*d, *w, dtype, nullptr, nullptr, stream);
}

// Tangent convolutions (direction 0, slab mode, 64x64 tiles) whose epilogue also writes the per-channel partial sums
// a TRAIN-mode BatchNorm behind them needs (ConvArgs::bn_*): one launch for up to GROUP_MAX problems, each with or
// without sums.  HF_ERR_ARG for anything the BNSUM instantiations do not cover -- the caller then issues the plain
// launch and the reduction launch.
int hf_conv2d_nhwc_group_slabs_bnsum(const hf_conv_problem* problems, int n_problems, const hf_conv_bnsum* sums,
                                     int dtype, void* stream) {
  if (!problems || !sums || n_problems < 1 || n_problems > GROUP_MAX) return HF_ERR_ARG;
  ConvArgs a[GROUP_MAX];
  GroupMeta m;
  memset(a, 0, sizeof(a));
  memset(&m, 0, sizeof(m));
  for (int i = 0; i < n_problems; ++i) {
    if (problems[i].direction != 0) return HF_ERR_ARG;
    int64_t blocks;
    const int rc = plan_problem(problems[i], dtype, nullptr, 0, a[i], blocks);
    if (rc) return rc;
    const hf_conv_bnsum& b = sums[i];
    if (b.part_1) {
      if (!b.part_x || !b.x || !b.mean || !b.rstd) return HF_ERR_ARG;
      if (b.part_rows != (int64_t)a[i].tiles_m * a[i].splits) return HF_ERR_ARG;  // (= ceil(rows / 64) * splits)
      a[i].bn_x = (const float*)b.x; a[i].bn_mean = (const float*)b.mean; a[i].bn_rstd = (const float*)b.rstd;
      a[i].bn_part_x = (float*)b.part_x; a[i].bn_part_1 = (float*)b.part_1;
    }
    if (group_add(m, i, false, blocks)) return HF_ERR_ARG;
  }
  launch_group(a, m, /*bnsum=*/true, (hipStream_t)stream);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

int hf_conv2d_nhwc_group_slabs(const hf_conv_problem* problems, int n_problems, int dtype, void* stream) {
  if (!problems || n_problems < 1 || n_problems > GROUP_MAX) return HF_ERR_ARG;
  ConvArgs a[GROUP_MAX];  // (passed to the kernel by value, one argument each)
  GroupMeta m;
  memset(a, 0, sizeof(a));
  memset(&m, 0, sizeof(m));
  for (int i = 0; i < n_problems; ++i) {
    int64_t blocks;
    const int rc = plan_problem(problems[i], dtype, nullptr, ALLOW_BIG | ALLOW_CLS, a[i], blocks);
    if (rc) return rc;
    if (group_add(m, i, problems[i].direction == 2, blocks)) return HF_ERR_ARG;
  }
  launch_group(a, m, /*bnsum=*/false, (hipStream_t)stream);
  HF_HIP(hipGetLastError());
  return HF_OK;
}

// ---- sum over the samples of the squared per-sample weight gradient (BackPACK's SumGradSquared) ----------------------
namespace {

// a split count that leaves no split without a sample: split s takes samples [s*ceil(n/splits), ...)
bool sq_shares_ok(int64_t n, int64_t splits) {
  return splits >= 1 && splits <= n && ((n + splits - 1) / splits) * (splits - 1) < n;
}

// Workgroups the per-sample form is split towards.  Its workgroups are long -- a sample's ceil(P / BK) steps times the
// samples of the share, with one step of loads in flight -- and four of them fit a CU (LDS, registers), so the matrix
// pipe is fed by the OTHER resident workgroups while one waits: two rounds of a full chip.  Measured per layer of
// All-CNN-C (batch 32 and 128) and ResNet-18 (batch 32), scripts/bench_diag_ef.py --split-sweep
// (profiles/r23_sqsum_split_sweep.jsonl): from the 256 of the latency-bound product launches the time still halves
// (All-CNN-C's 96 -> 96 layer on 32x32 maps, batch 128: 832 us at 288 workgroups, 467 at 1 152, 405 at 2 304, 399 at
// 4 608); beyond ~2 000 it is flat or rises, and every further split is one more slab for the gather to read.
#ifndef HF_SQSUM_TARGET_BLOCKS
#define HF_SQSUM_TARGET_BLOCKS 2048
#endif

// Geometry of a squared-sum problem through THE planner (direction 2, slab mode, one split, 64x64 tiles), and the
// planned split count over the samples: towards the workgroup target (the squared-operand form, P == 1, is an ordinary
// reduction over n rows: the conv planner's own K-split plan over its ceil(n / BK) steps), at most n, no split left
// without a sample.
int sq_plan(const hf_conv_problem& p, int target_blocks, ConvArgs& a, int64_t& tiles, int64_t& P) {
  int64_t blocks;
  const int rc = plan_problem(p, HF_F32, nullptr, ALLOW_SCALAR | PLAN_ONLY | FORCE_SMALL, a, blocks);
  if (rc) return rc;
  P = (int64_t)a.rh * a.rw;
  tiles = (int64_t)a.tiles_m * a.tiles_n;
  int64_t sp;
  if (P == 1) {
    sp = choose_splits(tiles, (p.n + Small::BK - 1) / Small::BK, target_blocks, 0, true, Small::BK);
  } else {
    sp = ((target_blocks > 0 ? target_blocks : HF_SQSUM_TARGET_BLOCKS) + tiles - 1) / tiles;
  }
  if (sp > p.n) sp = p.n;
  if (sp < 1) sp = 1;
  while (!sq_shares_ok(p.n, sp)) --sp;
  return (int)sp;
}

}  // namespace

int hf_conv2d_nhwc_sqsum_plan(int64_t n, int64_t h, int64_t w, int64_t c, int64_t k, int64_t r, int64_t s,
                              int64_t stride_h, int64_t stride_w, int64_t pad_h, int64_t pad_w, int target_blocks) {
  const hf_conv_problem p = {2, nullptr, nullptr, nullptr, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w,
                             0, 0, 1, 0, 0};
  ConvArgs a;
  int64_t tiles, P;
  return sq_plan(p, target_blocks, a, tiles, P);
}

int hf_conv2d_nhwc_sqsum_slabs(void* out, const void* act, const void* mat, int64_t n, int64_t h, int64_t w, int64_t c,
                               int64_t k, int64_t r, int64_t s, int64_t stride_h, int64_t stride_w, int64_t pad_h,
                               int64_t pad_w, int64_t act_ld, int64_t out_c, float pre, int splits,
                               int64_t slab_stride, int dtype, void* stream) {
  const hf_conv_problem p = {2, out, act, mat, n, h, w, c, k, r, s, stride_h, stride_w, pad_h, pad_w,
                             act_ld, out_c, 1, slab_stride, 0};
  ConvArgs a;
  int64_t tiles, P;
  if (act_ld < 0) return HF_ERR_ARG;
  const int planned = sq_plan(p, 0, a, tiles, P);  // (field ranges, live taps, tiles: the planner's)
  if (planned < 1) return planned;
  const int rc = check_common(p, a.rh, a.rw, dtype, nullptr);
  if (rc) return rc;
  if (!(pre - pre == 0.f) || !sq_shares_ok(n, splits)) return HF_ERR_ARG;  // (NaN / infinity; an empty split)
  if (splits > 1 && slab_stride < k * r * s * (int64_t)a.out_c) return HF_ERR_ARG;  // (slabs would overlap)
  if (tiles * splits > 0x7fffffffLL) return HF_ERR_ARG;
  a.splits = splits;
  seal(a);
  const SqArgs q = {pre, (int)n, (int)P, (int)((n + splits - 1) / splits)};
  const dim3 grid((unsigned)(tiles * splits)), block(CT);
  hipStream_t st = (hipStream_t)stream;
  if (P == 1) {
    if (a.scalar) hipLaunchKernelGGL((k_conv_tn_sq<true, true>), grid, block, 0, st, a, q);
    else hipLaunchKernelGGL((k_conv_tn_sq<false, true>), grid, block, 0, st, a, q);
  } else {
    if (a.scalar) hipLaunchKernelGGL((k_conv_tn_sq<true, false>), grid, block, 0, st, a, q);
    else hipLaunchKernelGGL((k_conv_tn_sq<false, false>), grid, block, 0, st, a, q);
  }
  HF_HIP(hipGetLastError());
  return HF_OK;
}
