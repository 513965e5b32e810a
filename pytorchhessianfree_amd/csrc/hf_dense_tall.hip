// hf_dense_tall.hip -- the dense-stack engine's kernels for TALL batches (257 .. 8192 rows): the three GEMMs of a
// fully-connected layer inside a curvature product (T: t_x W^T + x V^T, D: g_a W + g V, W: g^T x) as ordinary LDS-tiled
// fp32 GEMMs on __builtin_amdgcn_mfma_f32_32x32x2f32, and the two row reductions between them (activation adjoint with its
// bias sum, column sum of squares) split over row blocks.  The skinny kernels of hf_dense.hip hold the whole batch in
// registers and stage nothing; run over more row blocks they would re-read the activation operand c_out / 32 times.  Here
// both operands of a 128 x 128 output tile are reused out of LDS.  fp32, wave64, no atomics, every sum in one fixed order:
// two launches on the same operands agree bitwise.
//
// Rows: 257 <= rows <= 8192, and rows * c_in, rows * c_out, c_out * c_in < 2^31: every index into an operand is an `int`
// (only row offsets are widened where they are multiplied by a pitch).  Larger problems are refused with HF_ERR_ARG.
//
// The tile.  A 256-thread workgroup owns a 128 x 128 tile of C = A B (A: [m][k], B: [k][n]); its 4 waves form a 2 x 2 grid,
// wave (wm, wn) holds rows 64 wm .. + 63 and columns 64 wn .. + 63 as 2 x 2 MFMA tiles = 64 accumulator registers per
// lane (accumulator q of lane l is C[(q & 3) + 8 (q >> 2) + 4 (l >> 5)][l & 31] of its MFMA tile).  The reduction runs in
// steps of BK = 16 through two LDS stages: the global loads of step s + 1 are issued into registers before the MFMAs of
// step s and written to the other stage after them; one barrier per step.
//
// LDS layout: k-major, As[k][m] and Bs[k][n].  One MFMA operand is lane l -> X[k = 2 kk + (l >> 5)][i = l & 31]: each half
// wave reads 32 CONSECUTIVE words of one k-row -- 32 different banks whatever the row pitch: the read side has no bank
// conflict.  The write side depends on how the operand lies in memory:
//   * k-major in memory (rows contiguous along m / n: W and V of the D GEMM, both operands of the W GEMM): thread t copies
//     the quad n = 4 (t & 31) .. + 3 of row k = t >> 5 (and k + 8) with one 16-byte LDS store; a half wave writes 512
//     consecutive bytes.  Row pitch 128 words, no padding.
//   * reduction-contiguous in memory (t_x, x, W, V of the T GEMM; g_a, g of the D GEMM): the staging TRANSPOSES.  Thread t
//     loads the quad k = 4 (t & 3) .. + 3 of row m = t >> 2 (and m + 64) -- 4 lanes cover the 64 bytes a row contributes
//     to a step -- and writes its 4 words to rows 4 (t & 3) + e, column m.  With a pitch of 128 words the 4 quads of a row
//     group would fall on the same bank (4-way conflict); the pitch of these tiles is 130 words: the lanes of a half wave
//     (8 rows m x 4 quads) then write banks 8 (t & 3) + (m & 7) + const -- all 32 different.
// LDS per stage: 16 x (130 + 130) x 4 = 16640 B (T), 16 x (130 + 128) x 4 = 16512 B (D), 16384 B (W); twice that for the
// two-term forms, twice again for the two stages: at most 66560 B (T, both terms) of the CU's 160 KB.
//
// Order of the additions into one accumulator: k ascending in pairs (one MFMA adds entries 2 kk and 2 kk + 1); in the
// two-term forms of T and D per pair first the first term's product, then the second's (t_x W before x V; g_a W before
// g V).  The W GEMM's two-pair form (the Hessian product's weight gradient) keeps one accumulator set per pair, as
// hf_dense_wgrad2 does, and adds them once at the end.
//
// One tile shape only: a layer narrower than 128 columns (a 10-class last layer) wastes most of its tiles' MFMAs.
#include "hf_dense_act.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TALL_MIN_ROWS = 257, TALL_MAX_ROWS = 8192;
constexpr int TILE = 128, BK = 16;
constexpr int PITCH_T = 130;  // row pitch (words) of a tile staged by transposition
constexpr int PITCH_D = 128;  // row pitch of a tile copied straight
constexpr int TALL_TARGET_BLOCKS = 512;
constexpr int COLS_PER_BLOCK = 64;    // row reductions: a workgroup owns 64 columns x its row block, 4 row lanes
constexpr int TALL_MAX_ROW_BLOCKS = 64;
constexpr int64_t TALL_MAX_ELEMS = (int64_t)1 << 31;

// ---- the plan: ONE definition, run by hf_dense_tall_plan and by every launching entry point ------------------------
inline bool tall_dims_ok(int64_t rows, int64_t c_in, int64_t c_out) {
  if (rows < TALL_MIN_ROWS || rows > TALL_MAX_ROWS) return false;
  if (c_in < 1 || c_in > DENSE_MAX_C || c_out < 1 || c_out > DENSE_MAX_C) return false;
  return rows * c_in < TALL_MAX_ELEMS && rows * c_out < TALL_MAX_ELEMS && c_in * c_out < TALL_MAX_ELEMS;
}

// reduction entries per split: a multiple of BK
inline int64_t tall_kper(int64_t len, int splits) {
  const int64_t per = (len + splits - 1) / splits;
  return (per + BK - 1) / BK * BK;
}

// the rule of hf_dense.hip's dense_split_ok at this family's step: no split may start behind the end
inline bool tall_split_ok(int64_t len, int splits) {
  if (splits < 1 || splits > DENSE_MAX_SPLITS) return false;
  return (int64_t)(splits - 1) * tall_kper(len, splits) < len;
}

inline int64_t tiles_of(int64_t n) { return (n + TILE - 1) / TILE; }

// about TALL_TARGET_BLOCKS workgroups for an m x n output reduced over `len`
inline int tall_planned_splits(int64_t len, int64_t m, int64_t n) {
  const int64_t tiles = tiles_of(m) * tiles_of(n);
  int64_t want = (TALL_TARGET_BLOCKS + tiles - 1) / tiles;
  if (want > DENSE_MAX_SPLITS) want = DENSE_MAX_SPLITS;
  int s = (int)want;
  while (s > 1 && !tall_split_ok(len, s)) --s;
  return s;
}

// rows one workgroup of a row reduction over [rows, c] walks: about TALL_TARGET_BLOCKS workgroups, at least 16 rows each,
// at most TALL_MAX_ROW_BLOCKS blocks, none empty
inline int tall_rows_per_block(int64_t rows, int64_t c) {
  const int64_t col_blocks = (c + COLS_PER_BLOCK - 1) / COLS_PER_BLOCK;
  int64_t want = (TALL_TARGET_BLOCKS + col_blocks - 1) / col_blocks;
  if (want > TALL_MAX_ROW_BLOCKS) want = TALL_MAX_ROW_BLOCKS;
  int64_t per = (rows + want - 1) / want;
  if (per < 16) per = 16;
  return (int)per;
}
inline int tall_row_blocks(int64_t rows, int64_t c) {
  const int per = tall_rows_per_block(rows, c);
  return (int)((rows + per - 1) / per);
}

struct TallPlan {
  int splits_t, splits_d, splits_w, row_blocks;
};

inline int tall_plan(int64_t rows, int64_t c_in, int64_t c_out, TallPlan* p) {
  if (!tall_dims_ok(rows, c_in, c_out)) return HF_ERR_ARG;
  p->splits_t = tall_planned_splits(c_in, rows, c_out);   // T: reduction over c_in, output [rows, c_out]
  p->splits_d = tall_planned_splits(c_out, rows, c_in);   // D: reduction over c_out, output [rows, c_in]
  p->splits_w = tall_planned_splits(rows, c_out, c_in);   // W: reduction over the rows, output [c_out, c_in]
  p->row_blocks = tall_row_blocks(rows, c_out);           // the row reductions over [rows, c_out]
  return HF_OK;
}

// ---- staging ---------------------------------------------------------------------------------------------------------
// Two quads per thread and operand tile: 2 x 256 quads = 16 x 128 entries.
struct Stage { Quad q[2]; };

// src[i][k] (reduction-contiguous, row pitch ld): quad k0 + 4 (t & 3) of rows i0 + (t >> 2), + 64
template <bool AL>
__device__ __forceinline__ Stage ldg_t(const float* __restrict__ src, int i0, int i_end, int ld, int k0, int ke) {
  Stage s;
  const int k = k0 + 4 * (threadIdx.x & 3);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = i0 + (threadIdx.x >> 2) + 64 * u;
    const bool ok = i < i_end;
    s.q[u] = ld_quad<AL>(src + (size_t)(ok ? i : 0) * ld, k, ke, ok);
  }
  return s;
}
__device__ __forceinline__ void sts_t(float* __restrict__ tile, const Stage& s) {
  const int kq = 4 * (threadIdx.x & 3), i = threadIdx.x >> 2;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[(kq + e) * PITCH_T + i + 64 * u] = s.q[u].e[e];
}

// src[k][i] (k-major, row pitch ld): quad i0 + 4 (t & 31) of rows k0 + (t >> 5), + 8
template <bool AL>
__device__ __forceinline__ Stage ldg_d(const float* __restrict__ src, int i0, int i_end, int ld, int k0, int ke) {
  Stage s;
  const int i = i0 + 4 * (threadIdx.x & 31);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int k = k0 + (threadIdx.x >> 5) + 8 * u;
    const bool ok = k < ke;
    s.q[u] = ld_quad<AL>(src + (size_t)(ok ? k : 0) * ld, i, i_end, ok);
  }
  return s;
}
__device__ __forceinline__ void sts_d(float* __restrict__ tile, const Stage& s) {
  const int i = 4 * (threadIdx.x & 31), k = threadIdx.x >> 5;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    F4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v.e[e] = s.q[u].e[e];
    *reinterpret_cast<F4*>(tile + (k + 8 * u) * PITCH_D + i) = v;
  }
}

template <bool TR, bool AL>
__device__ __forceinline__ Stage ldg(const float* __restrict__ src, int i0, int i_end, int ld, int k0, int ke) {
  return TR ? ldg_t<AL>(src, i0, i_end, ld, k0, ke) : ldg_d<AL>(src, i0, i_end, ld, k0, ke);
}
template <bool TR>
__device__ __forceinline__ void sts(float* __restrict__ tile, const Stage& s) {
  if (TR) sts_t(tile, s);
  else sts_d(tile, s);
}
__device__ __forceinline__ void square(Stage& s) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) s.q[u].e[e] *= s.q[u].e[e];
}

// ---- the GEMM: C[m][n] = scale * sum_k (A1[m][k] B1[k][n] + A2[m][k] B2[k][n]) over split z's share of K ---------------
struct TallGemm {
  float* out;                 // slab z at out + z * slab_stride, [M][N] dense
  const float *a[2], *b[2];   // the pairs; pair 1 exists where NT == 2
  int M, N, K, ld_a, ld_b, kper;
  long long slab_stride;
  float scale;
};

// AT / BT: the operand is reduction-contiguous in memory (staged by transposition), else k-major (copied).  NT: pairs.
// SEP: one accumulator set per pair, added once at the end (else both pairs into one set, per k pair first pair 0).
// SQ: every operand entry is squared once after its load.  AL: all operands allow the 16-byte loads.
// grid (ceil(N / 128), ceil(M / 128), splits)
template <bool AT, bool BT, int NT, bool SEP, bool SQ, bool AL>
__global__ __launch_bounds__(BLOCK) void k_tall_gemm(const TallGemm g) {
  constexpr int PA = AT ? PITCH_T : PITCH_D, PB = BT ? PITCH_T : PITCH_D;
  constexpr int SZ_A = BK * PA, SZ_B = BK * PB, SZ_STAGE = NT * (SZ_A + SZ_B);
  constexpr int NACC = SEP ? NT : 1;
  __shared__ __attribute__((aligned(16))) float lds[2 * SZ_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  const int wm = 64 * (wave >> 1), wn = 64 * (wave & 1);
  const int m0 = blockIdx.y * TILE, n0 = blockIdx.x * TILE;
  const int kb = blockIdx.z * g.kper, ke = min(kb + g.kper, g.K);

  f32x16 acc[NACC][2][2];
#pragma unroll
  for (int p = 0; p < NACC; ++p)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[p][t >> 1][t & 1][q] = 0.0f;

  Stage ra[NT], rb[NT];
  auto load = [&](int k0) {
#pragma unroll
    for (int p = 0; p < NT; ++p) {
      ra[p] = ldg<AT, AL>(g.a[p], m0, g.M, g.ld_a, k0, ke);
      rb[p] = ldg<BT, AL>(g.b[p], n0, g.N, g.ld_b, k0, ke);
      if (SQ) {
        square(ra[p]);
        square(rb[p]);
      }
    }
  };
  auto store = [&](int stage) {
    float* base = lds + stage * SZ_STAGE;
#pragma unroll
    for (int p = 0; p < NT; ++p) {
      sts<AT>(base + p * (SZ_A + SZ_B), ra[p]);
      sts<BT>(base + p * (SZ_A + SZ_B) + SZ_A, rb[p]);
    }
  };

  load(kb);
  store(0);
  __syncthreads();
  int stage = 0;
  for (int k0 = kb; k0 < ke; k0 += BK, stage ^= 1) {
    const bool more = k0 + BK < ke;
    if (more) load(k0 + BK);
    const float* base = lds + stage * SZ_STAGE;
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
#pragma unroll
      for (int p = 0; p < NT; ++p) {
        const float* as = base + p * (SZ_A + SZ_B) + (2 * kk + h) * PA + wm + j;
        const float* bs = base + p * (SZ_A + SZ_B) + SZ_A + (2 * kk + h) * PB + wn + j;
        const float a0 = as[0], a1 = as[32], b0 = bs[0], b1 = bs[32];
        f32x16(&c)[2][2] = acc[SEP ? p : 0];
        c[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, c[0][0], 0, 0, 0);
        c[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, c[0][1], 0, 0, 0);
        c[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, c[1][0], 0, 0, 0);
        c[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c[1][1], 0, 0, 0);
      }
    }
    if (more) store(stage ^ 1);
    __syncthreads();
  }

  float* __restrict__ out = g.out + (long long)blockIdx.z * g.slab_stride;
#pragma unroll
  for (int im = 0; im < 2; ++im)
#pragma unroll
    for (int in = 0; in < 2; ++in) {
      const int col = n0 + wn + 32 * in + j;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = m0 + wm + 32 * im + (q & 3) + 8 * (q >> 2) + 4 * h;
        float v = acc[0][im][in][q];
        if (NACC == 2) v += acc[NACC - 1][im][in][q];
        if (row < g.M && col < g.N) out[(size_t)row * g.N + col] = v * g.scale;
      }
    }
}

template <bool AT, bool BT, int NT, bool SEP, bool SQ>
int tall_gemm_launch(const TallGemm& g, int splits, bool al, hipStream_t st) {
  const dim3 grid((unsigned)tiles_of(g.N), (unsigned)tiles_of(g.M), (unsigned)splits);
  if (al)
    k_tall_gemm<AT, BT, NT, SEP, SQ, true><<<grid, BLOCK, 0, st>>>(g);
  else
    k_tall_gemm<AT, BT, NT, SEP, SQ, false><<<grid, BLOCK, 0, st>>>(g);
  return (int)hipGetLastError();
}

// ---- finishing pass of a split W GEMM: out = scale * (slab 0 + slabs 1 .. n-1 in split order) ---------------------
__global__ __launch_bounds__(BLOCK) void k_tall_slab_finish(float* __restrict__ out, const float* __restrict__ slabs,
                                                            int splits, long long stride, float scale, int total) {
  const int idx = blockIdx.x * BLOCK + threadIdx.x;
  if (idx >= total) return;
  out[idx] = slab_sum<4>(slabs[idx], slabs, idx, splits, stride) * scale;
}

// ---- row reductions over [rows, c] -----------------------------------------------------------------------------------
// grid (ceil(c / 64), row_blocks), 256 threads: thread (cx = t & 63, ry = t >> 6) walks rows r_lo + ry, + 4, ... of its
// block in ascending order, one column; its fp64 sum joins the three others as ((s0 + s1) + s2) + s3 -> ws[block][col].
__device__ __forceinline__ void col_partial(double sum, double* __restrict__ ws, int col, int c) {
  __shared__ double red[WAVES][COLS_PER_BLOCK];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  red[ry][cx] = sum;
  __syncthreads();
  if (ry == 0 && col < c) ws[(size_t)blockIdx.y * c + col] = ((red[0][cx] + red[1][cx]) + red[2][cx]) + red[3][cx];
}

// g_a = k_dense_act_adjoint's entry (hf_dense_act.h: act_adjoint_value); the column sums of g_a leave as fp64 partials
template <bool CURV>
__global__ __launch_bounds__(BLOCK) void k_tall_act_adjoint(float* __restrict__ ga, double* __restrict__ ws,
                                                            const float* __restrict__ slabs, int splits, long long stride,
                                                            const float* __restrict__ y, int act,
                                                            const float* __restrict__ ty, const float* __restrict__ h1,
                                                            int rows, int c, int rows_per_block) {
  const int col = blockIdx.x * COLS_PER_BLOCK + (threadIdx.x & 63);
  const int r_lo = blockIdx.y * rows_per_block, r_hi = min(r_lo + rows_per_block, rows);
  double sum = 0.0;
  if (col < c)
    for (int r = r_lo + (threadIdx.x >> 6); r < r_hi; r += WAVES) {
      const int idx = r * c + col;
      const float gv = act_adjoint_value<CURV>(slabs, idx, splits, stride, y, act, ty, h1);
      ga[idx] = gv;
      sum += (double)gv;
    }
  if (ws) col_partial(sum, ws, col, c);  // (uniform: every thread of the grid takes the same branch)
}

// the same walk on squares (exact in fp64)
__global__ __launch_bounds__(BLOCK) void k_tall_sq_colsum(double* __restrict__ ws, const float* __restrict__ ga, int rows,
                                                          int c, int rows_per_block) {
  const int col = blockIdx.x * COLS_PER_BLOCK + (threadIdx.x & 63);
  const int r_lo = blockIdx.y * rows_per_block, r_hi = min(r_lo + rows_per_block, rows);
  double sum = 0.0;
  if (col < c)
    for (int r = r_lo + (threadIdx.x >> 6); r < r_hi; r += WAVES) {
      const double gv = (double)ga[r * c + col];
      sum += gv * gv;
    }
  col_partial(sum, ws, col, c);
}

// out[col] = (float)(partials of row blocks 0 .. n-1 added in ascending order in fp64) * scale
__global__ __launch_bounds__(BLOCK) void k_tall_colsum_finish(float* __restrict__ out, const double* __restrict__ ws,
                                                              int row_blocks, int c, float scale) {
  const int col = blockIdx.x * BLOCK + threadIdx.x;
  if (col >= c) return;
  double sum = 0.0;
  for (int b = 0; b < row_blocks; ++b) sum += ws[(size_t)b * c + col];
  out[col] = (float)sum * scale;
}

inline bool ws_ok(const void* ws) { return ws && (((uintptr_t)ws) & 7) == 0; }

}  // namespace

extern "C" {

int hf_dense_tall_plan(int64_t rows, int64_t c_in, int64_t c_out, int* splits_t, int* splits_d, int* splits_w,
                       int* row_blocks) {
  TallPlan p;
  if (!splits_t || !splits_d || !splits_w || !row_blocks) return HF_ERR_ARG;
  const int rc = tall_plan(rows, c_in, c_out, &p);
  if (rc != HF_OK) return rc;
  *splits_t = p.splits_t;
  *splits_d = p.splits_d;
  *splits_w = p.splits_w;
  *row_blocks = p.row_blocks;
  return HF_OK;
}

int hf_dense_tall_tangent_slabs(void* out_slabs, const void* t_x, const void* x, const void* W, const void* V,
                                int64_t rows, int64_t c_in, int64_t c_out, int64_t ld_x, int splits, int64_t slab_stride,
                                int dtype, void* stream) {
  TallPlan p;
  if (tall_plan(rows, c_in, c_out, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out_slabs) return HF_ERR_ARG;
  if (!t_x && !V) return HF_ERR_ARG;           // nothing to compute
  if ((t_x && !W) || (V && !x)) return HF_ERR_ARG;
  if (ld_x == 0) ld_x = c_in;
  if (ld_x < c_in || ld_x > DENSE_MAX_C || rows * ld_x >= TALL_MAX_ELEMS) return HF_ERR_ARG;
  if (!tall_split_ok(c_in, splits)) return HF_ERR_ARG;
  if (splits > 1 && slab_stride < rows * c_out) return HF_ERR_ARG;
  const bool al = (!t_x || (quad_ok(t_x, ld_x) && quad_ok(W, c_in))) && (!V || (quad_ok(x, ld_x) && quad_ok(V, c_in)));
  TallGemm g = {};
  g.out = (float*)out_slabs;
  int nt = 0;
  if (t_x) g.a[nt] = (const float*)t_x, g.b[nt++] = (const float*)W;
  if (V) g.a[nt] = (const float*)x, g.b[nt++] = (const float*)V;
  g.M = (int)rows, g.N = (int)c_out, g.K = (int)c_in, g.ld_a = (int)ld_x, g.ld_b = (int)c_in;
  g.kper = (int)tall_kper(c_in, splits), g.slab_stride = (long long)slab_stride, g.scale = 1.0f;
  hipStream_t st = (hipStream_t)stream;
  return nt == 2 ? tall_gemm_launch<true, true, 2, false, false>(g, splits, al, st)
                 : tall_gemm_launch<true, true, 1, false, false>(g, splits, al, st);
}

int hf_dense_tall_dgrad_slabs(void* out_slabs, const void* g_a, const void* W, const void* g2, const void* V, int64_t rows,
                              int64_t c_in, int64_t c_out, int splits, int64_t slab_stride, int dtype, void* stream) {
  TallPlan p;
  if (tall_plan(rows, c_in, c_out, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out_slabs || !g_a || !W) return HF_ERR_ARG;
  if ((g2 != nullptr) != (V != nullptr)) return HF_ERR_ARG;  // the second term needs both operands
  if (!tall_split_ok(c_out, splits)) return HF_ERR_ARG;
  if (splits > 1 && slab_stride < rows * c_in) return HF_ERR_ARG;
  const bool two = g2 != nullptr;
  const bool al = quad_ok(g_a, c_out) && quad_ok(W, c_in) && (!two || (quad_ok(g2, c_out) && quad_ok(V, c_in)));
  TallGemm g = {};
  g.out = (float*)out_slabs;
  g.a[0] = (const float*)g_a, g.b[0] = (const float*)W, g.a[1] = (const float*)g2, g.b[1] = (const float*)V;
  g.M = (int)rows, g.N = (int)c_in, g.K = (int)c_out, g.ld_a = (int)c_out, g.ld_b = (int)c_in;
  g.kper = (int)tall_kper(c_out, splits), g.slab_stride = (long long)slab_stride, g.scale = 1.0f;
  hipStream_t st = (hipStream_t)stream;
  return two ? tall_gemm_launch<true, false, 2, false, false>(g, splits, al, st)
             : tall_gemm_launch<true, false, 1, false, false>(g, splits, al, st);
}

int hf_dense_tall_wgrad(void* out, void* ws, const void* g1, const void* x1, const void* g2, const void* x2, int64_t rows,
                        int64_t c_in, int64_t c_out, int mode, double scale, int splits, int dtype, void* stream) {
  TallPlan p;
  if (tall_plan(rows, c_in, c_out, &p) != HF_OK) return HF_ERR_ARG;
  if (dtype != HF_F32 || !out || !g1 || !x1) return HF_ERR_ARG;
  if (mode < 0 || mode > 2) return HF_ERR_ARG;
  if (mode == 2 && (!g2 || !x2)) return HF_ERR_ARG;
  if (!(scale == scale)) return HF_ERR_ARG;
  if (!tall_split_ok(rows, splits)) return HF_ERR_ARG;
  if (splits > 1 && !ws) return HF_ERR_ARG;
  const bool two = mode == 2;
  const bool al = quad_ok(g1, c_out) && quad_ok(x1, c_in) && (!two || (quad_ok(g2, c_out) && quad_ok(x2, c_in)));
  const int64_t total = c_out * c_in;
  TallGemm g = {};
  g.out = splits > 1 ? (float*)ws : (float*)out;
  g.a[0] = (const float*)g1, g.b[0] = (const float*)x1, g.a[1] = (const float*)g2, g.b[1] = (const float*)x2;
  g.M = (int)c_out, g.N = (int)c_in, g.K = (int)rows, g.ld_a = (int)c_out, g.ld_b = (int)c_in;
  g.kper = (int)tall_kper(rows, splits), g.slab_stride = (long long)total;
  g.scale = splits > 1 ? 1.0f : (float)scale;  // (a split GEMM leaves plain sums: the finishing pass scales)
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (mode == 0) rc = tall_gemm_launch<false, false, 1, false, false>(g, splits, al, st);
  else if (mode == 1) rc = tall_gemm_launch<false, false, 1, false, true>(g, splits, al, st);
  else rc = tall_gemm_launch<false, false, 2, true, false>(g, splits, al, st);
  if (rc != 0 || splits == 1) return rc;
  k_tall_slab_finish<<<(unsigned)((total + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>((float*)out, (const float*)ws, splits,
                                                                               (long long)total, (float)scale, (int)total);
  return (int)hipGetLastError();
}

int hf_dense_tall_act_forward(void* y, const void* slabs, int splits, int64_t slab_stride, const void* b, int act,
                              int64_t rows, int64_t c, int dtype, void* stream) {
  return dense_act_forward_launch(y, slabs, splits, slab_stride, b, act, rows, c, dtype, stream, TALL_MIN_ROWS,
                                  TALL_MAX_ROWS);
}

int hf_dense_tall_act_tangent(void* t_y, const void* slabs, int splits, int64_t slab_stride, const void* v_b,
                              const void* y, int act, int64_t rows, int64_t c, int dtype, void* stream) {
  return dense_act_tangent_launch(t_y, slabs, splits, slab_stride, v_b, y, act, rows, c, dtype, stream, TALL_MIN_ROWS,
                                  TALL_MAX_ROWS);
}

int hf_dense_tall_act_adjoint(void* g_a, void* g_b_out, void* ws, const void* slabs, int splits, int64_t slab_stride,
                              const void* y, int act, const void* t_y, const void* h, int64_t rows, int64_t c,
                              double scale, int dtype, void* stream) {
  if (!g_a || !act_args_in(slabs, splits, slab_stride, y, act, rows, c, dtype, TALL_MIN_ROWS, TALL_MAX_ROWS))
    return HF_ERR_ARG;
  if (rows * c >= TALL_MAX_ELEMS) return HF_ERR_ARG;
  if ((t_y != nullptr) != (h != nullptr)) return HF_ERR_ARG;  // the curvature term needs both
  if (g_b_out && !ws_ok(ws)) return HF_ERR_ARG;
  if (!(scale == scale)) return HF_ERR_ARG;
  const int per = tall_rows_per_block(rows, c), blocks = tall_row_blocks(rows, c);
  const dim3 grid((unsigned)((c + COLS_PER_BLOCK - 1) / COLS_PER_BLOCK), (unsigned)blocks);
  double* part = g_b_out ? (double*)ws : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (t_y && act == ACT_TANH)  // (identity and relu have no curvature term)
    k_tall_act_adjoint<true><<<grid, BLOCK, 0, st>>>((float*)g_a, part, (const float*)slabs, splits,
                                                     (long long)slab_stride, (const float*)y, act, (const float*)t_y,
                                                     (const float*)h, (int)rows, (int)c, per);
  else
    k_tall_act_adjoint<false><<<grid, BLOCK, 0, st>>>((float*)g_a, part, (const float*)slabs, splits,
                                                      (long long)slab_stride, (const float*)y, act, nullptr, nullptr,
                                                      (int)rows, (int)c, per);
  HF_HIP(hipGetLastError());
  if (!g_b_out) return HF_OK;
  k_tall_colsum_finish<<<(unsigned)((c + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>((float*)g_b_out, (const double*)ws, blocks,
                                                                             (int)c, (float)scale);
  return (int)hipGetLastError();
}

int hf_dense_tall_sq_colsum(void* out, void* ws, const void* g_a, int64_t rows, int64_t c, double scale, int dtype,
                            void* stream) {
  if (rows < TALL_MIN_ROWS || rows > TALL_MAX_ROWS || c < 1 || c > DENSE_MAX_C || rows * c >= TALL_MAX_ELEMS)
    return HF_ERR_ARG;
  if (dtype != HF_F32 || !out || !g_a || !ws_ok(ws)) return HF_ERR_ARG;
  if (!(scale == scale)) return HF_ERR_ARG;
  const int per = tall_rows_per_block(rows, c), blocks = tall_row_blocks(rows, c);
  const dim3 grid((unsigned)((c + COLS_PER_BLOCK - 1) / COLS_PER_BLOCK), (unsigned)blocks);
  hipStream_t st = (hipStream_t)stream;
  k_tall_sq_colsum<<<grid, BLOCK, 0, st>>>((double*)ws, (const float*)g_a, (int)rows, (int)c, per);
  HF_HIP(hipGetLastError());
  k_tall_colsum_finish<<<(unsigned)((c + BLOCK - 1) / BLOCK), BLOCK, 0, st>>>((float*)out, (const double*)ws, blocks,
                                                                             (int)c, (float)scale);
  return (int)hipGetLastError();
}

}  // extern "C"
