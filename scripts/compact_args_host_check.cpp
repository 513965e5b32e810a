// Host-only check of the argument filling of the compact gather / scatter: hf_unpack.h's fill_unpack_args with a
// `compact` array, and the refusals of hf_pack_compact, hf_unpack_weights_compact, hf_live_copy_rows and
// hf_live_dead_check.  No kernel is launched: every launching call below must be refused before it reaches the device.
// Build with the host half of the translation units instrumented and run on any machine, GPU or not:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Ipytorchhessianfree_amd/csrc -Xarch_host \
//       -fsanitize=address,undefined scripts/compact_args_host_check.cpp pytorchhessianfree_amd/csrc/hf_pack.hip \
//       -o compact_args_host_check
//
// Exit status 0 and no sanitizer report = pass.
#include <cstdio>
#include <cstdlib>

#include "hf_pcg.h"
#include "hf_unpack.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

int main() {
  using hf_shared::UnpackArgs;
  const int64_t CENTRE = 1 << 4, CORNER = 0x1b0;
  float dummy[4];
  // ---- fill_unpack_args: three tensors [3, 8, 3, 3] NHWC (centre, corner, unmasked) and one [3, 8, 1, 1] ----
  {
    void* dsts[4] = {dummy, dummy, dummy, dummy};
    const int64_t offs[4] = {0, 24, 120, 336}, numels[4] = {216, 216, 216, 24}, slabs[4] = {72, 72, 72, 8};
    const int64_t inners[4] = {8, 8, 8, 0}, live[4] = {CENTRE, CORNER, 0, 0}, halves[4] = {1, 1, 0, 1};
    const int64_t compact[4] = {1, 4, 0, 0};
    UnpackArgs a;
    int blocks = -1;
    int next = hf_shared::fill_unpack_args<float>(a, &blocks, 0, dsts, offs, numels, slabs, inners, live, halves, compact,
                                                  4, true);
    EXPECT(next == 4 && a.nt == 4 && blocks == 4);
    EXPECT(a.cnl[0] == 1 && a.cnl[1] == 4 && a.cnl[2] == 0 && a.cnl[3] == 0);
    EXPECT(a.live[0] == CENTRE && a.live[1] == CORNER && a.src_off[1] == 24 && a.numel[1] == 216);
    // without the array: the flat layout
    next = hf_shared::fill_unpack_args<float>(a, &blocks, 0, dsts, offs, numels, slabs, inners, live, halves, nullptr, 4,
                                              true);
    EXPECT(next == 4 && a.cnl[0] == 0 && a.cnl[1] == 0);
    // a period that is not the mask's popcount; a period without a mask; a period on an NCHW destination; on half 2
    const int64_t wrong[4] = {2, 4, 0, 0}, nomask[4] = {1, 4, 9, 0}, nchw[4] = {1, 4, 0, 1};
    EXPECT(hf_shared::fill_unpack_args<float>(a, &blocks, 0, dsts, offs, numels, slabs, inners, live, halves, wrong, 4,
                                              true) == HF_ERR_ARG);
    EXPECT(hf_shared::fill_unpack_args<float>(a, &blocks, 0, dsts, offs, numels, slabs, inners, live, halves, nomask, 4,
                                              true) == HF_ERR_ARG);
    EXPECT(hf_shared::fill_unpack_args<float>(a, &blocks, 0, dsts, offs, numels, slabs, inners, live, halves, nchw, 4,
                                              true) == HF_ERR_ARG);
    const int64_t transposed[4] = {2, 1, 0, 1};
    EXPECT(hf_shared::fill_unpack_args<float>(a, &blocks, 0, dsts, offs, numels, slabs, inners, live, transposed, compact,
                                              4, true) == HF_ERR_ARG);
    // the C entry point refuses the same before any launch
    EXPECT(hf_unpack_weights_compact(dummy, dsts, offs, numels, slabs, inners, live, halves, wrong, 4, HF_F32, nullptr) ==
           HF_ERR_ARG);
    EXPECT(hf_unpack_weights_compact(nullptr, dsts, offs, numels, slabs, inners, live, halves, compact, 4, HF_F32,
                                     nullptr) == HF_ERR_ARG);
  }
  // ---- more tensors than one table holds: the second call continues where the first stopped ----
  {
    const int n = hf_shared::PACK_MAXT + 20;  // (every fifth tensor is empty: 67 non-empty ones)
    void** dsts = (void**)std::malloc(n * sizeof(void*));
    int64_t* cols = (int64_t*)std::malloc(7 * n * sizeof(int64_t));
    int64_t *offs = cols, *numels = cols + n, *slabs = cols + 2 * n, *inners = cols + 3 * n, *live = cols + 4 * n,
            *halves = cols + 5 * n, *compact = cols + 6 * n;
    for (int t = 0; t < n; ++t) {
      dsts[t] = dummy;
      offs[t] = 24 * t, numels[t] = (t % 5 == 2) ? 0 : 216, slabs[t] = 72, inners[t] = 8, live[t] = CENTRE;
      halves[t] = t & 1, compact[t] = 1;
    }
    UnpackArgs a;
    int blocks = 0;
    const int next = hf_shared::fill_unpack_args<float>(a, &blocks, 0, dsts, offs, numels, slabs, inners, live, halves,
                                                        compact, n, true);
    EXPECT(next > 0 && next < n && a.nt == hf_shared::PACK_MAXT && a.cnl[hf_shared::PACK_MAXT - 1] == 1);
    const int last = hf_shared::fill_unpack_args<float>(a, &blocks, next, dsts, offs, numels, slabs, inners, live, halves,
                                                        compact, n, true);
    EXPECT(last == n && a.nt >= 1 && a.cnl[a.nt - 1] == 1 && a.cnl[a.nt] == 0);
    std::free(dsts);
    std::free(cols);
  }
  // ---- hf_pack_compact, hf_live_copy_rows, hf_live_dead_check: refusals ----
  {
    const void* srcs[1] = {dummy};
    const int64_t numels[1] = {216}, perm[2] = {8, 9}, splits[2] = {1, 0};
    const int64_t live_c[1] = {CENTRE}, live_0[1] = {0};
    const int64_t two[1] = {2}, one[1] = {1};
    EXPECT(hf_pack_compact(dummy, srcs, numels, perm, splits, live_c, two, 1, 1.0, 0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_pack_compact(dummy, srcs, numels, perm, splits, live_0, one, 1, 1.0, 0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_pack_compact(dummy, srcs, numels, nullptr, splits, live_c, one, 1, 1.0, 0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_pack_compact(nullptr, srcs, numels, perm, splits, live_c, one, 1, 1.0, 0, HF_F32, nullptr) == HF_ERR_ARG);
    const int64_t foffs[2] = {0, 216}, counts[2] = {216, 7}, periods[2] = {9, 0}, masks[2] = {CENTRE, 0};
    const int64_t bad_counts[2] = {215, 7}, bad_periods[2] = {17, 0}, no_taps[2] = {0, 0};
    int flag = 0;
    EXPECT(hf_live_copy_rows(dummy, dummy, 0, 0, 0, 0, foffs, counts, periods, masks, 2, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_live_copy_rows(dummy, dummy, 0, 2, 223, 30, foffs, counts, periods, masks, 2, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_live_copy_rows(dummy, dummy, 0, 1, 0, 0, foffs, bad_counts, periods, masks, 2, HF_F32, nullptr) ==
           HF_ERR_ARG);
    EXPECT(hf_live_copy_rows(dummy, dummy, 0, 1, 0, 0, foffs, counts, bad_periods, masks, 2, HF_F32, nullptr) ==
           HF_ERR_ARG);
    EXPECT(hf_live_copy_rows(dummy, dummy, 0, 1, 0, 0, foffs, counts, periods, no_taps, 2, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_live_copy_rows(dummy, dummy, 0, 1, 0, 0, foffs, counts, periods, masks, 25, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_live_dead_check(nullptr, nullptr, &flag, foffs, counts, periods, masks, 2, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_live_dead_check(dummy, nullptr, nullptr, foffs, counts, periods, masks, 2, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_live_dead_check(dummy, nullptr, &flag, foffs, bad_counts, periods, masks, 2, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_live_dead_check(dummy, nullptr, &flag, foffs, counts, periods, masks, 2, 7, nullptr) == HF_ERR_ARG);
  }
  std::printf(failures ? "%d check(s) failed\n" : "compact argument filling: all checks passed\n", failures);
  return failures ? 1 : 0;
}
