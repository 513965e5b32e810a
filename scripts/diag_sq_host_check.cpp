// Host-only check of the squared-sum entry points' planner and argument validators (hf_conv2d_nhwc_sqsum_plan,
// hf_conv2d_nhwc_sqsum_slabs in hf_conv.hip; hf_chan_sqsum in hf_bn.hip): no kernel is launched -- accepted problems only
// go through the planner, every launching call below must be refused before it reaches the device.  Build with the host
// half of the translation units instrumented and run on any machine, GPU or not:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//       scripts/diag_sq_host_check.cpp pytorchhessianfree_amd/csrc/hf_conv.hip pytorchhessianfree_amd/csrc/hf_bn.hip \
//       -o diag_sq_host_check
//
// Exit status 0 and no sanitizer report = pass.
#include <cstdio>
#include <cstdlib>

#include "hf_pcg.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// the rule of the header: split s takes samples [s * ceil(n / splits), ...), none of them empty
static bool shares_ok(long long n, long long splits) {
  return splits >= 1 && splits <= n && ((n + splits - 1) / splits) * (splits - 1) < n;
}

int main() {
  // (n, h, w, c, k, r, s, stride, pad): the exact tests' cases, the engines' layers, large batches
  static const long long geo[][9] = {
      {3, 8, 8, 8, 8, 3, 3, 1, 1},     {5, 5, 5, 12, 20, 3, 3, 1, 1},   {4, 7, 7, 4, 36, 3, 3, 2, 1},
      {6, 2, 2, 8, 8, 3, 3, 1, 1},     {2, 16, 16, 4, 8, 3, 3, 1, 1},   {8, 4, 4, 64, 128, 1, 1, 1, 0},
      {37, 1, 1, 16, 24, 3, 3, 1, 1},  {9, 1, 1, 8, 8, 1, 1, 1, 0},     {4, 8, 8, 3, 8, 3, 3, 1, 1},
      {4, 5, 5, 12, 8, 1, 1, 1, 0},    {32, 28, 28, 52, 64, 1, 1, 1, 0}, {32, 7, 7, 64, 64, 3, 3, 1, 1},
      {32, 1, 1, 512, 512, 3, 3, 1, 1}, {256, 32, 32, 96, 96, 3, 3, 1, 1}, {128, 8, 8, 192, 100, 1, 1, 1, 0},
      {1, 4, 4, 8, 8, 3, 3, 1, 1},     {4096, 1, 1, 8, 8, 1, 1, 1, 0},  {1000, 2, 2, 4, 4, 3, 3, 1, 1}};
  for (const auto& g : geo)
    for (int target : {0, 1, 7, 64, 256, 1024, 1 << 20}) {
      const int sp = hf_conv2d_nhwc_sqsum_plan(g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[7], g[8], g[8], target);
      EXPECT(sp >= 1 && shares_ok(g[0], sp));
      if (target == 1) EXPECT(sp == 1);
    }
  static const long long bad[][9] = {{0, 4, 4, 8, 8, 3, 3, 1, 1},  {-1, 4, 4, 8, 8, 3, 3, 1, 1}, {2, 0, 4, 8, 8, 3, 3, 1, 1},
                                     {2, 4, 4, 0, 8, 3, 3, 1, 1},  {2, 4, 4, 8, 0, 3, 3, 1, 1},  {2, 4, 4, 8, 8, 0, 3, 1, 1},
                                     {2, 4, 4, 8, 8, 9, 9, 1, 4},  {2, 2, 2, 8, 8, 3, 3, 1, 0},  {2, 4, 4, 8, 8, 3, 3, 0, 1},
                                     {2, 4, 4, 8, 8, 3, 3, 1, -1}};
  alignas(16) float b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (const auto& g : bad) {
    EXPECT(hf_conv2d_nhwc_sqsum_plan(g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[7], g[8], g[8], 0) == HF_ERR_ARG);
    EXPECT(hf_conv2d_nhwc_sqsum_slabs(b, b, b, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[7], g[8], g[8], 0, 0, 1.f,
                                      1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  }
  // every split count the rule refuses, for batch sizes around the shares' edges: refused by both launching entry points
  for (long long n : {1LL, 2LL, 3LL, 5LL, 8LL, 9LL, 16LL, 37LL, 100LL, 256LL})
    for (int sp = -1; sp <= n + 2; ++sp)
      if (!shares_ok(n, sp)) {
        EXPECT(hf_conv2d_nhwc_sqsum_slabs(b, b, b, n, 4, 4, 8, 8, 3, 3, 1, 1, 1, 1, 0, 0, 1.f, sp, 1 << 20, HF_F32,
                                          nullptr) == HF_ERR_ARG);
        EXPECT(hf_chan_sqsum(b, b, b, b, b, b, n, 8, 4, 1.f, sp, HF_F32, nullptr) == HF_ERR_ARG);
      }
  const float nan = 0.0f / 0.0f, inf = 1.0f / 0.0f;
#define SQ(out, act, mat, act_ld, out_c, pre, sp, stride, dt) \
  hf_conv2d_nhwc_sqsum_slabs(out, act, mat, 4, 4, 4, 8, 8, 3, 3, 1, 1, 1, 1, act_ld, out_c, pre, sp, stride, dt, nullptr)
  EXPECT(SQ(nullptr, b, b, 0, 0, 1.f, 1, 0, HF_F32) == HF_ERR_ARG);
  EXPECT(SQ(b, nullptr, b, 0, 0, 1.f, 1, 0, HF_F32) == HF_ERR_ARG);
  EXPECT(SQ(b, b, nullptr, 0, 0, 1.f, 1, 0, HF_F32) == HF_ERR_ARG);
  EXPECT(SQ(b + 1, b, b, 0, 0, 1.f, 1, 0, HF_F32) == HF_ERR_ALIGN);
  EXPECT(SQ(b, b + 1, b, 0, 0, 1.f, 1, 0, HF_F32) == HF_ERR_ALIGN);
  EXPECT(SQ(b, b, b + 1, 0, 0, 1.f, 1, 0, HF_F32) == HF_ERR_ALIGN);
  EXPECT(SQ(b, b, b, 4, 0, 1.f, 1, 0, HF_F32) == HF_ERR_ARG);    // act_ld < c
  EXPECT(SQ(b, b, b, -1, 0, 1.f, 1, 0, HF_F32) == HF_ERR_ARG);
  EXPECT(SQ(b, b, b, 0, 9, 1.f, 1, 0, HF_F32) == HF_ERR_ARG);    // out_c > c
  EXPECT(SQ(b, b, b, 0, -1, 1.f, 1, 0, HF_F32) == HF_ERR_ARG);
  EXPECT(SQ(b, b, b, 0, 0, nan, 1, 0, HF_F32) == HF_ERR_ARG);
  EXPECT(SQ(b, b, b, 0, 0, inf, 1, 0, HF_F32) == HF_ERR_ARG);
  EXPECT(SQ(b, b, b, 0, 0, 1.f, 2, 8 * 9 * 8 - 1, HF_F32) == HF_ERR_ARG);  // slabs would overlap
  EXPECT(SQ(b, b, b, 0, 0, 1.f, 2, -1, HF_F32) == HF_ERR_ARG);
  EXPECT(SQ(b, b, b, 0, 0, 1.f, 1, 0, HF_F64) == HF_ERR_ARG);
#undef SQ
#define CH(gw2, gb2, g, x, mean, rstd, n, c, hw, pre, rb, dt) \
  hf_chan_sqsum(gw2, gb2, g, x, mean, rstd, n, c, hw, pre, rb, dt, nullptr)
  EXPECT(CH(nullptr, nullptr, b, b, b, b, 4, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);   // no output
  EXPECT(CH(b, b, nullptr, b, b, b, 4, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, nullptr, nullptr, nullptr, 4, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);  // the scale's entry needs xhat
  EXPECT(CH(nullptr, b, b, b, nullptr, b, 4, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);    // x, mean, rstd: all or none
  EXPECT(CH(nullptr, b, b, b, b, nullptr, 4, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(nullptr, b, b, nullptr, b, b, 4, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, 0, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, 4, 0, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, 4, 8, 0, 1.f, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, -4, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, 1LL << 31, 8, 4, 1.f, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, 1 << 20, 8, 1 << 20, 1.f, 1, HF_F32) == HF_ERR_ARG);   // n * hw past 2^31
  EXPECT(CH(b, b, b, b, b, b, 4, 8, 4, nan, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, 4, 8, 4, inf, 1, HF_F32) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, 4, 8, 4, 1.f, 1, HF_F64) == HF_ERR_ARG);
  EXPECT(CH(b, b, b, b, b, b, 1 << 20, 8, 4, 1.f, 1 << 17, HF_F32) == HF_ERR_ARG);    // more shares than a grid's y extent
#undef CH
  for (float v : b) EXPECT(v == 0.f);
  std::printf(failures ? "%d check(s) failed\n" : "squared-sum plan / validator host check: ok\n", failures);
  return failures ? 1 : 0;
}
