// Host-only check of hf_dense_tall.hip's planner and argument validators (the pattern of dense_plan_host_check.cpp): no
// kernel is launched -- accepted shapes only go through hf_dense_tall_plan, every launching call below must be refused
// before it reaches the device.  Build with the host half of the translation unit instrumented and run on any machine:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//       scripts/dense_tall_plan_host_check.cpp pytorchhessianfree_amd/csrc/hf_dense_tall.hip -o dense_tall_plan_host_check
//
// Exit status 0 and no sanitizer report = pass.
#include <cstdio>

#include "hf_pcg.h"

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static bool split_ok(long long len, int splits) {
  if (splits < 1 || splits > 32) return false;
  const long long per = (len + splits - 1) / splits, kper = (per + 15) / 16 * 16;
  return (splits - 1) * kper < len;
}

int main() {
  float b[4] = {0, 0, 0, 0};
  alignas(8) double w[4] = {0, 0, 0, 0};
  int st, sd, sw, rb;
  // every row count of the range against the split rule, over widths around the tile and the step
  static const long long widths[] = {1, 4, 15, 16, 17, 127, 128, 129, 260, 1000, 3072, 4096, 65536};
  for (long long rows = 257; rows <= 8192; ++rows)
    for (long long ci : widths)
      for (long long co : widths) {
        if (ci * co >= (1LL << 31)) {  // (an operand the kernels' int indices cannot address)
          EXPECT(hf_dense_tall_plan(rows, ci, co, &st, &sd, &sw, &rb) == HF_ERR_ARG);
          continue;
        }
        EXPECT(hf_dense_tall_plan(rows, ci, co, &st, &sd, &sw, &rb) == HF_OK);
        EXPECT(split_ok(ci, st) && split_ok(co, sd) && split_ok(rows, sw));
        const long long per = (rows + rb - 1) / rb;  // no row block may be empty
        EXPECT(rb >= 1 && rb <= 64 && (rb - 1) * per < rows);
      }
  // refused split counts never reach a launch
  for (long long len : {1LL, 15LL, 16LL, 17LL, 32LL, 33LL, 260LL, 3072LL})
    for (int sp = -1; sp <= 34; ++sp)
      if (!split_ok(len, sp)) {
        EXPECT(hf_dense_tall_tangent_slabs(b, b, b, b, b, 300, len, 1, 0, sp, 1 << 20, HF_F32, nullptr) == HF_ERR_ARG);
        EXPECT(hf_dense_tall_dgrad_slabs(b, b, b, b, b, 300, 1, len, sp, 1 << 20, HF_F32, nullptr) == HF_ERR_ARG);
      }
  for (int sp = -1; sp <= 34; ++sp)
    if (!split_ok(300, sp)) EXPECT(hf_dense_tall_wgrad(b, b, b, b, b, b, 300, 4, 4, 0, 1.0, sp, HF_F32, nullptr) == HF_ERR_ARG);
  // sizes outside the range: rows, widths, an operand of 2^31 elements or more
  static const long long bad[][3] = {{0, 4, 4},   {256, 4, 4},           {8193, 4, 4},          {300, 0, 4},
                                     {300, 4, 0}, {300, (1 << 20) + 1, 4}, {300, 4, (1 << 20) + 1}, {8192, 1 << 18, 4},
                                     {8192, 4, 1 << 18}, {300, 1 << 16, 1 << 15}, {-1, 4, 4}};
  for (const auto& s : bad) {
    EXPECT(hf_dense_tall_plan(s[0], s[1], s[2], &st, &sd, &sw, &rb) == HF_ERR_ARG);
    EXPECT(hf_dense_tall_tangent_slabs(b, b, b, b, b, s[0], s[1], s[2], 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_tall_dgrad_slabs(b, b, b, b, b, s[0], s[1], s[2], 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_tall_wgrad(b, b, b, b, b, b, s[0], s[1], s[2], 0, 1.0, 1, HF_F32, nullptr) == HF_ERR_ARG);
  }
  for (long long rows : {0LL, 256LL, 8193LL}) {
    EXPECT(hf_dense_tall_act_forward(b, b, 1, 0, b, 1, rows, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_tall_act_tangent(b, b, 1, 0, b, b, 1, rows, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_tall_act_adjoint(b, b, w, b, 1, 0, b, 1, b, b, rows, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_tall_sq_colsum(b, w, b, rows, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  }
  EXPECT(hf_dense_tall_plan(300, 4, 4, nullptr, &sd, &sw, &rb) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_plan(300, 4, 4, &st, &sd, &sw, nullptr) == HF_ERR_ARG);
  // operands, dtype, scale, workspace
  EXPECT(hf_dense_tall_tangent_slabs(b, b, b, b, b, 300, 40, 4, 0, 1, 0, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_tangent_slabs(nullptr, b, b, b, b, 300, 40, 4, 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_tangent_slabs(b, nullptr, b, b, nullptr, 300, 40, 4, 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_tangent_slabs(b, b, b, nullptr, b, 300, 40, 4, 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_tangent_slabs(b, b, nullptr, b, b, 300, 40, 4, 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_tangent_slabs(b, b, b, b, b, 300, 40, 4, 39, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_tangent_slabs(b, b, b, b, b, 300, 40, 4, 0, 2, 1199, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_dgrad_slabs(b, b, b, b, nullptr, 300, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_dgrad_slabs(b, b, b, nullptr, b, 300, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_dgrad_slabs(b, nullptr, b, nullptr, nullptr, 300, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_dgrad_slabs(b, b, b, nullptr, nullptr, 300, 4, 40, 2, 1199, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_wgrad(b, nullptr, b, b, nullptr, nullptr, 300, 4, 4, 0, 1.0, 2, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_wgrad(b, b, b, b, b, nullptr, 300, 4, 4, 2, 1.0, 1, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_wgrad(b, b, b, b, b, b, 300, 4, 4, 3, 1.0, 1, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_wgrad(b, b, b, b, b, b, 300, 4, 4, 0, 0.0 / 0.0, 1, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_wgrad(b, b, b, b, b, b, 300, 4, 4, 0, 1.0, 1, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_act_adjoint(b, b, nullptr, b, 1, 0, b, 1, nullptr, nullptr, 300, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_act_adjoint(b, b, (char*)w + 4, b, 1, 0, b, 1, nullptr, nullptr, 300, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_act_adjoint(b, nullptr, nullptr, b, 1, 0, b, 2, b, nullptr, 300, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_act_adjoint(b, nullptr, nullptr, b, 1, 0, nullptr, 2, nullptr, nullptr, 300, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_act_adjoint(b, nullptr, nullptr, b, 2, 1199, b, 1, nullptr, nullptr, 300, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_sq_colsum(b, nullptr, b, 300, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tall_sq_colsum(b, w, b, 300, 4, 0.0 / 0.0, HF_F32, nullptr) == HF_ERR_ARG);
  std::printf(failures ? "%d check(s) failed\n" : "dense tall plan / validator host check: ok\n", failures);
  return failures ? 1 : 0;
}
