// Host-only check of hf_dense.hip's planner and argument validators: no kernel is launched (accepted shapes only go
// through hf_dense_plan; every launching call below must be refused before it reaches the device).  Build with the host
// half of the translation unit instrumented and run on any machine, GPU or not:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Xarch_host -fsanitize=address,undefined \
//       scripts/dense_plan_host_check.cpp pytorchhessianfree_amd/csrc/hf_dense.hip -o dense_plan_host_check
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

static bool split_ok(long long len, int splits) {
  if (splits < 1 || splits > 32) return false;
  const long long per = (len + splits - 1) / splits, kper = (per + 31) / 32 * 32;
  return (splits - 1) * kper < len;
}

int main() {
  static const long long shapes[][3] = {{1, 1, 1},      {3, 7, 5},     {16, 10, 10},     {32, 5, 3},
                                        {33, 65, 31},   {64, 128, 96}, {64, 260, 132},   {65, 64, 64},
                                        {256, 36, 68},  {64, 3072, 4096}, {64, 4096, 3072}, {64, 3072, 100},
                                        {17, 3072, 64}, {256, 1 << 20, 1}, {1, 1, 1 << 20}};
  for (const auto& s : shapes) {
    int st = -1, sd = -1;
    EXPECT(hf_dense_plan(s[0], s[1], s[2], &st, &sd) == HF_OK);
    EXPECT(split_ok(s[1], st) && split_ok(s[2], sd));
  }
  // every count the rule accepts or refuses, over reduction lengths around the 32-entry step
  for (long long len : {1LL, 31LL, 32LL, 33LL, 64LL, 65LL, 260LL, 3072LL, 1LL << 20})
    for (int sp = -1; sp <= 34; ++sp) {
      float dummy[4] = {0, 0, 0, 0};
      // refused counts must come back as HF_ERR_ARG; accepted ones are not launched here
      if (!split_ok(len, sp)) {
        EXPECT(hf_dense_tangent_slabs(dummy, dummy, dummy, dummy, dummy, 1, len, 1, 0, sp, 1 << 20, HF_F32, nullptr) ==
               HF_ERR_ARG);
        EXPECT(hf_dense_dgrad_slabs(dummy, dummy, dummy, 1, 1, len, sp, 1 << 20, HF_F32, nullptr) == HF_ERR_ARG);
        EXPECT(hf_dense_dgrad2_slabs(dummy, dummy, dummy, dummy, dummy, 1, 1, len, sp, 1 << 20, HF_F32, nullptr) ==
               HF_ERR_ARG);
      }
    }
  float b[4] = {0, 0, 0, 0};
  int st, sd;
  static const long long bad[][3] = {{0, 4, 4}, {257, 4, 4}, {4, 0, 4}, {4, 4, 0}, {4, (1 << 20) + 1, 4},
                                     {4, 4, (1 << 20) + 1}, {-1, 4, 4}, {4, -1, 4}, {4, 4, -1}};
  for (const auto& s : bad) {
    EXPECT(hf_dense_plan(s[0], s[1], s[2], &st, &sd) == HF_ERR_ARG);
    EXPECT(hf_dense_tangent_slabs(b, b, b, b, b, s[0], s[1], s[2], 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_dgrad_slabs(b, b, b, s[0], s[1], s[2], 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_wgrad(b, b, b, s[0], s[1], s[2], 1.0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_sq_wgrad(b, b, b, s[0], s[1], s[2], 1.0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_wgrad2(b, b, b, b, b, s[0], s[1], s[2], 1.0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_dgrad2_slabs(b, b, b, b, b, s[0], s[1], s[2], 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
    if (s[1] == 4) {  // (rows, c) = (s[0], s[2]): only where one of THOSE two is out of range
      EXPECT(hf_dense_sq_colsum(b, b, s[0], s[2], 1.0, HF_F32, nullptr) == HF_ERR_ARG);
      EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, b, 2, b, b, s[0], s[2], 1.0, HF_F32, nullptr) == HF_ERR_ARG);
    }
  }
  EXPECT(hf_dense_plan(4, 4, 4, nullptr, &sd) == HF_ERR_ARG);
  EXPECT(hf_dense_plan(4, 4, 4, &st, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tangent_slabs(b, b, b, b, b, 4, 40, 4, 0, 1, 0, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tangent_slabs(nullptr, b, b, b, b, 4, 40, 4, 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tangent_slabs(b, nullptr, b, b, nullptr, 4, 40, 4, 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tangent_slabs(b, b, b, nullptr, b, 4, 40, 4, 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tangent_slabs(b, b, nullptr, b, b, 4, 40, 4, 0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tangent_slabs(b, b, b, b, b, 4, 40, 4, 39, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_tangent_slabs(b, b, b, b, b, 4, 40, 4, 0, 2, 15, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad_slabs(b, b, b, 4, 4, 40, 1, 0, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad_slabs(nullptr, b, b, 4, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad_slabs(b, nullptr, b, 4, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad_slabs(b, b, nullptr, 4, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad_slabs(b, b, b, 4, 4, 40, 2, 15, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad(b, b, b, 4, 4, 4, 1.0, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad(nullptr, b, b, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad(b, nullptr, b, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad(b, b, nullptr, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad(b, b, b, 4, 4, 4, 0.0 / 0.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_wgrad(b, b, b, 4, 4, 4, 1.0, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_wgrad(nullptr, b, b, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_wgrad(b, nullptr, b, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_wgrad(b, b, nullptr, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_wgrad(b, b, b, 4, 4, 4, 0.0 / 0.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_colsum(b, b, 4, 4, 1.0, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_colsum(nullptr, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_colsum(b, nullptr, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_sq_colsum(b, b, 4, 4, 0.0 / 0.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(nullptr, b, 1, 0, b, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, nullptr, 1, 0, b, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 0, 0, b, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 33, 16, b, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 2, 15, b, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 1, 0, b, b, 3, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 1, 0, b, b, -1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 1, 0, b, nullptr, 2, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 1, 0, b, b, 1, 0, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 1, 0, b, b, 1, 257, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 1, 0, b, b, 1, 4, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_tangent(b, b, 1, 0, b, b, 1, 4, 4, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(nullptr, b, b, 1, 0, b, 1, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, nullptr, 1, 0, b, 1, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, b, 0, 0, b, 1, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, b, 2, 15, b, 1, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, b, 1, 0, b, 3, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, b, 1, 0, nullptr, 1, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, b, 1, 0, b, 1, 257, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, b, 1, 0, b, 1, 4, 0, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, b, 1, 0, b, 1, 4, 4, 0.0 / 0.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint(b, b, b, 1, 0, b, 1, 4, 4, 1.0, HF_F64, nullptr) == HF_ERR_ARG);
  // the second-order adjoint sweep: each operand, the dtype, the scale, the split rule, tanh without t_y / h
  EXPECT(hf_dense_wgrad2(b, b, b, b, b, 4, 4, 4, 1.0, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad2(nullptr, b, b, b, b, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad2(b, nullptr, b, b, b, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad2(b, b, nullptr, b, b, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad2(b, b, b, nullptr, b, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad2(b, b, b, b, nullptr, 4, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_wgrad2(b, b, b, b, b, 4, 4, 4, 0.0 / 0.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(b, b, b, b, b, 4, 4, 40, 1, 0, HF_F64, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(nullptr, b, b, b, b, 4, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(b, nullptr, b, b, b, 4, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(b, b, nullptr, b, b, 4, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(b, b, b, nullptr, b, 4, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(b, b, b, b, nullptr, 4, 4, 40, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(b, b, b, b, b, 4, 4, 40, 0, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(b, b, b, b, b, 4, 4, 64, 3, 16, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_dgrad2_slabs(b, b, b, b, b, 4, 4, 40, 2, 15, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(nullptr, b, b, 1, 0, b, 2, b, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, nullptr, 1, 0, b, 2, b, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 0, 0, b, 2, b, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 33, 16, b, 2, b, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 2, 15, b, 2, b, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, b, 3, b, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, nullptr, 1, b, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, b, 2, nullptr, b, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, b, 2, b, nullptr, 4, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, b, 2, b, b, 257, 4, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, b, 2, b, b, 4, 0, 1.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, b, 2, b, b, 4, 4, 0.0 / 0.0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_adjoint2(b, b, b, 1, 0, b, 2, b, b, 4, 4, 1.0, HF_F64, nullptr) == HF_ERR_ARG);
  // the forward activation pass: each operand, the sizes, the split rule, the activation code, the dtype
  EXPECT(hf_dense_act_forward(nullptr, b, 1, 0, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, nullptr, 1, 0, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 0, 0, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 33, 16, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 2, 15, b, 1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 1, 0, b, 3, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 1, 0, b, -1, 4, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 1, 0, b, 1, 0, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 1, 0, b, 1, 257, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 1, 0, b, 1, 4, 0, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_act_forward(b, b, 1, 0, b, 1, 4, 4, HF_F64, nullptr) == HF_ERR_ARG);
  // the loss head, both kinds (0 cross-entropy, 1 mean-squared error): operands, sizes, kind, scales, dtype, workspace
  alignas(8) double w[512];
  long long tg[4] = {0, 0, 0, 0};
  const double nan = 0.0 / 0.0;
  for (int kind = 0; kind <= 1; ++kind) {
    const void* t = kind == 0 ? (const void*)tg : (const void*)b;
    EXPECT(hf_dense_loss_head(kind, nullptr, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, nullptr, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, nullptr, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, nullptr, b, w, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, nullptr, w, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, nullptr, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, (char*)w + 4, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) ==
           HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 0, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 257, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 0, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, (1 << 20) + 1, HF_F32, nullptr) ==
           HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, w, nan, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, w, 1.0, nan, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, w, 1.0, 1.0, nan, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
    EXPECT(hf_dense_loss_head(kind, b, t, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, HF_F64, nullptr) == HF_ERR_ARG);
  }
  EXPECT(hf_dense_loss_head(0, b, tg, nullptr, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_loss_head(0, b, tg, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 1025, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_loss_head(2, b, tg, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
  EXPECT(hf_dense_loss_head(-1, b, tg, b, b, b, b, b, w, 1.0, 1.0, 1.0, 1, 4, HF_F32, nullptr) == HF_ERR_ARG);
  std::printf(failures ? "%d check(s) failed\n" : "dense plan / validator host check: ok\n", failures);
  return failures ? 1 : 0;
}
