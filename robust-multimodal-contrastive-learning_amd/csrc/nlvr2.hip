// NLVR2 fine-tuning: the hard-label softmax cross-entropy of compute_nlvr2 / compute_nlvr2_attack / PGDAttack_nlvr2
// (objectives.py:898-1060, pgd_attack_vilt.py:285-300) with the logged accuracy and change_rate_cross counts (my_metrics.py:30-45).
//
// The head itself (nlvr2_classifier, vilt_module.py:193-200: Linear(2D,2D) - LayerNorm - GELU - Linear(2D,2)) runs on the VQA head
// kernels (vqa.hip) with D = H = 1536, N = 2, ldl = 64.  What is left is tiny: B rows of N = 2 logits.  One workgroup of four waves;
// each wave owns rows w, w + 4, w + 8, ... (one lane per column), so every reduction has a fixed order and nothing uses float
// atomics: loss, counts and dz are bit-reproducible.
#include "rmcl_common.h"
#include "kernels.h"
#include "head_rows.h"
#include "../../include/rmcl.h"

namespace {

#define CE_WAVES 4
#define CE_MAX_N 64

__global__ __launch_bounds__(256) void nlvr2_ce_kernel(const float* __restrict__ logits, int ldl, const int* __restrict__ labels, int B,
                                                       int N, float gscale, const float* __restrict__ gscale_dev, float* __restrict__ dz,
                                                       float* __restrict__ rows, int* __restrict__ argmax, const float* __restrict__ ref,
                                                       int ld_ref, float* __restrict__ stats) {
  __builtin_assume(labels && rows && argmax);           // (the launcher requires them)
  softmax_ce_rows(logits, ldl, labels, B, N, gscale, gscale_dev, dz, ldl, rows, argmax, ref, ld_ref, stats, 3);
}

}  // namespace

extern "C" {

int rmcl_nlvr2_ce(const float* logits, int ldl, const int32_t* labels, int B, int N, float grad_scale, const float* grad_scale_dev,
                  float* dz, float* rows, int32_t* argmax, const float* logits_ref, int ld_ref, float* stats, void* stream) {
  RMCL_REQUIRE(logits && labels && rows && argmax && stats, "nlvr2_ce: NULL argument");
  RMCL_REQUIRE(B >= 1 && B <= 65536 && N >= 1 && N <= CE_MAX_N && ldl >= N, "nlvr2_ce: bad shape (1 <= N <= 64, N <= ldl, B <= 65536)");
  RMCL_REQUIRE(!logits_ref || ld_ref >= N, "nlvr2_ce: ld_ref < N");
  RMCL_LAUNCH(nlvr2_ce_kernel, dim3(1), dim3(64 * CE_WAVES), 0, (hipStream_t)stream, logits, ldl, labels, B, N, grad_scale, grad_scale_dev,
              dz, rows, argmax, logits_ref, ld_ref, stats);
  RMCL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
