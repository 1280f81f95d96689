// NLVR2 fine-tuning: the hard-label softmax cross-entropy of compute_nlvr2 / compute_nlvr2_attack / PGDAttack_nlvr2
// (objectives.py:898-1060, pgd_attack_vilt.py:285-300) with the logged accuracy and change_rate_cross counts (my_metrics.py:30-45).
//
// The head itself (nlvr2_classifier, vilt_module.py:193-200: Linear(2D,2D) - LayerNorm - GELU - Linear(2D,2)) runs on the VQA head
// kernels (vqa.hip) with D = H = 1536, N = 2, ldl = 64.  What is left is tiny: B rows of N = 2 logits.  One workgroup of four waves;
// each wave owns rows w, w + 4, w + 8, ... (one lane per column), so every reduction has a fixed order and nothing uses float
// atomics: loss, counts and dz are bit-reproducible.
#include "rmcl_common.h"
#include "kernels.h"
#include "../../include/rmcl.h"

namespace {

#define CE_WAVES 4
#define CE_MAX_N 64

__device__ __forceinline__ float ce_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float ce_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// first maximum of a row held one column per lane (lanes >= N hold -inf / index N): ties go to the smaller column
__device__ __forceinline__ int ce_wave_argmax(float v, int i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
  }
  return i;
}

__global__ __launch_bounds__(256) void nlvr2_ce_kernel(const float* __restrict__ logits, int ldl, const int* __restrict__ labels, int B,
                                                       int N, float gscale, const float* __restrict__ gscale_dev, float* __restrict__ dz,
                                                       float* __restrict__ rows, int* __restrict__ argmax, const float* __restrict__ ref,
                                                       int ld_ref, float* __restrict__ stats) {
  __shared__ float s_loss[CE_WAVES];
  __shared__ int s_hit[CE_WAVES], s_chg[CE_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float scale = (gscale_dev ? gscale * gscale_dev[0] : gscale) / (float)B;
  float loss_acc = 0.f;                 // lane 0's running sum over this wave's rows, in row order
  int hit = 0, chg = 0;
  for (int b = wave; b < B; b += CE_WAVES) {
    const float z = lane < N ? logits[(long)b * ldl + lane] : -INFINITY;
    const float m = ce_wave_max(z);
    const float e = lane < N ? expf(z - m) : 0.f;
    const float s = ce_wave_sum(e);
    const int lbl = min(max(labels[b], 0), N - 1);
    const float zl = __shfl(z, lbl, 64);
    const int am = min(ce_wave_argmax(z, lane < N ? lane : N), N - 1);
    const float row = (logf(s) + m) - zl;
    if (dz) {
      for (int c = lane; c < ldl; c += 64)
        dz[(long)b * ldl + c] = c < N ? scale * (e / s - (c == lbl ? 1.f : 0.f)) : 0.f;
    }
    int changed = 0;
    if (ref) {
      const float zr = lane < N ? ref[(long)b * ld_ref + lane] : -INFINITY;
      changed = min(ce_wave_argmax(zr, lane < N ? lane : N), N - 1) != am;
    }
    if (lane == 0) {
      rows[b] = row;
      argmax[b] = am;
      loss_acc += row;
      hit += am == lbl;
      chg += changed;
    }
  }
  if (lane == 0) { s_loss[wave] = loss_acc; s_hit[wave] = hit; s_chg[wave] = chg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float l = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
    stats[0] = l / (float)B;
    stats[1] = (float)(s_hit[0] + s_hit[1] + s_hit[2] + s_hit[3]);
    stats[2] = (float)(s_chg[0] + s_chg[1] + s_chg[2] + s_chg[3]);
  }
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
