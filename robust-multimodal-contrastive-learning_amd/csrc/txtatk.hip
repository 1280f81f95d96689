// Text attack on the fine-tuning tasks (GreedyAttack_vqa / GreedyAttack_nlvr2, attack/greedy_attack_vilt.py:835-1478).
//
//   word saliency   get_important_scores (:221-228) on the device: per (sentence b, word w) the L1 norm over the hidden columns of the
//                   MEAN saliency gradient over the word's sub-word tokens,
//                       out[b, w] = sum_d | (1 / len) * sum_{t = start .. start + len - 1} g[row0 + b * row_step, t, d] |
//                   g is the [R, L, D] gradient rmcl_encoder_backward leaves in `dtext`.  One wave per (b, w): lane l owns the columns
//                   4 l + 256 k (float4 loads), sums the tokens in ascending order, scales, takes |.|, and the 64 partial sums meet in a
//                   butterfly.  One owner per output, a fixed summation order, no float atomics, no scratch: two identical calls give
//                   identical bits.  The host reads back [B, W] floats instead of [B, L, D].
#include "rmcl_common.h"
#include "kernels.h"

namespace {

__global__ __launch_bounds__(256) void word_saliency_kernel(const float* __restrict__ g, const int* __restrict__ spans,
                                                            float* __restrict__ out, int B, int W, int L, int D, int row0, int row_step) {
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);                // the (b, w) of this wave
  const int lane = threadIdx.x & 63;
  if (i >= (long)B * W) return;
  const int b = (int)(i / W);
  const int start = spans[2 * i], len = spans[2 * i + 1];
  float acc = 0.f;
  if (len > 0) {
    // a span that leaves [0, L) is cut to the tokens inside it (nothing is read out of bounds); the divisor stays its stated count
    const long end = (long)start + len;                                    // (64-bit: no span value can wrap the sum)
    const int t0 = start < 0 ? 0 : start, t1 = end > L ? L : (int)end;
    const float* row = g + ((long)row0 + (long)b * row_step) * L * D;
    const float inv = 1.0f / (float)len;
    for (int c = lane * 4; c < D; c += 256) {
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = t0; t < t1; ++t) {
        const float4 x = *reinterpret_cast<const float4*>(row + (long)t * D + c);
        s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
      }
      acc += (fabsf(s.x * inv) + fabsf(s.y * inv)) + (fabsf(s.z * inv) + fabsf(s.w * inv));
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) out[i] = acc;
}

}  // namespace

int rmcl_word_saliency_launch(const float* g, const int* spans, float* out, int B, int W, int L, int D, int row0, int row_step,
                              hipStream_t s) {
  RMCL_LAUNCH(word_saliency_kernel, dim3(cdiv((long)B * W, 4)), dim3(256), 0, s, g, spans, out, B, W, L, D, row0, row_step);
  RMCL_CHECK_LAUNCH();
  return 0;
}
