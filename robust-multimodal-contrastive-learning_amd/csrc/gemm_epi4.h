// The 4-column epilogue of the bf16 GEMMs whose MFMAs run with swapped operands (gemm_fast.hip 128x128, gemm_big.hip 256x256): the lane
// owns row m and the four consecutive columns n .. n + 3 of one 16x16 accumulator fragment.  Order (gemm.h, "Epilogue order"): alpha,
// bias, backward dropout mask, GELU'(aux), stash to C2, GELU, forward dropout mask, residual, then pack to bf16 or (fp32) accumulate,
// store.  DROP compiles the two dropout steps in; gemm_big has none (its launcher refuses them).  A scheduling barrier between two
// calls, where a kernel needs one, stays with the caller.
#pragma once
#include "rmcl_common.h"
#include "gemm.h"

template <typename TO, bool DROP>
__device__ __forceinline__ void epi4(const GemmArgs& g, int epi, TO* C, TO* C2, const f32x4& acc, int m, int n) {
  float v[4] = {g.alpha * acc[0], g.alpha * acc[1], g.alpha * acc[2], g.alpha * acc[3]};
  if (epi & EPI_BIAS) {
    const float4 b = *reinterpret_cast<const float4*>(g.bias + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (DROP && (epi & EPI_DROP_BWD)) {
    const uint32_t di = (uint32_t)((long)m * g.ld_aux + n);
    drop_scale4(g.drop_seed, di, g.drop_thresh, g.drop_inv_keep, v[0], v[1], v[2], v[3]);
  }
  if (epi & EPI_DGELU) {
    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(g.aux) + (long)m * g.ld_aux + n);
    v[0] *= gelu_fast_grad(__uint_as_float(u.x << 16)); v[1] *= gelu_fast_grad(__uint_as_float(u.x & 0xffff0000u));
    v[2] *= gelu_fast_grad(__uint_as_float(u.y << 16)); v[3] *= gelu_fast_grad(__uint_as_float(u.y & 0xffff0000u));
  }
  const long ci = (long)m * g.ldc + n;
  if (epi & EPI_SAVE_PREACT) store4<TO>(C2 + ci, v);
  if (epi & EPI_GELU) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_fast(v[r]);
  }
  if (DROP && (epi & EPI_DROPOUT)) drop_scale4(g.drop_seed, (uint32_t)ci, g.drop_thresh, g.drop_inv_keep, v[0], v[1], v[2], v[3]);
  if (epi & EPI_RESIDUAL) {
    const float4 r = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(g.aux) + (long)m * g.ld_aux + n);
    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
  }
  if constexpr (sizeof(TO) == 4) {
    if (epi & EPI_ACCUM) {
      const float4 o = *reinterpret_cast<const float4*>(C + ci);
      v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w;
    }
  }
  store4<TO>(C + ci, v);
}
