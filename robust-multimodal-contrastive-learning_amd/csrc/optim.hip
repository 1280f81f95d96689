// Guarded optimizer step: one statistics pass over the fp32 gradient arena that takes the skip / clip decision ON THE DEVICE
// (rmcl_step_ctl, include/rmcl.h), and the AdamW of embed_misc.hip reading that decision.  Both are pure streaming passes (4 B per
// element read; 16 B read + 14 B written): 16-byte loads, grids sized to the CUs, grid-stride loops.  Below them, the Adam and SGD
// sweeps (optim_rule_kernel), plain and guarded.
#include "rmcl_common.h"
#include "kernels.h"
#include "../../include/rmcl.h"

// ---------------------------------------------------------------------------------------------
// Gradient statistics.  Stage 1: a fixed grid of blocks, each thread walks float4 groups at the grid stride and keeps
//   cnt  = number of elements whose exponent bits are all ones (NaN, +inf, -inf)
//   sum  = sum of g^2 over the OTHER elements, in double: the square of an fp32 is exact in a double and cannot overflow it
//          (an fp32 sum of squares overflows from |g| ~ 1e19 on, on finite gradients)
// then the block adds its 256 partials in a fixed order (xor butterfly inside a wave, waves 0..3 in order) and stores ONE
// (sum, cnt) pair into the workspace: ws = double sum[nblk] followed by int64 cnt[nblk].  Stage 2: one block adds the nblk pairs in a
// fixed order and writes the decision.  No atomics, no cross-block hand-off inside a launch: the same bits on every call.
// ---------------------------------------------------------------------------------------------
#define RMCL_STATS_MAX_BLOCKS 1024      // 4 blocks of 256 threads per CU on 256 CUs; one pass of the full grid covers 1024 * 1024 elements

static inline int stats_blocks(long n) { return (int)std::min<long>(cdiv(n / 4, 256), RMCL_STATS_MAX_BLOCKS); }

__device__ __forceinline__ void stats_acc(const float4 g, double& sum, long& cnt) {
  const float G[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool bad = (__float_as_uint(G[j]) & 0x7f800000u) == 0x7f800000u;
    const double d = (double)G[j];
    cnt += bad ? 1 : 0;
    sum += bad ? 0.0 : d * d;
  }
}

// sum over the block, the same order on every call; the result is valid in thread 0
__device__ __forceinline__ void stats_block_sum(double& sum, long& cnt, double* sh_sum, long* sh_cnt) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh_sum[wave] = sum; sh_cnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = ((sh_sum[0] + sh_sum[1]) + sh_sum[2]) + sh_sum[3];
    cnt = sh_cnt[0] + sh_cnt[1] + sh_cnt[2] + sh_cnt[3];
  }
}

__global__ __launch_bounds__(256) void grad_stats_partial_kernel(const float* __restrict__ g, long n4, double* __restrict__ ws_sum,
                                                                 long* __restrict__ ws_cnt) {
  __shared__ double sh_sum[4];
  __shared__ long sh_cnt[4];
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const long stride = (long)gridDim.x * 256;
  double sum = 0.0;
  long cnt = 0;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n4; i += 4 * stride) {          // four independent 16-byte loads in flight per thread
    const float4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
    stats_acc(a, sum, cnt);
    stats_acc(b, sum, cnt);
    stats_acc(c, sum, cnt);
    stats_acc(d, sum, cnt);
  }
  for (; i < n4; i += stride) stats_acc(g4[i], sum, cnt);
  stats_block_sum(sum, cnt, sh_sum, sh_cnt);
  if (threadIdx.x == 0) {
    ws_sum[blockIdx.x] = sum;
    ws_cnt[blockIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(256) void grad_stats_final_kernel(const double* __restrict__ ws_sum, const long* __restrict__ ws_cnt, int nblk,
                                                               float grad_scale, float max_norm, float b1, float b2,
                                                               rmcl_step_ctl* __restrict__ ctl) {
  __shared__ double sh_sum[4];
  __shared__ long sh_cnt[4];
  double sum = 0.0;
  long cnt = 0;
  for (int i = threadIdx.x; i < nblk; i += 256) {
    sum += ws_sum[i];
    cnt += ws_cnt[i];
  }
  stats_block_sum(sum, cnt, sh_sum, sh_cnt);
  if (threadIdx.x != 0) return;
  const float norm = (float)((double)grad_scale * sqrt(sum));
  const float coef = max_norm > 0.f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f;   // torch.nn.utils.clip_grad_norm_
  const int skip = cnt > 0 ? 1 : 0;
  ctl->sumsq = sum;
  ctl->nonfinite = cnt;
  ctl->norm = norm;
  ctl->clip_coef = coef;
  ctl->skip = skip;
  if (skip) {
    ctl->skipped = ctl->skipped + 1;
  } else {
    const int t = ctl->applied + 1;                         // bias corrections of the step that IS applied: rmcl_adamw's host lines
    ctl->applied = t;
    ctl->bc1 = (float)(1.0 - pow((double)b1, (double)t));
    ctl->bc2s = (float)sqrt(1.0 - pow((double)b2, (double)t));
  }
}

long rmcl_grad_stats_workspace_bytes(long n) { return n >= 4 ? (long)stats_blocks(n) * 16 : 16; }

int rmcl_grad_stats(const float* g, long n, float grad_scale, float max_norm, float b1, float b2, void* ws, rmcl_step_ctl* ctl,
                    hipStream_t s) {
  RMCL_REQUIRE(n > 0 && n % 4 == 0, "grad_stats: n must be a positive multiple of 4");
  const int nblk = stats_blocks(n);
  double* ws_sum = reinterpret_cast<double*>(ws);
  long* ws_cnt = reinterpret_cast<long*>(ws_sum + nblk);
  RMCL_LAUNCH(grad_stats_partial_kernel, dim3(nblk), dim3(256), 0, s, g, n / 4, ws_sum, ws_cnt);
  RMCL_CHECK_LAUNCH();
  RMCL_LAUNCH(grad_stats_final_kernel, dim3(1), dim3(256), 0, s, ws_sum, ws_cnt, nblk, grad_scale, max_norm, b1, b2, ctl);
  RMCL_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// adamw_kernel (embed_misc.hip) with the decision read from ctl: skip set -> the kernel returns before its first store (p, m, v and the
// bf16 shadow keep every byte); otherwise g_j = g * grad_scale * clip_coef and the bias corrections are those of step ctl->applied.
// With clip_coef == 1 the extra product is exact, so m and v come out as adamw_kernel's.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, bf16_t* __restrict__ p_lp, const long* __restrict__ seg_end,
                                                            const float* __restrict__ seg_lr_mult, const float* __restrict__ seg_wd, int nseg,
                                                            float lr, float b1, float b2, float eps, const rmcl_step_ctl* __restrict__ ctl,
                                                            long n4, float grad_scale) {
  if (ctl->skip) return;
  const float bc1 = ctl->bc1, bc2s = ctl->bc2s, clip_coef = ctl->clip_coef;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long e = i * 4;
    int lo = 0, hi = nseg - 1;  // first segment with seg_end > e
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg_end[mid] > e) hi = mid; else lo = mid + 1; }
    const float slr = lr * seg_lr_mult[lo], wd = seg_wd[lo];
    const float step = slr * bc2s / bc1;
    float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    float P[4] = {pp.x, pp.y, pp.z, pp.w}, G[4] = {gg.x, gg.y, gg.z, gg.w}, Mo[4] = {mm.x, mm.y, mm.z, mm.w}, V[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = G[j] * grad_scale * clip_coef;
      Mo[j] = Mo[j] * b1 + gj * (1.0f - b1);
      V[j] = V[j] * b2 + gj * gj * (1.0f - b2);
      P[j] = P[j] - step * Mo[j] / (sqrtf(V[j]) + eps);
      if (wd > 0.f) P[j] = P[j] - slr * wd * P[j];
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(P[0], P[1], P[2], P[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(Mo[0], Mo[1], Mo[2], Mo[3]);
    reinterpret_cast<float4*>(v)[i] = make_float4(V[0], V[1], V[2], V[3]);
    if (p_lp) {
      uint2 pk;
      pk.x = (uint32_t)f2bf(P[0]) | ((uint32_t)f2bf(P[1]) << 16);
      pk.y = (uint32_t)f2bf(P[2]) | ((uint32_t)f2bf(P[3]) << 16);
      reinterpret_cast<uint2*>(p_lp)[i] = pk;
    }
  }
}

int rmcl_adamw_guarded(float* p, const float* g, float* m, float* v, void* p_lp, const long* seg_end, const float* seg_lr_mult,
                       const float* seg_wd, int nseg, float lr, float b1, float b2, float eps, float grad_scale, const rmcl_step_ctl* ctl,
                       long n, hipStream_t s) {
  RMCL_REQUIRE(n > 0 && n % 4 == 0 && nseg > 0, "adamw_guarded: bad args");
  RMCL_LAUNCH(adamw_guarded_kernel, dim3(std::min<long>(cdiv(n / 4, 256), 2048)), dim3(256), 0, s, p, g, m, v, (bf16_t*)p_lp, seg_end,
              seg_lr_mult, seg_wd, nseg, lr, b1, b2, eps, ctl, n / 4, grad_scale);
  RMCL_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Adam and SGD (the other two optim_type values of vilt_utils.set_schedule :399-402) over the same arenas, segment tables and bf16
// shadow as adamw_kernel: one float4 per thread and trip, the segment looked up per float4, 16-byte loads and stores, no atomics, no
// scratch.  gj = g * grad_scale (* clip_coef, guarded); both rules use torch's COUPLED L2 decay, gj += wd * p where the segment's wd > 0.
//   Adam (torch.optim.Adam, single tensor, amsgrad off):
//     m = b1 m + (1 - b1) gj;  v = b2 v + (1 - b2) gj^2;  p = p - ((slr / bc1) * m) / (sqrt(v) / bc2s + eps)
//     eps is added AFTER the division by bc2s = sqrt(1 - b2^t); adamw_kernel (HF AdamW) adds it before.
//   SGD (torch.optim.SGD, momentum b1, dampening 0, nesterov off):
//     m = b1 m + gj;  p = p - slr * m
//     torch's first step sets the buffer to gj, which is this update on a zero buffer: no first-step arm.  v is neither read nor written.
// GUARDED: skip set -> return before the first store; otherwise clip_coef (and, for Adam, bc1 / bc2s) come from ctl.  The product with
// clip_coef == 1 is exact, so the unclipped guarded form gives the plain form's bits.
// Bytes per element: Adam 16 read + 12 written, SGD 12 + 8; + 2 written with the shadow.
// ---------------------------------------------------------------------------------------------
template <int RULE, bool GUARDED>
__global__ __launch_bounds__(256) void optim_rule_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, bf16_t* __restrict__ p_lp, const long* __restrict__ seg_end,
                                                         const float* __restrict__ seg_lr_mult, const float* __restrict__ seg_wd, int nseg,
                                                         float lr, float b1, float b2, float eps, float bc1, float bc2s,
                                                         const rmcl_step_ctl* __restrict__ ctl, long n4, float grad_scale) {
  float clip_coef = 1.0f;
  if (GUARDED) {
    if (ctl->skip) return;
    clip_coef = ctl->clip_coef;
    if (RULE == RMCL_OPTIM_ADAM) { bc1 = ctl->bc1; bc2s = ctl->bc2s; }
  }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const long e = i * 4;
    int lo = 0, hi = nseg - 1;  // first segment with seg_end > e
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (seg_end[mid] > e) hi = mid; else lo = mid + 1; }
    const float slr = lr * seg_lr_mult[lo], wd = seg_wd[lo];
    float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i], mm = reinterpret_cast<float4*>(m)[i];
    float P[4] = {pp.x, pp.y, pp.z, pp.w}, G[4] = {gg.x, gg.y, gg.z, gg.w}, Mo[4] = {mm.x, mm.y, mm.z, mm.w};
    if (RULE == RMCL_OPTIM_ADAM) {
      const float step = slr / bc1;
      float4 vv = reinterpret_cast<float4*>(v)[i];
      float V[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gj = G[j] * grad_scale;
        if (GUARDED) gj = gj * clip_coef;
        if (wd > 0.f) gj = gj + wd * P[j];
        Mo[j] = Mo[j] * b1 + gj * (1.0f - b1);
        V[j] = V[j] * b2 + gj * gj * (1.0f - b2);
        P[j] = P[j] - (step * Mo[j]) / (sqrtf(V[j]) / bc2s + eps);
      }
      reinterpret_cast<float4*>(v)[i] = make_float4(V[0], V[1], V[2], V[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float gj = G[j] * grad_scale;
        if (GUARDED) gj = gj * clip_coef;
        if (wd > 0.f) gj = gj + wd * P[j];
        Mo[j] = Mo[j] * b1 + gj;
        P[j] = P[j] - slr * Mo[j];
      }
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(P[0], P[1], P[2], P[3]);
    reinterpret_cast<float4*>(m)[i] = make_float4(Mo[0], Mo[1], Mo[2], Mo[3]);
    if (p_lp) {
      uint2 pk;
      pk.x = (uint32_t)f2bf(P[0]) | ((uint32_t)f2bf(P[1]) << 16);
      pk.y = (uint32_t)f2bf(P[2]) | ((uint32_t)f2bf(P[3]) << 16);
      reinterpret_cast<uint2*>(p_lp)[i] = pk;
    }
  }
}

// ctl NULL: the plain form, bias corrections of `step` computed here like rmcl_adamw's; ctl given: the guarded form, `step` unused
int rmcl_optim_step(int rule, float* p, const float* g, float* m, float* v, void* p_lp, const long* seg_end, const float* seg_lr_mult,
                    const float* seg_wd, int nseg, float lr, float b1, float b2, float eps, int step, float grad_scale,
                    const rmcl_step_ctl* ctl, long n, hipStream_t s) {
  RMCL_REQUIRE(rule == RMCL_OPTIM_ADAM || rule == RMCL_OPTIM_SGD, "optim_step: unknown rule");
  RMCL_REQUIRE(n > 0 && n % 4 == 0 && nseg > 0, "optim_step: bad args (n must be a positive multiple of 4, nseg > 0)");
  RMCL_REQUIRE(rule == RMCL_OPTIM_ADAM ? v != nullptr : v == nullptr, "optim_step: Adam needs v, SGD keeps none (v must be NULL)");
  RMCL_REQUIRE(ctl || step >= 1, "optim_step: the plain form needs step >= 1");
  float bc1 = 1.0f, bc2s = 1.0f;
  if (!ctl && rule == RMCL_OPTIM_ADAM) {
    bc1 = (float)(1.0 - pow((double)b1, (double)step));
    bc2s = (float)sqrt(1.0 - pow((double)b2, (double)step));
  }
  auto kernel = rule == RMCL_OPTIM_ADAM ? (ctl ? optim_rule_kernel<RMCL_OPTIM_ADAM, true> : optim_rule_kernel<RMCL_OPTIM_ADAM, false>)
                                        : (ctl ? optim_rule_kernel<RMCL_OPTIM_SGD, true> : optim_rule_kernel<RMCL_OPTIM_SGD, false>);
  RMCL_LAUNCH(kernel, dim3(std::min<long>(cdiv(n / 4, 256), 4096)), dim3(256), 0, s, p, g, m, v, (bf16_t*)p_lp, seg_end, seg_lr_mult,
              seg_wd, nseg, lr, b1, b2, eps, bc1, bc2s, ctl, n / 4, grad_scale);
  RMCL_CHECK_LAUNCH();
  return 0;
}
