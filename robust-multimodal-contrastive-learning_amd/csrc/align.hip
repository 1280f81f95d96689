// Word-patch alignment maps of the prediction API (include/rmcl.h rmcl_ipot_plan_f32, rmcl_align_heat; the heat map of the
// reference's demo.py:86-151).
//
// 1. ipot_plan_kernel - IPOT (objectives.py:46-76, k = 1) shaped for the demo's 1000 iterations.  One 256-thread workgroup per sample.
//   ownership      Thread n owns plan row n, and row n + 256 when Li > 256 (ROWS = 2).  A thread's T[n][0 .. 40) and A[n][0 .. 40) =
//                  exp(-C / beta) live in registers, statically indexed (every loop over the 40 columns is unrolled); columns behind Lt,
//                  rows behind Li and every joint pad hold A = T = 0, which adds exact zeros to every sum.
//   one iteration  q = A * T;  delta[n] = 1 / (y_len * sum_m q[m] sigma[m] + y_mask[n])  - an in-thread dot product, m ascending,
//                  against the sigma the thread read from LDS at the end of the previous iteration;  u = delta * q;
//                  column m: (u of row n + u of row n + 256) summed over the wave by wave_sum_dpp, lane m of the wave keeps the total,
//                  lanes 0 .. 39 write the wave's partials to LDS;  BARRIER;  thread m < 40 adds the four partials in wave order and
//                  writes sigma[m] = 1 / (x_len * that + x_mask[m]);  BARRIER;  every thread reads the 40 sigmas once and forms
//                  T = u * sigma = (delta * (A * T)) * sigma.
//   Two barriers per iteration; the plan makes no LDS traffic inside the loop.  No atomics, no scratch, no workspace, every sum in a fixed
//   order: two calls give the same bytes.  Multiplications and additions are not contracted (tests/align_ref.py restates the order in
//   numpy float32).  A sample without a valid text token or without a valid patch leaves the loop out and writes T = 0.
//
// 2. align_heat_kernel - one workgroup per (sample, text position): the plan column scattered to the H x W patch grid, the demo's
//   standardise / clip(1, 3) / min-max arithmetic over the whole grid, and for one chosen position per sample the alpha bytes enlarged
//   by PIL's NEAREST index tables.  The statistics (mean, unbiased variance, extrema) are accumulated in fp64 from the fp32 cells, each
//   thread over its cells in ascending order, the 256 partials in a butterfly and then in wave order; heat is rounded to fp32 once.
#include <math.h>
#include "rmcl_common.h"
#include "kernels.h"
#include "../../include/rmcl.h"

namespace {

constexpr int IPOT_W = RMCL_IPOT_PLAN_MAX_LT;          // the unrolled plan width

template <int ROWS>
__global__ __launch_bounds__(256) void ipot_plan_kernel(const float* __restrict__ cost, const int* __restrict__ txt_valid,
                                                        const int* __restrict__ img_valid, float* __restrict__ Tout, int Lt, int Li, int ldc,
                                                        float beta, int iters) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float sh_part[4][IPOT_W];
  __shared__ __attribute__((aligned(16))) float sh_sigma[IPOT_W];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const float* C = cost + (long)b * Lt * ldc;
  const int* tv = txt_valid + (long)b * Lt;
  const int* iv = img_valid + (long)b * Li;
  float* out = Tout + (long)b * Li * Lt;

  const bool my_tv = t < Lt && tv[t] != 0;              // (Lt <= 40: wave 0 sees every text position)
  bool row_ok[ROWS];
  int y_cnt = 0;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int n = t + 256 * r;
    row_ok[r] = n < Li && iv[n] != 0;
    y_cnt += __syncthreads_count(row_ok[r]);
  }
  const int x_cnt = __syncthreads_count(my_tv);
  if (t < IPOT_W) sh_sigma[t] = my_tv ? 1.0f / (float)x_cnt : 0.f;
  __syncthreads();
  // text validity as a bit mask every thread holds: bit m = position m is valid
  unsigned long long tmask = 0;
#pragma unroll
  for (int m = 0; m < IPOT_W; ++m)
    if (sh_sigma[m] != 0.f) tmask |= 1ull << m;

  if (x_cnt == 0 || y_cnt == 0) {                       // uniform over the workgroup: no plan
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int n = t + 256 * r;
      if (n < Li)
        for (int m = 0; m < Lt; ++m) out[(long)n * Lt + m] = 0.f;
    }
    return;
  }
  const float x_len = (float)x_cnt, y_len = (float)y_cnt;

  float A[ROWS][IPOT_W], T[ROWS][IPOT_W], sg[IPOT_W], y_mask[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int n = t + 256 * r;
    y_mask[r] = row_ok[r] ? 0.f : 1e4f;
#pragma unroll
    for (int m = 0; m < IPOT_W; ++m) {
      const bool ok = row_ok[r] && ((tmask >> m) & 1ull);
      A[r][m] = ok ? expf(-C[(long)m * ldc + n] / beta) : 0.f;
      T[r][m] = ok ? 1.f : 0.f;
    }
  }
#pragma unroll
  for (int m = 0; m < IPOT_W; ++m) sg[m] = sh_sigma[m];
  const float x_mask = ((tmask >> (t < IPOT_W ? t : 0)) & 1ull) ? 0.f : 1e4f;      // (used by threads t < 40 only)

  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      float s = 0.f;
#pragma unroll
      for (int m = 0; m < IPOT_W; ++m) {
        T[r][m] = A[r][m] * T[r][m];                    // q
        s += T[r][m] * sg[m];
      }
      const float delta = 1.0f / (y_len * s + y_mask[r]);
#pragma unroll
      for (int m = 0; m < IPOT_W; ++m) T[r][m] = delta * T[r][m];       // u = delta * q
    }
    float mine = 0.f;
#pragma unroll
    for (int m = 0; m < IPOT_W; ++m) {
      float c = T[0][m];
      if (ROWS == 2) c += T[ROWS - 1][m];
      c = wave_sum_dpp(c);
      mine = lane == m ? c : mine;
    }
    if (lane < IPOT_W) sh_part[w][lane] = mine;
    __syncthreads();
    if (t < IPOT_W) {
      const float p = ((sh_part[0][t] + sh_part[1][t]) + sh_part[2][t]) + sh_part[3][t];
      sh_sigma[t] = 1.0f / (x_len * p + x_mask);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < IPOT_W; ++m) sg[m] = sh_sigma[m];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int m = 0; m < IPOT_W; ++m) T[r][m] = T[r][m] * sg[m];
  }

#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int n = t + 256 * r;
    if (n < Li) {
#pragma unroll
      for (int m = 0; m < IPOT_W; ++m)
        if (m < Lt) out[(long)n * Lt + m] = (row_ok[r] && ((tmask >> m) & 1ull)) ? T[r][m] : 0.f;
    }
  }
}

// ---- heat maps -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
  const long long x = __builtin_bit_cast(long long, v);
  const int lo = __shfl_xor((int)(x & 0xffffffffll), o, 64), hi = __shfl_xor((int)(x >> 32), o, 64);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

// OP 0: sum, 1: min, 2: max over the workgroup; butterfly over the wave, then the four waves in wave order; every thread gets the result
template <int OP>
__device__ __forceinline__ double block_reduce_f64(double v, double* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = shfl_xor_f64(v, o);
    v = OP == 0 ? v + v2 : (OP == 1 ? fmin(v, v2) : fmax(v, v2));
  }
  __syncthreads();                                       // (sh may still be read by the previous reduction)
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double r = sh[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) r = OP == 0 ? r + sh[q] : (OP == 1 ? fmin(r, sh[q]) : fmax(r, sh[q]));
  return r;
}

__global__ __launch_bounds__(256) void align_heat_kernel(const float* __restrict__ T, const int* __restrict__ patch_index,
                                                         const int* __restrict__ txt_valid, int Lt, int Li, int H, int W,
                                                         float* __restrict__ grid, float* __restrict__ heat, int* __restrict__ flat,
                                                         const int* __restrict__ token, const int* __restrict__ tables, int Hout, int Wout,
                                                         unsigned char* __restrict__ alpha) {
  __shared__ float g[RMCL_ALIGN_MAX_CELLS];
  __shared__ double sh[4];
  const int m = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int HW = H * W, P = Li - 1;
  for (int c = t; c < HW; c += 256) g[c] = 0.f;
  __syncthreads();
  const float* Tb = T + (long)b * Li * Lt;
  for (int i = t; i < P; i += 256) {
    const int c = patch_index[(long)b * P + i];
    if (c >= 0 && c < HW) g[c] = Tb[(long)(1 + i) * Lt + m];
  }
  __syncthreads();
  float* gout = grid + ((long)b * Lt + m) * HW;
  for (int c = t; c < HW; c += 256) gout[c] = g[c];

  bool is_flat = txt_valid[(long)b * Lt + m] == 0 || HW < 2;
  double mean = 0.0, sd = 0.0, lo = 0.0, hi = 0.0;
  if (!is_flat) {                                        // (uniform over the workgroup)
    double s = 0.0;
    for (int c = t; c < HW; c += 256) s += (double)g[c];
    mean = block_reduce_f64<0>(s, sh) / (double)HW;
    double q = 0.0;
    for (int c = t; c < HW; c += 256) {
      const double d = (double)g[c] - mean;
      q += d * d;
    }
    sd = sqrt(block_reduce_f64<0>(q, sh) / (double)(HW - 1));
    is_flat = !(sd > 0.0);
  }
  if (!is_flat) {
    double vlo = 3.0, vhi = 1.0;                         // (the clipped values lie in [1, 3])
    for (int c = t; c < HW; c += 256) {
      const double z = fmin(fmax(((double)g[c] - mean) / sd, 1.0), 3.0);
      vlo = fmin(vlo, z);
      vhi = fmax(vhi, z);
    }
    lo = block_reduce_f64<1>(vlo, sh);
    hi = block_reduce_f64<2>(vhi, sh);
    is_flat = !(hi > lo);
  }
  __syncthreads();                                       // every read of g above is done: g now takes the heat values
  float* hout = heat + ((long)b * Lt + m) * HW;
  for (int c = t; c < HW; c += 256) {
    float h = 0.f;
    if (!is_flat) {
      const double z = fmin(fmax(((double)g[c] - mean) / sd, 1.0), 3.0);
      h = (float)((z - lo) / (hi - lo));
    }
    g[c] = h;
    hout[c] = h;
  }
  if (t == 0) flat[(long)b * Lt + m] = is_flat ? 1 : 0;
  if (alpha == nullptr || token[b] != m) return;          // (uniform)
  __syncthreads();
  const int* ytab = tables;
  const int* xtab = tables + Hout;
  unsigned char* a = alpha + (long)b * Hout * Wout;
  for (long i = t; i < (long)Hout * Wout; i += 256) {
    const int y = (int)(i / Wout), x = (int)(i - (long)y * Wout);
    const int sy = min(max(ytab[y], 0), H - 1), sx = min(max(xtab[x], 0), W - 1);
    a[i] = (unsigned char)(int)(g[sy * W + sx] * 255.0f);     // np.uint8(heat * 255): the fp32 product, truncated
  }
}

}  // namespace

int rmcl_ipot_plan_launch(const float* cost, const int* txt_valid, const int* img_valid, float* T, int B, int Lt, int Li, int ld, float beta,
                          int iters, hipStream_t s) {
  if (Li <= 256)
    RMCL_LAUNCH(ipot_plan_kernel<1>, dim3(B), dim3(256), 0, s, cost, txt_valid, img_valid, T, Lt, Li, ld, beta, iters);
  else
    RMCL_LAUNCH(ipot_plan_kernel<2>, dim3(B), dim3(256), 0, s, cost, txt_valid, img_valid, T, Lt, Li, ld, beta, iters);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_align_heat_launch(const float* T, const int* patch_index, const int* txt_valid, int B, int Lt, int Li, int H, int W, float* grid,
                           float* heat, int* flat, const int* token, const int* tables, int Hout, int Wout, unsigned char* alpha,
                           hipStream_t s) {
  RMCL_LAUNCH(align_heat_kernel, dim3(Lt, B), dim3(256), 0, s, T, patch_index, txt_valid, Lt, Li, H, W, grid, heat, flat, token, tables,
              Hout, Wout, alpha);
  RMCL_CHECK_LAUNCH();
  return 0;
}
