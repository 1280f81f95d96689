// BERT prediction-head transform (BertPredictionHeadTransform, heads.py): Linear(D,D) - GELU (exact erf) - LayerNorm(D, eps 1e-12), forward
// and backward over a COMPACTED row list.  The one copy for every head that starts with it: mlm_score (mlm.hip) and mpp_score (mpp.hip);
// a further prediction head adds its decoder and calls pred_transform_forward / pred_transform_backward (head_rows.h).
//   gather     x [rows, D] = rows idx[r] of xn (rows >= n: zeros, so everything behind them is finite)
//   transform  a = x Wt^T + bt (exact fp32 GEMM), h = LayerNorm(GELU(a)) in one row pass; h is kept in the decoder's operand type
//              (bf16 / fp32), [rows, D] and - where the workspace has an hT (the MLM decoder's dW operand) - transposed [D, rows]
//   backward   da = GELU'(a) LayerNorm'(dh) in one row pass with per-workgroup partials of dgamma / dbeta / dbias, the partials summed in
//              workgroup order, dWt += da^T x, dx = da Wt and the scatter of dx into the zero-filled dxn of the encoder backward
// Every output has ONE owner and a fixed summation order (no float atomics): two identical calls give identical bits.
// The kernels are whole units: the four-phase LDS merge of the backward row pass stays literal inside it (DESIGN "Head row primitives").
#include <algorithm>
#include "rmcl_common.h"
#include "kernels.h"
#include "head_rows.h"

namespace {

// x [rows, D] = xn[idx[r]] for r < n, else 0
__global__ __launch_bounds__(256) void pred_gather_kernel(const float* __restrict__ xn, const int* __restrict__ idx, const int* __restrict__ count,
                                                          float* __restrict__ x, int rows, int D) {
  const int n = min(count[0], rows), per_row = D / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)rows * per_row; i += (long)gridDim.x * 256) {
    const int r = (int)(i / per_row), c = (int)(i - (long)r * per_row) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < n) v = *reinterpret_cast<const float4*>(xn + (long)idx[r] * D + c);
    *reinterpret_cast<float4*>(x + (long)r * D + c) = v;
  }
}

// dxn[idx[r]] = dx[r] for r < n (every listed row has exactly one destination; dxn was zero-filled by the caller)
__global__ __launch_bounds__(256) void pred_scatter_kernel(const float* __restrict__ dx, const int* __restrict__ idx, const int* __restrict__ count,
                                                           float* __restrict__ dxn, int rows, int D) {
  const int n = min(count[0], rows), per_row = D / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)n * per_row; i += (long)gridDim.x * 256) {
    const int r = (int)(i / per_row), c = (int)(i - (long)r * per_row) * 4;
    *reinterpret_cast<float4*>(dxn + (long)idx[r] * D + c) = *reinterpret_cast<const float4*>(dx + (long)r * D + c);
  }
}

// ---- h = LayerNorm(GELU(a)), eps 1e-12 -----------------------------------------------------------------------------------------------
// One wave per row, D = 256 NV.  h [rows, D] and (HT) hT [D, rows] in T; stat[2 row] = (mean, rstd) of GELU(a).
template <typename T, int NV, bool HT>
__global__ __launch_bounds__(256) void pred_gelu_ln_fwd_kernel(const float* __restrict__ a, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, T* __restrict__ h, T* __restrict__ hT,
                                                               float* __restrict__ stat, int rows) {
  constexpr int D = 256 * NV;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float4 v[NV];
  float s = 0.f, mu, rs;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float4 x = *reinterpret_cast<const float4*>(a + (long)row * D + (lane + 64 * i) * 4);
    v[i] = make_float4(gelu_erf(x.x), gelu_erf(x.y), gelu_erf(x.z), gelu_erf(x.w));
    s += sum4_pairwise(v[i]);
  }
  ln_row_stats<NV>(v, s, 1e-12f, mu, rs);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    const float4 w = *reinterpret_cast<const float4*>(gamma + c), bb = *reinterpret_cast<const float4*>(beta + c);
    const float o[4] = {(v[i].x - mu) * rs * w.x + bb.x, (v[i].y - mu) * rs * w.y + bb.y, (v[i].z - mu) * rs * w.z + bb.z,
                        (v[i].w - mu) * rs * w.w + bb.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const T t = from_f32<T>(o[j]);
      h[(long)row * D + c + j] = t;
      if constexpr (HT) hT[(long)(c + j) * rows + row] = t;
    }
  }
  if (lane == 0) {
    stat[2 * row] = mu;
    stat[2 * row + 1] = rs;
  }
}

// da = GELU'(a) * LayerNorm'(dh) per row (GELU(a) and xhat recomputed from a and the stashed statistics).  part[blk][3][D]: this
// workgroup's sums over its rows of dh * xhat (-> dgamma), dh (-> dbeta) and da (-> the dense bias); the four waves meet in LDS in a fixed order.
template <int NV>
__global__ __launch_bounds__(256) void pred_gelu_ln_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ a,
                                                               const float* __restrict__ stat, const float* __restrict__ gamma,
                                                               float* __restrict__ da, float* __restrict__ part, int rows) {
  constexpr int D = 256 * NV;
  __shared__ float red[3][D];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float4 w[NV], pg[NV], pb[NV], pa[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    w[i] = *reinterpret_cast<const float4*>(gamma + (lane + 64 * i) * 4);
    pg[i] = pb[i] = pa[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int r0 = blockIdx.x * PRED_ROWS_PER_BLK;
  for (int r = r0 + wave; r < min(r0 + PRED_ROWS_PER_BLK, rows); r += 4) {
    const float mu = stat[2 * r], rs = stat[2 * r + 1];
    float4 xh[NV], dx[NV], av[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      av[i] = *reinterpret_cast<const float4*>(a + (long)r * D + c);
      const float4 dy = *reinterpret_cast<const float4*>(dh + (long)r * D + c);
      xh[i] = make_float4((gelu_erf(av[i].x) - mu) * rs, (gelu_erf(av[i].y) - mu) * rs, (gelu_erf(av[i].z) - mu) * rs,
                          (gelu_erf(av[i].w) - mu) * rs);
      ln_bwd_acc(dy, xh[i], w[i], pg[i], pb[i], dx[i], s1, s2);
    }
    float m1, m2;
    ln_bwd_means(s1, s2, D, m1, m2);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      float4 o;
      o.x = ln_bwd_dx(dx[i].x, xh[i].x, m1, m2, rs) * gelu_erf_grad(av[i].x);
      o.y = ln_bwd_dx(dx[i].y, xh[i].y, m1, m2, rs) * gelu_erf_grad(av[i].y);
      o.z = ln_bwd_dx(dx[i].z, xh[i].z, m1, m2, rs) * gelu_erf_grad(av[i].z);
      o.w = ln_bwd_dx(dx[i].w, xh[i].w, m1, m2, rs) * gelu_erf_grad(av[i].w);
      pa[i].x += o.x; pa[i].y += o.y; pa[i].z += o.z; pa[i].w += o.w;
      *reinterpret_cast<float4*>(da + (long)r * D + c) = o;
    }
  }
  // (this merge stays literal in the kernel - behind a shared helper the row loop above compiles to other bits: DESIGN "Head row primitives")
  for (int ph = 0; ph < 4; ++ph) {
    if (wave == ph) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        const float x0[4] = {pg[i].x, pg[i].y, pg[i].z, pg[i].w}, x1[4] = {pb[i].x, pb[i].y, pb[i].z, pb[i].w},
                    x2[4] = {pa[i].x, pa[i].y, pa[i].z, pa[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          red[0][c + j] = ph == 0 ? x0[j] : red[0][c + j] + x0[j];
          red[1][c + j] = ph == 0 ? x1[j] : red[1][c + j] + x1[j];
          red[2][c + j] = ph == 0 ? x2[j] : red[2][c + j] + x2[j];
        }
      }
    }
    __syncthreads();
  }
  float* out = part + (long)blockIdx.x * 3 * D;
  for (int c = threadIdx.x; c < 3 * D; c += 256) out[c] = (&red[0][0])[c];
}

// dgamma[c] += sum_blk part[blk][0][c], dbeta[c] += ...[1][c], dbt[c] += ...[2][c], in workgroup order
__global__ __launch_bounds__(256) void pred_param_grad_kernel(const float* __restrict__ part, int nblk, int D, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, float* __restrict__ dbt) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= D) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int k = 0; k < nblk; ++k) {
    s0 += part[(long)k * 3 * D + c];
    s1 += part[(long)k * 3 * D + D + c];
    s2 += part[(long)k * 3 * D + 2 * D + c];
  }
  dgamma[c] += s0;
  dbeta[c] += s1;
  dbt[c] += s2;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
int row_grid(int rows, int D) { return std::min(1024, cdiv((long)rows * D / 4, 256)); }      // gather / scatter: one float4 per thread

template <typename T, bool HT>
int row_pass_fwd(const PredTransform& t, const float* params, const PredWs& w, int rows, hipStream_t s) {
  if (t.D == 768)
    RMCL_LAUNCH((pred_gelu_ln_fwd_kernel<T, 3, HT>), dim3(cdiv(rows, 4)), dim3(256), 0, s, w.a, params + t.lg, params + t.lb, (T*)w.h, (T*)w.hT, w.stat, rows);
  else
    RMCL_LAUNCH((pred_gelu_ln_fwd_kernel<T, 1, HT>), dim3(cdiv(rows, 4)), dim3(256), 0, s, w.a, params + t.lg, params + t.lb, (T*)w.h, (T*)w.hT, w.stat, rows);
  RMCL_CHECK_LAUNCH();
  return 0;
}
}  // namespace

int pred_transform_forward(const PredTransform& t, const float* params, const float* xn, const int* idx, const int* count, int rows, int dtype,
                           const PredWs& w, hipStream_t s) {
  const int D = t.D;
  RMCL_LAUNCH(pred_gather_kernel, dim3(row_grid(rows, D)), dim3(256), 0, s, xn, idx, count, w.x, rows, D);
  RMCL_CHECK_LAUNCH();
  GemmArgs g0 = head_gemm(w.x, params + t.tw, w.a, rows, D, D, D, D, D, GEMM_TAG_HEAD);                                    // a = x Wt^T + bt
  g0.epi = EPI_BIAS;
  g0.bias = params + t.tb;
  RMCL_TRY(rmcl_launch_gemm(g0, RMCL_F32, RMCL_F32, 1, 1, 1, s));
  if (dtype == RMCL_BF16) return w.hT ? row_pass_fwd<bf16_t, true>(t, params, w, rows, s) : row_pass_fwd<bf16_t, false>(t, params, w, rows, s);
  return w.hT ? row_pass_fwd<float, true>(t, params, w, rows, s) : row_pass_fwd<float, false>(t, params, w, rows, s);
}

int pred_transform_backward(const PredTransform& t, const float* params, const PredWs& w, const int* idx, const int* count, int rows, float* G,
                            float* dxn, hipStream_t s) {
  const int D = t.D, nblk = cdiv(rows, PRED_ROWS_PER_BLK);
  if (D == 768)
    RMCL_LAUNCH(pred_gelu_ln_bwd_kernel<3>, dim3(nblk), dim3(256), 0, s, w.dh, w.a, w.stat, params + t.lg, w.da, w.lnpart, rows);
  else
    RMCL_LAUNCH(pred_gelu_ln_bwd_kernel<1>, dim3(nblk), dim3(256), 0, s, w.dh, w.a, w.stat, params + t.lg, w.da, w.lnpart, rows);
  RMCL_CHECK_LAUNCH();
  if (G) {
    RMCL_LAUNCH(pred_param_grad_kernel, dim3(cdiv(D, 256)), dim3(256), 0, s, w.lnpart, nblk, D, G + t.lg, G + t.lb, G + t.tb);
    RMCL_CHECK_LAUNCH();
    GemmArgs gw = head_gemm(w.da, w.x, G + t.tw, D, D, rows, D, D, D, GEMM_TAG_HEAD);                                       // dWt += da^T x
    gw.epi = EPI_ACCUM;
    RMCL_TRY(rmcl_launch_gemm(gw, RMCL_F32, RMCL_F32, 0, 0, 1, s));
  }
  if (dxn) {
    RMCL_TRY(rmcl_launch_gemm(head_gemm(w.da, params + t.tw, w.dx, rows, D, D, D, D, D, GEMM_TAG_HEAD), RMCL_F32, RMCL_F32, 1, 0, 1, s));   // dx = da Wt
    RMCL_LAUNCH(pred_scatter_kernel, dim3(row_grid(rows, D)), dim3(256), 0, s, w.dx, idx, count, dxn, rows, D);
    RMCL_CHECK_LAUNCH();
  }
  return 0;
}
