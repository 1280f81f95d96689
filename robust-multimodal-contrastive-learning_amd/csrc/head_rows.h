// Row primitives that only the task heads share (vqa.hip, nlvr2.hip, irtr.hip, head_transform.hip, mlm.hip, mpp.hip; barlow.hip takes
// the host helpers), and the host interface of the prediction-head transform that mlm.hip and mpp.hip call (head_transform.hip).
// Every piece has a fixed summation order and uses no float atomics: a kernel built from them gives identical bits per call.
// The kernels keep what is their own - where GELU sits, eps, where gamma / beta are loaded, what is stored; nothing here knows
// which head calls it.  The encoder's LayerNorm (norm_softmax.hip: left-to-right sums, rsqrtf) and the text embedding's
// (embed_misc.hip: butterfly sums) are different arithmetic and stay out (DESIGN.md "Head row primitives").
// The LayerNorm pieces work on one float4 / one element, not on whole register arrays, on purpose: these files are built with
// -ffp-contract=fast, which multiply fuses into which add is decided over the whole unrolled row loop, and only the same statements
// in the same order reproduce the kernels' bits (whole-array helpers changed the count of fused multiply-adds in the backward kernels).
#pragma once
#include "rmcl_common.h"
#include "gemm.h"

// ---- LayerNorm row pass: one wave per row of H = 256 NV floats, lane l holds the float4 at columns (l + 64 i) * 4, i < NV ------------
// the lane's share of a row sum, one float4: pairwise.  A row sum is these added float4 after float4, then the DPP wave sum.
__device__ __forceinline__ float sum4_pairwise(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
// forward statistics from the lane's sum s of its NV float4: mean, centred squares (pairwise again), rs = 1 / sqrtf(var + eps)
template <int NV>
__device__ __forceinline__ void ln_row_stats(const float4 (&v)[NV], float s, float eps, float& mu, float& rs) {
  constexpr int H = 256 * NV;
  mu = wave_sum_dpp(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float a = v[i].x - mu, b = v[i].y - mu, c = v[i].z - mu, d = v[i].w - mu;
    q += (a * a + b * b) + (c * c + d * d);
  }
  rs = 1.0f / sqrtf(wave_sum_dpp(q) / (float)H + eps);
}
// backward, first half, one float4 of a row: this wave's running partials pg += dy * xhat (-> dgamma), pb += dy (-> dbeta) over its
// rows; dx = dy * gamma (d xhat); the lane's running sums s1 += dx, s2 += dx * xhat (pairwise inside the float4)
__device__ __forceinline__ void ln_bwd_acc(const float4& dy, const float4& xh, const float4& w, float4& pg, float4& pb, float4& dx,
                                           float& s1, float& s2) {
  pg.x = fmaf(dy.x, xh.x, pg.x); pg.y = fmaf(dy.y, xh.y, pg.y);
  pg.z = fmaf(dy.z, xh.z, pg.z); pg.w = fmaf(dy.w, xh.w, pg.w);
  pb.x += dy.x; pb.y += dy.y; pb.z += dy.z; pb.w += dy.w;
  dx = make_float4(dy.x * w.x, dy.y * w.y, dy.z * w.z, dy.w * w.w);
  s1 += (dx.x + dx.y) + (dx.z + dx.w);
  s2 += (dx.x * xh.x + dx.y * xh.y) + (dx.z * xh.z + dx.w * xh.w);
}
// the row means of the two sums: m1 = mean(dx), m2 = mean(dx * xhat) over H columns, by the DPP wave sum
__device__ __forceinline__ void ln_bwd_means(float s1, float s2, int H, float& m1, float& m2) {
  m1 = wave_sum_dpp(s1) / (float)H;
  m2 = wave_sum_dpp(s2) / (float)H;
}
// backward, second half, one element: d input of the normalisation = rs * (dx - m1 - xhat * m2)
__device__ __forceinline__ float ln_bwd_dx(float dx, float xh, float m1, float m2, float rs) { return rs * (dx - m1 - xh * m2); }

// ---- softmax cross-entropy over B rows of N <= 64 logits: one workgroup of four waves ------------------------------------------------
// Wave w owns rows w, w + 4, ... (one lane per column), lane 0 keeps the wave's running loss in row order, the four waves meet as
// (0 + 1) + (2 + 3).  The label of row b is labels[b] clamped into [0, N), or 0 for every row (labels = NULL).
//   dz [B, ld_dz] (optional) = scale (softmax - onehot), columns N..ld_dz-1 zero;  rows[b] (optional) = lse - z[label];
//   argmax[b] (optional) = first maximum;  ref (optional): logits whose first maximum is compared with this one's;
//   stats = (mean row loss, rows with argmax == label[, rows whose argmax differs from ref's]) - nstats floats, 2 or 3.
__device__ __forceinline__ void softmax_ce_rows(const float* __restrict__ logits, int ldl, const int* __restrict__ labels, int B, int N,
                                                float gscale, const float* __restrict__ gscale_dev, float* __restrict__ dz, int ld_dz,
                                                float* __restrict__ rows, int* __restrict__ argmax, const float* __restrict__ ref,
                                                int ld_ref, float* __restrict__ stats, int nstats) {
  __shared__ float s_loss[4];
  __shared__ int s_hit[4], s_chg[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float scale = (gscale_dev ? gscale * gscale_dev[0] : gscale) / (float)B;
  float loss_acc = 0.f;
  int hit = 0, chg = 0;
  for (int b = wave; b < B; b += 4) {
    const float z = lane < N ? logits[(long)b * ldl + lane] : -INFINITY;
    const float m = wave_max(z);
    const float e = lane < N ? expf(z - m) : 0.f;
    const float s = wave_sum(e);
    const int lbl = labels ? min(max(labels[b], 0), N - 1) : 0;
    const float zl = __shfl(z, lbl, 64);
    float zm = z;
    int am = lane < N ? lane : N;                         // lanes >= N hold -inf / index N
    wave_argmax_first(zm, am);
    am = min(am, N - 1);
    const float row = (logf(s) + m) - zl;
    if (dz) {
      for (int c = lane; c < ld_dz; c += 64)
        dz[(long)b * ld_dz + c] = c < N ? scale * (e / s - (c == lbl ? 1.f : 0.f)) : 0.f;
    }
    int changed = 0;
    if (ref) {
      float zr = lane < N ? ref[(long)b * ld_ref + lane] : -INFINITY;
      int ar = lane < N ? lane : N;
      wave_argmax_first(zr, ar);
      changed = min(ar, N - 1) != am;
    }
    if (lane == 0) {
      if (rows) rows[b] = row;
      if (argmax) argmax[b] = am;
      loss_acc += row;
      hit += am == lbl;
      chg += changed;
    }
  }
  if (lane == 0) {
    s_loss[wave] = loss_acc;
    s_hit[wave] = hit;
    if (nstats > 2) s_chg[wave] = chg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float l = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
    stats[0] = l / (float)B;
    stats[1] = (float)(s_hit[0] + s_hit[1] + s_hit[2] + s_hit[3]);
    if (nstats > 2) stats[2] = (float)(s_chg[0] + s_chg[1] + s_chg[2] + s_chg[3]);
  }
}

// ---- two sums over a workgroup of 256: red[0][0] = sum a, red[1][0] = sum b (the caller's strided partials, then halving in LDS) --------
__device__ __forceinline__ void block_tree_sum2(float (&red)[2][256], float a, float b) {
  red[0][threadIdx.x] = a;
  red[1][threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
    __syncthreads();
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
// a plain GEMM (alpha 1, no split, no batch) of profiling class `tag`; the caller adds its epilogue
static inline GemmArgs head_gemm(const void* A, const void* B, void* C, int M, int N, int K, long lda, long ldb, int ldc, int tag) {
  GemmArgs g = gemm_args(A, B, C, M, N, K, lda, ldb, ldc);
  g.tag = tag;
  return g;
}
// sub-allocation of a stash in 64-float (256-byte) steps; base = NULL: sizes only (used = the floats the stash needs)
struct StashCarver {
  float* base;
  long used = 0;
  float* take(long n) {
    float* p = base ? base + used : nullptr;
    used += (n + 63) / 64 * 64;
    return p;
  }
};

// ---- the BERT prediction-head transform, Linear(D,D) - GELU - LayerNorm(eps 1e-12) over a compacted row list (head_transform.hip) ------
#define PRED_ROWS_PER_BLK 16     // rows of one transform-backward workgroup (one partial of dgamma / dbeta / dbias per workgroup)
struct PredTransform {           // D and the arena offsets of dense.weight [D, D], dense.bias, LayerNorm.weight, LayerNorm.bias
  int D;
  long tw, tb, lg, lb;
};
struct PredWs {                  // views into the calling head's workspace; h / hT [D, rows] in the decoder's operand type, hT may be NULL
  float *x, *a, *stat;
  void *h, *hT;
  float *dh, *da, *dx, *lnpart;
};
static inline bool pred_head_ok(int D) { return D == 256 || D == 768; }
static inline bool pred_rows_ok(int rows) { return rows >= 128 && rows % 128 == 0 && rows <= (1 << 20); }
// the two runs of slices every head's workspace holds in this order, with the head's own slices between and behind them
static inline void pred_carve_fwd(StashCarver& c, int rows, int D, PredWs* w) {
  const long RD = (long)rows * D;
  w->x = c.take(RD);
  w->a = c.take(RD);
  w->stat = c.take(2L * rows);
  w->h = c.take(RD);                                        // (T <= 4 bytes)
  w->hT = nullptr;
}
static inline void pred_carve_bwd(StashCarver& c, int rows, int D, PredWs* w) {
  const long RD = (long)rows * D;
  w->dh = c.take(RD);
  w->da = c.take(RD);
  w->dx = c.take(RD);
  w->lnpart = c.take((long)cdiv(rows, PRED_ROWS_PER_BLK) * 3 * D);
}
// gather xn[idx] into w.x, a = x Wt^T + bt (exact fp32), h (and hT where w.hT is set) = LayerNorm(GELU(a)) in `dtype`, statistics in w.stat
int pred_transform_forward(const PredTransform& t, const float* params, const float* xn, const int* idx, const int* count, int rows, int dtype,
                           const PredWs& w, hipStream_t s);
// from w.dh: da; G != NULL: dgamma / dbeta / dbt and dWt accumulated into G; dxn != NULL: dx = da Wt stored to dxn[idx[r]] (else no dx GEMM)
int pred_transform_backward(const PredTransform& t, const float* params, const PredWs& w, const int* idx, const int* count, int rows, float* G,
                            float* dxn, hipStream_t s);
