// VQAv2 fine-tuning head (vilt_module.py:164-172: Linear(D,H) - LayerNorm(H) - GELU - Linear(H,N), H = 2D, N = vqav2_label_size)
// and the soft-target BCE of compute_vqa / compute_vqa_attack / PGDAttack_vqa (objectives.py:813-896, pgd_attack_vilt.py:418-483).
//
// Shapes: the batch is the SHORT dimension (B <= 256 rows), the features are 768 -> 1536 -> 3129.  So
//   * the two linears and their data gradients are weight-streaming skinny GEMMs (exact fp32, gemm_exact.hip), the biases in their
//     epilogues;
//   * the weight gradients are outer-product GEMMs with K = B (the short-K TN kernel of gemm_exact.hip), the bias gradients are its
//     column-sum by-product (EPI_COLSUM) - no separate pass;
//   * LayerNorm + GELU forward and GELU' + LayerNorm backward are one row pass each (one wave per row, DPP row sums);
//   * the BCE reads the targets sparsely (labels / scores per row) and scatters them into an LDS row.
// 3129 is not a multiple of 16: the logits / dz buffers have a pitch ldl (3136), whose pad columns are excluded from the loss and the
// argmax and carry dz = 0, and the arena keeps ldl rows for the last weight (rows N..ldl-1 zero), so dz W3 runs with K = ldl.
// Nothing here uses float atomics: loss, score, dz and every gradient are bit-reproducible.
#include <algorithm>
#include "rmcl_common.h"
#include "kernels.h"
#include "head_rows.h"
#include "../../include/rmcl.h"

namespace {

#define VQA_ROWS_PER_BLK 16     // rows of one LayerNorm-backward workgroup (one partial of dgamma / dbeta per workgroup)
#define VQA_MAX_N 4096          // widest label set the BCE row kernel stages in LDS

// g = GELU(LayerNorm(h)) per row, eps 1e-5, exact-erf GELU; stat[2 row] = (mean, rstd).  One wave per row, NV float4 per lane
// (H = 256 NV: no column guards).
template <int NV>
__global__ __launch_bounds__(256) void vqa_ln_gelu_fwd_kernel(const float* __restrict__ h, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ g,
                                                              float* __restrict__ stat, int B) {
  constexpr int H = 256 * NV;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B) return;
  const float* hr = h + (long)row * H;
  float4 v[NV], w[NV], bb[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    v[i] = *reinterpret_cast<const float4*>(hr + c);
    w[i] = *reinterpret_cast<const float4*>(gamma + c);
    bb[i] = *reinterpret_cast<const float4*>(beta + c);
  }
  float s = 0.f, mu, rs;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += sum4_pairwise(v[i]);
  ln_row_stats<NV>(v, s, 1e-5f, mu, rs);
  float* gr = g + (long)row * H;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    float4 o;
    o.x = gelu_erf((v[i].x - mu) * rs * w[i].x + bb[i].x);
    o.y = gelu_erf((v[i].y - mu) * rs * w[i].y + bb[i].y);
    o.z = gelu_erf((v[i].z - mu) * rs * w[i].z + bb[i].z);
    o.w = gelu_erf((v[i].w - mu) * rs * w[i].w + bb[i].w);
    *reinterpret_cast<float4*>(gr + c) = o;
  }
  if (lane == 0) {
    stat[2 * row] = mu;
    stat[2 * row + 1] = rs;
  }
}

// dh = LayerNorm'( GELU'(y) * dg ) per row, y = gamma xhat + beta recomputed from h and the stashed (mean, rstd).
// part != NULL: this workgroup's sums over its VQA_ROWS_PER_BLK rows of dy * xhat (-> dgamma) and dy (-> dbeta), dy = GELU'(y) dg,
// written to part[blk][2][H]; the four waves meet in LDS in a fixed order.
template <int NV>
__global__ __launch_bounds__(256) void vqa_ln_gelu_bwd_kernel(const float* __restrict__ dg, const float* __restrict__ h,
                                                              const float* __restrict__ stat, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ dh,
                                                              float* __restrict__ part, int B) {
  constexpr int H = 256 * NV;
  __shared__ float red[2][H];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float4 w[NV], bb[NV], pg[NV], pb[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (lane + 64 * i) * 4;
    w[i] = *reinterpret_cast<const float4*>(gamma + c);
    bb[i] = *reinterpret_cast<const float4*>(beta + c);
    pg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    pb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int r0 = blockIdx.x * VQA_ROWS_PER_BLK;
  for (int r = r0 + wave; r < min(r0 + VQA_ROWS_PER_BLK, B); r += 4) {
    const float mu = stat[2 * r], rs = stat[2 * r + 1];
    float4 xh[NV], dx[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      const float4 hv = *reinterpret_cast<const float4*>(h + (long)r * H + c);
      const float4 gv = *reinterpret_cast<const float4*>(dg + (long)r * H + c);
      xh[i] = make_float4((hv.x - mu) * rs, (hv.y - mu) * rs, (hv.z - mu) * rs, (hv.w - mu) * rs);
      const float4 dy = make_float4(gv.x * gelu_erf_grad(xh[i].x * w[i].x + bb[i].x), gv.y * gelu_erf_grad(xh[i].y * w[i].y + bb[i].y),
                                    gv.z * gelu_erf_grad(xh[i].z * w[i].z + bb[i].z), gv.w * gelu_erf_grad(xh[i].w * w[i].w + bb[i].w));
      ln_bwd_acc(dy, xh[i], w[i], pg[i], pb[i], dx[i], s1, s2);
    }
    float m1, m2;
    ln_bwd_means(s1, s2, H, m1, m2);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (lane + 64 * i) * 4;
      float4 o;
      o.x = ln_bwd_dx(dx[i].x, xh[i].x, m1, m2, rs);
      o.y = ln_bwd_dx(dx[i].y, xh[i].y, m1, m2, rs);
      o.z = ln_bwd_dx(dx[i].z, xh[i].z, m1, m2, rs);
      o.w = ln_bwd_dx(dx[i].w, xh[i].w, m1, m2, rs);
      *reinterpret_cast<float4*>(dh + (long)r * H + c) = o;
    }
  }
  if (!part) return;                                       // (uniform over the workgroup: no barrier is skipped by some threads only)
  // (this merge stays literal in the kernel - behind a shared helper the row loop above compiles to other bits: DESIGN "Head row primitives")
  for (int ph = 0; ph < 4; ++ph) {
    if (wave == ph) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        const float a[4] = {pg[i].x, pg[i].y, pg[i].z, pg[i].w}, b[4] = {pb[i].x, pb[i].y, pb[i].z, pb[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          red[0][c + j] = ph == 0 ? a[j] : red[0][c + j] + a[j];
          red[1][c + j] = ph == 0 ? b[j] : red[1][c + j] + b[j];
        }
      }
    }
    __syncthreads();
  }
  float* out = part + (long)blockIdx.x * 2 * H;
  for (int c = threadIdx.x; c < 2 * H; c += 256) out[c] = (&red[0][0])[c];
}

// dgamma[c] += sum_blk part[blk][0][c], dbeta[c] += sum_blk part[blk][1][c] in workgroup order
__global__ __launch_bounds__(256) void vqa_ln_param_grad_kernel(const float* __restrict__ part, int nblk, int H, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= H) return;
  float sg = 0.f, sb = 0.f;
  for (int k = 0; k < nblk; ++k) {
    sg += part[(long)k * 2 * H + c];
    sb += part[(long)k * 2 * H + H + c];
  }
  dgamma[c] += sg;
  dbeta[c] += sb;
}

// the dense target row of sample b in LDS: 0, then t[label] = score in list order (a repeated label keeps its LAST score, like the
// reference's loop); pads (label < 0) and labels outside [0, N) are skipped
__device__ __forceinline__ void vqa_target_row(float* T, const int* __restrict__ labels, const float* __restrict__ scores, int A, int b, int N) {
  for (int c = threadIdx.x; c < N; c += blockDim.x) T[c] = 0.f;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int a = 0; a < A; ++a) {
      const int l = labels[(long)b * A + a];
      if (l >= 0 && l < N) T[l] = scores[(long)b * A + a];
    }
  __syncthreads();
}

// One workgroup per sample: BCE-with-logits summed over the N classes, first-maximum argmax and the score t[argmax]; optionally
// dz = gscale (sigmoid(z) - t) / B (pad columns: 0).  rows[2 b] = (row BCE sum, row score), argmax[b].
__global__ __launch_bounds__(256) void vqa_bce_row_kernel(const float* __restrict__ logits, int ldl, const int* __restrict__ labels,
                                                          const float* __restrict__ scores, int A, int B, int N, float gscale,
                                                          const float* __restrict__ gscale_dev, float* __restrict__ dz, float* __restrict__ rows, int* __restrict__ argmax) {
  __shared__ float T[VQA_MAX_N];
  __shared__ float rl[4], rv[4];
  __shared__ int ri[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  vqa_target_row(T, labels, scores, A, b, N);
  const float* zr = logits + (long)b * ldl;
  const float inv_b = (gscale_dev ? gscale * gscale_dev[0] : gscale) / (float)B;
  float loss = 0.f, best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = threadIdx.x; c < N; c += 256) {
    const float z = zr[c], t = T[c];
    const float e = expf(-fabsf(z));
    loss += fmaxf(z, 0.f) - z * t + log1pf(e);
    if (z > best) { best = z; bi = c; }                   // columns grow along the loop: the first maximum of this thread
    if (dz) {
      const float sig = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      dz[(long)b * ldl + c] = inv_b * (sig - t);
    }
  }
  if (dz)
    for (int c = N + threadIdx.x; c < ldl; c += 256) dz[(long)b * ldl + c] = 0.f;
  // block reductions: the loss in a fixed order; argmax = largest value, ties to the smaller column
  loss = wave_sum_dpp(loss);
  wave_argmax_first(best, bi);
  if (lane == 0) { rl[wave] = loss; rv[wave] = best; ri[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = rv[0];
    int i = ri[0];
    for (int w = 1; w < 4; ++w)
      if (rv[w] > v || (rv[w] == v && ri[w] < i)) { v = rv[w]; i = ri[w]; }
    i = (i >= 0 && i < N) ? i : 0;                       // (an all-NaN row: column 0)
    rows[2 * b] = (rl[0] + rl[1]) + (rl[2] + rl[3]);
    rows[2 * b + 1] = T[i];
    argmax[b] = i;
  }
}

// loss2 = (sum_b rows[b].bce / B, sum_b rows[b].score / B): one workgroup, fixed order (strided partials, then a tree in LDS)
__global__ __launch_bounds__(256) void vqa_bce_finish_kernel(const float* __restrict__ rows, int B, float* __restrict__ loss2) {
  __shared__ float red[2][256];
  float l = 0.f, s = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) { l += rows[2 * b]; s += rows[2 * b + 1]; }
  block_tree_sum2(red, l, s);
  if (threadIdx.x == 0) { loss2[0] = red[0][0] / (float)B; loss2[1] = red[1][0] / (float)B; }
}

__global__ __launch_bounds__(256) void vqa_targets_dense_kernel(const int* __restrict__ labels, const float* __restrict__ scores, int A, int N,
                                                                float* __restrict__ out, int ldo) {
  __shared__ float T[VQA_MAX_N];
  const int b = blockIdx.x;
  vqa_target_row(T, labels, scores, A, b, N);
  for (int c = threadIdx.x; c < N; c += 256) out[(long)b * ldo + c] = T[c];
}

struct VqaStash {                    // per pass, all fp32 (rmcl_vqa_stash_floats)
  float *x0, *h, *g, *stat, *t0, *t1, *part;
};
long carve(const rmcl_vqa_head& hd, int B, float* base, VqaStash* s) {
  StashCarver c{base};
  s->x0 = c.take((long)B * hd.D);
  s->h = c.take((long)B * hd.H);
  s->g = c.take((long)B * hd.H);
  s->stat = c.take(2L * B);
  s->t0 = c.take((long)B * hd.H);
  s->t1 = c.take((long)B * hd.H);
  s->part = c.take((long)cdiv(B, VQA_ROWS_PER_BLK) * 2 * hd.H);
  return c.used;
}
bool head_ok(const rmcl_vqa_head* h) {
  return h && h->D >= 64 && h->D % 16 == 0 && (h->H == 512 || h->H == 768 || h->H == 1024 || h->H == 1536 || h->H == 2048) &&
         h->N >= 1 && h->N <= VQA_MAX_N && h->ldl >= h->N && h->ldl % 64 == 0;
}
// TN weight gradient with its bias gradient as the column-sum by-product: only the short-K kernel knows EPI_COLSUM
int wgrad(GemmArgs g, float* colsum, hipStream_t s) {
  g.epi = EPI_ACCUM | EPI_COLSUM;
  g.colsum = colsum;
  RMCL_REQUIRE(rmcl_gemm_tn_shortk_takes(g), "vqa_head_backward: the weight-gradient GEMM does not take the short-K form (B > 256 or skinny forms off)");
  return rmcl_launch_gemm_exact(g, RMCL_F32, RMCL_F32, 0, 0, s);
}
}  // namespace

extern "C" {

int64_t rmcl_vqa_stash_floats(const rmcl_vqa_head* h, int B) {
  VqaStash s;
  return carve(*h, B, nullptr, &s);
}

int rmcl_vqa_head_forward(const rmcl_vqa_head* h, const float* params, const float* cls, int B, float* stash, float* logits, void* stream) {
  RMCL_REQUIRE(head_ok(h), "vqa_head_forward: unsupported head widths (D % 16, H in {512, 768, 1024, 1536, 2048}, N <= 4096, ldl % 64)");
  RMCL_REQUIRE(params && cls && stash && logits && B >= 1 && B <= 256, "vqa_head_forward: NULL argument / B outside 1..256");
  hipStream_t s = (hipStream_t)stream;
  VqaStash st;
  carve(*h, B, stash, &st);
  HIP_TRY(hipMemcpyAsync(st.x0, cls, (size_t)B * h->D * 4, hipMemcpyDeviceToDevice, s));
  GemmArgs g0 = head_gemm(st.x0, params + h->w0, st.h, B, h->H, h->D, h->D, h->D, h->H, GEMM_TAG_HEAD);              // h = cls W0^T + b0
  g0.epi = EPI_BIAS;
  g0.bias = params + h->b0;
  RMCL_TRY(rmcl_launch_gemm_exact(g0, RMCL_F32, RMCL_F32, 1, 1, s));
  const dim3 grid(cdiv(B, 4));
  switch (h->H / 256) {
    case 2: RMCL_LAUNCH(vqa_ln_gelu_fwd_kernel<2>, grid, dim3(256), 0, s, st.h, params + h->g1, params + h->b1, st.g, st.stat, B); break;
    case 3: RMCL_LAUNCH(vqa_ln_gelu_fwd_kernel<3>, grid, dim3(256), 0, s, st.h, params + h->g1, params + h->b1, st.g, st.stat, B); break;
    case 4: RMCL_LAUNCH(vqa_ln_gelu_fwd_kernel<4>, grid, dim3(256), 0, s, st.h, params + h->g1, params + h->b1, st.g, st.stat, B); break;
    case 6: RMCL_LAUNCH(vqa_ln_gelu_fwd_kernel<6>, grid, dim3(256), 0, s, st.h, params + h->g1, params + h->b1, st.g, st.stat, B); break;
    default: RMCL_LAUNCH(vqa_ln_gelu_fwd_kernel<8>, grid, dim3(256), 0, s, st.h, params + h->g1, params + h->b1, st.g, st.stat, B); break;
  }
  RMCL_CHECK_LAUNCH();
  GemmArgs g3 = head_gemm(st.g, params + h->w3, logits, B, h->N, h->H, h->H, h->H, h->ldl, GEMM_TAG_HEAD);             // logits = g W3^T + b3
  g3.epi = EPI_BIAS;
  g3.bias = params + h->b3;
  return rmcl_launch_gemm_exact(g3, RMCL_F32, RMCL_F32, 1, 1, s);
}

int rmcl_vqa_bce(const float* logits, int ldl, const int32_t* labels, const float* scores, int A, int B, int N, float grad_scale,
                 const float* grad_scale_dev, float* dz, float* rows, int32_t* argmax, float* loss2, void* stream) {
  RMCL_REQUIRE(logits && rows && argmax && loss2 && B >= 1 && N >= 1 && N <= VQA_MAX_N && ldl >= N, "vqa_bce: NULL argument / bad shape");
  RMCL_REQUIRE(A == 0 || (labels && scores), "vqa_bce: NULL label / score table");
  hipStream_t s = (hipStream_t)stream;
  RMCL_LAUNCH(vqa_bce_row_kernel, dim3(B), dim3(256), 0, s, logits, ldl, labels, scores, A, B, N, grad_scale, grad_scale_dev, dz, rows,
              argmax);
  RMCL_CHECK_LAUNCH();
  RMCL_LAUNCH(vqa_bce_finish_kernel, dim3(1), dim3(256), 0, s, rows, B, loss2);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_vqa_targets_dense(const int32_t* labels, const float* scores, int A, int B, int N, float* out, int ldo, void* stream) {
  RMCL_REQUIRE(out && B >= 1 && N >= 1 && N <= VQA_MAX_N && ldo >= N && (A == 0 || (labels && scores)), "vqa_targets_dense: bad argument");
  RMCL_LAUNCH(vqa_targets_dense_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, labels, scores, A, N, out, ldo);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_vqa_head_backward(const rmcl_vqa_head* h, const float* params, float* stash, const float* dz, int B, float* G, float* dcls,
                           void* stream) {
  RMCL_REQUIRE(head_ok(h), "vqa_head_backward: unsupported head widths");
  RMCL_REQUIRE(params && stash && dz && dcls && B >= 1 && B <= 256, "vqa_head_backward: NULL argument / B outside 1..256");
  hipStream_t s = (hipStream_t)stream;
  VqaStash st;
  carve(*h, B, stash, &st);
  // dg = dz W3 over the padded K = ldl (dz pad columns are 0, the arena's pad rows of W3 are 0)
  RMCL_TRY(rmcl_launch_gemm_exact(head_gemm(dz, params + h->w3, st.t0, B, h->H, h->ldl, h->ldl, h->H, h->H, GEMM_TAG_HEAD), RMCL_F32, RMCL_F32, 1, 0, s));
  if (G) RMCL_TRY(wgrad(head_gemm(dz, st.g, G + h->w3, h->N, h->H, B, h->ldl, h->H, h->H, GEMM_TAG_HEAD), G + h->b3, s));   // dW3 += dz^T g, db3 += sum dz
  const int nblk = cdiv(B, VQA_ROWS_PER_BLK);
  float* part = G ? st.part : nullptr;
  switch (h->H / 256) {
    case 2: RMCL_LAUNCH(vqa_ln_gelu_bwd_kernel<2>, dim3(nblk), dim3(256), 0, s, st.t0, st.h, st.stat, params + h->g1, params + h->b1, st.t1, part, B); break;
    case 3: RMCL_LAUNCH(vqa_ln_gelu_bwd_kernel<3>, dim3(nblk), dim3(256), 0, s, st.t0, st.h, st.stat, params + h->g1, params + h->b1, st.t1, part, B); break;
    case 4: RMCL_LAUNCH(vqa_ln_gelu_bwd_kernel<4>, dim3(nblk), dim3(256), 0, s, st.t0, st.h, st.stat, params + h->g1, params + h->b1, st.t1, part, B); break;
    case 6: RMCL_LAUNCH(vqa_ln_gelu_bwd_kernel<6>, dim3(nblk), dim3(256), 0, s, st.t0, st.h, st.stat, params + h->g1, params + h->b1, st.t1, part, B); break;
    default: RMCL_LAUNCH(vqa_ln_gelu_bwd_kernel<8>, dim3(nblk), dim3(256), 0, s, st.t0, st.h, st.stat, params + h->g1, params + h->b1, st.t1, part, B); break;
  }
  RMCL_CHECK_LAUNCH();
  if (G) {
    RMCL_LAUNCH(vqa_ln_param_grad_kernel, dim3(cdiv(h->H, 256)), dim3(256), 0, s, st.part, nblk, h->H, G + h->g1, G + h->b1);
    RMCL_CHECK_LAUNCH();
    RMCL_TRY(wgrad(head_gemm(st.t1, st.x0, G + h->w0, h->H, h->D, B, h->H, h->D, h->D, GEMM_TAG_HEAD), G + h->b0, s));   // dW0 += dh^T cls, db0 += sum dh
  }
  return rmcl_launch_gemm_exact(head_gemm(st.t1, params + h->w0, dcls, B, h->D, h->H, h->H, h->D, h->D, GEMM_TAG_HEAD), RMCL_F32, RMCL_F32, 1, 0, s);   // dcls
}

}  // extern "C"
