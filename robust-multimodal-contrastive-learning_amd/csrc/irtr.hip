// Image-text retrieval (IRTR): the rank head of compute_irtr / compute_irtr_recall (objectives.py:1180-1346, vilt_module.py:233-239)
// and the token assembly of the cached rank pass.
//
//   score     s[i] = cls[i] . w + b (rank_output = Linear(D, 1) on the pooled cls rows): one wave per sequence, written to scores[i] or,
//             through an index array, straight into the [n_img, n_txt] score matrix of the recall evaluation.
//   ce        softmax cross-entropy against answer 0 over each group of R = 1 + draw_false_text scores (R <= 64): one workgroup, wave w owns
//             groups w, w + 4, ... (one lane per score).  Mean loss, correct-group count and dscore = grad_scale * d loss / d score.
//   backward  dcls[i, :] = dscore[i] * w;  dw[c] += sum_i dscore[i] * cls[i, c] (one thread per column, i ascending);  db += sum_i dscore[i].
//   visual    the image side of visual_embed (vision_transformer.py:559-677) WITHOUT the token-type row: cls / patch embedding + position
//             rows into [B, 1 + P, D].
//   assemble  one sequence of the rank pass = its text embedding (already in x) + the cached token rows of image img_of[b] + token-type
//             row 1, and its attention mask = text mask | cached image mask.
// Every reduction has a fixed order and nothing uses float atomics: two identical calls give identical bits.
#include "rmcl_common.h"
#include "kernels.h"
#include "head_rows.h"
#include "../../include/rmcl.h"

namespace {

#define IRTR_WAVES 4
#define IRTR_MAX_R 64

__global__ __launch_bounds__(256) void irtr_score_kernel(const float* __restrict__ cls, long ld_cls, const float* __restrict__ w,
                                                         const float* __restrict__ bias, int S, int D, float* __restrict__ scores,
                                                         const int* __restrict__ out_index, long out_n) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= S) return;
  const float* row = cls + (long)i * ld_cls;
  float acc = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const float4 x = *reinterpret_cast<const float4*>(row + c), ww = *reinterpret_cast<const float4*>(w + c);
    acc += x.x * ww.x + x.y * ww.y + x.z * ww.z + x.w * ww.w;
  }
  acc = wave_sum(acc) + bias[0];
  if (lane == 0) {
    const long o = out_index ? (long)out_index[i] : (long)i;
    if (o >= 0 && o < out_n) scores[o] = acc;              // an index outside the matrix is dropped, never written
  }
}

__global__ __launch_bounds__(256) void irtr_ce_kernel(const float* __restrict__ scores, int B, int R, float gscale,
                                                      const float* __restrict__ gscale_dev, float* __restrict__ dscore,
                                                      float* __restrict__ rows, float* __restrict__ stats) {
  __builtin_assume(R >= 1 && R <= IRTR_MAX_R);             // (the launcher requires it: the dscore loop runs at most once per lane)
  // answer 0 in every group, pitch R, two stats (runtime.py allocates two floats)
  softmax_ce_rows(scores, R, nullptr, B, R, gscale, gscale_dev, dscore, R, rows, nullptr, nullptr, 0, stats, 2);
}

// blocks [0, nbw): one thread per column c of w (dw, and db in block 0's first wave); blocks [nbw, ...): dcls, one float4 per thread
__global__ __launch_bounds__(256) void irtr_bwd_kernel(const float* __restrict__ dscore, const float* __restrict__ cls, long ld_cls,
                                                       const float* __restrict__ w, int S, int D, float* __restrict__ dcls,
                                                       float* __restrict__ dw, float* __restrict__ db, int nbw) {
  if ((int)blockIdx.x < nbw) {
    if (!dw) return;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < D) {
      float acc = 0.f;
#pragma unroll 4
      for (int i = 0; i < S; ++i) acc += dscore[i] * cls[(long)i * ld_cls + c];
      dw[c] += acc;
    }
    if (blockIdx.x == 0 && threadIdx.x < 64 && db) {
      float acc = 0.f;
      for (int i = threadIdx.x; i < S; i += 64) acc += dscore[i];
      acc = wave_sum(acc);
      if (threadIdx.x == 0) db[0] += acc;
    }
    return;
  }
  const int dv = D / 4;
  const long j = (long)(blockIdx.x - nbw) * 256 + threadIdx.x;
  if (j >= (long)S * dv) return;
  const int i = (int)(j / dv), c = (int)(j % dv) * 4;
  const float g = dscore[i];
  const float4 ww = *reinterpret_cast<const float4*>(w + c);
  *reinterpret_cast<float4*>(dcls + (long)i * D + c) = make_float4(g * ww.x, g * ww.y, g * ww.z, g * ww.w);
}

// out[b, tok] = (tok == 0 ? cls : pe[b * P + tok - 1]) + pos[tok]   (pos_bstride = 0: the shared table; else per-sample resized rows)
__global__ __launch_bounds__(256) void visual_assemble_kernel(const float* __restrict__ pe, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, long pos_bstride, float* __restrict__ out,
                                                              int B, int P, int D) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int dv = D / 4;
  if (i >= (long)B * (P + 1) * dv) return;
  const int c = (int)(i % dv) * 4;
  const int tok = (int)((i / dv) % (P + 1)), b = (int)(i / ((long)dv * (P + 1)));
  const float4 a = tok == 0 ? *reinterpret_cast<const float4*>(cls + c)
                            : *reinterpret_cast<const float4*>(pe + ((long)b * P + tok - 1) * D + c);
  const float4 p = *reinterpret_cast<const float4*>(pos + (long)b * pos_bstride + (long)tok * D + c);
  *reinterpret_cast<float4*>(out + ((long)b * (P + 1) + tok) * D + c) = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
}

// x[b * N + L + tok] = embeds[img_of[b], tok] + vtype1;  co[b, 0:L] = text_mask != 0;  co[b, L + tok] = masks[img_of[b], tok].
// A sequence whose image index is outside [0, n_img) gets zero rows and a zero image mask (nothing is read out of bounds).
__global__ __launch_bounds__(256) void rank_assemble_kernel(const float* __restrict__ embeds, const int* __restrict__ masks,
                                                            const int* __restrict__ img_of, int n_img, int ld_tok,
                                                            const long* __restrict__ text_mask, const float* __restrict__ vtype1,
                                                            float* __restrict__ x, int* __restrict__ co, int B, int P, int L, int N, int D) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int dv = D / 4;
  if (i >= (long)B * N * dv) return;
  const int c = (int)(i % dv) * 4;
  const int t = (int)((i / dv) % N), b = (int)(i / ((long)dv * N));
  if (t < L) {
    if (c == 0) co[(long)b * N + t] = text_mask[(long)b * L + t] != 0;
    return;
  }
  const int tok = t - L, im = img_of[b];
  const bool ok = im >= 0 && im < n_img;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) {
    const float4 a = *reinterpret_cast<const float4*>(embeds + ((long)im * ld_tok + tok) * D + c);
    const float4 ty = *reinterpret_cast<const float4*>(vtype1 + c);
    o = make_float4(a.x + ty.x, a.y + ty.y, a.z + ty.z, a.w + ty.w);
  }
  *reinterpret_cast<float4*>(x + ((long)b * N + t) * D + c) = o;
  if (c == 0) co[(long)b * N + t] = ok ? (masks[(long)im * ld_tok + tok] != 0) : 0;
}

}  // namespace

int rmcl_visual_assemble(const float* pe, const float* cls, const float* pos, int pos_per_sample, float* out, int B, int P, int D,
                         hipStream_t s) {
  RMCL_REQUIRE(D % 4 == 0, "visual_assemble: D%4");
  RMCL_LAUNCH(visual_assemble_kernel, dim3(cdiv((long)B * (P + 1) * (D / 4), 256)), dim3(256), 0, s, pe, cls, pos,
              pos_per_sample ? (long)(P + 1) * D : 0L, out, B, P, D);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_rank_assemble(const float* embeds, const int* masks, const int* img_of, int n_img, int ld_tok, const long* text_mask,
                       const float* vtype1, float* x, int* co, int B, int P, int L, int N, int D, hipStream_t s) {
  RMCL_REQUIRE(D % 4 == 0 && N == L + 1 + P && P + 1 <= ld_tok && n_img >= 1, "rank_assemble: bad shape (N = L + 1 + P, P + 1 <= ld_tok)");
  RMCL_LAUNCH(rank_assemble_kernel, dim3(cdiv((long)B * N * (D / 4), 256)), dim3(256), 0, s, embeds, masks, img_of, n_img, ld_tok, text_mask,
              vtype1, x, co, B, P, L, N, D);
  RMCL_CHECK_LAUNCH();
  return 0;
}

extern "C" {

int rmcl_irtr_score(const float* cls, int64_t ld_cls, const float* w, const float* bias, int S, int D, float* scores,
                    const int32_t* out_index, int64_t out_n, void* stream) {
  RMCL_REQUIRE(cls && w && bias && scores, "irtr_score: NULL argument");
  RMCL_REQUIRE(S >= 1 && D >= 4 && D % 4 == 0 && ld_cls >= D && ld_cls % 4 == 0 && out_n >= 1, "irtr_score: bad shape (D % 4 == 0, ld_cls >= D)");
  RMCL_REQUIRE(out_index || out_n >= S, "irtr_score: scores holds fewer than S elements");
  RMCL_LAUNCH(irtr_score_kernel, dim3(cdiv(S, 4)), dim3(256), 0, (hipStream_t)stream, cls, (long)ld_cls, w, bias, S, D, scores, out_index,
              (long)out_n);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_irtr_ce(const float* scores, int B, int R, float grad_scale, const float* grad_scale_dev, float* dscore, float* rows, float* stats,
                 void* stream) {
  RMCL_REQUIRE(scores && stats, "irtr_ce: NULL argument");
  RMCL_REQUIRE(B >= 1 && B <= 65536 && R >= 1 && R <= IRTR_MAX_R, "irtr_ce: bad shape (1 <= R <= 64, 1 <= B <= 65536)");
  RMCL_LAUNCH(irtr_ce_kernel, dim3(1), dim3(64 * IRTR_WAVES), 0, (hipStream_t)stream, scores, B, R, grad_scale, grad_scale_dev, dscore, rows,
              stats);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_irtr_bwd(const float* dscore, const float* cls, int64_t ld_cls, const float* w, int S, int D, float* dcls, float* dw, float* db,
                  void* stream) {
  RMCL_REQUIRE(dscore && cls && w && dcls, "irtr_bwd: NULL argument");
  RMCL_REQUIRE(S >= 1 && D >= 4 && D % 4 == 0 && ld_cls >= D, "irtr_bwd: bad shape (D % 4 == 0, ld_cls >= D)");
  const int nbw = (int)cdiv(D, 256);
  RMCL_LAUNCH(irtr_bwd_kernel, dim3(nbw + (unsigned)cdiv((long)S * (D / 4), 256)), dim3(256), 0, (hipStream_t)stream, dscore, cls, (long)ld_cls,
              w, S, D, dcls, dw, db, nbw);
  RMCL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
