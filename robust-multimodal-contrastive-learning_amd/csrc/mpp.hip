// Masked patch prediction head (compute_mpp, objectives.py:632-665; MPPHead, heads.py:198-207; VisionTransformer.mask_tokens,
// vision_transformer.py:525-557):
//   labels    per patch and channel, trunc(mean(img * 0.5 + 0.5 over the 32 x 32 patch) * 255), read from the fp32 image
//   mpp_score = Linear(D,D) - GELU (exact erf) - LayerNorm(D, eps 1e-12) - Linear(D, 768) + bias, the 768 logits read as 3 x 256
//   loss      = cross_entropy(logits.view(-1, 256), labels.view(-1), ignore_index = -100): the mean over the labelled (row, channel) pairs
// Only the masked valid image slots carry labels (~15 % of B x P), so the training path works on those rows, COMPACTED:
//   compact    one workgroup: ascending list of the masked valid slots as rows of xn, their three labels, the count n (on the device)
//   gather + transform   the prediction-head transform shared with the MLM head (head_transform.hip: pred_transform_forward) on the image
//              rows of xn; h is kept in the decoder's operand type
//   decoder    z [rows, 768] = h W^T + bias through the library's GEMM launcher (the logits of 768 columns are small: kept dense)
//   CE         one wave per row: three 256-way softmax cross-entropies (4 columns per lane), lse / first argmax per group, the row loss
//   backward   dz = s (softmax - onehot) / (3 n) from z and lse; dW += dz^T h, dbias += column sums (per 32-row chunk, then the chunks in
//              ascending order), dh = dz W, then pred_transform_backward (the scatter of dx into the zero-filled dxn of the encoder backward included)
// Every output has ONE owner and a fixed summation order (no float atomics): two identical calls give identical bits.
#include <algorithm>
#include "rmcl_common.h"
#include "kernels.h"
#include "head_rows.h"
#include "../../include/rmcl.h"

namespace {

#define MPP_V 768               // decoder width: 3 channels x 256 intensity classes

// ---- labels ---------------------------------------------------------------------------------------------------------------------------
// One wave per (sample, slot): lane l reads the float4 l + 64 k (k < 4) of the 256 float4 of a channel's 32 x 32 patch (row = i / 8),
// pairwise inside the float4, k ascending, then the DPP wave sum.  value = (sum * (1 / 1024)) * 255, truncated.  Pad slots: -100.
__global__ __launch_bounds__(256) void mpp_labels_kernel(const float* __restrict__ img, int B, int H, int W, const int* __restrict__ sel,
                                                         const int* __restrict__ counts, int sel_ld, int gw, int P, int* __restrict__ labels) {
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (slot >= B * P) return;
  const int b = slot / P, j = slot - b * P, gh = H / 32;
  int patch = j;
  bool valid = true;
  if (sel) {
    valid = j < counts[b] && j < sel_ld;
    patch = valid ? sel[(long)b * sel_ld + j] : 0;
  }
  valid = valid && patch >= 0 && patch < gh * gw;
  int* out = labels + (long)slot * 3;
  if (!valid) {                                              // (wave-uniform)
    if (lane < 3) out[lane] = -100;
    return;
  }
  const int py = patch / gw, px = patch - py * gw;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* base = img + (((long)b * 3 + ch) * H + (long)py * 32) * W + (long)px * 32;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = lane + 64 * k, row = i >> 3, c4 = (i & 7) * 4;
      const float4 v = *reinterpret_cast<const float4*>(base + (long)row * W + c4);
      // the reference sums the mapped pixels img * 0.5 + 0.5 (its weights 1 / 1024 are a power of two: scaling commutes with the sum)
      const float4 u = make_float4(v.x * 0.5f + 0.5f, v.y * 0.5f + 0.5f, v.z * 0.5f + 0.5f, v.w * 0.5f + 0.5f);
      s += sum4_pairwise(u);
    }
    const float t = wave_sum_dpp(s);
    const float val = (t * (1.0f / 1024.0f)) * 255.0f;
    if (lane == 0) out[ch] = (int)val;                       // truncation, like .long()
  }
}

// The same labels from the byte feed: img uint8 [B, Hmax, Wmax, 3] (HWC, every sample in its top-left corner), sizes [B, 2] = (h, w), lut =
// the 256 values of ToTensor + Normalize(0.5, 0.5) - the batch u8_to_patches_kernel takes.  The labels equal, integer for integer, those of
// mpp_labels_kernel on Uint8Batch.float_image() of the same bytes, because the arithmetic and its order are that kernel's: the pixel is
// lut[byte] * 0.5f + 0.5f (x * 0.5f is exact, so the contraction into an FMA cannot change a bit), a pixel outside its sample is the
// collate zero of the float batch, 0 * 0.5f + 0.5f (NOT lut[0]: a fully padded patch of the dense form has the label 127), lane l takes
// pixel group i = l + 64 k of patch line i >> 3, columns (i & 7) * 4 .. + 3, k ascending, pairwise inside the group, then the DPP wave sum.
// In HWC a lane's four pixels of all three channels are 12 contiguous bytes: three dwords per k give the three channel sums in ONE pass
// over the patch (the float kernel makes three passes over four times the bytes).
__global__ __launch_bounds__(256) void mpp_labels_u8_kernel(const unsigned char* __restrict__ img, const int* __restrict__ sizes, int B, int Hmax,
                                                            int Wmax, const float* __restrict__ lut, const int* __restrict__ sel,
                                                            const int* __restrict__ counts, int sel_ld, int gw, int P, int* __restrict__ labels) {
  __shared__ float tab[256];
  tab[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (slot >= B * P) return;
  const int b = slot / P, j = slot - b * P, gh = Hmax / 32;
  int patch = j;
  bool valid = true;
  if (sel) {
    valid = j < counts[b] && j < sel_ld;
    patch = valid ? sel[(long)b * sel_ld + j] : 0;
  }
  valid = valid && patch >= 0 && patch < gh * gw;
  int* out = labels + (long)slot * 3;
  if (!valid) {                                              // (wave-uniform)
    if (lane < 3) out[lane] = -100;
    return;
  }
  const int py = patch / gw, px = patch - py * gw;
  // extents clamped to the padded batch, like u8_to_patches_kernel: no read leaves [Hmax, Wmax] whatever `sizes` holds
  const int hb = min(sizes[2 * b], Hmax), wb = min(sizes[2 * b + 1], Wmax);
  float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = lane + 64 * k, y = py * 32 + (i >> 3), x = px * 32 + (i & 7) * 4;
    float u[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int q = 0; q < 4; ++q) u[c][q] = 0.f * 0.5f + 0.5f;
    if (y < hb && x < wb) {                                  // (x + 3 < Wmax: the 12 bytes lie inside the row of the padded batch)
      const uint3 w = *reinterpret_cast<const uint3*>(img + (((long)b * Hmax + y) * Wmax + x) * 3);
      const unsigned wd[3] = {w.x, w.y, w.z};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int byte = q * 3 + c;
          if (x + q < wb) u[c][q] = tab[(wd[byte >> 2] >> ((byte & 3) * 8)) & 0xff] * 0.5f + 0.5f;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += sum4_pairwise(make_float4(u[c][0], u[c][1], u[c][2], u[c][3]));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = wave_sum_dpp(s[c]);
    const float val = (t * (1.0f / 1024.0f)) * 255.0f;
    if (lane == 0) out[c] = (int)val;                        // truncation, like .long()
  }
}

// ---- compaction -----------------------------------------------------------------------------------------------------------------------
// labels [B, P, 3], masked [B, P].  A slot is LISTED when it is masked, valid (its labels are not the pad's -100) and all three labels lie
// in [0, 256); a masked valid slot with a label outside adds its out-of-range entries to count[1] and is skipped.  idx[r] = the row
// b N + L + 1 + j of xn, lab[r][3] its labels, ascending.  all = 1 (the dense-logits pass): EVERY image row b N + L + t, t = 0..P (the cls
// row first), is listed; lab keeps -100 for the cls row and for the slots the compacted form would not list.  Entries behind the count:
// idx -1, lab -100.  count[0] = n.  One workgroup.
__global__ __launch_bounds__(256) void mpp_compact_kernel(const int* __restrict__ labels, const int* __restrict__ masked, int B, int P, int L,
                                                          int N, int all, int cap, int* __restrict__ idx, int* __restrict__ lab,
                                                          int* __restrict__ count) {
  __shared__ int cnt[256], bad[256];
  const int PT = all ? P + 1 : P, M = B * PT;
  const int t = threadIdx.x, per = (M + 255) / 256, b0 = min(M, t * per), b1 = min(M, b0 + per);
  auto state = [&](int i, int* l3) -> int {                  // 1: listed with labels, 0: not labelled; *l3 = out-of-range entries
    const int b = i / PT, tt = i - b * PT, j = all ? tt - 1 : tt;
    l3[0] = l3[1] = l3[2] = -100;
    if (j < 0) return 0;
    const long s = (long)b * P + j;
    if (masked[s] == 0) return 0;
    const int x = labels[s * 3], y = labels[s * 3 + 1], z = labels[s * 3 + 2];
    if (x == -100 && y == -100 && z == -100) return 0;       // a masked pad slot
    const int nb = (x < 0 || x > 255) + (y < 0 || y > 255) + (z < 0 || z > 255);
    if (nb) return -nb;
    l3[0] = x; l3[1] = y; l3[2] = z;
    return 1;
  };
  int c = 0, nbad = 0, l3[3];
  for (int i = b0; i < b1; ++i) {
    const int st = state(i, l3);
    c += (all || st == 1) ? 1 : 0;
    nbad += st < 0 ? -st : 0;
  }
  cnt[t] = c;
  bad[t] = nbad;
  __syncthreads();
  if (t == 0) {
    int s = 0, q = 0;
    for (int i = 0; i < 256; ++i) { const int v = cnt[i]; cnt[i] = s; s += v; q += bad[i]; }
    count[0] = s;
    count[1] = q;
  }
  __syncthreads();
  int o = cnt[t];
  for (int i = b0; i < b1; ++i) {
    const int st = state(i, l3);
    if (all || st == 1) {
      const int b = i / PT, tt = i - b * PT;
      idx[o] = b * N + L + (all ? tt : tt + 1);
      lab[3 * o] = l3[0]; lab[3 * o + 1] = l3[1]; lab[3 * o + 2] = l3[2];
      ++o;
    }
  }
  __syncthreads();
  const int n = count[0];
  for (int i = n + t; i < cap; i += 256) { idx[i] = -1; lab[3 * i] = -100; lab[3 * i + 1] = -100; lab[3 * i + 2] = -100; }
}

// ---- three 256-way softmax cross-entropies per row: one wave per row, lane l holds columns 4 l .. 4 l + 3 of a group ------------------
// lse [rows, 3], argmax [rows, 3] (first maximum), rowloss [rows] = sum over the labelled groups of lse - z[label].  A label of -100
// (the dense-logits pass) leaves its group out of the row loss.  Rows >= n: 0 / -1 / 0.
__global__ __launch_bounds__(256) void mpp_ce_fwd_kernel(const float* __restrict__ z, const int* __restrict__ lab, const int* __restrict__ count,
                                                         int rows, float* __restrict__ lse, int* __restrict__ argmax, float* __restrict__ rowloss) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  if (r >= min(count[0], rows)) {                            // (wave-uniform)
    if (lane < 3) { lse[3 * r + lane] = 0.f; argmax[3 * r + lane] = -1; }
    if (lane == 0) rowloss[r] = 0.f;
    return;
  }
  float loss = 0.f;
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const float4 v = *reinterpret_cast<const float4*>(z + (long)r * MPP_V + g * 256 + lane * 4);
    const float m = wave_max(fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    const float4 e = make_float4(expf(v.x - m), expf(v.y - m), expf(v.z - m), expf(v.w - m));
    const float s = wave_sum_dpp(sum4_pairwise(e));
    float bv = v.x;
    int bi = lane * 4;
    if (v.y > bv) { bv = v.y; bi = lane * 4 + 1; }
    if (v.z > bv) { bv = v.z; bi = lane * 4 + 2; }
    if (v.w > bv) { bv = v.w; bi = lane * 4 + 3; }
    wave_argmax_first(bv, bi);
    const float l = m + logf(s);
    const int lb = lab[3 * r + g];
    const bool has = lb >= 0 && lb < 256;
    const int k = lb & 3;                                    // (the label is the same in every lane: each picks its k-th column)
    const float zl = __shfl(k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)), has ? (lb >> 2) : 0, 64);
    if (has) loss += l - zl;
    if (lane == 0) { lse[3 * r + g] = l; argmax[3 * r + g] = bi; }
  }
  if (lane == 0) rowloss[r] = loss;
}

// stats = (sum_r rowloss / pairs, pairs with argmax == label, pairs), pairs = the labelled (row, channel) entries of the first n rows
// (3 n on the compacted path): one workgroup, fixed order (strided partials, then a tree in LDS).  pairs = 0: 0 / 0 = NaN, like
// F.cross_entropy over an all-ignored batch.
__global__ __launch_bounds__(256) void mpp_stats_kernel(const float* __restrict__ rowloss, const int* __restrict__ argmax,
                                                        const int* __restrict__ lab, const int* __restrict__ count, int rows,
                                                        float* __restrict__ stats) {
  __shared__ float red[2][256];
  __shared__ float redp[2][256];
  const int n = min(count[0], rows);
  float l = 0.f, c = 0.f, p = 0.f;
  for (int r = threadIdx.x; r < n; r += 256) {
    l += rowloss[r];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const int lb = lab[3 * r + g];
      if (lb >= 0 && lb < 256) { p += 1.f; c += argmax[3 * r + g] == lb ? 1.f : 0.f; }
    }
  }
  block_tree_sum2(red, l, c);
  block_tree_sum2(redp, p, 0.f);
  if (threadIdx.x == 0) { stats[0] = red[0][0] / redp[0][0]; stats[1] = red[1][0]; stats[2] = redp[0][0]; }
}

// dz [rows, 768] in T = scale (softmax - onehot) with scale = s / (3 n); rows >= n (and n = 0): exactly 0
template <typename T>
__global__ __launch_bounds__(256) void mpp_ce_bwd_kernel(const float* __restrict__ z, const int* __restrict__ lab, const float* __restrict__ lse,
                                                         const int* __restrict__ count, float gscale, const float* __restrict__ gscale_dev,
                                                         int rows, T* __restrict__ dz) {
  const int n = min(count[0], rows);
  const float scale = n > 0 ? (gscale_dev ? gscale * gscale_dev[0] : gscale) / (3.0f * (float)n) : 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)rows * MPP_V; i += (long)gridDim.x * 256) {
    const int r = (int)(i / MPP_V), v = (int)(i - (long)r * MPP_V), g = v >> 8;
    float o = 0.f;
    if (r < n) {
      const int lb = lab[3 * r + g];
      if (lb >= 0 && lb < 256) o = scale * (expf(z[i] - lse[3 * r + g]) - ((v & 255) == lb ? 1.f : 0.f));
    }
    dz[i] = from_f32<T>(o);
  }
}

// dbias[v] += sum_r dz[r, v] in two steps with a fixed order: part[chunk][v] = the sum over the chunk's MPP_DB_ROWS rows (ascending), then
// the chunks in ascending order, one thread per column
#define MPP_DB_ROWS 32
template <typename T>
__global__ __launch_bounds__(256) void mpp_dbias_part_kernel(const T* __restrict__ dz, const int* __restrict__ count, int rows, float* __restrict__ part) {
  const int v = blockIdx.x * 256 + threadIdx.x, n = min(count[0], rows), r0 = blockIdx.y * MPP_DB_ROWS;
  if (v >= MPP_V) return;
  float s = 0.f;
  for (int r = r0; r < min(r0 + MPP_DB_ROWS, n); ++r) s += to_f32<T>(dz[(long)r * MPP_V + v]);
  part[(long)blockIdx.y * MPP_V + v] = s;
}
__global__ __launch_bounds__(256) void mpp_dbias_merge_kernel(const float* __restrict__ part, const int* __restrict__ count, int rows, float* __restrict__ dbias) {
  const int v = blockIdx.x * 256 + threadIdx.x, n = min(count[0], rows);
  if (v >= MPP_V || n == 0) return;
  float s = 0.f;
  for (int k = 0; k < (n + MPP_DB_ROWS - 1) / MPP_DB_ROWS; ++k) s += part[(long)k * MPP_V + v];
  dbias[v] += s;
}

__global__ __launch_bounds__(256) void mpp_logits_copy_kernel(const float* __restrict__ z, float* __restrict__ out, long n4) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256)
    reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(z)[i];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
struct MppWs {
  PredWs t;                                                 // the transform's slices (head_rows.h); no hT
  float *z, *dbpart;
  void* dz;
};
PredTransform transform_of(const rmcl_mpp_head* h) { return PredTransform{h->D, h->tw, h->tb, h->lg, h->lb}; }
long carve(const rmcl_mpp_head& hd, int rows, float* base, MppWs* w) {
  StashCarver c{base};
  const long RV = (long)rows * MPP_V;
  pred_carve_fwd(c, rows, hd.D, &w->t);
  w->z = c.take(RV);
  w->dz = c.take(RV);
  pred_carve_bwd(c, rows, hd.D, &w->t);
  w->dbpart = c.take((long)cdiv(rows, MPP_DB_ROWS) * MPP_V);
  return c.used;
}
bool head_ok(const rmcl_mpp_head* h) { return h && pred_head_ok(h->D); }
int grid_for(long elems) { return (int)std::min<long>(1024, (elems + 255) / 256); }

template <typename T>
int forward_t(const rmcl_mpp_head* h, const float* params, const T* W, int dtype, const float* xn, const int* idx, const int* lab,
              const int* count, int rows, const MppWs& w, float* lse, float* rowloss, int* argmax, float* stats, hipStream_t s) {
  const int D = h->D;
  RMCL_TRY(pred_transform_forward(transform_of(h), params, xn, idx, count, rows, dtype, w.t, s));
  GemmArgs g1 = head_gemm(w.t.h, W, w.z, rows, MPP_V, D, D, D, MPP_V, GEMM_TAG_HEAD);                                          // z = h W^T + bias
  g1.epi = EPI_BIAS;
  g1.bias = params + h->db;
  RMCL_TRY(rmcl_launch_gemm(g1, dtype, RMCL_F32, 1, 1, dtype == RMCL_F32, s));
  RMCL_LAUNCH(mpp_ce_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, w.z, lab, count, rows, lse, argmax, rowloss);
  RMCL_CHECK_LAUNCH();
  RMCL_LAUNCH(mpp_stats_kernel, dim3(1), dim3(256), 0, s, rowloss, argmax, lab, count, rows, stats);
  RMCL_CHECK_LAUNCH();
  return 0;
}

template <typename T>
int backward_t(const rmcl_mpp_head* h, const float* params, const T* W, int dtype, const int* idx, const int* lab, const int* count, int rows,
               const MppWs& w, const float* lse, float gscale, const float* gscale_dev, float* G, float* dxn, hipStream_t s) {
  const int D = h->D, exact = dtype == RMCL_F32;
  RMCL_LAUNCH(mpp_ce_bwd_kernel<T>, dim3(grid_for((long)rows * MPP_V)), dim3(256), 0, s, w.z, lab, lse, count, gscale, gscale_dev, rows, (T*)w.dz);
  RMCL_CHECK_LAUNCH();
  if (G) {
    GemmArgs gw = head_gemm(w.dz, w.t.h, G + h->dw, MPP_V, D, rows, MPP_V, D, D, GEMM_TAG_HEAD);                                // dW += dz^T h
    gw.epi = EPI_ACCUM;
    RMCL_TRY(rmcl_launch_gemm(gw, dtype, RMCL_F32, 0, 0, exact, s));
    RMCL_LAUNCH(mpp_dbias_part_kernel<T>, dim3(cdiv(MPP_V, 256), cdiv(rows, MPP_DB_ROWS)), dim3(256), 0, s, (const T*)w.dz, count, rows, w.dbpart);
    RMCL_CHECK_LAUNCH();
    RMCL_LAUNCH(mpp_dbias_merge_kernel, dim3(cdiv(MPP_V, 256)), dim3(256), 0, s, w.dbpart, count, rows, G + h->db);
    RMCL_CHECK_LAUNCH();
  }
  RMCL_TRY(rmcl_launch_gemm(head_gemm(w.dz, W, w.t.dh, rows, D, MPP_V, MPP_V, D, D, GEMM_TAG_HEAD), dtype, RMCL_F32, 1, 0, exact, s));   // dh = dz W
  return pred_transform_backward(transform_of(h), params, w.t, idx, count, rows, G, dxn, s);
}
}  // namespace

extern "C" {

int64_t rmcl_mpp_ws_floats(const rmcl_mpp_head* h, int rows) {
  if (!head_ok(h) || rows < 1) return 0;
  MppWs w;
  return carve(*h, rows, nullptr, &w);
}

int rmcl_mpp_labels(const float* img, int B, int H, int W, const int32_t* sel, const int32_t* counts, int sel_ld, int gw, int P,
                    int32_t* labels, void* stream) {
  RMCL_REQUIRE(img && labels && (!sel || counts), "mpp_labels: NULL argument");
  RMCL_REQUIRE(B >= 1 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0 && P >= 1 && (long)B * P <= (1L << 24),
               "mpp_labels: images must be [B, 3, H, W] with H, W multiples of the 32-pixel patch");
  RMCL_REQUIRE(sel ? (gw == W / 32 && sel_ld >= 1) : P == (H / 32) * (W / 32), "mpp_labels: the dense form covers the whole grid (P = H/32 x W/32); gw = W/32");
  RMCL_LAUNCH(mpp_labels_kernel, dim3(cdiv((long)B * P, 4)), dim3(256), 0, (hipStream_t)stream, img, B, H, W, sel, counts, sel_ld, W / 32, P, labels);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_mpp_labels_u8(const uint8_t* img, const int32_t* sizes, int B, int Hmax, int Wmax, const float* lut, const int32_t* sel,
                       const int32_t* counts, int sel_ld, int gw, int P, int32_t* labels, void* stream) {
  RMCL_REQUIRE(img && sizes && lut && labels && (!sel || counts), "mpp_labels_u8: NULL argument");
  RMCL_REQUIRE(B >= 1 && Hmax >= 32 && Wmax >= 32 && Hmax % 32 == 0 && Wmax % 32 == 0 && P >= 1 && (long)B * P <= (1L << 24),
               "mpp_labels_u8: images must be [B, Hmax, Wmax, 3] with Hmax, Wmax multiples of the 32-pixel patch");
  RMCL_REQUIRE(sel ? (gw == Wmax / 32 && sel_ld >= 1) : P == (Hmax / 32) * (Wmax / 32),
               "mpp_labels_u8: the dense form covers the whole grid (P = Hmax/32 x Wmax/32); gw = Wmax/32");
  RMCL_REQUIRE(((uintptr_t)img & 3) == 0, "mpp_labels_u8: img must be 4-byte aligned (the pixels are read as dwords)");
  RMCL_LAUNCH(mpp_labels_u8_kernel, dim3(cdiv((long)B * P, 4)), dim3(256), 0, (hipStream_t)stream, img, sizes, B, Hmax, Wmax, lut, sel, counts, sel_ld,
              Wmax / 32, P, labels);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_mpp_compact(const int32_t* labels, const int32_t* masked, int B, int P, int L, int N, int all_rows, int cap, int32_t* idx, int32_t* lab,
                     int32_t* count, void* stream) {
  RMCL_REQUIRE(labels && masked && idx && lab && count, "mpp_compact: NULL argument");
  RMCL_REQUIRE(B >= 1 && P >= 1 && L >= 0 && N >= L + 1 + P && cap >= B * (all_rows ? P + 1 : P) && (long)B * (P + 1) <= (1L << 24),
               "mpp_compact: bad shape (N >= L + 1 + P, cap >= the rows that can be listed)");
  RMCL_LAUNCH(mpp_compact_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, labels, masked, B, P, L, N, all_rows, cap, idx, lab, count);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_mpp_forward(const rmcl_mpp_head* h, const float* params, const void* params_lp, int dtype, const float* xn, const int32_t* idx,
                     const int32_t* lab, const int32_t* count, int rows, float* ws, float* lse, float* rowloss, int32_t* argmax, float* stats,
                     void* stream) {
  RMCL_REQUIRE(head_ok(h) && pred_rows_ok(rows), "mpp_forward: unsupported head (D in {256, 768}) / rows not a multiple of 128");
  RMCL_REQUIRE(params && xn && idx && lab && count && ws && lse && rowloss && argmax && stats && (dtype == RMCL_F32 || params_lp),
               "mpp_forward: NULL argument");
  MppWs w;
  carve(*h, rows, ws, &w);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RMCL_BF16)
    return forward_t<bf16_t>(h, params, (const bf16_t*)params_lp + h->dw, dtype, xn, idx, lab, count, rows, w, lse, rowloss, argmax, stats, s);
  return forward_t<float>(h, params, params + h->dw, RMCL_F32, xn, idx, lab, count, rows, w, lse, rowloss, argmax, stats, s);
}

int rmcl_mpp_backward(const rmcl_mpp_head* h, const float* params, const void* params_lp, int dtype, const int32_t* idx, const int32_t* lab,
                      const int32_t* count, int rows, float* ws, const float* lse, float grad_scale, const float* grad_scale_dev, float* G,
                      float* dxn, void* stream) {
  RMCL_REQUIRE(head_ok(h) && pred_rows_ok(rows), "mpp_backward: unsupported head (D in {256, 768}) / rows not a multiple of 128");
  RMCL_REQUIRE(params && idx && lab && count && ws && lse && (dtype == RMCL_F32 || params_lp), "mpp_backward: NULL argument");
  MppWs w;
  carve(*h, rows, ws, &w);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RMCL_BF16)
    return backward_t<bf16_t>(h, params, (const bf16_t*)params_lp + h->dw, dtype, idx, lab, count, rows, w, lse, grad_scale, grad_scale_dev, G, dxn, s);
  return backward_t<float>(h, params, params + h->dw, RMCL_F32, idx, lab, count, rows, w, lse, grad_scale, grad_scale_dev, G, dxn, s);
}

int rmcl_mpp_logits(const rmcl_mpp_head* h, float* ws, int rows, int rows_out, float* logits, void* stream) {
  RMCL_REQUIRE(head_ok(h) && pred_rows_ok(rows) && rows_out >= 1 && rows_out <= rows, "mpp_logits: bad shape");
  RMCL_REQUIRE(ws && logits, "mpp_logits: NULL argument");
  MppWs w;
  carve(*h, rows, ws, &w);
  const long n4 = (long)rows_out * MPP_V / 4;
  RMCL_LAUNCH(mpp_logits_copy_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, w.z, logits, n4);
  RMCL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
