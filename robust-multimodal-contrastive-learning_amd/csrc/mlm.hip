// Masked language modelling head (compute_mlm, objectives.py:604-630; MLMHead, heads.py:183-195):
//   mlm_score = Linear(D,D) - GELU (exact erf) - LayerNorm(D, eps 1e-12) - Linear(D, V, no bias) + bias[V],  V = vocab_size (30522),
//   loss = cross_entropy(logits.view(-1, V), labels.view(-1), ignore_index = -100).
//
// The loss reads only the rows whose label is not -100 (~15 % of B x L), so the training path works on those rows, COMPACTED, and never
// holds a [rows, V] logits tensor:
//   compact    one workgroup: ascending list of the rows with a label, their labels, the count n (stays on the device)
//   gather + transform   the prediction-head transform shared with the MPP head (head_transform.hip: pred_transform_forward) on the text
//              rows of xn; h is kept in the decoder's operand type (bf16 / fp32) twice: [rows, D] and transposed [D, rows]
//   decoder + CE forward   z = W h^T + bias tile by tile on the matrix cores (32 vocabulary x 32 rows per wave), every lane keeps the
//              running (max, sum exp, first argmax, label logit) of ONE row; the vocabulary is split over workgroups, the partials per
//              (vocabulary chunk, row) are merged in chunk order
//   backward   dz = s (softmax(z) - onehot) / n is RECOMPUTED from h, W, bias and the saved lse, twice:
//              * workgroups that own 32 vocabulary rows stream the token rows:  dW[v,:] += sum_r dz[r,v] h[r,:],  dbias[v] += sum_r dz[r,v]
//              * workgroups that own 32 token rows and one vocabulary chunk:    dh_part[chunk][r,:] = sum_v dz[r,v] W[v,:]
//                (operand W^T [D, V]: a transposed shadow of the decoder weight), then dh = sum over chunks in chunk order
//              every output element has ONE owner and a fixed summation order: no float atomics anywhere, identical bits per call
//   transform backward and the scatter of dx into the zero-filled dxn of the encoder backward: pred_transform_backward.
// Operand type T: bf16 (v_mfma_f32_32x32x16_bf16) or fp32 (v_mfma_f32_32x32x2_f32, the parity engine); accumulation and all softmax
// statistics are fp32.  V need not be a multiple of the tile: columns >= V are masked to -inf / dz = 0.
#include <algorithm>
#include "rmcl_common.h"
#include "kernels.h"
#include "head_rows.h"
#include "../../include/rmcl.h"

namespace {

#define MLM_RG 128              // rows (dW kernel) / vocabulary columns (dh kernel) per iteration: one 32 x 32 z tile per wave

typedef __bf16 mbf16x8 __attribute__((ext_vector_type(8)));

// one k-step of a 32 x 32 matrix-core tile.  A fragment: lane holds A[m = lane & 31][k0 + KL * (lane >> 5) .. + KL), B likewise with n;
// C: acc[i] = C[m = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)][n = lane & 31]
template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
  static constexpr int KS = 16, PAD = 8;
  typedef mbf16x8 Frag;
  static __device__ __forceinline__ Frag load(const bf16_t* p, int lane) { return *reinterpret_cast<const Frag*>(p + 8 * (lane >> 5)); }
  static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Mma<float> {
  static constexpr int KS = 2, PAD = 4;
  typedef float Frag;
  static __device__ __forceinline__ Frag load(const float* p, int lane) { return p[lane >> 5]; }
  static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};

// z tile [32 x 32] = A rows x B rows over K = D (both K-contiguous); arow / brow: this lane's row (lane & 31) of either operand
template <typename T>
__device__ __forceinline__ f32x16 z_tile(const T* arow, const T* brow, int D, int lane) {
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 8
  for (int k = 0; k < D; k += Mma<T>::KS) acc = Mma<T>::mma(Mma<T>::load(arow + k, lane), Mma<T>::load(brow + k, lane), acc);
  return acc;
}

// 32 rows of `src` (row index clamped to last) -> LDS tile [32][D + PAD], 16-byte vectors
template <typename T>
__device__ __forceinline__ void stage_rows(T* dst, const T* __restrict__ src, int row0, int last, int D) {
  constexpr int VE = 16 / sizeof(T);
  const int ldp = D + Mma<T>::PAD, per_row = D / VE;
  for (int i = threadIdx.x; i < 32 * per_row; i += 256) {
    const int r = i / per_row, c = (i - r * per_row) * VE;
    const uint4 v = *reinterpret_cast<const uint4*>(src + (long)min(row0 + r, last) * D + c);
    *reinterpret_cast<uint4*>(dst + r * ldp + c) = v;
  }
}

// ---- compaction -----------------------------------------------------------------------------------------------------------------------
// labels [M = B L] int64.  idx[j] = b * N + l of the j-th row (ascending) whose label is in [0, V) (all = 1: every row), lab[j] its label
// (all = 1: -100 kept for the rows without one); idx / lab behind the count: -1 / -100.  count[0] = n.  One workgroup.
__global__ __launch_bounds__(256) void mlm_compact_kernel(const long* __restrict__ labels, int M, int L, int N, int V, int all,
                                                          int* __restrict__ idx, int* __restrict__ lab, int* __restrict__ count) {
  __shared__ int cnt[256];
  const int t = threadIdx.x, per = (M + 255) / 256, b0 = t * per, b1 = min(M, b0 + per);
  int c = 0;
  for (int i = b0; i < b1; ++i) {
    const long l = labels[i];
    c += (all || (l >= 0 && l < V)) ? 1 : 0;
  }
  cnt[t] = c;
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int i = 0; i < 256; ++i) { const int v = cnt[i]; cnt[i] = s; s += v; }
    count[0] = s;
  }
  __syncthreads();
  int o = cnt[t];
  for (int i = b0; i < b1; ++i) {
    const long l = labels[i];
    const bool ok = l >= 0 && l < V;
    if (all || ok) {
      idx[o] = (i / L) * N + (i % L);
      lab[o] = ok ? (int)l : -100;
      ++o;
    }
  }
  __syncthreads();
  const int n = count[0];
  for (int i = n + t; i < M; i += 256) { idx[i] = -1; lab[i] = -100; }
}

// WT [D, ldv] (T) = W^T of the fp32 master W [V, D]; columns V..ldv-1 zero.  32 x 32 tiles through LDS.
template <typename T>
__global__ __launch_bounds__(256) void mlm_transpose_kernel(const float* __restrict__ W, T* __restrict__ WT, int V, int D, int ldv) {
  __shared__ float tile[32][33];
  const int v0 = blockIdx.x * 32, d0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) tile[j][tx] = (v0 + j < V) ? W[(long)(v0 + j) * D + d0 + tx] : 0.f;
  __syncthreads();
  for (int j = ty; j < 32; j += 8) WT[(long)(d0 + j) * ldv + v0 + tx] = from_f32<T>(tile[tx][j]);
}

// ---- decoder + cross-entropy forward -----------------------------------------------------------------------------------------------
struct RowState {
  float m, s, best, zl;
  int bi;
};
__device__ __forceinline__ void rs_init(RowState& a) { a.m = -INFINITY; a.s = 0.f; a.best = -INFINITY; a.zl = -INFINITY; a.bi = 0x7fffffff; }
// a <- a merged with b (b's columns may lie before or behind a's: the first maximum is the smaller column on a tie)
__device__ __forceinline__ void rs_merge(RowState& a, const RowState& b) {
  const float M = fmaxf(a.m, b.m);
  const float sa = a.m > -INFINITY ? a.s * expf(a.m - M) : 0.f, sb = b.m > -INFINITY ? b.s * expf(b.m - M) : 0.f;
  a.m = M;
  a.s = sa + sb;
  if (b.best > a.best || (b.best == a.best && b.bi < a.bi)) { a.best = b.best; a.bi = b.bi; }
  a.zl = fmaxf(a.zl, b.zl);
}

// grid (row tiles of 32, vocabulary chunks).  part[chunk][rows] = (max, sum exp(z - max), best logit, label logit), parti = argmax
template <typename T, int NT>
__global__ __launch_bounds__(256) void mlm_dec_fwd_kernel(const T* __restrict__ h, const T* __restrict__ W, const float* __restrict__ bias,
                                                          const int* __restrict__ lab, const int* __restrict__ count, int V, int rows,
                                                          float4* __restrict__ part, int* __restrict__ parti) {
  constexpr int D = 128 * NT;                            // (compile-time: the k-loop of a z tile unrolls)
  extern __shared__ __align__(16) unsigned char smem[];
  T* hs = reinterpret_cast<T*>(smem);
  __shared__ RowState red[4][32];
  const int n = min(count[0], rows), r0 = blockIdx.x * 32;
  if (r0 >= n) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 31, g = lane >> 5, ldp = D + Mma<T>::PAD;
  stage_rows<T>(hs, h, r0, rows - 1, D);
  __syncthreads();
  const int tiles = (V + 31) / 32, tpc = (tiles + gridDim.y - 1) / gridDim.y;
  const int t0 = blockIdx.y * tpc, t1 = min(tiles, t0 + tpc);
  const int r = r0 + ln, label = r < n ? lab[r] : -1;
  RowState st;
  rs_init(st);
  for (int t = t0 + wave; t < t1; t += 4) {
    const int v0 = t * 32;
    const f32x16 acc = z_tile<T>(W + (long)min(v0 + ln, V - 1) * D, hs + ln * ldp, D, lane);
    float z[16], tm = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = v0 + (i & 3) + 8 * (i >> 2) + 4 * g;
      z[i] = v < V ? acc[i] + bias[min(v, V - 1)] : -INFINITY;
      tm = fmaxf(tm, z[i]);
      if (z[i] > st.best) { st.best = z[i]; st.bi = v; }          // columns grow with i and with t: the first maximum of this lane
      if (v == label) st.zl = z[i];
    }
    if (tm > st.m) { st.s *= expf(st.m - tm); st.m = tm; }
    if (st.m > -INFINITY) {
      float e = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) e += expf(z[i] - st.m);
      st.s += e;
    }
  }
  {  // the two lanes of a row (lane, lane ^ 32)
    RowState o;
    o.m = __shfl_xor(st.m, 32, 64); o.s = __shfl_xor(st.s, 32, 64); o.best = __shfl_xor(st.best, 32, 64);
    o.zl = __shfl_xor(st.zl, 32, 64); o.bi = __shfl_xor(st.bi, 32, 64);
    rs_merge(st, o);
  }
  if (g == 0) red[wave][ln] = st;
  __syncthreads();
  if (threadIdx.x < 32) {
    RowState a = red[0][ln];
    for (int w = 1; w < 4; ++w) rs_merge(a, red[w][ln]);
    const long o = (long)blockIdx.y * rows + r0 + ln;
    part[o] = make_float4(a.m, a.s, a.best, a.zl);
    parti[o] = a.bi;
  }
}

// per row: merge the chunks in order -> lse, row loss lse - z[label], argmax.  Rows >= n: (0, 0, -1).
__global__ __launch_bounds__(256) void mlm_dec_finish_kernel(const float4* __restrict__ part, const int* __restrict__ parti, int nchunk, int rows,
                                                             const int* __restrict__ count, int V, float* __restrict__ lse,
                                                             float* __restrict__ rowloss, int* __restrict__ argmax) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  if (r >= min(count[0], rows)) { lse[r] = 0.f; rowloss[r] = 0.f; argmax[r] = -1; return; }
  RowState a;
  rs_init(a);
  for (int c = 0; c < nchunk; ++c) {
    const float4 p = part[(long)c * rows + r];
    RowState b;
    b.m = p.x; b.s = p.y; b.best = p.z; b.zl = p.w; b.bi = parti[(long)c * rows + r];
    rs_merge(a, b);
  }
  const float l = a.m + logf(a.s);
  lse[r] = l;
  rowloss[r] = l - a.zl;
  argmax[r] = (a.bi >= 0 && a.bi < V) ? a.bi : 0;                   // (an all-NaN row: column 0)
}

// stats = (sum_r rowloss / n, rows with argmax == label, n): one workgroup, fixed order (strided partials, then a tree in LDS).
// n = 0: 0 / 0 = NaN, like F.cross_entropy over an all-ignored batch.
__global__ __launch_bounds__(256) void mlm_stats_kernel(const float* __restrict__ rowloss, const int* __restrict__ argmax,
                                                        const int* __restrict__ lab, const int* __restrict__ count, int rows,
                                                        float* __restrict__ stats) {
  __shared__ float red[2][256];
  const int n = min(count[0], rows);
  float l = 0.f, c = 0.f;
  for (int r = threadIdx.x; r < n; r += 256) { l += rowloss[r]; c += argmax[r] == lab[r] ? 1.f : 0.f; }
  block_tree_sum2(red, l, c);
  if (threadIdx.x == 0) { stats[0] = red[0][0] / (float)n; stats[1] = red[1][0]; stats[2] = (float)n; }
}

// dz of this lane's 16 elements of a z tile C[v, r]: s (exp(z - lse_r) - [v == label_r]) for r < n, v < V, else exactly 0
__device__ __forceinline__ void dz_tile(const f32x16& acc, const float* __restrict__ bias, int v0, int g, int V, bool row_ok, float lse_r,
                                        int label, float scale, float* dz) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int v = v0 + (i & 3) + 8 * (i >> 2) + 4 * g;
    const float z = acc[i] + bias[min(v, V - 1)];
    const float p = expf(z - lse_r) - (v == label ? 1.f : 0.f);
    dz[i] = (row_ok && v < V) ? scale * p : 0.f;
  }
}

// ---- backward 1: workgroups own 32 vocabulary rows -> dW [V, D] +=, dbias [V] += ----------------------------------------------------------
// NT = D / 128: every wave owns D / 4 columns of dW = NT tiles of 32.
template <typename T, int NT>
__global__ __launch_bounds__(256) void mlm_dec_bwd_w_kernel(const T* __restrict__ h, const T* __restrict__ hT, const T* __restrict__ W,
                                                            const float* __restrict__ bias, const int* __restrict__ lab,
                                                            const float* __restrict__ lse, const int* __restrict__ count, float gscale,
                                                            const float* __restrict__ gscale_dev, int V, int rows, float* __restrict__ dW,
                                                            float* __restrict__ dbias) {
  constexpr int D = 128 * NT, LDP = D + Mma<T>::PAD, LDZ = MLM_RG + Mma<T>::PAD;
  extern __shared__ __align__(16) unsigned char smem[];
  T* ws = reinterpret_cast<T*>(smem);                    // [32][LDP]: this workgroup's rows of W
  T* dzs = ws + 32 * LDP;                                // [32 v][LDZ]: dz^T of the current 128 token rows
  const int n = min(count[0], rows);
  if (n == 0) return;                                    // (uniform) an all-ignored batch writes nothing
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 31, g = lane >> 5, v0 = blockIdx.x * 32;
  const float scale = (gscale_dev ? gscale * gscale_dev[0] : gscale) / (float)n;
  stage_rows<T>(ws, W, v0, V - 1, D);
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  float bs = 0.f;
  __syncthreads();
  for (int rb = 0; rb < n; rb += MLM_RG) {
    const int r = rb + 32 * wave + ln;
    float dz[16];
    if (rb + 32 * wave < n) {                            // (wave-uniform)
      const f32x16 z = z_tile<T>(ws + ln * LDP, h + (long)min(r, rows - 1) * D, D, lane);
      dz_tile(z, bias, v0, g, V, r < n, r < n ? lse[r] : 0.f, r < n ? lab[r] : -1, scale, dz);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) dz[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dzs[((i & 3) + 8 * (i >> 2) + 4 * g) * LDZ + 32 * wave + ln] = from_f32<T>(dz[i]);
    __syncthreads();
    if (threadIdx.x < 32)
      for (int c = 0; c < MLM_RG; ++c) bs += to_f32<T>(dzs[threadIdx.x * LDZ + c]);
#pragma unroll 2
    for (int ks = 0; ks < MLM_RG; ks += Mma<T>::KS) {
      const typename Mma<T>::Frag a = Mma<T>::load(dzs + ln * LDZ + ks, lane);
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = Mma<T>::mma(a, Mma<T>::load(hT + (long)(wave * (D / 4) + 32 * j + ln) * rows + rb + ks, lane), acc[j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = v0 + (i & 3) + 8 * (i >> 2) + 4 * g;
      if (v < V) dW[(long)v * D + wave * (D / 4) + 32 * j + ln] += acc[j][i];
    }
  if (threadIdx.x < 32 && v0 + (int)threadIdx.x < V) dbias[v0 + threadIdx.x] += bs;
}

// ---- backward 2: workgroups own 32 token rows and one vocabulary chunk -> dhp[chunk][rows][D] ------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(256) void mlm_dec_bwd_h_kernel(const T* __restrict__ h, const T* __restrict__ W, const T* __restrict__ WT,
                                                            const float* __restrict__ bias, const int* __restrict__ lab,
                                                            const float* __restrict__ lse, const int* __restrict__ count, float gscale,
                                                            const float* __restrict__ gscale_dev, int V, int ldv, int rows,
                                                            float* __restrict__ dhp) {
  constexpr int D = 128 * NT, LDP = D + Mma<T>::PAD, LDZ = MLM_RG + Mma<T>::PAD;
  extern __shared__ __align__(16) unsigned char smem[];
  T* hs = reinterpret_cast<T*>(smem);                    // [32][LDP]: this workgroup's rows of h
  T* dzs = hs + 32 * LDP;                                // [32 r][LDZ]: dz of the current 128 vocabulary columns
  const int n = min(count[0], rows), r0 = blockIdx.x * 32;
  if (r0 >= n) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 31, g = lane >> 5;
  const float scale = (gscale_dev ? gscale * gscale_dev[0] : gscale) / (float)n;
  stage_rows<T>(hs, h, r0, rows - 1, D);
  const int r = r0 + ln;
  const bool row_ok = r < n;
  const float lse_r = row_ok ? lse[r] : 0.f;
  const int label = row_ok ? lab[r] : -1;
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
  const int groups = ldv / MLM_RG, gpc = (groups + gridDim.y - 1) / gridDim.y;
  const int g0 = blockIdx.y * gpc, g1 = min(groups, g0 + gpc);
  __syncthreads();
  for (int gi = g0; gi < g1; ++gi) {
    const int v0 = gi * MLM_RG + 32 * wave;
    float dz[16];
    if (v0 < V) {                                        // (wave-uniform)
      const f32x16 z = z_tile<T>(W + (long)min(v0 + ln, V - 1) * D, hs + ln * LDP, D, lane);
      dz_tile(z, bias, v0, g, V, row_ok, lse_r, label, scale, dz);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) dz[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) dzs[ln * LDZ + 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * g] = from_f32<T>(dz[i]);
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < MLM_RG; ks += Mma<T>::KS) {
      const typename Mma<T>::Frag a = Mma<T>::load(dzs + ln * LDZ + ks, lane);
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = Mma<T>::mma(a, Mma<T>::load(WT + (long)(wave * (D / 4) + 32 * j + ln) * ldv + gi * MLM_RG + ks, lane), acc[j]);
    }
    __syncthreads();
  }
  float* out = dhp + ((long)blockIdx.y * rows + r0) * D;
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) out[(long)((i & 3) + 8 * (i >> 2) + 4 * g) * D + wave * (D / 4) + 32 * j + ln] = acc[j][i];
}

// dh [rows, D] = sum over chunks (in order) of dhp for the row tiles the dh kernel ran (tile start < n), else 0
__global__ __launch_bounds__(256) void mlm_dh_reduce_kernel(const float* __restrict__ dhp, int nchunk, int rows, int D,
                                                            const int* __restrict__ count, float* __restrict__ dh) {
  const int n = min(count[0], rows), per_row = D / 4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)rows * per_row; i += (long)gridDim.x * 256) {
    const int r = (int)(i / per_row);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((r & ~31) < n)
      for (int c = 0; c < nchunk; ++c) {
        const float4 p = *reinterpret_cast<const float4*>(dhp + (long)c * rows * D + i * 4);
        s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
      }
    *reinterpret_cast<float4*>(dh + i * 4) = s;
  }
}

// ---- dense logits [rows, ldl] (evaluation / on request): grid (row tiles, vocabulary chunks) --------------------------------------------------
template <typename T, int NT>
__global__ __launch_bounds__(256) void mlm_logits_kernel(const T* __restrict__ h, const T* __restrict__ W, const float* __restrict__ bias,
                                                         int V, int rows, int rows_out, float* __restrict__ logits, long ldl) {
  constexpr int D = 128 * NT;
  extern __shared__ __align__(16) unsigned char smem[];
  T* hs = reinterpret_cast<T*>(smem);
  const int r0 = blockIdx.x * 32;
  if (r0 >= rows_out) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ln = lane & 31, g = lane >> 5, ldp = D + Mma<T>::PAD;
  stage_rows<T>(hs, h, r0, rows - 1, D);
  __syncthreads();
  const int tiles = (V + 31) / 32, tpc = (tiles + gridDim.y - 1) / gridDim.y;
  const int t0 = blockIdx.y * tpc, t1 = min(tiles, t0 + tpc);
  for (int t = t0 + wave; t < t1; t += 4) {
    const int v0 = t * 32;
    // A = h rows, B = W rows: C[r, v], so a lane's column is a vocabulary index and the 32 lanes of a half wave store 128 contiguous bytes
    const f32x16 acc = z_tile<T>(hs + ln * ldp, W + (long)min(v0 + ln, V - 1) * D, D, lane);
    const int v = v0 + ln;
    if (v < V) {
      const float b = bias[v];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = r0 + (i & 3) + 8 * (i >> 2) + 4 * g;
        if (r < rows_out) logits[(long)r * ldl + v] = acc[i] + b;
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
struct MlmWs {
  PredWs t;                                                 // the transform's slices (head_rows.h); t.hT: the dW kernel's operand
  float* dhp;
  float4* part;
  int* parti;
};
PredTransform transform_of(const rmcl_mlm_head* h) { return PredTransform{h->D, h->tw, h->tb, h->lg, h->lb}; }
// vocabulary chunks of the dh kernel: enough workgroups to fill 256 CUs twice at the usual ~384 rows (12 row tiles x 32), fewer when the
// row tiles alone do that (the slab costs chunks x rows x D x 4 bytes written and read once)
int h_chunks(int rows) { return rows <= 512 ? 32 : (rows <= 1024 ? 16 : 8); }
int fwd_chunks(int rows) {                                // vocabulary chunks of the forward / logits kernels: ~2 workgroups per CU
  const int rt = rows / 32;
  return std::max(1, std::min(64, 512 / std::max(rt, 1)));
}
long carve(const rmcl_mlm_head& hd, int rows, float* base, MlmWs* w) {
  StashCarver c{base};
  pred_carve_fwd(c, rows, hd.D, &w->t);
  w->t.hT = c.take((long)rows * hd.D);
  w->part = reinterpret_cast<float4*>(c.take(4L * 64 * rows));   // (64: capacity of the partial table; the launch uses fwd_chunks(rows) <= 64)
  w->parti = reinterpret_cast<int*>(c.take(64L * rows));
  pred_carve_bwd(c, rows, hd.D, &w->t);
  // (monotone in rows and >= h_chunks(rows) x rows in each of its three regimes: buffers sized for a larger extent fit a smaller one)
  w->dhp = c.take(std::max({32L * std::min(rows, 512), 16L * std::min(rows, 1024), 8L * rows}) * hd.D);
  return c.used;
}
bool head_ok(const rmcl_mlm_head* h) { return h && pred_head_ok(h->D) && h->V >= 1; }

template <typename T>
int lds_bytes(int D, bool with_dz) { return (32 * (D + Mma<T>::PAD) + (with_dz ? 32 * (MLM_RG + Mma<T>::PAD) : 0)) * (int)sizeof(T); }

template <typename T, int NT>
int forward_t(const rmcl_mlm_head* h, const float* params, const T* W, const float* xn, const int* idx, const int* lab, const int* count, int rows,
              const MlmWs& w, float* lse, float* rowloss, int* argmax, float* stats, hipStream_t s) {
  RMCL_TRY(pred_transform_forward(transform_of(h), params, xn, idx, count, rows, sizeof(T) == 2 ? RMCL_BF16 : RMCL_F32, w.t, s));
  const int nch = fwd_chunks(rows), lds = lds_bytes<T>(h->D, false);
  static RmclLdsOnce once;
  RMCL_TRY(rmcl_set_max_lds(once, (const void*)mlm_dec_fwd_kernel<T, NT>, lds));
  RMCL_LAUNCH((mlm_dec_fwd_kernel<T, NT>), dim3(rows / 32, nch), dim3(256), lds, s, (const T*)w.t.h, W, params + h->db, lab, count, h->V, rows, w.part,
              w.parti);
  RMCL_CHECK_LAUNCH();
  RMCL_LAUNCH(mlm_dec_finish_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, s, w.part, w.parti, nch, rows, count, h->V, lse, rowloss, argmax);
  RMCL_CHECK_LAUNCH();
  RMCL_LAUNCH(mlm_stats_kernel, dim3(1), dim3(256), 0, s, rowloss, argmax, lab, count, rows, stats);
  RMCL_CHECK_LAUNCH();
  return 0;
}

template <typename T, int NT>
int backward_t(const rmcl_mlm_head* h, const float* params, const T* W, const T* WT, const int* idx, const int* lab, const int* count, int rows,
               const MlmWs& w, const float* lse, float gscale, const float* gscale_dev, float* G, float* dxn, hipStream_t s) {
  const int D = h->D, V = h->V, ldv = cdiv(V, MLM_RG) * MLM_RG, lds = lds_bytes<T>(D, true);
  static RmclLdsOnce once_w, once_h;
  if (G) {
    RMCL_TRY(rmcl_set_max_lds(once_w, (const void*)mlm_dec_bwd_w_kernel<T, NT>, lds));
    RMCL_LAUNCH((mlm_dec_bwd_w_kernel<T, NT>), dim3(cdiv(V, 32)), dim3(256), lds, s, (const T*)w.t.h, (const T*)w.t.hT, W, params + h->db, lab, lse, count,
                gscale, gscale_dev, V, rows, G + h->dw, G + h->db);
    RMCL_CHECK_LAUNCH();
  }
  RMCL_TRY(rmcl_set_max_lds(once_h, (const void*)mlm_dec_bwd_h_kernel<T, NT>, lds));
  RMCL_LAUNCH((mlm_dec_bwd_h_kernel<T, NT>), dim3(rows / 32, h_chunks(rows)), dim3(256), lds, s, (const T*)w.t.h, W, WT, params + h->db, lab, lse, count,
              gscale, gscale_dev, V, ldv, rows, w.dhp);
  RMCL_CHECK_LAUNCH();
  RMCL_LAUNCH(mlm_dh_reduce_kernel, dim3(std::min(1024, cdiv((long)rows * D / 4, 256))), dim3(256), 0, s, w.dhp, h_chunks(rows), rows, D, count, w.t.dh);
  RMCL_CHECK_LAUNCH();
  return pred_transform_backward(transform_of(h), params, w.t, idx, count, rows, G, dxn, s);
}

template <typename T, int NT>
int logits_t(const rmcl_mlm_head* h, const float* params, const T* W, const MlmWs& w, int rows, int rows_out, float* logits, long ldl, hipStream_t s) {
  const int lds = lds_bytes<T>(h->D, false);
  static RmclLdsOnce once;
  RMCL_TRY(rmcl_set_max_lds(once, (const void*)mlm_logits_kernel<T, NT>, lds));
  RMCL_LAUNCH((mlm_logits_kernel<T, NT>), dim3(cdiv(rows_out, 32), fwd_chunks(rows)), dim3(256), lds, s, (const T*)w.t.h, W, params + h->db, h->V, rows,
              rows_out, logits, ldl);
  RMCL_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" {

int64_t rmcl_mlm_ws_floats(const rmcl_mlm_head* h, int rows) {
  MlmWs w;
  return carve(*h, rows, nullptr, &w);
}

int rmcl_mlm_compact(const int64_t* labels, int M, int L, int N, int V, int all_rows, int32_t* idx, int32_t* lab, int32_t* count, void* stream) {
  RMCL_REQUIRE(labels && idx && lab && count && M >= 1 && L >= 1 && N >= L && M % L == 0 && V >= 1, "mlm_compact: NULL argument / bad shape");
  RMCL_LAUNCH(mlm_compact_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const long*)labels, M, L, N, V, all_rows, idx, lab, count);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_mlm_weight_transpose(const rmcl_mlm_head* h, const float* params, void* WT, int dtype, void* stream) {
  RMCL_REQUIRE(head_ok(h) && params && WT, "mlm_weight_transpose: bad argument (D in {256, 768})");
  const int ldv = cdiv(h->V, MLM_RG) * MLM_RG;
  const dim3 grid(ldv / 32, h->D / 32);
  if (dtype == RMCL_BF16)
    RMCL_LAUNCH(mlm_transpose_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, params + h->dw, (bf16_t*)WT, h->V, h->D, ldv);
  else
    RMCL_LAUNCH(mlm_transpose_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, params + h->dw, (float*)WT, h->V, h->D, ldv);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_mlm_forward(const rmcl_mlm_head* h, const float* params, const void* params_lp, int dtype, const float* xn, const int32_t* idx,
                     const int32_t* lab, const int32_t* count, int rows, float* ws, float* lse, float* rowloss, int32_t* argmax, float* stats,
                     void* stream) {
  RMCL_REQUIRE(head_ok(h) && pred_rows_ok(rows), "mlm_forward: unsupported head (D in {256, 768}) / rows not a multiple of 128");
  RMCL_REQUIRE(params && xn && idx && lab && count && ws && lse && rowloss && argmax && stats && (dtype == RMCL_F32 || params_lp),
               "mlm_forward: NULL argument");
  MlmWs w;
  carve(*h, rows, ws, &w);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RMCL_BF16) {
    const bf16_t* W = (const bf16_t*)params_lp + h->dw;
    if (h->D == 768) return forward_t<bf16_t, 6>(h, params, W, xn, idx, lab, count, rows, w, lse, rowloss, argmax, stats, s);
    return forward_t<bf16_t, 2>(h, params, W, xn, idx, lab, count, rows, w, lse, rowloss, argmax, stats, s);
  }
  if (h->D == 768) return forward_t<float, 6>(h, params, params + h->dw, xn, idx, lab, count, rows, w, lse, rowloss, argmax, stats, s);
  return forward_t<float, 2>(h, params, params + h->dw, xn, idx, lab, count, rows, w, lse, rowloss, argmax, stats, s);
}

int rmcl_mlm_backward(const rmcl_mlm_head* h, const float* params, const void* params_lp, const void* WT, int dtype, const int32_t* idx,
                      const int32_t* lab, const int32_t* count, int rows, float* ws, const float* lse, float grad_scale,
                      const float* grad_scale_dev, float* G, float* dxn, void* stream) {
  RMCL_REQUIRE(head_ok(h) && pred_rows_ok(rows), "mlm_backward: unsupported head (D in {256, 768}) / rows not a multiple of 128");
  RMCL_REQUIRE(params && WT && idx && lab && count && ws && lse && (dtype == RMCL_F32 || params_lp), "mlm_backward: NULL argument");
  MlmWs w;
  carve(*h, rows, ws, &w);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RMCL_BF16) {
    const bf16_t* W = (const bf16_t*)params_lp + h->dw;
    if (h->D == 768) return backward_t<bf16_t, 6>(h, params, W, (const bf16_t*)WT, idx, lab, count, rows, w, lse, grad_scale, grad_scale_dev, G, dxn, s);
    return backward_t<bf16_t, 2>(h, params, W, (const bf16_t*)WT, idx, lab, count, rows, w, lse, grad_scale, grad_scale_dev, G, dxn, s);
  }
  const float* W = params + h->dw;
  if (h->D == 768) return backward_t<float, 6>(h, params, W, (const float*)WT, idx, lab, count, rows, w, lse, grad_scale, grad_scale_dev, G, dxn, s);
  return backward_t<float, 2>(h, params, W, (const float*)WT, idx, lab, count, rows, w, lse, grad_scale, grad_scale_dev, G, dxn, s);
}

int rmcl_mlm_logits(const rmcl_mlm_head* h, const float* params, const void* params_lp, int dtype, float* ws, int rows, int rows_out, float* logits,
                    int64_t ldl, void* stream) {
  RMCL_REQUIRE(head_ok(h) && pred_rows_ok(rows) && rows_out >= 1 && rows_out <= rows && ldl >= h->V, "mlm_logits: bad shape");
  RMCL_REQUIRE(params && ws && logits && (dtype == RMCL_F32 || params_lp), "mlm_logits: NULL argument");
  MlmWs w;
  carve(*h, rows, ws, &w);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RMCL_BF16) {
    const bf16_t* W = (const bf16_t*)params_lp + h->dw;
    if (h->D == 768) return logits_t<bf16_t, 6>(h, params, W, w, rows, rows_out, logits, ldl, s);
    return logits_t<bf16_t, 2>(h, params, W, w, rows, rows_out, logits, ldl, s);
  }
  if (h->D == 768) return logits_t<float, 6>(h, params, params + h->dw, w, rows, rows_out, logits, ldl, s);
  return logits_t<float, 2>(h, params, params + h->dw, w, rows, rows_out, logits, ldl, s);
}

}  // extern "C"
