// Row top-k (include/rmcl.h rmcl_rows_topk): the k largest entries of every row of a row-major fp32 matrix x [R, C] with pitch ld >= C, in
// descending order, ties to the smaller column (the rule of wave_argmax_first), -inf an ordinary value that sorts last, NaN never selected;
// optionally the softmax / sigmoid probability of each selected entry and the row's log-sum-exp.
//
//   ownership      One 256-thread workgroup per row.  The row is cut at its first 16-byte boundary: a head of h <= 3 columns, G whole float4
//                  groups, a tail of <= 3 columns.  Thread t owns head column t (t < h), the groups g = t, t + 256, ..., and tail column j when
//                  t == 8 + j: every column has one owner, every load lies inside [row, row + C), and the groups are 16-byte loads whatever
//                  ld and the row start are.
//   pass 1         Every thread scans its columns once: its first maximum (value, column), and (SOFTMAX) the online log-sum-exp of its
//                  columns - a running maximum m and s = sum exp(x - m), fp32, columns in ascending order; NaN and -inf columns add nothing.
//                  The 256 (m, s) pairs meet in a butterfly over the wave and then wave by wave: a fixed order.
//   k rounds       Round j: the first maximum of the 256 thread candidates (butterfly, then the four waves in wave order) is output j.  Only the
//                  thread that owned it looks for its next candidate: the first maximum of its columns among the pairs that come
//                  lexicographically AFTER the winner (a smaller value, or an equal value in a larger column).  Every other thread's
//                  candidate is still its best unselected column, so a round re-reads C / 256 columns, not C.  A thread without a
//                  selectable column left holds the column TOPK_NONE, which loses to every real column - a -inf one included; when that wins,
//                  the row is exhausted and the remaining slots get idx -1, val -inf, prob 0.
//   no per-thread lists: the state of a thread is one (value, column) pair - no dynamic register indexing, no scratch, no workspace, no
//   atomics; thread 0 writes every output of its row.  Two calls on the same input give the same bytes.
#include <limits.h>
#include <math.h>
#include "rmcl_common.h"
#include "kernels.h"
#include "../../include/rmcl.h"

namespace {

constexpr int TOPK_NONE = INT_MAX;

// (x, c) replaces the candidate (v, i) when it is selectable - after the previous winner (pv, pi) when AFTER - and comes first
template <bool AFTER>
__device__ __forceinline__ void consider(float x, int c, float pv, int pi, float& v, int& i) {
  const bool ok = AFTER ? (x < pv || (x == pv && c > pi)) : true;
  if (ok && (x > v || (x == v && c < i))) { v = x; i = c; }     // (a NaN x fails every comparison)
}

// online log-sum-exp: (m, s) <- (m, s) + exp(x)
__device__ __forceinline__ void lse_add(float x, float& m, float& s) {
  if (!(x > -INFINITY)) return;                                  // NaN, -inf: nothing
  if (x > m) {
    s = s * expf(m - x) + 1.0f;                                  // (m = -inf: s = 0 stays 0, exp(-inf) = 0)
    m = x;
  } else {
    s += expf(x - m);
  }
}
__device__ __forceinline__ void lse_merge(float m2, float s2, float& m, float& s) {
  const float M = fmaxf(m, m2);
  if (M > -INFINITY) s = s * expf(m - M) + s2 * expf(m2 - M);    // (M = -inf: both sums are 0)
  m = M;
}

// One scan of this thread's columns.  AFTER = false: the first maximum of all of them (and the log-sum-exp when LSE); AFTER = true: the first
// maximum behind (pv, pi).
template <bool AFTER, bool LSE>
__device__ __forceinline__ void scan_own(const float* __restrict__ row, int C, int h, int G, int t, float pv, int pi, float& v, int& i,
                                         float& m, float& s) {
  v = -INFINITY;
  i = TOPK_NONE;
  if (t < h) {
    const float x = row[t];
    consider<AFTER>(x, t, pv, pi, v, i);
    if (LSE) lse_add(x, m, s);
  }
  const float4* body = reinterpret_cast<const float4*>(row + h);
  for (int g = t; g < G; g += 256) {
    const float4 q = body[g];
    const int c = h + 4 * g;
    consider<AFTER>(q.x, c, pv, pi, v, i);
    consider<AFTER>(q.y, c + 1, pv, pi, v, i);
    consider<AFTER>(q.z, c + 2, pv, pi, v, i);
    consider<AFTER>(q.w, c + 3, pv, pi, v, i);
    if (LSE) {
      lse_add(q.x, m, s);
      lse_add(q.y, m, s);
      lse_add(q.z, m, s);
      lse_add(q.w, m, s);
    }
  }
  const int c = h + 4 * G + (t - 8);
  if (t >= 8 && c < C) {                                         // (at most three tail columns: t = 8, 9, 10)
    const float x = row[c];
    consider<AFTER>(x, c, pv, pi, v, i);
    if (LSE) lse_add(x, m, s);
  }
}

template <bool LSE>
__global__ __launch_bounds__(256) void rows_topk_kernel(const float* __restrict__ x, long ld, int C, int k, int mode, int* __restrict__ idx,
                                                        float* __restrict__ val, float* __restrict__ prob, float* __restrict__ lse_out) {
  __shared__ float sh_v[4], sh_m[4], sh_s[4];
  __shared__ int sh_i[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long r = blockIdx.x;
  const float* row = x + r * ld;
  int h = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2);        // columns in front of the first 16-byte boundary
  if (h > C) h = C;
  const int G = (C - h) >> 2;

  float v, m = -INFINITY, s = 0.f, lse = 0.f;
  int i;
  scan_own<false, LSE>(row, C, h, G, t, 0.f, 0, v, i, m, s);
  if (LSE) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(__shfl_xor(m, o, 64), __shfl_xor(s, o, 64), m, s);
    if (lane == 0) { sh_m[w] = m; sh_s[w] = s; }
    __syncthreads();
    m = sh_m[0];
    s = sh_s[0];
    for (int j = 1; j < 4; ++j) lse_merge(sh_m[j], sh_s[j], m, s);
    lse = s > 0.f ? m + logf(s) : -INFINITY;                      // (no finite column: -inf)
    if (t == 0 && lse_out) lse_out[r] = lse;
  }

  int* oi = idx + r * k;
  float* ov = val + r * k;
  float* op = prob ? prob + r * k : nullptr;
  for (int j = 0; j < k; ++j) {
    float wv = v;
    int wi = i;
    wave_argmax_first(wv, wi);
    if (lane == 0) { sh_v[w] = wv; sh_i[w] = wi; }
    __syncthreads();
    wv = sh_v[0];
    wi = sh_i[0];
    for (int q = 1; q < 4; ++q) {
      const float v2 = sh_v[q];
      const int i2 = sh_i[q];
      if (v2 > wv || (v2 == wv && i2 < wi)) { wv = v2; wi = i2; }
    }
    __syncthreads();                                             // (sh_v / sh_i are rewritten next round)
    if (wi == TOPK_NONE) {                                       // the row is exhausted: uniform over the workgroup
      if (t == 0)
        for (int q = j; q < k; ++q) {
          oi[q] = -1;
          ov[q] = -INFINITY;
          if (op) op[q] = 0.f;
        }
      break;
    }
    if (t == 0) {
      oi[j] = wi;
      ov[j] = wv;
      if (op) {
        if (mode == RMCL_TOPK_SOFTMAX) op[j] = wv > -INFINITY ? expf(wv - lse) : 0.f;      // (a selected -inf column: 0, not exp(-inf + inf))
        else if (mode == RMCL_TOPK_SIGMOID) op[j] = 1.0f / (1.0f + expf(-wv));
      }
    }
    if (i == wi && j + 1 < k) scan_own<true, false>(row, C, h, G, t, wv, wi, v, i, m, s);     // the owner alone moves on
  }
}

}  // namespace

int rmcl_rows_topk_launch(const float* x, long ld, int R, int C, int k, int mode, int* idx, float* val, float* prob, float* lse, hipStream_t s) {
  if (mode == RMCL_TOPK_SOFTMAX)
    RMCL_LAUNCH(rows_topk_kernel<true>, dim3(R), dim3(256), 0, s, x, ld, C, k, mode, idx, val, prob, lse);
  else
    RMCL_LAUNCH(rows_topk_kernel<false>, dim3(R), dim3(256), 0, s, x, ld, C, k, mode, idx, val, prob, (float*)nullptr);
  RMCL_CHECK_LAUNCH();
  return 0;
}
