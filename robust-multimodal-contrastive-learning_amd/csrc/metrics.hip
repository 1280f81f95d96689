// Epoch metrics (vilt/gadgets/my_metrics.py: Accuracy, VQAScore, Scalar, change_rate): the (sum, count) pairs of a run's metrics live in one
// device table, double [n_slots][2], and a step adds to them with ONE launch - no synchronisation, no copy to the host, no launch per metric.
//
//   rmcl_metrics_update   up to 8 ops by value in the kernel arguments, one workgroup of 256 threads per op (include/rmcl.h lists the kinds).
//                         A row op keeps, per group (<= 4), a double sum and two int counts in registers: a thread's strided partial, a
//                         butterfly over the wave, the four waves through LDS in wave order, then thread 0 does a plain read-modify-write of
//                         the op's slots.  The workgroups of a call own disjoint slots (checked on the host) and stream order serialises
//                         calls, so nothing needs an atomic and the same inputs leave the same bytes.  SCALAR and PAIR are one thread's
//                         work; a SCALAR may carry a gate (a device float): it adds nothing when the gate holds 0.
#include <climits>
#include "rmcl_common.h"
#include "../../include/rmcl.h"

namespace {

#define MG RMCL_METRIC_MAX_GROUPS

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// group of row r: group[r] when it lies in [0, ng), else -1 (the row is left out)
__device__ __forceinline__ int row_group(const int* __restrict__ group, int r, int ng) {
  const int g = group ? group[r] : 0;
  return g >= 0 && g < ng ? g : -1;
}

__global__ __launch_bounds__(256) void metrics_update_kernel(double* __restrict__ table, const rmcl_metric_ops ops) {
  const rmcl_metric_op& op = ops.op[blockIdx.x];
  const int kind = op.kind;
  double* __restrict__ slot = table + 2 * (long)op.slot;
  if (kind == RMCL_METRIC_SCALAR || kind == RMCL_METRIC_PAIR) {
    if (threadIdx.x != 0) return;
    const float* a = reinterpret_cast<const float*>(op.a);
    if (kind == RMCL_METRIC_SCALAR) {
      const float* gate = reinterpret_cast<const float*>(op.b);
      if (gate && gate[0] == 0.f) return;                    // (the loss of a batch without a labelled row: not a byte is written)
      slot[0] += (double)op.scale * (double)(a ? a[0] : op.imm);
      slot[1] += 1.0;
    } else {
      const double den = (double)reinterpret_cast<const float*>(op.b)[0];
      if (den != 0.0) {
        slot[0] += (double)a[0];
        slot[1] += den;
      }
    }
    return;
  }
  __shared__ double sh_sum[4][MG];
  __shared__ int sh_cnt[4][MG], sh_hit[4][MG];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = op.rows, ng = op.n_groups;
  const int* __restrict__ group = op.group;
  double sum[MG];
  int cnt[MG], hit[MG];
#pragma unroll
  for (int j = 0; j < MG; ++j) { sum[j] = 0.0; cnt[j] = 0; hit[j] = 0; }

  if (kind == RMCL_METRIC_ROWSUM || kind == RMCL_METRIC_ROWMEAN) {
    const float* __restrict__ x = reinterpret_cast<const float*>(op.a);
    const long stride = op.stride;
    for (int r = threadIdx.x; r < rows; r += 256) {
      const int g = row_group(group, r, ng);
      const double v = (double)x[(long)r * stride];
#pragma unroll
      for (int j = 0; j < MG; ++j)
        if (g == j) { sum[j] += v; cnt[j] += 1; }
    }
  } else {
    const bool invert = (op.flags & RMCL_METRIC_INVERT) != 0;
    const int ignore = op.ignore_index;
    const int* __restrict__ b = reinterpret_cast<const int*>(op.b);
    if (kind == RMCL_METRIC_MATCH) {
      const int* __restrict__ a = reinterpret_cast<const int*>(op.a);
      for (int r = threadIdx.x; r < rows; r += 256) {
        const int g = row_group(group, r, ng);
        const int av = a[r], bv = b[r];
        const bool use = invert || bv != ignore;
        const int h = invert ? (av != bv) : (av == bv);
#pragma unroll
        for (int j = 0; j < MG; ++j)
          if (g == j && use) { cnt[j] += 1; hit[j] += h; }
      }
    } else {                                                 // RMCL_METRIC_ARGMAX_MATCH: wave w owns rows w, w + 4, ...
      const float* __restrict__ z = reinterpret_cast<const float*>(op.a);
      const int ncols = op.ncols;
      const long pitch = op.pitch;
      for (int r = wave; r < rows; r += 4) {
        const float* __restrict__ row = z + (long)r * pitch;
        float v = -INFINITY;
        int i = INT_MAX;                                     // (a lane without a column: -inf and an index behind the last one)
        for (int c = lane; c < ncols; c += 64) {
          const float zc = row[c];
          if (i == INT_MAX || zc > v) { v = zc; i = c; }     // ascending columns and a strict >: the lane keeps its first maximum
        }
        wave_argmax_first(v, i);
        const int g = row_group(group, r, ng);
        const int bv = b[r];
        const bool use = lane == 0 && (invert || bv != ignore);
        const int h = invert ? (i != bv) : (i == bv);
#pragma unroll
        for (int j = 0; j < MG; ++j)
          if (g == j && use) { cnt[j] += 1; hit[j] += h; }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < MG; ++j) {
    const double s = wave_sum_f64(sum[j]);
    const int c = wave_sum_i32(cnt[j]), h = wave_sum_i32(hit[j]);
    if (lane == 0) { sh_sum[wave][j] = s; sh_cnt[wave][j] = c; sh_hit[wave][j] = h; }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int j = 0; j < ng; ++j) {
    const int c = sh_cnt[0][j] + sh_cnt[1][j] + sh_cnt[2][j] + sh_cnt[3][j];
    if (c == 0) continue;                                    // an empty group (rows == 0, no labelled row): not a byte is written
    const double s = ((sh_sum[0][j] + sh_sum[1][j]) + sh_sum[2][j]) + sh_sum[3][j];
    const int h = sh_hit[0][j] + sh_hit[1][j] + sh_hit[2][j] + sh_hit[3][j];
    double add, n;
    if (kind == RMCL_METRIC_ROWSUM) { add = s; n = (double)c; }
    else if (kind == RMCL_METRIC_ROWMEAN) { add = s / (double)c; n = 1.0; }
    else { add = (double)h; n = (double)c; }
    slot[2 * j] += add;
    slot[2 * j + 1] += n;
  }
}

}  // namespace

extern "C" int rmcl_metrics_update(double* table, int n_slots, const rmcl_metric_ops* ops, void* stream) {
  RMCL_REQUIRE(table && ops, "metrics_update: NULL argument");
  RMCL_REQUIRE(n_slots >= 1, "metrics_update: n_slots < 1");
  const int n = ops->n_ops;
  RMCL_REQUIRE(n >= 1 && n <= RMCL_METRIC_MAX_OPS, "metrics_update: n_ops outside 1 .. 8");
  long lo[RMCL_METRIC_MAX_OPS], hi[RMCL_METRIC_MAX_OPS];
  for (int i = 0; i < n; ++i) {
    const rmcl_metric_op& o = ops->op[i];
    RMCL_REQUIRE(o.kind >= RMCL_METRIC_SCALAR && o.kind <= RMCL_METRIC_ARGMAX_MATCH, "metrics_update: unknown kind");
    RMCL_REQUIRE((o.flags & ~RMCL_METRIC_INVERT) == 0, "metrics_update: unknown flag");
    RMCL_REQUIRE(o.n_groups >= 1 && o.n_groups <= RMCL_METRIC_MAX_GROUPS, "metrics_update: n_groups outside 1 .. 4");
    const bool row_kind = o.kind >= RMCL_METRIC_ROWSUM;
    lo[i] = o.slot;
    hi[i] = (long)o.slot + (row_kind ? o.n_groups : 1);
    RMCL_REQUIRE(o.slot >= 0 && o.slot < n_slots && hi[i] <= n_slots, "metrics_update: slot range outside [0, n_slots)");
    switch (o.kind) {
      case RMCL_METRIC_SCALAR: break;                        // (a NULL: the immediate; b NULL: no gate)
      case RMCL_METRIC_PAIR: RMCL_REQUIRE(o.a && o.b, "metrics_update: PAIR with a NULL pointer"); break;
      case RMCL_METRIC_ROWSUM:
      case RMCL_METRIC_ROWMEAN: RMCL_REQUIRE(o.a, "metrics_update: ROWSUM / ROWMEAN with a NULL pointer"); break;
      default: RMCL_REQUIRE(o.a && o.b, "metrics_update: MATCH / ARGMAX_MATCH with a NULL pointer"); break;
    }
    if (row_kind) {
      RMCL_REQUIRE(o.rows >= 0, "metrics_update: rows < 0");
      RMCL_REQUIRE(o.kind > RMCL_METRIC_ROWMEAN || o.stride >= 1, "metrics_update: stride < 1");
      RMCL_REQUIRE(o.kind != RMCL_METRIC_ARGMAX_MATCH || (o.ncols >= 1 && o.ncols <= o.pitch), "metrics_update: ncols outside 1 .. pitch");
    }
    for (int k = 0; k < i; ++k)
      RMCL_REQUIRE(hi[k] <= lo[i] || hi[i] <= lo[k], "metrics_update: two ops of one call share a slot");
  }
  RMCL_LAUNCH(metrics_update_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, table, *ops);
  RMCL_CHECK_LAUNCH();
  return 0;
}
