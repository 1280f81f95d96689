// PGD threat models in patch layout (include/rmcl.h "PGD threat models"): one ascent step with a choice of direction (the
// reference's g / max|g|, sign(g), g / ||g||_2), projection onto the L-inf or the L2 ball, an optional pixel box, and the next
// forward's operand in the same pass; a counter-based random start; and the per-sample worst case over restarts.
//
// Streaming form of the PGD kernels of embed_misc.hip: 16-byte accesses, min(ceil(per_sample / 1024), 64) blocks per sample, per-block
// partials in a caller-provided scratch that need not be cleared (slot blockIdx.x of the sample's 64; slots of blocks that do not
// exist are neither written nor read), no atomics.  Sums of squares are accumulated in double: per thread in element order, across the
// wave by a fixed butterfly, across the block's four waves and the sample's partials in slot order - a repeated call writes the same bytes.
//
// Scratch of B samples (rmcl_pgd_ball_scratch_bytes): double sq[B][2][64] (0: direction norm ||g||^2 or the start's ||v||^2,
// 1: projection norm ||t||^2), then uint32 amax[B][64].
//
// Passes of rmcl_pgd_step_ball (bytes per element, gradient of G bytes, operand of O bytes):
//   direction NORMALISED / L2   one statistics pass over g                        G
//   ball L2, eps > 0            one norm pass: t = delta_old + lr d, ||t||^2      G + 4   (G with DELTA_ZERO)
//   always                      the step: t again (the same instructions, so the same bits as the norm pass saw), projection, box,
//                               delta and operand                                 G + 4 + 4 + 4 + O   (4 less with DELTA_ZERO)
// The norm pass writes nothing but its partials: recomputing t costs G + 4 bytes of reads where storing it would cost 4 written and 4
// read again, and it leaves delta untouched until the last pass.
#include <math.h>
#include <algorithm>
#include "rmcl_common.h"
#include "../../include/rmcl.h"

namespace {

constexpr int SLOTS = 64;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the block's sum in thread 0 (four waves, added in wave order)
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double red[4];
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double tot = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();                                         // (the slots may be written again by a later call)
  return tot;
}
// sum over the sample's nb partials, in every thread of the block
__device__ __forceinline__ double partial_sum(const double* __restrict__ part, int nb) {
  __shared__ double stot;
  if (threadIdx.x < 64) {
    double v = (int)threadIdx.x < nb ? part[threadIdx.x] : 0.0;
    v = wave_sum_f64(v);
    if (threadIdx.x == 0) stot = v;
  }
  __syncthreads();
  const double tot = stot;
  __syncthreads();
  return tot;
}
__device__ __forceinline__ float partial_max(const unsigned* __restrict__ part, int nb) {
  __shared__ float smax;
  if (threadIdx.x < 64) {
    float m = (int)threadIdx.x < nb ? __uint_as_float(part[threadIdx.x]) : 0.f;
    m = wave_max(m);
    if (threadIdx.x == 0) smax = m;
  }
  __syncthreads();
  const float m = smax;
  __syncthreads();
  return m;
}

// number of leading elements of sample b that belong to real patches (NULL: all), kept inside [0, per]
__device__ __forceinline__ long valid_count(const int* __restrict__ valid, int b, long per) {
  if (!valid) return per;
  const long v = valid[b];
  return v < 0 ? 0 : (v > per ? per : v);
}

struct Scratch {
  double* sq;        // [B][2][64]
  unsigned* amax;    // [B][64]
  __host__ __device__ Scratch(void* p, int B) : sq((double*)p), amax((unsigned*)((double*)p + (long)B * 2 * SLOTS)) {}
  __device__ double* sq_of(int b, int which) const { return sq + ((long)b * 2 + which) * SLOTS; }
};

template <typename T>
__device__ __forceinline__ void load4(const T* __restrict__ p, float (&v)[4]) {
  if constexpr (sizeof(T) == 2) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
  } else {
    const float4 u = *reinterpret_cast<const float4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  }
}

// The ascent direction's denominator of sample b from the statistics pass's partials: max(max|g|, 1e-8) (the arithmetic of
// pgd_update_fused_kernel), max(||g||_2, 1e-12), or 1 for sign(g).  Every thread of the block calls it.
__device__ __forceinline__ float direction_den(const Scratch& sc, int b, int nb, int dir) {
  if (dir == RMCL_PGD_DIR_NORMALISED) return fmaxf(partial_max(sc.amax + (long)b * SLOTS, nb), 1e-8f);
  if (dir == RMCL_PGD_DIR_L2) return fmaxf((float)sqrt(partial_sum(sc.sq_of(b, 0), nb)), 1e-12f);
  return 1.f;
}
// t = delta_old + lr d for four elements; the norm pass and the step both go through this one function.  Pad elements give 0.
template <bool ZERO>
__device__ __forceinline__ void ascent4(const float (&g)[4], const float* __restrict__ delta, long i, long nvalid, float lr, float den,
                                        int dir, float (&t)[4]) {
  float old[4] = {0.f, 0.f, 0.f, 0.f};
  if (!ZERO) { const float4 v = *reinterpret_cast<const float4*>(delta + i); old[0] = v.x; old[1] = v.y; old[2] = v.z; old[3] = v.w; }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float num = dir == RMCL_PGD_DIR_SIGN ? (g[j] > 0.f ? 1.f : (g[j] < 0.f ? -1.f : 0.f)) : g[j];
    const float v = old[j] + lr * num / den;
    t[j] = i + j < nvalid ? v : 0.f;
  }
}

// statistics of the gradient over the valid elements: mode 0 max|g| -> amax, mode 1 sum g^2 -> sq[0]
template <typename T>
__global__ __launch_bounds__(256) void grad_stats_kernel(const T* __restrict__ g, const int* __restrict__ valid, Scratch sc, long per, int dir) {
  const int b = blockIdx.y;
  const long nvalid = valid_count(valid, b, per);
  const T* p = g + (long)b * per;
  float m = 0.f;
  double s = 0.0;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < nvalid; i += (long)gridDim.x * 1024) {
    float v[4];
    load4(p + i, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < nvalid) {
        if (dir == RMCL_PGD_DIR_L2) s += (double)v[j] * (double)v[j];
        else m = fmaxf(m, fabsf(v[j]));
      }
    }
  }
  if (dir == RMCL_PGD_DIR_L2) {
    s = block_sum_f64(s);
    if (threadIdx.x == 0) sc.sq_of(b, 0)[blockIdx.x] = s;
  } else {
    __shared__ float red[4];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) sc.amax[(long)b * SLOTS + blockIdx.x] = __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
  }
}

// ||t||^2 of the unprojected step -> sq[1]
template <typename T, bool ZERO>
__global__ __launch_bounds__(256) void step_norm_kernel(const T* __restrict__ g, const float* __restrict__ delta, const int* __restrict__ valid,
                                                        Scratch sc, long per, float lr, int dir) {
  const int b = blockIdx.y;
  const long nvalid = valid_count(valid, b, per);
  const float den = direction_den(sc, b, gridDim.x, dir);
  const long off = (long)b * per;
  double s = 0.0;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < nvalid; i += (long)gridDim.x * 1024) {
    float gv[4], t[4];
    load4(g + off + i, gv);
    ascent4<ZERO>(gv, delta + off, i, nvalid, lr, den, dir, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (double)t[j] * (double)t[j];
  }
  s = block_sum_f64(s);
  if (threadIdx.x == 0) sc.sq_of(b, 1)[blockIdx.x] = s;
}

// box and stores shared by the step and the random start: t (projected, 0 on pads) -> delta_new and the operand
template <typename TO>
__device__ __forceinline__ void finish4(float (&t)[4], const float* __restrict__ base, float* __restrict__ delta, TO* __restrict__ out,
                                        long i, long nvalid, bool box, float lo, float hi) {
  if (base) {
    const float4 a = *reinterpret_cast<const float4*>(base + i);
    const float bv[4] = {a.x, a.y, a.z, a.w};
    float x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = __fadd_rn(bv[j], t[j]);                           // (the sum of the STORED delta: never contracted with the scaling before it)
      if (box && i + j < nvalid) {
        x[j] = fminf(fmaxf(x[j], lo), hi);
        t[j] = x[j] - bv[j];
      }
    }
    if (out) store4<TO>(out + i, x);
  }
  *reinterpret_cast<float4*>(delta + i) = make_float4(t[0], t[1], t[2], t[3]);
}

template <typename T, typename TO, bool ZERO>
__global__ __launch_bounds__(256) void step_ball_kernel(const T* __restrict__ g, float* __restrict__ delta, const int* __restrict__ valid,
                                                        Scratch sc, const float* __restrict__ base, TO* __restrict__ out, long per,
                                                        float lr, float eps, int dir, int ball, int box, float lo, float hi) {
  const int b = blockIdx.y;
  const long nvalid = valid_count(valid, b, per);
  const float den = direction_den(sc, b, gridDim.x, dir);
  float scale = 1.f;
  if (ball == RMCL_PGD_BALL_L2 && eps > 0.f) {
    const float nrm = (float)sqrt(partial_sum(sc.sq_of(b, 1), gridDim.x));
    scale = nrm > eps ? eps / nrm : 1.f;
  }
  const long off = (long)b * per;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < per; i += (long)gridDim.x * 1024) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < nvalid) {
      float gv[4];
      load4(g + off + i, gv);
      ascent4<ZERO>(gv, delta + off, i, nvalid, lr, den, dir, t);
      if (eps > 0.f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = ball == RMCL_PGD_BALL_LINF ? fminf(fmaxf(t[j], -eps), eps) : t[j] * scale;
      }
    }
    finish4<TO>(t, base ? base + off : nullptr, delta + off, out ? out + off : nullptr, i, nvalid, box != 0, lo, hi);
  }
}

// v = 2u - 1, u = (h >> 8) 2^-24, h = hash(hash(seed, sample), element): exact in fp32
__device__ __forceinline__ float start_draw(uint32_t sample_seed, uint32_t elem) {
  const float u = (float)(rmcl_rng_hash(sample_seed, elem) >> 8) * 5.9604644775390625e-08f;
  return 2.f * u - 1.f;
}
__global__ __launch_bounds__(256) void start_norm_kernel(const int* __restrict__ valid, Scratch sc, long per, uint32_t seed, int sample0) {
  const int b = blockIdx.y;
  const long nvalid = valid_count(valid, b, per);
  const uint32_t ss = rmcl_rng_hash(seed, (uint32_t)(sample0 + b));
  double s = 0.0;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < nvalid; i += (long)gridDim.x * 1024) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = i + j < nvalid ? start_draw(ss, (uint32_t)(i + j)) : 0.f;
      s += (double)v * (double)v;
    }
  }
  s = block_sum_f64(s);
  if (threadIdx.x == 0) sc.sq_of(b, 0)[blockIdx.x] = s;
}
template <typename TO>
__global__ __launch_bounds__(256) void random_start_kernel(float* __restrict__ delta, const int* __restrict__ valid, Scratch sc,
                                                           const float* __restrict__ base, TO* __restrict__ out, long per, uint32_t seed,
                                                           int sample0, float eps, int ball, int box, float lo, float hi) {
  const int b = blockIdx.y;
  const long nvalid = valid_count(valid, b, per);
  const uint32_t ss = rmcl_rng_hash(seed, (uint32_t)(sample0 + b));
  float nrm = 1.f;
  if (ball == RMCL_PGD_BALL_L2) nrm = fmaxf((float)sqrt(partial_sum(sc.sq_of(b, 0), gridDim.x)), 1e-12f);
  const long off = (long)b * per;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < per; i += (long)gridDim.x * 1024) {
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = __fmul_rn(eps, start_draw(ss, (uint32_t)(i + j)));     // (its own rounding: never contracted into base + eps v)
      t[j] = i + j < nvalid ? (ball == RMCL_PGD_BALL_L2 ? v / nrm : v) : 0.f;
    }
    finish4<TO>(t, base ? base + off : nullptr, delta + off, out ? out + off : nullptr, i, nvalid, box != 0, lo, hi);
  }
}

// rows of the decisions that take the new restart: delta and operand rows are copied; the scores are updated by the kernel behind it
template <typename TO>
__global__ __launch_bounds__(256) void keep_rows_kernel(const float* __restrict__ score_new, long stride, const float* __restrict__ best_score,
                                                        int restart, int G, const float* __restrict__ delta, float* __restrict__ best_delta,
                                                        const TO* __restrict__ op, TO* __restrict__ best_op, long per) {
  const int b = blockIdx.y, j = b / G;
  if (!(restart == 0 || score_new[j * stride] > best_score[j])) return;           // (uniform over the block; a NaN compares false)
  const long off = (long)b * per;
  for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < per; i += (long)gridDim.x * 1024) {
    *reinterpret_cast<float4*>(best_delta + off + i) = *reinterpret_cast<const float4*>(delta + off + i);
    if (op) {
      if constexpr (sizeof(TO) == 2) *reinterpret_cast<uint2*>(best_op + off + i) = *reinterpret_cast<const uint2*>(op + off + i);
      else *reinterpret_cast<float4*>(best_op + off + i) = *reinterpret_cast<const float4*>(op + off + i);
    }
  }
}
__global__ __launch_bounds__(256) void keep_scores_kernel(const float* __restrict__ score_new, long stride, float* __restrict__ best_score,
                                                          int* __restrict__ best_restart, int restart, int D) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= D) return;
  const float s = score_new[j * stride];
  if (restart == 0 || s > best_score[j]) {
    best_score[j] = s;
    best_restart[j] = restart;
  }
}

dim3 sample_grid(long per, int B) { return dim3(std::min<long>(cdiv(per, 1024), SLOTS), B); }

template <typename T, typename TO>
void step_launch(const void* g, float* delta, const int* valid, Scratch sc, const float* base, void* out, long per, float lr, float eps, int dir,
                 int ball, int box, float lo, float hi, bool zero, dim3 grid, hipStream_t s) {
  const T* gp = (const T*)g;
  if (ball == RMCL_PGD_BALL_L2 && eps > 0.f) {
    if (zero) RMCL_LAUNCH((step_norm_kernel<T, true>), grid, dim3(256), 0, s, gp, delta, valid, sc, per, lr, dir);
    else RMCL_LAUNCH((step_norm_kernel<T, false>), grid, dim3(256), 0, s, gp, delta, valid, sc, per, lr, dir);
  }
  if (zero) RMCL_LAUNCH((step_ball_kernel<T, TO, true>), grid, dim3(256), 0, s, gp, delta, valid, sc, base, (TO*)out, per, lr, eps, dir, ball, box, lo, hi);
  else RMCL_LAUNCH((step_ball_kernel<T, TO, false>), grid, dim3(256), 0, s, gp, delta, valid, sc, base, (TO*)out, per, lr, eps, dir, ball, box, lo, hi);
}

bool dtype_ok(int dt) { return dt == RMCL_F32 || dt == RMCL_BF16; }

}  // namespace

extern "C" {

int64_t rmcl_pgd_ball_scratch_bytes(int B) { return B < 0 ? -1 : (int64_t)B * (2 * SLOTS * (int64_t)sizeof(double) + SLOTS * (int64_t)sizeof(uint32_t)); }

int rmcl_pgd_step_ball(const void* grad, int dtype, float* delta, void* scratch, const int32_t* valid, int B, int64_t per_sample, float lr,
                       float eps, int direction, int ball, float lo, float hi, const float* base, void* operand, int operand_dtype, int flags,
                       void* stream) {
  RMCL_REQUIRE(grad && delta && scratch, "pgd_step_ball: NULL argument");
  RMCL_REQUIRE(B >= 0 && per_sample >= 0 && per_sample % 4 == 0, "pgd_step_ball: per_sample%4");
  RMCL_REQUIRE(dtype_ok(dtype) && (!operand || dtype_ok(operand_dtype)), "pgd_step_ball: unknown dtype");
  RMCL_REQUIRE(direction == RMCL_PGD_DIR_NORMALISED || direction == RMCL_PGD_DIR_SIGN || direction == RMCL_PGD_DIR_L2, "pgd_step_ball: unknown direction");
  RMCL_REQUIRE(ball == RMCL_PGD_BALL_LINF || ball == RMCL_PGD_BALL_L2, "pgd_step_ball: unknown ball");
  RMCL_REQUIRE((flags & ~RMCL_PGD_DELTA_ZERO) == 0, "pgd_step_ball: unknown flag");
  const int box = lo < hi;
  RMCL_REQUIRE(base || !(operand || box), "pgd_step_ball: an operand or a box needs the base image (NULL base)");
  if (B == 0 || per_sample == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid = sample_grid(per_sample, B);
  const Scratch sc(scratch, B);
  if (direction != RMCL_PGD_DIR_SIGN) {
    if (dtype == RMCL_F32) RMCL_LAUNCH(grad_stats_kernel<float>, grid, dim3(256), 0, s, (const float*)grad, valid, sc, per_sample, direction);
    else RMCL_LAUNCH(grad_stats_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)grad, valid, sc, per_sample, direction);
  }
  const bool zero = flags & RMCL_PGD_DELTA_ZERO, of32 = !operand || operand_dtype == RMCL_F32;
  if (dtype == RMCL_F32) {
    if (of32) step_launch<float, float>(grad, delta, valid, sc, base, operand, per_sample, lr, eps, direction, ball, box, lo, hi, zero, grid, s);
    else step_launch<float, bf16_t>(grad, delta, valid, sc, base, operand, per_sample, lr, eps, direction, ball, box, lo, hi, zero, grid, s);
  } else {
    if (of32) step_launch<bf16_t, float>(grad, delta, valid, sc, base, operand, per_sample, lr, eps, direction, ball, box, lo, hi, zero, grid, s);
    else step_launch<bf16_t, bf16_t>(grad, delta, valid, sc, base, operand, per_sample, lr, eps, direction, ball, box, lo, hi, zero, grid, s);
  }
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_pgd_random_start(float* delta, void* scratch, const int32_t* valid, int B, int64_t per_sample, int sample0, uint32_t seed, float eps,
                          int ball, float lo, float hi, const float* base, void* operand, int operand_dtype, void* stream) {
  RMCL_REQUIRE(delta && scratch, "pgd_random_start: NULL argument");
  RMCL_REQUIRE(B >= 0 && per_sample >= 0 && per_sample % 4 == 0, "pgd_random_start: per_sample%4");
  RMCL_REQUIRE(sample0 >= 0, "pgd_random_start: sample0 < 0");
  RMCL_REQUIRE(!operand || dtype_ok(operand_dtype), "pgd_random_start: unknown dtype");
  RMCL_REQUIRE(ball == RMCL_PGD_BALL_LINF || ball == RMCL_PGD_BALL_L2, "pgd_random_start: unknown ball");
  const int box = lo < hi;
  RMCL_REQUIRE(base || !(operand || box), "pgd_random_start: an operand or a box needs the base image (NULL base)");
  if (B == 0 || per_sample == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid = sample_grid(per_sample, B);
  const Scratch sc(scratch, B);
  if (ball == RMCL_PGD_BALL_L2) RMCL_LAUNCH(start_norm_kernel, grid, dim3(256), 0, s, valid, sc, per_sample, seed, sample0);
  if (!operand || operand_dtype == RMCL_F32)
    RMCL_LAUNCH(random_start_kernel<float>, grid, dim3(256), 0, s, delta, valid, sc, base, (float*)operand, per_sample, seed, sample0, eps, ball, box, lo, hi);
  else
    RMCL_LAUNCH(random_start_kernel<bf16_t>, grid, dim3(256), 0, s, delta, valid, sc, base, (bf16_t*)operand, per_sample, seed, sample0, eps, ball, box, lo, hi);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_pgd_keep_worst(const float* score_new, int64_t score_stride, float* best_score, int32_t* best_restart, int restart, int D,
                        int rows_per_decision, const float* delta, float* best_delta, const void* operand, void* best_operand,
                        int operand_dtype, int64_t per_sample, void* stream) {
  RMCL_REQUIRE(score_new && best_score && best_restart && delta && best_delta, "pgd_keep_worst: NULL argument");
  RMCL_REQUIRE(!operand == !best_operand, "pgd_keep_worst: operand and best_operand go together (NULL argument)");
  RMCL_REQUIRE(D >= 0 && per_sample >= 0 && per_sample % 4 == 0, "pgd_keep_worst: per_sample%4");
  RMCL_REQUIRE(rows_per_decision == 1 || rows_per_decision == 2, "pgd_keep_worst: rows_per_decision must be 1 or 2");
  RMCL_REQUIRE(restart >= 0 && score_stride >= 1, "pgd_keep_worst: restart >= 0, score_stride >= 1");
  RMCL_REQUIRE(!operand || dtype_ok(operand_dtype), "pgd_keep_worst: unknown dtype");
  if (D == 0) return 0;
  const hipStream_t s = (hipStream_t)stream;
  if (per_sample > 0) {
    const dim3 grid = sample_grid(per_sample, D * rows_per_decision);
    if (!operand || operand_dtype == RMCL_F32)
      RMCL_LAUNCH(keep_rows_kernel<float>, grid, dim3(256), 0, s, score_new, (long)score_stride, best_score, restart, rows_per_decision, delta, best_delta,
                  (const float*)operand, (float*)best_operand, per_sample);
    else
      RMCL_LAUNCH(keep_rows_kernel<bf16_t>, grid, dim3(256), 0, s, score_new, (long)score_stride, best_score, restart, rows_per_decision, delta, best_delta,
                  (const bf16_t*)operand, (bf16_t*)best_operand, per_sample);
  }
  RMCL_LAUNCH(keep_scores_kernel, dim3(cdiv(D, 256)), dim3(256), 0, s, score_new, (long)score_stride, best_score, best_restart, restart, D);
  RMCL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
