// RandAugment on the device (rmcl_randaug_u8, include/rmcl.h): the fourteen operations of the reference's vilt/transforms/randaug.py on the
// decoded bytes of a zero-padded batch [B, Hs, Ws, 3], every sample in its own h x w rectangle, in PIL's own arithmetic - the output bytes are
// PIL's bytes (vilt/transforms/randaug_model.py is the numpy statement of the same arithmetic, pinned against PIL on the CPU).
//
// Per stage s of the plan, three kernels:
//   statistics  three 256-bin histograms (AutoContrast, Equalize) or the sum of the luma (Contrast) of every sample whose stage-s op needs
//               them: LDS integer atomics per workgroup, merged into global memory with integer atomics - order-independent, so the result
//               is bit-reproducible.  Workgroups of other samples leave at once; the launch is skipped when no sample needs it.
//   table       one workgroup per sample builds the 3 x 256-byte table of the lookup-class ops (AutoContrast, Equalize, Posterize, Solarize,
//               SolarizeAdd, and Contrast / Brightness, whose degenerate image is a constant so that the blend is a function of the byte).
//   apply       one thread per pixel, the op class uniform per workgroup: table lookup, Color (luma + blend), the 16.16 fixed-point gather of
//               Rotate / ShearX / ShearY, the translate gather, the 3 x 3 SMOOTH stencil + blend of Sharpness.  Writes the whole padded
//               extent: zeros outside the sample.
// Stages ping-pong src -> tmp -> dst so that the last one lands in dst.
//
// PIL's blend, its 3 x 3 filter and AutoContrast's table are C arithmetic with SEPARATE multiply and add, and a fused multiply-add changes
// bytes (188 of the 65 536 (degenerate, source) pairs of the blend at factor 1.36).  The library is built with -ffp-contract=fast, under
// which the backend fuses whatever a pragma says: every product whose rounding matters goes through ra_mul, which pins it in a register.
#include "rmcl_common.h"
#include "kernels.h"

// a * b rounded on its own: the empty asm makes the product opaque, so no later add can be contracted into it under any -ffp-contract
__device__ __forceinline__ float ra_mul(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ double ra_mul(double a, double b) {
  double p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

enum { RA_AUTOCONTRAST = 0, RA_EQUALIZE = 1, RA_ROTATE = 2, RA_POSTERIZE = 3, RA_SOLARIZE = 4, RA_SOLARIZE_ADD = 5, RA_COLOR = 6, RA_CONTRAST = 7,
       RA_BRIGHTNESS = 8, RA_SHARPNESS = 9, RA_SHEAR_X = 10, RA_SHEAR_Y = 11, RA_TRANSLATE_X = 12, RA_TRANSLATE_Y = 13, RA_N_OPS = 14 };
#define RA_LOOKUP_MASK 0x1BB          // codes 0, 1, 3, 4, 5, 7, 8
#define RA_STAT_WORDS 784             // per sample: 3 x 256 histogram bins (u32), the luma sum (u64) at word 768, padding to 16 bytes
#define RA_TABLE_BYTES 768
#define RA_STAT_ROWS 8

__host__ __device__ static inline bool ra_is_lookup(int op) { return (RA_LOOKUP_MASK >> op) & 1; }
__host__ __device__ static inline bool ra_needs_hist(int op) { return op == RA_AUTOCONTRAST || op == RA_EQUALIZE; }

// the extents come from device memory the wrapper cannot read: clamped here, so no index below leaves the batch whatever they hold
__device__ __forceinline__ void ra_extent(const int* __restrict__ sizes, int b, int Hs, int Ws, int& h, int& w) {
  h = min(max(sizes[2 * b], 0), Hs);
  w = min(max(sizes[2 * b + 1], 0), Ws);
}
__device__ __forceinline__ int ra_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }
__device__ __forceinline__ int ra_clip8(float t) { return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t); }
// Image.blend(degenerate d, source s, f): interpolation (0 <= f <= 1) truncates, extrapolation clips
__device__ __forceinline__ int ra_blend(int d, int s, float f, bool interp) {
  const float t = (float)d + ra_mul(f, (float)(s - d));
  return interp ? (int)t : ra_clip8(t);
}

__global__ __launch_bounds__(256) void randaug_stats_kernel(const unsigned char* __restrict__ in, const int* __restrict__ sizes,
                                                            const int* __restrict__ ops, int n_ops, int stage, int Hs, int Ws,
                                                            unsigned int* __restrict__ stats) {
  const int b = blockIdx.y, op = ops[b * n_ops + stage];
  const bool hist = ra_needs_hist(op);
  if (!hist && op != RA_CONTRAST) return;
  int h, w;
  ra_extent(sizes, b, Hs, Ws, h, w);
  const int y0 = blockIdx.x * RA_STAT_ROWS, y1 = min(y0 + RA_STAT_ROWS, h);
  if (y0 >= h) return;
  __shared__ unsigned int bins[768];
  for (int i = threadIdx.x; i < 768; i += 256) bins[i] = 0;
  __syncthreads();
  unsigned int lsum = 0;                                         // at most 8 rows x ceil(w / 256) pixels x 255 per thread
  for (int y = y0; y < y1; ++y) {
    const unsigned char* row = in + ((long)b * Hs + y) * Ws * 3;
    for (int x = threadIdx.x; x < w; x += 256) {
      const int r = row[3 * x], g = row[3 * x + 1], bl = row[3 * x + 2];
      if (hist) {
        atomicAdd(&bins[r], 1u);
        atomicAdd(&bins[256 + g], 1u);
        atomicAdd(&bins[512 + bl], 1u);
      } else {
        lsum += (unsigned int)ra_luma(r, g, bl);
      }
    }
  }
  unsigned int* st = stats + (long)b * RA_STAT_WORDS;
  if (hist) {
    __syncthreads();
    for (int i = threadIdx.x; i < 768; i += 256)
      if (bins[i]) atomicAdd(&st[i], bins[i]);
  } else {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(st + 768), (unsigned long long)lsum);
  }
}

__global__ __launch_bounds__(256) void randaug_table_kernel(const int* __restrict__ sizes, const int* __restrict__ ops,
                                                            const double* __restrict__ params, int n_ops, int stage, int Hs, int Ws,
                                                            const unsigned int* __restrict__ stats, unsigned char* __restrict__ tables) {
  const int b = blockIdx.x, op = ops[b * n_ops + stage], i = threadIdx.x;
  if (!ra_is_lookup(op)) return;
  const double p0 = params[((long)b * n_ops + stage) * 6];
  const unsigned int* st = stats + (long)b * RA_STAT_WORDS;
  unsigned char* t = tables + (long)b * RA_TABLE_BYTES;
  if (ra_needs_hist(op)) {
    __shared__ unsigned int bins[768];
    __shared__ int lo[3], hi[3];
    for (int k = i; k < 768; k += 256) bins[k] = st[k];
    if (i < 3) { lo[i] = 256; hi[i] = -1; }
    __syncthreads();
    for (int c = 0; c < 3; ++c)
      if (bins[c * 256 + i]) { atomicMin(&lo[c], i); atomicMax(&hi[c], i); }
    __syncthreads();
    for (int c = 0; c < 3; ++c) {
      const int l = lo[c], u = hi[c];
      int v = i;                                                  // identity: an empty or single-valued channel
      if (u > l) {
        if (op == RA_AUTOCONTRAST) {
          const double scale = 255.0 / (double)(u - l), off = -ra_mul((double)l, scale);   // (a bare product would fuse into the sum below)
          v = min(max((int)(ra_mul((double)i, scale) + off), 0), 255);
        } else {
          // Equalize: lut[i] = min((step / 2 + sum of the bins below i) / step, 255); every lane reads the same bin at the same time
          unsigned int below = 0, total = 0;
          for (int j = 0; j < 256; ++j) {
            const unsigned int n = bins[c * 256 + j];
            total += n;
            if (j < i) below += n;
          }
          const unsigned int step = (total - bins[c * 256 + u]) / 255u;
          if (step) v = (int)min((step / 2 + below) / step, 255u);
        }
      }
      t[c * 256 + i] = (unsigned char)v;
    }
    return;
  }
  int v;
  if (op == RA_POSTERIZE) {
    const int bits = min(max((int)p0, 1), 8);
    v = i & ~((1 << (8 - bits)) - 1);
  } else if (op == RA_SOLARIZE) {
    v = (double)i < p0 ? i : 255 - i;
  } else if (op == RA_SOLARIZE_ADD) {
    const double s = (double)i + p0;
    const int u = (int)(s < 0.0 ? 0.0 : (s > 255.0 ? 255.0 : s));
    v = u < 128 ? u : 255 - u;
  } else {                                                        // Contrast (degenerate: the mean luma) / Brightness (degenerate: 0)
    int d = 0;
    if (op == RA_CONTRAST) {
      int h, w;
      ra_extent(sizes, b, Hs, Ws, h, w);
      const unsigned long long n = (unsigned long long)h * w, sum = *reinterpret_cast<const unsigned long long*>(st + 768);
      d = n ? (int)((2 * sum + n) / (2 * n)) : 0;
    }
    const float f = (float)p0;
    v = ra_blend(d, i, f, f >= 0.f && f <= 1.f);
  }
  t[i] = t[256 + i] = t[512 + i] = (unsigned char)v;
}

// PIL's FIX: floor(v * 65536 + 0.5)
__device__ __forceinline__ int ra_fix16(double v) {
  const double t = v * 65536.0 + 0.5;
  return t >= 0.0 ? (int)t : (int)floor(t);
}
// PIL's COORD on the scale path: a negative coordinate is outside, everything else truncates
__device__ __forceinline__ int ra_coord(double v) { return v < 0.0 ? -1 : (int)v; }

__global__ __launch_bounds__(256) void randaug_apply_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                            const int* __restrict__ sizes, const int* __restrict__ ops,
                                                            const double* __restrict__ params, int n_ops, int stage, int Hs, int Ws,
                                                            const unsigned char* __restrict__ tables) {
  const int b = blockIdx.z, op = ops[b * n_ops + stage];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  __shared__ unsigned char lut[RA_TABLE_BYTES];
  const bool lookup = ra_is_lookup(op);                           // uniform over the workgroup
  if (lookup) {
    for (int k = threadIdx.x; k < RA_TABLE_BYTES; k += 256) lut[k] = tables[(long)b * RA_TABLE_BYTES + k];
    __syncthreads();
  }
  if (x >= Ws || y >= Hs) return;
  int h, w;
  ra_extent(sizes, b, Hs, Ws, h, w);
  const unsigned char* img = in + (long)b * Hs * Ws * 3;
  int o0 = 0, o1 = 0, o2 = 0;                                     // outside the sample: the zeros of the collate padding
  if (x < w && y < h) {
    const double* a = params + ((long)b * n_ops + stage) * 6;
    const unsigned char* p = img + ((long)y * Ws + x) * 3;
    if (lookup) {
      o0 = lut[p[0]]; o1 = lut[256 + p[1]]; o2 = lut[512 + p[2]];
    } else if (op == RA_COLOR) {
      const float f = (float)a[0];
      const bool interp = f >= 0.f && f <= 1.f;
      const int r = p[0], g = p[1], bl = p[2], l = ra_luma(r, g, bl);
      o0 = ra_blend(l, r, f, interp); o1 = ra_blend(l, g, f, interp); o2 = ra_blend(l, bl, f, interp);
    } else if (op == RA_SHARPNESS) {
      const float f = (float)a[0];
      const bool interp = f >= 0.f && f <= 1.f;
      int d0 = p[0], d1 = p[1], d2 = p[2];                        // the border (and an image with a side below 3) keeps the source
      if (x >= 1 && y >= 1 && x < w - 1 && y < h - 1) {
        const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
        float s0 = 0.5f, s1 = 0.5f, s2 = 0.5f;
#pragma unroll
        for (int dy = 1; dy >= -1; --dy) {                        // rows y + 1, y, y - 1: PIL's order of the float additions
          const unsigned char* q = p + (long)dy * Ws * 3;
          const float kc = dy == 0 ? k5 : k1;
          s0 += (ra_mul((float)q[-3], k1) + ra_mul((float)q[0], kc)) + ra_mul((float)q[3], k1);
          s1 += (ra_mul((float)q[-2], k1) + ra_mul((float)q[1], kc)) + ra_mul((float)q[4], k1);
          s2 += (ra_mul((float)q[-1], k1) + ra_mul((float)q[2], kc)) + ra_mul((float)q[5], k1);
        }
        d0 = ra_clip8(s0); d1 = ra_clip8(s1); d2 = ra_clip8(s2);
      }
      o0 = ra_blend(d0, p[0], f, interp); o1 = ra_blend(d1, p[1], f, interp); o2 = ra_blend(d2, p[2], f, interp);
    } else {
      int xin, yin;
      if (op == RA_TRANSLATE_X || op == RA_TRANSLATE_Y) {
        xin = ra_coord((a[2] + a[0] * 0.5) + (double)x);
        yin = ra_coord((a[5] + a[4] * 0.5) + (double)y);
      } else {                                                    // Rotate, ShearX, ShearY: 32-bit wrap-around like PIL's running sums
        const unsigned int a0 = ra_fix16(a[0]), a1 = ra_fix16(a[1]), a3 = ra_fix16(a[3]), a4 = ra_fix16(a[4]);
        const unsigned int a2 = ra_fix16(a[2] + a[0] * 0.5 + a[1] * 0.5), a5 = ra_fix16(a[5] + a[3] * 0.5 + a[4] * 0.5);
        xin = (int)(a2 + (unsigned int)y * a1 + (unsigned int)x * a0) >> 16;
        yin = (int)(a5 + (unsigned int)y * a4 + (unsigned int)x * a3) >> 16;
      }
      if (xin >= 0 && xin < w && yin >= 0 && yin < h) {
        const unsigned char* q = img + ((long)yin * Ws + xin) * 3;
        o0 = q[0]; o1 = q[1]; o2 = q[2];
      }
    }
  }
  unsigned char* dst = out + (((long)b * Hs + y) * Ws + x) * 3;
  dst[0] = (unsigned char)o0; dst[1] = (unsigned char)o1; dst[2] = (unsigned char)o2;
}

// scratch: [B][RA_STAT_WORDS] u32 statistics | [B][768] tables | params double [B, n_ops, 6] | ops int32 [B, n_ops] (device copies of the plan)
long rmcl_randaug_scratch(int B, int n_ops) {
  return (long)B * (RA_STAT_WORDS * 4 + RA_TABLE_BYTES) + (long)B * n_ops * (6 * 8 + 4);
}
int rmcl_randaug(const unsigned char* src, const int* sizes, int B, int Hs, int Ws, const int* ops_host, const double* params_host, int n_ops,
                 unsigned char* tmp, void* scratch, unsigned char* dst, hipStream_t s) {
  RMCL_REQUIRE(B > 0 && B <= 65535 && Hs > 0 && Ws > 0 && Hs <= 4 * 65535, "randaug: bad dims");
  bool stats[8] = {}, lookup[8] = {};
  for (long k = 0; k < (long)B * n_ops; ++k) {
    const int op = ops_host[k], st = (int)(k % n_ops);
    stats[st] |= ra_needs_hist(op) || op == RA_CONTRAST;
    lookup[st] |= ra_is_lookup(op);
  }
  char* base = reinterpret_cast<char*>(scratch);
  unsigned int* st_d = reinterpret_cast<unsigned int*>(base);
  unsigned char* tab_d = reinterpret_cast<unsigned char*>(base + (size_t)B * RA_STAT_WORDS * 4);
  double* par_d = reinterpret_cast<double*>(base + (size_t)B * (RA_STAT_WORDS * 4 + RA_TABLE_BYTES));
  int* ops_d = reinterpret_cast<int*>(par_d + (size_t)B * n_ops * 6);
  HIP_TRY(hipMemcpyAsync(par_d, params_host, (size_t)B * n_ops * 6 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ops_d, ops_host, (size_t)B * n_ops * sizeof(int), hipMemcpyHostToDevice, s));
  const unsigned char* in = src;
  for (int stage = 0; stage < n_ops; ++stage) {
    unsigned char* out = (n_ops - 1 - stage) % 2 == 0 ? dst : tmp;
    if (stats[stage]) {
      HIP_TRY(hipMemsetAsync(st_d, 0, (size_t)B * RA_STAT_WORDS * 4, s));
      RMCL_LAUNCH(randaug_stats_kernel, dim3(cdiv(Hs, RA_STAT_ROWS), B), dim3(256), 0, s, in, sizes, ops_d, n_ops, stage, Hs, Ws, st_d);
      RMCL_CHECK_LAUNCH();
    }
    if (lookup[stage]) {
      RMCL_LAUNCH(randaug_table_kernel, dim3(B), dim3(256), 0, s, sizes, ops_d, par_d, n_ops, stage, Hs, Ws, st_d, tab_d);
      RMCL_CHECK_LAUNCH();
    }
    RMCL_LAUNCH(randaug_apply_kernel, dim3(cdiv(Ws, 64), cdiv(Hs, 4), B), dim3(256), 0, s, in, out, sizes, ops_d, par_d, n_ops, stage, Hs, Ws, tab_d);
    RMCL_CHECK_LAUNCH();
    in = out;
  }
  return 0;
}
