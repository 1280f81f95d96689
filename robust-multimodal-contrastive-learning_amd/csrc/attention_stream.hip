// Streaming masked multi-head self-attention for gfx950 (bf16 MFMA, fp32 softmax), forward and backward, 1 <= N <= 512.
// The fused kernels of attention.hip hold all keys of a (batch, head) in LDS and a whole score row in registers, which ends them at
// 256 tokens.  Here keys / values (forward, dQ) and queries / dO (dK, dV) stream through LDS in blocks of 64 rows, double buffered:
// block j + 1 is staged (16-byte global_load_lds) while block j is computed, and no N x N tensor exists anywhere.
//
//  forward : one workgroup (4 waves) per (batch, head, 64 queries); a wave keeps its 16 queries' Q fragments in registers and walks the
//            key blocks with an online softmax: S^T = K Q^T (keys on registers, query on the lane), running maximum m and sum l per
//            query, O^T rescaled by 2^(m_old - m_new) and extended by V^T P^T.  A block whose keys are all masked leaves m at -inf:
//            the exponent base is then 0 instead of m (2^(-inf - 0) = 0 for every score), so leading masked blocks cost nothing and
//            produce no NaN; the first valid key sets m and rescales the still-zero O by 2^(-inf) = 0.
//  backward: two kernels, both recompute P from the saved log-sum-exp:
//     dq  kernel (same decomposition as the forward): delta = rowsum(dO * O) from the forward's bf16 output (written to `delta` for
//                the second kernel), dS = P (dP - delta) / 8, dQ = dS K                                  (K via tr-read)
//     dkv kernel (one workgroup per (batch, head, 128 keys), K / V fragments in registers, Q / dO streamed):
//                dV = P^T dO, dK = dS^T Q on 16x16x16 MFMAs                                              (Q, dO via tr-read)
// Per-row statistics (lse, delta) are fp32 [B, H, NKP], NKP = N rounded up to the 64-row block (rmcl_attn_stream_stat_elems).
// LDS images, source-address swizzles and fragment readers are those of attention.hip (that file is pinned bit for bit by its tests
// and exports none of them, so the few helpers used here are repeated below).
#include "rmcl_common.h"
#include "kernels.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

#define SCALE 0.125f
#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f
#define SCALE_L2 (SCALE * LOG2E)
#define SB 64                 // rows of a streamed block
#define IMG (SB * 128)        // bytes of one 64-row x 64-column bf16 image
#define AS_NW 4               // waves per workgroup, every kernel
#define AS_TPW 2              // dkv kernel: key tiles per wave -> 128 keys per workgroup

// rows [r0, r0 + 64) of a [*, 64] bf16 slice (row pitch ld elements) -> LDS image of 64 rows x 128 B; rows past N - 1 repeat row N - 1
// (finite data that only ever meets P = 0).  r0 is a multiple of 64, so the swizzles see the same low row bits as attention.hip's.
template <bool TR>
__device__ __forceinline__ void stage_block(char* img, const bf16_t* __restrict__ src, long ld, int N, int r0, int wave, int lane) {
#pragma unroll
  for (int inst = wave; inst < SB / 8; inst += AS_NW) {
    const int row = inst * 8 + (lane >> 3), cp = lane & 7;
    int c;
    if (TR) c = (((cp >> 1) ^ ((row >> 1) & 3)) << 1) | (cp & 1);
    else c = cp ^ (row & 7);
    const bf16_t* p = src + (long)min(r0 + row, N - 1) * ld + c * 8;
    __builtin_amdgcn_global_load_lds((glb_void*)p, (lds_void*)(img + inst * 1024), 16, 0, 0);
  }
}

__device__ __forceinline__ bf16x8 frag_row_lds(const char* img, int row0, int s, int lane) {
  const int row = row0 + (lane & 15);
  const int chunk = (4 * s + (lane >> 4)) ^ (row & 7);
  return *reinterpret_cast<const bf16x8*>(img + row * 128 + chunk * 16);
}
// row fragment out of a TRANSPOSED-read image (stage_block<true>)
__device__ __forceinline__ bf16x8 frag_row_ldsT(const char* img, int row0, int s, int lane) {
  const int row = row0 + (lane & 15);
  const int c = 4 * s + (lane >> 4);
  const int cp = (((c >> 1) ^ ((row >> 1) & 3)) << 1) | (c & 1);
  return *reinterpret_cast<const bf16x8*>(img + row * 128 + cp * 16);
}
__device__ __forceinline__ bf16x8 frag_row_global(const bf16_t* __restrict__ src, long ld, int row0, int N, int s, int lane) {
  const int row = min(row0 + (lane & 15), N - 1);
  return *reinterpret_cast<const bf16x8*>(src + (long)row * ld + 32 * s + 8 * (lane >> 4));
}
__device__ __forceinline__ s16x4 tr4(const char* img, int row, int dt, int p) {
  const int t = dt ^ ((row >> 1) & 3);
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + row * 128 + t * 32 + p * 8));
}
// B operand for a 32-deep k step whose k order is the accumulator order: k(g,j) = base + 16*(j>>2) + 4g + (j&3)
__device__ __forceinline__ bf16x8 frag_tr32_lds(const char* img, int base, int dt, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  union { bf16x8 v; s16x4 h[2]; } u;
  u.h[0] = tr4(img, base + 4 * g + q, dt, p);
  u.h[1] = tr4(img, base + 16 + 4 * g + q, dt, p);
  return u.v;
}
// B operand for the 16x16x16 MFMA: rows base + 4g + j
__device__ __forceinline__ s16x4 frag_tr16_lds(const char* img, int base, int dt, int lane) {
  return tr4(img, base + 4 * (lane >> 4) + ((lane & 15) >> 2), dt, lane & 3);
}
__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  union { bf16x8 v; bf16_t e[8]; } u;
#pragma unroll
  for (int i = 0; i < 4; ++i) { u.e[i] = f2bf(a[i]); u.e[4 + i] = f2bf(b[i]); }
  return u.v;
}
__device__ __forceinline__ s16x4 pack4(const f32x4& a) {
  union { s16x4 v; bf16_t e[4]; } u;
#pragma unroll
  for (int i = 0; i < 4; ++i) u.e[i] = f2bf(a[i]);
  return u.v;
}
__device__ __forceinline__ float group_max(float v) {  // across the 4 lane groups that share lane&15
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ void store4(bf16_t* o, const f32x4& v) {
  uint2 pk;
  pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
  pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
  *reinterpret_cast<uint2*>(o) = pk;
}

// Barrier of the streaming loops: this wave's LDS-DMA of the block about to be read has landed before any wave passes (the compiler
// drains it earlier today, behind the first LDS reads that follow the staging; the explicit wait keeps that from being a coincidence).
__device__ __forceinline__ void block_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// LDS of the forward and dq kernels: two buffers of two images, then the mask bias of every key (0 / -inf), NKP floats
#define AS_QLDS(NKP) (4 * IMG + (NKP) * 4)
// LDS of the dkv kernel: two buffers of two images, then lse (log2 domain) and delta of every query, NKP floats each
#define AS_KLDS(NKP) (4 * IMG + 2 * (NKP) * 4)

// ================================================================================== forward
__global__ __launch_bounds__(AS_NW * 64) void attn_stream_fwd_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ mask,
                                                                    bf16_t* __restrict__ out, float* __restrict__ lse, int N, int H, int NG) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  const int nkb = (N + SB - 1) / SB, NKP = nkb * SB;
  float* mb = reinterpret_cast<float*>(sm + 4 * IMG);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4;
  const int bh = blockIdx.x / NG, grp = blockIdx.x % NG, b = bh / H, h = bh % H, D = H * 64;
  const long ld = 3 * D;
  const bf16_t* base = qkv + (long)b * N * ld + h * 64;
  const int q0 = (grp * AS_NW + wave) * 16;                    // (a wave whose tile starts past N - 1 computes on row N - 1 and stores nothing)
  bf16x8 qf[2];
  qf[0] = frag_row_global(base, ld, q0, N, 0, lane);
  qf[1] = frag_row_global(base, ld, q0, N, 1, lane);
  stage_block<false>(sm, base + D, ld, N, 0, wave, lane);
  stage_block<true>(sm + IMG, base + 2 * D, ld, N, 0, wave, lane);
  {
    const int* mrow = mask + (long)b * N;
    for (int j = t; j < NKP; j += AS_NW * 64) mb[j] = (j < N && mrow[j] != 0) ? 0.f : -INFINITY;
  }
  float m = -INFINITY, l = 0.f;                                // l: this lane's share of the row sum (the 4 lane groups are added at the end)
  f32x4 O[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) O[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < nkb; ++j) {
    block_sync();                                              // block j has landed; every wave is done with block j - 1
    const char* Kimg = sm + (j & 1) * 2 * IMG;
    const char* Vimg = Kimg + IMG;
    if (j + 1 < nkb) {
      char* nb = sm + ((j + 1) & 1) * 2 * IMG;
      stage_block<false>(nb, base + D, ld, N, (j + 1) * SB, wave, lane);
      stage_block<true>(nb + IMG, base + 2 * D, ld, N, (j + 1) * SB, wave, lane);
    }
    f32x4 S[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      S[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) S[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row_lds(Kimg, kt * 16, s, lane), qf[s], S[kt], 0, 0, 0);
    }
    float bm = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const float4 bias = *reinterpret_cast<const float4*>(mb + j * SB + kt * 16 + 4 * g);
      S[kt][0] = fmaf(S[kt][0], SCALE_L2, bias.x); S[kt][1] = fmaf(S[kt][1], SCALE_L2, bias.y);
      S[kt][2] = fmaf(S[kt][2], SCALE_L2, bias.z); S[kt][3] = fmaf(S[kt][3], SCALE_L2, bias.w);
      bm = fmaxf(bm, fmaxf(fmaxf(S[kt][0], S[kt][1]), fmaxf(S[kt][2], S[kt][3])));
    }
    const float mn = fmaxf(m, group_max(bm));
    const float mu = mn == -INFINITY ? 0.f : mn;               // no valid key so far: every exponent below is -inf, never -inf - -inf
    const float alpha = __builtin_amdgcn_exp2f(m - mu);        // (m = -inf: 0; O and l are still 0 then)
    m = mn;
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) O[dt][r] *= alpha;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { S[kt][r] = __builtin_amdgcn_exp2f(S[kt][r] - mu); l += S[kt][r]; }
    // O^T += V^T P^T: the S^T accumulators are the operand directly (permuted k order, matched by frag_tr32_lds)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8 pa = pack8(S[2 * u], S[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) O[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr32_lds(Vimg, 32 * u, dt, lane), pa, O[dt], 0, 0, 0);
    }
  }
  l = group_sum(l);
  const int q_lane = q0 + (lane & 15);
  if (g == 0 && q_lane < N) lse[(long)bh * NKP + q_lane] = m * LN2 + __logf(l);   // natural-log lse, as the backward expects
  const float linv = 1.0f / l;
  if (q_lane < N) {
    bf16_t* o = out + ((long)b * N + q_lane) * D + h * 64 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store4(o + 16 * dt, O[dt] * linv);
  }
}

// ================================================================================== backward: delta, dQ
__global__ __launch_bounds__(AS_NW * 64) void attn_stream_dq_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ mask,
                                                                   const bf16_t* __restrict__ dout, const bf16_t* __restrict__ out,
                                                                   const float* __restrict__ lse, float* __restrict__ delta,
                                                                   bf16_t* __restrict__ dqkv, int N, int H, int NG) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  const int nkb = (N + SB - 1) / SB, NKP = nkb * SB;
  float* mb = reinterpret_cast<float*>(sm + 4 * IMG);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4;
  const int bh = blockIdx.x / NG, grp = blockIdx.x % NG, b = bh / H, h = bh % H, D = H * 64;
  const long ld = 3 * D;
  const bf16_t* base = qkv + (long)b * N * ld + h * 64;
  const bf16_t* dob = dout + (long)b * N * D + h * 64;
  const bf16_t* ob = out + (long)b * N * D + h * 64;
  const int q0 = (grp * AS_NW + wave) * 16, q_lane = q0 + (lane & 15);
  bf16x8 qf[2], df[2], of[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    qf[s] = frag_row_global(base, ld, q0, N, s, lane);
    df[s] = frag_row_global(dob, D, q0, N, s, lane);
    of[s] = frag_row_global(ob, D, q0, N, s, lane);
  }
  const float L = (q_lane < N ? lse[(long)bh * NKP + q_lane] : INFINITY) * LOG2E;   // +inf for pad rows: P = 0
  stage_block<true>(sm, base + D, ld, N, 0, wave, lane);        // K, transposed-read image (its row fragments by frag_row_ldsT)
  stage_block<false>(sm + IMG, base + 2 * D, ld, N, 0, wave, lane);
  {
    const int* mrow = mask + (long)b * N;
    for (int j = t; j < NKP; j += AS_NW * 64) mb[j] = (j < N && mrow[j] != 0) ? 0.f : -INFINITY;
  }
  float dl = 0.f;                                              // delta = rowsum(dO * O) (= rowsum(P * dP))
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    union { bf16x8 v; uint32_t w[4]; } a, c;
    a.v = df[s];
    c.v = of[s];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dl = fmaf(__uint_as_float(a.w[e] << 16), __uint_as_float(c.w[e] << 16), dl);
      dl = fmaf(__uint_as_float(a.w[e] & 0xffff0000u), __uint_as_float(c.w[e] & 0xffff0000u), dl);
    }
  }
  dl = group_sum(dl);
  if (g == 0 && q_lane < N) delta[(long)bh * NKP + q_lane] = dl;
  f32x4 dQ[4];                                                 // dQ^T = K^T dS^T (swapped operands: 4 adjacent head dims per lane)
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dQ[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < nkb; ++j) {
    block_sync();
    const char* Ktr = sm + (j & 1) * 2 * IMG;
    const char* Vrow = Ktr + IMG;
    if (j + 1 < nkb) {
      char* nb = sm + ((j + 1) & 1) * 2 * IMG;
      stage_block<true>(nb, base + D, ld, N, (j + 1) * SB, wave, lane);
      stage_block<false>(nb + IMG, base + 2 * D, ld, N, (j + 1) * SB, wave, lane);
    }
    f32x4 S[4], dP[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      S[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      dP[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        S[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row_ldsT(Ktr, kt * 16, s, lane), qf[s], S[kt], 0, 0, 0);
        dP[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_row_lds(Vrow, kt * 16, s, lane), df[s], dP[kt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const float4 bias = *reinterpret_cast<const float4*>(mb + j * SB + kt * 16 + 4 * g);
      const float bb[4] = {bias.x, bias.y, bias.z, bias.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(S[kt][r], SCALE_L2, bb[r] - L));
        S[kt][r] = p * (dP[kt][r] - dl) * SCALE;               // dS
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8 sa = pack8(S[2 * u], S[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) dQ[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_tr32_lds(Ktr, 32 * u, dt, lane), sa, dQ[dt], 0, 0, 0);
    }
  }
  if (q_lane < N) {
    bf16_t* o = dqkv + ((long)b * N + q_lane) * ld + h * 64 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) store4(o + 16 * dt, dQ[dt]);
  }
}

// ================================================================================== backward: dK, dV
// wave w owns key tiles grp * 8 + 2 w, + 1: K / V row fragments and the key mask stay in registers, Q / dO stream through LDS
__global__ __launch_bounds__(AS_NW * 64) void attn_stream_dkv_kernel(const bf16_t* __restrict__ qkv, const int* __restrict__ mask,
                                                                    const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                    const float* __restrict__ delta, bf16_t* __restrict__ dqkv,
                                                                    int N, int H, int NG) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  const int nqb = (N + SB - 1) / SB, NKP = nqb * SB;
  float* Ls = reinterpret_cast<float*>(sm + 4 * IMG);          // lse per query, log2 domain (+inf for pad rows)
  float* Ds = Ls + NKP;                                        // delta per query
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4;
  const int bh = blockIdx.x / NG, grp = blockIdx.x % NG, b = bh / H, h = bh % H, D = H * 64;
  const long ld = 3 * D;
  const bf16_t* base = qkv + (long)b * N * ld + h * 64;
  const bf16_t* dob = dout + (long)b * N * D + h * 64;
  const int kt0 = (grp * AS_NW + wave) * AS_TPW;
  bf16x8 kf[AS_TPW][2], vf[AS_TPW][2];
  float mbk[AS_TPW];
  const int* mrow = mask + (long)b * N;
#pragma unroll
  for (int i = 0; i < AS_TPW; ++i) {
    const int key = (kt0 + i) * 16 + (lane & 15);
    mbk[i] = (key < N && mrow[min(key, N - 1)] != 0) ? 0.f : -INFINITY;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      kf[i][s] = frag_row_global(base + D, ld, (kt0 + i) * 16, N, s, lane);
      vf[i][s] = frag_row_global(base + 2 * D, ld, (kt0 + i) * 16, N, s, lane);
    }
  }
  stage_block<true>(sm, base, ld, N, 0, wave, lane);
  stage_block<true>(sm + IMG, dob, D, N, 0, wave, lane);
  for (int j = t; j < NKP; j += AS_NW * 64) {
    Ls[j] = j < N ? lse[(long)bh * NKP + j] * LOG2E : INFINITY;
    Ds[j] = j < N ? delta[(long)bh * NKP + j] : 0.f;
  }
  f32x4 dK[AS_TPW][4], dV[AS_TPW][4];
#pragma unroll
  for (int i = 0; i < AS_TPW; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) { dK[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dV[i][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  for (int j = 0; j < nqb; ++j) {
    block_sync();
    const char* Qtr = sm + (j & 1) * 2 * IMG;
    const char* Dtr = Qtr + IMG;
    if (j + 1 < nqb) {
      char* nb = sm + ((j + 1) & 1) * 2 * IMG;
      stage_block<true>(nb, base, ld, N, (j + 1) * SB, wave, lane);
      stage_block<true>(nb + IMG, dob, D, N, (j + 1) * SB, wave, lane);
    }
#pragma unroll 1
    for (int qt = 0; qt < 4; ++qt) {
      bf16x8 qf[2], df[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        qf[s] = frag_row_ldsT(Qtr, qt * 16, s, lane);
        df[s] = frag_row_ldsT(Dtr, qt * 16, s, lane);
      }
      const float4 L4 = *reinterpret_cast<const float4*>(Ls + j * SB + qt * 16 + 4 * g);
      const float4 D4 = *reinterpret_cast<const float4*>(Ds + j * SB + qt * 16 + 4 * g);
      const float Lr[4] = {L4.x, L4.y, L4.z, L4.w}, Dr[4] = {D4.x, D4.y, D4.z, D4.w};
      s16x4 dot[4], qtr[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dot[dt] = frag_tr16_lds(Dtr, qt * 16, dt, lane);
        qtr[dt] = frag_tr16_lds(Qtr, qt * 16, dt, lane);
      }
#pragma unroll
      for (int i = 0; i < AS_TPW; ++i) {
        f32x4 S = {0.f, 0.f, 0.f, 0.f}, dP = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          S = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf[s], kf[i][s], S, 0, 0, 0);        // S[q = 4g+r][key = lane&15]
          dP = __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[s], vf[i][s], dP, 0, 0, 0);
        }
        f32x4 P, dS;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          P[r] = __builtin_amdgcn_exp2f(fmaf(S[r], SCALE_L2, mbk[i] - Lr[r]));
          dS[r] = P[r] * (dP[r] - Dr[r]) * SCALE;
        }
        const s16x4 pa = pack4(P), sa = pack4(dS);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {                       // swapped operands: dV^T[d = 4g+r][key = lane&15]
          dV[i][dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(dot[dt], pa, dV[i][dt], 0, 0, 0);   // += dO^T P
          dK[i][dt] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(qtr[dt], sa, dK[i][dt], 0, 0, 0);   // += Q^T dS
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < AS_TPW; ++i) {
    const int key = (kt0 + i) * 16 + (lane & 15);
    if (key < N) {
      bf16_t* o = dqkv + ((long)b * N + key) * ld + h * 64 + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        store4(o + D + 16 * dt, dK[i][dt]);
        store4(o + 2 * D + 16 * dt, dV[i][dt]);
      }
    }
  }
}

// ================================================================================== launchers
static inline int as_nkp(int N) { return (N + SB - 1) / SB * SB; }

long rmcl_attn_stream_stat_elems(int B, int H, int N) { return (long)B * H * as_nkp(N); }

int rmcl_attn_stream_fwd(const void* qkv, const int* mask, void* out, float* lse, int B, int N, int H, hipStream_t s) {
  RMCL_REQUIRE(N >= 1 && N <= 512, "streaming attention: N must be in 1..512");
  const int NG = (N + AS_NW * 16 - 1) / (AS_NW * 16);
  const size_t lds = AS_QLDS(as_nkp(N));
  static RmclLdsOnce once;
  RMCL_TRY(rmcl_set_max_lds(once, reinterpret_cast<const void*>(attn_stream_fwd_kernel), AS_QLDS(512)));
  RMCL_LAUNCH(attn_stream_fwd_kernel, dim3(B * H * NG), dim3(AS_NW * 64), lds, s, (const bf16_t*)qkv, mask, (bf16_t*)out, lse, N, H, NG);
  RMCL_CHECK_LAUNCH();
  return 0;
}

int rmcl_attn_stream_bwd(const void* qkv, const int* mask, const void* dout, const void* out, const float* lse, float* delta, void* dqkv,
                         int B, int N, int H, hipStream_t s) {
  RMCL_REQUIRE(N >= 1 && N <= 512, "streaming attention: N must be in 1..512");
  const int NGq = (N + AS_NW * 16 - 1) / (AS_NW * 16), NGk = (N + AS_NW * AS_TPW * 16 - 1) / (AS_NW * AS_TPW * 16);
  const int NKP = as_nkp(N);
  static RmclLdsOnce once1, once2;
  RMCL_TRY(rmcl_set_max_lds(once1, reinterpret_cast<const void*>(attn_stream_dq_kernel), AS_QLDS(512)));
  RMCL_TRY(rmcl_set_max_lds(once2, reinterpret_cast<const void*>(attn_stream_dkv_kernel), AS_KLDS(512)));
  RMCL_LAUNCH(attn_stream_dq_kernel, dim3(B * H * NGq), dim3(AS_NW * 64), (size_t)AS_QLDS(NKP), s, (const bf16_t*)qkv, mask,
              (const bf16_t*)dout, (const bf16_t*)out, lse, delta, (bf16_t*)dqkv, N, H, NGq);
  RMCL_CHECK_LAUNCH();
  RMCL_LAUNCH(attn_stream_dkv_kernel, dim3(B * H * NGk), dim3(AS_NW * 64), (size_t)AS_KLDS(NKP), s, (const bf16_t*)qkv, mask,
              (const bf16_t*)dout, lse, (const float*)delta, (bf16_t*)dqkv, N, H, NGk);
  RMCL_CHECK_LAUNCH();
  return 0;
}
