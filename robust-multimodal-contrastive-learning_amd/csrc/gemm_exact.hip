// Exact-f32 GEMM on the gfx950 f32-input matrix cores (v_mfma_f32_32x32x2_f32).
//
// This is the arithmetic of the fp32 parity path (bit-for-bit a k-ordered fmaf chain per output,
// MI355X guide "FP32-input MFMA") and the any-shape fallback of the bf16 path (bf16 operands are
// widened to f32 when they are staged into LDS).  128x128x16 block tile, 4 waves (2x2), each wave
// 64x64 = 2x2 MFMA tiles of 32x32; LDS images are k-major [16][128+4] f32 so that the one-float
// A/B fragments (lane l: A[i=l&31][k=l>>5], B[k=l>>5][j=l&31]) are conflict-free ds_read_b32.
// Register-staged double buffering: tile t+1 is loaded to VGPRs before the MFMAs of tile t.
#include <type_traits>

#include "rmcl_common.h"
#include "gemm.h"
#include "skinny_select.h"

#define GBM 128
#define GBN 128
#define GBK 16
#define GLD (GBM + 4)

template <typename TI> struct VecTraits;
template <> struct VecTraits<float> { static constexpr int V = 4; };
template <> struct VecTraits<bf16_t> { static constexpr int V = 8; };

// Loads this thread's share (8 elements) of a [128 rows x 16 k] operand tile into f32 registers.
// KC: element (r,k) at base[r*ld + k];  MC: element (r,k) at base[k*ld + r].
template <typename TI, bool KC>
__device__ __forceinline__ void tile_load(float (&reg)[8], const TI* __restrict__ base, long ld, int r0, int R,
                                          int k0, int K, int t) {
  constexpr int V = VecTraits<TI>::V;
  constexpr int NV = 8 / V;  // vectors per thread
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + 256 * i;
    int r, k;
    if (KC) {
      r = v / (GBK / V);
      k = (v % (GBK / V)) * V;
    } else {
      k = v / (GBM / V);
      r = (v % (GBM / V)) * V;
    }
    const bool ok = (r0 + r < R) && (k0 + k < K);
    const TI* p = KC ? base + (long)(r0 + r) * ld + (k0 + k) : base + (long)(k0 + k) * ld + (r0 + r);
    if (ok) {
      if constexpr (V == 4) {
        const float4 x = *reinterpret_cast<const float4*>(p);
        reg[4 * i + 0] = x.x; reg[4 * i + 1] = x.y; reg[4 * i + 2] = x.z; reg[4 * i + 3] = x.w;
      } else {
        const uint4 x = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          reg[2 * j + 0] = __uint_as_float(w[j] << 16);
          reg[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
      }
      // zero the tail of a vector that straddles the end of the contiguous dimension
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const bool in = KC ? (k0 + k + j < K) : (r0 + r + j < R);
        if (!in) reg[V * i + j] = 0.0f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) reg[V * i + j] = 0.0f;
    }
  }
}

template <typename TI, bool KC>
__device__ __forceinline__ void tile_store(const float (&reg)[8], float* __restrict__ S, int t) {
  constexpr int V = VecTraits<TI>::V;
  constexpr int NV = 8 / V;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = t + 256 * i;
    if (KC) {
      const int r = v / (GBK / V), k = (v % (GBK / V)) * V;
#pragma unroll
      for (int j = 0; j < V; ++j) S[(k + j) * GLD + r] = reg[V * i + j];
    } else {
      const int k = v / (GBM / V), r = (v % (GBM / V)) * V;
#pragma unroll
      for (int j = 0; j < V; j += 4)
        *reinterpret_cast<float4*>(&S[k * GLD + r + j]) =
            make_float4(reg[V * i + j], reg[V * i + j + 1], reg[V * i + j + 2], reg[V * i + j + 3]);
    }
  }
}

template <typename TI, typename TO, bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_exact_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float smem[2 * 2 * GBK * GLD];
  float* As = smem;
  float* Bs = smem + 2 * GBK * GLD;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * GBN, m0 = blockIdx.y * GBM;

  const TI* A = reinterpret_cast<const TI*>(g.A);
  const TI* B = reinterpret_cast<const TI*>(g.B);
  TO* C = reinterpret_cast<TO*>(g.C);
  TO* C2 = reinterpret_cast<TO*>(g.C2);
  const char* aux = reinterpret_cast<const char*>(g.aux);
  int kbeg = 0, kend = g.K;
  if (g.splitk > 1) {
    const int per = ((g.K + g.splitk - 1) / g.splitk + GBK - 1) / GBK * GBK;
    kbeg = blockIdx.z * per;
    kend = min(g.K, kbeg + per);
  } else {
    const int b1 = blockIdx.z / g.nb2, b2 = blockIdx.z % g.nb2;
    A += b1 * g.sA1 + b2 * g.sA2;
    B += b1 * g.sB1 + b2 * g.sB2;
    const long co = b1 * g.sC1 + b2 * g.sC2;
    C += co;
    if (C2) C2 += co;
    if (aux) aux += co * ((g.epi & EPI_RESIDUAL) ? sizeof(float) : sizeof(TI));
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  float ra[8], rb[8];
  const int nk = (kend - kbeg + GBK - 1) / GBK;
  if (nk > 0) {
    tile_load<TI, A_KC>(ra, A, g.lda, m0, g.M, kbeg, kend, t);
    tile_load<TI, B_KC>(rb, B, g.ldb, n0, g.N, kbeg, kend, t);
    tile_store<TI, A_KC>(ra, As, t);
    tile_store<TI, B_KC>(rb, Bs, t);
  }
  __syncthreads();
  for (int it = 0; it < nk; ++it) {
    const int cur = it & 1;
    if (it + 1 < nk) {
      tile_load<TI, A_KC>(ra, A, g.lda, m0, g.M, kbeg + (it + 1) * GBK, kend, t);
      tile_load<TI, B_KC>(rb, B, g.ldb, n0, g.N, kbeg + (it + 1) * GBK, kend, t);
    }
    const float* as = As + cur * GBK * GLD + wm * 64 + (lane & 31);
    const float* bs = Bs + cur * GBK * GLD + wn * 64 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < GBK; kk += 2) {
      const int kr = (kk + (lane >> 5)) * GLD;
      const float a0 = as[kr], a1 = as[kr + 32];
      const float b0 = bs[kr], b1 = bs[kr + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (it + 1 < nk) {
      tile_store<TI, A_KC>(ra, As + (cur ^ 1) * GBK * GLD, t);
      tile_store<TI, B_KC>(rb, Bs + (cur ^ 1) * GBK * GLD, t);
    }
    __syncthreads();
  }

  // epilogue.  C/D map of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5).
  // Deliberately NOT skinny_epilogue: this kernel applies the backward dropout mask before GELU' and stashes after both (gemm.h,
  // "Epilogue order"); merging the two orders would change bits of the fp32 parity path.  It also converts types and knows split-K.
  const int epi = g.epi;
  const bool first_slice = (g.splitk <= 1) || (blockIdx.z == 0);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int col = n0 + wn * 64 + j * 32 + (lane & 31);
        if (row < g.M && col < g.N) {
          float v = g.alpha * acc[i][j][r];
          if ((epi & EPI_BIAS) && first_slice) v += g.bias[col];
          const long drow = (long)row * (g.drop_row_mul > 0 ? g.drop_row_mul : 1);
          if (epi & EPI_DROP_BWD) v *= drop_scale(g.drop_seed, (uint32_t)(drow * g.ld_aux + col), g.drop_thresh, g.drop_inv_keep);
          if (epi & EPI_DGELU) v *= gelu_erf_grad(to_f32<TI>(reinterpret_cast<const TI*>(aux)[(long)row * g.ld_aux + col]));
          const long ci = (long)row * g.ldc + col;
          if (epi & EPI_SAVE_PREACT) C2[ci] = from_f32<TO>(v);
          if (epi & EPI_GELU) v = gelu_erf(v);
          if (epi & EPI_TANH) v = tanhf(v);
          if (epi & EPI_DROPOUT) v *= drop_scale(g.drop_seed, (uint32_t)(drow * g.ldc + col), g.drop_thresh, g.drop_inv_keep);
          if (epi & EPI_RESIDUAL) v += reinterpret_cast<const float*>(aux)[(long)row * g.ld_aux + col];
          if (epi & EPI_ATOMIC) {
            if constexpr (sizeof(TO) == 4) atomicAdd(reinterpret_cast<float*>(C) + ci, v);
          } else if (epi & EPI_ACCUM) {
            C[ci] = from_f32<TO>(to_f32<TO>(C[ci]) + v);
          } else {
            C[ci] = from_f32<TO>(v);
          }
        }
      }
}

template <typename TI, typename TO>
static int launch_layout(const GemmArgs& g, int a_kc, int b_kc, dim3 grid, hipStream_t s) {
  if (a_kc && b_kc) RMCL_LAUNCH((gemm_exact_kernel<TI, TO, true, true>), grid, dim3(256), 0, s, g);
  else if (a_kc && !b_kc) RMCL_LAUNCH((gemm_exact_kernel<TI, TO, true, false>), grid, dim3(256), 0, s, g);
  else if (!a_kc && !b_kc) RMCL_LAUNCH((gemm_exact_kernel<TI, TO, false, false>), grid, dim3(256), 0, s, g);
  else RMCL_LAUNCH((gemm_exact_kernel<TI, TO, false, true>), grid, dim3(256), 0, s, g);
  RMCL_CHECK_LAUNCH();
  return 0;
}

bool rmcl_gemm_skinny_supported(const GemmArgs& g, int dt_in, int dt_out, int a_kc);
int rmcl_launch_gemm_skinny(const GemmArgs& g, int b_kc, hipStream_t s);
bool rmcl_gemm_skinny_streams(const GemmArgs& g, int b_kc);
extern int g_gemm_share;            // gemm_fast.hip, rmcl_tune_set key 10: chains sharing the chip
// rmcl_tune_set key 6: 0 = the first forms only (row-split skinny kernel, LDS-staged TN kernel); 1 = the k-split skinny kernel (the
// streaming form's A/B arm and bitwise reference); -1 (default) or 2 = the streaming k-split form wherever the k-split form ran 16-column tiles
static int g_skinny_form = -1;

// Outer-product-like fp32 GEMM: C[M, N] (+)= alpha * A^T B with A [K, M], B [K, N] and a SHORT reduction (K = the batch rows:
// the weight gradients of the heads, of the encoder's cls-only tail and of the Barlow-Twins head, and its cross-correlation
// matrix).  The 128x128x16 LDS-staged kernel above spends its time in four barrier-separated k-tiles for 64 k; here every
// wave owns a 64 x 64 output tile and streams both operands straight from L2 (lane (c, g) of a 16x16x4 MFMA reads A[k0+g][m0+c]
// and B[k0+g][n0+c]: 64-byte rows), 16 MFMAs per 8 loads, no LDS, no barrier.
__global__ __launch_bounds__(256) void gemm_tn_shortk_kernel(GemmArgs g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, gq = lane >> 4;
  const int m0 = blockIdx.y * 128 + (wave >> 1) * 64, n0 = blockIdx.x * 128 + (wave & 1) * 64;
  if (m0 >= g.M || n0 >= g.N) return;
  const float* A = reinterpret_cast<const float*>(g.A);
  const float* B = reinterpret_cast<const float*>(g.B);
  int am[4], bn[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    am[t] = min(m0 + t * 16 + c, g.M - 1);
    bn[t] = min(n0 + t * 16 + c, g.N - 1);
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // EPI_COLSUM: column sums of A over k (= the bias gradient that goes with this weight gradient) as a by-product of the operand
  // loads, written by the waves of the first column block (n0 == 0: one writer per column m) - no separate column-sum launch
  const bool want_cs = (g.epi & EPI_COLSUM) && n0 == 0;
  float sa[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < g.K; k0 += 8) {                    // two 4-k steps per trip, all 16 loads in flight before the MFMAs
    float a[2][4], b[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int k = min(k0 + 4 * u + gq, g.K - 1);
      const bool live = k0 + 4 * u + gq < g.K;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a[u][t] = live ? A[(long)k * g.lda + am[t]] : 0.f;
        b[u][t] = live ? B[(long)k * g.ldb + bn[t]] : 0.f;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], b[u][j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) sa[t] += a[0][t] + a[1][t];     // (rows past K were loaded as 0)
  }
  if (want_cs) {                                             // lane (c, gq) holds the rows k = gq (mod 4): sum over the four lane groups
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float v = sa[t];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int m = m0 + t * 16 + c;
      if (gq == 0 && m < g.M) g.colsum[m] += v;
    }
  }
  float* C = reinterpret_cast<float*>(g.C);
  // The tail is alpha * acc + old C and nothing else (one fma; rmcl_gemm_tn_shortk_takes admits no other flag), so it stays literal.
  // C += : every old value of the tile is loaded BEFORE the first store.  "load, add, store" per element cannot be reordered by the
  // compiler (the stores may alias the next loads for all it knows) and ran as 64 serial round trips per lane (tools/st_trace.py
  // found the same pattern in the weight-gradient launch's epilogue)
  float oldc[4][4][4];
  const bool accum = (g.epi & EPI_ACCUM) != 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + i * 16 + 4 * gq + r, col = n0 + j * 16 + c;
        oldc[i][j][r] = (accum && row < g.M && col < g.N) ? C[(long)row * g.ldc + col] : 0.f;
      }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + i * 16 + 4 * gq + r, col = n0 + j * 16 + c;
        if (row < g.M && col < g.N) C[(long)row * g.ldc + col] = g.alpha * acc[i][j][r] + oldc[i][j][r];
      }
}

// true when rmcl_launch_gemm_exact(g, f32, f32, a_kc = 0, b_kc = 0) runs the short-K kernel, the only one that knows EPI_COLSUM
bool rmcl_gemm_tn_shortk_takes(const GemmArgs& g) {
  return g.A && g.B && g.C && g.M > 0 && g.N > 0 && g.K >= 1 && g.K <= 256 && g.splitk <= 1 && g.nb1 * g.nb2 == 1 &&
         (g.epi & ~(EPI_ACCUM | EPI_COLSUM)) == 0 && g_skinny_form != 0;
}

int rmcl_launch_gemm_exact(const GemmArgs& g, int dt_in, int dt_out, int a_kc, int b_kc, hipStream_t s) {
  RMCL_REQUIRE(!g.a_bf16 || (a_kc && dt_in == RMCL_F32 && dt_out == RMCL_F32 && g.M > 0 && g.N > 0 && rmcl_gemm_skinny_streams(g, b_kc)),
               "gemm: a bf16 A operand beside fp32 weights is the streaming skinny kernel's alone (rmcl_tune_set key 6; K % 64 == 0, 128 <= K < 2048, N < 4096, weights [N][K])");
  if (g.A && g.B && g.C && g.M > 0 && g.N > 0 && rmcl_gemm_skinny_supported(g, dt_in, dt_out, a_kc)) return rmcl_launch_gemm_skinny(g, b_kc, s);
  if (!a_kc && !b_kc && dt_in == RMCL_F32 && dt_out == RMCL_F32 && (!(g.epi & EPI_COLSUM) || g.colsum) && rmcl_gemm_tn_shortk_takes(g)) {
    RMCL_LAUNCH(gemm_tn_shortk_kernel, dim3(cdiv(g.N, 128), cdiv(g.M, 128)), dim3(256), 0, s, g);
    RMCL_CHECK_LAUNCH();
    return 0;
  }
  const int V = dt_in == RMCL_F32 ? 4 : 8;
  RMCL_REQUIRE(g.M > 0 && g.N > 0 && g.K >= 0, "gemm: bad dims");
  RMCL_REQUIRE(g.lda % V == 0 && g.ldb % V == 0, "gemm: lda/ldb must be a multiple of the 16-byte vector width");
  // a vector may straddle the end of the contiguous dimension only if the row pitch covers it
  const int Kr = (g.K + V - 1) / V * V, Mr = (g.M + V - 1) / V * V, Nr = (g.N + V - 1) / V * V;
  RMCL_REQUIRE(a_kc ? (g.lda >= Kr) : (g.lda >= Mr), "gemm: lda too small for vector loads");
  RMCL_REQUIRE(b_kc ? (g.ldb >= Kr) : (g.ldb >= Nr), "gemm: ldb too small for vector loads");
  RMCL_REQUIRE(((uintptr_t)g.A & 15) == 0 && ((uintptr_t)g.B & 15) == 0, "gemm: A/B must be 16-byte aligned");
  RMCL_REQUIRE(!(g.epi & EPI_ATOMIC) || dt_out == RMCL_F32, "gemm: atomic epilogue needs fp32 C");
  RMCL_REQUIRE(g.splitk <= 1 || ((g.epi & EPI_ATOMIC) && g.nb1 * g.nb2 == 1), "gemm: split-K needs EPI_ATOMIC and no batching");
  const int z = g.splitk > 1 ? g.splitk : g.nb1 * g.nb2;
  RMCL_REQUIRE(z >= 1 && z <= 65535, "gemm: bad batch count");
  dim3 grid(cdiv(g.N, GBN), cdiv(g.M, GBM), z);
  if (dt_in == RMCL_F32 && dt_out == RMCL_F32) return launch_layout<float, float>(g, a_kc, b_kc, grid, s);
  if (dt_in == RMCL_BF16 && dt_out == RMCL_BF16) return launch_layout<bf16_t, bf16_t>(g, a_kc, b_kc, grid, s);
  if (dt_in == RMCL_BF16 && dt_out == RMCL_F32) return launch_layout<bf16_t, float>(g, a_kc, b_kc, grid, s);
  if (dt_in == RMCL_F32 && dt_out == RMCL_BF16) return launch_layout<float, bf16_t>(g, a_kc, b_kc, grid, s);
  rmcl_set_error("gemm: unsupported dtype combination");
  return -1;
}

// ---------------------------------------------------------------------------------------------------
// The element-wise tail of the skinny kernels below, written once (row-split and k-split kernel; the streaming kernel carries a literal
// copy of it and of skinny_reduce_store, for a measured reason given there).  Order (gemm.h, "Epilogue order"): alpha, bias, stash to C2,
// GELU, tanh, GELU'(aux), backward dropout mask, forward dropout mask, residual, accumulate, store, second copy.
// `ops` is the OPERAND SOURCE: bias() / aux() / oldc() of this element.  Where the operands come from is not cosmetic under
// -ffp-contract=fast: handed preloaded registers, the row-split kernel's `alpha * acc + bias` is if-converted and fused into an fma
// (other bits); loading at the point of use keeps its branches, and with them its mul and its add.  So the row-split kernel passes
// SkinnyOpsAtUse and the k-split forms, which must preload (skinny_reduce_store), pass SkinnyOpsLoaded.
// ---------------------------------------------------------------------------------------------------
struct SkinnyOpsAtUse {
  const GemmArgs& g;
  int row, n;
  __device__ __forceinline__ float bias() const { return g.bias[n]; }
  __device__ __forceinline__ float aux() const { return reinterpret_cast<const float*>(g.aux)[(long)row * g.ld_aux + n]; }
  __device__ __forceinline__ float oldc() const { return reinterpret_cast<const float*>(g.C)[(long)row * g.ldc + n]; }
};
struct SkinnyOpsLoaded {
  float b, a, o;
  __device__ __forceinline__ float bias() const { return b; }
  __device__ __forceinline__ float aux() const { return a; }
  __device__ __forceinline__ float oldc() const { return o; }
};

// v = the k-sum of element (row, n), row < M and n < N
template <typename Ops>
__device__ __forceinline__ void skinny_epilogue(const GemmArgs& g, float v, int row, int n, const Ops& ops) {
  float* C = reinterpret_cast<float*>(g.C);
  v *= g.alpha;
  if (g.epi & EPI_BIAS) v += ops.bias();
  const long ci = (long)row * g.ldc + n;
  if (g.epi & EPI_SAVE_PREACT) reinterpret_cast<float*>(g.C2)[ci] = v;
  if (g.epi & EPI_GELU) v = gelu_erf(v);
  if (g.epi & EPI_TANH) v = tanhf(v);
  if (g.epi & EPI_DGELU) v *= gelu_erf_grad(ops.aux());
  const long drow = (long)row * (g.drop_row_mul > 0 ? g.drop_row_mul : 1);                           // dense row of this compact row (gemm.h)
  if (g.epi & EPI_DROP_BWD) v *= drop_scale(g.drop_seed, (uint32_t)(drow * g.ld_aux + n), g.drop_thresh, g.drop_inv_keep);
  if (g.epi & EPI_DROPOUT) v *= drop_scale(g.drop_seed, (uint32_t)(drow * g.ldc + n), g.drop_thresh, g.drop_inv_keep);
  if (g.epi & EPI_RESIDUAL) v += ops.aux();
  if (g.epi & EPI_ACCUM) v += ops.oldc();
  C[ci] = v;
  if (g.epi & EPI_DUP) reinterpret_cast<float*>(g.C2)[ci] = v;
}

// Second half of the k-split kernel (and, as a literal copy, of the streaming kernel): the NW partial tiles of ROWS x NT elements lie in
// LDS (after the barrier); every thread sums its elements over the waves in k order and applies the tail.
template <int NW, int ROWS, int NT>
__device__ __forceinline__ void skinny_reduce_store(const GemmArgs& g, const float (&red)[NW][ROWS][NT + 1], int m0, int n0) {
  // every global operand of the epilogue (bias, aux, old C) is loaded for ALL of the thread's elements before the first store: in
  // "load, compute, store" order per element the loads of element i + 1 cannot pass the store of element i (possible alias)
  constexpr int ELEMS = ROWS * NT, THREADS = 64 * NW, ITER = (ELEMS + THREADS - 1) / THREADS;
  constexpr bool FULL = ELEMS % THREADS == 0;                  // no thread runs past the tile: the guard compiles out
  float bia[ITER], aux[ITER], oldc[ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int i = threadIdx.x + it * THREADS, rl = i / NT, cl = i % NT, row = m0 + rl, n = n0 + cl;
    const bool live = (FULL || i < ELEMS) && row < g.M && n < g.N;
    bia[it] = (live && (g.epi & EPI_BIAS)) ? g.bias[n] : 0.f;
    aux[it] = (live && (g.epi & (EPI_DGELU | EPI_RESIDUAL))) ? reinterpret_cast<const float*>(g.aux)[(long)row * g.ld_aux + n] : 0.f;
    oldc[it] = (live && (g.epi & EPI_ACCUM)) ? reinterpret_cast<const float*>(g.C)[(long)row * g.ldc + n] : 0.f;
  }
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int i = threadIdx.x + it * THREADS, rl = i / NT, cl = i % NT, row = m0 + rl, n = n0 + cl;
    if ((!FULL && i >= ELEMS) || row >= g.M || n >= g.N) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[w][rl][cl];                                              // k order: wave 0 .. NW-1
    skinny_epilogue(g, v, row, n, SkinnyOpsLoaded{bia[it], aux[it], oldc[it]});
  }
}

// ---------------------------------------------------------------------------------------------------
// Skinny exact-f32 GEMM for the heads (pooler / MoCo head / ITM): M <= 64 rows per block, K long.
// The 128x128 kernel above would run such a problem on N/128 = 6 workgroups, latency-bound at
// ~120 us; here every workgroup owns 64 rows x 16 columns (N/16 workgroups), each wave one 16x16
// MFMA tile (v_mfma_f32_16x16x4_f32), operands streamed straight from L2 with 16-byte loads, no LDS.
// k order inside a 16-wide chunk is permuted (lane group g, element j <-> k = 16c + 4g + j) on both
// operands, so one float4 per lane feeds four MFMAs.
// ---------------------------------------------------------------------------------------------------
template <bool B_KC>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(GemmArgs g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gq = lane >> 4;
  const int m = blockIdx.y * 64 + wave * 16 + (lane & 15), n = blockIdx.x * 16 + (lane & 15);
  const float* A = reinterpret_cast<const float*>(g.A) + (long)min(m, g.M - 1) * g.lda + 4 * gq;
  const float* B = reinterpret_cast<const float*>(g.B);
  const int nc = min(n, g.N - 1);
  B += B_KC ? (long)nc * g.ldb + 4 * gq : (long)(4 * gq) * g.ldb + nc;
  // four independent accumulator chains (the 16x16x4 MFMA is 8 passes deep: one chain would serialise on its own latency)
  // and 8 k-steps of loads in flight; the chains are summed in k order at the end.  NOTE: this changes the summation
  // order relative to a single chain only in the last bits (heads: fp32, tolerance 1e-5).
  f32x4 ac[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  // 64 k per iteration with every load of the iteration issued before the first MFMA (the compiler otherwise waits
  // vmcnt(0) after each scalar B load: four serial L2 round trips per 16 k); 16-k tail for K % 64
  int k0 = 0;
  for (; k0 + 64 <= g.K; k0 += 64) {
    float4 av[4];
    float bv[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = *reinterpret_cast<const float4*>(A + k0 + 16 * u);
      if (B_KC) {
        const float4 t = *reinterpret_cast<const float4*>(B + k0 + 16 * u);
        bv[u][0] = t.x; bv[u][1] = t.y; bv[u][2] = t.z; bv[u][3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[u][j] = B[(long)(k0 + 16 * u + j) * g.ldb];
      }
    }
    __builtin_amdgcn_sched_barrier(0);                       // all 20 loads are in flight before the first MFMA waits
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ac[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].x, bv[u][0], ac[0], 0, 0, 0);
      ac[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].y, bv[u][1], ac[1], 0, 0, 0);
      ac[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].z, bv[u][2], ac[2], 0, 0, 0);
      ac[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u].w, bv[u][3], ac[3], 0, 0, 0);
    }
  }
  for (; k0 < g.K; k0 += 16) {
    const float4 a = *reinterpret_cast<const float4*>(A + k0);
    float b[4];
    if (B_KC) {
      const float4 t = *reinterpret_cast<const float4*>(B + k0);
      b[0] = t.x; b[1] = t.y; b[2] = t.z; b[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = B[(long)(k0 + j) * g.ldb];
    }
    ac[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[0], ac[0], 0, 0, 0);
    ac[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[1], ac[1], 0, 0, 0);
    ac[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[2], ac[2], 0, 0, 0);
    ac[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[3], ac[3], 0, 0, 0);
  }
  f32x4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = (ac[0][r] + ac[1][r]) + (ac[2][r] + ac[3][r]);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = blockIdx.y * 64 + wave * 16 + 4 * gq + r;
    if (row < g.M && n < g.N) skinny_epilogue(g, acc[r], row, n, SkinnyOpsAtUse{g, row, n});
  }
}

// Second form of the skinny GEMM: the four waves of a workgroup split K instead of the rows.  Every wave covers all 64 rows
// (4 row tiles) x NT columns over its quarter of K, so a B fragment feeds 4 (x NT/16) MFMAs instead of 1, the serial k-loop
// of a workgroup is 4x shorter (N = 768, K = 3072: 48 workgroups were looping 3072 deep), and the partial tiles meet in LDS
// where the epilogue runs.  NT = 32 halves the re-reads of the A panel for very wide outputs (Barlow-Twins head, N = 8192).
// Same operand trick as above: lane (c, g) holds k = 16 s + 4 g + j in component j of one float4, on both operands.
template <bool B_KC, int NT, int NW>
__global__ __launch_bounds__(64 * NW) void gemm_skinny_ksplit_kernel(GemmArgs g) {
  constexpr int CT = NT / 16;
  __shared__ float red[NW][64][NT + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, gq = lane >> 4;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * NT;
  const int kq = g.K / NW, k_lo = wave * kq;                               // kq % 16 == 0 (launcher)
  const float* Ap[4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) Ap[rt] = reinterpret_cast<const float*>(g.A) + (long)min(m0 + rt * 16 + c, g.M - 1) * g.lda + 4 * gq;
  const float* Bp[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int nc = min(n0 + ct * 16 + c, g.N - 1);
    Bp[ct] = reinterpret_cast<const float*>(g.B) + (B_KC ? (long)nc * g.ldb + 4 * gq : (long)(4 * gq) * g.ldb + nc);
  }
  f32x4 acc[4][CT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  // register ring over 16-k steps, PD - 1 steps of loads in flight ahead of the MFMAs: the waves are few and every step is an L2 /
  // HBM round trip (64-byte row pieces of A), so with one step of lookahead the k-loop was a chain of 12 - 24 such round trips
  // (K = 3072, 8 waves: 41.8 us for 9 MB of weights).  The ring index is a compile-time constant (PD steps per trip).
  constexpr int PD = 4;                                       // (round 4: 8 steps of lookahead measured SLOWER in the step: 33.9 vs 33.6 ms, three alternating runs)
  float4 av[PD][4];
  float bv[PD][CT][4];
  auto load = [&](int buf, int k) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) av[buf][rt] = *reinterpret_cast<const float4*>(Ap[rt] + k);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      if (B_KC) {
        const float4 t = *reinterpret_cast<const float4*>(Bp[ct] + k);
        bv[buf][ct][0] = t.x; bv[buf][ct][1] = t.y; bv[buf][ct][2] = t.z; bv[buf][ct][3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[buf][ct][j] = Bp[ct][(long)(k + j) * g.ldb];
      }
    }
  };
  auto mac = [&](int buf) {
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[buf][rt].x, bv[buf][ct][0], acc[rt][ct], 0, 0, 0);
        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[buf][rt].y, bv[buf][ct][1], acc[rt][ct], 0, 0, 0);
        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[buf][rt].z, bv[buf][ct][2], acc[rt][ct], 0, 0, 0);
        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[buf][rt].w, bv[buf][ct][3], acc[rt][ct], 0, 0, 0);
      }
  };
  const int nsteps = kq / 16;
#pragma unroll
  for (int i = 0; i < PD - 1; ++i)
    if (i < nsteps) load(i, k_lo + 16 * i);
  for (int s0 = 0; s0 < nsteps; s0 += PD) {
#pragma unroll
    for (int j = 0; j < PD; ++j) {
      const int step = s0 + j;
      if (step < nsteps) {
        if (step + PD - 1 < nsteps) load((j + PD - 1) % PD, k_lo + 16 * (step + PD - 1));
        __builtin_amdgcn_sched_barrier(0);
        mac(j);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][rt * 16 + 4 * gq + r][ct * 16 + c] = acc[rt][ct][r];
  __syncthreads();
  skinny_reduce_store<NW, 64, NT>(g, red, m0, n0);
}

// Third form: the k-split kernel above with its loads re-timed and its rows cut to what the problem has.  The ARITHMETIC is the
// k-split kernel's, element for element (same K / NW chunk per wave, same 16-k steps, the same four MFMAs per step in x, y, z, w
// order on one accumulator, the same LDS sum over waves 0 .. NW-1, the same epilogue expressions), so the two forms agree bit for bit.
//   * Weights first.  The weights are cold on every pass (26 MB of fp32, evicted by the dense traffic between uses) while the A panel
//     was written by the previous launch; in the k-split kernel's ring both wait in one queue, 3 steps deep, and a wave's chunk is a
//     chain of 4 - 8 HBM round trips.  Here a wave issues the weight loads of a whole burst (skinny_select.h: 12 or 24 steps, i.e.
//     the whole chunk at the step's shapes) before its first MFMA, and only A keeps a ring (rmcl_skinny_a_ring steps).  Every burst
//     is straight-line code: all register indices and all waits (counted vmcnt) are the compiler's, none depends on a run-time trip.
//   * RT row tiles of 16 per workgroup instead of always 4: the launcher picks RT so that no workgroup covers a tile that begins
//     beyond M (the k-split kernel loads and multiplies min(m, M - 1) duplicates there) and so that launches with few column tiles
//     still fill the chain's part of the chip.  Per-element arithmetic does not depend on RT.
//   * A16: A holds bf16 (row stride lda in bf16 elements), widened in registers - exact, so the bits are those of a gather-and-cast
//     launch followed by the fp32 form (the cls-only tail's proj reads the attention output's cls rows in place).
template <bool B_KC, int NW, int RT, int BS, bool A16>
__global__ __launch_bounds__(64 * NW) void gemm_skinny_stream_kernel(GemmArgs g) {
  constexpr int ROWS = 16 * RT, AD = rmcl_skinny_a_ring(B_KC, RT);
  __shared__ float red[NW][ROWS][17];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), c = lane & 15, gq = lane >> 4;
  const int m0 = blockIdx.y * ROWS, n0 = blockIdx.x * 16;
  const int kq = g.K / NW, k_lo = wave * kq;                               // kq % 16 == 0 (launcher)
  const float* Ap[RT];
  const bf16_t* Ah[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const long off = (long)min(m0 + rt * 16 + c, g.M - 1) * g.lda + 4 * gq;
    Ap[rt] = reinterpret_cast<const float*>(g.A) + off;
    Ah[rt] = reinterpret_cast<const bf16_t*>(g.A) + off;
  }
  const int nc = min(n0 + c, g.N - 1);
  const float* Bp = reinterpret_cast<const float*>(g.B) + (B_KC ? (long)nc * g.ldb + 4 * gq : (long)(4 * gq) * g.ldb + nc);
  f32x4 acc[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // one burst of n steps from k: every weight load, then AD steps of A, then per step {A of step + AD; the step's MFMAs}
  auto burst = [&](auto nc_, int k) {
    constexpr int n = decltype(nc_)::value;
    float bv[n][4];
    float4 av[n][RT];
#pragma unroll
    for (int i = 0; i < n; ++i) {
      if (B_KC) {
        const float4 t = *reinterpret_cast<const float4*>(Bp + k + 16 * i);
        bv[i][0] = t.x; bv[i][1] = t.y; bv[i][2] = t.z; bv[i][3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[i][j] = Bp[(long)(k + 16 * i + j) * g.ldb];
      }
    }
    auto load_a = [&](int i) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        if (A16) {
          const f32x4 t = bf2f4(*reinterpret_cast<const uint2*>(Ah[rt] + k + 16 * i));
          av[i][rt] = make_float4(t.x, t.y, t.z, t.w);
        } else {
          av[i][rt] = *reinterpret_cast<const float4*>(Ap[rt] + k + 16 * i);
        }
      }
    };
#pragma unroll
    for (int i = 0; i < AD; ++i)
      if (i < n) load_a(i);
#pragma unroll
    for (int i = 0; i < n; ++i) {
      if (i + AD < n) load_a(i + AD);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][rt].x, bv[i][0], acc[rt], 0, 0, 0);
        acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][rt].y, bv[i][1], acc[rt], 0, 0, 0);
        acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][rt].z, bv[i][2], acc[rt], 0, 0, 0);
        acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][rt].w, bv[i][3], acc[rt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  const SkinnyBursts nb = rmcl_skinny_bursts(kq / 16, BS);
  int k = k_lo;
  for (int b = 0; b < nb.full; ++b, k += 16 * BS) burst(std::integral_constant<int, BS>{}, k);
  if constexpr (BS > 12) {
    if (nb.mid) { burst(std::integral_constant<int, 12>{}, k); k += 16 * 12; }
  }
  for (int b = 0; b < nb.quad; ++b, k += 64) burst(std::integral_constant<int, 4>{}, k);
  for (int b = 0; b < nb.single; ++b, k += 16) burst(std::integral_constant<int, 1>{}, k);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][rt * 16 + 4 * gq + r][c] = acc[rt][r];
  __syncthreads();
  float* C = reinterpret_cast<float*>(g.C);
  // skinny_reduce_store + skinny_epilogue, expression for expression, but LITERAL: behind the helper every instantiation kept its
  // floating-point instructions and gave the same bits, yet the compiler laid the tail's blocks out differently and the [K][N]
  // instantiations measured 0.1 - 0.3 us (1 - 2 %) slower per launch than the parent's run-to-run spread (DESIGN "GEMM epilogues").  A
  // change to either copy goes into both; tests/test_gemm_skinny_stream_gpu.py and tests/test_encoder_skinny_stream_gpu.py (dropout
  // tails) hold them to each other bit for bit.  ROWS x 16 elements over 64 * NW threads, every global operand loaded for all of the
  // thread's elements before the first store
  constexpr int ELEMS = ROWS * 16, THREADS = 64 * NW, ITER = (ELEMS + THREADS - 1) / THREADS;
  float bia[ITER], aux[ITER], oldc[ITER];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int i = threadIdx.x + it * THREADS, rl = i / 16, cl = i % 16, row = m0 + rl, n = n0 + cl;
    const bool live = i < ELEMS && row < g.M && n < g.N;
    bia[it] = (live && (g.epi & EPI_BIAS)) ? g.bias[n] : 0.f;
    aux[it] = (live && (g.epi & (EPI_DGELU | EPI_RESIDUAL))) ? reinterpret_cast<const float*>(g.aux)[(long)row * g.ld_aux + n] : 0.f;
    oldc[it] = (live && (g.epi & EPI_ACCUM)) ? C[(long)row * g.ldc + n] : 0.f;
  }
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int i = threadIdx.x + it * THREADS, rl = i / 16, cl = i % 16, row = m0 + rl, n = n0 + cl;
    if (i >= ELEMS || row >= g.M || n >= g.N) continue;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[w][rl][cl];                                              // k order: wave 0 .. NW-1
    v *= g.alpha;
    if (g.epi & EPI_BIAS) v += bia[it];
    const long ci = (long)row * g.ldc + n;
    if (g.epi & EPI_SAVE_PREACT) reinterpret_cast<float*>(g.C2)[ci] = v;
    if (g.epi & EPI_GELU) v = gelu_erf(v);
    if (g.epi & EPI_TANH) v = tanhf(v);
    if (g.epi & EPI_DGELU) v *= gelu_erf_grad(aux[it]);
    const long drow = (long)row * (g.drop_row_mul > 0 ? g.drop_row_mul : 1);                         // dense row of this compact row (gemm.h)
    if (g.epi & EPI_DROP_BWD) v *= drop_scale(g.drop_seed, (uint32_t)(drow * g.ld_aux + n), g.drop_thresh, g.drop_inv_keep);
    if (g.epi & EPI_DROPOUT) v *= drop_scale(g.drop_seed, (uint32_t)(drow * g.ldc + n), g.drop_thresh, g.drop_inv_keep);
    if (g.epi & EPI_RESIDUAL) v += aux[it];
    if (g.epi & EPI_ACCUM) v += oldc[it];
    C[ci] = v;
    if (g.epi & EPI_DUP) reinterpret_cast<float*>(g.C2)[ci] = v;
  }
}

bool rmcl_gemm_skinny_supported(const GemmArgs& g, int dt_in, int dt_out, int a_kc) {
  return a_kc && dt_in == RMCL_F32 && dt_out == RMCL_F32 && g.M <= 1024 && g.K % 16 == 0 && g.K >= 64 && g.splitk <= 1 &&
         g.nb1 * g.nb2 == 1 && (g.epi & ~(EPI_BIAS | EPI_TANH | EPI_ACCUM | EPI_GELU | EPI_SAVE_PREACT | EPI_DGELU | EPI_RESIDUAL | EPI_DUP | EPI_DROPOUT | EPI_DROP_BWD)) == 0 &&
         (!(g.epi & EPI_DROP_BWD) || (g.epi & EPI_DGELU)) &&
         !((g.epi & EPI_DUP) && (g.epi & EPI_SAVE_PREACT)) &&
         !((g.epi & EPI_DGELU) && (g.epi & EPI_RESIDUAL)) && g.lda % 4 == 0 && g.ldb % 4 == 0 &&
         ((uintptr_t)g.A & 15) == 0 && ((uintptr_t)g.B & 15) == 0;
}

void rmcl_gemm_skinny_set_form(int v) { g_skinny_form = v; }

// true when rmcl_launch_gemm_exact(g, f32, f32, a_kc = 1, b_kc) runs the streaming form - the only one that takes GemmArgs.a_bf16
bool rmcl_gemm_skinny_streams(const GemmArgs& g, int b_kc) {
  return g.A && g.B && g.C && g_skinny_form != 0 && g_skinny_form != 1 && rmcl_gemm_skinny_supported(g, RMCL_F32, RMCL_F32, 1) &&
         rmcl_skinny_plan(g.M, g.N, g.K, b_kc != 0, g_gemm_share).ok && (!g.a_bf16 || (b_kc && g.K < 2048));
}

template <bool B_KC, int NW, int BS, bool A16>
static void launch_skinny_stream(const GemmArgs& g, const SkinnyPlan& p, hipStream_t s) {
  const dim3 grid(p.grid_x, p.grid_y), block(64 * NW);
  if (p.rt == 4) RMCL_LAUNCH((gemm_skinny_stream_kernel<B_KC, NW, 4, BS, A16>), grid, block, 0, s, g);
  else if (p.rt == 2) RMCL_LAUNCH((gemm_skinny_stream_kernel<B_KC, NW, 2, BS, A16>), grid, block, 0, s, g);
  else RMCL_LAUNCH((gemm_skinny_stream_kernel<B_KC, NW, 1, BS, A16>), grid, block, 0, s, g);
}

int rmcl_launch_gemm_skinny(const GemmArgs& g, int b_kc, hipStream_t s) {
  if (rmcl_gemm_skinny_streams(g, b_kc)) {
    const SkinnyPlan p = rmcl_skinny_plan(g.M, g.N, g.K, b_kc != 0, g_gemm_share);
    if (g.a_bf16) launch_skinny_stream<true, 4, rmcl_skinny_burst_len(true, 4), true>(g, p, s);
    else if (b_kc && p.nw == 8) launch_skinny_stream<true, 8, rmcl_skinny_burst_len(true, 8), false>(g, p, s);
    else if (b_kc) launch_skinny_stream<true, 4, rmcl_skinny_burst_len(true, 4), false>(g, p, s);
    else if (p.nw == 8) launch_skinny_stream<false, 8, rmcl_skinny_burst_len(false, 8), false>(g, p, s);
    else launch_skinny_stream<false, 4, rmcl_skinny_burst_len(false, 4), false>(g, p, s);
    RMCL_CHECK_LAUNCH();
    return 0;
  }
  const SkinnyKsplitPlan kp = rmcl_skinny_ksplit_plan(g.M, g.N, g.K);
  if (g_skinny_form != 0 && kp.ok) {
    const dim3 grid(kp.grid_x, kp.grid_y), block(64 * kp.nw);
    if (kp.nt == 32) {
      if (b_kc) RMCL_LAUNCH((gemm_skinny_ksplit_kernel<true, 32, 4>), grid, block, 0, s, g);
      else RMCL_LAUNCH((gemm_skinny_ksplit_kernel<false, 32, 4>), grid, block, 0, s, g);
    } else if (kp.nw == 8) {
      if (b_kc) RMCL_LAUNCH((gemm_skinny_ksplit_kernel<true, 16, 8>), grid, block, 0, s, g);
      else RMCL_LAUNCH((gemm_skinny_ksplit_kernel<false, 16, 8>), grid, block, 0, s, g);
    } else {
      if (b_kc) RMCL_LAUNCH((gemm_skinny_ksplit_kernel<true, 16, 4>), grid, block, 0, s, g);
      else RMCL_LAUNCH((gemm_skinny_ksplit_kernel<false, 16, 4>), grid, block, 0, s, g);
    }
    RMCL_CHECK_LAUNCH();
    return 0;
  }
  dim3 grid(cdiv(g.N, 16), cdiv(g.M, 64));
  if (b_kc) RMCL_LAUNCH(gemm_skinny_kernel<true>, grid, dim3(256), 0, s, g);
  else RMCL_LAUNCH(gemm_skinny_kernel<false>, grid, dim3(256), 0, s, g);
  RMCL_CHECK_LAUNCH();
  return 0;
}
