// Host-side selection of the k-split skinny GEMMs (gemm_exact.hip, gemm_skinny_ksplit_kernel and gemm_skinny_stream_kernel): which
// instantiation a problem gets and, in the streaming form, how a wave's K chunk is cut into bursts.  Plain C++ (no HIP): the launcher and the kernel include it, and so
// does the stand-alone checker csrc/skinny_select_check.cpp, which walks it under the host sanitizers.
#pragma once

// A wave's chunk of K / NW reduction elements is nsteps = K / NW / 16 steps of 16 k.  The weight (B) loads of a whole burst are
// issued before the burst's first MFMA; a chunk is walked as `full` bursts of BS steps, then at most one of 12, then bursts of 4,
// then single steps - every burst straight-line code with compile-time register indices.
struct SkinnyBursts {
  int full, mid, quad, single;
};
constexpr SkinnyBursts rmcl_skinny_bursts(int nsteps, int BS) {
  SkinnyBursts b{nsteps / BS, 0, 0, 0};
  int rem = nsteps - b.full * BS;
  if (BS > 12 && rem >= 12) { b.mid = 1; rem -= 12; }
  b.quad = rem / 4;
  b.single = rem - 4 * b.quad;
  return b;
}
constexpr int rmcl_skinny_burst_steps(const SkinnyBursts& b, int BS) { return b.full * BS + b.mid * 12 + b.quad * 4 + b.single; }

// Steps per full burst.  [N][K] weights (b_kc): one 16-byte load per lane and step, 24 steps = 96 VGPRs of weights in flight (the
// longest chunk of the step, K = 3072 over 8 waves, in one burst); 4 waves never have more than 31 steps and take 12.  [K][N]
// weights: four 4-byte loads per step, and the 6-bit vmcnt counts 63 loads at most - 12 steps are 48 loads, plus the A ring's 12.
constexpr int rmcl_skinny_burst_len(bool b_kc, int nw) { return (b_kc && nw == 8) ? 24 : 12; }
// Steps of A loads in flight ahead of a step's MFMAs (the k-split kernel's PD - 1 = 3; the load of step i + ring is issued before the
// MFMAs of step i, so ring + 1 steps are out at the first wait).  [K][N] weights with 4 row tiles: 2, so that the 48 weight loads of a
// burst and 3 x 4 A loads stay within what vmcnt counts.
constexpr int rmcl_skinny_a_ring(bool b_kc, int rt) { return (!b_kc && rt == 4) ? 2 : 3; }
constexpr int rmcl_skinny_loads_in_flight(bool b_kc, int rt, int bs) { return (b_kc ? 1 : 4) * bs + (rmcl_skinny_a_ring(b_kc, rt) + 1) * rt; }

// Waves per workgroup = how many ways K is split.  Part of the ARITHMETIC (it fixes the summation order), so the k-split kernel and the
// streaming kernel, which promise each other's bits, both take it from here.  8 waves where the reduction is long
// (round 4: 8 waves from K = 512 on measured -0.05 ms per step over six alternating runs, but the different fp32 summation order moved the
// 4-sample BatchNorm golden of the Barlow-Twins step from 0.9 % to 1.03 % on one gradient norm - bound 1 % - so the threshold stays)
constexpr int rmcl_skinny_waves(int K) { return (K % 128 == 0 && K >= 2048) ? 8 : 4; }

// The k-split kernel's instantiation for a problem: 32-column tiles on 4 waves for very wide outputs (they halve the re-reads of the A
// panel: Barlow-Twins head, N = 8192), else 16-column tiles on rmcl_skinny_waves(K).  Not ok: the row-split kernel takes the problem.
struct SkinnyKsplitPlan {
  bool ok;
  int nt, nw;           // columns per workgroup, waves per workgroup (K split)
  int grid_x, grid_y;
};
constexpr SkinnyKsplitPlan rmcl_skinny_ksplit_plan(int M, int N, int K) {
  if (K % 64 != 0 || K < 128) return SkinnyKsplitPlan{false, 0, 0, 0, 0};
  const int nt = N >= 4096 ? 32 : 16;
  return SkinnyKsplitPlan{true, nt, N >= 4096 ? 4 : rmcl_skinny_waves(K), (N + nt - 1) / nt, (M + 63) / 64};
}

struct SkinnyPlan {
  bool ok;              // the streaming form takes the shape
  int nw, rt, bs;       // waves per workgroup (K split), 16-row tiles per workgroup, steps per full burst
  int grid_x, grid_y;
  int nsteps;           // 16-k steps of one wave
  SkinnyBursts bursts;
};

// M x N x K problem, `share` chains sharing the chip (rmcl_tune_set key 10).  NW is rmcl_skinny_waves(K), as in the k-split kernel (the K split
// is part of the arithmetic).  RT: no workgroup may cover a row tile that begins beyond M, so RT divides the number of live row tiles;
// among those, the largest RT (a weight fragment then feeds RT MFMAs, and the weights are pulled through L2 once per RT row tiles)
// that still leaves about 192 workgroups for the chain's part of the chip - launches with few column tiles otherwise sit on 48 CUs,
// each pulling the whole A panel.
inline SkinnyPlan rmcl_skinny_plan(int M, int N, int K, bool b_kc, int share) {
  SkinnyPlan p{};
  if (M < 1 || N < 1 || N >= 4096 || K < 128 || K % 64 != 0) return p;
  p.ok = true;
  p.nw = rmcl_skinny_waves(K);
  p.bs = rmcl_skinny_burst_len(b_kc, p.nw);
  p.nsteps = K / p.nw / 16;
  p.bursts = rmcl_skinny_bursts(p.nsteps, p.bs);
  const int tiles = (M + 15) / 16, ctiles = (N + 15) / 16;
  const int want = 192 / (share < 1 ? 1 : share);
  p.rt = 1;
  for (int rt = 4; rt > 1; rt >>= 1)
    if (tiles % rt == 0 && (long)ctiles * (tiles / rt) >= want) { p.rt = rt; break; }
  p.grid_x = ctiles;
  p.grid_y = tiles / p.rt;
  return p;
}
