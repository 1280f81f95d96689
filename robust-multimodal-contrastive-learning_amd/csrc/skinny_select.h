// Host-side selection of the streaming k-split skinny GEMM (gemm_exact.hip, gemm_skinny_stream_kernel): which instantiation a
// problem gets and how a wave's K chunk is cut into bursts.  Plain C++ (no HIP): the launcher and the kernel include it, and so
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

struct SkinnyPlan {
  bool ok;              // the streaming form takes the shape
  int nw, rt, bs;       // waves per workgroup (K split), 16-row tiles per workgroup, steps per full burst
  int grid_x, grid_y;
  int nsteps;           // 16-k steps of one wave
  SkinnyBursts bursts;
};

// M x N x K problem, `share` chains sharing the chip (rmcl_tune_set key 10).  NW follows the k-split kernel's rule (the K split is
// part of the arithmetic).  RT: no workgroup may cover a row tile that begins beyond M, so RT divides the number of live row tiles;
// among those, the largest RT (a weight fragment then feeds RT MFMAs, and the weights are pulled through L2 once per RT row tiles)
// that still leaves about 192 workgroups for the chain's part of the chip - launches with few column tiles otherwise sit on 48 CUs,
// each pulling the whole A panel.
inline SkinnyPlan rmcl_skinny_plan(int M, int N, int K, bool b_kc, int share) {
  SkinnyPlan p{};
  if (M < 1 || N < 1 || N >= 4096 || K < 128 || K % 64 != 0) return p;
  p.ok = true;
  p.nw = (K % 128 == 0 && K >= 2048) ? 8 : 4;
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
