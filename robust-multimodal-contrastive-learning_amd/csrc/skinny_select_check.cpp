// Stand-alone check of the k-split skinny GEMMs' host-side selection (skinny_select.h): every M = 1 .. 1024 at the (N, K) of the
// contrastive step and of the tests, both weight layouts, 1 .. 8 chains sharing the chip.  Built and run under the host sanitizers by
// tests/test_gemm_skinny_select_cpu.py; needs no GPU.  Exit status 0 = every assertion held.
#include <cstdio>
#include <cstdlib>

#include "skinny_select.h"

#define CHECK(cond)                                                                                                       \
  do {                                                                                                                    \
    if (!(cond)) {                                                                                                        \
      std::fprintf(stderr, "skinny_select_check: %s failed at M=%d N=%d K=%d b_kc=%d share=%d\n", #cond, M, N, K, b_kc, share); \
      return 1;                                                                                                           \
    }                                                                                                                     \
  } while (0)

int main() {
  static const int shapes[][2] = {{768, 768},  {3072, 768}, {768, 3072}, {128, 768},  {256, 768},  {768, 2048},
                                  {16, 128},   {40, 256},   {128, 768},  {768, 6144}, {2048, 512}, {4080, 1984}};
  long checked = 0;
  for (const auto& nk : shapes)
    for (int b_kc = 0; b_kc < 2; ++b_kc)
      for (int share = 1; share <= 8; ++share)
        for (int M = 1; M <= 1024; ++M) {
          const int N = nk[0], K = nk[1];
          const SkinnyPlan p = rmcl_skinny_plan(M, N, K, b_kc != 0, share);
          CHECK(p.ok);
          CHECK(p.rt == 1 || p.rt == 2 || p.rt == 4);
          CHECK(p.nw == ((K % 128 == 0 && K >= 2048) ? 8 : 4));                 // the k-split kernel's rule: the K split is arithmetic
          CHECK(rmcl_skinny_waves(K) == ((K % 128 == 0 && K >= 2048) ? 8 : 4));
          // both plans apply here: they name the same K split, or the two forms could not agree bit for bit
          const SkinnyKsplitPlan kp = rmcl_skinny_ksplit_plan(M, N, K);
          CHECK(kp.ok && kp.nt == 16 && kp.nw == p.nw);
          CHECK(kp.grid_x == p.grid_x && (long)kp.grid_y * 64 >= M && ((long)kp.grid_y - 1) * 64 < M && K % (16 * kp.nw) == 0);
          CHECK(K % (16 * p.nw) == 0 && p.nsteps * 16 * p.nw == K);
          CHECK(p.grid_x * 16 >= N && (p.grid_x - 1) * 16 < N);
          CHECK(p.grid_y >= 1 && (long)p.grid_y * 16 * p.rt >= M);              // every row is covered
          CHECK(((long)p.grid_y * p.rt - 1) * 16 < M);                          // no selected row tile begins beyond M
          CHECK(rmcl_skinny_burst_steps(p.bursts, p.bs) == p.nsteps);           // the bursts cover K / NW exactly
          CHECK(p.bursts.full >= 0 && p.bursts.mid >= 0 && p.bursts.mid <= 1 && p.bursts.quad >= 0 && p.bursts.single >= 0 && p.bursts.single < 4);
          CHECK(p.bs == rmcl_skinny_burst_len(b_kc != 0, p.nw));
          CHECK(rmcl_skinny_loads_in_flight(b_kc != 0, p.rt, p.bs) <= 63);      // loads of a burst in flight: within the 6-bit vmcnt
          // few column tiles: enough workgroups for the chain's part of the chip whenever the rows allow it
          const int tiles = (M + 15) / 16;
          if ((long)p.grid_x * tiles >= 192 / share) CHECK((long)p.grid_x * p.grid_y >= 192 / share);
          else CHECK(p.rt == 1);
          ++checked;
        }
  // the step's launches: 64 rows alone on the chip, 32 rows per half-batch lane
  {
    int M = 64, N = 768, K = 3072, b_kc = 1, share = 1;
    SkinnyPlan p = rmcl_skinny_plan(M, N, K, true, share);
    CHECK(p.rt == 1 && p.grid_x == 48 && p.grid_y == 4 && p.nw == 8 && p.bursts.full == 1 && p.bursts.quad == 0 && p.bursts.single == 0);
    N = 3072; K = 768;
    p = rmcl_skinny_plan(M, N, K, true, share);
    CHECK(p.rt == 4 && p.grid_x == 192 && p.grid_y == 1 && p.nw == 4 && p.bursts.full == 1);
    M = 32; share = 2;
    p = rmcl_skinny_plan(M, N, K, true, share);
    CHECK(p.rt == 2 && p.grid_y == 1);
    N = 768;
    p = rmcl_skinny_plan(M, N, K, true, share);
    CHECK(p.rt == 1 && p.grid_y == 2);
    // shapes the streaming form leaves to the other kernels
    CHECK(!rmcl_skinny_plan(64, 8192, 2048, true, 1).ok && !rmcl_skinny_plan(64, 768, 64, true, 1).ok && !rmcl_skinny_plan(64, 768, 720, true, 1).ok);
    CHECK(!rmcl_skinny_plan(0, 768, 768, true, 1).ok);
    // the k-split kernel alone: 32-column tiles get 4 waves whatever K says; short or ragged K goes to the row-split kernel
    for (K = 128; K <= 8192; K += 64)
      for (M = 1; M <= 1024; M += 33) {
        N = 8192;
        const SkinnyKsplitPlan kp = rmcl_skinny_ksplit_plan(M, N, K);
        CHECK(kp.ok && kp.nt == 32 && kp.nw == 4 && kp.grid_x == 256 && (long)kp.grid_y * 64 >= M && ((long)kp.grid_y - 1) * 64 < M);
        N = 4095;
        CHECK(rmcl_skinny_ksplit_plan(M, N, K).nt == 16 && rmcl_skinny_ksplit_plan(M, N, K).nw == ((K % 128 == 0 && K >= 2048) ? 8 : 4));
      }
    CHECK(!rmcl_skinny_ksplit_plan(64, 768, 64).ok && !rmcl_skinny_ksplit_plan(64, 768, 720).ok && rmcl_skinny_ksplit_plan(64, 768, 128).ok);
  }
  std::printf("skinny_select_check: %ld plans ok\n", checked);
  return 0;
}
