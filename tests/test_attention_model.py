"""CPU: the rounding model of tests/test_attention_kernels_gpu.py against the float64 reference, on its own.

The GPU tests allow a kernel 3 x the model's worst-row error on the same case.  These caps keep that from becoming a loose absolute
bound: the model alone (fp32 math, P and dS rounded to bf16 before the second GEMM, bf16 outputs) must stay within
                      recompute form      delta-from-O form
  unit-normal         5e-3                5e-3
  stress families     8e-3                2.5e-2
worst row over out, dQ, dK, dV at N = 65 and N = 185, B = 2, H = 12, with the text-pad + image-pad mask.  Measured, N = 65 / N = 185 (the
same figures as DESIGN "Attention kernel parity"):
                      recompute form      delta-from-O form
  unit-normal         2.9e-3 / 3.5e-3     3.8e-3 / 3.5e-3
  q x 4               3.2e-3 / 3.5e-3     1.26e-2 / 8.7e-3
  V + 3               2.8e-3 / 3.4e-3     1.16e-2 / 1.20e-2
  K + 2               5.8e-3 / 7.1e-3     1.14e-2 / 1.13e-2
- the first record of what taking delta from the bf16-rounded forward output costs; the worst block is dQ or dK wherever the two forms differ."""
import pytest

from tests.test_attention_kernels_gpu import BLOCKS, FAMILIES, Case, model_figures

CAPS = {("normal", "two_kernel"): 5e-3, ("normal", "one_kernel"): 5e-3, ("stress", "two_kernel"): 8e-3, ("stress", "one_kernel"): 2.5e-2}


@pytest.mark.parametrize("kind", ["two_kernel", "one_kernel"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N", [65, 185])
def test_rounding_model_stays_within_its_caps(N, family, kind):
    fig = model_figures(Case(2, N, 12, "text", family), kind)
    worst = max(fig[b][0] for b in BLOCKS)
    print(f"N {N} {family} {kind}: " + "  ".join(f"{b} {fig[b][0]:.3e}" for b in BLOCKS))
    assert worst <= CAPS[("normal" if family == "normal" else "stress", kind)], fig
