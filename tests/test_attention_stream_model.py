"""CPU: the rounding model of tests/test_attention_kernels_gpu.py at the lengths of the streaming attention kernels.

tests/test_attention_stream_gpu.py allows the kernels 3 x the model's worst-row error on the same case.  The model alone must stay inside
the EXISTING caps of tests/test_attention_model.py at N = 257, 281 and 512 too, so that the bound cannot turn loose at the new lengths:
                      recompute form      delta-from-O form
  unit-normal         5e-3                5e-3
  stress families     8e-3                2.5e-2
Measured over these three lengths (B = 2, H = 12), recompute / delta-from-O form:
  unit-normal, masks text, holes, tail, late   2.8e-3 .. 3.3e-3 / 2.9e-3 .. 4.4e-3
  K + 2                                        6.3e-3 .. 6.9e-3 / <= 1.05e-2
  q x 4, V + 3                                 <= 3.4e-3        / <= 1.55e-2
The streaming backward is the delta-from-O form; the recompute form is held too, as in the existing file."""
import pytest
import torch

from tests.test_attention_kernels_gpu import BLOCKS, Case, attention_autograd, bf, figures, inputs, rounding_model
from tests.test_attention_model import CAPS

CASES = [(N, "text", f) for N in (257, 281, 512) for f in ("normal", "qx4", "v+3", "k+2")] + \
        [(N, m, "normal") for N in (257, 281, 512) for m in ("holes", "tail", "late")]


def case_inputs(case):
    if case.mask != "late":
        return inputs(case)
    qkv, dout, _ = inputs(case._replace(mask="all"))
    m = torch.zeros(case.B, case.N, dtype=torch.int32)
    m[0, max(case.N - 60, 0):] = 1
    m[1:, case.N - 1] = 1
    return qkv, dout, m


@pytest.mark.parametrize("N,mask,family", CASES)
def test_rounding_model_stays_within_the_existing_caps(N, mask, family):
    case = Case(2, N, 12, mask, family)
    qkv, dout, m = case_inputs(case)
    qkv, dout = bf(qkv), bf(dout)
    ref = attention_autograd(qkv, dout, m, 2, N, 12, torch.float64)[0]
    for kind, from_o in (("two_kernel", False), ("one_kernel", True)):
        fig = figures(rounding_model(qkv, dout, m, 2, N, 12, delta_from_O=from_o), ref)
        worst = max(fig[b][0] for b in BLOCKS)
        print(f"N {N} {mask} {family} {kind}: " + "  ".join(f"{b} {fig[b][0]:.3e}" for b in BLOCKS))
        assert worst <= CAPS[("normal" if family == "normal" else "stress", kind)], (kind, fig)
