"""The two update rules of rmcl_optim_step_f32 restated from the comment in include/rmcl.h, on torch CPU tensors.  ``rule_step`` runs in
the dtype of the tensors handed to it: on float64 tensors it is the reference of tests/test_optim_rules_kernels_gpu.py, on float32
tensors the fp32 twin in the kernel's stated order (every product and sum rounded on its own; the kernel may fuse a product into the
sum that follows it, which is what the factor in the tolerance is for).  tests/test_optim_rules_cpu.py holds the float64 form to
torch.optim.Adam / torch.optim.SGD."""
import math

import torch

ADAM, SGD = 1, 2                             # include/rmcl.h RMCL_OPTIM_ADAM, RMCL_OPTIM_SGD
ADAM_BETAS, ADAM_EPS, SGD_MOMENTUM = (0.9, 0.999), 1e-8, 0.9      # the reference's calls (vilt_utils.py:399-402): torch's defaults, momentum 0.9


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def bias_corrections(b1, b2, t):
    """(bc1, bc2s) as the library forms them: double arithmetic on the fp32 betas, rounded to fp32 once."""
    b1, b2 = f32(b1), f32(b2)
    return f32(1.0 - b1 ** t), f32(math.sqrt(1.0 - b2 ** t))


def rule_step(rule, p, g, m, v, slr, wd, b1, b2, eps, bc1, bc2s):
    """One step, in place, on p, m (and v for Adam).  g: the effective gradient (grad_scale and clip_coef already applied); slr, wd:
    per-element tensors or numbers (learning rate times the segment's multiplier, the segment's weight decay).  Hyper-parameters are
    python floats holding the fp32 values the kernel receives."""
    dt = p.dtype
    slr = torch.as_tensor(slr, dtype=dt)
    wd = torch.as_tensor(wd, dtype=dt)
    gj = torch.where(wd > 0, g + wd * p, g)
    one = torch.tensor(1.0, dtype=dt)
    tb1, tb2 = torch.tensor(b1, dtype=dt), torch.tensor(b2, dtype=dt)
    if rule == ADAM:
        m.copy_(m * tb1 + gj * (one - tb1))
        v.copy_(v * tb2 + gj * gj * (one - tb2))
        step = slr / torch.tensor(bc1, dtype=dt)
        p.copy_(p - (step * m) / (v.sqrt() / torch.tensor(bc2s, dtype=dt) + torch.tensor(eps, dtype=dt)))
    else:
        m.copy_(m * tb1 + gj)
        p.copy_(p - slr * m)


def hf_adamw_p64(p, g, m, v, slr, b1, b2, eps, bc1, bc2s):
    """p after one step of the OTHER eps placement (HF AdamW, rmcl_adamw_f32: eps added before the bias correction reaches the
    denominator), float64, no weight decay, from the moments BEFORE the step - what a kernel with the eps in the wrong place computes."""
    m2 = m * b1 + g * (1 - b1)
    v2 = v * b2 + g * g * (1 - b2)
    return p - slr * bc2s / bc1 * m2 / (v2.sqrt() + eps)
