"""CPU: the Adam and SGD rules (optim_type "adam" / "sgd", include/rmcl.h rmcl_optim_step_f32) without a GPU.

  * set_schedule refuses an optim_type the reference does not have with a ValueError, before it touches the model;
  * the float64 statement of the two rules that the GPU tests use as their reference (tests/optim_rules_ref.py) IS torch.optim.Adam /
    torch.optim.SGD(momentum=0.9) in float64: four parameter groups (decay / no decay x base / lr_mult), five steps, weight decay on
    and off, 1e-12 relative per tensor (float64 rounding of two orders of the same sums is ~1e-16 per step);
  * csrc/optim.hip compiled for gfx950: the four instantiations of the new kernel use no scratch memory (tests/test_isa_budget_cpu.py's
    way of reading the compiler's own metadata)."""
import math
import os
import re
import shutil
import subprocess
import tempfile
import types

import pytest
import torch

import rmcl_pkg  # noqa: F401
from tests import optim_rules_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robust-multimodal-contrastive-learning_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-x", "hip", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include")]


def test_set_schedule_refuses_an_unknown_optim_type():
    from rmcl_amd.vilt.modules import vilt_utils
    assert set(vilt_utils.OPTIMIZERS) == {"adamw", "adam", "sgd"}
    module = types.SimpleNamespace(hparams=types.SimpleNamespace(config={"optim_type": "lamb"}))      # no engine: the check comes first
    with pytest.raises(ValueError) as err:
        vilt_utils.set_schedule(module)
    assert "lamb" in str(err.value)


@pytest.mark.parametrize("wd", [0.01, 0.0])
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_the_fp64_rules_are_torchs_optimizers(rule, wd):
    lr, lr_mult, steps = 1e-3, 10.0, 5
    gen = torch.Generator().manual_seed(11)
    sizes = [400, 100, 300, 224]                                                 # 1024 elements in the reference's four groups
    hyper = [(wd, lr), (0.0, lr), (wd, lr * lr_mult), (0.0, lr * lr_mult)]
    p0 = [torch.randn(n, generator=gen, dtype=torch.float64) for n in sizes]
    grads = [[torch.randn(n, generator=gen, dtype=torch.float64) * 0.1 for n in sizes] for _ in range(steps)]
    params = [p.clone().requires_grad_(True) for p in p0]
    groups = [{"params": [p], "weight_decay": w, "lr": l} for p, (w, l) in zip(params, hyper)]
    opt = torch.optim.Adam(groups, lr=lr) if rule == "adam" else torch.optim.SGD(groups, lr=lr, momentum=0.9)
    mine = [p.clone() for p in p0]
    m = [torch.zeros_like(p) for p in p0]
    v = [torch.zeros_like(p) for p in p0]
    b1, b2 = R.ADAM_BETAS if rule == "adam" else (R.SGD_MOMENTUM, 0.0)
    for t in range(1, steps + 1):
        for p, g in zip(params, grads[t - 1]):
            p.grad = g.clone()
        opt.step()
        for k, (w, l) in enumerate(hyper):
            R.rule_step(R.ADAM if rule == "adam" else R.SGD, mine[k], grads[t - 1][k], m[k], v[k], l, w, b1, b2, R.ADAM_EPS,
                        1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t))
        for k, p in enumerate(params):
            ref = p.detach()
            assert float((mine[k] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (rule, wd, t, k)
            st = opt.state[p]
            ref_m = st["exp_avg"] if rule == "adam" else st["momentum_buffer"]
            assert float((m[k] - ref_m).abs().max()) <= 1e-12 * float(ref_m.abs().max()), (rule, wd, t, k)
            if rule == "adam":
                assert float((v[k] - st["exp_avg_sq"]).abs().max()) <= 1e-12 * float(st["exp_avg_sq"].abs().max()), (rule, wd, t, k)
    assert all(not torch.equal(a, b) for a, b in zip(mine, p0))
    if wd:                                                                       # (the decayed and the undecayed run do differ)
        assert float(m[0].abs().max()) > 0


def test_the_eps_placements_differ_where_eps_dominates():
    """The input of the GPU test's eps case: |g| ~ 1e-9 against eps = 1e-8, lr = 1e-3.  At step 1 torch's update is
    lr |g| / (|g| + eps) ~ 9.1e-5, HF's lr sqrt(1 - b2) |g| / (sqrt(1 - b2) |g| + eps) ~ 3.2e-6: the gap, ~8.8e-5, is more than ten
    times 4 * 2^-23 * max|p| = 4.8e-7, the floor of the GPU tests' tolerance at p ~ 1."""
    g = torch.full((64,), 1e-9, dtype=torch.float64)
    p, m, v = torch.ones(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    b1, b2 = R.ADAM_BETAS
    bc1, bc2s = 1.0 - b1, math.sqrt(1.0 - b2)
    hf = R.hf_adamw_p64(p, g, m, v, 1e-3, b1, b2, R.ADAM_EPS, bc1, bc2s)
    R.rule_step(R.ADAM, p, g, m, v, 1e-3, 0.0, b1, b2, R.ADAM_EPS, bc1, bc2s)
    gap = float((p - hf).abs().min())
    assert 8e-5 < gap < 9e-5 and gap > 10 * 4 * 2.0 ** -23 * float(p.abs().max())


def test_the_new_kernels_use_no_scratch():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as tmp:
        dst = os.path.join(tmp, "optim.s")
        r = subprocess.run(["hipcc", *FLAGS, os.path.join(CSRC, "optim.hip"), "-o", dst], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(dst).read()
    sizes = {name: int(size) for name, size in re.findall(r"\.set (_Z\S+)\.private_seg_size, (\d+)", text) if "optim_rule_kernel" in name}
    assert len(sizes) == 4, sorted(sizes)                                        # Adam and SGD, plain and guarded
    assert all(s == 0 for s in sizes.values()), sizes
